"""Point location in a tetrahedral mesh and sampling of modes at the located points, on the device (wae_locator_*, include/waehip.h):
``find_tetrahedron_containing_point`` (src/Meshutils.jl:800-815) and ``get_p`` / ``get_n_grad_p`` (src/FEM/helmholtz_getters.jl:7-45) of the
reference for many points at once -- microphone arrays, lines, cut planes, the points of another mesh.  ``helmholtz/probe.py`` stays the
host form for a handful of probes; the rows are the same.

A ``Locator`` keeps the mesh and a uniform cell grid over it in HBM.  ``find`` returns, per point, the lowest tetrahedron index whose four
barycentric coordinates are all >= -tol (-1: none); ``weights`` the rows (idx, val) of the point functionals, ``sample`` applies them to
the columns of V in one gather kernel, ``observers`` hands them to ``nlevp.forced_response``, ``interpolation`` returns them as a CSR
matrix in the format of ``RefinedMesh.prolongator`` (the transfer onto a mesh that is no refinement of this one).

Out of scope: Hermite elements, nearest-tetrahedron answers for points outside the mesh, curved geometry, Bloch-expanded fields."""
from __future__ import annotations

import ctypes as C

import numpy as np
import scipy.sparse as sp

from .. import _lib

TOL_MAX = 1e-6
_ORDERS = {"lin": 1, "quad": 2}
_KINDS = {"p": 0, "n_grad_p": 1}
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)


def _queries(X):
    X = np.asarray(X)
    if X.ndim != 2 or X.shape[1] != 3 or not (np.issubdtype(X.dtype, np.floating) or np.issubdtype(X.dtype, np.integer)):
        raise ValueError(f"X must be a real array of shape (nq, 3), got {X.dtype} {X.shape}")
    return np.ascontiguousarray(X, dtype=np.float64)


class Locator:
    """``Locator(points, tets, device=0, cell_target=0)``: points (npoints, 3), tets (ntets, 4) 0-based; ``cell_target`` tetrahedra per
    cell of the grid (0: the default, about 8).  ``dims`` (3,), ``nrefs`` (the (cell, tetrahedron) pairs) and ``max_per_cell`` describe
    the grid that was built.  The device handle is freed by ``close()`` or with the object."""

    def __init__(self, points, tets, device=0, cell_target=0):
        self._h = None
        pts = np.asarray(points)
        tt = np.asarray(tets)
        if pts.ndim != 2 or pts.shape[1] != 3 or pts.shape[0] == 0 or not (np.issubdtype(pts.dtype, np.floating) or np.issubdtype(pts.dtype, np.integer)):
            raise ValueError(f"points must be a real array of shape (npoints, 3) with npoints > 0, got {pts.dtype} {pts.shape}")
        if tt.ndim != 2 or tt.shape[1] != 4 or tt.shape[0] == 0 or not np.issubdtype(tt.dtype, np.integer):
            raise ValueError(f"tets must be an integer array of shape (ntets, 4) with ntets > 0, got {tt.dtype} {tt.shape}")
        if tt.min() < -2 ** 31 or tt.max() >= 2 ** 31:
            raise ValueError("a point index does not fit 32 bits")
        if isinstance(cell_target, bool) or not isinstance(cell_target, (int, np.integer)) or cell_target < 0:
            raise ValueError(f"cell_target must be an integer >= 0, got {cell_target!r}")
        self.points = np.ascontiguousarray(pts, dtype=np.float64)
        self.tets = np.ascontiguousarray(tt, dtype=np.int32)
        self.device = int(device)
        self._tets10 = None
        h = C.c_void_p()
        L = _lib.lib()
        _lib.check(L.wae_locator_create(self.device, len(self.points), self.points.ctypes.data_as(_dp), len(self.tets), self.tets.ctypes.data_as(_ip),
                                        int(cell_target), C.byref(h)))
        self._h = h
        n, nt, nr, mx = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
        dims = (C.c_int64 * 3)()
        _lib.check(L.wae_locator_info(h, C.byref(n), C.byref(nt), dims, C.byref(nr), C.byref(mx)))
        self.dims, self.nrefs, self.max_per_cell = (int(dims[0]), int(dims[1]), int(dims[2])), int(nr.value), int(mx.value)

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None and getattr(_lib, "lib", None):         # (at interpreter exit the module may be gone already)
            _lib.lib().wae_locator_free(h)

    __del__ = close

    def _handle(self):
        if not self._h:
            raise ValueError("this Locator is closed")
        return self._h

    # ---- argument checks: all of them before the library is touched ---------------------------------------------------------------
    @staticmethod
    def _row_args(X, order, kind, n, tet, outside):
        X = _queries(X)
        if order not in _ORDERS:
            raise ValueError(f"order must be 'lin' or 'quad', got {order!r}")
        if kind not in _KINDS:
            raise ValueError(f"kind must be 'p' or 'n_grad_p', got {kind!r}")
        if outside not in ("raise", "nan"):
            raise ValueError(f"outside must be 'raise' or 'nan', got {outside!r}")
        if kind == "p" and n is not None:
            raise ValueError("n is the direction of kind='n_grad_p': kind='p' takes none")
        if kind == "n_grad_p":
            if n is None:
                raise ValueError("kind='n_grad_p' needs the directions n")
            n = np.asarray(n, dtype=np.float64)
            if n.shape == (3,):
                n = np.broadcast_to(n, X.shape)
            if n.shape != X.shape:
                raise ValueError(f"n must have shape (3,) or {X.shape}, got {n.shape}")
            n = np.ascontiguousarray(n)
        if tet is not None:
            tet = np.asarray(tet)
            if tet.shape != (len(X),) or not np.issubdtype(tet.dtype, np.integer):
                raise ValueError(f"tet must be an integer array of shape ({len(X)},), got {tet.dtype} {tet.shape}")
            tet = np.ascontiguousarray(tet, dtype=np.int32)
        return X, n, tet

    def _set_p2(self, tets10):
        """the P2 unknowns of the tetrahedra on the handle: the caller's, or those of ``p2_connectivity``"""
        if tets10 is None:
            if self._tets10 is not None:
                return
            from .assemble import p2_connectivity
            tets10 = p2_connectivity(self.points, self.tets, device=self.device)[1]
        t10 = np.asarray(tets10)
        if t10.shape != (len(self.tets), 10) or not np.issubdtype(t10.dtype, np.integer):
            raise ValueError(f"tets10 must be an integer array of shape ({len(self.tets)}, 10), got {t10.dtype} {t10.shape}")
        t10 = np.ascontiguousarray(t10, dtype=np.int32)
        if self._tets10 is not None and np.array_equal(t10, self._tets10):
            return
        ndof = int(t10.max()) + 1
        _lib.check(_lib.lib().wae_locator_set_p2(self._handle(), ndof, t10.ctypes.data_as(_ip)))
        self._tets10, self.ndof_p2 = t10, ndof

    def _located(self, X, tet, outside, tol):
        if tet is None:
            tet = self.find(X, tol=tol)
        if outside == "raise" and len(tet) and tet.min() < 0:
            q = int(np.argmax(tet < 0))
            raise ValueError(f"point {q}, {X[q].tolist()}, lies in no tetrahedron of the mesh")
        return tet

    # ---- queries ------------------------------------------------------------------------------------------------------------------
    def find(self, X, tol=0.0, barycentric=False):
        """The tetrahedron of every row of X (nq, 3): an int32 array (nq,), the lowest index whose barycentric coordinates of the point are
        all >= -tol, -1 where there is none; 0 <= tol <= 1e-6.  ``barycentric=True``: also the (nq, 4) coordinates that decided (NaN for -1)."""
        X = _queries(X)
        if isinstance(tol, bool) or not isinstance(tol, (int, float, np.integer, np.floating)) or not 0.0 <= tol <= TOL_MAX:
            raise ValueError(f"tol must lie in [0, {TOL_MAX}], got {tol!r}")
        h = self._handle()
        tet = np.full(len(X), -1, dtype=np.int32)
        lam = np.full((len(X), 4), np.nan) if barycentric else None
        _lib.check(_lib.lib().wae_locator_find(h, len(X), X.ctypes.data_as(_dp), float(tol), tet.ctypes.data_as(_ip),
                                               None if lam is None else lam.ctypes.data_as(_dp)))
        return (tet, lam) if barycentric else tet

    def weights(self, X, order="lin", kind="p", n=None, tet=None, tets10=None, outside="raise", tol=0.0):
        """The rows of ``probe.probe_p`` (kind "p") or ``probe.probe_n_grad_p`` (kind "n_grad_p", n: one direction (3,) or one per point) at
        every row of X: (idx, val) of shape (nq, 4) for order "lin", (nq, 10) for "quad" (``tets10``: the second result of
        ``p2_connectivity`` if the caller has it).  ``tet``: the tetrahedra of the points if known, else ``find(X, tol)``.  A point in no
        tetrahedron: ValueError naming the first (``outside="raise"``), or a row of idx 0, val 0 (``outside="nan"``)."""
        X, n, tet = self._row_args(X, order, kind, n, tet, outside)
        if order == "quad":
            self._set_p2(tets10)
        tet = self._located(X, tet, outside, tol)
        nw = 4 if order == "lin" else 10
        idx, val = np.zeros((len(X), nw), dtype=np.int32), np.zeros((len(X), nw))
        _lib.check(_lib.lib().wae_locator_weights(self._handle(), _ORDERS[order], _KINDS[kind], len(X), X.ctypes.data_as(_dp), tet.ctypes.data_as(_ip),
                                                  None if n is None else n.ctypes.data_as(_dp), idx.ctypes.data_as(_ip), val.ctypes.data_as(_dp)))
        return idx, val

    def sample(self, V, X, order="lin", kind="p", n=None, tet=None, tets10=None, outside="raise", tol=0.0):
        """p (or n . grad p) of every column of V at every row of X: a complex array (nq, ncols), (nq,) for a vector V.  V has one row per
        unknown: the points (order "lin") or the points and edges of ``assemble_p2`` ("quad").  ``outside="nan"``: NaN rows for the points
        in no tetrahedron."""
        X, n, tet = self._row_args(X, order, kind, n, tet, outside)
        V = np.asarray(V)
        if V.ndim not in (1, 2) or V.size == 0 or not (np.issubdtype(V.dtype, np.floating) or np.issubdtype(V.dtype, np.complexfloating)
                                                      or np.issubdtype(V.dtype, np.integer)):
            raise ValueError(f"V must be a real or complex vector or matrix, got {V.dtype} {V.shape}")
        if order == "lin" and V.shape[0] != len(self.points):
            raise ValueError(f"V has {V.shape[0]} rows, the mesh has {len(self.points)} points")
        if order == "quad":
            self._set_p2(tets10)
            if V.shape[0] != self.ndof_p2:
                raise ValueError(f"V has {V.shape[0]} rows, the P2 space has {self.ndof_p2} unknowns")
        tet = self._located(X, tet, outside, tol)
        ncols = 1 if V.ndim == 1 else V.shape[1]
        Vf = np.asfortranarray(V.reshape(V.shape[0], ncols), dtype=np.complex128)
        out = np.zeros((len(X), ncols), dtype=np.complex128, order="F")
        _lib.check(_lib.lib().wae_locator_sample(self._handle(), _ORDERS[order], _KINDS[kind], len(X), X.ctypes.data_as(_dp), tet.ctypes.data_as(_ip),
                                                 None if n is None else n.ctypes.data_as(_dp), Vf.shape[0], ncols, Vf.ctypes.data_as(_dp),
                                                 out.ctypes.data_as(_dp)))
        return out[:, 0] if V.ndim == 1 else out

    def observers(self, X, order="lin", kind="p", n=None, tet=None, tets10=None, tol=0.0):
        """the list of (idx, val) pairs, one per row of X, that ``nlevp.forced_response(..., observers=...)`` takes: a microphone array
        in one call.  Every point must lie in the mesh."""
        idx, val = self.weights(X, order, kind, n, tet, tets10, "raise", tol)
        return [(idx[q].copy(), val[q].copy()) for q in range(len(idx))]

    def interpolation(self, X, order="lin", tets10=None, tol=1e-10):
        """The interpolation onto the points X as a ``scipy.sparse.csr_matrix`` (nq x unknowns of this mesh) in the format of
        ``RefinedMesh.prolongator``: columns ascending, exact zeros kept out.  Every point must lie in the mesh.  The points of another
        mesh sit on vertices and faces of this one, where rounding leaves a coordinate at -1e-17 as often as at 0: the default ``tol`` is
        1e-10, not the 0 of ``find``."""
        idx, val = self.weights(X, order, "p", None, None, tets10, "raise", tol)
        nq, nw = idx.shape
        ncol = len(self.points) if order == "lin" else self.ndof_p2
        o = np.argsort(idx, axis=1, kind="stable")
        idx, val = np.take_along_axis(idx, o, axis=1), np.take_along_axis(val, o, axis=1)
        keep = val != 0.0
        ptr = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int32)
        return sp.csr_matrix((val[keep], idx[keep].astype(np.int32), ptr), shape=(nq, ncol))
