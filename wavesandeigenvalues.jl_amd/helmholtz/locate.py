"""Point location in a tetrahedral mesh and sampling of modes at the located points, on the device (wae_locator_*, include/waehip.h):
``find_tetrahedron_containing_point`` (src/Meshutils.jl:800-815) and ``get_p`` / ``get_n_grad_p`` (src/FEM/helmholtz_getters.jl:7-45) of the
reference for many points at once -- microphone arrays, lines, cut planes, the points of another mesh.  ``helmholtz/probe.py`` stays the
host form for a handful of probes; the rows are the same.

A ``Locator`` keeps the mesh and a uniform cell grid over it in HBM.  ``find`` returns, per point, the lowest tetrahedron index whose four
barycentric coordinates are all >= -tol (-1: none); ``weights`` the rows (idx, val) of the point functionals, ``sample`` applies them to
the columns of V in one gather kernel, ``observers`` hands them to ``nlevp.forced_response``, ``interpolation`` returns them as a CSR
matrix in the format of ``RefinedMesh.prolongator`` (the transfer onto a mesh that is no refinement of this one).

Orders: "lin" (P1), "quad" (P2, the edges numbered by ``p2_connectivity``) and "herm" (the cubic Hermite space of ``assemble_herm``).  The
Hermite numbering depends on the boundary triangles the family was assembled with, so the locator never numbers faces itself: the first
"herm" call takes ``tets20``, the second result of ``assemble.herm_connectivity``; later calls reuse it, another table replaces it.
``herm_transfer`` carries a Hermite vector onto another mesh (values, gradients and face-centroid values there).

Out of scope: Hermite source vectors, nearest-tetrahedron answers for points outside the mesh, curved geometry, Bloch-expanded fields."""
from __future__ import annotations

import ctypes as C

import numpy as np
import scipy.sparse as sp

from .. import _lib

TOL_MAX = 1e-6
_ORDERS = {"lin": 1, "quad": 2, "herm": 3}
_NW = {"lin": 4, "quad": 10, "herm": 20}
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
            raise ValueError(f"order must be 'lin', 'quad' or 'herm', got {order!r}")
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

    def _herm_table(self, tets20):
        """(tets20, ndof) of an order="herm" call, checked without the library: the caller's table, or the one on the handle"""
        if tets20 is None:
            have = getattr(self, "_tets20", None)
            if have is None:
                raise ValueError("order='herm' needs tets20, the second result of assemble.herm_connectivity(points, tets, tris) with the "
                                 "boundary triangles the family was assembled with")
            return have, self.ndof_herm
        t20 = np.asarray(tets20)
        if t20.shape != (len(self.tets), 20) or not np.issubdtype(t20.dtype, np.integer):
            raise ValueError(f"tets20 must be an integer array of shape ({len(self.tets)}, 20), got {t20.dtype} {t20.shape}")
        if t20.min() < 0 or t20.max() >= 2 ** 31 - 1:
            raise ValueError("tets20 holds an entry that is negative or does not fit 32 bits")
        return np.ascontiguousarray(t20, dtype=np.int32), int(t20.max()) + 1

    def _set_herm(self, t20, ndof):
        """the Hermite unknowns of the tetrahedra on the handle, unless they are there already"""
        have = getattr(self, "_tets20", None)
        if have is not None and (have is t20 or np.array_equal(have, t20)):
            return
        h = self._handle()
        _lib.check(_lib.lib().wae_hermite_locator_set(h, ndof, t20.ctypes.data_as(_ip)))
        self._tets20, self.ndof_herm = t20, ndof

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

    def weights(self, X, order="lin", kind="p", n=None, tet=None, tets10=None, outside="raise", tol=0.0, tets20=None):
        """The rows of ``probe.probe_p`` (kind "p") or ``probe.probe_n_grad_p`` (kind "n_grad_p", n: one direction (3,) or one per point) at
        every row of X: (idx, val) of shape (nq, 4) for order "lin", (nq, 10) for "quad" (``tets10``: the second result of
        ``p2_connectivity`` if the caller has it), (nq, 20) for "herm" (``tets20``: the second result of ``herm_connectivity``, needed by
        the first "herm" call; the rows act on the values, the physical gradients and the face values in the local order of tets20).
        ``tet``: the tetrahedra of the points if known, else ``find(X, tol)``.  A point in no
        tetrahedron: ValueError naming the first (``outside="raise"``), or a row of idx 0, val 0 (``outside="nan"``)."""
        X, n, tet = self._row_args(X, order, kind, n, tet, outside)
        if order == "herm":
            self._set_herm(*self._herm_table(tets20))
        if order == "quad":
            self._set_p2(tets10)
        tet = self._located(X, tet, outside, tol)
        nw = _NW[order]
        idx, val = np.zeros((len(X), nw), dtype=np.int32), np.zeros((len(X), nw))
        _lib.check(_lib.lib().wae_locator_weights(self._handle(), _ORDERS[order], _KINDS[kind], len(X), X.ctypes.data_as(_dp), tet.ctypes.data_as(_ip),
                                                  None if n is None else n.ctypes.data_as(_dp), idx.ctypes.data_as(_ip), val.ctypes.data_as(_dp)))
        return idx, val

    def sample(self, V, X, order="lin", kind="p", n=None, tet=None, tets10=None, outside="raise", tol=0.0, tets20=None):
        """p (or n . grad p) of every column of V at every row of X: a complex array (nq, ncols), (nq,) for a vector V.  V has one row per
        unknown: the points (order "lin"), the points and edges of ``assemble_p2`` ("quad") or the 4 npoints + nfaces unknowns of
        ``assemble_herm`` ("herm", ``tets20`` as in ``weights``).  ``outside="nan"``: NaN rows for the points in no tetrahedron."""
        X, n, tet = self._row_args(X, order, kind, n, tet, outside)
        V = np.asarray(V)
        if V.ndim not in (1, 2) or V.size == 0 or not (np.issubdtype(V.dtype, np.floating) or np.issubdtype(V.dtype, np.complexfloating)
                                                      or np.issubdtype(V.dtype, np.integer)):
            raise ValueError(f"V must be a real or complex vector or matrix, got {V.dtype} {V.shape}")
        if order == "lin" and V.shape[0] != len(self.points):
            raise ValueError(f"V has {V.shape[0]} rows, the mesh has {len(self.points)} points")
        if order == "herm":
            t20, ndof = self._herm_table(tets20)
            if V.shape[0] != ndof:
                raise ValueError(f"V has {V.shape[0]} rows, the Hermite space of tets20 has {ndof} unknowns")
            self._set_herm(t20, ndof)
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

    def observers(self, X, order="lin", kind="p", n=None, tet=None, tets10=None, tol=0.0, tets20=None):
        """the list of (idx, val) pairs, one per row of X, that ``nlevp.forced_response(..., observers=...)`` takes: a microphone array
        in one call.  Every point must lie in the mesh."""
        idx, val = self.weights(X, order, kind, n, tet, tets10, "raise", tol, tets20)
        return [(idx[q].copy(), val[q].copy()) for q in range(len(idx))]

    def interpolation(self, X, order="lin", tets10=None, tol=1e-10, tets20=None):
        """The interpolation onto the points X as a ``scipy.sparse.csr_matrix`` (nq x unknowns of this mesh) in the format of
        ``RefinedMesh.prolongator``: columns ascending, exact zeros kept out.  Every point must lie in the mesh.  The points of another
        mesh sit on vertices and faces of this one, where rounding leaves a coordinate at -1e-17 as often as at 0: the default ``tol`` is
        1e-10, not the 0 of ``find``."""
        idx, val = self.weights(X, order, "p", None, None, tets10, "raise", tol, tets20)
        nq, nw = idx.shape
        ncol = len(self.points) if order == "lin" else (self.ndof_p2 if order == "quad" else self.ndof_herm)
        o = np.argsort(idx, axis=1, kind="stable")
        idx, val = np.take_along_axis(idx, o, axis=1), np.take_along_axis(val, o, axis=1)
        keep = val != 0.0
        ptr = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int32)
        return sp.csr_matrix((val[keep], idx[keep].astype(np.int32), ptr), shape=(nq, ncol))

    def herm_transfer(self, V, points2, tets2, tris2=None, tets20=None, tol=1e-10):
        """The Hermite unknowns on another mesh (points2, tets2, boundary triangles tris2) of the field that the Hermite vector(s) V
        represent on this one: an array (ndof2, ncols), (ndof2,) for a vector V, in the order of ``assemble.herm_dofs`` -- the values, then
        the x, y, z derivatives at ``points2``, then the values at the face centroids of mesh 2, ``tris2`` first, then the faces that
        ``herm_connectivity(points2, tets2, tris2)`` returns.  This is how an eigenpair of a coarse Hermite mesh becomes a start vector
        on a finer one, nested or not.  One ``find`` for the points, one for the centroids, and ``sample`` with the found tetrahedra;
        every point and centroid must lie in this mesh (to ``tol``).  The field is C0 only: where a point of mesh 2 lies on an element
        boundary of this mesh, the gradient is that of the lowest-numbered tetrahedron holding the point."""
        from .assemble import _herm_mesh_checked, herm_connectivity
        p2, t2, s2 = _herm_mesh_checked(points2, tets2, tris2)
        if t2.min() < 0 or t2.max() >= len(p2) or (s2 is not None and s2.size and (s2.min() < 0 or s2.max() >= len(p2))):
            raise ValueError("tets2 or tris2 refers to a point outside points2")
        V = np.asarray(V)
        if V.ndim not in (1, 2) or V.size == 0 or V.dtype.kind not in "fciu":
            raise ValueError(f"V must be a real or complex vector or matrix, got {V.dtype} {V.shape}")
        t20, ndof = self._herm_table(tets20)
        if V.shape[0] != ndof:
            raise ValueError(f"V has {V.shape[0]} rows, the Hermite space of tets20 has {ndof} unknowns")
        self._set_herm(t20, ndof)
        faces2 = herm_connectivity(p2, t2, s2, device=self.device)[0]
        allf = faces2 if s2 is None else np.concatenate([s2, faces2])
        cen = p2[allf].mean(axis=1).reshape(-1, 3)
        tp = self._located(p2, None, "raise", tol)
        blocks = [self.sample(V, p2, "herm", tet=tp)]
        for e in np.eye(3):
            blocks.append(self.sample(V, p2, "herm", "n_grad_p", n=e, tet=tp))
        if len(cen):
            blocks.append(self.sample(V, cen, "herm", tet=self._located(cen, None, "raise", tol)))
        return np.concatenate(blocks, axis=0)
