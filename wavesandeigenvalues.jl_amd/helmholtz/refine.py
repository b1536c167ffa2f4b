"""Uniform mesh refinement on the device (wae_octosplit, include/waehip.h): ``octosplit`` of the reference (src/Meshutils.jl:589-747), every
tetrahedron split into 8 and every boundary triangle into 4, index for index the reference's lists, with the nested P1 prolongation between
the levels.  The levels stay in HBM behind one handle; what is carried from a mesh to its refinement by the labels alone (fields per
simplex, domains, the reference tetrahedron of a flame) is an O(n) gather on the host.

``RefinedMesh.prolongator`` returns a step of that prolongation as a sparse matrix, ``RefinedMesh.prolongators`` the list a family
assembled on a refined level hands to its multigrid set-up (``LinearOperatorFamily.solver_prolongators``, wae_solver_setup_nested).

With ``order="quad"`` the same three entries act on the P2 space of ``assemble_p2`` (one unknown per point, then one per edge, the edges
ascending by (smaller point, larger point)): the prolongation between two levels evaluates the coarse P2 basis at the fine unknowns'
locations, five kinds of row with fixed dyadic weights (``_p2_step``; wae_octosplit_prolong_p2, wae_octosplit_prolongator_p2).
``prolongators(order="quad")`` is the h-hierarchy of a P2 family, ``prolongators(order="quad", p_first=True)`` its p-hierarchy: the
embedding of the P1 space of the same mesh (``assemble.p2_embedding``), then the P1 steps.

Out of scope: meshes with a degree of symmetry (the point classes of a Bloch unit cell do not survive appended points), interior-triangle
lists, and Hermite prolongation."""
from __future__ import annotations

import ctypes as C

import numpy as np
import scipy.sparse as sp

from .. import _lib
from . import probe

_ORDERS = ("lin", "quad")
_FACE_TOL = 1e-10          # barycentric distance from a face of the parent below which a neighbour's child may contain x_ref as well


class RefinedMesh:
    """The levels 0..levels of one ``octosplit`` call; level 0 is the input.  Per level l: ``points[l]`` (n, 3), ``tets[l]`` (ntets, 4),
    ``tris[l]`` (ntris, 3); for l >= 1 also ``parents[l]`` (one (larger, smaller) pair of level-(l-1) points per new point),
    ``tet_labels[l]`` (ntets of l-1, 8) and ``tri_labels[l]`` (ntris of l-1, 4): the positions of every parent's children in the lists of
    level l (entry 0 of the three is None).  Everything is 0-based.  The device handle is freed with the object; without one (handle
    None: the arrays alone) everything but ``prolong`` works."""

    def __init__(self, handle, device, points, tets, tris, parents, tet_labels, tri_labels):
        self._h, self.device, self.levels = handle, int(device), len(points) - 1
        self.points, self.tets, self.tris = list(points), list(tets), list(tris)
        self.parents, self.tet_labels, self.tri_labels = list(parents), list(tet_labels), list(tri_labels)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            _lib.lib().wae_octosplit_free(h)

    def _level(self, l, what="level"):
        l = int(l)
        if l < 0:
            l += self.levels + 1
        if not 0 <= l <= self.levels:
            raise ValueError(f"{what} outside 0..{self.levels}")
        return l

    def _order(self, order):
        if order not in _ORDERS:
            raise ValueError(f"order must be 'lin' or 'quad', got {order!r}")
        return order

    def _edges(self, l):
        """the P2 edges of level l on the host, (nedges, 2) ascending by (smaller point, larger point)"""
        cache = self.__dict__.setdefault("_p2_edges", {})
        if l not in cache:
            cache[l] = host_edges(self.tets[l])
        return cache[l]

    def ndof(self, level=-1, order="lin"):
        """the number of unknowns of a level: its points ("lin"), or its points and edges ("quad": the size of ``assemble_p2``)"""
        l = self._level(level)
        n = len(self.points[l])
        if self._order(order) == "lin":
            return n
        if self._h:
            ne, nd, nz = C.c_int64(0), C.c_int64(0), C.c_int64(0)
            _lib.check(_lib.lib().wae_octosplit_p2_info(self._h, l, C.byref(ne), C.byref(nd), C.byref(nz)))
            return int(nd.value)
        return n + len(self._edges(l))

    def prolong(self, X, from_level=0, to_level=-1, order="lin"):
        """The nested embedding of level ``from_level`` into ``to_level``, level by level on the device.  ``order="lin"``
        (wae_octosplit_prolong): old points keep their value, a new point gets the mean of the two ends of its edge.  ``order="quad"``
        (wae_octosplit_prolong_p2): the P2 function with the coefficients X, in the P2 basis of ``to_level``.  X: (ndof(from),) or
        (ndof(from), ncols), real or complex; the result has the same number of dimensions and is complex exactly if X is."""
        quad = self._order(order) == "quad"
        f, t = self._level(from_level, "from_level"), self._level(to_level, "to_level")
        if f >= t:
            raise ValueError(f"prolongation needs from_level < to_level, got {f} and {t}")
        X = np.asarray(X)
        nf = self.ndof(f, order)
        if X.ndim not in (1, 2) or X.shape[0] != nf or X.size == 0:
            raise ValueError(f"X has shape {X.shape}, level {f} has {nf} {'unknowns' if quad else 'points'}")
        if not (np.issubdtype(X.dtype, np.floating) or np.issubdtype(X.dtype, np.complexfloating) or np.issubdtype(X.dtype, np.integer)):
            raise ValueError(f"X must be real or complex, got {X.dtype}")
        if not self._h:
            raise ValueError("this RefinedMesh holds no device handle")
        real = not np.iscomplexobj(X)
        ncols = 1 if X.ndim == 1 else X.shape[1]
        Xf = np.asfortranarray(X.reshape(X.shape[0], ncols), dtype=np.complex128)
        Y = np.zeros((self.ndof(t, order), ncols), dtype=np.complex128, order="F")
        entry = _lib.lib().wae_octosplit_prolong_p2 if quad else _lib.lib().wae_octosplit_prolong
        _lib.check(entry(self._h, f, t, ncols, _zptr_f(Xf), _zptr_f(Y)))
        Y = Y.real.copy() if real else Y
        return Y[:, 0] if X.ndim == 1 else Y

    def prolongator(self, from_level=0, order="lin"):
        """The step ``from_level`` -> ``from_level + 1`` of the nested embedding as a ``scipy.sparse.csr_matrix`` (unknowns of the finer
        level x unknowns of ``from_level``), columns ascending.  ``order="lin"``: the row of an old point holds 1.0 at its own column,
        the row of a new point 0.5 at its two parents.  ``order="quad"``: the rows of ``_p2_step``.  With a device handle the matrix is
        built by a kernel from the tables in HBM (wae_octosplit_prolongator, wae_octosplit_prolongator_p2); without one the same
        matrix is formed on the host."""
        if isinstance(from_level, bool) or not isinstance(from_level, (int, np.integer)):
            raise ValueError(f"from_level must be an integer, got {from_level!r}")
        quad = self._order(order) == "quad"
        f = self._level(from_level, "from_level")
        if f >= self.levels:
            raise ValueError(f"from_level must be below the last level {self.levels}, got {f}")
        ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
        if quad and self._h:
            ne, nd, nz = C.c_int64(0), C.c_int64(0), C.c_int64(0)
            _lib.check(_lib.lib().wae_octosplit_p2_info(self._h, f, C.byref(ne), C.byref(nd), C.byref(nz)))
            n_old, n_new, nnz = int(nd.value), self.ndof(f + 1, "quad"), int(nz.value)
            ptr, col, val = np.zeros(n_new + 1, dtype=np.int32), np.zeros(nnz, dtype=np.int32), np.zeros(nnz)
            _lib.check(_lib.lib().wae_octosplit_prolongator_p2(self._h, f, ptr.ctypes.data_as(ip), col.ctypes.data_as(ip), val.ctypes.data_as(dp)))
            return sp.csr_matrix((val, col, ptr), shape=(n_new, n_old))
        if quad:
            return _p2_step(len(self.points[f]), self._edges(f), len(self.points[f + 1]), self._edges(f + 1), self.parents[f + 1])
        n_old, n_new = len(self.points[f]), len(self.points[f + 1])
        nnz = 2 * n_new - n_old
        if self._h:
            ptr, col, val = np.zeros(n_new + 1, dtype=np.int32), np.zeros(nnz, dtype=np.int32), np.zeros(nnz)
            _lib.check(_lib.lib().wae_octosplit_prolongator(self._h, f, ptr.ctypes.data_as(ip), col.ctypes.data_as(ip), val.ctypes.data_as(dp)))
        else:
            par = np.sort(np.asarray(self.parents[f + 1], dtype=np.int32).reshape(-1, 2), axis=1)
            ptr = np.concatenate([np.arange(n_old, dtype=np.int32), n_old + 2 * np.arange(n_new - n_old + 1, dtype=np.int32)])
            col = np.concatenate([np.arange(n_old, dtype=np.int32), par.ravel()])
            val = np.concatenate([np.ones(n_old), np.full(2 * (n_new - n_old), 0.5)])
        return sp.csr_matrix((val, col, ptr), shape=(n_new, n_old))

    def prolongators(self, to_level=-1, coarsest=0, order="lin", p_first=False):
        """The prolongators of a family assembled on ``to_level``, finest first, down to level ``coarsest``: what
        ``LinearOperatorFamily.solver_prolongators`` and ``DeviceFamily.setup_solver(prolongators=...)`` take.  ``order="quad"``: of a
        P2 family, the P2 steps (h-coarsening); with ``p_first=True`` the embedding of the P1 space of ``to_level`` into its P2 space
        (p-coarsening), then the P1 steps -- there ``coarsest`` may equal ``to_level``: the embedding alone."""
        quad = self._order(order) == "quad"
        if not isinstance(p_first, (bool, np.bool_)):
            raise ValueError(f"p_first must be True or False, got {p_first!r}")
        if p_first and not quad:
            raise ValueError("p_first is the p-coarsening of a P2 family: it needs order='quad'")
        t, c = self._level(to_level, "to_level"), self._level(coarsest, "coarsest")
        if c > t or (c == t and not p_first):
            raise ValueError(f"prolongators needs coarsest < to_level, got {c} and {t}")
        if p_first:
            from .assemble import p2_embedding, p2_embedding_host
            E = p2_embedding(self.points[t], self.tets[t], device=self.device) if self._h else p2_embedding_host(len(self.points[t]), self._edges(t))
            return [E] + [self.prolongator(l) for l in range(t - 1, c - 1, -1)]
        return [self.prolongator(l, order) for l in range(t - 1, c - 1, -1)]

    # ---- host-side carriers: O(n) gathers through the labels ---------------------------------------------------------------------
    def _carry(self, values, labels, count, to_level, what):
        t = self._level(to_level, "to_level")
        v = np.asarray(values)
        if v.shape[:1] != (count,):
            raise ValueError(f"{what}: {v.shape[0] if v.ndim else 'a scalar'} values for the {count} simplices of level 0")
        for l in range(1, t + 1):
            out = np.empty((labels[l].size,) + v.shape[1:], dtype=v.dtype)
            out[labels[l].ravel()] = np.repeat(v, labels[l].shape[1], axis=0)
            v = out
        return v

    def tet_field(self, c_tet, to_level=-1):
        """a value per tetrahedron of level 0 (e.g. the speed of sound) on the tetrahedra of ``to_level``: children inherit the parent's"""
        return self._carry(c_tet, self.tet_labels, len(self.tets[0]), to_level, "tet_field")

    def tri_field(self, c_tri, to_level=-1):
        """the same for a value per boundary triangle of level 0"""
        return self._carry(c_tri, self.tri_labels, len(self.tris[0]), to_level, "tri_field")

    def _domain(self, idx, labels, count, to_level, what):
        t = self._level(to_level, "to_level")
        d = np.asarray(idx, dtype=np.int64).ravel()
        if d.size and (d.min() < 0 or d.max() >= count):
            raise ValueError(f"{what}: an index outside the {count} simplices of level 0")
        for l in range(1, t + 1):
            d = np.sort(labels[l][d].ravel().astype(np.int64))
        return d.astype(np.int32)

    def tet_domain(self, idx, to_level=-1):
        """the simplices of a 3-D domain of level 0 (indices into tets[0]) on ``to_level``: the sorted list of all their children
        (Meshutils.jl:724-740)"""
        return self._domain(idx, self.tet_labels, len(self.tets[0]), to_level, "tet_domain")

    def tri_domain(self, idx, to_level=-1):
        """the same for a 2-D domain (indices into tris[0])"""
        return self._domain(idx, self.tri_labels, len(self.tris[0]), to_level, "tri_domain")

    def reference_tet(self, parent_ref, x_ref, to_level=-1):
        """The reference tetrahedron of a flame on ``to_level``: the first tetrahedron in list order that contains ``x_ref``
        (find_tetrahedron_containing_point, Meshutils.jl:800-816), given the one of level 0, ``parent_ref``.  Inside the parent that is the
        first of its descendants that contains the point.  Within 1e-10 (barycentric) of a face of the parent a neighbour's child could
        come first in the list: then ``probe.find_tetrahedron`` searches the whole level."""
        t = self._level(to_level, "to_level")
        ref = int(parent_ref)
        if not 0 <= ref < len(self.tets[0]):
            raise ValueError(f"parent_ref outside the {len(self.tets[0])} tetrahedra of level 0")
        x = np.asarray(x_ref, dtype=np.float64)
        if x.shape != (3,):
            raise ValueError(f"a point has 3 coordinates, got shape {x.shape}")
        lam, _ = probe._barycentric(self.points[0][self.tets[0][ref]], x)
        if lam.min() < _FACE_TOL:
            return probe.find_tetrahedron(self.points[t], self.tets[t], x)
        cand = self.tet_domain([ref], t)
        for c in cand:                                                    # ascending: list order
            lam, _ = probe._barycentric(self.points[t][self.tets[t][c]], x)
            if lam.min() >= 0.0:
                return int(c)
        return probe.find_tetrahedron(self.points[t], self.tets[t], x)    # x_ref within a rounding of an inner face


def host_edges(tets):
    """the unique edges of the tetrahedra, (nedges, 2) int32 ascending by (smaller point, larger point): the edge order of the P2 space"""
    tt = np.asarray(tets, dtype=np.int64).reshape(-1, 4)
    pairs = np.concatenate([tt[:, [i, j]] for i in range(4) for j in range(i + 1, 4)])
    n = int(tt.max()) + 1
    keys = np.unique(pairs.min(axis=1) * n + pairs.max(axis=1))
    return np.stack([keys // n, keys % n], axis=1).astype(np.int32)


def _p2_step(n_c, edges_c, n_f, edges_f, parents):
    """The P2 prolongator of one refinement step on the host, the rule wae_octosplit_prolongator_p2 follows: the coarse basis
    (l_i (2 l_i - 1) on the points, 4 l_i l_j on the edges) at the fine unknowns.  n_c / n_f: points of the two levels; edges_c /
    edges_f: their edges ascending by (smaller, larger); parents: the (larger, smaller) coarse pair of every new point.  Rows:
      old point a                                   (a, 1)
      new point, midpoint of the coarse edge AB     (edge AB, 1)
      fine edge (A, AB)                             (A, 3/8) (B, -1/8) (edge AB, 3/4)
      fine edge (AB, AC)                            (B, -1/8) (C, -1/8) (edge AB, 1/2) (edge AC, 1/2) (edge BC, 1/4)
      fine edge (AB, CD)                            the four points -1/8, the six coarse edges among them 1/4
    columns ascending within a row."""
    ec = np.asarray(edges_c, dtype=np.int64).reshape(-1, 2)
    ef = np.asarray(edges_f, dtype=np.int64).reshape(-1, 2)
    par = np.asarray(parents, dtype=np.int64).reshape(-1, 2)
    if len(par) != n_f - n_c:
        raise ValueError(f"{len(par)} parent pairs for {n_f - n_c} new points")
    ckeys = ec[:, 0] * n_c + ec[:, 1]

    def edge_dof(u, v):
        k = np.minimum(u, v) * n_c + np.maximum(u, v)
        e = np.searchsorted(ckeys, k)
        if np.any(e >= len(ckeys)) or np.any(ckeys[np.minimum(e, len(ckeys) - 1)] != k):
            raise ValueError("a pair of points that is no edge of the coarser level")
        return n_c + e

    u, v = ef[:, 0], ef[:, 1]
    if np.any(v < n_c):
        raise ValueError("a fine edge between two points of the coarser level: not a refinement of it")
    half = u < n_c
    pv = par[v - n_c]
    pu = par[np.where(half, 0, u - n_c)]
    if np.any(half & (pv[:, 0] != u) & (pv[:, 1] != u)):
        raise ValueError("a fine edge from an old point to the midpoint of an edge that does not hold it")
    eq = pu[:, :, None] == pv[:, None, :]                        # eq[r, i, j]: end i of u's pair is end j of v's pair
    nshared = eq.sum(axis=(1, 2))
    if np.any(~half & (nshared > 1)):
        raise ValueError("two new points with the same parents")
    face, inner = ~half & (nshared == 1), ~half & (nshared == 0)
    rows, cols, vals = [np.arange(n_f)], [np.concatenate([np.arange(n_c), edge_dof(par[:, 0], par[:, 1])])], [np.ones(n_f)]

    def add(sel, columns, weights):
        r = n_f + np.nonzero(sel)[0]
        for c, w in zip(columns, weights):
            rows.append(r); cols.append(c); vals.append(np.full(len(r), w))

    a, o = u[half], pv[half].sum(axis=1) - u[half]
    add(half, (a, o, edge_dof(a, o)), (0.375, -0.125, 0.75))
    i = np.argmax(eq[face].any(axis=2), axis=1)                  # the shared point A in u's pair, and in v's
    j = np.argmax(eq[face].any(axis=1), axis=1)
    k = np.arange(int(face.sum()))
    A, B, Cc = pu[face][k, i], pu[face][k, 1 - i], pv[face][k, 1 - j]
    add(face, (B, Cc, edge_dof(A, B), edge_dof(A, Cc), edge_dof(B, Cc)), (-0.125, -0.125, 0.5, 0.5, 0.25))
    q = np.concatenate([pu[inner], pv[inner]], axis=1)
    add(inner, [q[:, m] for m in range(4)] + [edge_dof(q[:, m], q[:, l]) for m in range(4) for l in range(m + 1, 4)], [-0.125] * 4 + [0.25] * 6)
    rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    order = np.lexsort((cols, rows))
    nd_f, nd_c = n_f + len(ef), n_c + len(ec)
    ptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=nd_f))])
    if ptr[-1] > 2 ** 31 - 1:
        raise ValueError("the prolongator's entries do not fit a 32-bit index")
    return sp.csr_matrix((vals[order], cols[order].astype(np.int32), ptr.astype(np.int32)), shape=(nd_f, nd_c))


def _zptr_f(a):
    """pointer to the interleaved (re, im) doubles of a column-major complex128 array"""
    assert a.dtype == np.complex128 and a.flags.f_contiguous
    return a.ctypes.data_as(C.POINTER(C.c_double))


def octosplit(points, tets, tris=None, levels=1, device=0):
    """``levels`` uniform refinements of the mesh points (npoints, 3), tets (ntets, 4), tris (ntris, 3) or None, 0-based, on the device
    (wae_octosplit).  Returns a ``RefinedMesh``.  The library raises ``WaeError`` for an index outside the points, a triangle edge that is
    no tetrahedron's edge, a simplex listed twice, or a level beyond 32-bit indices."""
    pts = np.asarray(points, dtype=np.float64)
    tt = np.asarray(tets)
    tr = None if tris is None else np.asarray(tris)
    if pts.ndim != 2 or pts.shape[1] != 3 or pts.shape[0] == 0:
        raise ValueError(f"points must have shape (npoints, 3) with npoints > 0, got {pts.shape}")
    if tt.ndim != 2 or tt.shape[1] != 4 or tt.shape[0] == 0 or not np.issubdtype(tt.dtype, np.integer):
        raise ValueError(f"tets must be an integer array of shape (ntets, 4) with ntets > 0, got {tt.dtype} {tt.shape}")
    if tr is not None and tr.size == 0:
        tr = None
    if tr is not None and (tr.ndim != 2 or tr.shape[1] != 3 or not np.issubdtype(tr.dtype, np.integer)):
        raise ValueError(f"tris must be an integer array of shape (ntris, 3), got {tr.dtype} {tr.shape}")
    for a in (tt, tr):
        if a is not None and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
            raise ValueError("a point index does not fit 32 bits")
    if isinstance(levels, bool) or not isinstance(levels, (int, np.integer)) or levels < 1:
        raise ValueError(f"levels must be an integer >= 1, got {levels!r}")
    pts = np.ascontiguousarray(pts)
    tt = np.ascontiguousarray(tt, dtype=np.int32)
    tr = None if tr is None else np.ascontiguousarray(tr, dtype=np.int32)
    L = _lib.lib()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    h = C.c_void_p()
    _lib.check(L.wae_octosplit(int(device), pts.shape[0], pts.ctypes.data_as(dp), tt.shape[0], tt.ctypes.data_as(ip), 0 if tr is None else tr.shape[0],
                               None if tr is None else tr.ctypes.data_as(ip), int(levels), C.byref(h)))
    return _download(L, h, int(levels), device)


def _download(L, h, levels, device):
    """copy every level of the handle out into a RefinedMesh, which owns the handle from here on"""
    R = RefinedMesh(h, device, [], [], [], [None], [None], [None])
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    for l in range(levels + 1):
        n, nt, ns = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        _lib.check(L.wae_octosplit_info(h, l, C.byref(n), C.byref(nt), C.byref(ns)))
        pts = np.zeros((n.value, 3))
        tt = np.zeros((nt.value, 4), dtype=np.int32)
        tr = np.zeros((ns.value, 3), dtype=np.int32)
        par = tl = sl = None
        if l:
            par = np.zeros((n.value - len(R.points[-1]), 2), dtype=np.int32)
            tl = np.zeros((len(R.tets[-1]), 8), dtype=np.int32)
            sl = np.zeros((len(R.tris[-1]), 4), dtype=np.int32)
        _lib.check(L.wae_octosplit_get(h, l, pts.ctypes.data_as(dp), tt.ctypes.data_as(ip), tr.ctypes.data_as(ip),
                                       None if par is None else par.ctypes.data_as(ip), None if tl is None else tl.ctypes.data_as(ip),
                                       None if sl is None else sl.ctypes.data_as(ip)))
        R.points.append(pts); R.tets.append(tt); R.tris.append(tr)
        if l:
            R.parents.append(par); R.tet_labels.append(tl); R.tri_labels.append(sl)
    R.levels = levels
    return R
