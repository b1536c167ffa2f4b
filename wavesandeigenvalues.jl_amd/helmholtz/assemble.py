"""P1 mass and stiffness matrices assembled on the device (wae_p1_assemble, include/waehip.h) -- the element loops of
``discretize`` for the "interior" domain (src/Helmholtz.jl:405-441; kernels src/FEM/FEM.jl:704-710,1745-1766)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import scipy.sparse as sp

from .. import _lib


def speed_of_sound_kind(C, npoints, ntets):
    """"tet" or "point": how ``discretize`` reads its speed-of-sound array (Helmholtz.jl:59-74) -- one value per tetrahedron, tested first
    (it wins when the two counts coincide), or one per mesh point, interpolated linearly.  Any other length is a ValueError."""
    n = len(C)
    if n == ntets:
        return "tet"
    if n == npoints:
        return "point"
    raise ValueError(f"speed of sound: {n} values fit neither the {ntets} tetrahedra nor the {npoints} points")


def _nodal(c_point, c_simplex, npoints, what):
    """the checked nodal field of the c_point= keyword (one value per mesh point), or None if the per-simplex form is used"""
    if c_point is None:
        return None
    if c_simplex is not None:
        raise ValueError(f"give the speed of sound per point (c_point) or per simplex ({what}), not both")
    cp = np.ascontiguousarray(c_point, dtype=np.float64)
    if cp.shape != (npoints,):
        raise ValueError(f"c_point has shape {cp.shape}, the mesh has {npoints} points")
    return cp


DP, I32P = C.POINTER(C.c_double), C.POINTER(C.c_int32)


def _ptr(a):
    """the pointer of a float64 or int32 array; None stays NULL"""
    return None if a is None else a.ctypes.data_as(DP if a.dtype == np.float64 else I32P)


def _npoints(points):
    """``points``: the (npoints, 3) array or just npoints"""
    return int(points) if np.ndim(points) == 0 else np.asarray(points).reshape(-1, 3).shape[0]


def _mesh_args(points, tets=None, tris=None):
    pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    tt = None if tets is None else np.ascontiguousarray(tets, dtype=np.int32).reshape(-1, 4)
    tr = None if tris is None else np.ascontiguousarray(tris, dtype=np.int32).reshape(-1, 3)
    return pts, tt, tr


def _counted(a, optional=False):
    """(count, pointer) of an index list; optional: (0, NULL) for None and for an empty list"""
    return (0, None) if optional and (a is None or not len(a)) else (a.shape[0], _ptr(a))


def _prefix(device, pts, simplices, *tris):
    """the arguments every mesh entry starts with: device, npoints, points*, ntets, tets* (P1 boundary and source: the triangles in their
    place), and for the entries that take both lists what _counted made of the triangles: ntris, tris*"""
    return [int(device), pts.shape[0], _ptr(pts), *_counted(simplices), *tris]


def _matrix_c(c_simplex, c_point, npoints, what):
    """(values or None, nodal?) of the speed of sound of a matrix wrapper, c_point checked"""
    cp = _nodal(c_point, c_simplex, npoints, what)
    if cp is not None:
        return cp, True
    return None if c_simplex is None else np.ascontiguousarray(c_simplex, dtype=np.float64), False


def _take(L, h, dtype, pair=False):
    """copy an assembly handle out and free it: one scipy CSR matrix (values = the `mass` array) or, pair, (M, K) sharing one pattern"""
    try:
        n, nnz = C.c_int64(0), C.c_int64(0)
        _lib.check(L.wae_p1_info(h, C.byref(n), C.byref(nnz)))
        rowptr = np.zeros(n.value + 1, dtype=np.int32)
        col = np.zeros(nnz.value, dtype=np.int32)
        m = np.zeros(nnz.value, dtype=np.float64)
        k = np.zeros(nnz.value, dtype=np.float64) if pair else None
        _lib.check(L.wae_p1_get(h, _ptr(rowptr), _ptr(col), _ptr(m), _ptr(k)))
    finally:
        L.wae_p1_free(h)
    shape = (n.value, n.value)
    M = sp.csr_matrix((m.astype(dtype), col, rowptr), shape=shape)
    return (M, sp.csr_matrix((k.astype(dtype), col.copy(), rowptr.copy()), shape=shape)) if pair else M


def _assembled(name, args, dtype=np.complex128, pair=False):
    """the matrix (or pair) of the entry `name` called with args and the handle's address"""
    L = _lib.lib()
    h = C.c_void_p()
    _lib.check(getattr(L, name)(*args, C.byref(h)))
    return _take(L, h, dtype, pair)


def _flame(name, prefix, flame_tets, ref_tet, x_ref, n_ref, nglobal_scaled):
    """(Q, V_flame) of a flame entry; x_ref: None for P1, which takes none"""
    fl = np.ascontiguousarray(flame_tets, dtype=np.int32)
    ref = [np.ascontiguousarray(x, dtype=np.float64) for x in (x_ref, n_ref) if x is not None]
    assert x_ref is None or (ref[0].shape == (3,) and ref[1].shape == (3,))
    L = _lib.lib()
    h = C.c_void_p()
    vol = C.c_double(0.0)
    _lib.check(getattr(L, name)(*prefix, len(fl), _ptr(fl), int(ref_tet), *[_ptr(x) for x in ref], float(nglobal_scaled), C.byref(h), C.byref(vol)))
    return _take(L, h, np.complex128), vol.value


def assemble_p1(points, tets, c_tet=None, device=0, dtype=np.complex128, c_point=None):
    """points (npoints, 3), tets (ntets, 4) 0-based, c_tet (ntets,) speed of sound per tetrahedron (None = 1) or c_point (npoints,)
    speed of sound per mesh point, linear on every tetrahedron (wae_p1_assemble_cpoint; Helmholtz.jl:59-74).
    Returns (M, K) as scipy CSR matrices sharing one pattern; K = -∫ c² ∇φ_a·∇φ_b as in the reference (Helmholtz.jl:120-124)."""
    pts, tt, _ = _mesh_args(points, tets)
    cc, nodal = _matrix_c(c_tet, c_point, pts.shape[0], "c_tet")
    return _assembled("wae_p1_assemble_cpoint" if nodal else "wae_p1_assemble", [*_prefix(device, pts, tt), _ptr(cc)], dtype, pair=True)


def assemble_p1_boundary(points, tris, c_tri=None, device=0, c_point=None):
    """Boundary mass term of an admittance boundary on the device (wae_p1_assemble_boundary):
    C = -i·c·|e1×e2|·(1+δ_ab)/24 per boundary triangle (src/Helmholtz.jl:443-463, src/FEM/FEM.jl:435-441); with c_point (npoints,)
    instead of c_tri, C = -i·|e1×e2|·∫c φ_aφ_b with c linear on every triangle (wae_p1_assemble_boundary_cpoint).  Returns C (complex CSR)."""
    pts, _, tr = _mesh_args(points, tris=tris)
    cc, nodal = _matrix_c(c_tri, c_point, pts.shape[0], "c_tri")
    return -1j * _assembled("wae_p1_assemble_boundary_cpoint" if nodal else "wae_p1_assemble_boundary", [*_prefix(device, pts, tr), _ptr(cc)])


def assemble_p1_flame(points, tets, flame_tets, ref_tet, n_ref, nglobal_scaled, device=0):
    """Flame operator Q = Σ_flame S ⊗ g on the device (wae_p1_assemble_flame; src/Helmholtz.jl:292-344,464-487):
    ``nglobal_scaled`` = (γ-1)/ρ·Q02U0, the library divides by the flame volume it sums itself.  Returns (Q, V_flame)."""
    pts, tt, _ = _mesh_args(points, tets)
    return _flame("wae_p1_assemble_flame", _prefix(device, pts, tt), flame_tets, ref_tet, None, n_ref, nglobal_scaled)


# ---- P2 (second-order) elements: `discretize(...; order=:quad)` ---------------------------------------------------------------
def p2_connectivity(points, tets, tris=None, device=0):
    """Edge DoFs of the P2 space numbered on the device (wae_p2_connectivity; aggregate_elements, src/FEM/FEM.jl:84-116): the unique
    mesh edges sorted by (smaller point, larger point), DoF of edge e = npoints + e.  ``points``: the (npoints, 3) array or just
    npoints.  Returns (edges (nedges, 2), tets10 (ntets, 10), tris6 (ntris, 6)), 0-based, local node order = the points, then the
    edges (1,2), (1,3), (1,4), (2,3), (2,4), (3,4) resp. (1,2), (1,3), (2,3)."""
    npoints = _npoints(points)
    _, tt, tr = _mesh_args(np.zeros((0, 3)), tets, tris)
    L = _lib.lib()
    h = C.c_void_p()
    _lib.check(L.wae_p2_connectivity(int(device), npoints, *_counted(tt), *_counted(tr, True), C.byref(h)))
    try:
        ne, nt, ns = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        _lib.check(L.wae_p2_connectivity_info(h, C.byref(ne), C.byref(nt), C.byref(ns)))
        edges = np.zeros((ne.value, 2), dtype=np.int32)
        t10 = np.zeros((nt.value, 10), dtype=np.int32)
        t6 = np.zeros((ns.value, 6), dtype=np.int32)
        _lib.check(L.wae_p2_connectivity_get(h, _ptr(edges), _ptr(t10), _ptr(t6)))
    finally:
        L.wae_p2_connectivity_free(h)
    return edges, t10, t6


def p2_embedding_host(npoints, edges):
    """the P1 -> P2 embedding of one mesh formed on the host: the row of point a holds (a, 1), the row of edge (a, b), a < b, holds
    (a, 1/2) (b, 1/2) -- a P1 function's values at the P2 nodes, which are its P2 coefficients"""
    e = np.asarray(edges, dtype=np.int32).reshape(-1, 2)
    n, ne = int(npoints), len(e)
    ptr = np.concatenate([np.arange(n, dtype=np.int32), n + 2 * np.arange(ne + 1, dtype=np.int32)])
    col = np.concatenate([np.arange(n, dtype=np.int32), e.ravel()])
    val = np.concatenate([np.ones(n), np.full(2 * ne, 0.5)])
    return sp.csr_matrix((val, col, ptr), shape=(n + ne, n))


def p2_embedding(points, tets, device=0):
    """The embedding of the P1 space of a mesh into its P2 space as a ``csr_matrix`` (npoints + nedges rows, npoints columns,
    npoints + 2 nedges entries, columns ascending), built by a kernel from the edge list of ``wae_p2_connectivity``
    (wae_p2_embedding): the coarse space of p-coarsening, a prolongator ``DeviceFamily.setup_solver(prolongators=...)`` takes.
    ``points``: the (npoints, 3) array or just npoints."""
    npoints = _npoints(points)
    _, tt, _ = _mesh_args(np.zeros((0, 3)), tets)
    L = _lib.lib()
    h = C.c_void_p()
    _lib.check(L.wae_p2_connectivity(int(device), npoints, *_counted(tt), 0, None, C.byref(h)))
    try:
        ne = C.c_int64(0)
        _lib.check(L.wae_p2_connectivity_info(h, C.byref(ne), None, None))
        n, nnz = npoints + ne.value, npoints + 2 * ne.value
        ptr, col, val = np.zeros(n + 1, dtype=np.int32), np.zeros(nnz, dtype=np.int32), np.zeros(nnz)
        _lib.check(L.wae_p2_embedding(h, npoints, _ptr(ptr), _ptr(col), _ptr(val)))
    finally:
        L.wae_p2_connectivity_free(h)
    return sp.csr_matrix((val, col, ptr), shape=(n, npoints))


def assemble_p2(points, tets, c_tet=None, device=0, dtype=np.complex128, c_point=None):
    """P2 mass and stiffness matrices on the device (wae_p2_assemble, wae_p2_assemble_cpoint; src/Helmholtz.jl:120-149,405-441 with
    order=:quad), arguments as ``assemble_p1``.  Returns (M, K) as scipy CSR matrices of size npoints + nedges sharing one pattern."""
    pts, tt, _ = _mesh_args(points, tets)
    cc, nodal = _matrix_c(c_tet, c_point, pts.shape[0], "c_tet")
    assert nodal or cc is None or cc.shape == (tt.shape[0],)
    return _assembled("wae_p2_assemble_cpoint" if nodal else "wae_p2_assemble", [*_prefix(device, pts, tt), _ptr(cc)], dtype, pair=True)


def assemble_p2_boundary(points, tets, tris, c_tri=None, device=0, c_point=None):
    """P2 boundary mass term of an admittance boundary on the device (wae_p2_assemble_boundary; src/Helmholtz.jl:151-170,443-463):
    C = -i·c·|e1×e2|·∫φ_aφ_b on the 6-node triangles; ``tets`` gives the edge numbers; with c_point (npoints,) instead of c_tri, c is
    linear on every triangle and under the integral (wae_p2_assemble_boundary_cpoint).  Returns C (complex CSR, npoints + nedges)."""
    pts, tt, tr = _mesh_args(points, tets, tris)
    cc, nodal = _matrix_c(c_tri, c_point, pts.shape[0], "c_tri")
    assert nodal or cc is None or cc.shape == (tr.shape[0],)
    return -1j * _assembled("wae_p2_assemble_boundary_cpoint" if nodal else "wae_p2_assemble_boundary", [*_prefix(device, pts, tt, *_counted(tr)), _ptr(cc)])


def assemble_p2_flame(points, tets, flame_tets, ref_tet, x_ref, n_ref, nglobal_scaled, device=0):
    """P2 flame operator Q = Σ_flame S ⊗ g on the device (wae_p2_assemble_flame; src/Helmholtz.jl:292-344,464-487): as
    ``assemble_p1_flame``, and ``x_ref``, the reference point inside ``ref_tet`` at which the gradients are taken.  Returns (Q, V_flame)."""
    pts, tt, _ = _mesh_args(points, tets)
    return _flame("wae_p2_assemble_flame", _prefix(device, pts, tt), flame_tets, ref_tet, x_ref, n_ref, nglobal_scaled)


# ---- Hermite (cubic) elements: `discretize(...; order=:herm)` -------------------------------------------------------------------
def _herm_no_nodal_c(c_point):
    if c_point is not None:
        raise NotImplementedError("Hermite elements with a speed of sound per mesh point (c_point) are not implemented: "
                                  "the nodal element matrices of order='herm' are missing; give c per simplex")


def _herm_c(c_simplex, count, what, where):
    """the speed of sound per simplex of a Hermite matrix wrapper (None = 1), checked"""
    cc, _ = _matrix_c(c_simplex, None, 0, what)
    if cc is not None and cc.shape != (count,):
        raise ValueError(f"{what} has shape {cc.shape}, the {where}")
    return cc


def herm_connectivity(points, tets, tris=None, device=0):
    """DoFs of the Hermite space numbered on the device (wae_herm_connectivity; aggregate_elements, src/FEM/FEM.jl:117-160): values at
    the points (DoF p), the x, y, z derivatives there (N + p, 2N + p, 3N + p, N = npoints), one value per face centroid (4N + face).
    The boundary triangle at position t of ``tris`` is face t, every other tetrahedron face follows as ntris + rank, ascending by
    (largest, middle, smallest point).  ``points``: the (npoints, 3) array or just npoints.  Returns (faces (ninner, 3) -- the faces
    that are not in ``tris``, each as (smallest, middle, largest) --, tets20 (ntets, 20), tris13 (ntris, 13), ndof), 0-based; local
    order: the 4 (3) values, the x, the y, the z derivatives, then the faces opposite point 1, 2, 3, 4 (the triangle's own face)."""
    npoints = _npoints(points)
    _, tt, tr = _mesh_args(np.zeros((0, 3)), tets, tris)
    L = _lib.lib()
    h = C.c_void_p()
    _lib.check(L.wae_herm_connectivity(int(device), npoints, *_counted(tt), *_counted(tr, True), C.byref(h)))
    try:
        nf, nt, ns, nd = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
        _lib.check(L.wae_herm_connectivity_info(h, C.byref(nf), C.byref(nt), C.byref(ns), C.byref(nd)))
        faces = np.zeros((nf.value, 3), dtype=np.int32)
        t20 = np.zeros((nt.value, 20), dtype=np.int32)
        t13 = np.zeros((ns.value, 13), dtype=np.int32)
        _lib.check(L.wae_herm_connectivity_get(h, _ptr(faces), _ptr(t20), _ptr(t13)))
    finally:
        L.wae_herm_connectivity_free(h)
    return faces, t20, t13, nd.value


def herm_dof_count(points, tets, tris=None):
    """4 npoints + number of distinct tetrahedron faces = the dimension of the Hermite space (host side; the device numbers the faces
    itself).  ``points``: the array or just npoints; ``tris`` does not change the count (every listed triangle is a tetrahedron face)."""
    npoints = _npoints(points)
    tt = np.asarray(tets, dtype=np.int64).reshape(-1, 4)
    f = np.sort(np.concatenate([tt[:, [b for b in range(4) if b != a]] for a in range(4)]), axis=1)
    return 4 * npoints + len(np.unique(f, axis=0))


def herm_dofs(points, faces, tris, f, grad_f):
    """The DoF vector of a given function in the numbering of ``herm_connectivity`` (host helper: start fields, tests): f(points)
    (npoints,), then grad_f(points) (npoints, 3) as the x, the y, the z derivatives, then f at the centroids of the boundary triangles
    ``tris`` (None: none) and of ``faces``.  f and grad_f take an (n, 3) array of positions."""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    fc = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    tr = np.zeros((0, 3), dtype=np.int64) if tris is None else np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    cen = pts[np.concatenate([tr, fc])].mean(axis=1).reshape(-1, 3)
    val = np.asarray(f(pts))
    g = np.asarray(grad_f(pts)).reshape(len(pts), 3)
    return np.concatenate([val, g[:, 0], g[:, 1], g[:, 2], np.asarray(f(cen)).reshape(-1) if len(cen) else np.zeros(0, dtype=val.dtype)])


def assemble_herm(points, tets, tris=None, c_tet=None, device=0, dtype=np.complex128, c_point=None):
    """Hermite mass and stiffness matrices on the device (wae_herm_assemble; src/Helmholtz.jl:120-149,405-441 with order=:herm).
    ``tris``: the boundary triangles, which take the first face numbers (None: every face numbered by rank).  Returns (M, K) as scipy
    CSR matrices of size ndof sharing one pattern.  ``c_point`` raises NotImplementedError."""
    _herm_no_nodal_c(c_point)
    pts, tt, tr = _mesh_args(points, tets, tris)
    cc = _herm_c(c_tet, tt.shape[0], "c_tet", f"mesh has {tt.shape[0]} tetrahedra")
    return _assembled("wae_herm_assemble", [*_prefix(device, pts, tt, *_counted(tr, True)), _ptr(cc)], dtype, pair=True)


def assemble_herm_boundary(points, tets, tris, c_tri=None, device=0, c_point=None):
    """Hermite boundary mass term of an admittance boundary on the device (wae_herm_assemble_boundary; src/Helmholtz.jl:151-170,443-463):
    C = -i·c·|e1×e2|·∫φ_aφ_b on the 13-DoF triangles, the traces of the tetrahedron functions.  Returns C (complex CSR, ndof)."""
    _herm_no_nodal_c(c_point)
    pts, tt, tr = _mesh_args(points, tets, tris)
    cc = _herm_c(c_tri, tr.shape[0], "c_tri", f"boundary has {tr.shape[0]} triangles")
    return -1j * _assembled("wae_herm_assemble_boundary", [*_prefix(device, pts, tt, *_counted(tr)), _ptr(cc)])


def assemble_herm_flame(points, tets, tris, flame_tets, ref_tet, x_ref, n_ref, nglobal_scaled, device=0):
    """Hermite flame operator Q = Σ_flame S ⊗ g on the device (wae_herm_assemble_flame; src/Helmholtz.jl:292-344,464-487): as
    ``assemble_p2_flame``; ``tris`` (may be None) numbers the faces as in ``assemble_herm``.  Returns (Q, V_flame)."""
    pts, tt, tr = _mesh_args(points, tets, tris)
    return _flame("wae_herm_assemble_flame", _prefix(device, pts, tt, *_counted(tr, True)), flame_tets, ref_tet, x_ref, n_ref, nglobal_scaled)


# ---- speaker source vector: `discretize(...; source=true)` with a :speaker domain ---------------------------------------------
def _source_column(s):
    """the term m = -i·s of the `rhs` family as a complex d x 1 sparse column (sparsevec(I, V, dim) with V ./= 1im, Helmholtz.jl:500,520)"""
    s = np.asarray(s, dtype=np.float64)
    idx = np.nonzero(s)[0]
    return sp.csc_matrix((-1j * s[idx], (idx, np.zeros(len(idx), dtype=np.int64))), shape=(len(s), 1))


def _source_c(points, ntris, c_tri, c_point):
    """(values or None, nodal?) of the speed of sound of a source vector, checked"""
    cc, nodal = _matrix_c(c_tri, c_point, points.shape[0], "c_tri")
    if not nodal and cc is not None and cc.shape != (ntris,):
        raise ValueError(f"c_tri has shape {cc.shape}, the speaker domain has {ntris} triangles")
    return cc, nodal


def assemble_p1_source(points, tris, c_tri=None, device=0, c_point=None):
    """Source vector of a :speaker boundary on the device (wae_p1_assemble_source, wae_p1_assemble_source_cpoint; src/Helmholtz.jl:488-505):
    s_a = |e1×e2|·∫c φ_a over the speaker triangles, c per triangle (``c_tri``, None = 1) or per mesh point (``c_point``, linear on every
    triangle).  Returns the term m = -i·s of the ``rhs`` family as a complex npoints x 1 scipy sparse column."""
    pts, _, tr = _mesh_args(points, tris=tris)
    cc, nodal = _source_c(pts, tr.shape[0], c_tri, c_point)
    L = _lib.lib()
    out = np.zeros(pts.shape[0], dtype=np.float64)
    entry = L.wae_p1_assemble_source_cpoint if nodal else L.wae_p1_assemble_source
    _lib.check(entry(*_prefix(device, pts, tr), _ptr(cc), _ptr(out)))
    return _source_column(out)


def assemble_p2_source(points, tets, tris, c_tri=None, device=0, c_point=None):
    """P2 source vector of a :speaker boundary on the device (wae_p2_assemble_source, wae_p2_assemble_source_cpoint): as
    ``assemble_p1_source`` on the 6-node triangles; ``tets`` gives the edge numbers.  Returns m = -i·s, complex (npoints + nedges) x 1."""
    pts, tt, tr = _mesh_args(points, tets, tris)
    cc, nodal = _source_c(pts, tr.shape[0], c_tri, c_point)
    L = _lib.lib()
    out = np.zeros(pts.shape[0] + p2_edge_count(tt), dtype=np.float64)
    entry = L.wae_p2_assemble_source_cpoint if nodal else L.wae_p2_assemble_source
    _lib.check(entry(*_prefix(device, pts, tt, *_counted(tr)), _ptr(cc), _ptr(out), len(out)))
    return _source_column(out)


def p2_edge_count(tets):
    """number of distinct mesh edges = edge DoFs of the P2 space (host side; the device numbers them itself)"""
    tt = np.asarray(tets, dtype=np.int64).reshape(-1, 4)
    return len(np.unique(np.sort(np.concatenate([tt[:, [i, j]] for i in range(4) for j in range(i + 1, 4)]), axis=1), axis=0))


def _shape_arguments(pts, tt, order, c_tet, c_point, bnd_c, flame, vectors):
    """the checks of the shape-sensitivity keywords that need no device: element order, the form of the speed of sound, the flame's
    reference point, the lengths of the vectors.  Returns (c_point checked or None, dimension of the space)."""
    if order not in ("lin", "quad"):
        raise ValueError(f"order must be 'lin' or 'quad', not {order!r}")
    cp = _nodal(c_point, c_tet, pts.shape[0], "c_tet")
    if cp is not None and bnd_c is not None:
        raise ValueError("give the speed of sound per point (c_point) or per simplex (bnd_c), not both")
    if order == "quad" and flame is not None and flame.get("x_ref") is None:
        raise ValueError("order='quad': the flame needs x_ref, the point of the reference tetrahedron at which the gradients are taken")
    dim = pts.shape[0] + (p2_edge_count(tt) if order == "quad" else 0)
    for name, x in vectors:
        if np.shape(x) != (dim,):
            raise ValueError(f"{name} has shape {np.shape(x)}, the {'P2' if order == 'quad' else 'P1'} space has {dim} degrees of freedom")
    return cp, dim


def discrete_adjoint_shape_sensitivity(points, tets, c_tet, surface_points, sol, L, bnd_tris=None, bnd_c=None, Y=None, h=1e-9,
                                       device=0, flame=None, v_ext=None, order="lin", c_point=None):
    """sens = discrete_adjoint_shape_sensitivity(...)   (src/shape_sensitivity.jl:16-141, full mesh)

    Sensitivity of the eigenvalue ``sol.params[sol.eigval]`` to a displacement of every point in ``surface_points`` along
    x, y, z: -v_adj' (dL/dx) v with v'v = 1 and v_adj' L'(ω) v = 1 (the normalisation uses ``L``, the device-backed
    family).  The interior operators M, K (all tetrahedra touching the point) and, if given, the admittance boundary
    ω·Y·C (``bnd_tris``: boundary triangles, ``bnd_c``: speed of sound at each, ``Y``) take part, and -- round 3 -- the flame
    term: ``flame`` = dict(flame_tets, ref_tet, n_ref, nglobal_scaled[, coeff]) as produced by ``flame_description`` / the
    fixtures (``coeff``: the flame term's scalar n·exp(-iωτ) at ω; default: read from ``L``'s term with operator "Q").  As
    in the reference the flame domain is re-discretised REDUCED to the tetrahedra at the point, its volume included
    (``nlocal = nglobal_scaled / V_reduced``, Helmholtz.jl:325 on the reduced mesh of shape_sensitivity.jl:62-80).
    ``v_ext`` = (v, v_adj) already normalised and given on ``points`` (the unit-cell route extends the sector vectors to the
    image points and passes them here).
    ``order``: "lin" (P1) or "quad" (P2: the vectors have npoints + nedges entries in the numbering of ``p2_connectivity``, only the
    corner points of the straight-sided elements move, and ``flame`` needs ``x_ref``).  ``c_point`` (npoints,): the speed of sound per
    mesh point, linear on every simplex, instead of ``c_tet`` and ``bnd_c`` (the *_cpoint entries; the values stay with their points).
    Returns a complex array (3, len(surface_points))."""
    pts, tt, _ = _mesh_args(points, tets)
    cp, dim = _shape_arguments(pts, tt, order, c_tet, c_point, bnd_c, flame,
                               [("v", v_ext[0]), ("v_adj", v_ext[1])] if v_ext is not None else [("sol.v", sol.v), ("sol.v_adj", sol.v_adj)])
    quad = order == "quad"
    cc = cp if cp is not None else None if c_tet is None else np.ascontiguousarray(c_tet, dtype=np.float64)
    sp_ = np.asarray(surface_points, dtype=np.int64)
    w0 = complex(sol.params[sol.eigval])
    if v_ext is not None:
        v, va = (np.asarray(x, dtype=np.complex128) for x in v_ext)
    else:
        v = np.asarray(sol.v, dtype=np.complex128)
        v = v / np.sqrt(np.vdot(v, v))
        saved = (L.active, L.mode, dict(L.params))
        L.active, L.mode = [L.eigval], "all"
        try:
            va = np.asarray(sol.v_adj, dtype=np.complex128)
            va = va / np.conj(np.vdot(va, L(w0, 1) @ v))
        finally:
            L.active, L.mode, L.params = saved
    v, va = np.ascontiguousarray(v), np.ascontiguousarray(va)
    # (point, simplex) adjacency pairs, in surface-point order
    lut = np.full(pts.shape[0], -1, dtype=np.int64)
    lut[sp_] = np.arange(len(sp_))
    loc_t = lut[tt]
    it, ia = np.nonzero(loc_t >= 0)
    pair_tet = it.astype(np.int32)
    pair_pt_t = tt[it, ia].astype(np.int32)
    own_t = loc_t[it, ia]
    out_t = np.zeros((len(pair_tet), 3), dtype=np.complex128)
    tri = None
    npair_s = 0
    pair_tri = pair_pt_s = own_s = None
    out_s = np.zeros((0, 3), dtype=np.complex128)
    if bnd_tris is not None and len(bnd_tris):
        tri = np.ascontiguousarray(bnd_tris, dtype=np.int32).reshape(-1, 3)
        loc_s = lut[tri]
        js, ja = np.nonzero(loc_s >= 0)
        pair_tri, pair_pt_s, own_s = js.astype(np.int32), tri[js, ja].astype(np.int32), loc_s[js, ja]
        npair_s = len(pair_tri)
        out_s = np.zeros((npair_s, 3), dtype=np.complex128)
    dp, ip = DP, I32P
    om = np.array([w0.real, w0.imag])
    wy = complex(w0 * (Y if Y is not None else 0.0))
    omy = np.array([wy.real, wy.imag])
    bc = np.ascontiguousarray(bnd_c, dtype=np.float64) if npair_s and bnd_c is not None else None

    def P(a, t):
        return None if a is None else a.ctypes.data_as(t)
    lib = _lib.lib()
    entry = {(False, False): lib.wae_p1_shape_sensitivity, (False, True): lib.wae_p1_shape_sensitivity_cpoint,
             (True, False): lib.wae_p2_shape_sensitivity, (True, True): lib.wae_p2_shape_sensitivity_cpoint}[quad, cp is not None]
    args = [int(device), pts.shape[0], P(pts, dp), P(tt, ip), P(cc, dp), len(pair_tet), P(pair_pt_t, ip), P(pair_tet, ip),
            P(tri, ip) if npair_s else None]
    if cp is None:
        args.append(P(bc, dp))
    args += [npair_s, P(pair_pt_s, ip) if npair_s else None, P(pair_tri, ip) if npair_s else None,
             tt.shape[0], 0 if tri is None else tri.shape[0], P(om, dp), P(omy, dp)]
    if quad:
        args.append(dim)
    args += [v.view(np.float64).ctypes.data_as(dp), va.view(np.float64).ctypes.data_as(dp), float(h),
             out_t.view(np.float64).ctypes.data_as(dp) if len(pair_tet) else None, out_s.view(np.float64).ctypes.data_as(dp) if npair_s else None]
    _lib.check(entry(*args))
    sens = np.zeros((3, len(sp_)), dtype=np.complex128)
    np.add.at(sens.T, own_t, out_t)                                   # per point, in pair order: deterministic
    if npair_s:
        np.add.at(sens.T, own_s, out_s)
    if flame is not None:
        sens += _flame_shape_part(pts, tt, sp_, lut, v, va, w0, L, flame, h, device, order)
    return sens


def _flame_shape_part(pts, tt, sp_, lut, v, va, w0, L, flame, h, device, order="lin"):
    """-v_adj' n e^{-iωτ} (Q₊ - Q₋)/(2h) v per surface point and coordinate (wae_p1_shape_sensitivity_flame resp. wae_p2_shape_sensitivity_flame
    + the per-point sums).  The two orders differ in the entry and in the weights of S only: P1 S_a = |det J|/24 with ssum the plain sum of
    conj(v_adj), P2 S_a = |det J|·∫φ_a with the weights already inside ssum."""
    fl = np.asarray(flame["flame_tets"], dtype=np.int64)
    ref = int(flame["ref_tet"])
    nr = np.ascontiguousarray(flame["n_ref"], dtype=np.float64)
    coeff = flame.get("coeff")
    if coeff is None:
        k = [i for i, t in enumerate(L.terms) if t.operator == "Q"]
        assert len(k) == 1, "the family needs exactly one term with operator 'Q' (or pass flame['coeff'])"
        saved = (L.active, L.mode, dict(L.params))
        L.active, L.mode = [L.eigval], "all"
        try:
            coeff = complex(L.coefficients(w0)[k[0]])
        finally:
            L.active, L.mode, L.params = saved
    loc = lut[tt[fl]]                                                 # (nflame, 4): position of each node in surface_points, or -1
    it, ia = np.nonzero(loc >= 0)
    pair_tet = fl[it].astype(np.int32)
    pair_pt = tt[fl[it], ia].astype(np.int32)
    own = loc[it, ia]
    rsel = np.nonzero(lut[tt[ref]] >= 0)[0]
    pair_pt_r = tt[ref][rsel].astype(np.int32)
    own_r = lut[tt[ref]][rsel]
    npair, npr = len(pair_tet), len(pair_pt_r)
    det_pm = np.zeros((npair, 3, 2))
    ssum = np.zeros(npair, dtype=np.complex128)
    g_pm = np.zeros((npr, 3, 2), dtype=np.complex128)
    g0 = np.zeros(1, dtype=np.complex128)
    dp, ip = DP, I32P

    def P(a, t):
        return a.ctypes.data_as(t) if a.size else None
    outs = (P(det_pm, dp), P(ssum.view(np.float64), dp), P(g_pm.view(np.float64), dp), g0.view(np.float64).ctypes.data_as(dp))
    vecs = (v.view(np.float64).ctypes.data_as(dp), va.view(np.float64).ctypes.data_as(dp), float(h))
    mesh = (int(device), pts.shape[0], pts.ctypes.data_as(dp), tt.shape[0], tt.ctypes.data_as(ip), npair, P(pair_pt, ip), P(pair_tet, ip), ref, npr,
            P(pair_pt_r, ip))
    if order == "quad":
        xr = np.ascontiguousarray(flame["x_ref"], dtype=np.float64)
        assert xr.shape == (3,)
        _lib.check(_lib.lib().wae_p2_shape_sensitivity_flame(*mesh, xr.ctypes.data_as(dp), nr.ctypes.data_as(dp), len(v), *vecs, *outs))
    else:
        _lib.check(_lib.lib().wae_p1_shape_sensitivity_flame(*mesh, nr.ctypes.data_as(dp), *vecs, *outs))
    ns = len(sp_)
    a_pm = np.zeros((ns, 3, 2), dtype=np.complex128)                  # v_adj' S± per point and coordinate
    V_pm = np.zeros((ns, 3, 2))                                       # volume of the point's flame tetrahedra
    S_pm = det_pm if order == "quad" else det_pm / 24.0               # |det J| times the weight that ssum does not carry
    np.add.at(a_pm, own, S_pm * ssum[:, None, None])
    np.add.at(V_pm, own, det_pm / 6.0)
    b_pm = np.full((ns, 3, 2), g0[0], dtype=np.complex128)            # sum_b grad(phi_b).n_ref v_b on the reference tetrahedron
    b_pm[own_r] = g_pm
    out = np.zeros((3, ns), dtype=np.complex128)
    has = V_pm[:, 0, 0] > 0                                           # points without a flame tetrahedron: empty domain, no term
    nl = np.zeros_like(V_pm)
    nl[has] = float(flame["nglobal_scaled"]) / V_pm[has]
    q = a_pm * (-nl * b_pm)                                           # v_adj' Q± v  (g = -nlocal grad.n_ref)
    out[:, has] = (-coeff * (q[has, :, 0] - q[has, :, 1]) / (2 * h)).T
    return out


def herm_prolongators(points, tets, tris=None, device=0):
    """The p-hierarchy of a Hermite family on the device (wae_hermite_prolongators): ``[P_face, P_lin]``, scipy CSR, the form
    ``LinearOperatorFamily.solver_prolongators`` takes.  P_face (ndof x 4N) drops the face unknowns: the centroid value is the one the
    nine vertex data of the face fix when quadratics are to be reproduced.  P_lin (4N x N) drops the gradients: at a point, the
    volume-weighted mean of the P1 gradients of the tetrahedra around it.  ``tris`` numbers the faces as in ``assemble_herm``.
    ValueError, before the library is touched, for arrays that are not (npoints, 3) floats and (ntets, 4) / (ntris, 3) integers."""
    pts, tt, tr = _herm_mesh_checked(points, tets, tris)
    L = _lib.lib()
    h = C.c_void_p()
    _lib.check(L.wae_hermite_prolongators(*_prefix(device, pts, tt, *_counted(tr, True)), C.byref(h)))
    out = []
    try:
        for which in (0, 1):
            rows, cols, nnz = C.c_int64(0), C.c_int64(0), C.c_int64(0)
            _lib.check(L.wae_hermite_prolongators_info(h, which, C.byref(rows), C.byref(cols), C.byref(nnz)))
            ptr = np.zeros(rows.value + 1, dtype=np.int32)
            col = np.zeros(nnz.value, dtype=np.int32)
            val = np.zeros(nnz.value, dtype=np.float64)
            _lib.check(L.wae_hermite_prolongators_get(h, which, _ptr(ptr), _ptr(col), _ptr(val)))
            out.append(sp.csr_matrix((val, col, ptr), shape=(rows.value, cols.value)))
    finally:
        L.wae_hermite_prolongators_free(h)
    return out


def _herm_mesh_checked(points, tets, tris):
    """the mesh arrays of herm_prolongators as contiguous float64 / int32 arrays; ValueError for a wrong shape or dtype"""
    def ints(a, width, what):
        a = np.asarray(a)
        if a.dtype.kind not in "iu":
            raise ValueError(f"{what} must hold integers, got dtype {a.dtype}")
        if a.ndim != 2 or a.shape[1] != width:
            raise ValueError(f"{what} must have shape (n, {width}), got {a.shape}")
        if a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
            raise ValueError(f"{what} does not fit 32-bit indices")
        return np.ascontiguousarray(a, dtype=np.int32)
    pts = np.asarray(points)
    if pts.dtype.kind not in "fiu":
        raise ValueError(f"points must hold real numbers, got dtype {pts.dtype}")
    if pts.ndim != 2 or pts.shape[1] != 3 or pts.shape[0] < 1:
        raise ValueError(f"points must have shape (npoints, 3), got {pts.shape}")
    pts = np.ascontiguousarray(pts, dtype=np.float64)
    if not np.all(np.isfinite(pts)):
        raise ValueError("points holds a value that is not finite")
    tt = ints(tets, 4, "tets")
    if tt.shape[0] < 1:
        raise ValueError("tets must hold at least one tetrahedron")
    tr = None if tris is None else ints(tris, 3, "tris")
    return pts, tt, tr
