"""Host reference of the point location and the point functionals (csrc/locate.hip, helmholtz/locate.py) in numpy, sharing no code with the
product; pinned by tests/test_locref.py.  Everything is 0-based.

 - ``bary``: the barycentric coordinates by the device's Cramer formula, operation for operation (numpy rounds every one on its own), in
   float64 (the bits the device produces) or np.longdouble;
 - ``first_containing_tol``: brute force over all tetrahedra, the lowest index with all four coordinates >= -tol, -1 if none;
 - ``weight_rows``: the rows of probe_p / probe_n_grad_p for P1 and P2, in either precision;
 - ``cells``: a model of the cell grid: box, dims, the floor expression, the grown boxes of the tetrahedra, the list of every cell.
The keyword switches of ``first_containing_tol`` and ``cells`` (all off by default) plant the defects that tests/test_locref.py must catch."""
import numpy as np

EDGES = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
TOL_MAX = 1e-6
PAD = 4.0 * TOL_MAX + 2.0 ** -30
DIM_MAX = 1024
CELLS_PER_TET = 8


def _cross(u, v):
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], axis=-1)


def _dot(u, w):
    return (u[..., 0] * w[..., 0] + u[..., 1] * w[..., 1]) + u[..., 2] * w[..., 2]


def bary(P, x, n=None, dtype=np.float64):
    """P (..., 4, 3) corners, x (..., 3) points (broadcast against each other) -> l (..., 4); with n (..., 3) also g (..., 4) = n . grad l"""
    P, x = np.asarray(P, dtype=dtype), np.asarray(x, dtype=dtype)
    p4 = P[..., 3, :]
    a, b, c, r = P[..., 0, :] - p4, P[..., 1, :] - p4, P[..., 2, :] - p4, x - p4
    bc = _cross(b, c)
    det = _dot(a, bc)
    with np.errstate(divide="ignore", invalid="ignore"):
        l1 = _dot(r, bc) / det
        l2 = _dot(a, _cross(r, c)) / det
        l3 = _dot(a, _cross(b, r)) / det
        lam = np.stack([l1, l2, l3, dtype(1.0) - ((l1 + l2) + l3)], axis=-1)
        if n is None:
            return lam
        n = np.asarray(n, dtype=dtype)
        g1, g2, g3 = _dot(n, bc) / det, _dot(n, _cross(c, a)) / det, _dot(n, _cross(a, b)) / det
    return lam, np.stack([g1, g2, g3, -((g1 + g2) + g3)], axis=-1)


def all_coordinates(points, tets, X, dtype=np.float64, chunk=256):
    """(nq, ntets, 4): the coordinates of every point in every tetrahedron, as a generator over chunks of points: (q0, block)"""
    P = np.asarray(points, dtype=dtype)[np.asarray(tets, dtype=np.int64)]
    X = np.asarray(X, dtype=dtype)
    for q0 in range(0, len(X), chunk):
        yield q0, bary(P[None], X[q0:q0 + chunk, None, :], dtype=dtype)


def _first_containing_near(points, tets, X, tol, dtype, chunk=512):
    """first_containing_tol restricted, per point, to the tetrahedra whose bounding box grown by 1e-5 of the mesh extent holds it (a point
    that a tetrahedron accepts lies within 3 tol <= 3e-6 of the tetrahedron's own extent of its box): the same answers from far fewer
    coordinate evaluations on meshes of many tetrahedra; margin is taken over those tetrahedra -- another one is nowhere near a decision"""
    pts = np.asarray(points, dtype=np.float64)
    P = pts[np.asarray(tets, dtype=np.int64)]
    grow = 1e-5 * (pts.max(axis=0) - pts.min(axis=0))
    bmin, bmax = P.min(axis=1) - grow, P.max(axis=1) + grow
    Pd = P.astype(dtype)
    tet = np.full(len(X), -1, dtype=np.int32)
    lam = np.full((len(X), 4), np.nan, dtype=dtype)
    margin = np.full(len(X), np.inf)
    for q0 in range(0, len(X), chunk):
        Xc = X[q0:q0 + chunk]
        near = np.ones((len(Xc), len(P)), dtype=bool)
        for k in range(3):
            near &= (Xc[:, None, k] >= bmin[None, :, k]) & (Xc[:, None, k] <= bmax[None, :, k])
        qi, ti = np.nonzero(near)                                          # ascending by point, then by tetrahedron
        L = bary(Pd[ti], Xc[qi], dtype=dtype)
        with np.errstate(invalid="ignore"):
            m = np.abs(L.min(axis=1) + dtype(tol)).astype(np.float64)
        np.minimum.at(margin, q0 + qi, np.where(np.isnan(m), np.inf, m))
        hit = np.nonzero(np.all(L >= -dtype(tol), axis=1))[0]
        q_hit, first = np.unique(qi[hit], return_index=True)
        tet[q0 + q_hit] = ti[hit[first]]
        lam[q0 + q_hit] = L[hit[first]]
    return tet, lam, margin


def first_containing_tol(points, tets, X, tol, dtype=np.float64, last=False, oriented=False, near=False):
    """(tet (nq,) int32, lam (nq, 4), margin (nq,)): the lowest index whose coordinates are all >= -tol (-1: none), those coordinates (NaN
    for -1), and margin = min over ALL tetrahedra of |min_i l_i + tol|: how far the smallest coordinate, which decides, is from its threshold
    in any tetrahedron.
    near=True: the same search restricted to the tetrahedra whose grown bounding box holds the point (_first_containing_near).
    Seeded defects: last = the highest index instead; oriented = the sign test a formula without the division by det J would make
    (numerators against 0: right only where det J > 0)."""
    X = np.asarray(X, dtype=np.float64)
    if near:
        return _first_containing_near(points, tets, X, tol, dtype)
    tet = np.full(len(X), -1, dtype=np.int32)
    lam = np.full((len(X), 4), np.nan, dtype=dtype)
    margin = np.full(len(X), np.inf)
    if oriented:
        Pt = np.asarray(points, dtype=dtype)[np.asarray(tets, dtype=np.int64)]
        sgn = np.sign(np.linalg.det((Pt[:, :3] - Pt[:, 3:4]).astype(np.float64)))
    for q0, L in all_coordinates(points, tets, X, dtype):
        T = L * sgn[None, :, None] if oriented else L
        ok = np.all(T >= -dtype(tol), axis=2)
        with np.errstate(invalid="ignore"):
            margin[q0:q0 + len(L)] = np.nanmin(np.abs(L.min(axis=2) + dtype(tol)), axis=1).astype(np.float64)
        for i in range(len(L)):
            hit = np.nonzero(ok[i])[0]
            if len(hit):
                t = hit[-1] if last else hit[0]
                tet[q0 + i] = t
                lam[q0 + i] = L[i, t]
    return tet, lam, margin


def nodes_p2(npoints, tets):
    """(tets10 (ntets, 10), ndof): the points, then the edges (0,1) (0,2) (0,3) (1,2) (1,3) (2,3), edge DoF = npoints + the position of the
    edge in the list ascending by (smaller point, larger point)"""
    tt = np.asarray(tets, dtype=np.int64)
    pairs = np.stack([np.sort(tt[:, [i, j]], axis=1) for i, j in EDGES], axis=1)
    keys = pairs[..., 0] * npoints + pairs[..., 1]
    uniq = np.unique(keys)
    return np.concatenate([tt, npoints + np.searchsorted(uniq, keys)], axis=1).astype(np.int32), npoints + len(uniq)


def weight_rows(points, tets, X, tet, order=1, kind=0, n=None, dtype=np.longdouble):
    """val (nq, 4 | 10) of the functionals at the points X in their tetrahedra tet (all >= 0), in the operation order of the device"""
    P = np.asarray(points, dtype=dtype)[np.asarray(tets, dtype=np.int64)[np.asarray(tet, dtype=np.int64)]]
    if kind == 0:
        l = bary(P, X, dtype=dtype)
    else:
        l, g = bary(P, X, n=np.broadcast_to(np.asarray(n, dtype=dtype), np.shape(X)), dtype=dtype)
    one, two, four = dtype(1.0), dtype(2.0), dtype(4.0)
    if order == 1:
        return l if kind == 0 else g
    if kind == 0:
        return np.concatenate([l * (two * l - one), np.stack([(four * l[:, i]) * l[:, j] for i, j in EDGES], axis=1)], axis=1)
    return np.concatenate([(four * l - one) * g, np.stack([four * (l[:, j] * g[:, i] + l[:, i] * g[:, j]) for i, j in EDGES], axis=1)], axis=1)


def conditioning(points, tets, tet):
    """(kappa_inf(J), ||J^-1||_inf) of the listed tetrahedra"""
    P = np.asarray(points, dtype=np.float64)[np.asarray(tets, dtype=np.int64)[np.asarray(tet, dtype=np.int64)]]
    J = np.transpose(P[:, :3] - P[:, 3:4], (0, 2, 1))
    Ji = np.linalg.inv(J)
    ninf = lambda A: np.abs(A).sum(axis=2).max(axis=1)
    return ninf(J) * ninf(Ji), ninf(Ji)


# ---- the cell grid -----------------------------------------------------------------------------------------------------------------------
def grid_dims(lo, hi, ntets, cell_target):
    """about ntets / cell_target cells (0: 8 per cell), as cubical as the box allows, at most DIM_MAX per axis and, halving all axes until
    it holds, at most CELLS_PER_TET * ntets cells"""
    want = ntets / float(cell_target if cell_target > 0 else 8)
    ext = hi - lo
    ax = ext > 0
    dims = np.ones(3, dtype=np.int64)
    if not ax.any() or not want > 1.0:
        return dims
    h = (np.prod(ext[ax]) / want) ** (1.0 / ax.sum())
    dims[ax] = np.clip(np.ceil(ext[ax] / h), 1, DIM_MAX).astype(np.int64)
    while np.prod(dims) > CELLS_PER_TET * ntets:
        dims = (dims + 1) // 2
    return dims


def axis_cell(x, lo, inv, dim, clamp=True, other_floor=False):
    """the device's expression clamp(floor((x - lo) * inv), 0, dim - 1); other_floor: a different but equally plausible expression
    (floor(x * inv - lo * inv)); clamp=False leaves the upper end open"""
    f = np.floor(x * inv - lo * inv) if other_floor else np.floor((x - lo) * inv)
    f = np.maximum(f, 0)
    return (np.minimum(f, dim - 1) if clamp else f).astype(np.int64)


class Cells:
    """lo, hi, dims, inv, lists: dict cell -> ascending tetrahedron indices; nrefs; ``cell_of(X)`` (-1 outside the box or the grid)"""


def cells(points, tets, cell_target=0, dims=None, inflate=True, point_other_floor=False, clamp_upper=True):
    """The model.  Seeded defects: inflate=False (the bare boxes), point_other_floor (points use another floor expression than the box
    corners), clamp_upper=False (a point on an upper face of the box gets no cell)."""
    pts = np.asarray(points, dtype=np.float64)
    tt = np.asarray(tets, dtype=np.int64)
    G = Cells()
    G.lo, G.hi = pts.min(axis=0), pts.max(axis=0)
    d = grid_dims(G.lo, G.hi, len(tt), cell_target) if dims is None else np.asarray(dims, dtype=np.int64)
    G.pad = PAD * (G.hi - G.lo)                      # (the rim of the box in which a point is still looked up)
    pad = G.pad if inflate else np.zeros(3)
    P = pts[tt]
    bmin, bmax = P.min(axis=1) - pad, P.max(axis=1) + pad
    while True:
        ext = G.hi - G.lo
        inv = np.where(ext > 0, d / np.where(ext > 0, ext, 1.0), 0.0)
        c0 = np.stack([axis_cell(bmin[:, k], G.lo[k], inv[k], d[k]) for k in range(3)], axis=1)
        c1 = np.stack([axis_cell(bmax[:, k], G.lo[k], inv[k], d[k]) for k in range(3)], axis=1)
        nrefs = int(np.prod(c1 - c0 + 1, axis=1).sum())
        if nrefs <= 32 * len(tt) or np.all(d == 1):
            break
        d = (d + 1) // 2
    G.dims, G.inv, G.nrefs = d, inv, nrefs
    G.lists = {}
    for t in range(len(tt)):
        for z in range(c0[t, 2], c1[t, 2] + 1):
            for y in range(c0[t, 1], c1[t, 1] + 1):
                for x in range(c0[t, 0], c1[t, 0] + 1):
                    G.lists.setdefault(int((z * d[1] + y) * d[0] + x), []).append(t)

    def cell_of(X):
        X = np.asarray(X, dtype=np.float64)
        inside = np.all((X >= G.lo - G.pad) & (X <= G.hi + G.pad), axis=1)
        c = np.stack([axis_cell(X[:, k], G.lo[k], inv[k], d[k], clamp=clamp_upper, other_floor=point_other_floor) for k in range(3)], axis=1)
        ingrid = np.all(c < d, axis=1)
        return np.where(inside & ingrid, (c[:, 2] * d[1] + c[:, 1]) * d[0] + c[:, 0], -1)

    G.cell_of = cell_of
    return G


def find_by_cells(points, tets, G, X, tol, last=False):
    """the query through the model's lists: what the device does"""
    P = np.asarray(points, dtype=np.float64)[np.asarray(tets, dtype=np.int64)]
    out = np.full(len(X), -1, dtype=np.int32)
    for q, c in enumerate(G.cell_of(X)):
        cand = G.lists.get(int(c), []) if c >= 0 else []
        if not len(cand):
            continue
        ok = np.all(bary(P[cand], np.asarray(X[q], dtype=np.float64)[None]) >= -tol, axis=1)
        hit = np.nonzero(ok)[0]
        if len(hit):
            out[q] = cand[hit[-1] if last else hit[0]]
    return out


def expression_mismatches(G, other_floor=True, ulps=4):
    """the number of coordinates within a few ulps of a cell boundary that the points' expression puts into another cell than the box
    corners' expression: 0 when the two are the same expression (the monotonicity argument needs no more), > 0 for another one"""
    bad = 0
    for k in range(3):
        if G.dims[k] < 2:
            continue
        v = G.lo[k] + np.arange(1, G.dims[k]) / G.inv[k]
        up, down, vals = v, v, [v]
        for _ in range(ulps):
            up, down = np.nextafter(up, np.inf), np.nextafter(down, -np.inf)
            vals += [up, down]
        vals = np.concatenate(vals)
        bad += int(np.sum(axis_cell(vals, G.lo[k], G.inv[k], G.dims[k], other_floor=other_floor) != axis_cell(vals, G.lo[k], G.inv[k], G.dims[k])))
    return bad


# ---- query sets --------------------------------------------------------------------------------------------------------------------------
def edge_midpoints(points, tets):
    tt = np.asarray(tets, dtype=np.int64)
    pairs = np.unique(np.sort(np.concatenate([tt[:, [i, j]] for i, j in EDGES]), axis=1), axis=0)
    return (points[pairs[:, 0]] + points[pairs[:, 1]]) * 0.5


def boundary_offsets(points, tets, factor, tol=TOL_MAX, limit=200):
    """points displaced outward from the centroids of boundary faces (faces of one tetrahedron only) by factor * tol * the local height
    (the distance of the opposite corner from the face): barycentric coordinate -factor * tol in the owner"""
    tt = np.asarray(tets, dtype=np.int64)
    faces = {}
    for t, v in enumerate(tt):
        for k in range(4):
            faces.setdefault(tuple(sorted(np.delete(v, k))), []).append((t, k))
    out = []
    for key in sorted(faces):
        if len(faces[key]) == 1 and len(out) < limit:
            t, k = faces[key][0]
            lam = np.full(4, (1.0 + factor * tol) / 3.0)
            lam[k] = -factor * tol
            out.append(lam @ points[tt[t]])
    return np.array(out)


def dyadic_points():
    """vertices, edge midpoints, face and cell centres of the 2 x 2 x 2 Kuhn cube of edge 1: all multiples of 1/4 in [0, 1]^3"""
    g = np.arange(5) * 0.25
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
