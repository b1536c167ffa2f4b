"""GPU tests (-m gpu) of the point locator (csrc/locate.hip through helmholtz/locate.py) against tests/_locref.py (pinned by
tests/test_locref.py): the located tetrahedra and their coordinates, independence of the cell grid, repeatability, the weight rows, the
gather kernel, polynomial exactness, the nested hierarchy, forced-response observers and the error contract of the C entries.

Meshes: the five of _octoref.mesh and `rijke1`, the level-1 octosplit of the Rijke tube (27 040 tetrahedra), each at cell_target 1, the
default and ntets (one cell).  Query sets (seeded): 2 000 uniform points in the box enlarged by 10 % a side (inside and outside), 40 points
far outside the box, the six points that attain the box's faces, all vertices, all edge midpoints, all centroids.  On rijke1 the host
brute force (computed once and shared) sees a seeded 500 of each of the last three, so that it stays at a few seconds; the full sets of
that mesh (about 68 000 points) go through the checks that need no host search: test_full_sets_on_the_large_mesh."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import _locref as R
import _octoref as O
from wae_amd import _lib
from wae_amd.helmholtz import Locator, octosplit
from wae_amd.helmholtz.assemble import p2_connectivity

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
INVALID = _lib.WAE_ERR_INVALID
NAMES = ["one", "two", "cube", "sheared", "rijke", "rijke1"]
SMALL = ["two", "sheared", "rijke"]
# the weight bound: see test_weight_rows
C_MEASURED = 1.2
C_WEIGHTS = 8 * C_MEASURED
N_DIR = np.array([0.3, -0.5, 0.8])


@functools.lru_cache(maxsize=None)
def mesh(name):
    if name == "rijke1":
        L = O.refine(*O.mesh("rijke"), levels=1)[1]
        return L.points, L.tets
    pts, tets, _ = O.mesh(name)
    return pts, tets


@functools.lru_cache(maxsize=None)
def queries(name):
    """dict of the query sets, and their concatenation under "all" with the slices under "slices" """
    pts, tets = mesh(name)
    rng = np.random.default_rng(17)
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    pick = (lambda A: A[np.sort(rng.permutation(len(A))[:500])]) if name == "rijke1" else (lambda A: A)
    sets = {"uniform": lo + rng.uniform(-0.1, 1.1, (2000, 3)) * (hi - lo),
            "outside": hi + rng.uniform(0.5, 2.0, (40, 3)) * (hi - lo) * rng.choice([-3.0, 1.0], (40, 3)),
            "extreme": np.concatenate([pts[np.argmax(pts, axis=0)], pts[np.argmin(pts, axis=0)]]),       # on the faces of the box
            "vertices": pick(pts), "midpoints": pick(R.edge_midpoints(pts, tets)), "centroids": pick(pts[tets].mean(axis=1))}
    out, sl, k = dict(sets), {}, 0
    for key, A in sets.items():
        sl[key] = slice(k, k + len(A))
        k += len(A)
    out["all"], out["slices"] = np.concatenate(list(sets.values())), sl
    return out


@functools.lru_cache(maxsize=None)
def reference(name, tol=0.0):
    """(tet, lam, margin) of _locref.first_containing_tol on queries(name)["all"] in float64"""
    pts, tets = mesh(name)
    return R.first_containing_tol(pts, tets, queries(name)["all"], tol, near=len(tets) > 1000)


@functools.lru_cache(maxsize=None)
def locator(name, which):
    pts, tets = mesh(name)
    return Locator(pts, tets, cell_target={"fine": 1, "default": 0, "one": len(tets)}[which])


@functools.lru_cache(maxsize=None)
def found(name, which):
    return locator(name, which).find(queries(name)["all"], barycentric=True)


# ---- find --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["fine", "default", "one"])
@pytest.mark.parametrize("name", NAMES)
def test_find_at_tol_zero(name, which):
    pts, tets = mesh(name)
    Q = queries(name)
    X, sl = Q["all"], Q["slices"]
    ref_tet, ref_lam, margin = reference(name)
    tet, lam = found(name, which)
    loc = locator(name, which)
    assert tet.dtype == np.int32 and tet.shape == (len(X),) and lam.shape == (len(X), 4)
    if which == "one":
        assert loc.dims == (1, 1, 1) and loc.nrefs == len(tets) == loc.max_per_cell
    else:
        assert len(tets) <= loc.nrefs <= 32 * len(tets) and 1 <= loc.max_per_cell <= len(tets)
    # unambiguous points: the same index, and (the same formula, operation for operation) the same coordinates
    clear = margin >= 1e-9
    assert clear[sl["uniform"]].mean() >= 0.9 and clear[sl["centroids"]].all()
    assert np.array_equal(tet[clear], ref_tet[clear])
    assert np.array_equal(lam[clear], ref_lam[clear], equal_nan=True)
    assert np.all(tet[sl["outside"]] == -1) and np.all(np.isnan(lam[tet < 0])) and np.all(lam[tet >= 0] >= 0)
    assert np.all(tet[sl["centroids"]] >= 0)
    # the others (vertices, midpoints: on faces): the answer holds the point to 1e-12 in extended precision, and no tetrahedron before
    # it holds it by more than that
    amb = np.nonzero(~clear)[0]
    if len(amb):
        Xa, ta = X[amb], tet[amb]
        strict = R.first_containing_tol(pts, tets, Xa, -1e-12, dtype=np.longdouble, near=len(tets) > 1000)[0]
        got = ta >= 0
        la = R.bary(pts[tets[ta[got]]], Xa[got], dtype=np.longdouble)
        assert np.all(la >= -1e-12)
        assert np.all(strict[~got] == -1)
        assert np.all((strict[got] == -1) | (strict[got] >= ta[got]))
    # what the inputs must exercise: misses, clamped points (on an upper face of the box), ties
    assert (tet[sl["uniform"]] < 0).any() and (tet[sl["uniform"]] >= 0).any()
    assert np.any(Q["extreme"] == pts.max(axis=0)) and (tet[sl["extreme"]] >= 0).any()


@pytest.mark.parametrize("which", ["fine", "default", "one"])
@pytest.mark.parametrize("name", ["cube", "one"])
def test_dyadic_queries_are_decided_bit_for_bit(name, which):
    """ties between up to 24 tetrahedra, every operation exact (tests/test_locref.py; on `one` without the origin, which is inexact there)"""
    pts, tets = mesh(name)
    X = R.dyadic_points()
    if name == "one":
        X = X[np.any(X != 0.0, axis=1)]
    ref_tet, ref_lam, _ = R.first_containing_tol(pts, tets, X, 0.0)
    tet, lam = locator(name, which).find(X, barycentric=True)
    assert np.array_equal(tet, ref_tet) and np.array_equal(lam, ref_lam, equal_nan=True)
    assert np.array_equal(tet, np.array([O.first_containing(pts, tets, x) for x in X]))
    if name == "cube":
        L = np.concatenate([b for _, b in R.all_coordinates(pts, tets, X)])
        assert (np.all(L >= 0, axis=2).sum(axis=1) > 1).sum() > 60 and np.all(tet >= 0)


@pytest.mark.parametrize("name", NAMES)
def test_find_with_a_tolerance(name):
    pts, tets = mesh(name)
    near, far = R.boundary_offsets(pts, tets, 0.5), R.boundary_offsets(pts, tets, 2.0)
    X = np.concatenate([near, far, queries(name)["all"][:300]])
    ref = R.first_containing_tol(pts, tets, X, 1e-6, near=len(tets) > 1000)
    assert np.all(ref[0][:len(near)] >= 0) and np.all(ref[0][len(near):len(near) + len(far)] == -1)
    res = [locator(name, w).find(X, tol=1e-6, barycentric=True) for w in ("fine", "default", "one")]
    for tet, lam in res:
        assert np.all(tet[:len(near)] >= 0) and np.all(tet[len(near):len(near) + len(far)] == -1)
        assert np.array_equal(tet, ref[0]) and np.array_equal(lam, ref[1], equal_nan=True)
    assert np.all(locator(name, "default").find(near) == -1)              # at tol = 0 they are outside


@pytest.mark.parametrize("name", NAMES)
def test_results_do_not_depend_on_the_grid_and_repeat(name):
    a, b, c = (found(name, w) for w in ("fine", "default", "one"))
    for o in (b, c):
        assert np.array_equal(a[0], o[0]) and np.array_equal(a[1].view(np.int64), o[1].view(np.int64))
    again = locator(name, "default").find(queries(name)["all"], barycentric=True)
    assert np.array_equal(again[0], b[0]) and np.array_equal(again[1].view(np.int64), b[1].view(np.int64))
    pts, tets = mesh(name)
    fresh = Locator(pts, tets)
    assert (fresh.dims, fresh.nrefs, fresh.max_per_cell) == (locator(name, "default").dims, locator(name, "default").nrefs,
                                                             locator(name, "default").max_per_cell)
    assert np.array_equal(fresh.find(queries(name)["all"]), b[0])
    fresh.close()
    fresh.close()


def test_full_sets_on_the_large_mesh():
    """all vertices, all edge midpoints and all centroids of rijke1 without a host search: the three grids agree bit for bit, the one-cell
    grid being the device's own brute force in list order; every centroid is found in its own tetrahedron (the only one that holds it);
    every vertex and midpoint that is found lies in the returned tetrahedron to 1e-12 in extended precision, and the few that no tetrahedron
    accepts at tol = 0 (a rounding residue below zero on a face) are found at tol = 1e-6"""
    pts, tets = mesh("rijke1")
    sets = [pts, R.edge_midpoints(pts, tets), pts[tets].mean(axis=1)]
    X = np.ascontiguousarray(np.concatenate(sets))
    nc = len(tets)
    assert len(X) - nc > 30000
    a, b, c = (locator("rijke1", w).find(X, barycentric=True) for w in ("fine", "default", "one"))
    for o in (b, c):
        assert np.array_equal(a[0], o[0]) and np.array_equal(a[1].view(np.int64), o[1].view(np.int64))
    tet, lam = a
    assert np.array_equal(tet[-nc:], np.arange(nc))
    got = tet >= 0
    print(f"rijke1 full sets: {len(X)} points, {np.sum(~got)} not found at tol = 0")
    assert got.mean() > 0.9 and np.all(lam[got] >= 0) and np.all(np.isnan(lam[~got]))
    assert np.all(R.bary(pts[tets[tet[got]]], X[got], dtype=np.longdouble) >= -1e-12)
    if (~got).any():
        assert np.all(locator("rijke1", "fine").find(X[~got], tol=1e-6) >= 0)


def test_cell_count_is_bounded_by_the_mesh():
    """a thin box at cell_target = 1: rounding the short axes up to one cell leaves far more than ntets cells along the long one; the grid
    is halved to at most 8 ntets cells (the model of _locref.cells has the same rule) and answers as before"""
    pts, tets = mesh("two")
    thin = np.ascontiguousarray(pts * np.array([1.0, 1.0, 4000.0]))
    G = R.cells(thin, tets, 1)
    loc = Locator(thin, tets, cell_target=1)
    try:
        assert np.prod(loc.dims) <= 8 * len(tets) and loc.dims == tuple(int(v) for v in G.dims) and loc.nrefs == G.nrefs
        R.CELLS_PER_TET, keep = 10 ** 9, R.CELLS_PER_TET
        try:
            assert np.prod(R.cells(thin, tets, 1).dims) > 8 * len(tets)        # the rule is what bounds it
        finally:
            R.CELLS_PER_TET = keep
        assert np.array_equal(loc.find(thin[tets].mean(axis=1)), np.arange(len(tets)))
    finally:
        loc.close()


# ---- weights and sampling ------------------------------------------------------------------------------------------------------------------
def located_points(name, count=600):
    """a seeded share of the located queries, with their tetrahedra"""
    tet = reference(name)[0]
    X = queries(name)["all"]
    sel = np.nonzero(tet >= 0)[0]
    sel = sel[:: max(1, len(sel) // count)]
    return X[sel], tet[sel]


def measured_weight_ratio(name):
    """the largest |float64 transliteration - longdouble| / (eps kappa_inf(J) [||J^-1||_inf ||n||]) over the rows of one mesh"""
    pts, tets = mesh(name)
    X, t = located_points(name)
    kap, jinv = R.conditioning(pts, tets, t)
    worst = 0.0
    for order in (1, 2):
        for kind in (0, 1):
            d = np.abs(R.weight_rows(pts, tets, X, t, order, kind, N_DIR, dtype=np.float64)
                       - R.weight_rows(pts, tets, X, t, order, kind, N_DIR).astype(np.float64)).max(axis=1)
            worst = max(worst, np.max(d / (EPS * kap * (jinv * np.linalg.norm(N_DIR) if kind else 1.0))))
    return worst


@pytest.mark.parametrize("order", ["lin", "quad"])
@pytest.mark.parametrize("name", NAMES)
def test_weight_rows(name, order):
    """|val_dev - val_ref| <= c eps kappa_inf(J) per row against the longdouble rows of _locref, for kind "n_grad_p" times ||J^-1||_inf
    ||n||.  c: the float64 transliteration of the device formula in _locref.py reaches at most C_MEASURED times eps kappa against
    longdouble on these same inputs (measured_weight_ratio: 0.57, 0.45, 0.34, 0.93, 1.06, 1.19 on the six meshes, on the CPU); c =
    C_WEIGHTS = 9.6 is 8 times that, which covers
    another equally stable operation order and fused multiply-adds on the device."""
    pts, tets = mesh(name)
    X, t = located_points(name)
    no = 1 if order == "lin" else 2
    t10 = p2_connectivity(pts, tets)[1] if no == 2 else None
    nodes = tets if no == 1 else t10
    if no == 2:
        assert np.array_equal(np.sort(t10, axis=1), np.sort(R.nodes_p2(len(pts), tets)[0], axis=1))
    kap, jinv = R.conditioning(pts, tets, t)
    loc = locator(name, "default")
    for kind, kname in ((0, "p"), (1, "n_grad_p")):
        n = N_DIR if kind else None
        idx, val = loc.weights(X, order, kname, n=n, tets10=t10)
        idx2, val2 = loc.weights(X, order, kname, n=n, tet=t, tets10=t10)
        assert np.array_equal(idx, idx2) and np.array_equal(val, val2)
        assert idx.dtype == np.int32 and np.array_equal(idx, nodes[t])
        ref = R.weight_rows(pts, tets, X, t, no, kind, N_DIR)
        err = np.abs(val.astype(np.longdouble) - ref).max(axis=1).astype(np.float64)
        bound = C_WEIGHTS * EPS * kap * (jinv * np.linalg.norm(N_DIR) if kind else 1.0)
        print(f"{name} {order} {kname}: max err / (eps kappa [|J^-1| |n|]) = {np.max(err / bound) * C_WEIGHTS:.2f}, host float64 "
              f"{measured_weight_ratio(name):.2f}")
        assert np.all(err <= bound)
    # the rows of points outside: idx 0, val 0 under outside="nan", an error that names the first under "raise"
    Xo = np.concatenate([X[:3], queries(name)["outside"][:2]])
    idx, val = loc.weights(Xo, order, tets10=t10, outside="nan")
    assert np.all(idx[3:] == 0) and np.all(val[3:] == 0) and np.array_equal(idx[:3], nodes[t[:3]])
    with pytest.raises(ValueError, match="point 3"):
        loc.weights(Xo, order, tets10=t10)


@pytest.mark.parametrize("ncols", [1, 3, 8])
@pytest.mark.parametrize("name", SMALL + ["rijke1"])
def test_sample_is_the_row_sum_in_order(name, ncols):
    """out[q, c] against sum_i val[q, i] V[idx[q, i], c] accumulated in float64 in the order of i, val the float64 rows of _locref (the
    device's formula operation for operation), within 16 eps sum_i |val_i| |V_i| per entry"""
    pts, tets = mesh(name)
    X, t = located_points(name, 300)
    Xo = np.concatenate([X, queries(name)["outside"][:5]])
    rng = np.random.default_rng(ncols)
    loc = locator(name, "default")
    t10 = p2_connectivity(pts, tets)[1]
    for order, no, nodes in (("lin", 1, tets), ("quad", 2, t10)):
        d = int(nodes.max()) + 1
        V = rng.standard_normal((d, ncols)) + 1j * rng.standard_normal((d, ncols))
        for kind, kname in ((0, "p"), (1, "n_grad_p")):
            n = N_DIR if kind else None
            val = R.weight_rows(pts, tets, X, t, no, kind, N_DIR, dtype=np.float64)
            want = np.zeros((len(X), ncols), dtype=np.complex128)
            mag = np.zeros((len(X), ncols))
            for i in range(val.shape[1]):
                want = want + val[:, i, None] * V[nodes[t, i]]
                mag += np.abs(val[:, i, None]) * np.abs(V[nodes[t, i]])
            got = loc.sample(V, Xo, order, kname, n=n, tets10=t10, outside="nan")
            assert got.shape == (len(Xo), ncols) and got.dtype == np.complex128
            assert np.all(np.isnan(got[len(X):].real)) and np.all(np.isnan(got[len(X):].imag))
            assert np.all(np.abs(got[:len(X)] - want) <= 16 * EPS * mag)
            with pytest.raises(ValueError):
                loc.sample(V, Xo, order, kname, n=n, tets10=t10)
    v1 = loc.sample(V[:, 0], X, "quad", tets10=t10)
    assert v1.shape == (len(X),) and np.array_equal(v1, loc.sample(V[:, :1], X, "quad", tets10=t10)[:, 0])


@pytest.mark.parametrize("name", NAMES)
def test_polynomials_are_reproduced(name):
    """an affine function from its P1 vector, a quadratic from its P2 vector, at every located point to 1e-13 max|f| (the bound of the quadratic
    reproduction in tests/test_gpu_p2_prolong.py), their derivatives along a direction to 1e-11 max|grad f| (maxima over the mesh
    points): no reference involved.  The float64 rows of _locref reach 5e-16 and 2e-13 on these inputs."""
    pts, tets = mesh(name)
    X, _ = located_points(name, 2000)
    loc = locator(name, "fine")
    c = pts.mean(axis=0)
    s = 1.0 / np.max(pts.max(axis=0) - pts.min(axis=0))
    g, A = np.array([0.7, -1.1, 0.4]), np.array([[0.5, 0.2, -0.3], [0.2, -0.8, 0.1], [-0.3, 0.1, 0.6]])
    aff = lambda Y: 0.3 + ((Y - c) * s) @ g
    quad = lambda Y: aff(Y) + np.einsum("qi,ij,qj->q", (Y - c) * s, A, (Y - c) * s)
    daff = lambda Y: np.full(len(Y), s * (g @ N_DIR))
    dquad = lambda Y: s * (g @ N_DIR) + 2 * s * (((Y - c) * s) @ A @ N_DIR)
    edges, t10, _ = p2_connectivity(pts, tets)
    mids = (pts[edges[:, 0]] + pts[edges[:, 1]]) * 0.5
    v1, v2 = aff(pts), np.concatenate([quad(pts), quad(mids)])
    gmax1 = s * np.linalg.norm(g)
    gmax2 = np.max(np.linalg.norm(s * g + 2 * s * ((pts - c) * s) @ A, axis=1))
    e1 = np.max(np.abs(loc.sample(v1, X).real - aff(X))) / np.max(np.abs(v1))
    e2 = np.max(np.abs(loc.sample(v2, X, "quad", tets10=t10).real - quad(X))) / np.max(np.abs(v2))
    d1 = np.max(np.abs(loc.sample(v1, X, kind="n_grad_p", n=N_DIR).real - daff(X))) / gmax1
    d2 = np.max(np.abs(loc.sample(v2, X, "quad", "n_grad_p", n=N_DIR, tets10=t10).real - dquad(X))) / gmax2
    print(f"{name}: affine {e1:.2e}, quadratic {e2:.2e} of max|f|; derivatives {d1:.2e}, {d2:.2e} of max|grad f|")
    assert e1 <= 1e-13 and e2 <= 1e-13
    assert d1 <= 1e-11 and d2 <= 1e-11


# ---- the layers above ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cube", "rijke"])
def test_interpolation_onto_a_refinement_is_its_prolongator(name):
    pts, tets, tris = O.mesh(name)
    Rm = octosplit(pts, tets, tris, levels=2 if name == "cube" else 1)
    P = Rm.prolongator(0)
    P.eliminate_zeros()
    loc = Locator(Rm.points[0], Rm.tets[0])
    I = loc.interpolation(Rm.points[1])
    assert sp.isspmatrix_csr(I) and I.shape == P.shape and I.indices.dtype == np.int32 and I.has_sorted_indices
    if name == "cube":
        assert np.array_equal(I.indptr, P.indptr) and np.array_equal(I.indices, P.indices) and np.array_equal(I.data, P.data)
    else:
        assert abs(I - P).max() <= 1e-14
    I2 = loc.interpolation(Rm.points[1], order="quad")
    assert I2.shape == (len(Rm.points[1]), Rm.ndof(0, "quad")) and np.max(np.abs(np.asarray(I2.sum(axis=1)) - 1)) <= 1e-13


def test_observers_feed_the_forced_response():
    """the microphone array of tests/test_gpu_forcing.py's Rijke P1 sweep from one call: the same H as its per-point probe_p observers, to
    the 1e-8 of that file's observer comparison (what is read from a linear solve)"""
    import _forcingref as F
    from wae_amd.helmholtz.assemble import assemble_p1_source
    from wae_amd.helmholtz.family import helmholtz_family, speaker_source
    from wae_amd.helmholtz.probe import probe_n_grad_p, probe_p
    from wae_amd.nlevp import forced_response
    pts, tets, tris, c_tri = F.rijke_mesh()
    mics = np.array([[0.004, -0.003, 0.10], [-0.006, 0.005, -0.18], [0.001, 0.002, 0.05]])
    nz = np.array([0.0, 0.0, 1.0])
    omegas = F.rijke_p1_sweep()[0][:4]
    Lp = helmholtz_family(F.rijke_terms(), Y=F.RIJKE["Y"], n=F.RIJKE["n"], tau=F.RIJKE["tau"])
    Lp.solver_ref = 2 * np.pi * 400
    rhs = speaker_source(assemble_p1_source(pts, tris, c_tri=c_tri), Y=F.RIJKE["Y"], A=F.RIJKE["A"])
    loc = Locator(pts, tets)
    obs = loc.observers(mics) + loc.observers(mics[:1], kind="n_grad_p", n=nz)
    old = [probe_p(pts, tets, x) for x in mics] + [probe_n_grad_p(pts, tets, mics[0], nz)]
    for (i1, v1), (i0, v0) in zip(obs, old):
        assert np.array_equal(np.sort(i1), np.sort(i0))
    try:
        H1 = forced_response(Lp, rhs, omegas, observers=obs, tol=1e-12).H
        H0 = forced_response(Lp, rhs, omegas, observers=old, tol=1e-12).H
    finally:
        Lp._drop_device()
    assert H1.shape == (4, 4) and np.max(np.abs(H1 - H0)) / np.max(np.abs(H0)) < 1e-8


# ---- the error contract of the C entries -----------------------------------------------------------------------------------------------------
def test_error_contract_and_the_handle_stays_usable():
    L = _lib.lib()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    pts, tets = mesh("cube")
    pts, tets = np.ascontiguousarray(pts), np.ascontiguousarray(tets, dtype=np.int32)
    np_, nt = len(pts), len(tets)
    D, I = (lambda a: a.ctypes.data_as(dp)), (lambda a: a.ctypes.data_as(ip))

    def refused(code):
        msg = L.wae_last_error().decode()
        assert code == INVALID and msg, (code, msg)

    h = C.c_void_p()
    bad_t, bad_p = tets.copy(), pts.copy()
    bad_t[5, 2], bad_p[3, 1] = np_, np.inf
    low_t = tets.copy()
    low_t[0, 0] = -1
    for args in ((-1, pts, nt, tets, 0), (np_, pts, -1, tets, 0), (np_, pts, nt, tets, -1), (np_, pts, nt, bad_t, 0), (np_, pts, nt, low_t, 0),
                 (np_, bad_p, nt, tets, 0)):
        refused(L.wae_locator_create(0, args[0], D(args[1]), args[2], I(args[3]), args[4], C.byref(h)))
        assert not h.value
    assert L.wae_locator_create(0, np_, D(pts), nt, I(tets), 0, C.byref(h)) == 0 and h.value
    try:
        X = np.ascontiguousarray(queries("cube")["all"][:64])
        nq = len(X)
        want = reference("cube")[0][:64]
        tet, lam = np.zeros(nq, dtype=np.int32), np.zeros((nq, 4))
        idx, val = np.zeros((nq, 10), dtype=np.int32), np.zeros((nq, 10))

        def still_fine():
            tet[:] = -7
            assert L.wae_locator_find(h, nq, D(X), 0.0, I(tet), D(lam)) == 0
            clear = reference("cube")[2][:64] >= 1e-9
            assert np.array_equal(tet[clear], want[clear])

        still_fine()
        Xn = X.copy()
        Xn[7, 0] = np.nan
        tet[:] = -7
        for code in (L.wae_locator_find(h, -1, D(X), 0.0, I(tet), None), L.wae_locator_find(h, nq, D(Xn), 0.0, I(tet), None),
                     L.wae_locator_find(h, nq, D(X), -1e-9, I(tet), None), L.wae_locator_find(h, nq, D(X), 1.1e-6, I(tet), None),
                     L.wae_locator_find(h, nq, D(X), float("nan"), I(tet), None)):
            refused(code)
        assert np.all(tet == -7)                                            # nothing was written
        assert L.wae_locator_find(h, 0, None, 0.0, None, None) == 0        # nq == 0 touches nothing
        assert L.wae_locator_weights(h, 1, 0, 0, None, None, None, None, None) == 0
        assert L.wae_locator_sample(h, 1, 0, 0, None, None, None, np_, 1, None, None) == 0
        still_fine()
        loc_t = want.copy()
        V = np.zeros((np_, 2), dtype=np.complex128, order="F")
        out = np.zeros((nq, 2), dtype=np.complex128, order="F")
        n3 = np.ones((nq, 3))
        hi_t, lo_t = loc_t.copy(), loc_t.copy()
        hi_t[1], lo_t[2] = nt, -2
        for code in (L.wae_locator_weights(h, 2, 0, nq, D(X), I(loc_t), None, I(idx), D(val)),          # order 2 before set_p2
                     L.wae_locator_weights(h, 1, 0, nq, D(X), I(hi_t), None, I(idx), D(val)),
                     L.wae_locator_weights(h, 1, 0, nq, D(X), I(lo_t), None, I(idx), D(val)),
                     L.wae_locator_weights(h, 1, 0, -1, D(X), I(loc_t), None, I(idx), D(val)),
                     L.wae_locator_weights(h, 1, 0, nq, D(Xn), I(loc_t), None, I(idx), D(val)),
                     L.wae_locator_weights(h, 1, 1, nq, D(X), I(loc_t), None, I(idx), D(val)),          # kind 1 without n
                     L.wae_locator_weights(h, 3, 0, nq, D(X), I(loc_t), None, I(idx), D(val)),
                     L.wae_locator_sample(h, 1, 0, nq, D(X), I(loc_t), None, np_ + 1, 2, D(V), D(out)),
                     L.wae_locator_sample(h, 1, 1, nq, D(X), I(loc_t), None, np_, 2, D(V), D(out)),
                     L.wae_locator_sample(h, 2, 0, nq, D(X), I(loc_t), None, np_, 2, D(V), D(out)),
                     L.wae_locator_sample(h, 1, 0, nq, D(X), I(hi_t), None, np_, 2, D(V), D(out))):
            refused(code)
        t10, ndof = R.nodes_p2(np_, tets)
        t10 = np.ascontiguousarray(t10)
        bad10 = t10.copy()
        bad10[4, 7] = ndof
        refused(L.wae_locator_set_p2(h, ndof, I(bad10)))
        refused(L.wae_locator_set_p2(h, -1, I(t10)))
        refused(L.wae_locator_weights(h, 2, 0, nq, D(X), I(loc_t), None, I(idx), D(val)))              # the refused table was not kept
        assert L.wae_locator_set_p2(h, ndof, I(t10)) == 0
        refused(L.wae_locator_sample(h, 2, 0, nq, D(X), I(loc_t), None, np_, 2, D(V), D(out)))   # d != ndof
        assert L.wae_locator_weights(h, 2, 0, nq, D(X), I(loc_t), None, I(idx), D(val)) == 0
        got = loc_t >= 0
        assert np.array_equal(idx[got], t10[loc_t[got]]) and np.all(idx[~got] == 0) and np.all(val[~got] == 0)
        assert np.max(np.abs(val[got].sum(axis=1) - 1)) <= 64 * EPS
        dims = (C.c_int64 * 3)()
        a, b, c, d = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
        assert L.wae_locator_info(h, C.byref(a), C.byref(b), dims, C.byref(c), C.byref(d)) == 0
        assert (a.value, b.value) == (np_, nt) and min(dims) >= 1 and nt <= c.value <= 32 * nt and 1 <= d.value <= nt
        refused(L.wae_locator_info(None, None, None, None, None, None))
        still_fine()
    finally:
        L.wae_locator_free(h)
