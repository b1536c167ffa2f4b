"""GPU tests (-m gpu) of the nested multigrid set-up: wae_octosplit_prolongator and wae_solver_setup_nested, through
``RefinedMesh.prolongator(s)`` and ``LinearOperatorFamily.solver_prolongators``, with the hierarchy recovered by tests/_hier.py.

Two families, the smallest on which each part can go wrong:
  N -- the sheared Kuhn cube of tests/_octoref.py (27 points) refined three times on the device: 4913 -> 729 -> 125 -> 27 unknowns; M, K, C (top
       face, Y = 1e15: its 289 points are penalty rows) and a flame Q of three tetrahedra, assembled on the device from the carried fields;
       max_coarse = 32: three supplied levels, the last one dense.
  R -- the tutorial Rijke tube refined once (6172 unknowns, assembled as tests/test_gpu_octosplit.py does it), ONE supplied level (1006) and
       max_coarse = 128: smoothed aggregation continues from the supplied level's planes.

Tolerances: transfers and prolongators exact; the Galerkin identity 1e-13 |R||A||P| entrywise (tests/test_gpu_multigrid.py); the coarse
planes against the assembly on the coarser mesh 1e-13 of the largest entry (the project's assembly tolerance; tests/test_nested_args.py
measures 1.3e-14 for the same identity on the oracle); the cycle 16 x max(e64, 1e-13 / 16), unchanged; solves 1e-10 relative residual,
recomputed on the host in extended precision; the eigenvalue 1e-10 relative (tests/test_gpu_octosplit.py)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sp

import _mgref as M
import _octoref as O
import _solveref as S
from _hier import LINE, MASKS, RATIOS, Hier, recover
from oracle import fixtures as F
from oracle import helmholtz_p1 as OH
from oracle import solvers as OS
from test_gpu_multigrid import check_transfers
from wae_amd import _lib
from wae_amd.helmholtz import octosplit
from wae_amd.helmholtz.assemble import assemble_p1, assemble_p1_boundary, assemble_p1_flame
from wae_amd.helmholtz.family import helmholtz_family
from wae_amd.nlevp import householder

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
Z_N = 2 * np.pi * (0.35 + 0.02j)             # the cube has edge 1 and c = 1: its first modes lie at omega ~ pi
# the tube's modes lie at 272 Hz (G1) and near its odd multiples; the line of shifts 440..560 Hz keeps 150 Hz from them, so that the cycle
# comparisons measure the composition of the cycle, not the conditioning of a nearly singular coarse level (a first choice, 280..400 Hz + 2..14i,
# passed 8 Hz from G1: the float64 reference itself moved by 2e-13 there and one light cycle came out at 17.7 units of 16)
Z_R = 2 * np.pi * (500 + 20j)
LINE_N = LINE / 1000.0


# ---- the two families ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mesh_n():
    return octosplit(*O.mesh("sheared"), levels=3)


def terms_n(level):
    """M, K, C, Q on a level of the cube, from the fields carried over from level 0"""
    Rm = mesh_n()
    nt0 = len(Rm.tets[0])
    c0 = 1.0 + 0.1 * np.arange(nt0) / nt0                               # a speed of sound per tetrahedron of level 0
    x_ref = np.array([0.4, 0.3, 0.2, 0.1]) @ Rm.points[0][Rm.tets[0][20]]
    pts, tets, tris = Rm.points[level], Rm.tets[level], Rm.tris[level]
    Mm, K = assemble_p1(pts, tets, Rm.tet_field(c0, level))
    Cm = assemble_p1_boundary(pts, tris, Rm.tri_field(np.ones(len(Rm.tris[0])), level))
    Q, _ = assemble_p1_flame(pts, tets, Rm.tet_domain([5, 6, 7], level), Rm.reference_tet(20, x_ref, level), np.array([0.0, 0.0, 1.0]), 0.5)
    return {"M": Mm, "K": K, "C": Cm, "Q": Q}


def operator_n(**solver_opts):
    L = helmholtz_family(terms_n(3), n=0.01, tau=0.001)
    L.solver_ref = 2 * np.pi * 0.3
    L.solver_opts = {"max_coarse": 32}
    L.solver_opts.update(solver_opts)
    L.solver_prolongators = mesh_n().prolongators()
    return L


@functools.lru_cache(maxsize=None)
def mesh_r():
    return octosplit(*O.mesh("rijke"), levels=1)


@functools.lru_cache(maxsize=None)
def terms_r():
    Rm = mesh_r()
    z = np.load(os.path.join(GOLDEN, "rijke_mesh.npz"))
    fl = np.load(os.path.join(GOLDEN, "rijke_flame.npz"))
    pts, tets, tris = Rm.points[1], Rm.tets[1], Rm.tris[1]
    Mm, K = assemble_p1(pts, tets, Rm.tet_field(z["c_tet"], 1))
    Cm = assemble_p1_boundary(pts, tris, Rm.tri_field(z["outlet_c"], 1))
    Q, _ = assemble_p1_flame(pts, tets, Rm.tet_domain(fl["flame_tets"], 1), Rm.reference_tet(int(fl["ref_tet"]), fl["x_ref"], 1), fl["n_ref"],
                             float(fl["nglobal_scaled"]))
    return {"M": Mm, "K": K, "C": Cm, "Q": Q}


def operator_r(nested=True, **solver_opts):
    L = helmholtz_family(terms_r(), n=0.01, tau=0.001)
    L.solver_ref = 340 * 2 * np.pi
    L.solver_opts = dict(solver_opts)
    if nested:
        L.solver_prolongators = mesh_r().prolongators()
    return L


def drop(H):
    print(f"family {H.name}: largest device error of the cycle comparisons {RATIOS.get(H.name, 0.0):.2f} units of max(e64, 1e-13 / 16); 16 allowed")
    H.L._drop_device()


@pytest.fixture(scope="module")
def fam_n():
    H = Hier("N", operator_n(), (0.8, 0.9, 0.5), 1, Z_N, Z_N + LINE_N, distinct=16)
    yield H
    drop(H)


@pytest.fixture(scope="module")
def fam_r():
    H = Hier("R", operator_r(), (0.8, 0.9, 0.5), 1, Z_R, Z_R + LINE, distinct=16)
    yield H
    drop(H)


def supplied(H):
    return mesh_n().prolongators() if H.name == "N" else mesh_r().prolongators()


def match_columns(Prec, Pexp):
    """q with Prec[:, q[c]] == Pexp[:, c], entry for entry (rows and values exact); every column of either matrix is used once"""
    A, B = sp.csc_matrix(Prec), sp.csc_matrix(Pexp)
    A.sort_indices(); B.sort_indices()
    assert A.shape == B.shape
    key = lambda X, c: (X.indices[X.indptr[c]:X.indptr[c + 1]].tobytes(), X.data[X.indptr[c]:X.indptr[c + 1]].tobytes())
    table = {key(A, c): c for c in range(A.shape[1])}
    assert len(table) == A.shape[1], "two equal columns"
    q = np.array([table.get(key(B, c), -1) for c in range(B.shape[1])])
    assert np.all(q >= 0), f"{int(np.sum(q < 0))} columns of the caller's prolongator are not among the stored ones"
    assert len(set(q.tolist())) == len(q)
    return q


def column_maps(H):
    """per supplied level l: q_l, the internal number of the caller's unknown c of level l + 1; asserts the transfers while finding them"""
    qs, rowmap = [], None
    for l, P in enumerate(supplied(H)):
        P = sp.csr_matrix(P)
        if l == 0:
            P = sp.diags((~H.pen).astype(float)) @ P                        # the penalty rows are emptied
            P.eliminate_zeros()
        else:
            P = sp.csr_matrix((P.data, P.indices, P.indptr), shape=P.shape)[np.argsort(rowmap)]     # row q[c] of the stored matrix is the caller's c
        rec = H.Pm[l].real.tocsr()
        assert set(np.unique(rec.data)) <= {0.5, 1.0}
        q = match_columns(rec, P)
        # the permutation read off the rows with a single entry 1
        rows = np.nonzero((np.diff(rec.indptr) == 1) & (rec.data[np.minimum(rec.indptr[:-1], rec.nnz - 1)] == 1.0))[0]
        Pc = P.tocsr()
        for i in rows[::max(1, len(rows) // 200)]:
            assert Pc.indptr[i + 1] - Pc.indptr[i] == 1 and q[Pc.indices[Pc.indptr[i]]] == rec.indices[rec.indptr[i]]
        qs.append(q)
        rowmap = q
    return qs


# ---- 1. the prolongator of a refinement step ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["two", "sheared", "rijke"])
def test_device_prolongator_equals_the_host_form(name):
    Rd = octosplit(*O.mesh(name), levels=2)
    H = O.refine(*O.mesh(name), levels=2)
    for frm in (0, 1):
        P = Rd.prolongator(frm)
        h, Rd._h = Rd._h, None                                              # the same object without its handle: the host form
        try:
            Ph = Rd.prolongator(frm)
        finally:
            Rd._h = h
        for f in ("indptr", "indices", "data"):
            assert np.array_equal(getattr(P, f), getattr(Ph, f)) and getattr(P, f).dtype == getattr(Ph, f).dtype, (name, frm, f)
        X = np.random.default_rng(frm).standard_normal((len(H[frm].points), 3))
        assert np.array_equal(P @ X, O.prolong(H, X, frm, frm + 1))
    L = _lib.lib()
    n1 = len(H[1].points)
    ptr, col, val = np.zeros(n1 + 1, dtype=np.int32), np.zeros(2 * n1, dtype=np.int32), np.zeros(2 * n1)
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    for lvl in (-1, 2, 3):
        assert L.wae_octosplit_prolongator(Rd._h, lvl, ptr.ctypes.data_as(ip), col.ctypes.data_as(ip), val.ctypes.data_as(dp)) == _lib.WAE_ERR_INVALID
    assert L.wae_octosplit_prolongator(Rd._h, 0, None, col.ctypes.data_as(ip), val.ctypes.data_as(dp)) == _lib.WAE_ERR_INVALID


# ---- 2, 3. the stored hierarchy -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fx", ["fam_n", "fam_r"])
def test_transfers_levels_and_galerkin_identity(fx, request):
    H = request.getfixturevalue(fx)
    print(f"family {H.name}: levels {H.n} (the last one dense), {int(H.pen.sum())} penalty rows, {H.fam.T} terms")
    if H.name == "N":
        assert H.n == [4913, 729, 125, 27] and int(H.pen.sum()) == 289
    else:
        assert H.n[:2] == [6172, 1006] and np.all(np.diff(H.n) < 0) and H.n[-1] <= 128 and H.nl >= 3 and int(H.pen.sum()) == 83
    for l in range(H.nl - 1):
        Rm, Pm = H.Rm[l], H.Pm[l]
        assert np.all(Rm.data.imag == 0) and np.all(Pm.data.imag == 0)
        assert Rm.shape == (H.n[l + 1], H.n[l]) and Pm.shape == (H.n[l], H.n[l + 1])
        D = (Rm - Pm.T).tocsr()
        assert D.nnz == 0 or np.all(D.data == 0), (l, "R is not the transpose of P, bit for bit")
        assert Rm.nnz == Pm.nnz and np.all(np.diff(Rm.indptr) > 0), (l, "an empty column")
    assert np.all(np.diff(H.Pm[0].indptr)[H.pen] == 0), "a penalty row is interpolated"
    assert np.all(np.diff(H.Pm[0].indptr)[~H.pen] > 0), "a row that is no penalty row is not interpolated"
    qs = column_maps(H)
    assert len(qs) == (3 if H.name == "N" else 1)
    worst = 0.0
    for l in range(1, H.nl - 1):
        for k in range(H.fam.T):
            G, bound = H.gal[(l, k)]
            A = np.asarray(H.terms[l][k].todense())
            assert not np.any((A != 0) & (bound == 0)), (l, k, "a stored entry where R A P has none")
            q = np.abs(A - G)[bound > 0] / bound[bound > 0]
            worst = max(worst, float(np.max(q)) if q.size else 0.0)
            assert np.all(np.abs(A - G) <= 1e-13 * bound), (l, k, float(np.max(q)))
    print(f"family {H.name}: Galerkin identity, largest |A - R A P| / |R||A||P| = {worst:.2e}")
    if H.name == "N":
        # level 1 is the mesh's level 2: away from the penalty points, M and K are what the device assembles there
        coarse = terms_n(2)
        q, free = qs[0], ~H.pen[:729]                                       # (old points keep their numbers; the top face of level 2)
        assert free.sum() == 729 - 81
        for name in ("M", "K"):
            k = next(i for i, t in enumerate(H.L.terms) if t.operator == name)
            A = H.terms[1][k].tocsr()[q][:, q][free][:, free].toarray()
            B = sp.csr_matrix(coarse[name])[free][:, free].toarray()
            err, scale = np.max(np.abs(A - B)), np.max(np.abs(B))
            print(f"N level 1, {name}: max|P^T A P - assembled| = {err:.3e} = {err / scale:.3e} * max|entry|")
            assert np.array_equal(A != 0, B != 0) and err <= 1e-13 * scale, name


def test_two_setups_give_identical_bits(fam_n):
    H = fam_n
    L2 = operator_n()
    try:
        fam2 = L2.ensure_solver()
        for l in range(H.nl - 1):
            for which, mine in ((1, H.Rm[l]), (2, H.Pm[l])):
                ni, no = (H.n[l], H.n[l + 1]) if which == 1 else (H.n[l + 1], H.n[l])
                other = recover(fam2, which, l, ni, no)
                assert (other != mine).nnz == 0 and np.array_equal(other.tocsr().data, mine.tocsr().data), (l, which)
        for l in range(1, H.nl - 1):
            for k in range(H.fam.T):
                other, mine = recover(fam2, 0, l, H.n[l], H.n[l], k).tocsr(), H.terms[l][k].tocsr()
                assert np.array_equal(other.indptr, mine.indptr) and np.array_equal(other.indices, mine.indices), (l, k)
                assert np.array_equal(other.data.view(np.uint64), mine.data.view(np.uint64)), (l, k)
        B = H.B[0][:, :5]
        assert np.array_equal(fam2.debug_vcycle(H.ct1, B), H.fam.debug_vcycle(H.ct1, B))       # (the dense level included)
    finally:
        L2._drop_device()


# ---- 5. the cycle ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("light", [False, True], ids=["full", "light"])
@pytest.mark.parametrize("percol", [False, True], ids=["one_system", "per_column"])
@pytest.mark.parametrize("op", ["N", "T", "C"])
@pytest.mark.parametrize("fx", ["fam_n", "fam_r"])
def test_cycle_from_every_level(fx, op, percol, light, request):
    H = request.getfixturevalue(fx)
    for level in range(H.nl - 2, -1, -1):
        for r in (64, 21):
            H.check_cycle(level, op, percol, light, r, final_out=(r == 21))
            H.check_cycle(level, op, percol, light, r, final_out=(r == 64), masked=True)
    for r in (64, 21):
        H.check_cycle(0, op, percol, light, r, fused=True, final_out=(r == 64))
        H.check_cycle(0, op, percol, light, r, fused=True, masked=True)


@pytest.mark.parametrize("fx", ["fam_n", "fam_r"])
def test_transfers_in_tile_and_csr_form(fx, request):
    """where the fine level has a tile plan the transfers of level 0 take the tile kernels from 8 columns on: both storage forms"""
    H = request.getfixturevalue(fx)
    for r in (8, 64):
        for no_tiles in (False, True):
            check_transfers(H, 0, r, no_tiles=no_tiles)
            check_transfers(H, 1, r, no_tiles=no_tiles)
    check_transfers(H, 0, 64, cmask=MASKS[64])


# ---- 6. solves -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fx", ["fam_n", "fam_r"])
def test_solve_converges(fx, request):
    """wae_solve stops on the residual of the left-preconditioned system, ||M^-1 (b - A x)|| / ||M^-1 b|| (tests/_solveref.py states the
    driver's rules): that is the residual recomputed here, in extended precision, with the V-cycle of tests/_mgref.py on the recovered
    hierarchy.  The plain residual ||b - A x|| / ||b|| is printed beside it; it is not what the tolerance bounds.  MI355X: preconditioned
    2.3e-11..5.2e-11 (N, 21 iterations) and 4.0e-11..5.2e-11 (R, 34 iterations); plain 0.9e-10..3.2e-10 and 3.7e-10..7.9e-10."""
    H = request.getfixturevalue(fx)
    B = H.B[0][:, :8]
    X = H.fam.solve(H.ct1, B, tol=1e-10, maxit=300, strict=False, quiet=True)
    info, code = dict(H.fam.last_info), H.fam.last_code
    rho = np.asarray(S.SolveRef(H.levels, H.transfers, "N", H.w, H.nsweeps).rho(X, B, H.ct1), dtype=np.float64)
    res = B.astype(M.LD) - H.levels[0].apply(H.ct1, "N", X, M.LD)
    plain = np.array([float(np.linalg.norm(res[:, j]) / np.linalg.norm(B[:, j].astype(M.LD))) for j in range(8)])
    print(f"family {H.name}: solve of 8 columns at tol 1e-10: code {code}, info {info}, recomputed preconditioned residuals {rho.min():.2e}.."
          f"{rho.max():.2e}, plain residuals {plain.min():.2e}..{plain.max():.2e}")
    assert code == 0 and info["n_unconverged"] == 0 and info["levels"] == H.nl
    assert np.all(rho <= 1e-10), rho


def test_truncated_solve_is_the_least_squares_minimum():
    """family N on a handle of batch 16 / restart 6, as tests/test_gpu_solve_driver.py holds its families to tests/_solveref.py"""
    H = Hier("N", operator_n(batch=S.NB_SMALL, restart=S.RESTART_SMALL), (0.8, 0.9, 0.5), 1, Z_N, Z_N + LINE_N, distinct=S.DISTINCT)
    try:
        Ct = S.Contract(H.levels, H.transfers, H.w, H.nsweeps, H.B[0][:, :S.DISTINCT].copy(), H.ct64[:S.DISTINCT].copy(), H.ct1.copy(), nlevels=H.nl)
        r, k = 8, 3
        B, ct = Ct.columns(r, False)
        X = H.fam.solve(ct, B, tol=1e-300, maxit=k, strict=False, quiet=True)
        Ct.check_truncated(X, dict(H.fam.last_info), H.fam.last_code, r, k, False, "N", S.NB_SMALL, S.RESTART_SMALL)
    finally:
        H.L._drop_device()


# ---- 7. end to end on the Rijke tube ---------------------------------------------------------------------------------------------------------
def test_rijke_tube_refined_once_with_the_nested_setup():
    Rm, Href = mesh_r(), O.refine(*O.mesh("rijke"), levels=1)
    z = np.load(os.path.join(GOLDEN, "rijke_mesh.npz"))
    fl = np.load(os.path.join(GOLDEN, "rijke_flame.npz"))
    w_G1 = complex(*F.golden()["G1"]["omega"])
    L0 = helmholtz_family(F.rijke_terms(), n=0.01, tau=0.001)
    L0.solver_ref = 340 * 2 * np.pi
    sol0, _, flag0 = householder(L0, 340 * 2 * np.pi, maxiter=20, tol=1e-11)
    L0._drop_device()
    assert flag0 in (0, 1) and abs(sol0.params["ω"] - w_G1) < 1e-10 * abs(w_G1)
    L1 = operator_r()
    sol1, n1, flag1 = householder(L1, w_G1, v0=Rm.prolong(sol0.v, 0, 1), v0_adj=Rm.prolong(sol0.v_adj, 0, 1), maxiter=20, tol=1e-11)
    L1._drop_device()
    # the oracle on the reference's refined arrays
    m = OH.Mesh()
    m.points, m.tetrahedra, m.triangles = Href[1].points, Href[1].tets.astype(np.int64), Href[1].tris.astype(np.int64)
    flame = O.carry_domain(Href, fl["flame_tets"], "tet", 1)
    m.domains = {"Interior": {"dimension": 3, "simplices": list(range(len(Href[1].tets)))},
                 "Outlet": {"dimension": 2, "simplices": list(range(len(Href[1].tris)))},
                 "Flame": {"dimension": 3, "simplices": [int(i) for i in flame]}}
    dscrp = {"Interior": ("interior", ()), "Outlet": ("admittance", ("Y", 1e15)),
             "Flame": ("flame", (2.0, 1.0, float(fl["nglobal_scaled"]), list(fl["x_ref"]), list(fl["n_ref"]), "n", "τ", 0.01, 0.001))}
    Lo = OH.discretize_p1(m, dscrp, np.asarray(O.carry_field(Href, z["c_tet"], "tet", 1), dtype=float))
    solo, no, _ = OS.inveriter(Lo, w_G1, maxiter=40, tol=1e-9)
    w1, wo = sol1.params["ω"], solo.params["ω"]
    print(f"refined Rijke tube, nested set-up: device householder {w1 / (2 * np.pi):.8f} Hz in {n1} steps (flag {flag1}), oracle "
          f"inveriter {wo / (2 * np.pi):.8f} Hz in {no} steps, relative difference {abs(w1 - wo) / abs(wo):.2e}")
    assert flag1 in (0, 1) and no < 40
    assert abs(w1 - wo) < 1e-10 * abs(wo)
    assert abs(w1 - w_G1) < 1e-2 * abs(w_G1)


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable(fam_r):
    H = fam_r
    fam, d = H.fam, H.n[0]
    P0 = sp.csr_matrix(mesh_r().prolongator(0))
    c = np.ascontiguousarray(H.L.coefficients(H.L.solver_ref), dtype=np.complex128)      # the coefficients the fixture was set up with
    L = _lib.lib()
    i32p, i64p, dp = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double)

    def call(mats, nlev=None, rows=None):
        n = len(mats)
        keep = [(np.ascontiguousarray(ptr, dtype=np.int32), np.ascontiguousarray(col, dtype=np.int32), np.ascontiguousarray(val, dtype=np.float64))
                for ptr, col, val, _ in mats]
        arr = [(C.c_void_p * max(n, 1))(*[k[j].ctypes.data for k in keep]) for j in range(3)]
        rws = (C.c_int64 * max(n, 1))(*(rows if rows is not None else [m[3][0] for m in mats]))
        cls = (C.c_int64 * max(n, 1))(*[m[3][1] for m in mats])
        return L.wae_solver_setup_nested(fam.handle, _lib.zptr(c), None, 0, n if nlev is None else nlev, rws, cls, arr[0], arr[1], arr[2])

    def still_solves():
        B = H.B[0][:, :2]
        X = fam.solve(H.ct1, B, tol=1e-10, maxit=300, strict=False, quiet=True)
        assert fam.last_code == 0 and fam.last_info["levels"] == H.nl and fam.last_info["n_unconverged"] == 0
        rho = np.asarray(S.SolveRef(H.levels, H.transfers, "N", H.w, H.nsweeps).rho(X, B, H.ct1), dtype=np.float64)
        assert np.all(rho <= 1e-10), rho

    good = (P0.indptr, P0.indices, P0.data, P0.shape)
    tail = sp.random(1006, 100, density=0.02, format="csr", random_state=1)
    tail_t = (tail.indptr, tail.indices, tail.data, tail.shape)
    swapped = P0.indices.copy()
    a = P0.indptr[d - 1]
    swapped[a], swapped[a + 1] = swapped[a + 1], swapped[a]                 # the last row: its two parents descending
    dup = P0.indices.copy()
    dup[a + 1] = dup[a]
    big = P0.indices.copy()
    big[5] = 1006
    neg = P0.indices.copy()
    neg[5] = -1
    nan, inf = P0.data.copy(), P0.data.copy()
    nan[7], inf[7] = np.nan, np.inf
    cases = {
        "nlev = 0": lambda: call([good], nlev=0),
        "nlev < 0": lambda: call([good], nlev=-1),
        "P_0 with other than d rows": lambda: call([(P0.indptr[:-1], P0.indices, P0.data, (d - 1, 1006))]),
        "dimensions that do not chain": lambda: call([good, tail_t], rows=[d, 1005]),
        "a column out of range": lambda: call([(P0.indptr, big, P0.data, P0.shape)]),
        "a negative column": lambda: call([(P0.indptr, neg, P0.data, P0.shape)]),
        "unsorted columns": lambda: call([(P0.indptr, swapped, P0.data, P0.shape)]),
        "duplicate columns": lambda: call([(P0.indptr, dup, P0.data, P0.shape)]),
        "a NaN": lambda: call([(P0.indptr, P0.indices, nan, P0.shape)]),
        "an infinity": lambda: call([(P0.indptr, P0.indices, inf, P0.shape)]),
    }
    for what, f in cases.items():
        code = f()
        msg = L.wae_last_error().decode(errors="replace")
        assert code == _lib.WAE_ERR_INVALID and "nested set-up" in msg, (what, code, msg)
        print(f"{what}: {msg}")
    still_solves()
    # a column without entries (here: inserted at 500) is dropped from its level: the hierarchy of the fixture again
    sizes0 = fam.level_sizes()
    Pext = sp.csr_matrix((P0.data, P0.indices + (P0.indices >= 500), P0.indptr), shape=(d, 1007))
    fam.setup_solver(c, prolongators=[Pext])
    assert fam.level_sizes() == sizes0
    for l in range(H.nl - 1):
        assert (recover(fam, 1, l, H.n[l], H.n[l + 1]) != H.Rm[l]).nnz == 0, l
    still_solves()
    # a family set up nested, then again by smoothed aggregation: the hierarchy of a fresh handle
    fam.setup_solver(c)
    Lf = operator_r(nested=False)
    try:
        Lf.solver_ref_coeffs = c
        fresh = Lf.ensure_solver()
        sizes = fam.level_sizes()
        assert sizes == fresh.level_sizes() and [s for s in sizes if s[0] == 1][0][3] != 1006
        for which, lv, ni, no in sizes:
            if which == 1:
                assert (recover(fam, 1, lv, ni, no) != recover(fresh, 1, lv, ni, no)).nnz == 0, lv
        for lv in range(1, len([s for s in sizes if s[0] == 0])):
            n = [s for s in sizes if s[0] == 0][lv][2]
            for k in range(fam.T):
                assert (recover(fam, 0, lv, n, n, k) != recover(fresh, 0, lv, n, n, k)).nnz == 0, (lv, k)
    finally:
        Lf._drop_device()
        fam.setup_solver(c, prolongators=mesh_r().prolongators())          # the fixture's hierarchy again
    still_solves()
