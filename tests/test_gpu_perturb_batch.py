"""GPU tests (-m gpu) of the batched adjoint perturbation recurrence: wae_perturb_batch / wae_perturb_batch_slots (include/waehip.h),
``DeviceFamily.perturb_batch`` and ``perturb_many`` -- nsys eigenpairs expanded in lock-step by one library call -- against the CPU
oracle and the reference's recorded outputs; the single-pair calls wae_perturb / wae_perturb_slots run the same recurrence at nsys = 1
and are held to returning exactly what the batched call returns for one pair.

Tolerances: those the single-pair path is held to (tests/test_gpu_parity.py: test_perturb_device_call_all_modes, test_G1_..., test_G4_G6_...;
tests/test_gpu_fullsize.py: test_c5_adjoint_perturbation_order_30_half_million_dof)."""
import warnings

import numpy as np
import pytest

from oracle import fixtures as F
from oracle import solvers as OS
from wae_amd import _lib
from wae_amd.helmholtz.family import annulus_family, helmholtz_family
from wae_amd.nlevp import conv_radius, householder, householder_many, mslp, perturb_many
from wae_amd.nlevp import perturbation as P
from wae_amd.nlevp.linopfam import UnconvergedWarning

pytestmark = pytest.mark.gpu
G = F.golden()
c = lambda p: complex(p[0], p[1])
RNG = np.random.default_rng(11)


def test_perturb_many_matches_the_oracle_for_all_three_kinds():
    """Rijke family, the three eigenpairs of test_householder_many_matches_single_runs, N = 6: every lambda_k of every pair within 1e-7
    relative of the oracle's perturb_ / perturb_fast_ / perturb_norm_ on the same base state, v_1..v_3 within 1e-5 up to the phase of v_0."""
    Lo = F.rijke_family(n=0.01, tau=0.001)
    Lp = helmholtz_family(F.rijke_terms(), n=0.01, tau=0.001)
    Lp.solver_ref = 2 * np.pi * 400.0
    starts = [2 * np.pi * 340.0, 2 * np.pi * 700.0, 2 * np.pi * 250.0]
    sols = [s for s, _, _ in householder_many(Lp, starts, maxiter=20, tol=1e-11)]
    osols = [OS.householder(Lo, z0, maxiter=20, tol=1e-11)[0] for z0 in starts]
    for sp_, so in zip(sols, osols):
        assert abs(sp_.params["ω"] - so.params["ω"]) < 1e-10 * abs(so.params["ω"])
    N = 6
    for kind, fo in (("plain", OS.perturb_), ("fast", OS.perturb_fast_), ("norm", OS.perturb_norm_)):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UnconvergedWarning)
            status = perturb_many(sols, Lp, "τ", N, kind=kind)
        print(kind, "status", list(status), Lp.device().last_info)
        if kind != "norm":          # (kind "norm": the left vector has passed through a solve with Y to 1e-12, so the right-hand sides are
            #                          consistent with the singular L(0,0) to ~1e-11 only and a solve may end there: reported, not wrong)
            assert list(status) == [0, 0, 0] and Lp.device().last_info["n_unconverged"] == 0
        for j, (sp_, so) in enumerate(zip(sols, osols)):
            fo(so, Lo, "τ", N)
            lo, lp = so.eigval_pert["τ/Taylor"], sp_.eigval_pert["τ/Taylor"]
            assert len(lp) == N + 1 and lp[0] == sp_.params["ω"]
            for k in range(1, N + 1):
                print(kind, j, k, abs(lp[k] - lo[k]) / abs(lo[k]))
                assert abs(lp[k] - lo[k]) < 1e-7 * abs(lo[k]), (kind, j, k, lp[k], lo[k])
            vo, vp = so.v_pert["τ/Taylor"], sp_.v_pert["τ/Taylor"]
            assert len(vp) == N + 1
            ph = np.vdot(vo[0], vp[0]) / abs(np.vdot(vo[0], vp[0]))
            for k in range(1, 4):
                assert np.linalg.norm(vp[k] - ph * vo[k]) < 1e-5 * np.linalg.norm(vo[k]), (kind, j, k)
    Lp._drop_device()


def test_two_parameter_points_in_one_batch_match_the_recorded_reference_outputs():
    """Column 0: the G1 state (n = 0.01, householder to 1e-11); column 1: the G5 state (n = 1.0, mslp to 1e-11); ONE family and ONE
    multigrid hierarchy (built at n = 0.01), both at solver_tol = 1e-13, expanded together to N = 30 (kind "fast").  Column 0's first 21
    coefficients against G2.taylor (1e-8 relative), column 1's convergence-radius table against G4.conv_radius (1e-7) and its order-30
    estimate at tau + 5e-4 (1e-7 absolute): the tolerances of the single-pair tests."""
    Lp = helmholtz_family(F.rijke_terms(), n=0.01, tau=0.001)
    Lp.solver_ref = 340 * 2 * np.pi
    Lp.solver_tol = 1e-13
    sol0, _, _ = householder(Lp, 340 * 2 * np.pi, maxiter=20, tol=1e-11)
    assert abs(sol0.params["ω"] - c(G["G1"]["omega"])) < 1e-10 * abs(c(G["G1"]["omega"]))
    Lp.params["n"] = complex(1.0)
    sol1, _, _ = mslp(Lp, 340 * 2 * np.pi, maxiter=20, tol=1e-11)
    assert abs(sol1.params["ω"] - c(G["G5"]["omega"])) < 1e-10 * abs(c(G["G5"]["omega"]))
    assert sol0.params["n"] != sol1.params["n"]
    before = (Lp.params, Lp.active, Lp.mode, dict(Lp.params))
    status = perturb_many([sol0, sol1], Lp, "τ", 30, kind="fast")
    info = Lp.device().last_info
    assert info["n_unconverged"] == 0 and list(status) == [0, 0]
    assert Lp.params is before[0] and Lp.active is before[1] and Lp.mode == before[2] and dict(Lp.params) == before[3]
    lam0, lam1 = sol0.eigval_pert["τ/Taylor"], sol1.eigval_pert["τ/Taylor"]
    assert len(lam0) == 31 and len(lam1) == 31 and len(sol1.v_pert["τ/Taylor"]) == 31
    for k, ref in enumerate(G["G2"]["taylor"]):
        print("G2", k, abs(lam0[k] - c(ref)) / abs(c(ref)))
        assert abs(lam0[k] - c(ref)) < 1e-8 * abs(c(ref)), (k, lam0[k], c(ref))
    r = conv_radius(lam1)
    ref = np.array(G["G4"]["conv_radius"])
    assert len(r) == len(ref) == 30
    print("G4 conv radius", np.max(np.abs(r - ref) / ref))
    assert np.max(np.abs(r - ref) / ref) < 1e-7, np.max(np.abs(r - ref) / ref)
    est30 = sol1("τ", 0.0015, 30) / 2 / np.pi
    assert abs(est30 - c(G["G4"]["taylor30_estimate_over_2pi_at_tau_plus_5e-4"])) < 1e-7
    Lp._drop_device()


@pytest.fixture(scope="module")
def small():
    """small annulus (8 736 DoF, multi-level hierarchy): the two simple modes near 195 and 735 Hz at two delays each -- four distinct
    eigenpairs at two parameter points (the other modes of the annulus come in near-degenerate pairs)."""
    L, pb = annulus_family("small", tau=2e-4)
    L.solver_tol = 1e-12
    L.solver_ref = 2 * np.pi * 500.0
    sols = []
    for tau in (2e-4, 2.2e-4):
        L.params["τ"] = complex(tau)
        for z0 in (2 * np.pi * (195 + 9j), 2 * np.pi * (735 + 3j)):
            s, n, flag = householder(L, z0, maxiter=15, tol=1e-11)
            assert abs(s.history[-1] - s.history[-2]) < 1e-9 * abs(s.params["ω"]), (tau, z0, s.history)
            sols.append(s)
    L.params["τ"] = complex(2e-4)
    tables = P.solution_tables(sols, L, "τ", 4)
    yield L, pb, sols, tables
    L._drop_device()


@pytest.fixture(scope="module")
def oracle_series(small):
    """The CPU oracle's perturb_disk (norm_mode 1; one sparse LU of L(0,0) each) for the four pairs of `small`, N = 4, on
    Lhost(m, n) = sum_t tables[i][m, n, t] A_t assembled from the scipy term matrices (the family's term order: M, K, C, Q, -M)."""
    L, pb, sols, tables = small
    t = pb["terms"]
    mats = [t["M"].tocsr(), t["K"].tocsr(), t["C"].tocsr(), t["Q"].tocsr(), (-t["M"]).tocsr()]
    refs = []
    for sol, table in zip(sols, tables):
        assert table.shape[2] == len(mats)
        cache = {}

        def Lhost(m, n, table=table, cache=cache):
            if (m, n) not in cache:
                cache[(m, n)] = sum(table[m, n, k] * A for k, A in enumerate(mats)).tocsr()
            return cache[(m, n)]

        lam, v = OS.perturb_disk(Lhost, 4, sol.v, sol.v_adj)
        refs.append((lam, np.stack(v, axis=1)))
    return refs


@pytest.mark.parametrize("nsys", [1, 3, 8, 9])
def test_every_column_matches_the_cpu_oracle(small, oracle_series, nsys):
    """nsys = 1, 3, 8, 9 (9 crosses an 8-column chunk; pairs repeat, rescaled, beyond the four the fixture has): every column's lambda
    within 1e-7 relative of the CPU oracle's perturb_disk for that pair, v_1 within 1e-5 up to the phase of v_0; norm_mode + 16 returns
    the same lambda and leaves v_out untouched; the slot-column form agrees with the host-vector form."""
    L, pb, sols, tables = small
    fam = L.ensure_solver()
    N = 4
    idx = [j % len(sols) for j in range(nsys)]
    scale = [(1.0 + 0.5 * (j // len(sols))) * np.exp(0.3j * j) for j in range(nsys)]
    V0 = np.stack([scale[j] * sols[i].v for j, i in enumerate(idx)], axis=1)
    W0 = np.stack([np.conj(scale[j]) * sols[i].v_adj for j, i in enumerate(idx)], axis=1)
    tabs = np.stack([tables[i] for i in idx])
    lam, V, status = fam.perturb_batch(tabs, N, V0, W0, norm_mode=1, tol=L.solver_tol, maxit=L.solver_maxit)
    assert list(status) == [0] * nsys and fam.last_info["n_unconverged"] == 0
    assert V.shape == (nsys, pb["d"], N + 1) and np.all(np.isfinite(V)) and np.all(np.isfinite(lam))
    for j, i in enumerate(idx):
        ls, Vs = oracle_series[i]
        for k in range(1, N + 1):
            print(nsys, j, k, abs(lam[j, k] - ls[k]) / abs(ls[k]))
            assert abs(lam[j, k] - ls[k]) < 1e-7 * abs(ls[k]), (nsys, j, k, lam[j, k], ls[k])
        ph = np.vdot(Vs[:, 0], V[j][:, 0]) / abs(np.vdot(Vs[:, 0], V[j][:, 0]))
        print(nsys, j, "v1", np.linalg.norm(V[j][:, 1] - ph * Vs[:, 1]) / np.linalg.norm(Vs[:, 1]))
        assert np.linalg.norm(V[j][:, 1] - ph * Vs[:, 1]) < 1e-5 * np.linalg.norm(Vs[:, 1])
    # eigenvalue series only: same lambda, v_out untouched
    lib = _lib.lib()
    lam16 = np.zeros((nsys, N + 1), dtype=np.complex128)
    sentinel = complex(7.0, -3.0)
    Vbuf = np.full((nsys, N + 1, pb["d"]), sentinel, dtype=np.complex128)
    st16 = np.zeros(nsys, dtype=np.int32)
    info = _lib.SolveInfo()
    V0f, W0f = np.asfortranarray(V0), np.asfortranarray(W0)
    import ctypes as C
    code = lib.wae_perturb_batch(fam.handle, nsys, _lib.zptr(np.ascontiguousarray(tabs)), N, _lib.zptr(V0f), _lib.zptr(W0f), 1 + 16, None,
                                 L.solver_tol, L.solver_maxit, _lib.zptr(lam16), _lib.zptr(Vbuf), st16.ctypes.data_as(C.POINTER(C.c_int32)),
                                 C.byref(info))
    assert code == _lib.WAE_OK and np.all(Vbuf == sentinel)
    assert np.max(np.abs(lam16[:, 1:] - lam[:, 1:]) / np.abs(lam[:, 1:])) < 1e-9
    # slot columns (deliberately not consecutive) == host vectors
    order = list(range(nsys))[::-1]
    fam.slot_write(2, V0[:, order])
    fam.slot_write(3, W0[:, order])
    cols = [order.index(j) for j in range(nsys)]
    lam_s, V_s, st_s = fam.perturb_batch(tabs, N, slots=(2, cols, 3, cols), norm_mode=1, tol=L.solver_tol, maxit=L.solver_maxit)
    assert list(st_s) == [0] * nsys
    assert np.max(np.abs(lam_s[:, 1:] - lam[:, 1:]) / np.abs(lam[:, 1:])) < 1e-9
    assert np.max(np.abs(V_s - V)) <= 1e-8 * np.max(np.abs(V))
    fam.slot_write(2, ncols_total=1)
    fam.slot_write(3, ncols_total=1)


@pytest.mark.parametrize("norm_mode", [0, 1, 2])
def test_single_pair_calls_return_what_the_batched_call_returns_for_one_pair(small, oracle_series, norm_mode):
    """wae_perturb and wae_perturb_slots are the batched recurrence at nsys = 1: on one pair of `small`, N = 4, norm_mode 0, 1, 2,
    perturb, perturb_slots(vectors=True) and perturb_batch with one system return the same lambda and the same vectors, and with
    norm_mode + 16 perturb returns the same lambda and v_0..v_{N-1} of the full call (column N is left as the caller passed it).
    "Same" is bitwise: the three calls run the same launches on the same data, and the kernels under them reduce in a fixed order
    (whether repeated perturb_batch calls of the library before the fold are bitwise equal on this fixture has NOT been measured yet;
    if they are not, the bound here becomes 4 x the largest repeat-to-repeat difference).  At norm_mode 1 the single-pair call is also
    held to the oracle bounds of test_every_column_matches_the_cpu_oracle."""
    L, pb, sols, tables = small
    fam = L.ensure_solver()
    N = 4
    sol, table = sols[1], tables[1]
    cY = L.term_operator(len(L.terms) - 1, -1.0).coeffs if norm_mode == 2 else None
    kw = dict(norm_mode=norm_mode, coeffsY=cY, tol=L.solver_tol, maxit=L.solver_maxit, quiet=True)
    lam_b, V_b, st_b = fam.perturb_batch(table[None], N, sol.v[:, None], sol.v_adj[:, None], **kw)
    lam_s, V_s = fam.perturb(table, N, sol.v, sol.v_adj, **kw)
    assert np.all(np.isfinite(lam_s)) and np.all(np.isfinite(V_s))
    assert np.array_equal(lam_s[1:], lam_b[0, 1:]) and np.array_equal(V_s, V_b[0])
    fam.slot_write(2, np.stack([sol.v_adj, sol.v], axis=1))
    lam_t, V_t = fam.perturb_slots(table, N, 2, 1, 2, 0, vectors=True, **kw)
    fam.slot_write(2, ncols_total=1)
    assert np.array_equal(lam_t[1:], lam_b[0, 1:]) and np.array_equal(V_t, V_b[0])
    kw["norm_mode"] = norm_mode + 16
    lam_e, V_e = fam.perturb(table, N, sol.v, sol.v_adj, **kw)
    assert np.array_equal(lam_e[1:], lam_b[0, 1:]) and np.array_equal(V_e[:, :N], V_b[0][:, :N]) and np.all(V_e[:, N] == 0)
    if norm_mode == 1:
        ls, Vs = oracle_series[1]
        for k in range(1, N + 1):
            print("single", k, abs(lam_s[k] - ls[k]) / abs(ls[k]))
            assert abs(lam_s[k] - ls[k]) < 1e-7 * abs(ls[k]), (k, lam_s[k], ls[k])
        ph = np.vdot(Vs[:, 0], V_s[:, 0]) / abs(np.vdot(Vs[:, 0], V_s[:, 0]))
        print("single v1", np.linalg.norm(V_s[:, 1] - ph * Vs[:, 1]) / np.linalg.norm(Vs[:, 1]))
        assert np.linalg.norm(V_s[:, 1] - ph * Vs[:, 1]) < 1e-5 * np.linalg.norm(Vs[:, 1])


def test_one_failing_system_is_reported_and_does_not_touch_the_others(small):
    """Three good pairs and, in column 1, a system that cannot be solved: the coefficient table of a true eigenpair -- L(0,0) singular
    -- with random right and left vectors, so that the right-hand side of every order has a component outside the range of L(0,0)
    and no iteration count reaches tol.  With maxit just above what the good columns need, that system is reported in status_out, the
    call returns WAE_WARN_MAXITER, the other columns equal the clean batch, and nothing is NaN.  Bad arguments are rejected on the host."""
    L, pb, sols, tables = small
    fam = L.ensure_solver()
    d = pb["d"]
    N = 3
    tabs4 = P.solution_tables(sols[:3], L, "τ", N)
    V0 = np.stack([s.v for s in sols[:3]], axis=1)
    W0 = np.stack([s.v_adj for s in sols[:3]], axis=1)
    lam_c, V_c, st_c = fam.perturb_batch(np.stack(tabs4), N, V0, W0, norm_mode=1, tol=L.solver_tol, maxit=L.solver_maxit)
    assert list(st_c) == [0, 0, 0]
    m_good = fam.last_info["iters_max"]
    assert m_good + 2 < 60                      # (the solver's stagnation test needs more than 60 steps: the outcome below is the iteration limit)
    bad_v = RNG.standard_normal(d) + 1j * RNG.standard_normal(d)
    bad_w = RNG.standard_normal(d) + 1j * RNG.standard_normal(d)
    Vb = np.stack([V0[:, 0], bad_v, V0[:, 1], V0[:, 2]], axis=1)
    Wb = np.stack([W0[:, 0], bad_w, W0[:, 1], W0[:, 2]], axis=1)
    tb = np.stack([tabs4[0], tabs4[0], tabs4[1], tabs4[2]])
    fam.strict = False
    try:
        lam_b, V_b, st_b = fam.perturb_batch(tb, N, Vb, Wb, norm_mode=1, tol=L.solver_tol, maxit=m_good + 2)
    finally:
        fam.strict = True
    print("status", st_b, "code", fam.last_code, fam.last_info)
    assert fam.last_code == _lib.WAE_WARN_MAXITER
    assert list(st_b) == [0, _lib.WAE_WARN_MAXITER, 0, 0]
    assert fam.last_info["n_unconverged"] >= 1
    assert np.all(np.isfinite(lam_b)) and np.all(np.isfinite(V_b))
    for jb, jc in ((0, 0), (2, 1), (3, 2)):
        for k in range(1, N + 1):
            assert abs(lam_b[jb, k] - lam_c[jc, k]) < 1e-7 * abs(lam_c[jc, k]), (jb, k)
        assert np.linalg.norm(V_b[jb][:, 1] - V_c[jc][:, 1]) < 1e-5 * np.linalg.norm(V_c[jc][:, 1])
    # host-side argument checks
    import ctypes as C
    one = np.ones((d, 1), dtype=complex, order="F")
    out = np.zeros(4, dtype=complex)
    for nsys, NN in ((0, 1), (fam.batch + 1, 1), (-1, 1), (1, 201), (1, -1)):
        tab = np.zeros((2, 2, fam.T), dtype=complex)      # (rejected before anything is read)
        code = _lib.lib().wae_perturb_batch(fam.handle, nsys, _lib.zptr(tab), NN, _lib.zptr(one), _lib.zptr(one), 1, None, 1e-12, 10, _lib.zptr(out),
                                            None, None, None)
        assert code == _lib.WAE_ERR_INVALID, (nsys, NN, code)
    cols = np.zeros(1, dtype=np.int32)
    code = _lib.lib().wae_perturb_batch_slots(fam.handle, 0, _lib.zptr(tab), 1, 6, cols.ctypes.data_as(C.POINTER(C.c_int32)), 7,
                                              cols.ctypes.data_as(C.POINTER(C.c_int32)), 1, None, 1e-12, 10, _lib.zptr(out), None, None, None)
    assert code == _lib.WAE_ERR_INVALID


def test_c5_batch_of_four_order_30_half_million_dof():
    """C5 annulus (498 624 DoF) as test_c5_adjoint_perturbation_order_30_half_million_dof builds it: four start values refined together
    by householder_many, expanded together to N = 30; every column's Taylor (order 30) and Pade [15/15] prediction at 1.05 tau agrees
    with a re-solve of the perturbed problem to 1e-8 relative -- that test's bounds.  The start values lie next to the two SIMPLE
    modes of the annulus inside the benchmark contour (near 195 and 735 Hz), two each: its other modes come in pairs split by 1e-5
    relative and are left out of this prediction check (dev/perturb_many_time.py expands all eight)."""
    tau0 = 2e-4
    L, pb = annulus_family("C5", tau=tau0)
    assert pb["d"] == 498624
    L.solver_tol = 1e-12
    L.solver_ref = 2 * np.pi * 500.0
    L.solver_opts = {"batch": 16, "restart": 40, "sweeps": 1}
    fam = L.ensure_solver()
    starts = [2 * np.pi * (195 + 9j), 2 * np.pi * (735 + 3j), 2 * np.pi * (196.5 + 8j), 2 * np.pi * (733.5 + 4j)]
    res = householder_many(L, starts, maxiter=12, tol=1e-11)
    sols = [s for s, _, _ in res]
    for s in sols:
        w0 = s.params["ω"]
        first = next(i for i, zk in enumerate(s.history) if abs(zk - w0) < 1e-12 * abs(w0))
        assert first <= 9, s.history
    status = perturb_many(sols, L, "τ", 30, kind="fast")
    info = dict(fam.last_info)
    print("C5 batch info", info)
    assert info["n_unconverged"] == 0 and list(status) == [0, 0, 0, 0]
    eps = 1.05 * tau0
    preds = []
    for s in sols:
        lam = s.eigval_pert["τ/Taylor"]
        assert len(lam) == 31 and len(s.v_pert["τ/Taylor"]) == 31 and np.all(np.isfinite(lam))
        rad = conv_radius(lam)
        assert np.all(np.isfinite(rad)) and rad[-1] > 0.05 * tau0
        preds.append((s("τ", eps, 30), s("τ", eps, 15, 15)))
    L.params["τ"] = eps
    re = householder_many(L, [p[1] for p in preds], maxiter=8, tol=1e-11, v0s=[s.v for s in sols], v0s_adj=[s.v_adj for s in sols])
    for (w_taylor, w_pade), (s2, n2, f2) in zip(preds, re):
        w2 = s2.params["ω"]
        print("C5 column", w2 / 2 / np.pi, abs(w_pade - w2) / abs(w2), abs(w_taylor - w2) / abs(w2))
        assert f2 in (-1, 0, 1)
        assert abs(w_pade - w2) <= 1e-8 * abs(w2), (w_pade, w2)
        assert abs(w_taylor - w2) <= 1e-8 * abs(w2), (w_taylor, w2)
    L._drop_device()
