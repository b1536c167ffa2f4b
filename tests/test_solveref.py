"""tests/_solveref.py where no GPU is: the reference GMRES satisfies its own definition (the least-squares minimum over an explicitly
built Krylov space, before and after a restart), the complex128 replays of the library's two orthogonalisations agree with it (the
MEASUREMENT of BETA), and DISCRIMINATION: each of seven defects of a solve driver, seeded into the replay, misses the bounds that
tests/test_gpu_solve_driver.py asserts by at least 100 budgets (or, where the bound is a count of steps, falls outside it) at the
widths, step counts and recurrence lengths that module uses.  Without that the bounds would prove nothing.

The hierarchy is synthetic, as in tests/test_mgref.py but smaller: the four terms of a 384-DoF annulus (grid 12 x 8 x 4, 48 penalty rows
of 1e15 on the diagonal) and the auxiliary term -M, two plain-aggregation prolongators (groups of 4 and 4): 384 -> 84 -> 21, the last
level dense.  Columns and coefficient rows as in the GPU module: 16 distinct right-hand sides scaled to their rows, one of them zero,
coefficient rows on the line Z_AB + LINE.  Plain aggregation is a weaker preconditioner than the library's: the restarted converged case
needs RESTART_SYN here where the GPU module runs restart 6."""
import numpy as np
import pytest
import scipy.sparse as sp

import _mgref as M
import _solveref as S
from _hier import LINE, Z_AB
from _tilecheck import annulus_coeffs
from test_mgref import aggregation
from wae_amd.helmholtz import annulus

W = dict(w_pre=0.7, w_post=0.9, w_light=0.5)
NB, RESTART = S.NB_SMALL, S.RESTART_SMALL
RESTART_SYN = 9              # pick_restart(start=6) on this hierarchy: GMRES(6) .. GMRES(8) stall or run past maxit here


@pytest.fixture(scope="module")
def syn():
    pb = annulus.build(grid=(12, 8, 4), tau=2e-4)
    T = pb["terms"]
    terms0 = [T["M"].tocsr(), T["K"].tocsr(), T["C"].tocsr(), T["Q"].tocsr(), (-T["M"]).tocsr()]
    n0 = terms0[0].shape[0]
    pen = np.asarray(abs(T["C"]).sum(axis=1)).ravel() > 0
    assert n0 == 384 and 0 < pen.sum() < n0 // 2
    P0 = aggregation(n0, pen, 4)
    R0 = P0.T.tocsr()
    terms1 = [sp.csr_matrix(R0 @ A @ P0) for A in terms0]
    P1 = aggregation(P0.shape[1], np.zeros(P0.shape[1], dtype=bool), 4)
    R1 = P1.T.tocsr()
    levels = [M.Level(terms0), M.Level(terms1), M.dense_level(R1, terms1, P1)]
    ct16 = annulus_coeffs((Z_AB + LINE)[::4], tau=2e-4)
    ct1 = annulus_coeffs(np.array([Z_AB]), tau=2e-4)
    rng = np.random.default_rng(11)
    B16 = rng.standard_normal((n0, 16)) + 1j * rng.standard_normal((n0, 16))
    B16 = B16 * np.maximum(np.abs(levels[0].diag(ct1, "N", 1, np.complex128)), 1.0)
    return S.Contract(levels, [(P0, R0), (P1, R1)], W, 1, B16, ct16, ct1)


def run(C, r, percol, op, tol, maxit, NB=NB, restart=RESTART, **kw):
    B, ct = C.columns(r, percol)
    return S.replay(C.ref(op), B, ct, NB, restart, tol, maxit, **kw)


# ----------------------------------------------------------------------------------------------------
# the rules
# ----------------------------------------------------------------------------------------------------
def test_recurrence_lengths_and_chunks():
    assert [S.recurrence_length(6, 16, nb) for nb in (16, 12, 8, 3, 1)] == [6, 8, 13, 36, 111]
    assert [S.recurrence_length(30, 64, nb) for nb in (64, 16, 5, 1)] == [30, 123, 150, 150]
    assert S.recurrence_length(30, 64, 16, deflated=True) == 122
    assert S.chunks(35, 16) == [(0, 16), (16, 16), (32, 3)] and S.chunks(16, 16) == [(0, 16)] and S.chunks(5, 64) == [(0, 5)]
    assert S.ks_for(12) == (1, 2, 5, 7, 8, 9, 10) and S.ks_for(8) == (1, 2, 5, 12, 13, 14, 15)
    h = np.array([[0.5, 0.5], [0.1, 0.2], [0.01, 0.1]])
    assert list(S.steps_to(h, 0.1)) == [2, 3]
    with pytest.raises(ValueError):
        S.steps_to(h, 0.05)


def test_columns_of_a_case(syn):
    B, ct = syn.columns(35, True)
    assert B.shape[1] == 35 and ct.shape[0] == 35
    assert [j for j in range(35) if not B[:, j].any()] == [1, 17, 33]
    assert np.array_equal(B[:, 16:32], B[:, :16]) and np.array_equal(ct[16:32], ct[:16]) and not np.array_equal(ct[0], ct[2])
    B, ct = syn.columns(3, False)
    assert ct.shape[0] == 1 and not B[:, 1].any() and B[:, 0].any() and B[:, 2].any()


# ----------------------------------------------------------------------------------------------------
# the reference satisfies its own definition
# ----------------------------------------------------------------------------------------------------
def _krylov_minimum(ref, z, ct, k):
    """min_y ||z - Op V y|| over the Krylov space of Op = M^-1 A and z, dimension k, with NO Hessenberg matrix: an orthonormal basis V
    of span{z, Op z, ...} (each new direction Op v orthogonalised twice), the products Op V formed afresh, and a QR of them"""
    V = [z / S._norm(z)]
    for j in range(k - 1):
        w = ref.minv(ref.apply(V[j], ct), ct)
        for _ in range(2):
            for v in V:
                w = w - S._dot(v, w) * v
        V.append(w / S._norm(w))
    Wk = [ref.minv(ref.apply(v, ct), ct) for v in V]
    Q = []
    for a in Wk:
        for _ in range(2):
            for q in Q:
                a = a - S._dot(q, a) * q
        Q.append(a / S._norm(a))
    res = z
    for _ in range(2):
        for q in Q:
            res = res - S._dot(q, res) * q
    return S._norm(res)


@pytest.mark.parametrize("percol", [False, True])
def test_reference_is_the_least_squares_minimum(syn, percol):
    ref = syn.ref("N")
    B, ct = syn.columns(4, percol)
    B, ct = B[:, [0, 2, 3]], (ct[[0, 2, 3]] if percol else ct)
    m, kmax = 4, 7
    hist, xs = ref.gmres(B, ct, m, kmax, keep=range(1, kmax + 1))
    bn = ref.bnorm(B, ct)
    z0 = ref.minv(B.astype(M.LD), ct)
    for k in range(1, m + 1):                                        # the first cycle
        want = _krylov_minimum(ref, z0, ct, k) / bn
        assert np.all(np.abs(hist[k - 1] - want) <= 1e-15 * want), (k, np.abs(hist[k - 1] / want - 1))
    z1 = ref.minv(B.astype(M.LD) - ref.apply(xs[m], ct), ct)         # after the restart: from the recomputed residual
    assert np.all(np.abs(S._norm(z1) / bn - hist[m - 1]) <= 1e-15 * hist[m - 1])
    for k in range(m + 1, kmax + 1):
        want = _krylov_minimum(ref, z1, ct, k - m) / bn
        assert np.all(np.abs(hist[k - 1] - want) <= 1e-15 * want), (k, np.abs(hist[k - 1] / want - 1))
    for k in range(1, kmax + 1):                                     # the iterates attain the minima
        rho = ref.rho(xs[k], B, ct)
        assert np.all(np.abs(rho - hist[k - 1]) <= 1e-15 * hist[k - 1]), k
    assert np.all(np.diff(np.asarray(hist, dtype=float), axis=0) <= 0)
    # until: the history is cut at the first step at which every column is there
    cut = ref.gmres(B, ct, m, kmax, until=hist[2].max())[0]
    assert len(cut) == 3 and np.array_equal(cut, hist[:3])


def test_zero_right_hand_side_and_least_squares_helper(syn):
    ref = syn.ref("N")
    B, ct = syn.columns(3, True)
    hist, xs = ref.gmres(B[:, 1], ct[1:2], 6, 4, keep=(2,))
    assert hist.shape == (0, 1) and not xs[2].any()
    hist, xs = ref.gmres(B, ct, 6, 4, keep=(4,))
    assert not hist[:, 1].any() and not xs[4][:, 1].any() and hist[:, [0, 2]].all()
    one, _ = ref.gmres(B[:, 2], ct[2:3], 6, 4)
    assert np.all(np.abs(one[:, 0] - hist[:, 2]) <= 1e-16 * hist[:, 2])     # (one row for all columns: the operator is assembled first)
    assert np.all(ref.rho_u(xs[4], B, ct)[0][[1]] == 0)
    rng = np.random.default_rng(0)
    H = np.triu(rng.standard_normal((6, 5)) + 1j * rng.standard_normal((6, 5)), -1)
    ls = S._Lsq(5, np.array([2.0 + 0j]))
    for k in range(5):
        got = ls.push(H[:, k:k + 1])
        g = np.zeros(6, dtype=complex)
        g[0] = 2.0
        y = np.linalg.lstsq(H[:, :k + 1], g, rcond=None)[0]
        assert abs(got[0] - np.linalg.norm(g - H[:, :k + 1] @ y)) <= 1e-13
        assert np.max(np.abs(ls.y()[:, 0] - y)) <= 1e-12 * np.max(np.abs(y))


# ----------------------------------------------------------------------------------------------------
# the replays against the reference: BETA
# ----------------------------------------------------------------------------------------------------
def test_restart_of_the_restarted_case(syn):
    assert syn.pick_restart("N", False, 16, NB, start=RESTART_SYN) == RESTART_SYN
    B, ct = syn.columns(16, False)
    h6 = np.asarray(syn.ref("N").gmres(B, ct, RESTART, S.MAXIT, dtype=np.complex128, until=0.35 * S.TOL)[0], dtype=float)
    assert len(h6) == S.MAXIT and h6[-1].max() > S.TOL                # (restart 6, the GPU module's, does not get there on this hierarchy)


def _floor_step(C, r, percol, NB_, restart):
    """the last step at which every column of a converged case is still above the floor"""
    h = np.asarray(C.case_history("N", percol, r, NB_, restart, S.MAXIT, until=0.35 * S.TOL), dtype=np.float64)
    live = h[0] > 0
    return int(np.nonzero(np.all(h[:, live] >= S.FLOOR, axis=1))[0][-1]) + 1


def test_beta_measurement(syn):
    """every case of the GPU module, run by the replay with the orthogonalisation the library gives that width: the truncated table as
    it stands, the three converged solves cut at the last step above the floor of 1e-9 (below it the attainable accuracy of float64
    enters, which the bounds carry as u).  Measured on this hierarchy: see BETA_MEASURED."""
    C = syn
    worst = 0.0
    cases = [(c, NB, RESTART, {}) for c in S.truncated_cases()]
    cases += [((64, _floor_step(C, 64, True, S.NB_WIDE, S.RESTART_WIDE), True, "N"), S.NB_WIDE, S.RESTART_WIDE, {}),
              ((5, _floor_step(C, 5, False, S.NB_WIDE, S.RESTART_WIDE), False, "N"), S.NB_WIDE, S.RESTART_WIDE, {}),
              ((16, _floor_step(C, 16, False, NB, RESTART_SYN), False, "N"), NB, RESTART_SYN, {})]
    cases += [((16, 7, True, "N"), NB, RESTART, dict(pair_min=-1)), ((16, 7, True, "N"), NB, RESTART, dict(pair_min=0)),
              ((16, 13, False, "N"), NB, RESTART, dict(device=False)), ((8, 14, True, "N"), NB, RESTART, dict(narrow_pair=True))]
    for (r, k, percol, op), nb_, rs_, kw in cases:
        X, info, _ = run(C, r, percol, op, 1e-300, k, NB=nb_, restart=rs_, **kw)
        fig = C.check_truncated(X, info, info["code"], r, k, percol, op, nb_, rs_, enforce=False)
        assert fig["counts"], ((r, k, percol, op), info)
        dist = float(np.max(np.abs(fig["rho"] / fig["rk"] - 1)))
        if dist > worst:
            worst = dist
            print(f"r={r} k={k} percol={percol} op={op} NB={nb_} restart={rs_} {kw}: |rho / r_k - 1| = {dist:.3e} (r_k {fig['rk'].min():.1e}..)")
        assert np.all(np.abs(fig["units"]) <= 1) and fig["rdist"] <= 1 and not X[:, S.ZERO_COL].any(), ((r, k, percol, op), fig)   # the clean replay meets the contract
    print(f"BETA: measured {worst:.3e}, written {S.BETA_MEASURED:.3e}, budget {S.BETA:.3e}")
    assert worst <= S.BETA / 4, (worst, S.BETA)
    assert S.BETA == 8 * S.BETA_MEASURED


def test_clean_replay_meets_the_converged_contract(syn):
    C = syn
    for r, percol, nb_, rs_ in ((64, True, S.NB_WIDE, S.RESTART_WIDE), (5, False, S.NB_WIDE, S.RESTART_WIDE), (16, False, NB, RESTART_SYN)):
        X, info, iters = run(C, r, percol, "N", S.TOL, S.MAXIT, NB=nb_, restart=rs_)
        klo, khi = C.check_converged(X, info, info["code"], r, percol, "N", nb_, rs_)
        assert np.all((klo <= iters) & (iters <= khi)), (r, klo, iters, khi)


# ----------------------------------------------------------------------------------------------------
# discrimination
# ----------------------------------------------------------------------------------------------------
TRUNC_DEFECTS = [
    # defect, (r, k, percol), side on which the bound is missed
    ("update_one_short", (16, 5, True), +1),                         # (a) x += V y from k - 1 columns: the iterate of step k - 1
    ("update_one_short", (8, 13, False), +1),
    ("late_restart", (16, 7, True), -1),                             # (b) m + 1 steps in the first cycle: below the restarted minimum
    ("late_restart", (8, 14, False), -1),
    ("pair_across_maxit", (16, 3, True), -1),                        # (c) steps 3 and 4 as a pair although maxit = 3
    ("pair_across_maxit", (35, 11, False), -1),
    ("neighbour_coefficients", (16, 3, True), +1),                   # (d)
    ("neighbour_coefficients", (35, 2, True), +1),
    ("m_from_batch", (12, 8, True), +1),                             # (f) the ragged chunk restarts after 6 steps instead of 8
    ("m_from_batch", (35, 13, True), +1),                            #     ... and the last chunk of 3 after 6 instead of 36
    ("m_from_batch", (3, 12, False), +1),
]


@pytest.mark.parametrize("defect,case,side", TRUNC_DEFECTS, ids=[f"{d}-r{c[0]}-k{c[1]}" for d, c, _ in TRUNC_DEFECTS])
def test_seeded_defect_misses_the_rho_bounds(syn, defect, case, side):
    r, k, percol = case
    X, info, _ = run(syn, r, percol, "N", 1e-300, k, defects=(defect,))
    fig = syn.check_truncated(X, info, info["code"], r, k, percol, "N", NB, RESTART, enforce=False)
    far = side * fig["units"]
    print(f"{defect} {case}: rho - r_k in units of the budget {fig['units'].min():+.3g}..{fig['units'].max():+.3g}")
    assert np.max(far) >= 100, (defect, case, float(np.max(far)))
    with pytest.raises(AssertionError):
        syn.check_truncated(X, info, info["code"], r, k, percol, "N", NB, RESTART)
    if defect == "pair_across_maxit":
        assert info["iters_max"] == k + 1 and not fig["counts"]


def test_seeded_defect_in_the_step_counts(syn):
    """(e) a frozen column goes on being updated and (g) iters_total counts lock-step iterations times columns: both leave every
    residual inside its bounds and show in the counts alone, which are integers -- they fall outside the bounds, by how much is printed.
    (e) shows where a cycle is long and the columns stop steps apart, the 64 columns under m = 30: iters_total 1500 against sum khi = 1468
    here (sum klo 1436).  Under a short restart a frozen column is taken out at the next cycle start anyway.)"""
    C = syn
    X, info, _ = run(C, 64, True, "N", S.TOL, S.MAXIT, NB=S.NB_WIDE, restart=S.RESTART_WIDE, defects=("frozen_updated",))
    klo, khi, inside = C.check_converged(X, info, info["code"], 64, True, "N", S.NB_WIDE, S.RESTART_WIDE, enforce=False)
    print(f"frozen_updated: iters_total {info['iters_total']} against sum khi {khi.sum()} (sum klo {klo.sum()})")
    assert not inside and info["iters_total"] > khi.sum()
    with pytest.raises(AssertionError):
        C.check_converged(X, info, info["code"], 64, True, "N", S.NB_WIDE, S.RESTART_WIDE)
    for r, k in ((16, 3), (35, 7), (3, 2)):
        X, info, _ = run(C, r, True, "N", 1e-300, k, defects=("iters_lockstep",))
        fig = C.check_truncated(X, info, info["code"], r, k, True, "N", NB, RESTART, enforce=False)
        assert not fig["counts"] and info["iters_total"] == k * r and np.max(np.abs(fig["units"])) <= 1
        with pytest.raises(AssertionError):
            C.check_truncated(X, info, info["code"], r, k, True, "N", NB, RESTART)
    X, info, _ = run(C, 64, True, "N", S.TOL, S.MAXIT, NB=S.NB_WIDE, restart=S.RESTART_WIDE, defects=("iters_lockstep",))
    klo, khi, inside = C.check_converged(X, info, info["code"], 64, True, "N", S.NB_WIDE, S.RESTART_WIDE, enforce=False)
    print(f"iters_lockstep: iters_total {info['iters_total']} against sum khi {khi.sum()}")
    assert not inside
