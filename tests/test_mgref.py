"""The references of tests/_mgref.py against second formulations, where no GPU is: the extended-precision CSR product and the
Galerkin triple product against scipy, the elimination against numpy.linalg.solve, the V-cycle recursion against the densely
assembled error-propagation operator of a two-grid cycle -- and DISCRIMINATION: every defect a comparison with the reference is
meant to catch (a post weight taken from the pre weight, a dropped coarse post-sweep, ...) moves the reference by at least 10^4
times the budget the device gets in tests/test_gpu_multigrid.py, on every column.  Without that the budget would prove nothing.

The hierarchy is synthetic: the four terms of the 1 152-DoF annulus (and the auxiliary term -M) with two plain-aggregation
prolongators made here (groups of 8 and of 6 consecutive unknowns; the rows of the 1e15 boundary term have no aggregate, as the
library's set-up leaves its penalty rows out): 1 152 -> 132 -> 22 unknowns, the last level dense."""
import numpy as np
import pytest
import scipy.sparse as sp

import _mgref as M
from _tilecheck import annulus_coeffs
from wae_amd.helmholtz import annulus

W = dict(w_pre=0.7, w_post=0.9, w_light=0.5)            # (not the defaults 0.8 / 0.9 / 0.5: pre and light weight further apart)
Z0 = 2 * np.pi * (430 + 15j)
R_COLS = 8


def aggregation(n, skip, size):
    """P (n x groups): row i has a single 1 in the column of its group of `size` consecutive kept unknowns; rows in `skip` are empty"""
    keep = np.nonzero(~skip)[0]
    grp = np.arange(len(keep)) // size
    return sp.csr_matrix((np.ones(len(keep)), (keep, grp)), shape=(n, grp[-1] + 1))


@pytest.fixture(scope="module")
def hier():
    pb = annulus.build("tiny", tau=2e-4)
    T = pb["terms"]
    terms0 = [T["M"].tocsr(), T["K"].tocsr(), T["C"].tocsr(), T["Q"].tocsr(), (-T["M"]).tocsr()]
    n0 = terms0[0].shape[0]
    assert n0 == 1152
    pen = np.asarray(abs(T["C"]).sum(axis=1)).ravel() > 0            # rows of the boundary term: 1e15 on their diagonal
    assert 0 < pen.sum() < n0 // 2
    P0 = aggregation(n0, pen, 8)
    R0 = P0.T.tocsr()
    terms1 = [sp.csr_matrix(R0 @ A @ P0) for A in terms0]
    n1 = P0.shape[1]
    P1 = aggregation(n1, np.zeros(n1, dtype=bool), 6)
    R1 = P1.T.tocsr()
    levels = [M.Level(terms0), M.Level(terms1), M.dense_level(R1, terms1, P1)]
    transfers = [(P0, R0), (P1, R1)]
    rng = np.random.default_rng(7)
    zs = Z0 + 2 * np.pi * np.linspace(-40, 40, R_COLS) * (1 + 0.2j)
    ct = annulus_coeffs(zs, tau=2e-4)
    ct[:, 4] = 0.3 * np.exp(1j * np.arange(R_COLS))                  # (the auxiliary term takes part: its coefficient is 0 in L(z) alone)
    B = [rng.standard_normal((lv.n, R_COLS)) + 1j * rng.standard_normal((lv.n, R_COLS)) for lv in levels]
    B[0] = B[0] * np.maximum(np.abs(levels[0].diag(ct[:1], "N", 1, np.complex128)), 1.0)   # right-hand sides of the size of their rows
    return dict(levels=levels, transfers=transfers, pen=pen, ct=ct, B=B, rng=rng, sizes=(n0, n1, P1.shape[1]))


def test_sizes(hier):
    n0, n1, n2 = hier["sizes"]
    assert (n0, hier["levels"][1].n, hier["levels"][2].n) == (n0, n1, n2) and 100 < n1 < 150 and 16 < n2 < 26


def test_csr_product_against_scipy(hier):
    rng = hier["rng"]
    P0 = hier["transfers"][0][0]
    for A in (hier["levels"][0].terms[3], hier["levels"][1].terms[1], P0.astype(np.complex128), P0.T.tocsr().astype(np.complex128)):
        X = rng.standard_normal((A.shape[1], 5)) + 1j * rng.standard_normal((A.shape[1], 5))
        Y, mag = M.csr_matmat(A, X)
        assert Y.dtype == M.LD
        want, wmag = A @ X, abs(A) @ np.abs(X)
        nmax = int(np.max(np.diff(A.indptr)))
        assert np.all(np.abs(Y - want) <= 2 * (nmax + 2) * M.EPS * wmag)     # scipy's own float64 summation
        assert np.all(np.abs(mag - wmag) <= 2 * (nmax + 2) * M.EPS * wmag)
        empty = np.diff(A.indptr) == 0
        assert np.all(Y[empty] == 0) and np.all(mag[empty] == 0)             # (P0 has empty rows: the penalty rows)
    assert np.any(np.diff(P0.indptr) == 0)
    # one column and a vector argument
    x = rng.standard_normal(P0.shape[1])
    y, _ = M.csr_matmat(P0, x)
    assert y.shape == (P0.shape[0],) and np.all(np.abs(y - P0 @ x) <= 4 * M.EPS * np.abs(P0 @ x))


def test_galerkin_against_scipy(hier):
    P0, R0 = hier["transfers"][0]
    for k in (0, 2, 3):
        A = hier["levels"][0].terms[k]
        G, bound = M.galerkin(R0, A, P0)
        want = np.asarray((R0 @ A @ P0).todense())
        wb = np.asarray((abs(R0) @ abs(A) @ abs(P0)).todense())
        assert np.all(np.abs(G - want) <= 256 * M.EPS * wb)                  # (8 x 8 fine entries per aggregate pair, ~15 per row)
        assert np.all(np.abs(bound - wb) <= 256 * M.EPS * wb)
        assert np.all((bound == 0) == (wb == 0))


def test_dense_solve_against_numpy(hier):
    rng = hier["rng"]
    lv = hier["levels"][2]
    A = lv.matrix(hier["ct"][0], "N", np.complex128)
    Bm = rng.standard_normal((lv.n, 3)) + 1j * rng.standard_normal((lv.n, 3))
    X = M.dense_solve(A.astype(M.LD), Bm)
    want = np.linalg.solve(A, Bm)
    kappa = np.linalg.cond(A)
    assert np.max(np.abs(X - want)) <= 64 * lv.n * M.EPS * kappa * np.max(np.abs(want))
    assert np.max(np.abs(A.astype(M.LD) @ X - Bm)) <= 64 * lv.n * M.EPS * np.max(np.abs(A)) * np.max(np.abs(X)) / 1e3      # extended: residual 1e3 below float64's


@pytest.mark.parametrize("op", ["N", "T", "C"])
@pytest.mark.parametrize("nsweeps", [1, 2])
def test_cycle_against_the_error_propagation_operator(hier, op, nsweeps):
    """two-grid cycle on levels 1 -> 2: M^-1 A x = x - E x with E = (I - w_post D^-1 A)^p (I - P Ac^-1 R A) (I - w_pre D^-1 A)^p,
    assembled densely in float64.  Tolerance: the float64 side inverts Ac (22 x 22) and multiplies 132 x 132 matrices:
    64 n eps kappa(Ac), the measure of the dense-level tests."""
    lv1, lv2 = hier["levels"][1], hier["levels"][2]
    P, R = (np.asarray(m.todense()) for m in hier["transfers"][1])
    n = lv1.n
    x = hier["B"][1]
    for j, c in enumerate(hier["ct"][:3]):
        cc = c.conj() if op == "C" else c
        A = sum(ck * np.asarray((Ak if op == "N" else (Ak.T if op == "T" else Ak.conj().T)).todense()) for ck, Ak in zip(cc, lv1.terms))
        Ac = lv2.matrix(cc, op, np.complex128)
        Di = 1.0 / np.diag(A)
        I = np.eye(n)
        Spre, Spost = I - W["w_pre"] * Di[:, None] * A, I - W["w_post"] * Di[:, None] * A
        E = np.linalg.matrix_power(Spost, nsweeps) @ (I - P @ np.linalg.solve(Ac, R @ A)) @ np.linalg.matrix_power(Spre, nsweeps)
        want = x[:, j:j + 1] - E @ x[:, j:j + 1]
        got = M.vcycle_ref(hier["levels"], hier["transfers"], A @ x[:, j:j + 1], c[None, :], level=1, op=op, nsweeps=nsweeps, **W)
        tol = 64 * n * M.EPS * np.linalg.cond(Ac)
        assert np.max(np.abs(got - want)) <= tol * np.max(np.abs(want)), (j, float(np.max(np.abs(got - want)) / np.max(np.abs(want))), tol)
        # the light cycle: E = (I - P Ac^-1 R A) (I - w_light D^-1 A)^p
        El = (I - P @ np.linalg.solve(Ac, R @ A)) @ np.linalg.matrix_power(I - W["w_light"] * Di[:, None] * A, nsweeps)
        gotl = M.vcycle_ref(hier["levels"], hier["transfers"], A @ x[:, j:j + 1], c[None, :], level=1, op=op, nsweeps=nsweeps, light=True, **W)
        wantl = x[:, j:j + 1] - El @ x[:, j:j + 1]
        assert np.max(np.abs(gotl - wantl)) <= tol * np.max(np.abs(wantl))


def test_one_row_for_all_columns_equals_one_row_per_column(hier):
    """columns never mix: a batch with one coefficient row per column is the single-system cycles side by side.  (The single system
    multiplies with the operator assembled in extended precision, the batch term by term: two summation orders, far below eps apart.)"""
    H = hier
    full = M.vcycle_ref(H["levels"], H["transfers"], H["B"][0], H["ct"], **W)
    for j in (0, 5):
        one = M.vcycle_ref(H["levels"], H["transfers"], H["B"][0][:, j:j + 1], H["ct"][j:j + 1], **W)
        assert np.max(np.abs(one[:, 0] - full[:, j])) <= 1e-3 * M.EPS * np.max(np.abs(full[:, j]))


def _groups(H, level):
    return (H["pen"], ~H["pen"]) if level == 0 else (np.ones(H["levels"][level].n, dtype=bool),)


def _true_and_budget(H, level, **kw):
    args = (H["levels"], H["transfers"], H["B"][level], kw.pop("ct", H["ct"]))
    ref = M.vcycle_ref(*args, level=level, **W, **kw)
    r64 = M.vcycle_ref(*args, level=level, dtype=np.complex128, **W, **kw)
    e64 = M.column_errors(r64, ref, _groups(H, level))
    assert np.all(e64 < 1e-9), e64                                   # the float64 evaluation is itself a sane evaluation
    return ref, M.budget(e64)


CASES = [
    # name, arguments of the true reference, arguments that replace them in the defective one
    ("post weight taken from the pre weight", dict(), dict(w_post=W["w_pre"])),
    ("coarse post-sweep dropped in the full cycle", dict(), dict(post=lambda l, light, ns: 0 if (light or l >= 1) else ns)),
    ("light cycle run with the pre weight", dict(light=True), dict(w_light=W["w_pre"])),
    ("b restricted instead of the residual", dict(), dict(mutate=("restrict_b",))),
    ("b restricted instead of the residual, light", dict(light=True), dict(mutate=("restrict_b",))),
    ("level 1 not conjugated for op C", dict(op="C"), dict(mutate=("level1_unconjugated",))),
    ("level 1: column j with the coefficients of column j + 1", dict(), dict(mutate=("level1_neighbour",))),
    ("two sweeps, iterate before the last one returned", dict(nsweeps=2), dict(mutate=("early_return",))),
    ("two sweeps, iterate before the last one returned, light", dict(nsweeps=2, light=True), dict(mutate=("early_return",))),
]


@pytest.mark.parametrize("name,true_kw,bad_kw", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("level", [0, 1])
def test_discrimination(hier, name, true_kw, bad_kw, level):
    if level == 1 and "level 1" in name:
        level = 0                                                    # (a defect of level 1 seen from the fine level and ...
        true_kw = dict(true_kw, ct=hier["ct"][::-1].copy())          # ... with the systems in the opposite order)
    H = hier
    ref, bud = _true_and_budget(H, level, **dict(true_kw))
    kw = dict(W)
    kw.update({k: v for k, v in true_kw.items() if k != "ct"})
    kw.update(bad_kw)
    bad = M.vcycle_ref(H["levels"], H["transfers"], H["B"][level], true_kw.get("ct", H["ct"]), level=level, **kw)
    dist = M.column_errors(bad, ref, _groups(H, level))
    assert np.all(dist >= 1e4 * bud), (name, level, float(np.min(dist / bud)))
