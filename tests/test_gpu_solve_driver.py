"""The lock-step GMRES DRIVERS (csrc/gmres.hip struct Gmres: run_device, run_host, start, cycle_start, finish, converged_by_estimate; the
chunk loop of wae_solve_guess) against a reference preconditioned solve.  The kernels they launch are pinned one by one elsewhere
(test_gpu_vector_kernels, test_gpu_gmres_recurrence, test_gpu_multigrid); this module holds what composes them: how long a cycle is,
when it restarts, whether a pair step may still be taken before maxit, which columns are frozen, when a true residual is recomputed,
which recurrence a batch gets, and how wae_solve_info is filled and summed over chunks.

The contract (tests/_solveref.py, whose docstring states the driver's rules): after k steps the iterate minimises
||M^-1 (b - A x)|| over x0 + K_k, whatever the orthogonalisation.  The minimum r_k is computed in extended precision for the RECOVERED
hierarchy of the family (tests/_hier.py) with the V-cycle of tests/_mgref.py, on 16 distinct columns; wider batches repeat them.
Every solve goes through wae_solve / wae_solve_guess; rho_b = ||M^-1 (b - A x_b)|| / ||M^-1 b|| of what they return is evaluated by
the reference, u_b is the distance of its complex128 evaluation, BETA the allowance for float64 Gram-Schmidt measured in
tests/test_solveref.py, which also shows that seven seeded defects of a driver miss these bounds by more than 100 budgets.

  a. truncated solves (tol = 1e-300, maxit = k): r_k (1 - BETA) - 16 u_b <= rho_b <= r_k (1 + BETA) + 16 u_b (below: more than k steps
     were taken; above: not the minimiser), the counts of info exactly, relres_max the recomputed residual, zero columns exact zeros.
     Widths 16 (device recurrence), 12 (ragged device chunk, m = 8), 8 and 3 (host recurrence, m = 13 and 36), 35 (chunks 16 + 16 + 3).
     Width 3 reaches 1e-17 long before its m = 36: its steps around m lie below the floor of 1e-9 the bounds need, so its table has
     7, 12, 13 and 18 instead -- all past the recurrence length 6 that the batch width would give, the defect a narrow chunk can have.
  b. converged solves (tol = 1e-10): residuals, relres_max, and the step counts between the first steps of the reference at
     0.7 tol (1 + BETA) -- or at tol at the start of a cycle, where the driver recomputes -- and at 0.35 tol; the same column by column;
     X against a sparse LU.
  c. a guess direction (random, with a zero column, the solution itself); d. the Bloch family with complex coefficients;
  e. the switches of the drivers, each in a child process held to the same bounds; f. a handle used again after a cycle cut short.

Near-singular shifts and the drift mode of the host recurrence stay with the Newton-solver tests (test_gpu_parity); NaN inputs with
test_nan_column_stays_alone.

Figures on an MI355X: see the docstrings of the tests."""
import ctypes as C_
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse.linalg as spla

import _solveref as S
from _hier import OPS, family_a, family_c
from wae_amd import _lib
from wae_amd._lib import SolveInfo, zptr

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
NB, RESTART = S.NB_SMALL, S.RESTART_SMALL


def contract_of(H):
    return S.Contract(H.levels, H.transfers, H.w, H.nsweeps, H.B[0][:, :S.DISTINCT].copy(), H.ct64[:S.DISTINCT].copy(), H.ct1.copy(), nlevels=H.nl)


def report(name, C):
    print(f"family {name}: largest figures in units of their bounds: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(C.worst.items())))


@pytest.fixture(scope="module")
def a16():
    """family A (annulus "tiny", 1 152 DoF, three levels), batch 16 / restart 6"""
    H = family_a(1, distinct=S.DISTINCT, batch=NB, restart=RESTART)
    assert H.nl == 3 and H.n[0] == 1152
    C = contract_of(H)
    yield H, C
    report("A", C)
    H.L._drop_device()


@pytest.fixture(scope="module")
def a64(a16):
    """family A, batch 64 with the default restart (30): the same hierarchy, so the same references"""
    H = family_a(1, distinct=S.DISTINCT, batch=S.NB_WIDE)
    H0, C = a16
    for l in range(H.nl - 1):
        assert (H.Pm[l] != H0.Pm[l]).nnz == 0
    assert all((a != b).nnz == 0 for a, b in zip(H.terms[1], H0.terms[1])) and np.array_equal(H.B[0], H0.B[0])
    yield H, C
    H.L._drop_device()


@pytest.fixture(scope="module")
def c16():
    """family C (Bloch cell, 728 DoF, complex coefficients, b = 5), batch 16 / restart 6"""
    H = family_c(distinct=S.DISTINCT, batch=NB, restart=RESTART)
    assert H.nl == 3 and H.n[0] == 728
    C = contract_of(H)
    yield H, C
    report("C", C)
    H.L._drop_device()


def solve(H, C, r, percol, op, tol, maxit, guess=None, cols=None):
    B, ct = C.columns(r, percol)
    if cols is not None:
        B, ct = B[:, cols], (ct[cols] if percol else ct)
    X = H.fam.solve(ct, B, op=OPS[op], tol=tol, maxit=maxit, strict=False, quiet=True, guess=guess)
    return X, dict(H.fam.last_info), H.fam.last_code


def lu_solution(H, C, r, percol, op="N"):
    B, ct = C.columns(min(r, S.DISTINCT), percol)
    X = np.zeros_like(B)
    for j in range(B.shape[1]):
        c = ct[j] if percol else ct[0]
        A = sum(ck * t for ck, t in zip(c, H.terms[0])).tocsc()
        A = A if op == "N" else (A.T if op == "T" else A.conj().T).tocsc()
        X[:, j] = spla.splu(A).solve(B[:, j])
    return np.tile(X, (1, -(-r // S.DISTINCT)))[:, :r]


def assert_lu_parity(X, Xlu, what):
    live = np.any(Xlu != 0, axis=0)
    err = np.linalg.norm(X[:, live] - Xlu[:, live], axis=0) / np.linalg.norm(Xlu[:, live], axis=0)
    print(f"{what}: against the sparse LU, largest relative error per column {err.max():.2e}")
    assert np.all(err < 1e-8), (what, float(err.max()))


# ----------------------------------------------------------------------------------------------------
# a. truncated solves
# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [16, 12, 8, 3, 35])
def test_truncated_solves(a16, r):
    """MI355X: over the whole table |rho - r_k| stays below 0.005 of its budget BETA r_k + 16 u (0.25 of 16 u alone; worst: r = 8, k = 15,
    one row per column), relres_max within 0.49 of its budget 16 max u (r = 3, k = 2); every count exact."""
    H, C = a16
    for k in S.ks_for(r):
        for percol in (False, True):
            X, info, code = solve(H, C, r, percol, "N", 1e-300, k)
            C.check_truncated(X, info, code, r, k, percol, "N", NB, RESTART)


@pytest.mark.parametrize("op", ["C", "T"])
def test_truncated_solves_of_the_adjoint_and_the_transpose(a16, op):
    H, C = a16
    for k in (3, 7):
        for percol in (False, True):
            X, info, code = solve(H, C, 16, percol, op, 1e-300, k)
            C.check_truncated(X, info, code, 16, k, percol, op, NB, RESTART)


# ----------------------------------------------------------------------------------------------------
# b. converged solves
# ----------------------------------------------------------------------------------------------------
def check_singles(H, C, percol, klo, khi, cols):
    for j in cols:
        X, info, code = solve(H, C, S.DISTINCT, percol, "N", S.TOL, S.MAXIT, cols=[j])
        if klo[j] == 0:
            assert code == S.WAE_OK and info["iters_total"] == 0 and not X.any(), (j, info)
            continue
        assert code == S.WAE_OK and info["n_unconverged"] == 0, (j, info)
        assert info["iters_max"] == info["iters_total"] and klo[j] <= info["iters_total"] <= khi[j], (j, int(klo[j]), info, int(khi[j]))
        assert info["relres_max"] <= S.TOL
    print(f"columns one at a time, percol={percol}: every count inside [klo, khi] = {[(int(klo[j]), int(khi[j])) for j in cols]}")


def test_converged_wide_batch_on_the_device_path(a64):
    """r = 64, one coefficient row per column, batch 64 (m = 30).  MI355X: iters_total 1412 = sum klo (sum khi 1432), iters_max 27 = max klo =
    max khi: no slack used."""
    H, C = a64
    X, info, code = solve(H, C, 64, True, "N", S.TOL, S.MAXIT)
    C.check_converged(X, info, code, 64, True, "N", S.NB_WIDE, S.RESTART_WIDE)
    assert_lu_parity(X, lu_solution(H, C, 64, True), "r=64")
    klo, khi = C.single_bounds("N", True, S.NB_WIDE, S.RESTART_WIDE)
    check_singles(H, C, True, klo, khi, range(S.DISTINCT))


def test_converged_narrow_batch_on_the_host_path(a64):
    """r = 5, one system, batch 64 (m = 150).  MI355X: iters_total 100 = sum klo (sum khi 104), iters_max 25 = max klo (max khi 26)."""
    H, C = a64
    X, info, code = solve(H, C, 5, False, "N", S.TOL, S.MAXIT)
    klo, khi = C.check_converged(X, info, code, 5, False, "N", S.NB_WIDE, S.RESTART_WIDE)
    assert_lu_parity(X, lu_solution(H, C, 5, False), "r=5")
    check_singles(H, C, False, klo, khi, range(5))                   # (a single column has the same m = 150)


def test_converged_restarted_batch(a16):
    """r = 16, one system, batch 16 / restart 6: about twenty cycles.  The builder checks on the reference that GMRES(6) is a fair case
    (at least three cycles to tol, more than 10 % gain per 30 steps throughout: restart 6 was enough, none had to be raised).  MI355X:
    iters_total 1585 = sum klo (sum khi 1647), iters_max 120 = max klo (max khi 130).  Half the columns stop at the start of a cycle
    with a recomputed residual between 0.7 tol and tol."""
    H, C = a16
    assert C.pick_restart("N", False, 16, NB) == RESTART
    X, info, code = solve(H, C, 16, False, "N", S.TOL, S.MAXIT)
    klo, khi = C.check_converged(X, info, code, 16, False, "N", NB, RESTART)
    assert klo[klo > 0].min() >= 3 * RESTART
    assert_lu_parity(X, lu_solution(H, C, 16, False), "r=16 restart 6")
    klo1, khi1 = C.single_bounds("N", False, NB, RESTART)            # (a single column gets m = 111: another solve than its chunk's)
    check_singles(H, C, False, klo1, khi1, [0, 1, 2, 9, 15])


# ----------------------------------------------------------------------------------------------------
# c. a guess direction
# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [4, 16])
def test_guess_direction(a64, r):
    """wae_solve_guess at a regular shift, batch 64 (host recurrence, the guess deflated: m - 1)"""
    H, C = a64
    rng = np.random.default_rng(5 + r)
    B, _ = C.columns(r, True)
    Xp, ip, cp = solve(H, C, r, True, "N", S.TOL, S.MAXIT)
    C.check_residuals(Xp, ip, cp, r, True, "N", what=f"plain r={r}")
    Xlu = lu_solution(H, C, r, True)
    G = rng.standard_normal(B.shape) + 1j * rng.standard_normal(B.shape)
    G0 = G.copy()
    G0[:, 2] = 0                                                     # (column 2 has a right-hand side: it is solved undeflated)
    for name, g in (("random", G), ("one zero column", G0), ("the solution", Xlu)):
        X, info, code = solve(H, C, r, True, "N", S.TOL, S.MAXIT, guess=g)
        C.check_residuals(X, info, code, r, True, "N", what=f"guess r={r}, G {name}", relres=False)
        assert_lu_parity(X, Xlu, f"guess r={r}, G {name}")
        if name == "the solution":
            assert info["iters_max"] <= ip["iters_max"], (info, ip)


# ----------------------------------------------------------------------------------------------------
# d. the Bloch family: complex coefficients
# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", ["N", "C"])
def test_bloch_family(c16, op):
    """MI355X: truncated at k = 5 rho - r_k below 1e-4 of its budget; converged in 18 steps = 3 cycles, iters_total 270 (N) and 269 (C)
    = sum klo."""
    H, C = c16
    X, info, code = solve(H, C, 16, True, op, 1e-300, 5)
    C.check_truncated(X, info, code, 16, 5, True, op, NB, RESTART)
    X, info, code = solve(H, C, 16, True, op, S.TOL, S.MAXIT)
    C.check_converged(X, info, code, 16, True, op, NB, RESTART)
    assert_lu_parity(X, lu_solution(H, C, 16, True, op), f"Bloch op={op}")


# ----------------------------------------------------------------------------------------------------
# e. the switches, one child process each
# ----------------------------------------------------------------------------------------------------
VARIANTS = [("WAE_GMRES_DEVICE", "0"), ("WAE_GMRES_PAIR", "-1"), ("WAE_GMRES_PAIR", "0"), ("WAE_GMRES_SYNC", "1"), ("WAE_NARROW_PAIR", "1")]


@pytest.mark.parametrize("var,val", VARIANTS, ids=[f"{a}={b}" for a, b in VARIANTS])
def test_variants(a16, tmp_path, var, val):
    """each child is held to the reference and the bounds of the default, not to another child"""
    H, C = a16
    for name, arr in (("B16", C.B16), ("ct16", C.ct16), ("ct1", C.ct1)):
        np.save(tmp_path / f"{name}.npy", arr)
    env = dict(os.environ)
    for v, _ in VARIANTS:
        env.pop(v, None)
    env[var] = val
    p = subprocess.run([sys.executable, os.path.join(HERE, "solve_worker.py"), str(tmp_path)], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    with open(tmp_path / "info.json") as f:
        done = json.load(f)
    for r in (16, 8):
        for k in S.ks_for(r):
            for percol in (False, True):
                name = f"trunc_r{r}_k{k}_p{int(percol)}"
                info = done[name]
                C.check_truncated(np.load(tmp_path / f"{name}.npy"), info, info["code"], r, k, percol, "N", NB, RESTART, what=f"{var}={val} {name}")
    info = done["conv_r64"]
    C.check_converged(np.load(tmp_path / "conv_r64.npy"), info, info["code"], 64, True, "N", S.NB_WIDE, S.RESTART_WIDE, what=f"{var}={val} conv_r64")


# ----------------------------------------------------------------------------------------------------
# f. handle state
# ----------------------------------------------------------------------------------------------------
def test_handle_after_a_cycle_cut_short(a16):
    """no state leaks from a cycle cut short: the same handle then solves the same systems with the results of (b)"""
    H, C = a16
    for r, percol, k in ((16, False, 4), (3, True, 5)):
        X, info, code = solve(H, C, r, percol, "N", 1e-300, k)
        C.check_truncated(X, info, code, r, k, percol, "N", NB, RESTART)
        X, info, code = solve(H, C, r, percol, "N", S.TOL, S.MAXIT)
        C.check_converged(X, info, code, r, percol, "N", NB, RESTART, what=f"after a truncated call, r={r}")


def test_no_columns(a16):
    """r = 0 returns WAE_OK with a zeroed info, with and without a guess direction"""
    H, C = a16
    lib, h = _lib.lib(), H.fam.handle
    c = np.ascontiguousarray(C.ct1[0])
    none = np.zeros((H.n[0], 0), dtype=np.complex128, order="F")
    for guess in (False, True):
        info = SolveInfo()
        info.iters_max, info.iters_total, info.n_unconverged, info.levels, info.relres_max = 7, 7, 7, 7, 7.0
        if guess:
            code = lib.wae_solve_guess(h, zptr(c), 1, zptr(none), zptr(none), zptr(none), 0, 0, S.TOL, S.MAXIT, C_.byref(info))
        else:
            code = lib.wae_solve(h, zptr(c), 1, zptr(none), zptr(none), 0, 0, S.TOL, S.MAXIT, C_.byref(info))
        d = info.as_dict()
        assert code == S.WAE_OK and all(d[k] == 0 for k in ("iters_max", "iters_total", "n_unconverged", "levels", "relres_max", "seconds")), (code, d)
    X, info, code = solve(H, C, 3, True, "N", S.TOL, S.MAXIT)       # (and the handle goes on solving)
    C.check_residuals(X, info, code, 3, True, "N", what="after r = 0")
