"""The shift-invert Arnoldi entries (csrc/arnoldi.hip arnoldi_core behind wae_arnoldi_shiftinvert, wae_arnoldi_shiftinvert_batch,
wae_arnoldi_shiftinvert_slots, wae_arnoldi_ritz_to_slot) against the references of tests/_arnref.py, whose docstring states the contract
(a) .. (f) with the lines of arnoldi_core it mirrors; tests/test_arnref.py shows where no GPU is that a clean replay of arnoldi_core meets
it and that ten seeded defects do not.  The kernels underneath are pinned one by one elsewhere (test_gpu_vector_kernels,
test_gpu_gmres_recurrence, test_gpu_multigrid, test_gpu_solve_driver); this module holds the composition: the start and its replacement
by a step of inverse iteration, the early exit on the dominant Ritz residual and the step it takes, the relaxed inner tolerance, dead
columns inside a live batch, the columns of V_out that must not be written, op = C / T with complex coefficients, one coefficient row
of M per system, m = 1, more than 8 systems, and arn_cols after an early exit.

Families (tests/_hier.py, batch 16): A, the annulus "tiny" (1 152 DoF, three levels), and C, the Bloch cell (728 DoF, complex
coefficients, b = 5): the smallest operators with a sparse coarse level, so the pre-step is reachable.  The hierarchy is recovered once
per family; P in the bounds is the V-cycle of tests/_mgref.py on it.  Every call goes through ctypes with the test's own H_out / V_out
filled with the sentinel 3 + 7j (the wrapper hands over zeros and hides what is not written).

Shifts: generic (Z_AB, Z_C and the line through them) and near (_arnref.near_shifts: an eigenvalue of the family found on the host
term matrices, moved off so that the pencil's smallest |lambda| is 1e-5 .. 1e-4 of the next: asserted in the fixtures).  tol = 1e-10,
ritz_tol = 1e-10 where the Ritz test is on.  The near cases are certified on the reference before the device is called
(_arnref.certify); where the pre-step replaces the start the schedule is certified again from the column 0 that came back.

No bound is tuned from a measurement: BETA, the factor 16 and M.budget come from the references that define them.

A mixed batch on family C (two eigenvector starts, two random ones at the near shifts, m = 6) is not among the cases: two of its inner
solves end with WAE_WARN_STAGNATION after 114 iterations (n_unconverged = 2), so rule (f) does not hold there.  That is the solver's
stall rule at a near-singular shift under the hierarchy of b = 0, not a rule of arnoldi_core.

Figures on an MI355X, largest over the module in units of their bounds (A / C):
  a. column 0 against v0 / ||v0||: 0.0022 / 0.0024 of M.budget; the pre-step's solve 0.44 of its bound, a replaced column 1.4 from its
     start (0.1 asked); q of the eigenvector starts 1e-6 .. 1e-5, of the random ones 0.94 .. 1.04.
  b. every exact rule holds, the batch of zeros included (H = 0, columns 0 and 1 zero, the rest zero-filled or the sentinel).
  c. orthonormality 0.0067 / 0.011 of M.budget.
  d. rho_j 0.70 / 0.70 of tol_j (1 + BETA) + 16 u_j -- the solves stop at 0.7 tol_j, as the driver's rule says.
  e. the early exits after 2 steps on both families with tol_1 = 1e-5 (0.1 tol / worst_0, worst_0 = 1e-6); with the pre-step
     tol_1 = 2.5e-7 .. 5.6e-7; every stopping step the reference's.
  f. relres_max 0.70 / 0.70 of max tol_j, n_unconverged 0.
  slots: H identical to the batch entry's (difference 0.0), the combinations of wae_arnoldi_ritz_to_slot at 0.0025 of M.budget.
  eigs_many / eigs_many_slots: eigenvalue errors 7e-10 .. 1.7e-8 (A, |lambda| 5 .. 10) and 2e-8 .. 9e-8 (C, |lambda| 180 .. 320), 0.0026
     / 7e-5 of the weighted first-order bound (the plain one stands at 1e8 and more: its ||r|| runs over the penalty rows of 1e15); the
     residual of the accepted pair 0.0099 / 0.019 of what (d) and (e) imply.
The whole module takes 15 s."""
import ctypes as C_

import numpy as np
import pytest

import _arnref as R
import _mgref as M
from _hier import OPS, SENT, family_a, family_c
from wae_amd import _lib
from wae_amd._lib import SolveInfo, WaeError, zptr
from wae_amd.nlevp.local_solvers import eigs_many, eigs_many_slots

pytestmark = pytest.mark.gpu
NB = 16
TOL, RITZ_TOL, MAXIT = 1e-10, 1e-10, 300
LD, Z = R.LD, R.Z
WORST = {}


class Fam:
    def __init__(self, name, H):
        self.name, self.H, self.fam = name, H, H.fam
        self.ctx = R.Ctx(H.levels, H.transfers, H.w, H.nsweeps)
        self.d, self.T = H.n[0], H.fam.T
        self.cM = np.zeros(self.T, dtype=Z)
        self.cM[-1] = -1.0                                           # M = -terms[-1] (local_solvers._mass)
        self.generic = H.ct64[:16].copy()
        self.near_z = R.near_shifts(name, 4)
        self.near = np.array([H.L.coefficients(z) for z in self.near_z])
        for c in self.near:                                          # the near shifts are near: smallest |lambda| 1e-5 .. 1e-4 of the next
            lam = np.abs(R.pencil_smallest(self.ctx, c, self.cM, "N")[0])
            assert 1e-5 <= lam[0] / lam[1] <= 1e-4, (name, lam)
        self._starts = {}

    def starts(self, kind, cA, op, seed):
        key = (kind, op, seed)
        if key not in self._starts:
            self._starts[key] = R.starts(self.ctx, kind, cA, self.cM, op, np.random.default_rng(seed))
        return self._starts[key]

    def note(self, fig):
        for k, v in R.units_of(fig).items():
            WORST[(self.name, k)] = max(WORST.get((self.name, k), 0.0), float(v))


def report(name):
    print(f"family {name}: largest figures in units of their bounds: " + ", ".join(f"{k[1]} {v:.3g}" for k, v in sorted(WORST.items()) if k[0] == name))


@pytest.fixture(scope="module")
def famA():
    H = family_a(1, distinct=16, batch=NB)
    assert H.nl == 3 and H.n[0] == 1152
    yield Fam("A", H)
    report("A")
    H.L._drop_device()


@pytest.fixture(scope="module")
def famC():
    H = family_c(distinct=16, batch=NB)
    assert H.nl == 3 and H.n[0] == 728
    yield Fam("C", H)
    report("C")
    H.L._drop_device()


@pytest.fixture
def fams(famA, famC):
    return {"A": famA, "C": famC}


def call(F, V0, cA, cM, op, m, tol, ritz_tol, single=False):
    """wae_arnoldi_shiftinvert_batch (single: wae_arnoldi_shiftinvert) on sentinel-filled buffers: (H (nsys, m+1, m), V (nsys, d, m+1),
    info, code)"""
    lib, h = _lib.lib(), F.fam.handle
    nsys = V0.shape[1]
    cA = np.ascontiguousarray(R.rows(cA, nsys))
    cM = np.ascontiguousarray(R.rows(cM, nsys))
    V0f = np.asfortranarray(V0)
    Hb = np.full((nsys, m, m + 1), SENT, dtype=Z)                    # each block column-major (m+1) x m
    Vb = np.full((nsys, m + 1, F.d), SENT, dtype=Z)                  # each block column-major d x (m+1)
    info = SolveInfo()
    if single:
        assert nsys == 1 and ritz_tol == 0
        code = lib.wae_arnoldi_shiftinvert(h, zptr(cA), zptr(cM), m, zptr(V0f), OPS[op], tol, MAXIT, zptr(Hb), zptr(Vb), C_.byref(info))
    else:
        code = lib.wae_arnoldi_shiftinvert_batch(h, nsys, zptr(cA), zptr(cM), m, zptr(V0f), OPS[op], tol, MAXIT, float(ritz_tol), zptr(Hb),
                                                 zptr(Vb), C_.byref(info))
    return Hb.transpose(0, 2, 1), Vb.transpose(0, 2, 1), info.as_dict(), code


def call_slots(F, slot, cols, cA, cM, op, m, tol, ritz_tol):
    lib, h = _lib.lib(), F.fam.handle
    nsys = len(cols)
    cA = np.ascontiguousarray(R.rows(cA, nsys))
    cM = np.ascontiguousarray(R.rows(cM, nsys))
    Hb = np.full((nsys, m, m + 1), SENT, dtype=Z)
    info = SolveInfo()
    cc = np.ascontiguousarray(cols, dtype=np.int32)
    code = lib.wae_arnoldi_shiftinvert_slots(h, nsys, zptr(cA), zptr(cM), m, slot, cc.ctypes.data_as(C_.POINTER(C_.c_int32)), OPS[op], tol, MAXIT,
                                             float(ritz_tol), zptr(Hb), C_.byref(info))
    return Hb.transpose(0, 2, 1), info.as_dict(), code


def run_and_check(F, V0, cA, cM, op, m, ritz_tol, what, single=False):
    H, V, info, code = call(F, V0, cA, cM, op, m, TOL, ritz_tol, single=single)
    assert code == 0, (what, code, info)
    fig = R.check_factorisation(F.ctx, H, V, info, V0, cA, cM, op, m, TOL, ritz_tol, sent=SENT, what=what)
    F.note(fig)
    return H, V, info, fig


def certified(F, V0, cA, cM, op, m, what):
    """the step count the reference schedules for these inputs (rule (e)'s condition asserted, and the reference's own solves at 1e-3 of ritz_tol)"""
    return R.certify(R.reference_run(F.ctx, V0, cA, cM, op, m), m, RITZ_TOL, what)


# ----------------------------------------------------------------------------------------------------
# 1. fixed length: ritz_tol = 0, generic shifts, random starts, one coefficient row of A and of M per system
# ----------------------------------------------------------------------------------------------------
FIXED = [(f, op, m, ns) for f, ops in (("A", "NC"), ("C", "NCT")) for op in ops for m in (1, 3, 6) for ns in (1, 3, 8, 9, 16)]


@pytest.mark.parametrize("f,op,m,ns", FIXED, ids=[f"{f}-{op}-m{m}-n{ns}" for f, op, m, ns in FIXED])
def test_fixed_length_processes(fams, f, op, m, ns):
    """m steps, every solve to tol; the M rows are 1, 2, 1/2 - 1/2 j, ... times the mass coefficients (a library that read row 0 for every
    system misses (d) by 1e10, tests/test_arnref.py); ns = 1 with op N goes through the single-system entry wae_arnoldi_shiftinvert;
    ns = 9 and 16 run the host recurrence with a deflation direction at a width that otherwise goes to the device recurrence."""
    F = fams[f]
    cA = F.generic[:ns]
    cM = R.MFACT[:ns, None] * F.cM[None, :]
    V0 = F.starts("r" * ns, cA, op, 100 + ns)
    _, _, _, fig = run_and_check(F, V0, cA, cM, op, m, 0.0, f"fixed {f} op={op} m={m} nsys={ns}", single=(ns == 1 and op == "N"))
    assert fig["steps"] == m


# ----------------------------------------------------------------------------------------------------
# 2. early exit: near shifts, eigenvector starts perturbed at 1e-6
# ----------------------------------------------------------------------------------------------------
EARLY = [("A", "N", 6), ("A", "N", 1), ("C", "C", 6), ("C", "N", 6)]


def near_case(F, kind, op):
    cA = F.near[:len(kind)]
    return F.starts(kind, cA, op, 7), cA, F.cM[None, :]


@pytest.mark.parametrize("f,op,m", EARLY, ids=[f"{f}-{op}-m{m}" for f, op, m in EARLY])
def test_early_exit_and_relaxed_tolerance(fams, f, op, m):
    F = fams[f]
    V0, cA, cM = near_case(F, "eee", op)
    what = f"early exit {f} op={op} m={m}"
    want = certified(F, V0, cA, cM, op, m, what)
    q = R.start_quality(F.ctx, V0, cA, op)
    print(f"{what}: the reference stops after {want} steps; q of the starts {q}")
    assert np.all(q < 0.01)
    _, _, _, fig = run_and_check(F, V0, cA, cM, op, m, RITZ_TOL, what)
    assert fig["steps"] == want and "a: a poor start is replaced" not in fig
    if m > 1:
        assert want in (2, 3) and fig["tols"][1] > TOL                # relaxed


# ----------------------------------------------------------------------------------------------------
# 3. poor starts: the pre-step
# ----------------------------------------------------------------------------------------------------
PRE_M = 2


@pytest.mark.parametrize("kind", ["rrr", "erre"], ids=["random", "mixed"])
def test_poor_starts_are_replaced_and_good_ones_kept(famA, kind):
    """m = 2: the stop test looks at step 1 only, where the reference stands at 2e-5 .. 4e-5.  At m = 6 the process stops after 2 or 3
    steps on a residual of 5e-11 .. 1.5e-10 after step 2 -- inside [ritz_tol / 4, 4 ritz_tol] for every shift that keeps the pencil's
    ratio within 1e-5 .. 1e-4 (the residual moves with the square of the ratio, the band is 16 wide and the systems of one batch lie a
    factor 3 apart): a case the reference cannot certify, replaced by this one.  MI355X: the pre-step's solve at 0.44 of its bound,
    the kept columns 0 at 0.002 of M.budget, the replaced ones 1.4 away from their starts (0.1 asked), tol_1 = 2.5e-7 / 5.6e-7."""
    F = famA
    V0, cA, cM = near_case(F, kind, "N")
    what = f"pre-step A starts {kind}"
    q = R.start_quality(F.ctx, V0, cA, "N")
    print(f"{what}: q of the starts {q}")
    assert np.array_equal(q > 0.5, [k == "r" for k in kind]) and np.all((q > 0.5) | (q < 0.01))
    H, V, info, fig = run_and_check(F, V0, cA, cM, "N", PRE_M, RITZ_TOL, what)
    assert "a: a poor start is replaced" in fig and ("e" not in kind or "a: column 0 is v0 / ||v0||" in fig)
    # the schedule from the column 0 that came back: certified, and the steps taken are the reference's
    assert fig["steps"] == certified(F, V[:, :, 0].T, cA, cM, "N", PRE_M, what) == PRE_M and fig["tols"][1] > TOL


# ----------------------------------------------------------------------------------------------------
# 4. a dead column inside a live batch; nothing but dead columns
# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", ["A", "C"])
def test_zero_start_column_inside_a_live_batch(fams, f):
    """a zero column is a documented input (wae_solve_info: "a zero right-hand side takes no step")"""
    F = fams[f]
    cA = F.generic[:4]
    V0 = F.starts("rzrr", cA, "N", 31)
    _, _, info, fig = run_and_check(F, V0, cA, F.cM[None, :], "N", 3, 0.0, f"zero column {f} ritz_tol=0")
    assert fig["steps"] == 3 and info["n_unconverged"] == 0
    V0, cA, cM = near_case(F, "ezee", "N")
    want = certified(F, V0, cA, cM, "N", 6, f"zero column {f}")
    _, _, info, fig = run_and_check(F, V0, cA, cM, "N", 6, RITZ_TOL, f"zero column {f} ritz_tol={RITZ_TOL}")
    assert fig["steps"] == want and info["n_unconverged"] == 0


@pytest.mark.parametrize("ritz_tol", [0.0, RITZ_TOL])
def test_nothing_but_zero_columns(famA, ritz_tol):
    """after a live call on the same handle (the work space holds its basis): H zero, the basis zero -- column 1 included, which the step
    that killed every process never wrote --, the rest zero-filled (ritz_tol = 0) or left alone (ritz_tol > 0), WAE_OK"""
    F = famA
    cA = F.generic[:3]
    run_and_check(F, F.starts("rrr", cA, "N", 41), cA, F.cM[None, :], "N", 3, 0.0, "before the zeros")
    V0 = np.zeros((F.d, 3), dtype=Z)
    H, V, info, code = call(F, V0, cA, F.cM[None, :], "N", 3, TOL, ritz_tol)
    assert code == 0 and info["n_unconverged"] == 0 and info["iters_total"] == 0, (code, info)
    fig = R.check_factorisation(F.ctx, H, V, info, V0, cA, F.cM[None, :], "N", 3, TOL, ritz_tol, sent=SENT, what=f"zeros only ritz_tol={ritz_tol}")
    assert not H.any() and not V[:, :, :2].any() and fig["steps"] == 1
    assert (not V.any()) if ritz_tol == 0 else bool(np.all(V[:, :, 2:] == SENT))


# ----------------------------------------------------------------------------------------------------
# 5. the slots entry and wae_arnoldi_ritz_to_slot after an early exit
# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f,kind,op,m", [("A", "eee", "N", 6), ("A", "erre", "N", PRE_M), ("C", "eee", "C", 6)], ids=["A-early", "A-prestep", "C-early-C"])
def test_slots_entry_and_ritz_to_slot_after_an_early_exit(fams, f, kind, op, m):
    """cases 2 and 3 through wae_arnoldi_shiftinvert_slots: H equal to the batch entry's, then wae_arnoldi_ritz_to_slot on the basis the
    call left: steps + 1 vectors, not m + 1 (arn_cols after the early exit).  MI355X: H identical (0.0), the combinations at 0.003 of
    M.budget."""
    F = fams[f]
    fam, ns = F.fam, len(kind)
    V0, cA, cM = near_case(F, kind, op)
    H1, V1, info, fig = run_and_check(F, V0, cA, cM, op, m, RITZ_TOL, f"slots {f} {kind} op={op}: the batch entry")
    steps = fig["steps"]
    assert steps < m or m == PRE_M                                   # (an early exit; the pre-step case takes its two steps)
    rng = np.random.default_rng(3)
    pad = rng.standard_normal((F.d, ns + 2)) + 1j * rng.standard_normal((F.d, ns + 2))
    cols = list(range(ns, 0, -1))                                    # scattered: ns, ..., 1
    pad[:, cols] = V0
    fam.slot_write(0, pad)
    H2, info2, code = call_slots(F, 0, cols, cA, cM, op, m, TOL, RITZ_TOL)
    assert code == 0
    rel = float(np.linalg.norm(H2 - H1) / np.linalg.norm(H1))
    print(f"slots {f} {kind}: H against the batch entry {rel:.2e}")
    assert rel < 1e-9
    R.check_factorisation(F.ctx, H2, None, info2, V0, cA, cM, op, m, TOL, RITZ_TOL, what=f"slots {f} {kind} op={op}: the slots entry")
    # ny = steps + 1 is the basis on the device; steps + 2 is not, although it is <= m + 1 after an early exit
    D0 = rng.standard_normal((F.d, ns + 1)) + 1j * rng.standard_normal((F.d, ns + 1))
    fam.slot_write(1, D0)
    dst = list(range(ns))                                            # column ns stays untouched
    Y = rng.standard_normal((ns, steps + 2)) + 1j * rng.standard_normal((ns, steps + 2))
    with pytest.raises(WaeError):
        fam.ritz_to_slot(Y, 1, dst, normalise=False)
    assert np.array_equal(fam.slot_read(1, 0, ns + 1), D0)
    worst = 0.0
    for normalise in (False, True):
        fam.ritz_to_slot(Y[:, :steps + 1], 1, dst, normalise=normalise)
        got = fam.slot_read(1, 0, ns + 1)
        assert np.array_equal(got[:, ns], D0[:, ns])
        for s in range(ns):
            ref = [V1[s, :, :steps + 1].astype(dt) @ Y[s, :steps + 1].astype(dt) for dt in (LD, Z)]
            if normalise:
                ref = [r / R._norm(r[:, None])[0] for r in ref]
                assert abs(np.linalg.norm(got[:, s]) - 1) <= 1e-14
            one = (np.ones(F.d, dtype=bool),)
            e64 = M.column_errors(ref[1][:, None], ref[0][:, None], one)
            err = M.column_errors(got[:, s:s + 1], ref[0][:, None], one)
            worst = max(worst, float(err[0] / M.budget(e64)[0]))
    print(f"slots {f} {kind}: ritz_to_slot against V y of the batch entry, {worst:.3g} of M.budget")
    assert worst <= 1


# ----------------------------------------------------------------------------------------------------
# 6. the host half on the device
# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f,op", [("A", "N"), ("A", "C"), ("C", "N"), ("C", "C")])
def test_eigs_many_and_eigs_many_slots_on_the_device(fams, f, op):
    """four systems at the near shifts, sigma = 0: the eigenvalues against the pencil's (_arnref.first_order_bounds: scipy's shift-invert
    Arnoldi on the host term matrices, refined by a two-sided Rayleigh quotient in extended precision), each within the first-order bound
    2 ||w|| ||A x - lambda M x|| / |w^H M x| that the reference evaluates in extended precision from the returned Ritz vector x and its
    own left eigenvector w -- and within the same bound weighted with |diag A|, which the penalty rows of 1e15 do not blow up.  The
    residual of the accepted pair, in the preconditioned norm, is held to what (d) and (e) imply for it."""
    F = fams[f]
    ns = 4
    cA = F.near[:ns]
    V0 = F.starts("eeee", cA, op, 7)
    sig = np.zeros(ns)
    out = eigs_many(F.fam, cA, F.cM, V0, OPS[op], sig, tol=RITZ_TOL, stol=TOL)
    F.fam.slot_write(2, V0)
    F.fam.slot_write(3, None, ncols_total=ns)
    outs = eigs_many_slots(F.fam, cA, F.cM, 2, list(range(ns)), OPS[op], sig, 3, tol=RITZ_TOL, stol=TOL)
    Xs = F.fam.slot_read(3, 0, ns)
    worst = 0.0
    for s in range(ns):
        for name, lam, x in (("eigs_many", out[s][0][0], out[s][1][:, 0]), ("eigs_many_slots", outs[s][0], Xs[:, s])):
            assert abs(np.linalg.norm(x) - 1) <= 1e-14
            want, plain, weighted = R.first_order_bounds(F.ctx, cA[s], F.cM, op, lam, x)
            err = abs(lam - want)
            print(f"{name} {f} op={op} system {s}: lambda {complex(lam):.12g}, |error| {err:.2e}, first-order bound {plain:.2e}, weighted {weighted:.2e}")
            assert err <= weighted <= plain, (name, s, lam, want, plain, weighted)
            worst = max(worst, err / weighted)
    WORST[(f, f"6: eigenvalue error op={op}")] = worst
    # the residual of the accepted pair against what (d) and (e) imply.  The first round of eigs_many is this call: summing (d) over the
    # columns with the weights y_j and H y = theta y gives, for x = V_k y,
    #   ||P (op(M) x - theta op(A) x)|| <= sum_j |y_j| tol_j beta_j + ritz_tol |theta| ||P op(A) v_{k+1}||,   beta_j = ||P op(M) v_j||
    cM = F.cM[None, :]
    H, V, info, fig = run_and_check(F, V0, cA, cM, op, 6, RITZ_TOL, f"eigs_many {f} op={op}: its first round")
    k, tols, ref = fig["steps"], fig["tols"], F.ctx.ref(op)
    assert k < 6
    worst = 0.0
    for s in range(ns):
        th, y, res, _ = R.dominant(H[s], k)
        assert res <= RITZ_TOL
        x = V[s, :, :k] @ y
        y, x = y / np.linalg.norm(x), x / np.linalg.norm(x)
        assert abs(np.vdot(x, out[s][1][:, 0])) >= 1 - 1e-12 and abs(np.vdot(x, Xs[:, s])) >= 1 - 1e-12
        assert abs(out[s][0][0] - 1 / th) <= 1e-14 * abs(1 / th)
        z = []
        for dt in (LD, Z):
            X = x.astype(dt)[:, None]
            rhs = F.ctx.lev.apply(cM, op, X, dt) - dt(th) * F.ctx.lev.apply(cA[s:s + 1], op, X, dt)
            cols = [F.ctx.lev.apply(cM, op, V[s, :, :k].astype(dt), dt), F.ctx.lev.apply(cA[s:s + 1], op, V[s, :, k:k + 1].astype(dt), dt), rhs]
            z.append(ref.minv(np.concatenate(cols, axis=1), cA[s:s + 1], dt))
        nz = R._norm(z[0]).astype(np.float64)
        beta, pav, got = nz[:k], nz[k], nz[k + 1]
        u = float(R._norm((z[0] - z[1])[:, k + 1:])[0])
        bound = float(np.sum(np.abs(y) * np.array(tols[:k]) * beta) * (1 + R.S.BETA) + RITZ_TOL * abs(th) * np.linalg.norm(y) * pav) + R.S.U_FACTOR * u
        print(f"eigs_many {f} op={op} system {s}: ||P (op(M) x - theta op(A) x)|| {got:.2e}, bound {bound:.2e} (16 u {R.S.U_FACTOR * u:.1e})")
        assert got <= bound, (s, got, bound)
        worst = max(worst, got / bound)
    WORST[(f, f"6: residual of the accepted pair op={op}")] = worst
