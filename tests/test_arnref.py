"""tests/_arnref.py where no GPU is: `apply_S` and `arnoldi_ref` against dense extended-precision algebra on a 192-DoF annulus, the clean
complex128 `replay` of arnoldi_core inside every bound of `check_factorisation` in every case family of tests/test_gpu_arnoldi.py,
DISCRIMINATION -- every seeded defect of _arnref.DEFECTS outside a bound, by the printed factor -- and the host half of the Arnoldi
entries (nlevp/local_solvers.py _ritz, eigs_many, eigs_many_slots) on a stand-in family that runs the replay.

The hierarchy is the synthetic one of tests/test_solveref.py (384 DoF, 384 -> 84 -> 21), so the pre-step is reachable.  Its near shifts
are found here: a secant iteration on the pencil's smallest eigenvalue, then moved off so that it is 3e-5 of the next one.

Measured.  The clean replay, largest figure in units of its bound over the twelve cases: (a) 0.005 of M.budget, the pre-step's solve
0.34, (c) 0.014, (d) and (f) 0.68 -- the solves stop at 0.7 tol_j.  The seeded defects miss by: m_row0 1.0e10 and m_not_conjugated 1.4e10
(d); stop_late 47 and stop_early 1e4 (e); prestep_never 5e14 and prestep_all 8.6e11 (a); one_gs_pass 1.5e8 (c); dead_not_zeroed and
complex_subdiagonal break an exact rule of (b).  relax_loose misses (d) and (f) by 1.4: tol / worst against 0.1 tol / worst are
allowances exactly 10 apart and a solve that stops at 0.7 of its own lands below 7 -- a factor 10 is out of reach for that one defect,
which is asserted at 1.25.  apply_S: backward error 3e-20, 1e-18 .. 1e-17 from a dense extended-precision solve; arnoldi_ref: H against
V^H S V 7e-18."""
import numpy as np
import pytest
import scipy.linalg as sla

import _arnref as R
import _mgref as M
from _hier import LINE, Z_AB
from _tilecheck import annulus_coeffs
from test_solveref import syn  # noqa: F401  (the fixture)
from wae_amd.helmholtz import annulus
from wae_amd.nlevp.local_solvers import EigsError, _ritz, eigs_many, eigs_many_slots

LD, Z = R.LD, R.Z
TOL, RITZ_TOL = 1e-10, 1e-10
CM = np.array([0, 0, 0, 0, -1.0], dtype=Z)                            # M = -terms[-1]


def coeffs(z):
    return annulus_coeffs(np.atleast_1d(z), tau=2e-4)


@pytest.fixture(scope="module")
def ctx(syn):
    c = R.Ctx(*syn.args, syn.w, syn.nsweeps)
    assert c.multilevel and c.n == 384
    # a near shift of this family: secant iteration on lambda_min(z) from Z_AB
    z0, z1 = Z_AB, Z_AB * (1 + 1e-3)
    f0 = R.pencil_smallest(c, coeffs(z0)[0], CM, "N")[0][0]
    for _ in range(12):
        f1 = R.pencil_smallest(c, coeffs(z1)[0], CM, "N")[0][0]
        if abs(f1) < 1e-6:
            break
        z0, z1, f0 = z1, z1 - f1 * (z1 - z0) / (f1 - f0), f1
    lam = R.pencil_smallest(c, coeffs(z1)[0], CM, "N")[0]
    slope = abs(f1 - f0) / abs(z1 - z0) if z1 != z0 else 1.0
    slope = abs(R.pencil_smallest(c, coeffs(z1 + 1e-2)[0], CM, "N")[0][0]) / 1e-2
    c.near = z1 + 3e-5 * abs(lam[1]) / slope * (1 + 0.25 * np.arange(4))
    for z in c.near:
        lam = np.abs(R.pencil_smallest(c, coeffs(z)[0], CM, "N")[0])
        assert 1e-5 <= lam[0] / lam[1] <= 1e-4, lam
    return c


@pytest.fixture(scope="module")
def small():
    """192 DoF, one level: for the dense checks"""
    pb = annulus.build(grid=(8, 6, 4), tau=2e-4)
    T = pb["terms"]
    terms = [T["M"].tocsr(), T["K"].tocsr(), T["C"].tocsr(), T["Q"].tocsr(), (-T["M"]).tocsr()]
    c = R.Ctx([M.Level(terms)], [], dict(w_pre=0.7, w_post=0.9, w_light=0.5), 1)
    assert c.n <= 200
    return c


def dense_op(c, row, op, dt=LD):
    row = np.asarray(row, dtype=Z)
    A = sum(dt(ck) * t.toarray().astype(dt) for ck, t in zip(row, c.terms) if ck != 0)
    return A if op == "N" else (A.T if op == "T" else A.conj().T)


# ----------------------------------------------------------------------------------------------------
# the two references against dense algebra
# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", ["N", "T", "C"])
def test_apply_S_against_a_dense_extended_solve(small, op):
    c = small
    rng = np.random.default_rng(3)
    V = rng.standard_normal((c.n, 3)) + 1j * rng.standard_normal((c.n, 3))
    cA = coeffs((Z_AB + LINE)[[0, 20, 40]])
    cM = R.MFACT[[0, 2, 3], None] * CM[None, :]
    X, res = R.apply_S(c, V, cA, cM, op)
    for s in range(3):
        want = M.dense_solve(dense_op(c, cA[s], op), (dense_op(c, cM[s], op) @ V[:, s].astype(LD))[:, None])[:, 0]
        err = float(np.max(np.abs(X[:, s] - want)) / np.max(np.abs(want)))
        print(f"apply_S op={op} system {s}: residual reached {res[s]:.1e}, distance from the dense extended solve {err:.1e}")
        assert res[s] <= 1e-17 and err <= 1e-15, (op, s, res[s], err)
    if op == "C":                                                    # the coefficients are conjugated with the matrix
        bad = R.apply_S(c, V, cA, cM.conj(), op)[0]
        assert np.max(np.abs(bad[:, 1] - X[:, 1])) > 1e-3 * np.max(np.abs(X[:, 1]))


def test_arnoldi_ref_against_dense_algebra(small):
    c = small
    m = 5
    lam0 = R.pencil_smallest(c, coeffs(Z_AB)[0], CM, "N")[0]
    cA, cM = coeffs(Z_AB), CM[None, :]
    rng = np.random.default_rng(4)
    v0 = rng.standard_normal((c.n, 1)) + 1j * rng.standard_normal((c.n, 1))
    out = R.reference_run(c, v0, cA, cM, "N", m)
    Sd = M.dense_solve(dense_op(c, cA[0], "N"), dense_op(c, cM[0], "N"))
    V, H = out["V"][0], out["H"][0]
    G = V.conj().T @ V
    assert np.max(np.abs(G - np.eye(m + 1))) <= 1e-17
    Hd = V[:, :m].conj().T @ (Sd @ V[:, :m])
    scale = float(np.max(np.abs(Hd)))
    err = float(np.max(np.abs(Hd - H[:m, :m])) / scale)
    rel = float(np.max(np.abs(Sd @ V[:, :m] - V @ H)) / scale)
    print(f"arnoldi_ref: H - V^H S V {err:.1e}, S V - V H {rel:.1e} of max |H|")
    assert err <= 1e-16 and rel <= 1e-16
    assert np.all(H[np.arange(1, m + 1), np.arange(m)].imag == 0) and np.all(H[np.arange(1, m + 1), np.arange(m)].real > 0)
    # Ritz values converge to the pencil's: dense eig on the rows without a penalty (a dense QZ loses the small eigenvalues to the 1e15)
    free = np.abs(dense_op(c, cA[0], "N", Z).diagonal()) < 1e10
    lam = sla.eig(dense_op(c, cA[0], "N", Z)[np.ix_(free, free)], dense_op(c, cM[0], "N", Z)[np.ix_(free, free)], right=False)
    lam = lam[np.argsort(np.abs(lam))]
    assert abs(lam[0] - lam0[0]) <= 1e-8 * abs(lam0[0])
    long = R.reference_run(c, v0, cA, cM, "N", 30)
    th = long["theta"][:, 0]
    d = np.abs(1 / th - lam[0]) / abs(lam[0])
    print(f"arnoldi_ref: dominant Ritz value against the dense pencil after 5, 15, 30 steps: {d[4]:.1e} {d[14]:.1e} {d[29]:.1e}; residual {long['res'][29, 0]:.1e}")
    assert d[29] <= 1e-8 and d[29] < d[4]


# ----------------------------------------------------------------------------------------------------
# the case families of the GPU module, on the replay
# ----------------------------------------------------------------------------------------------------
def case(ctx, name):
    """(V0, cA, cM, op, m, tol, ritz_tol) of a named case"""
    rng = np.random.default_rng(len(name) + 7)
    if name.startswith("generic"):                                   # generic-N-m3-n3
        _, op, m, ns = name.split("-")
        m, ns = int(m[1:]), int(ns[1:])
        cA = coeffs((Z_AB + LINE)[::4][:ns])
        cM = R.MFACT[:ns, None] * CM[None, :]
        return R.starts(ctx, "r" * ns, cA, cM, op, rng), cA, cM, op, m, TOL, 0.0
    kind, op, m = {"near": ("eee", "N", 6), "near-C": ("eee", "C", 6), "near-m1": ("eee", "N", 1), "poor": ("rrr", "N", 6),
                   "mixed": ("erre", "N", 6), "zero": ("rzrr", "N", 3), "zero-ritz": ("ezee", "N", 6), "zeros": ("zzz", "N", 3)}[name]
    ns = len(kind)
    cA = coeffs(ctx.near[:ns])
    cM = np.repeat(CM[None, :], ns, axis=0)
    rt = 0.0 if name in ("zero", "zeros") else RITZ_TOL
    if name == "zero":
        cA = coeffs((Z_AB + LINE)[::4][:ns])
    return R.starts(ctx, kind, cA, cM, op, rng), cA, cM, op, m, TOL, rt


CASES = ["generic-N-m1-n1", "generic-N-m3-n3", "generic-C-m3-n3", "generic-T-m3-n3", "near", "near-C", "near-m1", "poor", "mixed", "zero", "zero-ritz",
         "zeros"]


@pytest.mark.parametrize("name", CASES)
def test_clean_replay_meets_the_contract(ctx, name):
    V0, cA, cM, op, m, tol, rt = case(ctx, name)
    live = np.any(V0 != 0, axis=0)
    want = None
    if live.any():
        ref = R.reference_run(ctx, V0, cA, cM, op, m)
        want = R.certify(ref, m, rt, name)
        print(f"{name}: the reference stops after {want} steps, residuals {ref['res'].max(axis=1)}, separation {ref['sep'].min(axis=1)[1:]}")
    H, V, info = R.replay(ctx, V0, cA, cM, op, m, tol, rt)
    fig = R.check_factorisation(ctx, H, V, info, V0, cA, cM, op, m, tol, rt, what=name)
    if name in ("near", "near-C", "zero-ritz"):
        assert fig["steps"] in (2, 3) and fig["steps"] == want and np.all(fig["q"] < 0.01) and fig["tols"][1] > tol
    if name in ("poor", "mixed"):
        # (the pre-step changes the start: the schedule is certified from the column 0 that came back)
        again = R.reference_run(ctx, V[np.nonzero(live)[0], :, 0].T, cA, cM, op, m)
        assert fig["steps"] == R.certify(again, m, rt, name) == 3
        assert np.array_equal(fig["q"] > 0.5, [k == "r" for k in ("rrr" if name == "poor" else "erre")])
        assert "a: a poor start is replaced" in fig and (name == "poor" or "a: column 0 is v0 / ||v0||" in fig)
    if name == "near-m1":
        assert fig["steps"] == 1 and "q" not in fig
    if name == "zeros":
        assert not H.any() and not V.any()


SEEDED = [("m_row0", "generic-N-m3-n3"), ("m_not_conjugated", "generic-C-m3-n3"), ("stop_late", "near"), ("stop_early", "near"),
          ("relax_loose", "near"), ("prestep_never", "poor"), ("prestep_all", "near"), ("prestep_all", "mixed"), ("dead_not_zeroed", "zero"),
          ("dead_not_zeroed", "zero-ritz"), ("one_gs_pass", "near"), ("complex_subdiagonal", "generic-N-m3-n3")]


@pytest.mark.parametrize("defect,name", SEEDED, ids=[f"{d}-{n}" for d, n in SEEDED])
def test_seeded_defect_misses_the_contract(ctx, defect, name):
    V0, cA, cM, op, m, tol, rt = case(ctx, name)
    H, V, info = R.replay(ctx, V0, cA, cM, op, m, tol, rt, defects=(defect,))
    fig = R.check_factorisation(ctx, H, V, info, V0, cA, cM, op, m, tol, rt, enforce=False)
    rule, factor = R.worst_unit(fig)
    print(f"{defect} on {name}: misses '{rule}' by a factor {factor:.3g}")
    # relax_loose: tol / worst against 0.1 tol / worst -- the two allowances differ by exactly 10, and a solve that stops at 0.7 of its
    # own tolerance lands below 7: a miss by 10 is arithmetically out of reach for this one defect (measured: 1.4)
    assert factor >= (10 if defect != "relax_loose" else 1.25), (defect, name, rule, factor, R.units_of(fig))
    with pytest.raises(AssertionError):
        R.check_factorisation(ctx, H, V, info, V0, cA, cM, op, m, tol, rt)


# ----------------------------------------------------------------------------------------------------
# the host half: _ritz, eigs_many, eigs_many_slots on a stand-in family that runs the replay
# ----------------------------------------------------------------------------------------------------
def pencil_pair(ctx, cA, op, target):
    """(the eigenvalue of op(A) x = lambda op(M) x nearest `target`, 10 x its condition number as an eigenvalue of op(A)^-1 op(M):
    ||y|| ||x|| / |y^H x| with y = op(M)^H w, w the left eigenvector) -- what an eigenvalue from Ritz pairs of residual tol may be off by"""
    lam, X = R.pencil_smallest(ctx, cA, CM, op, k=3)
    i = int(np.argmin(np.abs(lam - target)))
    opl = {"N": "C", "C": "N"}[op]
    lamw, Wl = R.pencil_smallest(ctx, cA, CM, opl, k=3)
    w = Wl[:, int(np.argmin(np.abs(np.conj(lamw) - lam[i])))]
    y = R.op_matrix(ctx.terms, CM, op).conj().T @ w
    return lam[i], 10 * np.linalg.norm(y) * np.linalg.norm(X[:, i]) / abs(np.vdot(y, X[:, i])), X[:, i] / np.linalg.norm(X[:, i])


@pytest.mark.parametrize("op", ["N", "C"])
@pytest.mark.parametrize("slots", [False, True], ids=["eigs_many", "eigs_many_slots"])
def test_eigs_many_on_the_replay(ctx, op, slots):
    """lambda = sigma + 1 / theta on the right, conj(sigma) + 1 / theta on the left, against the pencil's eigenvalue; unit Ritz vectors"""
    ns = 3
    rng = np.random.default_rng(21)
    cA = coeffs(ctx.near[:ns])
    sig = np.array([40 + 25j, -30 + 10j, 15 - 35j])
    shifted = cA - sig[:, None] * CM[None, :]
    V0 = R.starts(ctx, "eee", shifted, CM, op, rng)
    fam = R.FakeFam(ctx)
    if slots:
        fam.slot_write(0, np.column_stack([np.zeros(ctx.n), V0]))
        fam.slot_write(1, None, ncols_total=ns + 1)
        out = eigs_many_slots(fam, cA, CM, 0, [1, 2, 3], R.OPS[op], sig, 1, tol=RITZ_TOL, stol=TOL)
        X = fam.slot_read(1, 1, ns)
        assert not fam.slot_read(1, 0, 1).any()
    else:
        out = eigs_many(fam, cA, CM, V0, R.OPS[op], sig, tol=RITZ_TOL, stol=TOL)
        X = np.column_stack([o[1][:, 0] for o in out])
    for s in range(ns):
        lam = complex(np.ravel(out[s][0])[0])
        want, kappa, xref = pencil_pair(ctx, cA[s], op, np.conj(sig[s]) if op == "C" else sig[s])
        centre = np.conj(sig[s]) if op == "C" else sig[s]
        err = abs(lam - want) / abs(want - centre)
        print(f"{'slots' if slots else 'host'} op={op} system {s}: lambda {lam:.6g}, off by {err:.2e} of |lambda - sigma|, bound {kappa * RITZ_TOL:.2e}")
        assert err <= kappa * RITZ_TOL, (op, s, lam, want)
        assert abs(np.linalg.norm(X[:, s]) - 1) <= 1e-14
        assert abs(np.vdot(xref, X[:, s])) >= 1 - 1e-8, (op, s, abs(np.vdot(xref, X[:, s])))
        # the first-order bounds of the GPU module, on the shifted pencil
        lam0, plain, weighted = R.first_order_bounds(ctx, shifted[s], CM, op, lam - centre, X[:, s])
        print(f"    refined reference {lam0 + centre:.12g} (scipy's {want:.12g}); |error| {abs(lam - centre - lam0):.2e}, bounds {plain:.2e} / weighted {weighted:.2e}")
        assert abs(lam - centre - lam0) <= weighted <= plain
    # the sign rule is seen: with sigma instead of conj(sigma) on the left the eigenvalue is off by 2 |Im sigma|
    assert abs(2 * sig[0].imag) > 1e3 * kappa * RITZ_TOL * abs(want - centre)


def test_eigs_many_restarts_and_fails(ctx):
    """m is capped at 6: a start that needs more steps is restarted from its Ritz vector; with stalled inner solves the systems that
    are not done come back as EigsError"""
    ns = 2
    rng = np.random.default_rng(5)
    V0 = None
    for far in (16000, 32000):                             # further from the eigenvalue until the reference needs 7 .. 12 steps
        cA = coeffs(ctx.near[:ns] + far * (ctx.near[1] - ctx.near[0]))
        V0 = R.starts(ctx, "rr", cA, CM, "N", rng) if V0 is None else V0
        ref = R.reference_run(ctx, V0, cA, CM[None, :], "N", 12)
        need = [int(np.argmax(ref["res"][:, s] <= RITZ_TOL)) + 1 if ref["res"][-1, s] <= RITZ_TOL else 99 for s in range(ns)]
        print(f"{far} offsets away the reference needs {need} steps; residuals after 6 steps {ref['res'][5]}")
        if all(6 < k <= 12 for k in need) and np.all(ref["res"][5] > 4 * RITZ_TOL):
            break
    else:
        raise AssertionError("no case that needs a restart")
    fam = R.FakeFam(ctx)
    out = eigs_many(fam, cA, CM, V0, 0, np.zeros(ns), tol=RITZ_TOL, stol=TOL)
    assert len(fam.calls) >= 2 and fam.calls[0] == (ns, 6)
    restarted = fam.calls[1][0]                                      # (the pre-step improves a random start: not every system needs the restart)
    for s in range(ns):
        want, kappa, _ = pencil_pair(ctx, cA[s], "N", 0)
        assert abs(out[s][0][0] - want) <= kappa * RITZ_TOL * abs(want), (s, out[s][0], want)
    fam = R.FakeFam(ctx)
    fam.slot_write(0, V0)
    fam.slot_write(1, None, ncols_total=ns)
    out = eigs_many_slots(fam, cA, CM, 0, [0, 1], 0, np.zeros(ns), 1, tol=RITZ_TOL, stol=TOL)
    assert len(fam.calls) >= 2
    for s in range(ns):
        want, kappa, _ = pencil_pair(ctx, cA[s], "N", 0)
        assert abs(out[s][0] - want) <= kappa * RITZ_TOL * abs(want), (s, out[s][0], want)
    bad = R.FakeFam(ctx, unconverged=True)
    out = eigs_many(bad, cA, CM, V0, 0, np.zeros(ns), tol=RITZ_TOL, stol=TOL)
    assert sum(isinstance(o, EigsError) for o in out) == restarted and len(bad.calls) == 1
    bad = R.FakeFam(ctx, unconverged=True)
    bad.slot_write(0, V0)
    bad.slot_write(1, None, ncols_total=ns)
    out = eigs_many_slots(bad, cA, CM, 0, [0, 1], 0, np.zeros(ns), 1, tol=RITZ_TOL, stol=TOL)
    assert sum(isinstance(o, EigsError) for o in out) == restarted and len(bad.calls) == 1


def test_eigs_many_with_a_zero_start_column(ctx):
    """a zero start column (a dead process: H = 0) reports through _ritz as done -- theta = 0, no finite eigenvalue -- and its
    neighbours return what they return without it"""
    rng = np.random.default_rng(8)
    cA = coeffs(ctx.near[:3])
    V0 = R.starts(ctx, "eze", cA, CM, "N", rng)
    fam = R.FakeFam(ctx)
    with np.errstate(all="ignore"):
        out = eigs_many(fam, cA, CM, V0, 0, np.zeros(3), tol=RITZ_TOL, stol=TOL)
    alone = eigs_many(R.FakeFam(ctx), cA[[0, 2]], CM, V0[:, [0, 2]], 0, np.zeros(2), tol=RITZ_TOL, stol=TOL)
    assert len(fam.calls) == 1 and not np.isfinite(out[1][0][0])
    for a, b in zip((out[0], out[2]), alone):
        assert abs(a[0][0] - b[0][0]) <= 1e-12 * abs(b[0][0]) and abs(np.vdot(a[1][:, 0], b[1][:, 0])) >= 1 - 1e-12
        want, kappa, _ = pencil_pair(ctx, cA[0 if a is out[0] else 2], "N", 0)
        assert abs(a[0][0] - want) <= kappa * RITZ_TOL * abs(want)


def test_ritz_on_hand_made_hessenberg_matrices():
    rng = np.random.default_rng(2)
    m = 5
    H = np.triu(rng.standard_normal((m + 1, m)) + 1j * rng.standard_normal((m + 1, m)), -1)
    H[np.arange(1, m + 1), np.arange(m)] = np.abs(H[np.arange(1, m + 1), np.arange(m)])
    ev = lambda k: sorted(np.linalg.eigvals(H[:k, :k]), key=lambda t: -abs(t))
    # every step taken, not converged
    theta, Y, mm, k, done = _ritz(H, 1, 1e-10, 100)
    assert mm == m and k == 1 and not done and np.allclose(theta, ev(m)) and np.all(np.abs(theta[:-1]) >= np.abs(theta[1:]))
    assert np.allclose(H[:m, :m] @ Y[:, 0], theta[0] * Y[:, 0])
    # ... and converged when the residual |h_{m+1,m}| |y_m| is below tol |theta|
    Hc = H.copy()
    Hc[m, m - 1] = 1e-13
    assert _ritz(Hc, 1, 1e-10, 100)[4] and not _ritz(Hc, 1, 1e-16, 100)[4]
    # trailing zero columns: an early exit after 3 steps; the residual comes from h_{4,3}
    He = H.copy()
    He[:, 3:] = 0
    theta, Y, mm, k, done = _ritz(He, 1, 1e-10, 100)
    assert mm == 3 and np.allclose(theta, ev(3)) and Y.shape == (3, 3) and not done
    He[3, 2] = 1e-14
    assert _ritz(He, 1, 1e-10, 100)[4]
    # a zero subdiagonal in the middle: an invariant subspace after 2 steps -- cut there and done, whatever follows
    Hz = H.copy()
    Hz[2, 1] = 0
    theta, Y, mm, k, done = _ritz(Hz, 1, 1e-10, 100)
    assert mm == 2 and done and np.allclose(theta, ev(2))
    theta, Y, mm, k, done = _ritz(Hz, 3, 1e-10, 100)                 # more pairs wanted than the subspace holds
    assert mm == 2 and k == 2 and done
    # m >= d: the Krylov space is the whole space
    assert _ritz(H, 1, 1e-10, m)[4] and _ritz(H, 1, 1e-10, m - 1)[4] and not _ritz(H, 1, 1e-10, m + 1)[4]
    # nothing but zeros (a zero start): one step, theta = 0, done
    theta, Y, mm, k, done = _ritz(np.zeros((m + 1, m), dtype=complex), 1, 1e-10, 100)
    assert mm == 1 and theta[0] == 0 and done
