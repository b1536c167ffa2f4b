"""The recurrence kernels of the lock-step GMRES (vec.hip gmres_init, gmres_step, gmres_rescale, gmres_clear_rescale,
gmres_pair_coef, gmres_solve_y), run as scripts of single launches on caller-supplied data (wae_debug_gmres) against the
extended-precision references of tests/_gmresref.py: an Arnoldi process with real vectors, the least-squares problem GMRES solves
and projections of Op v_{j+1}.  The references contain no Givens rotation and no statement of the kernels; whole solves cannot pin
these kernels, because a wrong rotation or coefficient only moves the residual ESTIMATE, which a solve's tolerance hides.

Tolerances, none of them taken from the kernels:
  flags, counts, masks, frozen state, untouched vectors      exact / bit for bit
  alpha, c2m, hd2 of a pair step    4 (j + 4) eps (sum of the magnitudes of the terms) per entry; alpha carries gram[0]/uu
  residual estimates                c (j + 2) eps kappa_2(Hbar_j) beta/bnorm
  solve_y solutions                 c (j + 2) eps kappa_2(Hbar_j) ||x_ref||, and ||r - A x||/bnorm within the same times ||A|| ||x_ref||/bnorm
with kappa_2 of the true normalised Hessenberg matrix and c = 8.16: 8 times the largest ratio (1.02) of |float64 textbook replay -
extended-precision least squares| to (j + 2) eps kappa_2 over every case of this module, measured on the CPU by
tests/test_gmresref.py, which fails if that ratio drifts above c/4.  The factor 8 allows another, equally valid order of operations.

Operators: A_b = s_b (I + 0.3 G_b / sqrt(n)) per column, n = 24, m = 12, everything seeded (tests/_gmresref.py holds the cases, and
asserts while it builds them that no case depends on a tie of the range guard or of the stopping test).
solve_y is run with ju = m and with ju = the largest step count of the batch (the value the solver passes when a cycle ends early);
ju below a column's own steps cannot happen in the solver (ju is the cycle's step count, steps[b] <= it), so there is no such case."""
import numpy as np
import pytest

import _gmresref as G
from wae_amd import _lib

pytestmark = pytest.mark.gpu

SENT = 3 + 7j


def z(a):
    return np.ascontiguousarray(np.asarray(a).astype(np.complex128))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def add_cycle(sc, case, poison=None):
    """INIT, the case's events and SOLVE_Y(m) appended to the script; returns the event indices.  poison = (event number, column):
    a NaN in that column's hd[0]"""
    idx = dict(init=sc.init(z(case.script.beta), case.done, case.use_mask), events=[])
    for k, ev in enumerate(case.script.events):
        if ev["kind"] == "step":
            hd = z(ev["hd"])
            if poison is not None and poison[0] == k:
                hd[0, poison[1]] = np.nan
            idx["events"].append(sc.step(ev["j"], hd, case.tol, case.lim, z(ev["Vnew"]), case.use_mask))
        else:
            idx["events"].append(sc.pair(ev["j"], z(ev["c1"]), z(ev["c2"]), z(ev["gram"]), z(ev["norms"]), case.tol, case.lim, z(ev["W1"]),
                                         z(ev["W2"]), case.use_mask))
    idx["solve"] = sc.solve_y(case.m)
    return idx


def run_case(case, poison=None):
    sc = _lib.GmresScript(case.nb, case.m, case.n)
    idx = add_cycle(sc, case, poison)
    _, res = sc.run(case.bnorm)
    return sc, idx, res


def observed(case, res, idx, hist0=None):
    """what G.compare takes, from the snapshots; the state after the first step of a pair from the residual history and the step
    counts after the pair.  hist0[b]: the history length of column b before this cycle (default 0)."""
    m, nb = case.m, case.nb
    obs = dict(relres=np.zeros((m, nb)), conv=np.zeros((m, nb), dtype=int), steps=np.zeros((m, nb), dtype=int), pairs={})
    hist0 = np.zeros(nb, dtype=int) if hist0 is None else hist0
    for e, ev in zip(idx["events"], case.script.events):
        s, j = res.events[e], ev["j"]
        if ev["kind"] == "pair":
            took2 = s["steps"] == j + 2
            obs["steps"][j] = np.minimum(s["steps"], j + 1)
            obs["conv"][j] = np.where(took2, 0, s["conv"])
            first = res.hist[np.minimum(hist0 + j, res.hist.shape[0] - 1), np.arange(nb)]         # (recorded by the first step, if taken)
            obs["relres"][j] = np.where(took2, first, s["relres"])
            obs["pairs"][j] = (s["alpha"], s["c2m"], s["hd2"])
            j += 1
        obs["relres"][j], obs["conv"][j], obs["steps"][j] = s["relres"], s["conv"], s["steps"]
    obs["out"] = res.events[idx["solve"]]["out"]
    return obs


def check_state(case, res, idx, first_cycle=True):
    """masks, counts, the rows of sv / vsq, the range guard and the raw recurrence after every event: exact"""
    nb, m = case.nb, case.m
    chunk = np.arange(nb) >> 3
    nch = (nb + 7) // 8

    def check_mask(s, active, what):
        assert s["status"][0] == active.sum(), what
        want = np.zeros(nch, dtype=bool)
        np.logical_or.at(want, chunk, active)
        assert np.array_equal(s["cmask"] != 0, want if case.use_mask else np.ones(nch, dtype=bool)), what
        assert s["status"][2] == 0, what + ": renormalisation still pending"

    s = res.events[idx["init"]]
    check_mask(s, ~case.done, "init")
    assert np.array_equal(s["conv"], case.done.astype(int)) and np.all(s["steps"] == 0) and s["status"][1] == 0
    assert np.all(s["sv"][0] == 1) and np.all(s["vsq"][0] == 1)
    ok = ~case.breakdown
    for e, ev in zip(idx["events"], case.script.events):
        s, j = res.events[e], ev["j"]
        what = f"{case.name} event at {j}"
        last = j + (1 if ev["kind"] == "pair" else 0)
        check_mask(s, ~case.done & (last < case.conv_step), what)
        assert s["status"][1] == 0, what
        norms = [z(ev["hd"])[j + 1].real] if ev["kind"] == "step" else list(z(ev["norms"]).real)
        vecs = [s["Vnew"]] if ev["kind"] == "step" else [s["W1"], s["W2"]]
        given = [z(ev["Vnew"])] if ev["kind"] == "step" else [z(ev["W1"]), z(ev["W2"])]
        for k, (r, flagged) in enumerate(zip(norms, ev["resc"])):
            pos = r > 0
            rr = np.where(pos, r, 1.0)
            assert np.array_equal(s["sv"][k], np.where(flagged, 1.0, np.where(pos, 1.0 / rr, 0.0))), what
            assert np.array_equal(s["vsq"][k], np.where(flagged, 1.0, np.where(pos, 1.0 / (rr * rr), 0.0)).astype(np.complex128)), what
            assert not first_cycle or np.array_equal(res.sub[j + k], np.where(flagged, r, 1.0)), what
            assert np.array_equal(bits(vecs[k][:, ~flagged]), bits(given[k][:, ~flagged])), what + ": an unflagged vector changed"
            if flagged.any():
                want = given[k][:, flagged] / r[flagged][None, :]
                assert np.all(np.abs(vecs[k][:, flagged] - want) <= G.EPS * np.abs(want)), what + ": renormalised vector"
        assert np.array_equal(s["rescale"], np.where(ev["resc"][-1], norms[-1], 0.0).astype(np.complex128)), what
        # the unnormalised recurrence as the pair steps read it
        if not first_cycle:                             # (the final state holds the last cycle's)
            continue
        if ev["kind"] == "step":
            assert np.array_equal(bits(res.Hraw[j, :j + 1]), bits(z(ev["hd"])[:j + 1])), what
        else:
            assert np.array_equal(bits(res.Hraw[j, :j + 1]), bits(z(ev["c1"]))), what
            assert np.array_equal(bits(res.Hraw[j + 1, :j + 2][:, ok]), bits(s["hd2"][:, ok])), what
    if first_cycle:
        s = res.events[idx["events"][-1]]
        assert np.array_equal(s["iters"], s["steps"]) and np.array_equal(s["histlen"], s["steps"]) and np.all(s["stalled"] == 0)


def check_case(case, poison=None):
    sc, idx, res = run_case(case, poison)
    bad = G.compare(case, observed(case, res, idx))
    assert bad == [], bad
    check_state(case, res, idx)
    return sc, idx, res


@pytest.mark.parametrize("nb", G.NBS)
def test_residual_estimate_and_stopping_test(nb):
    """a single column, ragged last chunks and every thread of the workgroup: the residual estimate after every step equals the
    least-squares minimum / bnorm, conv turns 1 at exactly the step where the reference first drops to 0.7 tol, solve_y gives the
    reference minimiser of each column's own stopping step"""
    case = G.width_case(nb)
    live = case.conv_step[case.conv_step < case.m]
    assert nb < 8 or len(set(live)) >= 2, "columns must converge at different steps"
    sc, idx, res = check_case(case)
    # solve_y with the step count of a cycle that ended early: the same rows, nothing past ju
    ju = int(min(case.m, case.conv_step.max() + 1))
    e2 = sc.solve_y(ju)
    _, res2 = sc.run(case.bnorm)
    a, b = res.events[idx["solve"]]["out"], res2.events[e2]["out"]
    assert np.array_equal(bits(a[:ju]), bits(b[:ju])) and np.all(b[ju:] == SENT)


def test_frozen_columns():
    """once converged, a column's g, R columns, cs and sn are bit-identical ever after: the state after k steps against the state
    after all m, on the columns converged before step k (a script cut after k steps is the full script's state at that point:
    columns never mix and nothing is random)"""
    case = G.width_case(65)
    states = []
    for k in range(1, case.m + 1):
        sc = _lib.GmresScript(case.nb, case.m, case.n)
        sc.init(z(case.script.beta), case.done, case.use_mask)
        for ev in case.script.events[:k]:
            sc.step(ev["j"], z(ev["hd"]), case.tol, case.lim, z(ev["Vnew"]), case.use_mask)
        states.append(sc.run(case.bnorm)[1])
    full = states[-1]
    seen = 0
    for k in range(1, case.m):
        frozen = case.conv_step < k
        seen += int(frozen.sum())
        for name in ("g", "R", "cs", "sn"):
            a, b = getattr(states[k - 1], name)[..., frozen], getattr(full, name)[..., frozen]
            assert np.array_equal(bits(a), bits(b)), (name, k)
    assert seen > 0


@pytest.mark.parametrize("use_mask", [1, 0])
def test_chunk_mask_and_count(use_mask):
    """done on entry for whole chunks and single columns: those take no step and get exact zeros from solve_y; cmask follows the
    activity of each 8-column chunk with use_mask = 1 and stays 1 without, status[0] counts either way (check_state)"""
    case = G.mask_case(use_mask)
    sc, idx, res = check_case(case)
    last = res.events[idx["events"][-1]]
    assert np.all(last["steps"][case.done] == 0) and np.all(last["iters"][case.done] == 0)
    assert np.all(res.events[idx["solve"]]["out"][:, case.done] == 0)
    if use_mask:
        masks = np.array([res.events[e]["cmask"] for e in [idx["init"]] + idx["events"]])
        assert np.all(masks[:, [1, 4]] == 0) and masks[0, 0] == 1 and len({tuple(r) for r in masks}) >= 3


@pytest.mark.parametrize("lim", [4.0, 1e300])
def test_range_guard(lim):
    """lim = 4 with scales spread over [0.2, 5]: some columns renormalise at most steps and others never; flagged vectors are divided
    by the norm passed in, unflagged ones stay bit-identical, sv = vsq = 1 and sub = r for the flagged (check_state), and the residual
    estimates of the later steps still match the reference, which normalised the same vectors.  lim = 1e300 touches nothing."""
    case = G.guard_case(lim)
    count = np.sum([ev["resc"][0] for ev in case.script.events], axis=0)
    if lim == 4.0:
        assert np.any(count >= case.m // 2) and np.any(count == 0) and np.any((count > 0) & (count < case.m // 2))
    else:
        assert np.all(count == 0)
    check_case(case)


@pytest.mark.parametrize("pair_from", [0, 2, 3])
def test_pair_steps(pair_from):
    """pair events from j = 0, from j = 2 (the last pair ends exactly at m in both) and from j = 3 after three single steps (a single
    step closes the cycle): alpha, c2m, hd2 against the projections, the two residual estimates of every pair against the
    least-squares minima, Hraw[j] = c1 and sub[j] = 1 (check_state)"""
    case = G.pair_case(pair_from)
    kinds = [(ev["kind"], ev["j"]) for ev in case.script.events]
    assert ("pair", pair_from) in kinds and (pair_from == 3) == (kinds[-1] == ("step", case.m - 1))
    check_case(case)


@pytest.mark.parametrize("pair_from", [None, 0])
def test_exact_breakdown(pair_from):
    """A_b = 2 I in one column of a 16-wide batch: the new vector is exactly 0; the column converges at step 1 with relres = 0, alpha =
    0 in a pair, no NaN flag, solve_y gives r/2; the other 15 columns are checked as usual"""
    case = G.breakdown_case(pair_from)
    b = G.BREAK_COL
    sc, idx, res = check_case(case)
    for e in idx["events"]:
        s = res.events[e]
        assert s["conv"][b] == 1 and s["steps"][b] == 1 and s["relres"][b] == 0.0 and s["status"][1] == 0
    if pair_from == 0:
        assert all(res.events[e]["alpha"][b] == 0 for e in idx["events"])
    out = res.events[idx["solve"]]["out"]
    assert np.all(out[1:, b] == 0)
    x = G.solution(case, out)[b]
    half = case.r[b].astype(G.LD) / 2
    assert np.sqrt(G._sq(x - half)) <= 4 * G.EPS * np.sqrt(G._sq(half))


def test_zero_right_hand_side():
    case = G.zero_rhs_case()
    b = G.BREAK_COL
    assert case.script.beta[b] == 0 and case.bnorm[b] == 1 and case.done[b]
    sc, idx, res = check_case(case)
    last = res.events[idx["events"][-1]]
    assert last["steps"][b] == 0 and last["conv"][b] == 1 and last["status"][1] == 0
    assert np.all(res.events[idx["solve"]]["out"][:, b] == 0)


def test_nan_column_stays_alone():
    """a NaN in one column's hd sets status[1], retires that column and changes no output of any other column"""
    case = G.breakdown_case(None)
    b, at = 9, 3
    assert case.conv_step[b] > at
    _, idx, clean = run_case(case)
    _, _, dirty = run_case(case, poison=(at, b))
    others = np.arange(case.nb) != b
    for k, e in enumerate(idx["events"]):
        s, c = dirty.events[e], clean.events[e]
        assert s["status"][1] == (1 if k >= at else 0)
        if k >= at:
            assert s["conv"][b] == 1 and s["steps"][b] == at
            assert s["status"][0] == c["status"][0] - (1 if c["conv"][b] == 0 else 0)
        for name in ("relres", "conv", "steps", "iters", "histlen", "stalled", "rescale", "sv", "vsq", "Vnew"):
            assert np.array_equal(s[name][..., others], c[name][..., others]), (name, k)
    for name in ("R", "cs", "sn", "g", "sv", "vsq", "Hraw", "sub", "hist"):
        assert np.array_equal(getattr(dirty, name)[..., others], getattr(clean, name)[..., others]), name
    assert np.array_equal(dirty.events[idx["solve"]]["out"][:, others], clean.events[idx["solve"]]["out"][:, others])


def test_stagnation_verdict():
    """Column 0: the cyclic shift of size 64 and r = e_1, whose residual stays 1; column 1: the circle operator with tol = 0, which
    improves by more than 0.9 per 30 steps (asserted by the reference) and must never be flagged.  Five restart cycles of 16 steps
    against ONE state: histlen carries across the cycles, stalled[0] and conv[0] turn 1 exactly at the 61st recorded step."""
    cases, (scyc, sj) = G.stall_cycles()
    m = G.STALL_M
    sc = _lib.GmresScript(2, m, G.STALL_N, histcap=G.STALL_CYCLES * m + 8)
    idxs = [add_cycle(sc, c) for c in cases]
    _, res = sc.run(cases[0].bnorm)
    taken = np.zeros(2, dtype=int)
    for cyc, (case, idx) in enumerate(zip(cases, idxs)):
        bad = G.compare(case, observed(case, res, idx))
        assert bad == [], bad
        check_state(case, res, idx, first_cycle=False)
        for e, ev in zip(idx["events"], case.script.events):
            s, j = res.events[e], ev["j"]
            taken += case.active(j)
            stalled_now = (cyc, j) >= (scyc, sj)
            assert np.array_equal(s["histlen"], taken) and np.array_equal(s["iters"], taken), (cyc, j)
            assert s["stalled"][0] == int(stalled_now) and s["stalled"][1] == 0 and s["conv"][1] == 0, (cyc, j)
            assert s["conv"][0] == int(stalled_now or case.done[0]), (cyc, j)
    assert taken[0] == 61 and taken[1] == G.STALL_CYCLES * m
    assert np.all(res.hist[:61, 0] == 1.0) and np.all(res.hist[61:, 0] == SENT.real)


def test_refusals():
    """bad sizes: WAE_ERR_INVALID with a message, before anything is uploaded or launched"""
    n, m = 4, 3

    def script(nb, m_, build):
        sc = _lib.GmresScript(nb, m_, n)
        build(sc, max(nb, 1))
        return sc

    def init(sc, nb):
        sc.init(np.ones(nb, dtype=complex), np.zeros(nb), 1)

    def step(j):
        return lambda sc, nb: (init(sc, nb), sc.step(j, np.ones((max(j, 0) + 2, nb), dtype=complex), 1e-3, 1e300, np.ones((n, nb), dtype=complex), 1))

    def pair(j):
        return lambda sc, nb: (init(sc, nb), sc.pair(j, np.ones((j + 1, nb), dtype=complex), np.ones((j + 1, nb), dtype=complex),
                                                     np.ones((3, nb), dtype=complex), np.ones((2, nb), dtype=complex), 1e-3, 1e300,
                                                     np.ones((n, nb), dtype=complex), np.ones((n, nb), dtype=complex), 1))

    def unknown(sc, nb):
        init(sc, nb)
        sc.ev[0][0] = 9

    bad = [(0, m, init, 0), (257, m, init, 0), (4, 0, init, 0), (4, m, step(m), 0), (4, m, step(-1), 0), (4, m, pair(m - 1), 0),
           (4, m, lambda sc, nb: sc.solve_y(0), 0), (4, m, lambda sc, nb: sc.solve_y(m + 1), 0), (4, m, step(1), 1), (4, m, unknown, 0)]
    for nb, m_, build, short in bad:
        sc = script(nb, m_, build)
        code, res = sc.run(np.ones(max(nb, 1)), raise_on_error=False, short=short)
        assert code == _lib.WAE_ERR_INVALID and res is None, (nb, m_, short)
        assert len(_lib.lib().wae_last_error()) > 0
    code, res = script(4, m, step(0)).run(np.ones(4))       # ... and the smallest valid script runs
    assert code == 0 and np.all(res.events[1]["steps"] == 1)
