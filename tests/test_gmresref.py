"""The references of tests/_gmresref.py checked where no GPU is: a float64 replay of the GMRES recurrence with Givens rotations,
written from the textbook (Saad, Iterative Methods, 6.5.3, complex form), fed with the same event inputs the device gets, must agree
with the extended-precision least-squares references on every case of tests/test_gpu_gmres_recurrence.py; the largest ratio of their
difference to (j + 2) eps kappa_2 is what the constant of that module's bounds is 8 times of.  And the comparison function of the
GPU module must reject three deliberately wrong replays, so that its tolerances are known to be able to fail."""
import numpy as np
import pytest

import _gmresref as G


def _replay64(case, wrong=None, hist=None):
    """one cycle in float64; returns what G.compare takes.  wrong: None | "sn" (the rotation's sine not conjugated when g is updated)
    | "sub" (H[j+1][j] = r instead of r / ||v_j||) | "hd2" (hd2 without the sub[i-1] c1[i-1] term).  hist: residual history carried
    across cycles (the stagnation rule), one list per column."""
    m, nb = case.m, case.nb
    c128 = np.complex128
    H = np.zeros((m + 1, m, nb), dtype=c128)           # rotated Hessenberg matrix
    cs, sn = np.zeros((m, nb)), np.zeros((m, nb), dtype=c128)
    g = np.zeros((m + 1, nb), dtype=c128)
    g[0] = case.script.beta.astype(np.float64)
    nu = [np.ones(nb)]                                 # norms of the basis vectors as held
    coef, sub = {}, {}                                 # A v_k = sum_i coef[k][i] v_i + sub[k] v_{k+1}
    conv = case.done.copy()
    steps = np.zeros(nb, dtype=int)
    relres = np.zeros(nb)
    hist = [[] for _ in range(nb)] if hist is None else hist
    obs = dict(relres=np.zeros((m, nb)), conv=np.zeros((m, nb), dtype=int), steps=np.zeros((m, nb), dtype=int), pairs={})

    def column(j, hd, r, lim):
        nonlocal conv
        coef[j] = hd[:j + 1]
        flagged = (r > 0) & ((1 / np.where(r > 0, r, 1) > lim) | (1 / np.where(r > 0, r, 1) < 1 / lim))
        sub[j] = np.where(flagged, r, 1.0)
        h = np.zeros((j + 2, nb), dtype=c128)
        for i in range(j + 1):
            h[i] = hd[i] * nu[i] / np.where(nu[j] > 0, nu[j], np.inf)
        h[j + 1] = r if wrong == "sub" else r / np.where(nu[j] > 0, nu[j], np.inf)
        nu.append(np.where(flagged, 1.0, r))
        for i in range(j):                              # the earlier rotations: [c conj(s); -s c]
            a, b = h[i].copy(), h[i + 1].copy()
            h[i] = cs[i] * a + np.conj(sn[i]) * b
            h[i + 1] = -sn[i] * a + cs[i] * b
        a, b = h[j], h[j + 1]
        t = np.sqrt(np.abs(a) ** 2 + np.abs(b) ** 2)
        live = ~conv & (t > 0)
        conv = conv | ~(t > 0)
        tt = np.where(t > 0, t, 1)
        c = np.abs(a) / tt
        s = np.where(np.abs(a) > 0, b * np.conj(a) / np.where(np.abs(a) > 0, np.abs(a) * tt, 1), 1.0)
        gn = -(np.conj(s) if wrong == "sn" else s) * g[j]
        for b_ in np.nonzero(live)[0]:
            cs[j, b_], sn[j, b_] = c[b_], s[b_]
            H[:j + 1, j, b_] = h[:j + 1, b_]
            H[j, j, b_] = c[b_] * a[b_] + np.conj(s[b_]) * h[j + 1, b_]
            g[j + 1, b_] = gn[b_]
            g[j, b_] = c[b_] * g[j, b_]
            steps[b_] = j + 1
            relres[b_] = abs(gn[b_]) / case.bnorm[b_]
            hist[b_].append(relres[b_])
            hn = len(hist[b_])
            if relres[b_] <= 0.7 * case.tol or (hn > 60 and relres[b_] > 0.9 * hist[b_][hn - 31]):
                conv[b_] = True
        obs["relres"][j], obs["conv"][j], obs["steps"][j] = relres, conv, steps

    for ev in case.script.events:
        j = ev["j"]
        if ev["kind"] == "step":
            hd = ev["hd"].astype(c128)
            column(j, hd, hd[j + 1].real, case.lim)
        else:
            c1, c2, gram, norms = (ev[k].astype(c128) for k in ("c1", "c2", "gram", "norms"))
            q = np.array(nu[:j + 1]) ** 2
            uu = gram[0].real - (np.abs(c1) ** 2 * q).sum(axis=0)
            u12 = gram[1] - (np.conj(c1) * c2 * q).sum(axis=0)
            alpha = np.where(uu > 1e-28 * gram[0].real, u12 / np.where(uu > 0, uu, 1), 0)
            c2m = c2 - alpha * c1
            column(j, c1, norms[0].real, 1e300)
            hd2 = np.zeros((j + 2, nb), dtype=c128)
            for i in range(j + 2):
                t = c2[i].copy() if i <= j else alpha.copy()
                for k in range(i, j + 1):
                    t -= coef[k][i] * c1[k]
                if i >= 1 and wrong != "hd2":
                    t -= sub[i - 1] * c1[i - 1]
                hd2[i] = t
            obs["pairs"][j] = (alpha, c2m, hd2)
            column(j + 1, hd2, norms[1].real, case.lim)
    out = np.zeros((m, nb), dtype=c128)                 # y = R^-1 g over each column's steps, against the basis as held
    for b in range(nb):
        k = steps[b]
        if k:
            y = np.linalg.solve(np.triu(H[:k, :k, b]), g[:k, b]) if k > 1 else g[:1, b] / H[0, 0, b]
            out[:k, b] = y / np.array([nu[i][b] for i in range(k)])
    obs["out"] = out
    return obs


def _replays(wrong=None):
    hist = [[], []]                                     # (carried through the restart cycles of the stagnation case)
    stall = {c.name: _replay64(c, wrong, hist) for c in G.stall_cycles()[0]}
    for c in G.all_cases():
        yield c, stall[c.name] if c.name in stall else _replay64(c, wrong)


def test_textbook_replay_agrees_with_least_squares():
    worst = 0.0
    for case, obs in _replays():
        assert G.compare(case, obs) == [], case.name
        worst = max(worst, G.ratios(case, obs))
    print(f"largest |replay - least squares| / ((j + 2) eps kappa_2): {worst:.3f}   C_BOUND = {G.C_BOUND:.3f}")
    assert worst <= G.C_BOUND / 4, worst
    assert abs(G.C_BOUND - 8 * G.RATIO_MEASURED) < 1e-12


@pytest.mark.parametrize("wrong, case", [("sn", "width12"), ("sub", "width12"), ("hd2", "pair2")])
def test_comparison_rejects_wrong_replays(wrong, case):
    c = {x.name: x for x in G.all_cases()}[case]
    assert G.compare(c, _replay64(c)) == []
    bad = G.compare(c, _replay64(c, wrong))
    assert bad, (wrong, case)
    want = {"sn": "solution", "sub": "residual estimate", "hd2": "hd2"}[wrong]
    assert any(want in s for s in bad), bad


def test_reference_self_checks():
    """threshold ties, the uu floor, the 0.7 tol band and the slow column's rate are asserted while the cases are built; the
    algebraic hd2 and alpha equal the projections in extended precision (n = 24, j = 2)"""
    c = G.pair_case(2)
    ev = next(e for e in c.script.events if e["kind"] == "pair" and e["j"] == 2)
    T, V = c.pairs[2], c.script.V
    q = np.array([G._sq(V[i]) for i in range(3)])
    uu = ev["gram"][0] - (np.abs(ev["c1"]) ** 2 * q).sum(axis=0)
    u12 = ev["gram"][1] - (np.conj(ev["c1"]) * ev["c2"] * q).sum(axis=0)
    assert np.max(np.abs(u12 / uu - T.alpha)) < 5e-18 * max(1.0, float(np.max(np.abs(T.alpha))))
    Al = c.A.astype(G.LD)
    for i in range(4):
        t = ev["c2"][i].copy() if i <= 2 else T.alpha.copy()
        for k in range(i, 3):
            t = t - G._proj(V[i], G._mv(Al, V[k])) * ev["c1"][k]
        if i >= 1:
            t = t - G._proj(V[i], G._mv(Al, V[i - 1])) * ev["c1"][i - 1]
        assert np.max(np.abs(t - T.hd2[i])) < 5e-18 * max(1.0, float(np.max(np.abs(T.hd2)))), i
    with pytest.raises(ValueError):
        G.guard(np.array([0.25 * (1 + 1e-8)], dtype=G.RD), 4.0)
    cases, (cyc, j) = G.stall_cycles()
    assert (cyc, j) == (3, 12) and cases[4].done[0] and not cases[3].done[0]
