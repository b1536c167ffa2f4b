"""References of the recurrence kernels of the lock-step GMRES (tests/test_gpu_gmres_recurrence.py), in numpy's extended precision
(clongdouble), each restating what a kernel MEANS rather than replaying its statements: an Arnoldi process with real vectors whose
basis is left unnormalised, the least-squares problem GMRES solves, and projections of Op v_{j+1}.  None of them contains a Givens
rotation.  Functions return the value together with the magnitude sums its rounding bound is built from.  The cases of the GPU
module and the function that compares an observed recurrence with the references are here too, so that tests/test_gmresref.py can run
both on the CPU against a float64 replay of the textbook recurrence."""
import functools

import numpy as np

LD = np.clongdouble
RD = np.longdouble
EPS = float(np.finfo(np.float64).eps)

# Constant of the bounds on residual estimates and solutions, c (j + 2) eps kappa_2(Hbar_j): 8 times the largest ratio of
# |float64 textbook replay - extended-precision least squares| to (j + 2) eps kappa_2 over every case below (RATIO_MEASURED, by
# tests/test_gmresref.py::test_textbook_replay_agrees_with_least_squares, which fails if the ratio drifts above C_BOUND / 4).
RATIO_MEASURED = 1.02
C_BOUND = 8 * RATIO_MEASURED


def _sq(x):
    a = np.abs(x)
    return (a * a).sum(axis=-1)


def _dot(a, b):
    return (np.conj(a) * b).sum(axis=-1)


def _mv(A, v):
    return np.einsum("bij,bj->bi", A, v)


def _safe_div(a, b):
    """a / b per column, 0 where b is 0"""
    ok = b != 0
    return np.where(ok, a / np.where(ok, b, 1), 0)


def _proj(v, w):
    """v^H w / ||v||^2 per column (0 for a zero v)"""
    return _safe_div(_dot(v, w), _sq(v))


def guard(nrm, lim):
    """the range guard as the kernel documents it: a new vector of norm r is normalised when 1/r > lim or 1/r < 1/lim.  Raises if
    any column lies within 1e-6 relative of a threshold, so that no case depends on a tie."""
    svn = _safe_div(np.ones_like(nrm), nrm)
    pos = svn > 0
    for t in (RD(lim), 1 / RD(lim)):
        if np.any(pos & (np.abs(svn / t - 1) < 1e-6)):
            raise ValueError("a column's 1/norm lies within 1e-6 of a guard threshold")
    return pos & ((svn > RD(lim)) | (svn < 1 / RD(lim)))


class Script:
    """what arnoldi_script returns: events (the inputs of the hook's events, extended precision), the basis V as the solver holds it
    (list of (nb, n); normalised where the guard flagged it), beta"""


def arnoldi_script(A, r, m, lim, pair_from=None):
    """The lazy Arnoldi process of A (nb, n, n) from r (nb, n) with real vectors: v_0 = r/beta, hd_i = v_i^H w / ||v_i||^2,
    v_{j+1} = w - sum hd_i v_i left unnormalised unless the range guard flags it, hd_{j+1} = ||v_{j+1}||.  From step pair_from on (while
    two steps fit the cycle) pair events: w1 = A v_j, w2 = A w1, c_k = V^H w_k (scaled), the Gram entries and the two new vectors."""
    Al, rl = A.astype(LD), r.astype(LD)
    nb, n = rl.shape
    S = Script()
    S.beta = np.sqrt(_sq(rl))
    V = [_safe_div(rl, S.beta[:, None])]
    S.events = []
    j = 0
    while j < m:
        if pair_from is not None and j >= pair_from and j + 2 <= m:
            w1 = _mv(Al, V[j])
            w2 = _mv(Al, w1)
            c1 = np.array([_proj(V[i], w1) for i in range(j + 1)])
            c2 = np.array([_proj(V[i], w2) for i in range(j + 1)])
            gram = np.array([_sq(w1).astype(LD), _dot(w1, w2), _sq(w2).astype(LD)])
            u1, u2 = w1.copy(), w2.copy()
            for i in range(j + 1):
                u1 = u1 - c1[i][:, None] * V[i]
                u2 = u2 - c2[i][:, None] * V[i]
            alpha = _proj(u1, u2)
            v2 = u2 - alpha[:, None] * u1
            norms = np.array([np.sqrt(_sq(u1)), np.sqrt(_sq(v2))])
            resc = guard(norms[1], lim)                      # (the middle vector is never renormalised)
            S.events.append(dict(kind="pair", j=j, c1=c1, c2=c2, gram=gram, norms=norms, W1=u1.T.copy(), W2=v2.T.copy(),
                                 resc=[np.zeros(nb, dtype=bool), resc], uu_ratio=_safe_div(_sq(u1), _sq(w1))))
            V.append(u1)
            V.append(np.where(resc[:, None], _safe_div(v2, norms[1][:, None]), v2))
            j += 2
        else:
            w = _mv(Al, V[j])
            hd = np.zeros((j + 2, nb), dtype=LD)
            v = w.copy()
            for i in range(j + 1):
                hd[i] = _proj(V[i], w)
                v = v - hd[i][:, None] * V[i]
            nrm = np.sqrt(_sq(v))
            hd[j + 1] = nrm
            resc = guard(nrm, lim)
            S.events.append(dict(kind="step", j=j, hd=hd, Vnew=v.T.copy(), norm=nrm, resc=[resc]))
            V.append(np.where(resc[:, None], _safe_div(v, nrm[:, None]), v))
            j += 1
    S.V = V
    return S


def min_residual(A, r, Vk):
    """min_y ||r - A V_k y|| and its minimiser per column, by a QR of A V_k (modified Gram-Schmidt, every vector orthogonalised
    twice) in extended precision.  Vk: (k, nb, n).  Returns (minimum (nb,), y (k, nb)); a vector of A V_k that vanishes gets y = 0."""
    Al, rl = A.astype(LD), r.astype(LD)
    k, nb = len(Vk), rl.shape[0]
    Q, Rm = [], np.zeros((k, k, nb), dtype=LD)
    for i in range(k):
        a = _mv(Al, Vk[i].astype(LD))
        for _ in range(2):
            for p in range(i):
                h = _dot(Q[p], a)
                a = a - h[:, None] * Q[p]
                Rm[p, i] += h
        nrm = np.sqrt(_sq(a))
        Rm[i, i] = nrm
        Q.append(_safe_div(a, nrm[:, None]))
    res, c = rl.copy(), np.zeros((k, nb), dtype=LD)
    for _ in range(2):
        for i in range(k):
            h = _dot(Q[i], res)
            res = res - h[:, None] * Q[i]
            c[i] += h
    y = np.zeros((k, nb), dtype=LD)
    for i in range(k - 1, -1, -1):
        s = c[i].copy()
        for q in range(i + 1, k):
            s = s - Rm[i, q] * y[q]
        y[i] = _safe_div(s, Rm[i, i])
    return np.sqrt(_sq(res)), y


def history(A, r, V, m):
    """min_residual for the spaces of dimension 1..m: minima (m, nb) and minimisers x_k = V_k y_k (m, nb, n)"""
    nb, n = r.shape
    res, x = np.zeros((m, nb), dtype=RD), np.zeros((m, nb, n), dtype=LD)
    for k in range(1, m + 1):
        res[k - 1], y = min_residual(A, r, V[:k])
        for i in range(k):
            x[k - 1] += y[i][:, None] * V[i]
    return res, x


def kappa(A, V, m):
    """kappa_2 of the true normalised Hessenberg matrices Hbar_j = Q_{j+2}^H A Q_{j+1}, j = 0..m-1 (float64 SVD of the
    extended-precision matrix); nan where a basis vector vanishes (exact breakdown)"""
    Al = A.astype(LD)
    Q = np.array([_safe_div(v, np.sqrt(_sq(v))[:, None]) for v in V[:m + 1]])          # (m+1, nb, n)
    AQ = np.array([_mv(Al, q) for q in Q[:m]])
    H = np.einsum("ibn,jbn->bij", np.conj(Q), AQ).astype(np.complex128)                 # (nb, m+1, m)
    dead = np.array([_sq(v) == 0 for v in V[:m + 1]])                                   # (m+1, nb)
    out = np.full((m, H.shape[0]), np.nan)
    for j in range(m):
        sv = np.linalg.svd(H[:, :j + 2, :j + 1], compute_uv=False)
        ok = ~dead[:j + 2].any(axis=0)
        out[j, ok] = sv[ok, 0] / sv[ok, -1]
    return out


class PairTruth:
    pass


def pair_truth(A, V, j):
    """What the pair step's coefficient kernel must produce, from projections: alpha = v_{j+1}^H u2 / ||v_{j+1}||^2 with
    u2 = w2 - V c2, c2m = c2 - alpha c1, hd2_i = v_i^H (A v_{j+1}) / ||v_i||^2 for i <= j+1.  mag_*: the sums of the magnitudes of the
    terms of the kernel's algebraic forms (uu = w1^H w1 - sum |c1_i|^2 ||v_i||^2, u12 alike, hd2_i = c2_i or alpha - sum_k Hraw[k][i] c1_k
    - sub[i-1] c1_{i-1} with Hraw[k][i], sub[k] the coefficients of A v_k), which the rounding bounds are built from."""
    Al = A.astype(LD)
    T = PairTruth()
    w1 = _mv(Al, V[j])
    w2 = _mv(Al, w1)
    c1 = np.array([_proj(V[i], w1) for i in range(j + 1)])
    c2 = np.array([_proj(V[i], w2) for i in range(j + 1)])
    u2 = w2.copy()
    for i in range(j + 1):
        u2 = u2 - c2[i][:, None] * V[i]
    T.alpha = _proj(V[j + 1], u2)
    T.c2m = c2 - T.alpha[None, :] * c1
    Av = _mv(Al, V[j + 1])
    T.hd2 = np.array([_proj(V[i], Av) for i in range(j + 2)])
    q = np.array([_sq(V[i]) for i in range(j + 1)])
    T.gram0 = _sq(w1)
    T.uu = _sq(V[j + 1])
    T.mag_uu = T.gram0 + (np.abs(c1) ** 2 * q).sum(axis=0)
    T.mag_u12 = np.abs(_dot(w1, w2)) + (np.abs(c1) * np.abs(c2) * q).sum(axis=0)
    T.mag_c2m = np.abs(c2) + np.abs(T.alpha)[None, :] * np.abs(c1)
    T.c1 = c1
    mag = np.zeros((j + 2, c1.shape[1]), dtype=RD)
    mag[:j + 1] = np.abs(c2)
    mag[j + 1] = np.abs(T.alpha)
    for k in range(j + 1):
        Avk = _mv(Al, V[k])
        for i in range(k + 2):
            if i <= j + 1:
                mag[i] += np.abs(_proj(V[i], Avk)) * np.abs(c1[k])       # i <= k: Hraw[k][i];  i = k + 1: sub[k]
    T.mag_hd2 = mag
    return T


def pair_bounds(T, j):
    """rounding bounds 4 (j + 4) eps (sum of the magnitudes of the terms) per entry; the bound on alpha = u12/uu carries gram[0]/uu
    through mag_uu/uu, and c2m and hd2[j+1] carry the bound on alpha"""
    f = 4 * (j + 4) * EPS
    b_alpha = f * _safe_div(T.mag_u12 + np.abs(T.alpha) * T.mag_uu, T.uu)
    b_c2m = f * T.mag_c2m + np.abs(T.c1) * b_alpha[None, :]
    b_hd2 = f * T.mag_hd2
    b_hd2[j + 1] = b_hd2[j + 1] + b_alpha
    return b_alpha, b_c2m, b_hd2


# ---------------------------------------------------------------------------------------------------------------------------------
# the cases of the GPU module
# ---------------------------------------------------------------------------------------------------------------------------------
def default_operator(rng, nb, n, smin=0.5, smax=2.0):
    """A_b = s_b (I + 0.3 G_b / sqrt(n)), G_b complex Gaussian, s_b log-uniform in [smin, smax]: a stand-in for a preconditioned
    operator whose condition number is small"""
    G = rng.standard_normal((nb, n, n)) + 1j * rng.standard_normal((nb, n, n))
    s = np.exp(rng.uniform(np.log(smin), np.log(smax), nb))
    return s[:, None, None] * (np.eye(n)[None] + 0.3 * G / np.sqrt(n))


def circle_operator(rng, n):
    """I + 0.9 U diag(e^{i theta}) U^H: normal, spectrum on the circle of radius 0.9 about 1 (GMRES gains 0.9 per step, no faster)"""
    q, _ = np.linalg.qr(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))
    th = 2 * np.pi * (np.arange(n) + 0.5) / n
    return np.eye(n) + 0.9 * (q * np.exp(1j * th)[None, :]) @ q.conj().T


def rhs(rng, nb, n):
    return rng.standard_normal((nb, n)) + 1j * rng.standard_normal((nb, n))


def choose_tol(rel, live, at):
    """a tolerance from the reference's own history: 0.7 tol is the median over the live columns of the reference at step `at`, moved
    up in steps of 0.3 % until no reference value lies within 1e-3 relative of it (asserted)"""
    t = float(np.median(rel[at, live]))
    for _ in range(200):
        if not np.any(np.abs(rel[:, live] / t - 1) < 1e-3):
            break
        t *= 1.003
    assert not np.any(np.abs(rel[:, live] / t - 1) < 1e-3)
    return t / 0.7


class Case:
    """one cycle: operators, right-hand sides, script and references.  rel (m, nb): reference residual / bnorm; x (m, nb, n): the
    minimisers; kap (m, nb); conv_step[b]: the first step (0-based) whose reference is <= 0.7 tol, m if none (`stop` overrides it for
    columns another rule retires); active[j][b]: b takes step j."""

    def __init__(self, name, A, r, m, lim=1e300, pair_from=None, done=None, use_mask=1, tol_at=None, tol=None, bnorm=None, seed=0,
                 breakdown=()):
        self.name, self.A, self.r, self.m, self.lim, self.pair_from, self.use_mask = name, A, r, m, lim, pair_from, use_mask
        self.nb, self.n = r.shape
        nb = self.nb
        self.done = np.zeros(nb, dtype=bool) if done is None else np.asarray(done, dtype=bool)
        self.breakdown = np.zeros(nb, dtype=bool)
        self.breakdown[list(breakdown)] = True
        self.script = arnoldi_script(A, r, m, lim, pair_from)
        beta = self.script.beta.astype(np.float64)
        self.bnorm = beta * np.random.default_rng(seed + 977).uniform(1.0, 3.0, nb) if bnorm is None else np.asarray(bnorm, dtype=np.float64)
        res, self.x = history(A, r, self.script.V, m)
        self.rel = (res / self.bnorm.astype(RD))
        self.kap = kappa(A, self.script.V, m)
        self.scale = beta / self.bnorm
        live = ~self.done & ~self.breakdown
        self.tol = tol if tol is not None else choose_tol(self.rel, live, m // 2 if tol_at is None else tol_at)
        if self.tol > 0:
            assert not np.any(np.abs(self.rel[:, live] / RD(0.7 * self.tol) - 1) < 1e-3)
        below = self.rel <= RD(0.7 * self.tol)
        self.conv_step = np.where(below.any(axis=0), below.argmax(axis=0), m)
        self.pairs = {}
        for ev in self.script.events:
            if ev["kind"] == "pair":
                assert np.all(ev["uu_ratio"][~self.breakdown] >= 1e-3), "uu floor"
                self.pairs[ev["j"]] = pair_truth(A, self.script.V, ev["j"])
        self.anorm = np.linalg.norm(A, 2, axis=(1, 2))

    def active(self, j):
        """columns that take step j"""
        return ~self.done & (j <= self.conv_step)


NBS = (1, 7, 8, 12, 64, 65, 200, 256)
N, M = 24, 12


@functools.lru_cache(maxsize=None)
def width_case(nb):
    rng = np.random.default_rng(1000 + nb)
    return Case(f"width{nb}", default_operator(rng, nb, N), rhs(rng, nb, N), M, seed=nb)


@functools.lru_cache(maxsize=None)
def mask_case(use_mask):
    """done on entry for the whole chunks 1 and 4 and for single columns"""
    nb = 44
    rng = np.random.default_rng(2000)
    done = np.zeros(nb, dtype=bool)
    done[8:16] = True
    done[32:40] = True
    done[[0, 21, 43]] = True
    return Case(f"mask{use_mask}", default_operator(rng, nb, N), rhs(rng, nb, N), M, done=done, use_mask=use_mask, seed=5)


@functools.lru_cache(maxsize=None)
def guard_case(lim):
    nb = 40
    rng = np.random.default_rng(3000)
    return Case(f"guard{lim:g}", default_operator(rng, nb, N, 0.2, 5.0), rhs(rng, nb, N), M, lim=lim, seed=6)


@functools.lru_cache(maxsize=None)
def pair_case(pair_from):
    nb = 20
    rng = np.random.default_rng(4000 + pair_from)
    return Case(f"pair{pair_from}", default_operator(rng, nb, N), rhs(rng, nb, N), M, pair_from=pair_from, seed=7)


BREAK_COL = 5


@functools.lru_cache(maxsize=None)
def breakdown_case(pair_from):
    """A_b = 2 I in column BREAK_COL of a 16-wide batch: the new vector is exactly 0"""
    nb = 16
    rng = np.random.default_rng(5000)
    A = default_operator(rng, nb, N)
    A[BREAK_COL] = 2 * np.eye(N)
    r = rhs(rng, nb, N)
    r[BREAK_COL] = 0                                  # 16 entries out of {1, i, -1, -i}: beta = 4 and v_0 = r/4, w = 2 v_0, hd_0 = 2 are exact
    r[BREAK_COL, :16] = 1j ** rng.integers(0, 4, 16)
    c = Case(f"breakdown{pair_from}", A, r, M, pair_from=pair_from, seed=8, breakdown=(BREAK_COL,))
    assert all(np.all(np.asarray(ev["W1" if ev["kind"] == "pair" else "Vnew"])[:, BREAK_COL] == 0) for ev in c.script.events)
    return c


@functools.lru_cache(maxsize=None)
def zero_rhs_case():
    nb = 16
    rng = np.random.default_rng(6000)
    r = rhs(rng, nb, N)
    r[BREAK_COL] = 0
    done = np.zeros(nb, dtype=bool)
    done[BREAK_COL] = True
    c = Case("zero_rhs", default_operator(rng, nb, N), r, M, done=done, seed=9, breakdown=(BREAK_COL,),
             bnorm=np.where(done, 1.0, np.sqrt(_sq(r.astype(LD))).astype(np.float64) * 1.5))
    return c


STALL_N, STALL_M, STALL_CYCLES = 64, 16, 5


@functools.lru_cache(maxsize=None)
def stall_cycles():
    """Column 0: the cyclic shift of size 64 and r = e_1 (the residual stays 1); column 1: the circle operator with tol = 0, which
    keeps improving by more than 0.9 per 30 steps (asserted).  STALL_CYCLES restart cycles of STALL_M steps: one Case per cycle, the
    residual of column 1 carried in extended precision.  Returns (cases, stall): stall = (cycle, step) of the 61st recorded step."""
    n, m = STALL_N, STALL_M
    rng = np.random.default_rng(7000)
    A = np.zeros((2, n, n), dtype=np.complex128)
    A[0] = np.roll(np.eye(n), 1, axis=0)
    A[1] = circle_operator(rng, n)
    r = np.zeros((2, n), dtype=LD)
    r[0, 0] = 1
    r[1] = rhs(rng, 1, n)[0]
    bnorm = np.sqrt(_sq(r)).astype(np.float64)
    cases, hist = [], []
    for cyc in range(STALL_CYCLES):
        done = np.array([len(hist) > 60, False])
        c = Case(f"stall{cyc}", A, r, m, tol=0.0, bnorm=bnorm, done=done)
        cases.append(c)
        for j in range(m):
            hist.append(c.rel[j])
        r = r - _mv(A.astype(LD), c.x[m - 1])
        r[0] = 0
        r[0, 0] = 1                                   # (column 0: the minimiser is 0 and the residual e_1, exactly)
    hist = np.array(hist)
    assert np.all(np.abs(hist[:61, 0] - 1) < 1e-15)
    for hn in range(61, len(hist) + 1):              # the slow column's rate, with a margin of 10 %
        assert hist[hn - 1, 1] < 0.81 * hist[hn - 31, 1], (hn, hist[hn - 1, 1] / hist[hn - 31, 1])
    assert hist[-1, 1] > 1e-10                      # ... and it has not reached rounding level
    cyc, j = divmod(60, m)
    cases[cyc].conv_step = np.array([j, m])
    return cases, (cyc, j)


def all_cases():
    out = [width_case(nb) for nb in NBS] + [mask_case(1), mask_case(0), guard_case(4.0), guard_case(1e300)]
    out += [pair_case(0), pair_case(2), pair_case(3), breakdown_case(None), breakdown_case(0), zero_rhs_case()] + list(stall_cycles()[0])
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# comparison of an observed recurrence (the device's, or a replay's) with the references
# ---------------------------------------------------------------------------------------------------------------------------------
def solution(case, out):
    """x = sum_i out[i] v_i with the reference's basis as the solver holds it;  out: (m, nb)"""
    x = np.zeros((case.nb, case.n), dtype=LD)
    for i in range(case.m):
        x += out[i].astype(LD)[:, None] * case.script.V[i]
    return x


def ratios(case, obs):
    """largest |obs - ref| / ((j + 2) eps kappa_2 scale) over the residual estimates of the columns that take step j (scale:
    beta/bnorm) and over the solutions at each column's own stopping step (scale: ||x_ref||)"""
    worst = 0.0
    ok = ~case.done & ~case.breakdown
    for j in range(case.m):
        a = case.active(j) & ok
        if a.any():
            err = np.abs(obs["relres"][j][a].astype(RD) - case.rel[j][a])
            worst = max(worst, float(np.max(err / ((j + 2) * EPS * case.kap[j][a] * case.scale[a]))))
    if "out" in obs:
        x = solution(case, obs["out"])
        ks = np.minimum(case.conv_step, case.m - 1)
        for b in np.nonzero(ok)[0]:
            xr = case.x[ks[b], b]
            if not _sq(xr) > 0:                           # (a zero minimiser is compared exactly, by compare)
                continue
            err = np.sqrt(_sq(x[b] - xr)) / np.sqrt(_sq(xr))
            worst = max(worst, float(err / ((ks[b] + 2) * EPS * case.kap[ks[b], b])))
    return worst


def compare(case, obs, c=C_BOUND):
    """Every numerical claim of the GPU module about one cycle.  obs: relres, conv, steps (m, nb): the state after each step;
    out (m, nb): solve_y at the end; pairs {j: (alpha, c2m, hd2)}.  Returns the list of failures (empty: the recurrence is right)."""
    bad = []
    m, nb = case.m, case.nb
    ok = ~case.done & ~case.breakdown
    for j in range(m):
        a = case.active(j) & ok
        tol = c * (j + 2) * EPS * case.kap[j] * case.scale
        err = np.abs(obs["relres"][j].astype(RD) - case.rel[j])
        if a.any() and (np.any(~np.isfinite(obs["relres"][j][a])) or np.any(err[a] > tol[a])):
            bad.append(f"{case.name}: residual estimate of step {j}: {float(np.max(err[a] / tol[a])):.3g} times the bound")
        want_conv = case.done | (j >= case.conv_step)
        if not np.array_equal(obs["conv"][j] != 0, want_conv):
            bad.append(f"{case.name}: conv after step {j}")
        want_steps = np.where(case.done, 0, np.minimum(j, case.conv_step) + 1)
        if not np.array_equal(obs["steps"][j], want_steps):
            bad.append(f"{case.name}: steps after step {j}")
    if "out" in obs:
        out = obs["out"]
        x = solution(case, out)
        ks = np.minimum(case.conv_step, m - 1)
        res = np.sqrt(_sq(case.r.astype(LD) - _mv(case.A.astype(LD), x))) / case.bnorm
        for b in np.nonzero(ok)[0]:
            k = ks[b]
            xr = case.x[k, b]
            t = c * (k + 2) * EPS * case.kap[k, b]
            nx = np.sqrt(_sq(xr))
            if not np.sqrt(_sq(x[b] - xr)) <= t * nx:
                bad.append(f"{case.name}: solution of column {b}: {float(np.sqrt(_sq(x[b] - xr)) / (t * nx)):.3g} times the bound")
            if not abs(res[b] - case.rel[k, b]) <= t * case.anorm[b] * nx / case.bnorm[b]:
                bad.append(f"{case.name}: residual of the solution of column {b}")
            if np.any(out[k + 1:, b] != 0):
                bad.append(f"{case.name}: solve_y rows past the steps of column {b} are not 0")
        if np.any(out[:, case.done] != 0):
            bad.append(f"{case.name}: solve_y of a column done on entry is not 0")
    for j, (alpha, c2m, hd2) in obs.get("pairs", {}).items():
        T = case.pairs[j]
        b_alpha, b_c2m, b_hd2 = pair_bounds(T, j)
        for name, got, ref, bound in (("alpha", alpha, T.alpha, b_alpha), ("c2m", c2m, T.c2m, b_c2m), ("hd2", hd2, T.hd2, b_hd2)):
            err = np.abs(got.astype(LD) - ref)
            if np.any(~np.isfinite(got[..., ok])) or np.any(err[..., ok] > bound[..., ok]):
                bad.append(f"{case.name}: {name} of the pair at {j}: {float(np.max(_safe_div(err, bound)[..., ok])):.3g} times the bound")
    return bad
