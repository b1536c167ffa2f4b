"""Reference of the lock-step GMRES DRIVERS (csrc/gmres.hip struct Gmres and the chunk loop of wae_solve_guess), for
tests/test_gpu_solve_driver.py; tests/test_solveref.py checks it where no GPU is.

GMRES gives the drivers an implementation-independent contract: after k steps from a zero guess the iterate minimises
||M^-1 (b - A x)|| over the Krylov space of M^-1 A and M^-1 b, and that minimum is unique whatever the orthogonalisation, the scaling
of the basis or the pairing of steps.  `SolveRef.gmres` computes it in numpy's extended precision (clongdouble) from the V-cycle of
tests/_mgref.py (the FULL cycle, which tests/test_gpu_multigrid.py pins the device's to) and the term matrices: Arnoldi with two
passes of modified Gram-Schmidt on normalised vectors and a QR least-squares solve of the Hessenberg problem.  No Givens recurrence,
no unnormalised basis.  Columns never mix; a block of columns is handled side by side only to share the sparse products.

The rules of the driver that the reference mirrors -- the contract under test (lines of csrc/gmres.hip):

  * Recurrence length (Gmres::m, "int m = min(150, h->V.n / vec - 1) - off", the basis holding (restart + 1) vectors of d x NB):
    m = min(150, floor((restart + 1) * NB / nb) - 1), NB the set-up's batch width (opts[6]), nb the width of the chunk, restart =
    opts[4].  A request of r columns runs in chunks NB, NB, ..., remainder (wae_solve_guess, "for (c0 = 0; c0 < r; c0 += h->NB)").
    A guess direction that is deflated takes one slot: m - 1.
  * Stopping (absorb / vec.hip gmres_step_kernel: "relres <= 0.7 * tol"): a column stops at the first step whose estimate is
    <= 0.7 tol.  A cycle that ends with every column stopped after at most 12 steps is accepted on the estimate
    (converged_by_estimate: "if (j > 12) return false"); otherwise the true preconditioned residual is recomputed at the next cycle
    start, and a column is done when it is <= tol (cycle_start: "done[b] = relres[b] <= tol || stalled[b]").
  * Stall (absorb: "hs > 60 && relres > 0.9 * hist[hs - 31]"): needs more than 60 steps of history and less than 10 % gain over 30.
  * maxit (run_device / run_host: "j + 2 <= m && total_it + 2 <= maxit", "j < m && total_it < maxit"): a step, or a pair of steps,
    is only started if it ends at or before maxit.
  * Routing (gmres(): "device = env.device && s.lazy && !guess_dir && s.nb > 8"): more than 8 columns without a guess direction run
    the device recurrence (single-pass Gram-Schmidt, unnormalised basis, pair steps from step 2 of a cycle); 8 or fewer columns, or
    a guess direction, the host recurrence (8 or fewer: classical Gram-Schmidt twice on a normalised basis).  WAE_GMRES_DEVICE=0
    sends everything to the host recurrence.
  * wae_solve_info (Gmres::finish): iters_max / relres_max are maxima, iters_total / n_unconverged sums of per-COLUMN figures over all
    chunks; a column with a zero right-hand side takes no step, counts as converged and is returned as zeros.

`replay` is a complex128 restatement of the driver with the library's two orthogonalisations.  It is NOT an oracle: it measures what
float64 Gram-Schmidt costs in optimality (BETA below) and carries the seeded defects of tests/test_solveref.py.

BETA.  rho of the replays' iterates against the reference history r_k, largest relative distance |rho / r_k - 1| over every case of
the GPU module (tests/test_solveref.py::test_beta_measurement, on the synthetic hierarchy of that module; it fails if the
measured value drifts above BETA / 4).  It is the allowance for float64 Gram-Schmidt in the bounds of the GPU module and comes from the
reference and its replay, never from the library.  Measured: 7.1e-8, at the converged cases cut where r_k reaches the floor of 1e-9
(float64 rounding of the iterate relative to so small a residual); the truncated table alone gives 1.2e-9.

u.  The unit of float64 evaluation error of rho, see SolveRef.rho_u: the distance of the complex128 evaluation from the extended one,
taken on the residual VECTOR before its norm.

Step counts of a converged solve, see Contract.step_bounds: nothing converges faster than the minimiser, so a column takes at least
the steps the reference needs to 0.7 tol (1 + BETA) -- unless it is found at or below tol when a cycle starts, which the stopping rule
above allows; and at most the steps the reference needs to 0.35 tol.
"""
import numpy as np

import _mgref as M

LD = M.LD
RD = np.longdouble
BETA_MEASURED = 7.1e-8       # (the converged cases cut at r_k ~ 1e-9; the truncated table alone: 1.2e-9)
BETA = 8 * BETA_MEASURED
U_FACTOR = 16.0              # the device may differ from the extended-precision rho by U_FACTOR x its float64 distance u

WAE_OK, WAE_WARN_MAXITER, WAE_WARN_STAGNATION = 0, 1, 2
M_MAX, EST_FACTOR, SHORT_CYCLE, NARROW = 150, 0.7, 12, 8
DEFECTS = ("update_one_short", "late_restart", "pair_across_maxit", "neighbour_coefficients", "frozen_updated", "m_from_batch",
           "iters_lockstep")


def recurrence_length(restart, NB, nb, deflated=False):
    return min(M_MAX, (restart + 1) * NB // nb - 1) - (1 if deflated else 0)


def chunks(r, NB):
    return [(c0, min(NB, r - c0)) for c0 in range(0, r, NB)]


def _norm(v):
    a = np.abs(v)
    return np.sqrt((a * a).sum(axis=0))


def _dot(a, b):
    return (np.conj(a) * b).sum(axis=0)


class _Lsq:
    """min_y ||beta e1 - Hbar_k y|| for k = 1, 2, ... as the columns of Hbar arrive: a QR of Hbar by modified Gram-Schmidt, every column
    orthogonalised twice, in the precision of the input; per column of the batch (last axis)"""

    def __init__(self, m, beta):
        self.m, self.nb, self.dt = m, beta.shape[0], beta.dtype
        self.Q, self.R = [], np.zeros((m, m, self.nb), dtype=np.result_type(beta.dtype, np.complex64))
        self.res = np.zeros((m + 1, self.nb), dtype=self.R.dtype)
        self.res[0] = beta
        self.c = np.zeros((m, self.nb), dtype=self.R.dtype)

    def push(self, col):
        """col: (m + 1, nb), the new column of Hbar zero-padded; returns the minimum per batch column"""
        k = len(self.Q)
        a = col.astype(self.R.dtype)
        for _ in range(2):
            for p in range(k):
                h = _dot(self.Q[p], a)
                a = a - h * self.Q[p]
                self.R[p, k] += h
        nrm = _norm(a)
        self.R[k, k] = nrm
        q = a / np.where(nrm > 0, nrm, 1)
        self.Q.append(q)
        for _ in range(2):
            h = _dot(q, self.res)
            self.res = self.res - h * q
            self.c[k] += h
        return _norm(self.res)

    def y(self, k=None):
        k = len(self.Q) if k is None else k
        y = np.zeros((k, self.nb), dtype=self.R.dtype)
        for i in range(k - 1, -1, -1):
            s = self.c[i].copy()
            for q in range(i + 1, k):
                s = s - self.R[i, q] * y[q]
            d = self.R[i, i]
            y[i] = np.where(d != 0, s / np.where(d != 0, d, 1), 0)
        return y


class SolveRef:
    """levels, transfers: as tests/_mgref.vcycle_ref takes them (levels[0] holds the term matrices of the family); op in N/T/C; weights:
    dict(w_pre, w_post, w_light); nsweeps: the set-up's sweep count.  Every method takes the columns b (n, r) together with their
    coefficient rows ct ((1, T): one system, or (r, T))."""

    def __init__(self, levels, transfers, op, weights, nsweeps):
        self.levels, self.transfers, self.op, self.w, self.nsweeps = levels, transfers, op, dict(weights), nsweeps

    def minv(self, b, ct, dtype=LD):
        return M.vcycle_ref(self.levels, self.transfers, b, ct, level=0, op=self.op, nsweeps=self.nsweeps, light=False, dtype=dtype, **self.w)

    def apply(self, x, ct, dtype=LD):
        return self.levels[0].apply(ct, self.op, x, dtype)

    def bnorm(self, b, ct, dtype=LD):
        return _norm(self.minv(np.asarray(b).astype(dtype), ct, dtype))

    def rho(self, x, b, ct, dtype=LD):
        """||M^-1 (b - A x)|| / ||M^-1 b|| per column (0 for a zero right-hand side), evaluated in `dtype`"""
        return self.rho_u(x, b, ct, dtypes=(dtype,))[0]

    def rho_u(self, x, b, ct, bn=None, dtypes=(LD, np.complex128)):
        """(rho in extended precision, u) per column as float64.  u is the distance of the complex128 evaluation of rho from the
        extended one, measured BEFORE the norm is taken: ||z_ld - z_64|| / ||M^-1 b|| + rho |1 - bn_64 / bn_ld| with z = M^-1 (b - A x),
        an upper bound of |rho_ld - rho_64| by the triangle inequality.  (The scalar difference of the two norms is no unit: the
        rounding errors of ~1000 rows cancel in a norm to a random fraction of eps -- 3.6e-16 for two columns of family A -- while
        a second float64 evaluation with another summation order, the device's, sits at its own random place: the ratio of two such
        numbers has no bound that holds.)  bn: (extended, complex128) norms of M^-1 b, when the caller has them."""
        z, n = [], []
        for i, dt in enumerate(dtypes):
            bd = np.asarray(b).astype(dt)
            n.append(self.bnorm(bd, ct, dt) if bn is None else bn[i])
            z.append(self.minv(bd - self.apply(np.asarray(x).astype(dt), ct, dt), ct, dt))
        live = n[0] > 0
        safe = np.where(live, n[0], 1)
        rho = np.where(live, _norm(z[0]) / safe, 0)
        if len(dtypes) == 1:
            return (rho,)
        u = np.where(live, _norm(z[0] - z[1]) / safe + rho * np.abs(1 - n[1] / safe), 0)
        return rho.astype(np.float64), u.astype(np.float64)

    def gmres(self, b, ct, m, kmax, keep=(), dtype=LD, until=None):
        """left-preconditioned restarted GMRES(m) from a zero guess.  Returns (hist, xs): hist (kmax, r) the minimal relative
        residuals r_1 .. r_kmax, running across restarts (after a restart the cycle starts from the recomputed residual); xs[k] the
        iterate after k steps for every k in `keep`.  dtype = complex128: the same statements in float64 (a cheap preview for the
        builders of the cases, never a bound); until: stop at the first step at which every column is <= until (the history is cut
        there).  A zero right-hand side: zeros in xs and, for a single column, an empty
        history; inside a block its history column is 0."""
        b = np.asarray(b)
        if b.ndim == 1:
            b = b[:, None]
        n, r = b.shape
        live = np.any(b != 0, axis=0)
        hist = np.zeros((kmax, r), dtype=RD)
        xs = {k: np.zeros((n, r), dtype=dtype) for k in keep}
        if not live.any():
            return (hist[:0] if r == 1 else hist), xs
        if not live.all():
            ctl = ct if np.shape(ct)[0] == 1 else np.asarray(ct)[live]
            h, x = self.gmres(b[:, live], ctl, m, kmax, keep, dtype, until)
            hist = hist[:len(h)]
            hist[:, live] = h
            for k in keep:
                xs[k][:, live] = x[k]
            return hist, xs
        bl = b.astype(dtype)
        zb = self.minv(bl, ct, dtype)
        bn = _norm(zb)
        x = np.zeros((n, r), dtype=dtype)
        z, k = zb, 0
        while k < kmax:
            beta = _norm(z)
            V = [z / beta]
            ls = _Lsq(m, beta.astype(dtype))
            steps = min(m, kmax - k)
            for j in range(steps):
                w = self.minv(self.apply(V[j], ct, dtype), ct, dtype)
                col = np.zeros((m + 1, r), dtype=dtype)
                for _ in range(2):
                    for i in range(j + 1):
                        h = _dot(V[i], w)
                        w = w - h * V[i]
                        col[i] += h
                hn = _norm(w)
                col[j + 1] = hn
                V.append(w / hn)
                hist[k] = (ls.push(col) / bn).real
                k += 1
                if k in xs or j == steps - 1:
                    y = ls.y()
                    xk = x + sum(y[i] * V[i] for i in range(j + 1))
                    if k in xs:
                        xs[k] = xk
                if until is not None and np.all(hist[k - 1] <= until):
                    return hist[:k], xs
            x = xk
            if k < kmax:
                z = self.minv(bl - self.apply(x, ct, dtype), ct, dtype)
        return hist, xs


def steps_to(hist, tol_eff):
    """per column: the first k (1-based) with r_k <= tol_eff; raises if a column never gets there"""
    ok = np.asarray(hist) <= tol_eff
    if not np.all(ok.any(axis=0)):
        raise ValueError("the reference history does not reach the threshold")
    return np.argmax(ok, axis=0) + 1


# ----------------------------------------------------------------------------------------------------
# complex128 replay of the driver (not an oracle)
# ----------------------------------------------------------------------------------------------------
def replay(ref, B, ct, NB, restart, tol, maxit, device=True, pair_min=2, narrow_pair=False, defects=()):
    """wae_solve restated in complex128: chunks, recurrence length, lock-step cycles with per-column stopping, the library's two
    orthogonalisations (chunks of more than 8 columns: single-pass classical Gram-Schmidt on an UNNORMALISED basis; 8 or fewer: classical
    Gram-Schmidt twice on a normalised basis), pair steps as the granularity at which maxit is met.  Returns (X, info, iters per column);
    info: dict(code, iters_max, iters_total, n_unconverged, relres_max).  defects: names out of DEFECTS, see tests/test_solveref.py."""
    assert all(d in DEFECTS for d in defects)
    Z = np.complex128
    B = np.asarray(B, dtype=Z)
    n, r = B.shape
    ct = np.asarray(ct, dtype=Z)
    percol = ct.shape[0] != 1
    X = np.zeros((n, r), dtype=Z)
    info = dict(code=WAE_OK, iters_max=0, iters_total=0, n_unconverged=0, relres_max=0.0)
    iters_all = np.zeros(r, dtype=int)
    stag = False
    for c0, nb in chunks(r, NB):
        b = B[:, c0:c0 + nb]
        c = ct[c0:c0 + nb] if percol else ct
        if percol and "neighbour_coefficients" in defects:
            c = np.roll(ct, -1, axis=0)[c0:c0 + nb]
        m = recurrence_length(restart, NB, NB if "m_from_batch" in defects else nb)
        wide = nb > NARROW
        pair_on = (device and wide and pair_min >= 0) or (not wide and narrow_pair)
        pmin = pair_min if wide else 4
        zb = ref.minv(b, c, Z)
        bnorm = np.linalg.norm(zb, axis=0)
        live = bnorm > 0
        x = np.zeros((n, nb), dtype=Z)
        relres = np.zeros(nb)
        iters = np.zeros(nb, dtype=int)
        hist = [[] for _ in range(nb)]
        stalled = np.zeros(nb, dtype=bool)
        total, first = 0, True
        while True:
            z = zb if first else ref.minv(b - ref.apply(x, c, Z), c, Z)
            first = False
            zn = np.linalg.norm(z, axis=0)
            relres[live] = zn[live] / bnorm[live]
            done = ~live | (relres <= tol) | stalled
            if done.all() or total >= maxit:
                break
            # the basis: V[i] (n, nb); wide chunks keep it unnormalised (scale s_i per column), narrow ones normalised
            V = [z / np.where(zn > 0, zn, 1)]
            s = [np.ones(nb)]
            H = np.zeros((m + 3, m + 2, nb), dtype=Z)                    # normalised Hessenberg columns
            conv = done.copy()
            steps = np.zeros(nb, dtype=int)
            mm = m + (1 if "late_restart" in defects else 0)
            j = 0
            while j < mm and total < maxit:
                two = pair_on and j >= pmin and j + 2 <= mm and (total + 2 <= maxit or "pair_across_maxit" in defects)
                if two and wide:
                    two = (~conv).sum() > nb // 4
                for _ in range(2 if two else 1):
                    w = ref.minv(ref.apply(V[j], c, Z), c, Z)
                    if wide:                                               # one pass, coefficients s_i^2 (V_i^H w), all from the same w
                        cf = [s[i] ** 2 * _dot(V[i], w) for i in range(j + 1)]
                        w = w - sum(cf[i] * V[i] for i in range(j + 1))
                        nw = np.linalg.norm(w, axis=0)
                        for i in range(j + 1):
                            H[i, j] = np.where(s[i] > 0, s[j] / np.where(s[i] > 0, s[i], 1), 0) * cf[i]
                        H[j + 1, j] = s[j] * nw
                        s.append(np.where(nw > 0, 1 / np.where(nw > 0, nw, 1), 0))
                        V.append(w)
                    else:                                                  # classical Gram-Schmidt twice
                        cf = [_dot(V[i], w) for i in range(j + 1)]
                        w = w - sum(cf[i] * V[i] for i in range(j + 1))
                        cf2 = [_dot(V[i], w) for i in range(j + 1)]
                        w = w - sum(cf2[i] * V[i] for i in range(j + 1))
                        nw = np.linalg.norm(w, axis=0)
                        for i in range(j + 1):
                            H[i, j] = cf[i] + cf2[i]
                        H[j + 1, j] = nw
                        s.append(np.ones(nb))
                        V.append(w / np.where(nw > 0, nw, 1))
                    j += 1
                    total += 1
                    for q in np.nonzero(~conv)[0]:
                        g = np.zeros(j + 1, dtype=Z)
                        g[0] = zn[q]
                        yq = np.linalg.lstsq(H[:j + 1, :j, q], g, rcond=None)[0]
                        est = np.linalg.norm(g - H[:j + 1, :j, q] @ yq) / bnorm[q]
                        steps[q] = j
                        iters[q] += 1
                        relres[q] = est
                        hist[q].append(est)
                        if est <= EST_FACTOR * tol:
                            conv[q] = True
                        elif len(hist[q]) > 60 and est > 0.9 * hist[q][-31]:
                            conv[q] = stalled[q] = True
                    if "frozen_updated" in defects:                        # a frozen column goes on with the batch
                        for q in np.nonzero(conv & live & ~done)[0]:
                            if steps[q] < j:
                                steps[q] = j
                                iters[q] += 1
                if conv.all():
                    break
            for q in range(nb):
                k = steps[q] - (1 if "update_one_short" in defects and steps[q] > 0 else 0)
                if k <= 0:
                    continue
                g = np.zeros(steps[q] + 1, dtype=Z)
                g[0] = zn[q]
                yq = np.linalg.lstsq(H[:steps[q] + 1, :k, q], g, rcond=None)[0]
                x[:, q] += sum(yq[i] * s[i][q] * V[i][:, q] for i in range(k))
            if j <= SHORT_CYCLE and not stalled.any() and np.all(relres[live] <= tol):
                break
        X[:, c0:c0 + nb] = x
        iters_all[c0:c0 + nb] = iters
        info["iters_max"] = max(info["iters_max"], int(iters.max()))
        info["iters_total"] += int(total * nb) if "iters_lockstep" in defects else int(iters.sum())
        info["n_unconverged"] += int(np.sum(live & ~(relres <= tol)))
        info["relres_max"] = max(info["relres_max"], float(relres[live].max()) if live.any() else 0.0)
        stag = stag or bool(np.any(stalled & ~(relres <= tol)))
    info["code"] = WAE_OK if info["n_unconverged"] == 0 else (WAE_WARN_STAGNATION if stag else WAE_WARN_MAXITER)
    return X, info, iters_all


# ----------------------------------------------------------------------------------------------------
# the cases of the GPU module (tests/test_gpu_solve_driver.py) and their bounds
# ----------------------------------------------------------------------------------------------------
NB_SMALL, RESTART_SMALL, NB_WIDE, RESTART_WIDE = 16, 6, 64, 30
DISTINCT = 16
ZERO_COL = 1                 # column ZERO_COL of every 16 is exactly zero: every batch of 3 columns or more holds one
TOL, MAXIT = 1e-10, 300
FLOOR = 1e-9                 # truncated solves keep to k with r_k >= FLOOR: no attainable-accuracy floor enters


def ks_for(r):
    """the step counts of the truncated solves of width r (handle batch 16 / restart 6)"""
    if r in (16, 35):
        return (1, 2, 3, 4, 5, 6, 7, 11, 12, 13)
    if r == 3:
        return (1, 2, 5, 7, 12, 13, 18)
    m = recurrence_length(RESTART_SMALL, NB_SMALL, r)
    return (1, 2, 5, m - 1, m, m + 1, m + 2)


def truncated_cases():
    """(r, k, percol, op) of table (a)"""
    out = []
    for r in (16, 12, 8, 3, 35):
        for k in ks_for(r):
            for percol in (False, True):
                out.append((r, k, percol, "N"))
    for op in ("C", "T"):
        for k in (3, 7):
            for percol in (False, True):
                out.append((16, k, percol, op))
    return out


def columns(B16, ct16, ct1, r, percol):
    """the r columns of a case out of the 16 distinct ones: right-hand sides (one in 16 zero) and coefficient rows"""
    rep = -(-r // DISTINCT)
    B = np.tile(B16, (1, rep))[:, :r].copy()
    B[:, ZERO_COL::DISTINCT] = 0
    return B, (np.tile(ct16, (rep, 1))[:r] if percol else ct1)


def rho_bounds(rk, u, beta=None):
    """[r_k (1 - beta) - 16 u, r_k (1 + beta) + 16 u]: below means more than k steps were taken, above that the iterate is not the minimiser"""
    beta = BETA if beta is None else beta
    return rk * (1 - beta) - U_FACTOR * u, rk * (1 + beta) + U_FACTOR * u


class Contract:
    """the bounds of the GPU module for one family: the extended-precision histories, cached per (op, coefficient mode, recurrence length,
    columns), and the assertions on what a driver returned.  tests/test_solveref.py runs it on `replay`, tests/test_gpu_solve_driver.py
    on the library.  B16, ct16: the 16 distinct columns; ct1: the single system."""

    def __init__(self, levels, transfers, weights, nsweeps, B16, ct16, ct1, nlevels=3):
        self.args = (levels, transfers)
        self.w, self.nsweeps, self.B16, self.ct16, self.ct1, self.nlevels = dict(weights), nsweeps, B16, ct16, ct1, nlevels
        self._ref, self._hist, self._bn = {}, {}, {}
        self.worst = {}                                              # kind of figure -> largest value in units of its bound

    def ref(self, op):
        if op not in self._ref:
            self._ref[op] = SolveRef(*self.args, op, self.w, self.nsweeps)
        return self._ref[op]

    def columns(self, r, percol):
        return columns(self.B16, self.ct16, self.ct1, r, percol)

    def history(self, op, percol, m, nd, kmax, until=None):
        """the reference history of the first nd distinct columns under GMRES(m): at least kmax steps, or up to `until`"""
        key = (op, percol, m, nd)
        have = self._hist.get(key)
        if have is None or (until is None and len(have) < kmax) or (until is not None and not np.all(have[-1] <= until)):
            B, ct = self.columns(nd, percol)
            self._hist[key] = self.ref(op).gmres(B, ct, m, kmax, until=until)[0]
        return self._hist[key]

    def case_history(self, op, percol, r, NB, restart, kmax, until=None):
        """(kmax, r) histories of the r columns of a request, chunk by chunk with the chunk's own recurrence length; a history that
        `until` cut short is continued with its last value (columns below `until` stay below it)"""
        parts = []
        for c0, nb in chunks(r, NB):
            assert c0 % DISTINCT == 0
            nd = min(nb, DISTINCT)
            h = self.history(op, percol, recurrence_length(restart, NB, nb), nd, kmax, until)
            parts.append(np.tile(h, (1, -(-nb // nd)))[:, :nb])
        n = max(len(p) for p in parts)
        return np.concatenate([np.concatenate([p, np.tile(p[-1:], (n - len(p), 1))]) for p in parts], axis=1)

    def rho_u(self, X, r, percol, op):
        B, ct = self.columns(r, percol)
        key = (op, percol, r)
        if key not in self._bn:
            self._bn[key] = tuple(self.ref(op).bnorm(B, ct, dt) for dt in (LD, np.complex128))
        return self.ref(op).rho_u(X, B, ct, bn=self._bn[key])

    def note(self, what, value):
        self.worst[what] = max(self.worst.get(what, 0.0), float(value))

    def check_truncated(self, X, info, code, r, k, percol, op, NB, restart, beta=None, what="", enforce=True):
        """tol = 1e-300, maxit = k.  Returns dict(units, rdist, counts): units = (rho - r_k) / (beta r_k + 16 u) per live column (within
        [-1, 1] is inside the bounds), rdist = |relres_max - max rho| / (16 max u), counts = the integers of info are right.
        enforce = False: nothing is asserted but the floor (tests/test_solveref.py looks at the figures of seeded defects)."""
        beta = BETA if beta is None else beta
        B, ct = self.columns(r, percol)
        live = np.any(B != 0, axis=0)
        nz = int(live.sum())
        what = what or f"truncated r={r} k={k} percol={percol} op={op} NB={NB} restart={restart}"
        rk = self.case_history(op, percol, r, NB, restart, k)[k - 1].astype(np.float64)
        assert np.all(rk[live] >= FLOOR), (what, "the case lies below the floor", float(rk[live].min()))
        rho, u = self.rho_u(X, r, percol, op)
        units = ((rho - rk) / (beta * rk + U_FACTOR * u + 1e-300))[live]
        rdist = abs(info["relres_max"] - rho.max()) / (U_FACTOR * u.max())
        counts = (code == WAE_WARN_MAXITER and info["iters_max"] == k and info["iters_total"] == k * nz and info["n_unconverged"] == nz
                  and info.get("levels", self.nlevels) == self.nlevels)
        fig = dict(units=units, rdist=rdist, counts=counts, rk=rk[live], rho=rho[live], u=u[live])
        if not enforce:
            return fig
        print(f"{what}: r_k {rk[live].min():.2e}..{rk[live].max():.2e}, rho - r_k in units of the budget {units.min():+.3f}..{units.max():+.3f}, "
              f"relres_max {rdist:.3f} of its budget, info {info}")
        assert code == WAE_WARN_MAXITER, (what, code)
        assert info["iters_max"] == k, (what, info)
        assert info["iters_total"] == k * nz, (what, info, nz)
        assert info["n_unconverged"] == nz, (what, info, nz)
        assert info.get("levels", self.nlevels) == self.nlevels, (what, info)
        assert np.all(X[:, ~live] == 0), (what, "a zero right-hand side did not return exact zeros")
        assert np.all(units >= -1), (what, "more than k steps were taken", float(units.min()))
        assert np.all(units <= 1), (what, "the iterate is not the minimiser", float(units.max()))
        assert rdist <= 1, (what, "relres_max is not the recomputed residual", info["relres_max"], float(rho.max()), float(u.max()))
        self.note("rho (truncated)", np.max(np.abs(units)))
        self.note("relres_max (truncated)", rdist)
        return fig

    def step_bounds(self, op, percol, r, NB, restart, tol=TOL, maxit=MAXIT, beta=None):
        """(klo, khi) per column, 0 for a zero column.  khi: the first step of the reference at 0.35 tol.  klo: the first step at
        0.7 tol (1 + beta) -- or, if it comes earlier, the first START OF A CYCLE (a multiple of the chunk's recurrence length) at which
        the reference is at tol (1 + beta): there the driver recomputes the residual and a column at or below tol is done (the stopping
        rule in the module docstring; GMRES(6) crosses the band between tol and 0.7 tol at a cycle start for half its columns)."""
        beta = BETA if beta is None else beta
        B, _ = self.columns(r, percol)
        live = np.any(B != 0, axis=0)
        hist = self.case_history(op, percol, r, NB, restart, maxit, until=0.35 * tol)
        ms = np.concatenate([np.full(nb, recurrence_length(restart, NB, nb)) for _, nb in chunks(r, NB)])
        return self._bounds(hist, ms, live, tol, beta)

    @staticmethod
    def _bounds(hist, ms, live, tol, beta):
        r = hist.shape[1]
        klo, khi = np.zeros(r, dtype=int), np.zeros(r, dtype=int)
        klo[live] = steps_to(hist[:, live], EST_FACTOR * tol * (1 + beta))
        khi[live] = steps_to(hist[:, live], 0.5 * EST_FACTOR * tol)
        for b in np.nonzero(live)[0]:
            for k in range(ms[b], klo[b], ms[b]):
                if hist[k - 1, b] <= tol * (1 + beta):
                    klo[b] = k
                    break
        return klo, khi

    def single_bounds(self, op, percol, NB, restart, tol=TOL, maxit=MAXIT, beta=None):
        """(klo, khi) of the 16 distinct columns solved one at a time: every one a chunk of width 1 with the recurrence length of that"""
        beta = BETA if beta is None else beta
        B, _ = self.columns(DISTINCT, percol)
        live = np.any(B != 0, axis=0)
        m = recurrence_length(restart, NB, 1)
        hist = self.history(op, percol, m, DISTINCT, maxit, until=0.35 * tol)
        return self._bounds(hist, np.full(DISTINCT, m), live, tol, beta)

    def check_residuals(self, X, info, code, r, percol, op, tol=TOL, beta=None, what="", relres=True):
        """the residual half of the contract of a converged solve; relres = False: without the bounds on relres_max (a solve with a
        guess direction, whose contract is rho, the return code and n_unconverged)"""
        beta = BETA if beta is None else beta
        B, ct = self.columns(r, percol)
        live = np.any(B != 0, axis=0)
        rho, u = self.rho_u(X, r, percol, op)
        lower = rho.max() * EST_FACTOR / (1 + beta) - U_FACTOR * u.max()
        print(f"{what}: rho max {rho.max():.2e} (tol {tol:.0e}), u max {u.max():.1e}, relres_max {info['relres_max']:.3e} >= {lower:.3e}, info {info}")
        assert code == WAE_OK and info["n_unconverged"] == 0, (what, code, info)
        assert info.get("levels", self.nlevels) == self.nlevels, (what, info)
        assert np.all(X[:, ~live] == 0), (what, "a zero right-hand side did not return exact zeros")
        assert np.all(rho <= tol + U_FACTOR * u), (what, float(rho.max()))
        if relres:
            assert info["relres_max"] <= tol, (what, info)
            assert info["relres_max"] >= lower, (what, "relres_max is smaller than what was reached", info["relres_max"], float(rho.max()))
        self.note("rho / tol (converged)", rho.max() / tol)
        return rho, u

    def check_converged(self, X, info, code, r, percol, op, NB, restart, tol=TOL, maxit=MAXIT, beta=None, what="", enforce=True):
        """returns (klo, khi); enforce = False: only the step counts are looked at, and (klo, khi, inside) is returned"""
        what = what or f"converged r={r} percol={percol} op={op} NB={NB} restart={restart}"
        klo, khi = self.step_bounds(op, percol, r, NB, restart, tol, maxit, beta)
        inside = klo.sum() <= info["iters_total"] <= khi.sum() and klo.max() <= info["iters_max"] <= khi.max()
        if not enforce:
            return klo, khi, inside
        self.check_residuals(X, info, code, r, percol, op, tol, beta, what)
        slack_t = (info["iters_total"] - klo.sum()) / max(1, khi.sum() - klo.sum())
        slack_m = (info["iters_max"] - klo.max()) / max(1, khi.max() - klo.max())
        print(f"{what}: sum klo {klo.sum()} <= iters_total {info['iters_total']} <= sum khi {khi.sum()} (slack used {slack_t:.2f}); "
              f"max klo {klo.max()} <= iters_max {info['iters_max']} <= max khi {khi.max()} (slack used {slack_m:.2f})")
        assert klo.sum() <= info["iters_total"] <= khi.sum(), (what, int(klo.sum()), info["iters_total"], int(khi.sum()))
        assert klo.max() <= info["iters_max"] <= khi.max(), (what, int(klo.max()), info["iters_max"], int(khi.max()))
        self.note("step slack, total", slack_t)
        self.note("step slack, max", slack_m)
        return klo, khi

    def pick_restart(self, op, percol, r, NB, start=RESTART_SMALL, tol=TOL, maxit=MAXIT):
        """the smallest restart >= start with which the restarted case is a fair one: the reference reaches 0.35 tol within maxit, needs
        at least three cycles to reach tol, and gains more than 10 % per 30 steps throughout (no stall verdict in play).  Searched on the
        complex128 preview of the history, then CONFIRMED on the extended-precision one."""
        B, ct = self.columns(min(r, DISTINCT), percol)
        live = np.any(B != 0, axis=0)

        def fair(h, m):
            h = np.asarray(h, dtype=np.float64)[:, live]
            if not np.all(h[-1] <= 0.35 * tol):
                return False
            if np.min(steps_to(h, tol)) < 2 * m + 1:
                return False
            return len(h) <= 30 or bool(np.all(h[30:] <= 0.9 * h[:-30]))

        for restart in range(start, 61):
            m = recurrence_length(restart, NB, r)
            if fair(self.ref(op).gmres(B, ct, m, maxit, dtype=np.complex128, until=0.35 * tol)[0], m):
                assert fair(self.history(op, percol, m, min(r, DISTINCT), maxit, until=0.35 * tol), m), ("the preview misled", restart)
                return restart
        raise AssertionError("no restart up to 60 makes the restarted case a fair one")
