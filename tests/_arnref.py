"""Reference of the shift-invert Arnoldi entries (csrc/arnoldi.hip arnoldi_core behind wae_arnoldi_shiftinvert, wae_arnoldi_shiftinvert_batch,
wae_arnoldi_shiftinvert_slots and wae_arnoldi_ritz_to_slot) and of their host half (nlevp/local_solvers.py _ritz, eigs_many,
eigs_many_slots), for tests/test_gpu_arnoldi.py; tests/test_arnref.py checks it where no GPU is.

Two references, both from the caller's term matrices (Hier.terms[0]) and nothing of the library:

  * `apply_S`: op(A)^-1 op(M) V, A = sum_k cA_k A_k, M = sum_k cM_k A_k (op = T: the transpose, op = C: the conjugate transpose of the
    SUMMED matrix, i.e. the coefficients conjugated with it), by a scipy sparse LU in complex128 and iterative refinement with residuals
    formed in clongdouble from the term matrices, until the correction no longer shrinks.  It returns the residual it reached.
  * `arnoldi_ref`: the textbook process in clongdouble: v_0 = v0 / ||v0||, modified Gram-Schmidt twice, a real positive subdiagonal; per
    step the dominant Ritz pair of the leading block by numpy.linalg.eig (largest |theta|) and its relative residual
    |h_{j+1,j}| |y_j| / |theta|.  It chooses and certifies inputs and drives the CPU tests.  H is NOT compared entry by entry: at the
    accuracy of an iterative solve that comparison is ill-posed, and the contract does not need it.

The contract `check_factorisation` holds an entry to -- what it returned (H, V), its inputs, wae_solve_info -- with the lines of
arnoldi_core it mirrors:

  a. START ("launch_norms(t.p ...); launch_scale_inv(t.p, hcol.p, EV.p ...)"): column 0 of V is v0 / ||v0|| within M.budget of the
     distance of its complex128 evaluation from the extended one.  Where the pre-step applies ("if (prestep_on && ritz_tol > 0.0 &&
     m > 1 && h->ops.size() > 1 && tol < 1e-3)", "poor = hh[sy].x > 0.1" with q = ||P op(A) v_0||, P the V-cycle) column 0 of a poor
     system is instead parallel to an approximate solution of op(A) x = op(M) v_0 ("gmres(h, bt, t.p, h->Xs.p, 1e-3, ...)"): with
     x = s V[:, 0], s minimising the preconditioned residual in extended precision, rho(x) meets the bound of (d) at tol = 1e-3, and
     ||V[:, 0] - v_0|| > 0.1.  The reference's own q must lie outside [0.05, 0.2], or the case certifies nothing.
  b. STRUCTURE, exact: zeros below the subdiagonal; the subdiagonal real and >= 0 ("hc[sy][j + 1] = brk ? zc(0) : zc(hh[sy].x)"); H
     columns of steps not taken zero; with ritz_tol > 0 the V_out columns beyond steps taken + 1 still hold the caller's sentinel ("only
     the columns the processes produced are written"); a dead system ("brk = dead[sy] || !(hh[sy].x > 1e-14 * scale)", "al[sy] = brk ?
     cplx{0.0, 0.0} : ...") has every H entry and every returned basis column from its death on exactly zero; all systems dead and
     ritz_tol = 0: the remaining V_out columns zero-filled ("every process ended in an invariant subspace: the documented zeros").
     A system is dead if and only if its start column is zero (the cases hold no other breakdown; the reference certifies that).
  c. ORTHONORMALITY of the live columns, max |V^H V - I|, within M.budget of the same quantity of a complex128 run of `arnoldi_ref`
     from the returned column 0.
  d. THE DEFINING RELATION, backward and preconditioned, column by column: for step j of system s, w = V[:, :j+2] H[:j+2, j],
     rho_j = ||P (op(M) v_j - op(A) w)|| / ||P op(M) v_j||  <=  tol_j (1 + BETA) + 16 u_j ("gmres(h, bt, t.p, h->Xs.p, tol_j, ...)"; BETA
     and the 16 of tests/_solveref.py; u_j the distance of the complex128 evaluation of the whole expression, reconstruction of w
     included, from the extended one, taken on the residual vector before its norm as SolveRef.rho_u does).  tol_j comes from (e).
  e. THE SCHEDULE, recomputed from the returned H with eig: worst_j the largest dominant-Ritz residual over the live systems after step
     j; with ritz_tol > 0 the process stopped at the first j + 1 < m with worst_j <= ritz_tol and not before ("if (ritz_tol > 0.0 &&
     j + 1 < m) ... if (worst <= ritz_tol) break"); tol_0 = tol, tol_{j+1} = max(tol, min(1e-3, 0.1 tol / worst_j)) ("tol_j =
     std::max(tol, std::min(1e-3, 0.1 * tol / worst))"); ritz_tol = 0: m steps, every tol_j = tol.  Certified on the reference before a
     case is run (`certify`): no worst_j of `arnoldi_ref` inside [ritz_tol / 4, 4 ritz_tol], and its two largest Ritz moduli 10 x apart
     at every step the stop test looks at -- the library's power iteration and eig then name the same pair and the stopping step is
     no coin toss.
  f. wae_solve_info: n_unconverged == 0 and relres_max <= max_j tol_j.

`replay` is a complex128 restatement of arnoldi_core's rules (normalise; the q test and the pre-step; classical Gram-Schmidt twice; the
dead rule; the stop test; the relaxation) with solves from SolveRef.gmres stopped at the first step at or below 0.7 tol_j.  Like
_solveref.replay it is NOT an oracle: it carries the seeded defects DEFECTS of tests/test_arnref.py.

Near shifts.  NEAR_A, NEAR_C: eigenvalues of the two families of tests/_hier.py, found on the host term matrices by the oracle's
Newton iteration (the line below each constant), then moved off the eigenvalue by `near_shifts` so that the pencil's smallest |lambda|
is 1e-5 .. 1e-4 of the next one (asserted by the GPU module's fixtures)."""
import numpy as np
import scipy.sparse.linalg as spla

import _mgref as M
import _solveref as S

LD = M.LD
Z = np.complex128
OPS = {"N": 0, "T": 1, "C": 2}
OPNAME = {v: k for k, v in OPS.items()}
SENT = 3 + 7j
DEFECTS = ("m_row0", "m_not_conjugated", "stop_late", "stop_early", "relax_loose", "prestep_never", "prestep_all", "dead_not_zeroed",
           "one_gs_pass", "complex_subdiagonal")
Q_POOR = 0.1
MFACT = np.array([1, 2, 0.5 - 0.5j, -1.5j, 3, 0.25 + 1j, -2, 1 + 1j, 0.75, -0.5 + 2j, 1.5 - 1j, 4j, 0.3, -1 - 1j, 2.5, 0.6 + 0.8j])

# oracle.solvers.householder(HostL(annulus_family("tiny", tau=2e-4)[0]), Z_AB, maxiter=12, tol=1e-9, v0=default_rng(0).standard_normal(d))
#   -> 4 steps, flag 1   (HostL: the family with L(...) evaluated as the scipy sum of its terms; pencil |lambda|_min 8e-9 there)
NEAR_A = 2732.0160891612304 + 82.76892604200874j
# oracle.solvers.householder(HostL(bloch_family(build_unit_cell(grid=(4, 26, 7), DOS=12, tau=2e-4)), b = 5), Z_C, maxiter=12, tol=1e-9,
#   v0=default_rng(0).standard_normal(d))  -> 5 steps, flag 1   (pencil |lambda|_min 3e-8 there)
NEAR_C = 27509.10458800617 + 5.166916407945146j
NEAR_OFF = {"A": 1e-3, "C": 3e-3}            # |lambda|_min / |lambda|_next = 3.1e-5 (A), 2.7e-5 (C) at one offset


def near_shifts(name, nsys):
    """nsys shifts next to the eigenvalue of family `name`: offsets 1, 1.25, 1.5, ... times NEAR_OFF (ratios 3e-5 .. 6e-5 for 4)"""
    z0 = NEAR_A if name == "A" else NEAR_C
    return z0 + NEAR_OFF[name] * (1 + 0.25 * np.arange(nsys))


def _norm(v):
    return S._norm(v)


def rows(c, r):
    c = np.asarray(c, dtype=Z).reshape(-1, np.shape(c)[-1])
    return c if c.shape[0] == r else np.repeat(c[:1], r, axis=0)


def op_matrix(terms, c, op):
    """op(sum_k c_k A_k) as a scipy CSC matrix in complex128"""
    A = sum(ck * t for ck, t in zip(c, terms) if ck != 0).tocsc()
    return A if op == "N" else (A.T.tocsc() if op == "T" else A.conj().T.tocsc())


class Ctx:
    """what the references of one family are built from: the levels and transfers of tests/_mgref.vcycle_ref (levels[0] holds the term
    matrices), the cycle's weights and sweep count"""

    def __init__(self, levels, transfers, weights, nsweeps):
        self.levels, self.transfers, self.w, self.nsweeps = levels, transfers, dict(weights), nsweeps
        self.lev = levels[0]
        self.terms = self.lev.terms
        self.n = self.lev.n
        self.multilevel = len(levels) > 2                            # a sparse coarse level: "h->ops.size() > 1"
        self._ref, self._lu = {}, {}

    def ref(self, op):
        if op not in self._ref:
            self._ref[op] = S.SolveRef(self.levels, self.transfers, op, self.w, self.nsweeps)
        return self._ref[op]

    def lu(self, c, op):
        key = (op, np.asarray(c, dtype=Z).tobytes())
        if key not in self._lu:
            if len(self._lu) > 64:
                self._lu.clear()
            self._lu[key] = spla.splu(op_matrix(self.terms, c, op))
        return self._lu[key]

    def mat(self, c, op):
        key = ("m", op, np.asarray(c, dtype=Z).tobytes())
        if key not in self._lu:
            self._lu[key] = op_matrix(self.terms, c, op).tocsr()
        return self._lu[key]

    def lusolve(self, B, cA, op):
        """op(A)^-1 B in complex128, column by column with its own coefficient row"""
        cA = rows(cA, B.shape[1])
        X = np.zeros(B.shape, dtype=Z)
        for s in range(B.shape[1]):
            X[:, s] = self.lu(cA[s], op).solve(np.ascontiguousarray(B[:, s], dtype=Z))
        return X


def apply_S(ctx, V, cA, cM, op, rounds=12):
    """(op(A)^-1 op(M) V in clongdouble, the residual it reached per column).  The residual is the normwise backward error
    ||b - op(A) x|| / || |op(A)| |x| + |b| ||, b = op(M) v: what forming a residual in clongdouble can resolve, 1e-19.  (Relative to
    ||b|| alone a near shift leaves eps |A| |x| / |b| = 1e-19 x 1e7 -- x is the eigenvector times 1 / lambda_min -- which says nothing
    about x: that rounding, solved for, lies along the eigenvector to 3e-5 and moves theta, not a Ritz residual.)"""
    V = np.asarray(V)
    if V.ndim == 1:
        V = V[:, None]
    r = V.shape[1]
    cA, cM = rows(cA, r), rows(cM, r)
    B = ctx.lev.apply(cM, op, V.astype(LD), LD)
    X = ctx.lusolve(B.astype(Z), cA, op).astype(LD)
    prev = None
    for _ in range(rounds):
        R = B - ctx.lev.apply(cA, op, X, LD)
        dX = ctx.lusolve(R.astype(Z), cA, op)
        nd = _norm(dX).astype(np.float64)
        if prev is not None and np.all(nd >= 0.5 * prev):            # the correction no longer shrinks
            break
        X = X + dX.astype(LD)
        prev = nd
    R = B - ctx.lev.apply(cA, op, X, LD)
    scale = np.stack([abs(ctx.mat(cA[s], op)) @ np.abs(X[:, s]).astype(np.float64) for s in range(r)], axis=1) + np.abs(B).astype(np.float64)
    sn = np.linalg.norm(scale, axis=0)
    return X, (_norm(R).astype(np.float64) / np.where(sn > 0, sn, 1))


def dominant(Hs, k):
    """the dominant Ritz pair of the leading k x k block of one Hessenberg matrix ((m+1) x m): (theta, unit y, relative residual
    |h_{k+1,k}| |y_k| / |theta|, |theta_1| / |theta_2|)"""
    th, Y = np.linalg.eig(np.asarray(Hs[:k, :k], dtype=Z))
    order = np.argsort(-np.abs(th))
    th, y = th[order], Y[:, order[0]]
    y = y / np.linalg.norm(y)
    res = float(abs(complex(Hs[k, k - 1])) * abs(y[k - 1]) / abs(th[0])) if abs(th[0]) > 0 else np.inf
    sep = float(abs(th[0]) / abs(th[1])) if k > 1 and abs(th[1]) > 0 else np.inf
    return th[0], y, res, sep


def arnoldi_ref(Sfun, v0, m, dtype=LD):
    """the textbook process for the columns of v0 side by side (columns never mix).  Sfun(V) -> S V.  Returns dict(H (r, m+1, m),
    V (r, n, m+1) in `dtype`, theta (m, r), res (m, r), sep (m, r): the dominant Ritz pair after every step)"""
    v0 = np.asarray(v0)
    if v0.ndim == 1:
        v0 = v0[:, None]
    n, r = v0.shape
    H = np.zeros((r, m + 1, m), dtype=dtype)
    V = np.zeros((r, n, m + 1), dtype=dtype)
    v = v0.astype(dtype)
    V[:, :, 0] = (v / _norm(v)).T
    theta, res, sep = np.zeros((m, r), dtype=Z), np.zeros((m, r)), np.zeros((m, r))
    for j in range(m):
        w = np.asarray(Sfun(V[:, :, j].T)).astype(dtype)
        for _ in range(2):
            for i in range(j + 1):
                h = S._dot(V[:, :, i].T, w)
                w = w - h * V[:, :, i].T
                H[:, i, j] += h
        hn = _norm(w)
        H[:, j + 1, j] = hn
        V[:, :, j + 1] = (w / hn).T
        for s in range(r):
            theta[j, s], _, res[j, s], sep[j, s] = dominant(H[s], j + 1)
    return dict(H=H, V=V, theta=theta, res=res, sep=sep)


def schedule(H, live, m, tol, ritz_tol):
    """(steps the process must have taken, [tol_0 ..], [worst_0 ..], smallest separation met) from Hessenberg matrices H (nsys, m+1, m)
    by rule (e); live: the systems that are not dead"""
    tols, worst, sepmin = [tol], [], np.inf
    if not np.any(live):
        return 1, tols, worst, sepmin
    for j in range(m):
        if not (ritz_tol > 0 and j + 1 < m):
            if j + 1 < m:
                tols.append(tol)
            continue
        fig = [dominant(H[s], j + 1) for s in np.nonzero(live)[0]]
        wj = max(f[2] for f in fig)
        sepmin = min(sepmin, min(f[3] for f in fig))
        worst.append(wj)
        if wj <= ritz_tol:
            return j + 1, tols, worst, sepmin
        tols.append(max(tol, min(1e-3, 0.1 * tol / wj)))
    return m, tols, worst, sepmin


def certify(out, m, ritz_tol, what=""):
    """rule (e)'s condition on a run of arnoldi_ref; returns the step count the reference schedules"""
    r = out["H"].shape[0]
    steps, _, worst, sepmin = schedule(np.asarray(out["H"], dtype=Z), np.ones(r, dtype=bool), m, 0.0, ritz_tol)
    if ritz_tol > 0:
        assert not any(ritz_tol / 4 <= w <= 4 * ritz_tol for w in worst), (what, "a Ritz residual of the reference sits at the threshold", worst)
        assert sepmin >= 10, (what, "the dominant Ritz value of the reference is not separated", sepmin)
    return steps


def start_quality(ctx, v0, cA, op):
    """q = ||P op(A) v_0|| of the normalised start columns, in extended precision (0 for a zero column)"""
    v = np.asarray(v0).astype(LD)
    nv = _norm(v)
    vn = v / np.where(nv > 0, nv, 1)
    ref = ctx.ref(op)
    return _norm(ref.minv(ref.apply(vn, rows(cA, v.shape[1])), rows(cA, v.shape[1]))).astype(np.float64)


def rho_recon(ctx, Vb, hcols, vj, cA, cM, op):
    """(rho, u) of rule (d) for k columns side by side: Vb[i] (n, p_i) the basis block, hcols[i] (p_i,) the Hessenberg column, vj (n, k)
    the basis vector the step started from, cA / cM (k, T)"""
    ref = ctx.ref(op)
    k = vj.shape[1]
    zs, ns = [], []
    for dt in (LD, Z):
        W = np.stack([Vb[i].astype(dt) @ np.asarray(hcols[i]).astype(dt) for i in range(k)], axis=1)
        B = ctx.lev.apply(cM, op, vj.astype(dt), dt)
        R = B - ctx.lev.apply(cA, op, W, dt)
        Zz = ref.minv(np.concatenate([B, R], axis=1), np.concatenate([cA, cA]), dt)
        ns.append(_norm(Zz[:, :k]))
        zs.append(Zz[:, k:])
    safe = np.where(ns[0] > 0, ns[0], 1)
    rho = _norm(zs[0]) / safe
    u = _norm(zs[0] - zs[1]) / safe + rho * np.abs(1 - ns[1] / safe)
    return rho.astype(np.float64), u.astype(np.float64)


def rho_bound(tol, u):
    return tol * (1 + S.BETA) + S.U_FACTOR * u


def check_factorisation(ctx, H, V, info, v0, cA, cM, op, m, tol, ritz_tol, sent=SENT, enforce=True, what=""):
    """holds what an entry returned to the contract of the module docstring.  H (nsys, m+1, m), V (nsys, n, m+1) as the entry filled
    the caller's sentinel-filled buffers (V None: a slots call, the rules on V are skipped), info: dict of wae_solve_info.  Returns the
    figures, each in units of its bound (exact rules: 0 or inf); enforce: assert them all <= 1."""
    H, v0 = np.asarray(H, dtype=Z), np.asarray(v0, dtype=Z)
    nsys, n = H.shape[0], v0.shape[0]
    cA, cM = rows(cA, nsys), rows(cM, nsys)
    fig = {}
    zero = ~np.any(v0 != 0, axis=0)
    live = ~zero

    def exact(name, ok):
        fig[name] = max(fig.get(name, 0.0), 0.0 if ok else np.inf)

    # (b) the steps taken, from H; structure
    nzcol = [j for j in range(m) if np.any(H[:, :, j] != 0)]
    steps = (max(nzcol) + 1) if nzcol else 1
    exact("b: zeros below the subdiagonal", all(np.all(H[:, j + 2:, j] == 0) for j in range(m)))
    sub = np.array([[H[s, j + 1, j] for j in range(m)] for s in range(nsys)])
    exact("b: subdiagonal real and >= 0", bool(np.all(sub.imag == 0) and np.all(sub.real >= 0)))
    exact("b: columns of steps not taken are zero", bool(np.all(H[:, :, steps:] == 0)))
    exact("b: a zero start is dead and all zeros", bool(np.all(H[zero] == 0)))
    exact("b: only a zero start is dead", bool(np.all(sub.real[live][:, :steps] > 0)) if live.any() else True)
    if V is not None:
        V = np.asarray(V, dtype=Z)
        exact("b: a dead system's basis is zero", bool(np.all(V[zero][:, :, :steps + 1] == 0)))
        if ritz_tol > 0:
            exact("b: columns beyond steps + 1 keep the sentinel", bool(np.all(V[:, :, steps + 1:] == sent)))
        else:
            exact("b: every step taken, or the documented zeros", steps == m or (not live.any() and bool(np.all(V[:, :, steps + 1:] == 0))))
    # (e) the schedule
    want, tols, worst, sepmin = schedule(H, live, m, tol, ritz_tol)
    fig["e: stopped late"] = 0.0 if steps <= want else (ritz_tol / max(worst[want - 1], 1e-300))
    fig["e: stopped early"] = 0.0 if steps >= want else (worst[steps - 1] / ritz_tol if steps - 1 < len(worst) else np.inf)
    tols = (tols + [tols[-1]] * m)[:max(steps, 1)]
    # (f) info
    if info is not None:
        exact("f: n_unconverged == 0", info["n_unconverged"] == 0)
        fig["f: relres_max"] = info["relres_max"] / max(tols)
    if not live.any():
        return _finish(fig, enforce, what, steps, tols)
    ls = np.nonzero(live)[0]
    # (a) the start
    v0l = v0[:, ls]
    vn = [(v0l.astype(dt) / _norm(v0l.astype(dt))) for dt in (LD, Z)]
    applies = ritz_tol > 0 and m > 1 and ctx.multilevel and tol < 1e-3
    poor = np.zeros(len(ls), dtype=bool)
    if applies:
        q = start_quality(ctx, v0l, cA[ls], op)
        assert not np.any((q >= Q_POOR / 2) & (q <= 2 * Q_POOR)), (what, "the reference's q sits at the threshold", q)
        poor = q > Q_POOR
        fig["q"] = q
    if V is not None:
        c0 = V[ls, :, 0].T
        e64 = M.column_errors(vn[1], vn[0], (np.ones(n, dtype=bool),))
        err = M.column_errors(c0, vn[0], (np.ones(n, dtype=bool),))
        dist = np.linalg.norm(c0 - vn[1], axis=0)
        good = ~poor
        if good.any():
            fig["a: column 0 is v0 / ||v0||"] = float(np.max(err[good] / M.budget(e64[good])))
        if poor.any():
            p = np.nonzero(poor)[0]
            fig["a: a poor start is replaced"] = float(np.max(Q_POOR / np.maximum(dist[p], 1e-300)))
            # x = s V[:, 0] with the s that minimises ||P (b - s op(A) c0)||, b = op(M) v_0
            ref = ctx.ref(op)
            ca, cm = cA[ls][p], cM[ls][p]
            out = []
            for dt in (LD, Z):
                B = ctx.lev.apply(cm, op, vn[0 if dt == LD else 1][:, p], dt)
                A0 = ctx.lev.apply(ca, op, c0[:, p].astype(dt), dt)
                Zz = ref.minv(np.concatenate([B, A0], axis=1), np.concatenate([ca, ca]), dt)
                zb, za = Zz[:, :len(p)], Zz[:, len(p):]
                s = S._dot(za, zb) / S._dot(za, za)
                out.append((zb - s * za, _norm(zb)))
            rho = (_norm(out[0][0]) / out[0][1])
            u = _norm(out[0][0] - out[1][0]) / out[0][1] + rho * np.abs(1 - out[1][1] / out[0][1])
            fig["a: the pre-step's solve"] = float(np.max(rho.astype(np.float64) / rho_bound(1e-3, u.astype(np.float64))))
        # (c) orthonormality against a complex128 run of the reference from the returned column 0
        out64 = arnoldi_ref(lambda X: ctx.lusolve(ctx.lev.apply(cM[ls], op, X, Z), cA[ls], op), c0, steps, dtype=Z)
        k = steps + 1
        g = np.array([np.max(np.abs(V[s, :, :k].conj().T @ V[s, :, :k] - np.eye(k))) for s in ls])
        g64 = np.array([np.max(np.abs(out64["V"][i].conj().T @ out64["V"][i] - np.eye(k))) for i in range(len(ls))])
        fig["c: orthonormality"] = float(np.max(g / M.budget(g64)))
        # (d) the defining relation
        Vb, hc, vj, ca, cm, tj = [], [], [], [], [], []
        for s in ls:
            for j in range(steps):
                Vb.append(V[s, :, :j + 2])
                hc.append(H[s, :j + 2, j])
                vj.append(V[s, :, j])
                ca.append(cA[s])
                cm.append(cM[s])
                tj.append(tols[j])
        rho, u = rho_recon(ctx, Vb, hc, np.stack(vj, axis=1), np.array(ca), np.array(cm), op)
        units = rho / rho_bound(np.array(tj), u)
        fig["d: rho_j"] = float(np.max(units))
        fig["rho"], fig["u"], fig["tol_j"] = rho, u, np.array(tj)
    return _finish(fig, enforce, what, steps, tols)


def units_of(fig):
    return {k: v for k, v in fig.items() if k[1:2] == ":"}


def _finish(fig, enforce, what, steps, tols):
    fig["steps"], fig["tols"] = steps, tols
    un = units_of(fig)
    if enforce:
        print(f"{what}: {steps} steps, tol_j {['%.1e' % t for t in tols]}; in units of their bounds: " +
              ", ".join(f"{k} {v:.3g}" for k, v in un.items() if v > 0))
        for k, v in un.items():
            assert v <= 1, (what, k, v)
    return fig


def worst_unit(fig):
    """(name, value) of the figure that misses its bound by the most"""
    return max(units_of(fig).items(), key=lambda kv: kv[1])


# ----------------------------------------------------------------------------------------------------
# complex128 replay of arnoldi_core (not an oracle)
# ----------------------------------------------------------------------------------------------------
KMAX = 120


def _solve(ctx, op, B, cA, tol):
    """GMRES (one unrestarted cycle) on the columns of B, stopped at the first step at which every column's minimum is at or below
    0.7 tol; returns (X, largest minimum reached, steps)"""
    if not np.any(B != 0):
        return np.zeros(B.shape, dtype=Z), 0.0, 0
    hist, xs = ctx.ref(op).gmres(B, cA, KMAX, KMAX, keep=range(1, KMAX + 1), dtype=Z, until=S.EST_FACTOR * tol)
    k = len(hist)
    if k == 0:
        return np.zeros(B.shape, dtype=Z), 0.0, 0
    return xs[k], float(np.max(np.asarray(hist[k - 1], dtype=np.float64))), k


def replay(ctx, v0, cA, cM, op, m, tol, ritz_tol, defects=(), sent=SENT, force_steps=None):
    """arnoldi_core restated in complex128.  Returns (H (nsys, m+1, m), V (nsys, n, m+1) sentinel-filled, info dict)."""
    assert all(d in DEFECTS for d in defects)
    if force_steps is None and ("stop_late" in defects or "stop_early" in defects):
        clean = replay(ctx, v0, cA, cM, op, m, tol, ritz_tol, tuple(d for d in defects if not d.startswith("stop_")), sent)
        steps = int(max([j + 1 for j in range(m) if np.any(clean[0][:, :, j] != 0)] or [1]))
        force = steps + 1 if "stop_late" in defects else steps - 1
        assert 1 <= force <= m, "the case leaves no room for the seeded stop"
        return replay(ctx, v0, cA, cM, op, m, tol, ritz_tol, defects, sent, force_steps=force)
    v0 = np.asarray(v0, dtype=Z)
    n, nsys = v0.shape
    cA, cM = rows(cA, nsys), rows(cM, nsys)
    cMe = np.repeat(cM[:1], nsys, axis=0) if "m_row0" in defects else cM
    if "m_not_conjugated" in defects and op == "C":
        cMe = cMe.conj()                                             # (Level.apply conjugates once more)
    ref, lev = ctx.ref(op), ctx.lev
    info = dict(n_unconverged=0, relres_max=0.0, iters_total=0)
    H = np.zeros((nsys, m + 1, m), dtype=Z)
    EV = np.zeros((m + 1, n, nsys), dtype=Z)
    nv = np.linalg.norm(v0, axis=0)
    EV[0] = v0 / np.where(nv > 1e-300, nv, np.inf)
    dead = np.zeros(nsys, dtype=bool)
    loose = "dead_not_zeroed" in defects
    if ritz_tol > 0 and m > 1 and ctx.multilevel and tol < 1e-3 and "prestep_never" not in defects:
        q = np.linalg.norm(ref.minv(ref.apply(EV[0], cA, Z), cA, Z), axis=0)
        poor = (q > Q_POOR) | ("prestep_all" in defects)
        poor = poor & (nv > 0)
        if poor.any():
            X, _, k = _solve(ctx, op, lev.apply(cMe, op, EV[0], Z), cA, 1e-3)
            info["iters_total"] += k * nsys
            xn = np.linalg.norm(X, axis=0)
            EV[0][:, poor] = (X / np.where(xn > 0, xn, 1))[:, poor]
    tol_j, done = tol, 0
    for j in range(m):
        W, rel, k = _solve(ctx, op, lev.apply(cMe, op, EV[j], Z), cA, tol_j)
        info["iters_total"] += k * nsys
        info["relres_max"] = max(info["relres_max"], rel)
        info["n_unconverged"] += int(rel > tol_j)
        hc = np.zeros((j + 2, nsys), dtype=Z)
        for _ in range(1 if "one_gs_pass" in defects else 2):
            cf = np.array([S._dot(EV[i], W) for i in range(j + 1)])
            W = W - sum(cf[i] * EV[i] for i in range(j + 1))
            hc[:j + 1] += cf
        hn = np.linalg.norm(W, axis=0)
        done = j + 1
        scale = np.max(np.abs(hc[:j + 1]), axis=0)
        brk = dead | ~(hn > 1e-14 * scale)
        hc[j + 1] = np.where(brk, 0, hn)
        ph = np.exp(0.3j) if "complex_subdiagonal" in defects else 1.0
        for s in range(nsys):
            if not dead[s] or loose:
                H[s, :j + 2, j] = hc[:, s]
                H[s, j + 1, j] *= np.conj(ph)
        dead = dead | brk
        if not (~brk).any() and not loose:
            EV[j + 1] = 0
            break
        EV[j + 1] = ph * W / np.where(brk, np.inf, hn)
        if loose:                                                    # the dead column is not masked: whatever the buffer held
            EV[j + 1][:, brk] = 1.0 / np.sqrt(n)
        if force_steps is not None:
            if done == force_steps:
                break
            stop_ok = False
        else:
            stop_ok = True
        if ritz_tol > 0 and j + 1 < m:
            worst = max([dominant(H[s], j + 1)[2] for s in range(nsys) if not dead[s]] or [0.0])
            if stop_ok and worst <= ritz_tol:
                break
            if worst > 0:
                tol_j = max(tol, min(1e-3, (1.0 if "relax_loose" in defects else 0.1) * tol / worst))
    V = np.full((nsys, n, m + 1), sent, dtype=Z)
    for j in range(min(done, m) + 1):
        V[:, :, j] = EV[j].T
    if done < m and not ritz_tol > 0:
        V[:, :, done + 1:] = 0
    return H, V, info


# ----------------------------------------------------------------------------------------------------
# a stand-in for the device family under eigs_many / eigs_many_slots (the host half)
# ----------------------------------------------------------------------------------------------------
class FakeFam:
    """d, T, last_info, arnoldi_batch, slot_write / slot_read, arnoldi_slots, ritz_to_slot with the signatures of DeviceFamily, on the
    replay (buffers handed over as zeros, as the wrapper does)"""

    def __init__(self, ctx, unconverged=False):
        self.ctx, self.d, self.T = ctx, ctx.n, len(ctx.terms)
        self.last_info, self.slots, self.basis, self.calls = {}, {}, None, []
        self.unconverged = unconverged

    def arnoldi_batch(self, coeffsA, coeffsM, m, V0, op=0, tol=1e-12, maxit=300, ritz_tol=0.0, quiet=False):
        cA = np.asarray(coeffsA, dtype=Z).reshape(-1, self.T)
        V0 = np.asarray(V0, dtype=Z).reshape(self.d, cA.shape[0])
        H, V, info = replay(self.ctx, V0, cA, rows(coeffsM, cA.shape[0]), OPNAME[op], m, tol, ritz_tol, sent=0.0)
        if self.unconverged:
            info = dict(info, n_unconverged=cA.shape[0], relres_max=1e-2)
        self.last_info = info
        self.calls.append((cA.shape[0], m))
        return H, V

    def slot_write(self, slot, X=None, ncols_total=None, col0=0):
        if X is None:
            if slot not in self.slots or self.slots[slot].shape[1] != ncols_total:
                self.slots[slot] = np.zeros((self.d, ncols_total), dtype=Z)
            return
        X = np.asarray(X, dtype=Z).reshape(self.d, -1)
        nt = X.shape[1] if ncols_total is None else ncols_total
        if slot not in self.slots or self.slots[slot].shape[1] != nt:
            self.slots[slot] = np.zeros((self.d, nt), dtype=Z)
        self.slots[slot][:, col0:col0 + X.shape[1]] = X

    def slot_read(self, slot, col0, ncols):
        return self.slots[slot][:, col0:col0 + ncols].copy()

    def arnoldi_slots(self, coeffsA, coeffsM, m, v0_slot, v0_cols, op=0, tol=1e-12, maxit=300, ritz_tol=0.0, quiet=False):
        H, V = self.arnoldi_batch(coeffsA, coeffsM, m, self.slots[v0_slot][:, list(v0_cols)], op, tol, maxit, ritz_tol)
        steps = int(max([j + 1 for j in range(m) if np.any(H[:, :, j] != 0)] or [1]))
        self.basis = V[:, :, :steps + 1]
        return H

    def ritz_to_slot(self, Y, dst_slot, dst_cols, normalise=True):
        Y = np.asarray(Y, dtype=Z)
        assert Y.shape[0] == self.basis.shape[0] and Y.shape[1] <= self.basis.shape[2], "no Arnoldi basis of that shape"
        for s, c in enumerate(dst_cols):
            x = self.basis[s][:, :Y.shape[1]] @ Y[s]
            self.slots[dst_slot][:, c] = x / np.linalg.norm(x) if normalise else x


# ----------------------------------------------------------------------------------------------------
# inputs of the cases
# ----------------------------------------------------------------------------------------------------
def pencil_smallest(ctx, cA, cM, op, k=3):
    """(the k eigenvalues of smallest modulus of op(A) x = lambda op(M) x sorted by modulus, their eigenvectors) by scipy's shift-invert
    Arnoldi at 0 (a sparse LU: the penalty rows of 1e15 on the diagonal leave a dense QZ no accuracy for the small eigenvalues)"""
    lam, X = spla.eigs(op_matrix(ctx.terms, cA, op), k=k, M=op_matrix(ctx.terms, cM, op), sigma=0, tol=0,
                       v0=np.ones(ctx.n, dtype=Z))
    order = np.argsort(np.abs(lam))
    return lam[order], X[:, order]


def starts(ctx, kind, cA, cM, op, rng, eps=1e-6):
    """start columns, one per coefficient row.  kind: a string of one letter per system -- 'e' the eigenvector of smallest |lambda|
    perturbed at eps, 'r' random, 'z' zero"""
    cA, cM = rows(cA, len(kind)), rows(cM, len(kind))
    V0 = np.zeros((ctx.n, len(kind)), dtype=Z)
    for s, kd in enumerate(kind):
        g = rng.standard_normal(ctx.n) + 1j * rng.standard_normal(ctx.n)
        if kd == "e":
            x = pencil_smallest(ctx, cA[s], cM[s], op)[1][:, 0]
            V0[:, s] = x / np.linalg.norm(x) + eps * g / np.linalg.norm(g)
        elif kd == "r":
            V0[:, s] = g
    return V0


def reference_run(ctx, V0, cA, cM, op, m, need=1e-13):
    """arnoldi_ref on apply_S for the non-zero columns; asserts that the solves of the reference reached `need`: 1e-3 of the smallest
    bound the run is used in (tol = ritz_tol = 1e-10)"""
    live = np.any(V0 != 0, axis=0)
    cA, cM = rows(cA, V0.shape[1])[live], rows(cM, V0.shape[1])[live]
    worst = [0.0]

    def Sfun(X):
        Y, res = apply_S(ctx, X, cA, cM, op)
        worst[0] = max(worst[0], float(res.max()))
        return Y
    out = arnoldi_ref(Sfun, V0[:, live], m)
    assert worst[0] <= need, ("the reference's own solves", worst[0], need)
    out["solve_residual"] = worst[0]
    return out


def first_order_bounds(ctx, cA, cM, op, lam, x):
    """for a computed eigenpair (lam, x) of op(A) x = lambda op(M) x: (the pencil's eigenvalue of smallest modulus, the bound
    2 ||w|| ||r|| / |w^H op(M) x| on |lam - lambda|, the same with a diagonal weight), r = op(A) x - lam op(M) x, all in clongdouble.
    w is scipy's left eigenvector; lambda is the two-sided Rayleigh quotient w^H op(A) x_0 / w^H op(M) x_0 of scipy's pair evaluated in
    clongdouble (its error is of second order in theirs).  The bound is the identity (lambda - lam) w^H op(M) x = w^H r and the
    Cauchy-Schwarz inequality, with 2 for w's own error; |w^H r| <= ||D w|| ||D^-1 r|| holds for every positive diagonal D as well, and
    D = |diag op(A)| takes the penalty rows of 1e15, over which the plain ||r|| is taken, out of it."""
    opl = {"N": "C", "C": "N", "T": "T"}[op]
    assert op != "T"
    cA1, cM1 = rows(cA, 1), rows(cM, 1)
    x0 = pencil_smallest(ctx, cA1[0], cM1[0], op)[1][:, :1].astype(LD)
    w = pencil_smallest(ctx, cA1[0], cM1[0], opl)[1][:, 0].astype(LD)
    lam0 = np.sum(np.conj(w) * ctx.lev.apply(cA1, op, x0, LD)[:, 0]) / np.sum(np.conj(w) * ctx.lev.apply(cM1, op, x0, LD)[:, 0])
    xl = np.asarray(x).astype(LD)[:, None]
    Mx = ctx.lev.apply(cM1, op, xl, LD)[:, 0]
    r = ctx.lev.apply(cA1, op, xl, LD)[:, 0] - LD(lam) * Mx
    den = abs(np.sum(np.conj(w) * Mx))
    D = np.abs(ctx.lev.diag(cA1, op, 1, LD)[:, 0])
    nrm = lambda v: _norm(v[:, None])[0]
    return complex(lam0), float(2 * nrm(w) * nrm(r) / den), float(2 * nrm(D * w) * nrm(r / D) / den)
