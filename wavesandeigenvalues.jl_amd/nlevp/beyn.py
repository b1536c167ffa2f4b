"""Beyn's contour-integral solver on the device family (reference: src/NLEVP/beyn.jl).

The quadrature loop -- ``length(Γ)·N`` times {assemble L(z), sparse LU, l solves} in the reference
(beyn.jl:62-74,112-138) -- is ONE call into libwaehip (``wae_beyn_moments``): all quadrature points and probe
columns are solved in lock-step batches by multigrid-GMRES and the moments are accumulated in HBM.  The small
dense tail (block Hankel SVD + eigen, beyn.jl:76-107) stays on the host, as in the reference (LAPACK) -- or, with
`moments2eigs_native` / `beyn_native`, keeps its tall half in HBM too (wae_tall_*) and only the (lK x lK) problems on the host.
"""
from __future__ import annotations

import numpy as np


def wn(z, G):
    """beyn.jl:185-209 winding number"""
    def isleft(a, b, c):
        return (b.real - a.real) * (c.imag - a.imag) - (c.real - a.real) * (b.imag - a.imag)
    z = complex(z)
    w = 0
    n = len(G)
    for i in range(n):
        a, b = complex(G[i]), complex(G[(i + 1) % n])
        if a.imag <= z.imag:
            if b.imag > z.imag and isleft(a, b, z) > 0:
                w += 1
        elif b.imag <= z.imag and isleft(a, b, z) < 0:
            w -= 1
    return w


def inpoly(z, G):
    """beyn.jl:178"""
    return wn(z, G) != 0


def gauss_points(G, N):
    """Nodes and effective weights of `gauss` (beyn.jl:112-138): N Gauss-Legendre points per polygon edge,
    weights already multiplied by (b-a)/2.  (FastGaussQuadrature.gausslegendre -> numpy leggauss.)"""
    X, W = np.polynomial.legendre.leggauss(N)
    zs, ws = [], []
    n = len(G)
    for i in range(n):
        a, b = complex(G[i]), complex(G[(i + 1) % n])
        zs.append(X * (b - a) / 2 + (a + b) / 2)
        ws.append(W * (b - a) / 2)
    return np.concatenate(zs), np.concatenate(ws)


def initialize_V(d, l):
    """beyn.jl:41-57 / :379-392 (random=false)"""
    V = np.zeros((d, l), dtype=np.complex128)
    for i in range(min(d, l)):
        V[i, i] = 1.0
    return V


def coefficient_table(L, zs):
    """row j = the T coefficients of L(z_j); leaves L.params[eigval] at the last point like repeated L(z) calls."""
    saved_active, saved_mode = L.active, L.mode
    L.active, L.mode = [L.eigval], "all"
    try:
        return np.array([L.coefficients(z) for z in zs], dtype=np.complex128).reshape(len(zs), len(L.terms))
    finally:
        L.active, L.mode = saved_active, saved_mode


def snapshot_split(n, S):
    """indices of S snapshot points spread evenly through a list of n quadrature points, and the remaining indices"""
    S = int(min(S, n))
    idx = np.unique(((np.arange(S) + 0.5) * n / max(S, 1)).astype(int)) if S > 0 else np.zeros(0, dtype=int)
    rest = np.setdiff1d(np.arange(n), idx)
    return idx, rest


def spread_order(idx):
    """bit-reversal-like order: every prefix of the list covers the whole contour (the snapshot solves are progressive:
    each chunk starts from the projection on the chunks before it)"""
    idx = list(idx)
    n = len(idx)
    if n < 3:
        return np.asarray(idx, dtype=int)
    bits = max(1, int(np.ceil(np.log2(n))))
    key = [int(format(i, f"0{bits}b")[::-1], 2) for i in range(n)]
    return np.asarray([idx[i] for i in np.argsort(key, kind="stable")], dtype=int)


def compute_moment_matrices(L, G, V=None, l=5, K=1, N=16, points=None, out_dev=0, rb=None):
    """beyn.jl:233-268.  ``points=(z, w)`` overrides the contour (used to shard the quadrature over GPUs).

    ``rb`` = number of snapshot points (default ``L.rb_snapshots``; None = 40, at most half of the points, when there are
    at least 64 points and d >= 1000 -- the measured optimum both for 128 points at C2 (of 32/40/48/56) and for 256 points at
    C3 (of 24...72: the count follows the solution manifold, not the quadrature); 0 = every system from a zero guess): the solutions
    at ``rb`` points spread along the contour are kept in HBM, all other points start from their Galerkin projection on
    those (wae_beyn_moments_rb); same moments to the inner tolerance, several times fewer Krylov iterations."""
    d = L.size()
    if V is None:
        V = initialize_V(d, l)
    zs, ws = gauss_points(G, N) if points is None else points
    zs, ws = np.asarray(zs), np.asarray(ws)
    fam = L.ensure_solver()
    ct = coefficient_table(L, zs) if len(zs) else np.zeros((0, len(L.terms)), dtype=np.complex128)
    rb = getattr(L, "rb_snapshots", None) if rb is None else rb
    if rb is None:                                   # automatic, for contours worth the set-up
        rb = min(40, len(zs) // 2) if (len(zs) >= 64 and d >= 1000) else 0
    if not rb or len(zs) < 2 * rb:
        return fam.beyn_moments(zs, ws, ct, V, K=K, tol=L.solver_tol, maxit=L.solver_maxit, out_dev=out_dev)
    idx, rest = snapshot_split(len(zs), rb)
    idx = spread_order(idx)
    kw = dict(K=K, tol=L.solver_tol, maxit=L.solver_maxit, out_dev=out_dev)
    cap = len(idx) + getattr(L, "rb_extra", 0)              # room for adaptive enrichment (WAE_RB_ENRICH)
    V = np.asarray(V)
    l = V.shape[1]
    NB = int(getattr(fam, "batch", 64))
    infos, A = [], None
    # the per-column snapshot bases are independent: probe columns beyond the solver's batch width are handled in slices
    # of <= NB columns (the reference accepts any l, beyn.jl:39-57), each slice = snapshot phase + projected phase
    for c0 in range(0, l, NB):
        Vs = V[:, c0:c0 + NB]
        sl = dict(l_total=l, col0=c0) if l > NB else {}
        A0 = fam.beyn_moments_rb(zs[idx], ws[idx], ct[idx], Vs, 0, cap, accumulate=bool(out_dev) and c0 > 0, **sl, **kw)
        i0 = dict(fam.last_info)
        if l > NB:
            A1 = fam.beyn_moments_rb(zs[rest], ws[rest], ct[rest], Vs, 2, cap, accumulate=bool(out_dev), **sl, **kw)
        else:   # V=None: the probe matrix uploaded by the snapshot call is still on the device
            A1 = fam.beyn_moments_rb(zs[rest], ws[rest], ct[rest], None, 2, cap, accumulate=bool(out_dev), l_total=l, **kw)
        infos.append((i0, dict(fam.last_info)))
        if not out_dev:
            A = A0 + A1 if A is None else A + A0 + A1
    fam.last_info = {"iters_max": max(max(a["iters_max"], b["iters_max"]) for a, b in infos),
                     "iters_total": sum(a["iters_total"] + b["iters_total"] for a, b in infos),
                     "n_unconverged": sum(a["n_unconverged"] + b["n_unconverged"] for a, b in infos), "levels": infos[-1][1]["levels"],
                     "relres_max": max(max(a["relres_max"], b["relres_max"]) for a, b in infos),
                     "seconds": sum(a["seconds"] + b["seconds"] for a, b in infos),
                     "snapshot_iters": sum(a["iters_total"] for a, _ in infos), "projected_iters": sum(b["iters_total"] for _, b in infos),
                     "snapshots": len(idx)}
    return None if out_dev else A


def moments2eigs(A_list, tol_sigma=0.0, return_sigma=False):
    """beyn.jl:289-323 (and :76-102)"""
    if isinstance(A_list, np.ndarray):
        A_list = [A_list]
    d, dl = A_list[0].shape[:2]
    l = len(A_list) * dl
    K = A_list[0].shape[2] // 2
    B0 = np.zeros((d * K, l * K), dtype=np.complex128)
    B1 = np.zeros((d * K, l * K), dtype=np.complex128)
    for i in range(K):
        for j in range(K):
            for ll, A in enumerate(A_list):
                c0 = ll * dl + l * j
                B0[d * i:d * (i + 1), c0:c0 + dl] = A[:, :, i + j]
                B1[d * i:d * (i + 1), c0:c0 + dl] = A[:, :, i + j + 1]
    if B0.shape[0] > 8 * B0.shape[1]:
        # tall-skinny: thin QR first, SVD of the small triangular factor (same factorisation up to rounding,
        # a few times cheaper than LAPACK's SVD of the d x l matrix)
        Q, R = np.linalg.qr(B0)
        Ur, S, Wh = np.linalg.svd(R)
        U = Q @ Ur
    else:
        U, S, Wh = np.linalg.svd(B0, full_matrices=False)
    W = Wh.conj().T
    if tol_sigma > 0:
        mask = S > tol_sigma
        U, S, W = U[:, mask], S[mask], W[:, mask]
    Om, P = np.linalg.eig(U.conj().T @ B1 @ W @ np.diag(1.0 / S))
    P = U[:d, :] @ P
    return (Om, P, S) if return_sigma else (Om, P)


def pos_test(Om, P, G):
    """beyn.jl:333-337"""
    mask = np.array([inpoly(z, G) for z in Om], dtype=bool)
    return Om[mask], P[:, mask]


def beyn(L, G, l=5, K=1, N=16, tol=0.0, pos_test_=True, output=False, random=False, return_sigma=False):
    """Ω, P = beyn(L, Γ; l, K, N, tol, pos_test, output, random)   (beyn.jl:34-110)"""
    d = L.size()
    K = max(K, l // d + int(l % d != 0))
    if random:
        rng = np.random.default_rng()
        V = rng.random((d, l)) + 1j * rng.random((d, l))
    else:
        V = initialize_V(d, l)
    A = compute_moment_matrices(L, G, V, K=K, N=N)
    Om, P, S = moments2eigs(A, tol_sigma=tol, return_sigma=True)
    if output:
        print("############\nsingular values:\n", S)
    if pos_test_:
        Om, P = pos_test(Om, P, G)
    return (Om, P, S) if return_sigma else (Om, P)


def moments2eigs_native(M, shape, tol_sigma=0.0, rel_tol=0.0, info=None):
    """`moments2eigs` (beyn.jl:289-323) with everything tall kept in HBM behind the C ABI (``wae_tall_*``): no torch, only the
    (lK x lK) problems run on the host (numpy).  M: a TallMatrix holding the d x (l 2K) moments (what ``out_dev=M.ptr`` of
    ``compute_moment_matrices`` leaves there), or a host array d x l x 2K that is uploaded.  shape = (d, l, 2K).
    rel_tol > 0 keeps the singular directions above rel_tol sigma_1 (the reference's `tol`, beyn.jl:92-95, relative), rel_tol = 0
    all of them; tol_sigma > 0 is the reference's absolute threshold on top.  For K = 1, B0 and B1 are column ranges of M itself:
    nothing is copied.  Returns (Omega, P as TallMatrix d x kept, Sigma of all l K directions); see tall.staged_extract."""
    from .tall import TallMatrix, staged_extract
    d, l, K2 = (int(v) for v in shape)
    K = K2 // 2
    uploaded = not hasattr(M, "gram")
    if uploaded:
        M = TallMatrix.from_host(np.asarray(M, dtype=np.complex128).reshape(d, l * K2, order="F"))
    if M.rows != d or M.ncols != l * K2:
        raise ValueError(f"moments2eigs_native: M is {M.rows} x {M.ncols}, shape says {d} x {l * K2}")
    n = l * K
    try:
        if K == 1:
            return staged_extract(M, 0, M, l, d, n, rel_tol=rel_tol, tol_sigma=tol_sigma, info=info)
        B0 = M.new(d * K, n).hankel(M, l, K, 0)
        B1 = M.new(d * K, n).hankel(M, l, K, 1)
        try:
            return staged_extract(B0, 0, B1, 0, d, n, rel_tol=rel_tol, tol_sigma=tol_sigma, info=info)
        finally:
            B0.release()
            B1.release()
    finally:
        if uploaded:
            M.destroy()


def beyn_native(L, G, l=5, K=1, N=16, rel_tol=1e-6, pos_test_=True):
    """`beyn` (beyn.jl:34-110) without a host copy of anything tall: the moments are written into a TallMatrix, the eigenpairs are
    extracted there (`moments2eigs_native`), the residual test of the pairs inside the contour reads P in HBM, and only those n
    eigenvectors come back.  Returns (Omega, P (d x n, numpy), Sigma, residuals of wae_eig_residuals)."""
    from .tall import TallMatrix
    d = L.size()
    K = max(K, l // d + int(l % d != 0))
    M = TallMatrix.create(d, l * 2 * K, device=L.device_id)
    try:
        compute_moment_matrices(L, G, initialize_V(d, l), K=K, N=N, out_dev=M.ptr)
        Om, P, S = moments2eigs_native(M, (d, l, 2 * K), rel_tol=rel_tol)
    finally:
        M.destroy()
    keep = np.array([inpoly(z, G) for z in Om], dtype=bool) if pos_test_ else np.ones(len(Om), dtype=bool)
    Om = Om[keep]
    if len(Om) == 0:
        P.release()
        return Om, np.zeros((d, 0), dtype=np.complex128), S, np.zeros(0)
    Pk = P.new(d, len(Om)).mul(P, np.eye(P.ncols)[:, keep])         # the kept columns, contiguous: the layout P_dev wants
    P.release()
    res = L.ensure_solver().eig_residuals(coefficient_table(L, Om), P_dev=Pk.ptr)
    Ph = Pk.to_host()
    Pk.release()
    return Om, Ph, S, res


# ------------------------------------------------------------------------------------------------------
# reduced-basis helpers  (beyn.jl:395-595)
# ------------------------------------------------------------------------------------------------------
def _orth_append(Q, x):
    """next column of the incremental QR (beyn.jl:604-626 uses Householder reflectors; Gram-Schmidt with
    re-orthogonalisation spans the same nested subspaces, only the column phases differ)."""
    x = np.array(x, dtype=np.complex128).ravel()
    for _ in range(2):
        if Q.shape[1]:
            x = x - Q @ (Q.conj().T @ x)
    return np.hstack([Q, (x / np.linalg.norm(x))[:, None]])


def generate_subspace(L, Y, tol, Z, N=None, output=False, tol_err=np.inf, include_Y=True):
    """Q, resnorm = generate_subspace(L, Y, tol, Z[, N])   (beyn.jl:429-577)

    Greedy orthonormal basis Q such that the Galerkin solution of L(z) x = y in span(Q) has residual <= tol for every
    sample point z in Z and every column y of Y (with N given, Z is a polygon and N Gauss-Legendre nodes per edge are
    the sample points).  The exact solves L(z)\\y and the products L(z)·Q run on the device; the small projected
    solves on the host.  As in the reference the residual is the plain 2-norm of L(z)X - y."""
    Y = np.asarray(Y, dtype=np.complex128)
    if Y.ndim == 1:
        Y = Y[:, None]
    d, k = Y.shape
    if N is not None:
        Z, _ = gauss_points(Z, N)
    Z = list(Z)
    Q = np.zeros((d, 0), dtype=np.complex128)
    A = L(Z[0])
    first = Y if include_Y else A.solve(Y)
    for kk in range(k):
        Q = _orth_append(Q, first[:, kk])
    resnorm = np.zeros(len(Z) * k)
    for idx, z in enumerate(Z):
        if Q.shape[1] == d:
            break
        A = L(z)
        AQ = A @ Q                                    # d x dim on the device, kept and extended column by column
        QY = Q.conj().T @ Y
        for kk in range(k):
            X = Q @ np.linalg.solve(Q.conj().T @ AQ, QY[:, kk])
            res = np.linalg.norm(A @ X - Y[:, kk])
            if res > tol:
                Q = _orth_append(Q, A.solve(Y[:, kk]))
                AQ = np.hstack([AQ, (A @ Q[:, -1])[:, None]])
                QY = Q.conj().T @ Y
                X = Q @ np.linalg.solve(Q.conj().T @ AQ, QY[:, kk])
                res = np.linalg.norm(A @ X - Y[:, kk])
            resnorm[kk + idx * k] = res
            if output:
                print(kk + idx * k + 1, "/", len(Z) * k, " dim", Q.shape[1], " res", res)
    return Q, resnorm


def project(L, Q):
    """P = project(L, Q): the family P(z) = Q' L(z) Q, term by term (beyn.jl:579-595).  The projected terms are small
    dense matrices; P is an ordinary (device-backed) family, so beyn / householder / ... run on it unchanged."""
    from .linopfam import LinearOperatorFamily, Term
    Q = np.asarray(Q, dtype=np.complex128)
    P = LinearOperatorFamily([L.eigval], [L.params[L.eigval]], device=L.device_id)
    P.params = dict(L.params)
    P.eigval, P.auxval, P.mode, P.active = L.eigval, L.auxval, L.mode, list(L.active)
    P.solver_tol, P.solver_maxit, P.solver_ref = L.solver_tol, L.solver_maxit, L.solver_ref
    P.solver_opts = {"max_coarse": max(128, Q.shape[1])}          # one dense level: the projected operator is inverted directly
    for k, t in enumerate(L.terms):
        M = Q.conj().T @ (L.term_operator(k) @ Q)
        P.push(Term(np.asarray(M), t.func, t.params, t.symbol, t.operator))
    for key, val in L.params.items():
        P.params[key] = val
    return P
