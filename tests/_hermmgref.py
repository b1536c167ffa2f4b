"""Host reference of the Hermite p-hierarchy (numpy / scipy, no device): the two prolongators of wae_hermite_prolongators by a route other
than the product's, the power iteration behind the per-level weight scale (opts[12] of the set-up), and the three-level cycle
Hermite -> point unknowns -> P1 inside a left-preconditioned GMRES(30).  tests/test_hermmg_ref.py pins it by properties.

P_face.  The product writes the centroid formula down; here the cubic is FITTED, face by face: in the 9-dimensional space
V9 = P2 + span{l_i^2 l_j - l_i l_j^2} of the triangle (l: barycentric coordinates; the antisymmetric edge cubics are what the nine vertex
data see of a cubic beyond the quadratics -- the tenth cubic, the bubble l_1 l_2 l_3, has no vertex data at all) the function with the
given nine data -- the 3 values and the 6 edge derivatives grad u(a_p) . (a_q - a_p) -- is found by solving the 9 x 9 system, and
evaluated at the centroid.

P_lin.  A loop over the points: the P1 gradient of every tetrahedron around the point from a 4 x 4 solve ([1 x] c = e_k), averaged with the
volumes as weights.

Seeded defects (``defect=``): "sixth" (the gradient entries of P_face doubled: 1/6 -> 1/3), "unweighted" (a plain mean in P_lin),
"signed" (det J instead of |det J| as the weight)."""
import functools
import os

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import _hermref as R

POWER_STEPS = 40          # WAE_WEIGHT_POWER_STEPS of include/waehip.h
BASE_WEIGHTS = (0.8, 0.9)  # pre / post, the set-up's defaults


# ---- meshes and the Rijke operator -----------------------------------------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHAPES = ["one", "two", "cube", "rijke"]


@functools.lru_cache(maxsize=None)
def mesh(name):
    """(points, tets, tris) of the meshes of tests/test_gpu_herm.py: one tetrahedron; two on a shared face, one listed with det J < 0;
    the Kuhn cube of 48 with only its top face listed; the Rijke tube"""
    if name == "one":
        pts = np.array([[0.0, 0.0, 0.0], [1.0, 0.1, 0.0], [0.2, 0.9, 0.1], [0.1, 0.2, 0.8]])
        return pts, np.array([[0, 1, 2, 3]], dtype=np.int32), np.array([[0, 1, 2], [3, 1, 0]], dtype=np.int32)
    if name == "two":
        pts = np.array([[0.1, 0.2, 1.1], [1.0, 0.0, 0.1], [0.3, 0.1, -0.9], [0.0, 0.0, 0.0], [0.1, 1.2, 0.0]])
        tets = np.array([[3, 1, 4, 0], [3, 1, 4, 2]], dtype=np.int32)
        dets = [np.linalg.det((pts[t[:3]] - pts[t[3]]).T) for t in tets]
        assert dets[0] * dets[1] < 0
        return pts, tets, np.array([[4, 1, 0], [2, 3, 1]], dtype=np.int32)
    if name == "cube":
        return R.kuhn_cube(2)
    z = np.load(os.path.join(GOLDEN, "rijke_mesh.npz"))
    return z["points"], z["tetrahedra"], z["outlet_triangles"]


@functools.lru_cache(maxsize=None)
def rijke_terms():
    """M, K, C, Q of the Hermite Rijke tube from tests/_hermref.py (float64), as helmholtz_family takes them"""
    pts, tets, tris = mesh("rijke")
    z = np.load(os.path.join(GOLDEN, "rijke_mesh.npz"))
    fl = np.load(os.path.join(GOLDEN, "rijke_flame.npz"))
    M, K = R.assemble(pts, tets, tris, z["c_tet"])
    Cm, _ = R.assemble_boundary(pts, tets, tris, z["outlet_c"])
    Q = R.assemble_flame(pts, tets, tris, fl["flame_tets"], int(fl["ref_tet"]), np.array([0.0, 0.0, -0.00101]), fl["n_ref"], float(fl["nglobal_scaled"]))[0]
    return {"M": M, "K": K, "C": Cm, "Q": Q}


def rijke_operator(w, t=None, Y=1e15, n=1.0, tau=1e-3):
    """L(w) of helmholtz_family on those terms: w^2 M + K + w Y C + n exp(-i w tau) Q"""
    t = rijke_terms() if t is None else t
    return sp.csr_matrix(w * w * t["M"] + t["K"] + w * Y * t["C"] + n * np.exp(-1j * w * tau) * t["Q"])


# ---- P_face ---------------------------------------------------------------------------------------------------------------------------
def _v9(lam):
    """values (..., 9) of the basis of V9 at barycentric points lam (..., 3), and d/dl (..., 3, 9)"""
    l = [lam[..., i] for i in range(3)]
    zero = np.zeros_like(l[0])
    val, grad = [], []
    for i in range(3):                                                # l_i^2
        val.append(l[i] * l[i])
        grad.append([2 * l[i] if k == i else zero for k in range(3)])
    for i, j in ((0, 1), (0, 2), (1, 2)):                             # l_i l_j
        val.append(l[i] * l[j])
        grad.append([l[j] if k == i else l[i] if k == j else zero for k in range(3)])
    for i, j in ((0, 1), (0, 2), (1, 2)):                             # l_i^2 l_j - l_i l_j^2
        val.append(l[i] * l[i] * l[j] - l[i] * l[j] * l[j])
        grad.append([2 * l[i] * l[j] - l[j] * l[j] if k == i else l[i] * l[i] - 2 * l[i] * l[j] if k == j else zero for k in range(3)])
    return np.stack(val, axis=-1), np.stack([np.stack(g, axis=-1) for g in grad], axis=-1)


def centroid_weights():
    """w (9,): u(centroid) = sum_k w_k d_k(u) for u in V9, d = (u(a_0), u(a_1), u(a_2), then for p = 0, 1, 2 and the two q != p ascending
    the edge derivative grad u(a_p) . (a_q - a_p))"""
    E = np.eye(3)
    val, grad = _v9(E)                                                 # at the vertices: (3, 9), (3, 3, 9)
    rows = [val[p] for p in range(3)]
    for p in range(3):
        for q in range(3):
            if q != p:
                rows.append((E[q] - E[p]) @ grad[p])                  # d/dt u(a_p + t (a_q - a_p)) in barycentric coordinates
    F = np.array(rows)                                                 # functional k of basis function j
    assert abs(np.linalg.det(F)) > 1e-3
    c, _ = _v9(np.full(3, 1.0 / 3.0))
    return np.linalg.solve(F.T, c)


def p_face_ref(points, tets, tris=None, defect=None):
    """P_face (ndof x 4N), the faces numbered as tests/_hermref.connectivity numbers them"""
    pts = np.asarray(points, dtype=np.float64)
    N = len(pts)
    faces, _, _, ndof = R.connectivity(N, tets, tris)
    tr = np.zeros((0, 3), dtype=np.int64) if tris is None else np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    allf = np.sort(np.concatenate([tr, np.asarray(faces, dtype=np.int64).reshape(-1, 3)]), axis=1)
    w = centroid_weights()
    rows, cols, vals = [np.arange(4 * N)], [np.arange(4 * N)], [np.ones(4 * N)]
    for f, abc in enumerate(allf):
        k = 3
        for p in range(3):
            rows.append([4 * N + f]); cols.append([abc[p]]); vals.append([w[p]])
            g = np.zeros(3)
            for q in range(3):
                if q != p:
                    g += w[k] * (pts[abc[q]] - pts[abc[p]])
                    k += 1
            if defect == "sixth":
                g = 2 * g
            rows.append([4 * N + f] * 3); cols.append([(1 + i) * N + abc[p] for i in range(3)]); vals.append(g)
    A = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(ndof, 4 * N)).tocsr()
    A.sort_indices()
    return A


# ---- P_lin ----------------------------------------------------------------------------------------------------------------------------
def p_lin_ref(points, tets, defect=None):
    """P_lin (4N x N) by a loop over the points; entries that cancel stay in the pattern"""
    pts = np.asarray(points, dtype=np.float64)
    tets = np.asarray(tets, dtype=np.int64).reshape(-1, 4)
    N = len(pts)
    around = [[] for _ in range(N)]
    for t, tet in enumerate(tets):
        for p in tet:
            around[p].append(t)
    grads, dets = [], []
    for tet in tets:
        V = np.hstack([np.ones((4, 1)), pts[tet]])                    # lambda_k(x) = c_k0 + c_k[1:] . x,  V c_k = e_k
        grads.append(np.linalg.solve(V, np.eye(4))[1:, :])            # (3, 4): d lambda_k / d x_i
        dets.append(np.linalg.det((pts[tet[:3]] - pts[tet[3]]).T))
    rows, cols, vals = [], [], []
    for p in range(N):
        rows.append(p); cols.append(p); vals.append(1.0)
        acc, wsum = {}, 0.0
        for t in around[p]:
            wt = 1.0 if defect == "unweighted" else dets[t] if defect == "signed" else abs(dets[t])
            wsum += wt
            for k in range(4):
                acc[tets[t][k]] = acc.get(tets[t][k], np.zeros(3)) + wt * grads[t][:, k]
        for c in sorted(acc):
            for i in range(3):
                rows.append((1 + i) * N + p); cols.append(c); vals.append(acc[c][i] / wsum)
    A = sp.coo_matrix((vals, (rows, cols)), shape=(4 * N, N))
    A = sp.csr_matrix((A.data, (A.row, A.col)), shape=A.shape)        # (no duplicates; explicit zeros are kept)
    A.sort_indices()
    return A


def point_weights(points, tets):
    """W_p = sum of |det J| over the tetrahedra around p"""
    pts = np.asarray(points, dtype=np.float64)
    tets = np.asarray(tets, dtype=np.int64).reshape(-1, 4)
    d = np.abs(np.linalg.det(np.transpose(pts[tets[:, :3]] - pts[tets[:, 3:4]], (0, 2, 1))))
    W = np.zeros(len(pts))
    np.add.at(W, tets.reshape(-1), np.repeat(d, 4))
    return W, d


# ---- properties -----------------------------------------------------------------------------------------------------------------------
def quadratics():
    """the ten monomials of degree <= 2 as (f, grad f) taking (m, 3) positions"""
    out = []
    for a, b, c in [e for e in R.EXPONENTS if sum(e) <= 2]:
        def f(x, a=a, b=b, c=c):
            return x[:, 0] ** a * x[:, 1] ** b * x[:, 2] ** c

        def g(x, a=a, b=b, c=c):
            o = np.zeros((len(x), 3))
            if a:
                o[:, 0] = a * x[:, 0] ** (a - 1) * x[:, 1] ** b * x[:, 2] ** c
            if b:
                o[:, 1] = b * x[:, 0] ** a * x[:, 1] ** (b - 1) * x[:, 2] ** c
            if c:
                o[:, 2] = c * x[:, 0] ** a * x[:, 1] ** b * x[:, 2] ** (c - 1)
            return o
        out.append((f, g, a + b + c))
    return out


def properties(points, tets, tris, Pf, Pl):
    """the five figures that pin the prolongators, each a relative error:
    quad: P_face reproduces the DoF vector of every quadratic (largest miss / largest entry of that vector);
    lin: P_lin reproduces the point unknowns of every linear function (the miss of a row relative to (|P_lin| |u|) of that row plus max |u|: the
         gradient entries are of size 1/h and cancel);
    grad_rows: the gradient rows of P_lin sum to 0 (relative to the row's largest entry);
    unit_rows: the value rows of P_lin and all rows of P_face' value part sum to 1 (value and face rows);
    volume: sum_p W_p (P_lin u)_{grad, p} = 4 sum_t |det J_t| grad u_t for random P1 functions u -- the mean is the volume-weighted one."""
    pts = np.asarray(points, dtype=np.float64)
    N = len(pts)
    faces, _, _, _ = R.connectivity(N, tets, tris)
    out = {"quad": 0.0, "lin": 0.0}
    for f, g, deg in quadratics():
        u = R.dofs(pts, faces, tris, f, g)
        out["quad"] = max(out["quad"], np.max(np.abs(Pf @ u[:4 * N] - u)) / np.max(np.abs(u)))
        if deg <= 1:
            out["lin"] = max(out["lin"], np.max(np.abs(Pl @ u[:N] - u[:4 * N]) / (abs(sp.csr_matrix(Pl)) @ np.abs(u[:N]) + np.max(np.abs(u)))))
    Pl = sp.csr_matrix(Pl)
    s = np.asarray(Pl.sum(axis=1)).ravel()
    big = np.asarray(abs(Pl).max(axis=1).todense()).ravel()
    out["grad_rows"] = float(np.max(np.abs(s[N:]) / big[N:]))
    # value rows of P_lin; value and face rows of P_face restricted to the value columns
    sf = np.asarray(sp.csr_matrix(Pf)[:, :N].sum(axis=1)).ravel()
    out["unit_rows"] = float(max(np.max(np.abs(s[:N] - 1)), np.max(np.abs(sf[:N] - 1)), np.max(np.abs(sf[4 * N:] - 1))))
    W, d = point_weights(pts, tets)
    tt = np.asarray(tets, dtype=np.int64).reshape(-1, 4)
    rng = np.random.default_rng(5)
    worst = 0.0
    for _ in range(3):
        u = rng.standard_normal(N)
        gu = np.stack([np.linalg.solve(np.hstack([np.ones((4, 1)), pts[t]]), u[t])[1:] for t in tt])       # (nt, 3): grad u on every tetrahedron
        want = 4 * (d[:, None] * gu).sum(axis=0)
        got = (W[None, :] * (Pl @ u)[N:].reshape(3, N)).sum(axis=1)
        worst = max(worst, float(np.max(np.abs(got - want)) / np.sum(d[:, None] * np.abs(gu))))
    out["volume"] = worst
    return out


# ---- level operators, spectral estimates -------------------------------------------------------------------------------------------------
def penalty_rows(A, ratio=1e8):
    dg = np.abs(A.diagonal())
    return dg > ratio * np.median(dg)


def hierarchy(A_ref, Ps):
    """the set-up's rule for supplied prolongators: the penalty rows of the fine level leave prolongator 0, a column left without entries
    leaves its level and the rows of the next prolongator.  Returns the prolongators as the hierarchy uses them, finest first"""
    Ps = [sp.csr_matrix(P).astype(np.float64) for P in Ps]
    keep = ~penalty_rows(A_ref)                                       # the rows of prolongator k that its level still has
    out = []
    for k in range(len(Ps)):
        idx = np.nonzero(keep)[0]
        sub = Ps[k][idx]
        used = np.zeros(Ps[k].shape[1], dtype=bool)
        used[sub.indices] = True
        cols = np.nonzero(used)[0]
        if k == 0:                                                     # the fine level keeps its penalty rows, empty
            S = sp.csr_matrix((np.ones(len(idx)), (idx, np.arange(len(idx)))), shape=(Ps[0].shape[0], len(idx)))
            out.append(sp.csr_matrix(S @ sub[:, cols]))
        else:                                                          # a coarser level has lost the dropped columns' rows for good
            out.append(sp.csr_matrix(sub[:, cols]))
        keep = used
    return out


def level_operators(A, Ps):
    """A_0 = A, A_{l+1} = P_l^T A_l P_l (complex CSR)"""
    ops = [sp.csr_matrix(A)]
    for P in Ps:
        ops.append(sp.csr_matrix(P.T @ ops[-1] @ P))
    return ops


def start_vector(n):
    i = np.arange(n, dtype=np.uint64)
    return ((((i * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(16)).astype(np.float64)) / 32768.0 - 1.0


def power_estimate(A, steps=POWER_STEPS, perm=None):
    """the host restatement of the set-up's estimate of lambda_max(D^-1 Re A), D = diag(Re A): `steps` steps of the power iteration on
    |D|^-1/2 Re(A) |D|^-1/2 from the library's start vector (perm: the library's row numbering, row i of it = row perm[i] here)"""
    Ar = sp.csr_matrix(A).real.astype(np.float64).tocsr()
    if perm is not None:
        Ar = Ar[perm][:, perm]
    d = Ar.diagonal()
    s = np.where(d != 0, 1.0 / np.sqrt(np.abs(np.where(d != 0, d, 1.0))), 0.0)
    v = start_vector(Ar.shape[0])
    prev = np.linalg.norm(v)
    lam = 0.0
    for _ in range(steps):
        v = (1.0 / prev) * (s * (Ar @ (s * v)))
        lam = prev = np.linalg.norm(v)
    return float(lam)


def lambda_max(A):
    """lambda_max(D^-1 Re A) by scipy's Arnoldi (largest real part)"""
    Ar = sp.csr_matrix(A).real.astype(np.float64).tocsr()
    d = Ar.diagonal()
    B = sp.diags(1.0 / d) @ Ar
    ev = spla.eigs(B, k=1, which="LR", return_eigenvectors=False, tol=1e-10, v0=np.ones(B.shape[0]), maxiter=20000)
    return float(ev[0].real)


def scale_of(lam):
    return min(1.0, 5.0 / (3.0 * 1.1 * lam))


# ---- the three-level cycle in GMRES(30) ---------------------------------------------------------------------------------------------------
class Cycle:
    """V(1,1): scalar Jacobi with the weights 0.8 s_l before and 0.9 s_l after the coarse correction on every level but the last, which is
    solved exactly"""

    def __init__(self, ops, Ps, scales):
        self.ops, self.Ps, self.scales = ops, Ps, scales
        self.dinv = [1.0 / A.diagonal() for A in ops[:-1]]
        self.lu = spla.splu(sp.csc_matrix(ops[-1]))

    def apply(self, b, l=0):
        if l == len(self.ops) - 1:
            return self.lu.solve(b)
        A, P, s = self.ops[l], self.Ps[l], self.scales[l]
        x = BASE_WEIGHTS[0] * s * self.dinv[l] * b
        x = x + P @ self.apply(P.T @ (b - A @ x), l + 1)
        return x + BASE_WEIGHTS[1] * s * self.dinv[l] * (b - A @ x)


def gmres_left(A, M, b, tol=1e-10, maxit=300, restart=30):
    """left-preconditioned GMRES(restart) from zero on ||M(b - A x)|| / ||M b||, the residual recomputed at every restart.
    Returns (x, iterations, final relative preconditioned residual)"""
    x = np.zeros_like(b, dtype=np.complex128)
    beta0 = np.linalg.norm(M(b))
    its, rel = 0, 1.0
    while its < maxit:
        r = M(b - A @ x)
        beta = np.linalg.norm(r)
        rel = beta / beta0
        if rel <= tol or not np.isfinite(rel):
            break
        V = [r / beta]
        H = np.zeros((restart + 1, restart), dtype=np.complex128)
        k = 0
        y = None
        while k < restart and its < maxit:
            w = M(A @ V[k])
            for i in range(k + 1):
                H[i, k] = np.vdot(V[i], w)
                w = w - H[i, k] * V[i]
            H[k + 1, k] = np.linalg.norm(w)
            V.append(w / H[k + 1, k])
            k += 1
            its += 1
            e1 = np.zeros(k + 1, dtype=np.complex128)
            e1[0] = beta
            y, res, _, _ = np.linalg.lstsq(H[:k + 1, :k], e1, rcond=None)
            rel = np.linalg.norm(H[:k + 1, :k] @ y - e1) / beta0
            if rel <= tol or not np.isfinite(rel):
                break
        x = x + np.stack(V[:k], axis=1) @ y
        if not np.isfinite(rel):
            break
    r = M(b - A @ x)
    return x, its, float(np.linalg.norm(r) / beta0)


def rhs(n, r):
    """the right-hand sides of the solve tests: r seeded random complex columns"""
    rng = np.random.default_rng(340)
    return rng.standard_normal((n, r)) + 1j * rng.standard_normal((n, r))
