"""CPU reference of the Hermite (cubic) tetrahedral discretisation, for tests only: it shares no code with the product or with the table
generator, and it takes another route.  The product recombines reference-element matrices with J; this file builds every element's basis
on the physical element.

The element: P3 on the tetrahedron p0..p3; the basis is dual to the 20 functionals
    local 0..3    u(p_k)                                            global p_k
    local 4..15   du/dx_i (p_k) at 4 (1 + i) + k                    global (1 + i) N + p_k
    local 16..19  u at the centroid of the face opposite p_k        global 4 N + face number.
With the monomials of degree <= 3 in y = (x - centre) / h (centre, h: centroid and longest edge of the element, which keeps the system
well conditioned; the gradient functionals are scaled by h for the same reason and the scaling is undone on the functions) the
coefficients of the basis are the inverse of the functional-by-monomial matrix.  In float64 that is numpy's inverse; in numpy.longdouble
the float64 inverse is refined by two Newton-Schulz steps X <- X (2 - A X) carried out in longdouble.  Integrals: Gauss-Legendre rules on
the collapsed cube (exact for the degree at hand: 6 for M and the boundary, 4 for K, 3 for the flame), nodes and weights polished by
Newton's method in the working precision.

The boundary matrix is NOT built from a 13-DoF triangle element: it is the face integral of the traces of the 20 functions of the
tetrahedron behind the triangle.  The 13 DoF that live on the face are scattered (full coupling, zeros kept); the traces of the other 7
functions vanish, `assemble_boundary` returns the largest entry they produce.

Face numbering: the triangle at position t of `tris` is face t, every other tetrahedron face follows as ntris + rank, rank ascending by
(largest, middle, smallest point) -- np.unique on the rows (largest, middle, smallest)."""
import functools
from itertools import permutations

import numpy as np
import scipy.sparse as sp

EXPONENTS = [(a, b, c) for a in range(4) for b in range(4) for c in range(4) if a + b + c <= 3]
FACE_OF = [[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]]                # face k lies opposite point k


# ---- connectivity -----------------------------------------------------------------------------------------------------------------
def connectivity(npoints, tets, tris=None):
    """(faces (ninner, 3) as (smallest, middle, largest), tets20, tris13, ndof), 0-based; KeyError for a triangle that is no face"""
    tets = np.asarray(tets, dtype=np.int64).reshape(-1, 4)
    tris = np.zeros((0, 3), dtype=np.int64) if tris is None else np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    allf = np.sort(np.concatenate([tets[:, f] for f in FACE_OF]), axis=1)[:, ::-1]          # rows (largest, middle, smallest)
    uniq = np.unique(allf, axis=0)                                                            # lexicographic: by largest, then middle, then smallest
    number = {}
    for t, tri in enumerate(tris.tolist()):
        key = tuple(sorted(tri, reverse=True))
        if key in number:
            raise ValueError("triangle listed twice")
        number[key] = t
    listed = set(number)
    if not listed <= set(map(tuple, uniq.tolist())):
        raise KeyError("a triangle is no tetrahedron's face")
    inner = [f for f in map(tuple, uniq.tolist()) if f not in listed]
    for r, f in enumerate(inner):
        number[f] = len(tris) + r
    N = int(npoints)
    t20 = np.zeros((len(tets), 20), dtype=np.int64)
    for k in range(4):
        for blk in range(4):
            t20[:, 4 * blk + k] = blk * N + tets[:, k]
        t20[:, 16 + k] = [4 * N + number[tuple(sorted(row, reverse=True))] for row in tets[:, FACE_OF[k]].tolist()]
    t13 = np.zeros((len(tris), 13), dtype=np.int64)
    for k in range(3):
        for blk in range(4):
            t13[:, 3 * blk + k] = blk * N + tris[:, k]
    t13[:, 12] = 4 * N + np.arange(len(tris))
    faces = np.array([f[::-1] for f in inner], dtype=np.int64).reshape(-1, 3)
    return faces, t20, t13, 4 * N + len(uniq)


def dofs(points, faces, tris, f, grad_f):
    """the DoF vector of a function: values, x, y, z derivatives at the points, then the values at the face centroids (tris first)"""
    points = np.asarray(points)
    tris = np.zeros((0, 3), dtype=np.int64) if tris is None else np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    allf = np.concatenate([tris, np.asarray(faces, dtype=np.int64).reshape(-1, 3)])
    cen = (points[allf[:, 0]] + points[allf[:, 1]] + points[allf[:, 2]]) / 3
    g = grad_f(points)
    return np.concatenate([f(points), g[:, 0], g[:, 1], g[:, 2], f(cen)])


# ---- quadrature -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gauss01(n, dtype):
    """n-point Gauss-Legendre rule on [0, 1] in the given precision"""
    x = np.polynomial.legendre.leggauss(n)[0].astype(dtype)
    for _ in range(3):                                                # Newton on P_n with the three-term recurrence
        p0, p1 = np.ones_like(x), x.copy()
        for k in range(2, n + 1):
            p0, p1 = p1, ((2 * k - 1) * x * p1 - (k - 1) * p0) / k
        dp = n * (x * p1 - p0) / (x * x - 1)
        x = x - p1 / dp
    p0, p1 = np.ones_like(x), x.copy()
    for k in range(2, n + 1):
        p0, p1 = p1, ((2 * k - 1) * x * p1 - (k - 1) * p0) / k
    dp = n * (x * p1 - p0) / (x * x - 1)
    w = 2 / ((1 - x * x) * dp * dp)
    return (x + 1) / 2, w / 2


@functools.lru_cache(maxsize=None)
def tet_rule(degree, dtype):
    """(barycentric coordinates (nq, 4), weights (nq,)) exact for polynomials of that degree on the tetrahedron; the weights sum to 1/6"""
    (u, wu), (v, wv), (w, ww) = _gauss01((degree + 4) // 2, dtype), _gauss01((degree + 3) // 2, dtype), _gauss01((degree + 2) // 2, dtype)
    U, V, W = np.meshgrid(u, v, w, indexing="ij")
    wt = (wu[:, None, None] * wv[None, :, None] * ww[None, None, :] * (1 - U) ** 2 * (1 - V)).ravel()
    x0, x1, x2 = U.ravel(), (V * (1 - U)).ravel(), (W * (1 - U) * (1 - V)).ravel()
    return np.stack([x0, x1, x2, 1 - x0 - x1 - x2], axis=1), wt


@functools.lru_cache(maxsize=None)
def tri_rule(degree, dtype):
    """(barycentric coordinates (nq, 3), weights (nq,)) on the triangle; the weights sum to 1/2"""
    (u, wu), (v, wv) = _gauss01((degree + 3) // 2, dtype), _gauss01((degree + 2) // 2, dtype)
    U, V = np.meshgrid(u, v, indexing="ij")
    wt = (wu[:, None] * wv[None, :] * (1 - U)).ravel()
    x0, x1 = U.ravel(), (V * (1 - U)).ravel()
    return np.stack([x0, x1, 1 - x0 - x1], axis=1), wt


# ---- the basis on the physical element -----------------------------------------------------------------------------------------------
def _monomials(Y):
    """Y (..., 3) -> (values (..., 20), gradients (..., 3, 20)) of the monomials y^e"""
    P = [np.ones_like(Y), Y, Y * Y, Y * Y * Y]                        # P[k][..., j] = y_j^k
    val = np.stack([P[a][..., 0] * P[b][..., 1] * P[c][..., 2] for a, b, c in EXPONENTS], axis=-1)
    zero = np.zeros_like(Y[..., 0])
    grad = np.stack([
        np.stack([a * P[a - 1][..., 0] * P[b][..., 1] * P[c][..., 2] if a else zero for a, b, c in EXPONENTS], axis=-1),
        np.stack([b * P[a][..., 0] * P[b - 1][..., 1] * P[c][..., 2] if b else zero for a, b, c in EXPONENTS], axis=-1),
        np.stack([c * P[a][..., 0] * P[b][..., 1] * P[c - 1][..., 2] if c else zero for a, b, c in EXPONENTS], axis=-1)], axis=-2)
    return val, grad


class Elements:
    """the Hermite bases of a batch of tetrahedra X (nt, 4, 3) in the precision of X: coef[t, m, a] = coefficient of monomial m in the
    function a, in the element's scaled coordinates y = (x - centre) / h"""

    def __init__(self, X):
        X = np.asarray(X)
        self.dtype = X.dtype.type
        self.X = X
        self.centre = X.mean(axis=1)
        edges = np.stack([X[:, i] - X[:, j] for i in range(4) for j in range(i + 1, 4)], axis=1)
        self.h = np.sqrt((edges.astype(np.float64) ** 2).sum(axis=2).max(axis=1)).astype(X.dtype)
        J = np.transpose(X[:, :3] - X[:, 3:4], (0, 2, 1)).astype(np.float64)
        self.det = self._det3(np.transpose(X[:, :3] - X[:, 3:4], (0, 2, 1)))
        assert np.all(np.sign(np.linalg.det(J)) == np.sign(self.det.astype(np.float64)))
        Yv = self.scaled(X)                                                   # (nt, 4, 3)
        Yc = self.scaled(np.stack([X[:, f].mean(axis=1) for f in FACE_OF], axis=1))
        vv, gv = _monomials(Yv)
        vc, _ = _monomials(Yc)
        A = np.concatenate([vv, gv[:, :, 0], gv[:, :, 1], gv[:, :, 2], vc], axis=1)      # (nt, 20 functionals, 20 monomials); gradients times h
        Xi = np.linalg.inv(A.astype(np.float64))
        if self.dtype is not np.float64:
            Xi = Xi.astype(X.dtype)
            two = 2 * np.eye(20, dtype=X.dtype)
            for _ in range(2):
                Xi = Xi @ (two - A @ Xi)
        self.residual = float(np.max(np.abs(A @ Xi - np.eye(20, dtype=X.dtype))))
        Xi = Xi.copy()
        Xi[:, :, 4:16] *= self.h[:, None, None]                               # functional h d/dx -> function / h; undo
        self.coef = Xi

    @staticmethod
    def _det3(J):
        return (J[:, 0, 0] * (J[:, 1, 1] * J[:, 2, 2] - J[:, 1, 2] * J[:, 2, 1]) - J[:, 0, 1] * (J[:, 1, 0] * J[:, 2, 2] - J[:, 1, 2] * J[:, 2, 0])
                + J[:, 0, 2] * (J[:, 1, 0] * J[:, 2, 1] - J[:, 1, 1] * J[:, 2, 0]))

    def scaled(self, x):
        """physical positions (nt, n, 3) -> scaled coordinates"""
        return (x - self.centre[:, None, :]) / self.h[:, None, None]

    def values(self, x):
        """the 20 functions at the positions x (nt, n, 3) -> (nt, n, 20)"""
        return _monomials(self.scaled(x))[0] @ self.coef

    def gradients(self, x):
        """physical gradients -> (nt, n, 3, 20)"""
        g = _monomials(self.scaled(x))[1] / self.h[:, None, None, None]
        return np.stack([g[:, :, i] @ self.coef for i in range(3)], axis=2)

    def at_barycentric(self, lam):
        """positions of the barycentric points lam (nq, 4) in every element -> (nt, nq, 3)"""
        return np.einsum("qk,tkd->tqd", lam.astype(self.X.dtype), self.X)


def local_matrices(X, c=None):
    """(M, K, S) of the tetrahedra X (nt, 4, 3): M = |det J| int phi_a phi_b, K = -c^2 |det J| int grad phi_a . grad phi_b, S = |det J| int phi_a"""
    E = Elements(X)
    dt = E.dtype
    adet = np.abs(E.det)
    lam, w = tet_rule(6, dt)
    F = E.values(E.at_barycentric(lam))
    M = adet[:, None, None] * (np.swapaxes(F * w[None, :, None], 1, 2) @ F)
    S = adet[:, None] * np.einsum("q,tqa->ta", w, F)
    lam, w = tet_rule(4, dt)
    G = E.gradients(E.at_barycentric(lam))
    K = sum(np.swapaxes(G[:, :, i] * w[None, :, None], 1, 2) @ G[:, :, i] for i in range(3))
    cc = np.ones(len(adet), dtype=X.dtype) if c is None else np.asarray(c).astype(X.dtype)
    return M, -(cc * cc * adet)[:, None, None] * K, S


# ---- assembly ---------------------------------------------------------------------------------------------------------------------
def _csr(rows, cols, vals, dim):
    """sum the triplets in the precision they come in (sorted by key, np.add.reduceat), then hand float64 or complex to scipy"""
    rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    key = rows * dim + cols
    order = np.argsort(key, kind="stable")
    key, vals = key[order], vals[order]
    first = np.concatenate([[True], key[1:] != key[:-1]])
    summed = np.add.reduceat(vals, np.nonzero(first)[0])
    uk = key[first]
    A = sp.csr_matrix((summed.astype(np.float64), (uk // dim, uk % dim)), shape=(dim, dim))
    A.sort_indices()
    return A, summed


def _chunks(n, size=1024):
    return [slice(i, min(i + size, n)) for i in range(0, n, size)]


def assemble(points, tets, tris=None, c_tet=None, dtype=np.float64):
    """(M, K) of the mesh as float64 CSR matrices with one pattern, every sum formed in `dtype`"""
    points = np.asarray(points).astype(dtype)
    tets = np.asarray(tets, dtype=np.int64).reshape(-1, 4)
    _, t20, _, dim = connectivity(len(points), tets, tris)
    Ms, Ks = [], []
    for s in _chunks(len(tets)):
        M, K, _ = local_matrices(points[tets[s]], None if c_tet is None else np.asarray(c_tet)[s])
        Ms.append(M.ravel()); Ks.append(K.ravel())
    rows, cols = [np.repeat(t20, 20, axis=1).ravel()], [np.tile(t20, (1, 20)).ravel()]
    return _csr(rows, cols, Ms, dim)[0], _csr(rows, cols, Ks, dim)[0]


def tet_behind(tets, tri):
    """(index of a tetrahedron that has the triangle as a face, local positions of the triangle's points in it, local position of the fourth)"""
    tets = np.asarray(tets, dtype=np.int64).reshape(-1, 4)
    hit = np.nonzero(np.isin(tets, tri).sum(axis=1) == 3)[0]
    t = int(hit[0])
    loc = [int(np.nonzero(tets[t] == p)[0][0]) for p in tri]
    return t, loc, [k for k in range(4) if k not in loc][0]


def assemble_boundary(points, tets, tris, c_tri=None, dtype=np.float64):
    """(C, stray): C = -i b, b_ab = c |(x0-x2) x (x1-x2)| int phi_a phi_b over the boundary triangles with phi the traces of the functions of
    the tetrahedron behind; stray = the largest |entry| of the 7 functions that do not live on the face, relative to the largest of b"""
    points = np.asarray(points).astype(dtype)
    tets = np.asarray(tets, dtype=np.int64).reshape(-1, 4)
    tris = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    _, t20, t13, dim = connectivity(len(points), tets, tris)
    lam3, w = tri_rule(6, dtype)
    rows, cols, vals, stray, big = [], [], [], 0.0, 0.0
    for s, tri in enumerate(tris):
        t, loc, opp = tet_behind(tets, tri)
        E = Elements(points[tets[t]][None])
        q = points[tri]
        x = np.einsum("qk,kd->qd", lam3.astype(dtype), q)[None]
        F = E.values(x)[0]                                                        # (nq, 20)
        n = np.cross(q[0] - q[2], q[1] - q[2])
        area2 = np.sqrt((n * n).sum())
        B = (1 if c_tri is None else dtype(c_tri[s])) * area2 * ((F * w[:, None]).T @ F)
        on = loc + [4 + k for k in loc] + [8 + k for k in loc] + [12 + k for k in loc] + [16 + opp]
        assert np.array_equal(t20[t, on], t13[s]), "the triangle's DoF are not those of the tetrahedron behind it"
        off = [a for a in range(20) if a not in on]
        big = max(big, float(np.max(np.abs(B[np.ix_(on, on)]))))
        stray = max(stray, float(np.max(np.abs(B[off, :]))))
        rows.append(np.repeat(t13[s], 13)); cols.append(np.tile(t13[s], 13)); vals.append(B[np.ix_(on, on)].ravel())
    b, _ = _csr(rows, cols, vals, dim)
    return -1j * b.astype(complex), stray / big


def assemble_flame(points, tets, tris, flame_tets, ref_tet, x_ref, n_ref, nglobal_scaled, dtype=np.float64):
    """(Q, flame volume, S (ndof,), g (ndof,)): Q = sum_flame S (x) g, S_a = |det J| int phi_a, g_b = -nlocal grad phi_b(x_ref) . n_ref"""
    points = np.asarray(points).astype(dtype)
    tets = np.asarray(tets, dtype=np.int64).reshape(-1, 4)
    flame_tets = np.asarray(flame_tets, dtype=np.int64)
    _, t20, _, dim = connectivity(len(points), tets, tris)
    E = Elements(points[tets[flame_tets]])
    lam, w = tet_rule(3, dtype)
    F = E.values(E.at_barycentric(lam))
    S = np.abs(E.det)[:, None] * np.einsum("q,tqa->ta", w, F)
    # an integral that vanishes identically (the gradient functions: S . u = int p in tests/test_herm_ref.py holds only if it does) comes out
    # of the rule as rounding noise; what lies below 64 eps |det J| max|phi_a| is that noise and is set to the zero it stands for
    S[np.abs(S) < 64 * np.finfo(dtype).eps * np.abs(E.det)[:, None] * np.max(np.abs(F), axis=1)] = 0
    volume = np.abs(E.det).sum() / 6
    R = Elements(points[tets[int(ref_tet)]][None])
    grad = R.gradients(np.asarray(x_ref).astype(dtype)[None, None, :])[0, 0]     # (3, 20)
    g = -(dtype(nglobal_scaled) / volume) * (np.asarray(n_ref).astype(dtype) @ grad)
    ref = t20[int(ref_tet)]
    rows = [np.repeat(t20[flame_tets], 20, axis=1).ravel()]
    cols = [np.tile(ref, (len(flame_tets), 20)).ravel()]
    Q, _ = _csr(rows, cols, [(S[:, :, None] * g[None, None, :]).ravel()], dim)
    Sg, gg = np.zeros(dim, dtype=dtype), np.zeros(dim, dtype=dtype)
    np.add.at(Sg, t20[flame_tets].ravel(), S.ravel())
    gg[ref] = g
    return Q.astype(complex), float(volume), Sg.astype(np.float64), gg.astype(np.float64)


# ---- comparison -------------------------------------------------------------------------------------------------------------------
def dof_class(index, npoints):
    """0 = value, 1 = derivative, 2 = face"""
    index = np.asarray(index)
    return np.where(index < npoints, 0, np.where(index < 4 * npoints, 1, 2))


def blockwise_distance(A, B, npoints):
    """{(class of row, class of column): max|A - B| / max|B| over that block} for two CSR matrices with one pattern; a block that is all zero
    in B counts 0.0 if it is all zero in A too and inf otherwise, an empty block is left out"""
    assert A.shape == B.shape and np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices)
    rc = dof_class(np.repeat(np.arange(A.shape[0]), np.diff(A.indptr)), npoints)
    cc = dof_class(A.indices, npoints)
    out = {}
    for r in range(3):
        for c in range(3):
            sel = (rc == r) & (cc == c)
            if sel.any() and np.max(np.abs(B.data[sel])) > 0:
                out[(r, c)] = float(np.max(np.abs(A.data[sel] - B.data[sel])) / np.max(np.abs(B.data[sel])))
            elif sel.any():
                out[(r, c)] = 0.0 if np.all(A.data[sel] == 0) else float("inf")
    return out


# ---- meshes -----------------------------------------------------------------------------------------------------------------------
def kuhn_cube(n, length=1.0):
    """Kuhn triangulation of [0, length]^3 with n^3 cells, 6 tetrahedra per cell.  Returns (points, tets, top), top = the boundary triangles
    of the face z = length"""
    idx = lambda i, j, k: (i * (n + 1) + j) * (n + 1) + k
    g = np.arange(n + 1) * (length / n)
    points = np.array([[g[i], g[j], g[k]] for i in range(n + 1) for j in range(n + 1) for k in range(n + 1)])
    tets = []
    for i in range(n):
        for j in range(n):
            for k in range(n):
                for perm in permutations(range(3)):
                    p = [i, j, k]
                    tet = [idx(*p)]
                    for ax in perm:
                        p[ax] += 1
                        tet.append(idx(*p))
                    tets.append(tet)
    tets = np.array(tets, dtype=np.int32)
    zmax = set(np.nonzero(np.isclose(points[:, 2], length))[0].tolist())
    top = sorted({tuple(sorted(int(tet[a]) for a in f)) for tet in tets for f in FACE_OF if all(int(tet[a]) in zmax for a in f)})
    return points, tets, np.array(top, dtype=np.int32)


def smallest_nonzero_eigenvalue(M, K):
    """smallest eigenvalue above the constant mode's 0 of (-K) u = w^2 M u (scipy eigsh, shift-invert)"""
    import scipy.sparse.linalg as spla
    A = sp.csc_matrix(-K).real.astype(float)
    B = sp.csc_matrix(M).real.astype(float)
    A = (A + A.T) / 2
    B = (B + B.T) / 2
    lam = spla.eigsh(A, k=6, M=B, sigma=5.0, which="LM", return_eigenvectors=False)
    return float(np.min(lam[lam > 1.0]))
