"""CPU reference of the P2 (second-order) tetrahedral discretisation, for tests only: it shares no code with the product.

Basis on a simplex with barycentric coordinates l_1..l_n (n = 4: tetrahedron, n = 3: triangle): vertex functions l_i (2 l_i - 1), edge
functions 4 l_i l_j; local order: vertices, then the edges (1,2), (1,3), (1,4), (2,3), (2,4), (3,4) resp. (1,2), (1,3), (2,3).  Every basis
function is kept as a polynomial {exponent tuple: Fraction}; integrals come from the monomial formula
    int l^alpha = |det J| * prod(alpha_i!) / (|alpha| + n - 1)!
in exact rational arithmetic.  Edge DoFs are numbered npoints + position in np.unique of the sorted vertex pairs; matrices are
assembled with scipy.sparse.coo_matrix."""
from fractions import Fraction
from itertools import combinations, permutations
from math import factorial

import numpy as np
import scipy.sparse as sp


# ---- polynomials in the barycentric coordinates ---------------------------------------------------------------------------------
def _mul(p, q):
    out = {}
    for ea, ca in p.items():
        for eb, cb in q.items():
            e = tuple(x + y for x, y in zip(ea, eb))
            out[e] = out.get(e, Fraction(0)) + ca * cb
    return out


def _diff(p, i):
    out = {}
    for e, c in p.items():
        if e[i]:
            f = list(e); f[i] -= 1
            out[tuple(f)] = out.get(tuple(f), Fraction(0)) + c * e[i]
    return out


def _integral(p, nv):
    """int p over the reference simplex (|det J| = 1)"""
    s = Fraction(0)
    for e, c in p.items():
        num = 1
        for x in e:
            num *= factorial(x)
        s += c * Fraction(num, factorial(sum(e) + nv - 1))
    return s


def _value(p, lam):
    return sum(float(c) * np.prod([l ** x for l, x in zip(lam, e)]) for e, c in p.items())


def local_edges(nv):
    return list(combinations(range(nv), 2))


def basis(nv):
    """the P2 basis polynomials in local order"""
    def unit(i, power=1):
        e = [0] * nv; e[i] = power
        return tuple(e)
    fs = [{unit(i, 2): Fraction(2), unit(i): Fraction(-1)} for i in range(nv)]
    for i, j in local_edges(nv):
        e = [0] * nv; e[i] = 1; e[j] = 1
        fs.append({tuple(e): Fraction(4)})
    return fs


def local_mass_exact(nv):
    """int phi_a phi_b / |det J| as Fractions"""
    fs = basis(nv)
    return [[_integral(_mul(a, b), nv) for b in fs] for a in fs]


def local_source_exact(nv):
    return [_integral(a, nv) for a in basis(nv)]


def local_mass(nv):
    return np.array([[float(x) for x in row] for row in local_mass_exact(nv)])


def local_source(nv):
    return np.array([float(x) for x in local_source_exact(nv)])


_STIFF = None


def stiffness_tensor():
    """T[a, b, i, j] = int (d phi_a / d l_i)(d phi_b / d l_j) / |det J| on the tetrahedron"""
    global _STIFF
    if _STIFF is None:
        fs = basis(4)
        d = [[_diff(f, i) for i in range(4)] for f in fs]
        T = np.zeros((10, 10, 4, 4))
        for a in range(10):
            for b in range(10):
                for i in range(4):
                    for j in range(4):
                        T[a, b, i, j] = float(_integral(_mul(d[a][i], d[b][j]), 4))
        _STIFF = T
    return _STIFF


# ---- geometry -------------------------------------------------------------------------------------------------------------------
def barycentric_gradients(X):
    """X (4, 3) corners -> (grad l_a (4, 3), det J); corner 4 is the origin of the local coordinates"""
    J = (X[:3] - X[3]).T                       # columns x_a - x_4
    Ji = np.linalg.inv(J)                      # rows = grad l_1..l_3
    return np.vstack([Ji, -Ji.sum(axis=0)]), np.linalg.det(J)


def local_matrices(X, c=1.0):
    """(M, K) of one tetrahedron: M = |det J| int phi_a phi_b,  K = -c^2 |det J| int grad phi_a . grad phi_b"""
    G, det = barycentric_gradients(np.asarray(X, dtype=float))
    M = abs(det) * local_mass(4)
    K = -c * c * abs(det) * np.einsum("abij,ij->ab", stiffness_tensor(), G @ G.T)
    return M, K


def basis_gradients_at(X, x):
    """grad phi_b (10, 3) at the physical point x of the tetrahedron with corners X"""
    X = np.asarray(X, dtype=float)
    G, _ = barycentric_gradients(X)
    lam3 = G[:3] @ (np.asarray(x, dtype=float) - X[3])
    lam = np.append(lam3, 1.0 - lam3.sum())
    return np.array([sum(_value(_diff(f, i), lam) * G[i] for i in range(4)) for f in basis(4)])


# ---- connectivity -----------------------------------------------------------------------------------------------------------------
def edge_list(tets):
    tets = np.asarray(tets, dtype=np.int64).reshape(-1, 4)
    pairs = np.concatenate([tets[:, [i, j]] for i, j in local_edges(4)])
    return np.unique(np.sort(pairs, axis=1), axis=0)


def connectivity(npoints, tets, tris=None):
    """(edges (nedges, 2), tets10 (ntets, 10), tris6 (ntris, 6)), 0-based; raises KeyError for a triangle edge no tetrahedron has"""
    tets = np.asarray(tets, dtype=np.int64).reshape(-1, 4)
    edges = edge_list(tets)
    number = {(int(a), int(b)): npoints + k for k, (a, b) in enumerate(edges)}

    def extend(s, nv):
        out = np.zeros((len(s), nv + len(local_edges(nv))), dtype=np.int64)
        out[:, :nv] = s
        for col, (i, j) in enumerate(local_edges(nv)):
            out[:, nv + col] = [number[(min(a, b), max(a, b))] for a, b in zip(s[:, i].tolist(), s[:, j].tolist())]
        return out
    t6 = np.zeros((0, 6), dtype=np.int64) if tris is None else extend(np.asarray(tris, dtype=np.int64).reshape(-1, 3), 3)
    return edges, extend(tets, 4), t6


# ---- assembly ---------------------------------------------------------------------------------------------------------------------
def _coo(rows, cols, vals, dim):
    A = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(dim, dim)).tocsr()
    A.sum_duplicates(); A.sort_indices()
    return A


def assemble(points, tets, c_tet=None):
    """(M, K) of the mesh: local_matrices of every tetrahedron (all at once), summed by coo_matrix"""
    points = np.asarray(points, dtype=float)
    edges, t10, _ = connectivity(len(points), tets)
    dim = len(points) + len(edges)
    X = points[t10[:, :4]]                                            # (ntets, 4, 3)
    J = np.transpose(X[:, :3] - X[:, 3:4], (0, 2, 1))
    Ji = np.linalg.inv(J)
    G = np.concatenate([Ji, -Ji.sum(axis=1, keepdims=True)], axis=1)
    adet = np.abs(np.linalg.det(J))
    c = np.ones(len(t10)) if c_tet is None else np.asarray(c_tet, dtype=float)
    Ml = adet[:, None, None] * local_mass(4)
    Kl = (-c * c * adet)[:, None, None] * np.einsum("abij,tij->tab", stiffness_tensor(), G @ np.transpose(G, (0, 2, 1)))
    rows, cols = [np.repeat(t10, 10, axis=1).ravel()], [np.tile(t10, (1, 10)).ravel()]
    return _coo(rows, cols, [Ml.ravel()], dim), _coo(rows, cols, [Kl.ravel()], dim)


def assemble_boundary(points, tets, tris, c_tri=None):
    """C = -i b,  b_ab = c |(x0-x2) x (x1-x2)| int phi_a phi_b on the 6-node triangle"""
    points = np.asarray(points, dtype=float)
    edges, _, t6 = connectivity(len(points), tets, tris)
    dim = len(points) + len(edges)
    Mt = local_mass(3)
    rows, cols, vals = [], [], []
    for t, nodes in enumerate(t6):
        X = points[nodes[:3]]
        det = np.linalg.norm(np.cross(X[0] - X[2], X[1] - X[2]))
        rows.append(np.repeat(nodes, 6)); cols.append(np.tile(nodes, 6))
        vals.append(((1.0 if c_tri is None else float(c_tri[t])) * det * Mt).ravel())
    return -1j * _coo(rows, cols, vals, dim)


def assemble_flame(points, tets, flame_tets, ref_tet, x_ref, n_ref, nglobal_scaled):
    """(Q, flame volume): Q = sum_flame S (x) g,  S_a = |det J| int phi_a,  g_b = -nlocal grad phi_b(x_ref) . n_ref"""
    points = np.asarray(points, dtype=float)
    edges, t10, _ = connectivity(len(points), tets)
    dim = len(points) + len(edges)
    dets = np.array([abs(barycentric_gradients(points[t10[t, :4]])[1]) for t in flame_tets])
    volume = dets.sum() / 6.0
    ref = t10[int(ref_tet)]
    g = -(nglobal_scaled / volume) * (basis_gradients_at(points[ref[:4]], x_ref) @ np.asarray(n_ref, dtype=float))
    S = local_source(4)
    rows, cols, vals = [], [], []
    for t, det in zip(flame_tets, dets):
        rows.append(np.repeat(t10[t], 10)); cols.append(np.tile(ref, 10))
        vals.append(np.outer(det * S, g).ravel())
    return _coo(rows, cols, vals, dim).astype(complex), volume


# ---- meshes -----------------------------------------------------------------------------------------------------------------------
def kuhn_cube(n, length=1.0):
    """Kuhn triangulation of [0, length]^3 with n^3 cells, 6 tetrahedra per cell (one per order of the axes; half of them negatively
    oriented).  Returns (points, tets, top) with top = the boundary triangles of the face z = length."""
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
    top = []
    zmax = set(np.nonzero(np.isclose(points[:, 2], length))[0].tolist())
    for tet in tets:
        for f in combinations(range(4), 3):
            if all(int(tet[a]) in zmax for a in f):
                top.append([tet[a] for a in f])
    return points, tets, np.array(top, dtype=np.int32)


def assemble_p1(points, tets, c_tet=None):
    """the P1 pair (M, K) on the same mesh, for the convergence comparison: M_ab = |det J| (1 + delta_ab)/120, K_ab = -c^2 |det J|/6 grad l_a . grad l_b"""
    points = np.asarray(points, dtype=float)
    tets = np.asarray(tets, dtype=np.int64).reshape(-1, 4)
    rows, cols, mv, kv = [], [], [], []
    for t, nodes in enumerate(tets):
        G, det = barycentric_gradients(points[nodes])
        c = 1.0 if c_tet is None else float(c_tet[t])
        rows.append(np.repeat(nodes, 4)); cols.append(np.tile(nodes, 4))
        mv.append((abs(det) / 120.0 * (1.0 + np.eye(4))).ravel())
        kv.append((-c * c * abs(det) / 6.0 * (G @ G.T)).ravel())
    return _coo(rows, cols, mv, len(points)), _coo(rows, cols, kv, len(points))


def smallest_nonzero_eigenvalue(M, K):
    """smallest eigenvalue above the constant mode's 0 of (-K) u = w^2 M u (scipy eigsh, shift-invert)"""
    import scipy.sparse.linalg as spla
    A = sp.csc_matrix(-K).real.astype(float)
    B = sp.csc_matrix(M).real.astype(float)
    A = (A + A.T) / 2
    B = (B + B.T) / 2
    lam = spla.eigsh(A, k=6, M=B, sigma=5.0, which="LM", return_eigenvectors=False)
    return float(np.min(lam[lam > 1.0]))
