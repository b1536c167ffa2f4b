"""CPU reference of the stiffness and admittance-boundary matrices with a NODAL speed of sound, for tests only: it shares no code with
the product.  One value c_p per mesh point, c(x) = sum_p c_p l_p on every simplex (l: barycentric coordinates of its 4 resp. 3 corners):

    K_ab = -|det J| int c(x)^2 grad(phi_a).grad(phi_b)                  (tetrahedra)
    b_ab = |(x0-x2) x (x1-x2)| int c(x) phi_a phi_b,    C = -i b        (boundary triangles)

for the P1 basis phi_a = l_a (order 1) and the P2 basis of tests/_p2ref.py (order 2).  Built on that file's exact-rational polynomials:
with d phi_a / d l_i the polynomial _diff gives,

    T[a, b, i, j, p, q] = int l_p l_q (d phi_a / d l_i)(d phi_b / d l_j)        B[a, b, p] = int l_p phi_a phi_b

are Fractions from the monomial formula (_integral), rounded once to doubles; a local matrix is their contraction with
grad l_i . grad l_j and the corner values, and the global one a scipy coo_matrix sum, numbering as _p2ref.connectivity."""
import functools
from fractions import Fraction

import numpy as np
import scipy.sparse as sp

from _p2ref import _diff, _integral, _mul, basis, connectivity, kuhn_cube  # noqa: F401  (kuhn_cube: for the tests that import this file)


def _unit(nv, i):
    e = [0] * nv; e[i] = 1
    return {tuple(e): Fraction(1)}


def functions(nv, order):
    """the basis polynomials in local order: P1 = the barycentric coordinates themselves, P2 = _p2ref.basis"""
    if order == 1:
        return [_unit(nv, i) for i in range(nv)]
    assert order == 2
    return basis(nv)


@functools.lru_cache(maxsize=None)
def stiffness_tensor(order):
    """T[a, b, i, j, p, q] on the reference tetrahedron (|det J| = 1)"""
    fs = functions(4, order)
    n = len(fs)
    d = [[_diff(f, i) for i in range(4)] for f in fs]
    ll = {(p, q): _mul(_unit(4, p), _unit(4, q)) for p in range(4) for q in range(p, 4)}
    T = np.zeros((n, n, 4, 4, 4, 4))
    for a in range(n):
        for b in range(n):
            for i in range(4):
                for j in range(4):
                    dd = _mul(d[a][i], d[b][j])
                    if not dd:
                        continue
                    for (p, q), lpq in ll.items():
                        T[a, b, i, j, p, q] = T[a, b, i, j, q, p] = float(_integral(_mul(dd, lpq), 4))
    return T


@functools.lru_cache(maxsize=None)
def boundary_tensor(order):
    """B[a, b, p] on the reference triangle (|(x0-x2) x (x1-x2)| = 1)"""
    fs = functions(3, order)
    n = len(fs)
    B = np.zeros((n, n, 3))
    for a in range(n):
        for b in range(n):
            ab = _mul(fs[a], fs[b])
            for p in range(3):
                B[a, b, p] = float(_integral(_mul(ab, _unit(3, p)), 3))
    return B


def _coo(nodes, local, dim):
    """sum the local matrices (nelements, n, n) on the nodes (nelements, n) into a CSR matrix with sorted indices"""
    n = nodes.shape[1]
    A = sp.coo_matrix((local.ravel(), (np.repeat(nodes, n, axis=1).ravel(), np.tile(nodes, (1, n)).ravel())), shape=(dim, dim)).tocsr()
    A.sum_duplicates(); A.sort_indices()
    return A


def _dofs(points, tets, tris, order):
    """(dimension, nodes per tetrahedron, nodes per triangle)"""
    tets = np.asarray(tets, dtype=np.int64).reshape(-1, 4)
    tr = None if tris is None else np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    if order == 1:
        return len(points), tets, tr
    edges, t10, t6 = connectivity(len(points), tets, tr)
    return len(points) + len(edges), t10, t6


def stiffness(points, tets, c_point, order):
    """K of the mesh as a real CSR matrix"""
    points = np.asarray(points, dtype=float)
    c_point = np.asarray(c_point, dtype=float)
    assert c_point.shape == (len(points),)
    dim, nodes, _ = _dofs(points, tets, None, order)
    X = points[nodes[:, :4]]                                          # (ntets, 4, 3)
    J = np.transpose(X[:, :3] - X[:, 3:4], (0, 2, 1))
    Ji = np.linalg.inv(J)
    G = np.concatenate([Ji, -Ji.sum(axis=1, keepdims=True)], axis=1)
    GG = G @ np.transpose(G, (0, 2, 1))
    c = c_point[nodes[:, :4]]
    Tc = np.einsum("abijpq,tp,tq->tabij", stiffness_tensor(order), c, c, optimize=True)
    Kl = -np.abs(np.linalg.det(J))[:, None, None] * np.einsum("tabij,tij->tab", Tc, GG)
    return _coo(nodes, Kl, dim)


def boundary(points, tets, tris, c_point, order):
    """C = -i b of the boundary triangles as a complex CSR matrix (tets: for the edge numbers of the P2 space)"""
    points = np.asarray(points, dtype=float)
    c_point = np.asarray(c_point, dtype=float)
    assert c_point.shape == (len(points),)
    dim, _, nodes = _dofs(points, tets, tris, order)
    X = points[nodes[:, :3]]
    det = np.linalg.norm(np.cross(X[:, 0] - X[:, 2], X[:, 1] - X[:, 2]), axis=1)
    bl = det[:, None, None] * np.einsum("abp,tp->tab", boundary_tensor(order), c_point[nodes[:, :3]])
    return -1j * _coo(nodes, bl, dim)


def dof_points(points, tets, order):
    """coordinates of the DoFs: the mesh points and, for order 2, the edge midpoints in the order of their numbers"""
    points = np.asarray(points, dtype=float)
    if order == 1:
        return points
    edges, _, _ = connectivity(len(points), tets)
    return np.vstack([points, 0.5 * (points[edges[:, 0]] + points[edges[:, 1]])])
