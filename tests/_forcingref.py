"""CPU reference of the forced-response feature, for tests only: it shares no code with the product.

  * the speaker source vector  s_a = |(x0-x2) x (x1-x2)| int c(x) phi_a  over boundary triangles, c per triangle or linear between the
    corner values, for the P1 basis phi_a = l_a and the P2 basis of tests/_p2ref.py.  The element vectors are Fractions: the basis
    polynomials are expanded (tests/_p2ref.py keeps them as {exponent tuple: Fraction}) and integrated with the monomial formula
    int l^alpha = alpha! / (|alpha| + 2)!  (_p2ref._integral); no closed form is typed in;
  * the point probes get_p / get_n_grad_p as weights on the nodes of one tetrahedron, from the same polynomials (_p2ref._value, _diff);
  * the sweep  x_j = L(w_j)^{-1} (w_j Y A m),  L(w) = w^2 M + K + w Y C + n exp(-i w tau) Q,  assembled with scipy, solved with splu.

Pinned by tests/test_forcing_ref.py."""
import functools
import os

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from _nodalref import _unit, functions
from _p2ref import _diff, _integral, _mul, _value, barycentric_gradients, connectivity

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FREQS_HZ = (50.0, 100.0, 150.0, 200.0, 250.0, 300.0, 400.0, 500.0, 700.0, 1000.0)       # the Rijke P1 sweep
RIJKE = dict(Y=1e15, n=0.01, tau=1e-3, A=1.0)


# ---- element vectors ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def element_vectors_exact(order):
    """(S[a] = int phi_a, SC[p][a] = int l_p phi_a) on the reference triangle (|(x0-x2) x (x1-x2)| = 1), as Fractions"""
    fs = functions(3, order)
    S = [_integral(f, 3) for f in fs]
    SC = [[_integral(_mul(_unit(3, p), f), 3) for f in fs] for p in range(3)]
    return S, SC


def element_vectors(order):
    S, SC = element_vectors_exact(order)
    return np.array([float(x) for x in S]), np.array([[float(x) for x in row] for row in SC])


def _nodes(points, tets, tris, order):
    tris = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    if order == 1:
        return len(points), tris
    edges, _, t6 = connectivity(len(points), tets, tris)
    return len(points) + len(edges), t6


def source(points, tets, tris, order, c_tri=None, c_point=None):
    """the dense real vector s (tets: for the edge numbers of the P2 space)"""
    points = np.asarray(points, dtype=float)
    dim, nodes = _nodes(points, tets, tris, order)
    s = np.zeros(dim)
    if not len(nodes):
        return s
    X = points[nodes[:, :3]]
    det = np.linalg.norm(np.cross(X[:, 0] - X[:, 2], X[:, 1] - X[:, 2]), axis=1)
    S, SC = element_vectors(order)
    if c_point is not None:
        assert c_tri is None
        local = det[:, None] * (np.asarray(c_point, dtype=float)[nodes[:, :3]] @ SC)
    else:
        c = np.ones(len(nodes)) if c_tri is None else np.asarray(c_tri, dtype=float)
        local = (c * det)[:, None] * S[None, :]
    np.add.at(s, nodes.ravel(), local.ravel())
    return s


# ---- probes -------------------------------------------------------------------------------------------------------------------------
def _local(points, tets, t, x):
    X = np.asarray(points, dtype=float)[np.asarray(tets)[t][:4]]
    G, _ = barycentric_gradients(X)
    lam3 = G[:3] @ (np.asarray(x, dtype=float) - X[3])
    return np.append(lam3, 1.0 - lam3.sum()), G


def probe_p(points, nodes, t, x, order):
    """weights of p(x) on the nodes of tetrahedron t (nodes: (ntets, 4) for order 1, the 10-node connectivity for order 2)"""
    lam, _ = _local(points, nodes, t, x)
    return np.asarray(nodes)[t], np.array([_value(f, lam) for f in functions(4, order)])


def probe_n_grad_p(points, nodes, t, x, n, order):
    """weights of n . grad p(x)"""
    lam, G = _local(points, nodes, t, x)
    gn = G @ np.asarray(n, dtype=float)
    return np.asarray(nodes)[t], np.array([sum(_value(_diff(f, i), lam) * gn[i] for i in range(4)) for f in functions(4, order)])


# ---- sweep --------------------------------------------------------------------------------------------------------------------------
def operator(t, w, Y, n, tau):
    return sp.csc_matrix(w * w * t["M"] + t["K"] + w * Y * t["C"] + n * np.exp(-1j * w * tau) * t["Q"])


def sweep(t, m, omegas, Y, n, tau, A):
    """X (d x nfreq): column j = L(w_j)^{-1} (w_j Y A m);  m: dense complex vector"""
    m = np.asarray(m, dtype=np.complex128).reshape(-1)
    return np.column_stack([spla.splu(operator(t, w, Y, n, tau)).solve(w * Y * A * m) for w in omegas])


def rijke_mesh():
    z = np.load(os.path.join(GOLDEN, "rijke_mesh.npz"))
    return z["points"], z["tetrahedra"], z["outlet_triangles"], z["outlet_c"]


def rijke_terms():
    z = np.load(os.path.join(GOLDEN, "rijke_p1.npz"))
    d = int(z["d"])
    return {k: sp.csr_matrix((z[f"{k}_data"], z[f"{k}_indices"], z[f"{k}_indptr"]), shape=(d, d)) for k in ("M", "K", "C", "Q")}


@functools.lru_cache(maxsize=None)
def rijke_p1_sweep():
    """(omegas, m, X) of the Rijke P1 sweep with the golden matrices: computed once, shared, not to be modified"""
    pts, tets, tris, c_tri = rijke_mesh()
    m = -1j * source(pts, tets, tris, 1, c_tri=c_tri)
    omegas = 2 * np.pi * np.array(FREQS_HZ)
    X = sweep(rijke_terms(), m, omegas, **RIJKE)
    X.setflags(write=False)
    return omegas, m, X
