"""Pins tests/_forcingref.py -- the CPU reference of the speaker source vectors, the point probes and the frequency sweep -- with checks
that do not go through it: the boundary matrix of the golden fixture, analytic sums, polynomial fields.  No library, no device."""
import numpy as np
import pytest

import _forcingref as F
import _p2ref as R

RNG = np.random.default_rng(17)


@pytest.fixture(scope="module")
def rijke():
    return F.rijke_mesh()


def plain_p1_source(pts, tris, c_tri):
    """s_a = sum over the triangles at a of c * 2 * area / 6, written out in plain numpy (a third of c * area per corner)"""
    s = np.zeros(len(pts))
    for t, c in zip(tris, c_tri):
        a = 0.5 * np.linalg.norm(np.cross(pts[t[1]] - pts[t[0]], pts[t[2]] - pts[t[0]]))
        s[t] += c * a / 3.0
    return s


def areas(pts, tris):
    return 0.5 * np.linalg.norm(np.cross(pts[tris[:, 1]] - pts[tris[:, 0]], pts[tris[:, 2]] - pts[tris[:, 0]]), axis=1)


def test_row_sums_of_the_golden_boundary_matrix(rijke):
    """partition of unity: sum_b int c phi_a phi_b = int c phi_a, so s = (i C) 1 with the golden C"""
    pts, tets, tris, c_tri = rijke
    rows = (1j * F.rijke_terms()["C"]) @ np.ones(len(pts))
    assert np.max(np.abs(rows.imag)) == 0.0
    for what, s in (("plain numpy", plain_p1_source(pts, tris, c_tri)), ("_forcingref", F.source(pts, tets, tris, 1, c_tri=c_tri))):
        err = np.max(np.abs(s - rows.real)) / np.max(np.abs(rows))
        print(f"{what}: max|s - (iC)1| = {err:.3e} relative")
        assert err <= 1e-13


def test_p2_point_entries_vanish_for_a_constant_c(rijke):
    pts, tets, tris, c_tri = rijke
    S, _ = F.element_vectors_exact(2)
    assert all(x == 0 for x in S[:3]) and all(x > 0 for x in S[3:])
    s = F.source(pts, tets, tris, 2, c_tri=c_tri)
    assert np.all(s[:len(pts)] == 0.0) and np.count_nonzero(s[len(pts):]) > 0


@pytest.mark.parametrize("order", [1, 2])
def test_total_is_the_integral_of_c(rijke, order):
    pts, tets, tris, c_tri = rijke
    want = np.sum(c_tri * areas(pts, tris))
    got = F.source(pts, tets, tris, order, c_tri=c_tri).sum()
    assert abs(got - want) <= 1e-12 * abs(want)
    cp = 300.0 + 50.0 * pts[:, 0] - 20.0 * pts[:, 1]                  # linear: the integral is area * mean of the corner values
    want = np.sum(cp[tris].mean(axis=1) * areas(pts, tris))
    got = F.source(pts, tets, tris, order, c_point=cp).sum()
    assert abs(got - want) <= 1e-12 * abs(want)


@pytest.mark.parametrize("order", [1, 2])
def test_a_constant_nodal_c_reproduces_the_per_triangle_vector(rijke, order):
    pts, tets, tris, _ = rijke
    a = F.source(pts, tets, tris, order, c_tri=np.full(len(tris), 347.0))
    b = F.source(pts, tets, tris, order, c_point=np.full(len(pts), 347.0))
    assert np.max(np.abs(a - b)) <= 1e-13 * np.max(np.abs(a))


def test_no_triangles_no_source(rijke):
    pts, tets, _, _ = rijke
    assert not F.source(pts, tets, np.zeros((0, 3), dtype=int), 1).any() and not F.source(pts, tets, np.zeros((0, 3), dtype=int), 2).any()


@pytest.mark.parametrize("order", [1, 2])
def test_probes_reproduce_polynomial_fields(rijke, order):
    """weights sum to 1; a linear (P1) resp. quadratic (P2) field and its gradient are reproduced at random interior points"""
    pts, tets, _, _ = rijke
    nodes = tets if order == 1 else R.connectivity(len(pts), tets)[1]
    xdof = pts if order == 1 else np.vstack([pts, 0.5 * (pts[R.edge_list(tets)[:, 0]] + pts[R.edge_list(tets)[:, 1]])])
    g0, H = np.array([0.3, -1.2, 0.7]), np.array([[1.0, 0.4, -0.3], [0.4, -2.0, 0.6], [-0.3, 0.6, 0.5]]) * (order == 2)
    field = lambda x: 2.0 + x @ g0 + 0.5 * np.einsum("...i,ij,...j->...", x, H, x)
    v = field(xdof)
    scale = np.max(np.abs(v))
    for t in RNG.integers(0, len(tets), 12):
        lam = RNG.dirichlet(np.ones(4))
        x = lam @ pts[tets[t]]
        n = RNG.standard_normal(3)
        idx, w = F.probe_p(pts, nodes, t, x, order)
        assert abs(w.sum() - 1.0) <= 1e-12
        assert abs(w @ v[idx] - field(x)) <= 1e-12 * scale
        idx, gw = F.probe_n_grad_p(pts, nodes, t, x, n, order)
        bound = 1e-12 * np.sum(np.abs(gw))                            # weights are O(1 / edge length): rounding relative to their size
        assert abs(gw.sum()) <= bound                                 # the gradient of the constant field
        assert abs(gw @ v[idx] - n @ (g0 + H @ x)) <= bound * scale


def test_the_rijke_sweep_is_benign():
    """with Y = 1e15 the solution equals A on the speaker surface, and the listed frequencies stay away from the resonances"""
    pts, tets, tris, _ = F.rijke_mesh()
    omegas, m, X = F.rijke_p1_sweep()
    outlet = np.unique(tris)
    err = np.max(np.abs(X[outlet] - F.RIJKE["A"]))
    amp = np.max(np.abs(X), axis=0)
    print(f"worst outlet error {err:.3e}; max|p| per frequency {np.array2string(amp, precision=2)}")
    assert err <= 1e-12
    assert amp.min() >= 1.0 and amp.max() <= 50.0
