"""Pins of tests/_nodalref.py, the CPU reference of K and C with a nodal speed of sound, by facts that need no GPU and no library.
All on the unit cube kuhn_cube(2) with c = 1 + x, which the nodal (piecewise linear) form represents exactly, so every number below is
an integral of a polynomial that both element orders must reproduce:
    u = x:    u' K u = -int (1 + x)^2 |grad x|^2 = -7/3               u = x^2 (P2 only):   -int (1 + x)^2 4 x^2 = -62/15
    top face z = 1:   1' b 1 = int (1 + x) = 3/2                       u = x (P2):   int (1 + x) x^2 = 7/12
Tolerance 1e-12 relative; a constant field must reproduce the per-simplex references of tests/_p2ref.py to 1e-14 * max|entry|."""
import functools

import numpy as np
import pytest

import _nodalref as N
import _p2ref as R

TOL = 1e-12


@functools.lru_cache(maxsize=None)
def cube():
    pts, tets, top = N.kuhn_cube(2)
    return pts, tets, top, 1.0 + pts[:, 0]


@functools.lru_cache(maxsize=None)
def K(order):
    pts, tets, _, c = cube()
    return N.stiffness(pts, tets, c, order)


@functools.lru_cache(maxsize=None)
def b(order):
    pts, tets, top, c = cube()
    return (1j * N.boundary(pts, tets, top, c, order)).real.tocsr()


def x_of_dofs(order):
    pts, tets, _, _ = cube()
    return N.dof_points(pts, tets, order)[:, 0]


@pytest.mark.parametrize("order", [1, 2])
def test_linear_u(order):
    u = x_of_dofs(order)
    assert abs(u @ (K(order) @ u) + 7 / 3) <= TOL * 7 / 3


def test_quadratic_u():
    u = x_of_dofs(2) ** 2
    assert abs(u @ (K(2) @ u) + 62 / 15) <= TOL * 62 / 15


@pytest.mark.parametrize("order", [1, 2])
def test_null_space(order):
    A = K(order)
    assert np.max(np.abs(A @ np.ones(A.shape[0]))) <= TOL * np.max(np.abs(A.data))


@pytest.mark.parametrize("order", [1, 2])
def test_stiffness_is_symmetric(order):
    A = K(order)
    assert abs(A - A.T).max() <= TOL * np.max(np.abs(A.data))


@pytest.mark.parametrize("order", [1, 2])
def test_boundary_of_the_top_face(order):
    B = b(order)
    one = np.ones(B.shape[0])
    assert abs(one @ (B @ one) - 3 / 2) <= TOL * 3 / 2
    if order == 2:
        u = x_of_dofs(2)
        assert abs(u @ (B @ u) - 7 / 12) <= TOL * 7 / 12


def same(A, B):
    assert A.shape == B.shape and np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices)
    return np.max(np.abs(A.data - B.data)) <= 1e-14 * np.max(np.abs(B.data))


def test_a_constant_field_reproduces_the_per_simplex_references():
    pts, tets, top, _ = cube()
    c0 = 1.75
    cp = np.full(len(pts), c0)
    assert same(N.stiffness(pts, tets, cp, 2), R.assemble(pts, tets, np.full(len(tets), c0))[1])
    assert same(N.stiffness(pts, tets, cp, 1), R.assemble_p1(pts, tets, np.full(len(tets), c0))[1])
    assert same(N.boundary(pts, tets, top, cp, 2), R.assemble_boundary(pts, tets, top, np.full(len(top), c0)))
    # P1 boundary mass of one triangle with constant c: c |(x0-x2) x (x1-x2)| (1 + delta_ab)/24
    rows, cols, vals = [], [], []
    for tri in top:
        X = pts[tri]
        det = np.linalg.norm(np.cross(X[0] - X[2], X[1] - X[2]))
        rows.append(np.repeat(tri, 3)); cols.append(np.tile(tri, 3)); vals.append((c0 * det / 24.0 * (1.0 + np.eye(3))).ravel())
    assert same(N.boundary(pts, tets, top, cp, 1), -1j * R._coo(rows, cols, vals, len(pts)))
