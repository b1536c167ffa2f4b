"""tests/_p2ref.py, the CPU reference that tests/test_gpu_p2.py holds the device P2 assembly against, pinned by itself (no GPU)."""
from fractions import Fraction

import numpy as np

import _p2ref as R

RNG = np.random.default_rng(7)


def _duffy_rule(m=5):
    """quadrature on the reference tetrahedron {l_1 + l_2 + l_3 <= 1}: Gauss-Legendre (m points per direction) on the cube, collapsed;
    with m = 5 it is exact to degree 9 - 3 = 6 >= 4"""
    x, w = np.polynomial.legendre.leggauss(m)
    x, w = (x + 1) / 2, w / 2
    pts, wts = [], []
    for a, wa in zip(x, w):
        for b, wb in zip(x, w):
            for c, wc in zip(x, w):
                l1, l2, l3 = a, b * (1 - a), c * (1 - a) * (1 - b)
                pts.append((l1, l2, l3, 1 - l1 - l2 - l3))
                wts.append(wa * wb * wc * (1 - a) ** 2 * (1 - b))
    return np.array(pts), np.array(wts)


def test_local_mass_matches_quadrature_and_its_row_sums_are_the_source_vector():
    pts, wts = _duffy_rule()
    assert abs(wts.sum() - 1 / 6) < 1e-15
    fs = R.basis(4)
    vals = np.array([[R._value(f, lam) for lam in pts] for f in fs])
    Mq = (vals * wts) @ vals.T
    assert np.max(np.abs(Mq - R.local_mass(4))) < 1e-15
    Me, Se = R.local_mass_exact(4), R.local_source_exact(4)
    assert [sum(row) for row in Me] == Se                      # partition of unity, exactly
    assert Se == [Fraction(-1, 120)] * 4 + [Fraction(1, 30)] * 6 and sum(Se) == Fraction(1, 6)
    assert all(Me[a][b] == Me[b][a] for a in range(10) for b in range(10))
    Mt, St = R.local_mass_exact(3), R.local_source_exact(3)
    assert [sum(row) for row in Mt] == St and St == [Fraction(0)] * 3 + [Fraction(1, 6)] * 3


def _random_tet():
    while True:
        X = RNG.standard_normal((4, 3))
        if abs(np.linalg.det((X[:3] - X[3]).T)) > 0.2:
            return X


def test_local_stiffness_annihilates_constants_and_reproduces_the_dirichlet_energy_of_a_quadratic():
    for c in (1.0, 347.0):
        X = _random_tet()
        M, K = R.local_matrices(X, c)
        assert np.max(np.abs(K @ np.ones(10))) < 1e-12 * np.max(np.abs(K))
        assert np.max(np.abs(K - K.T)) < 1e-13 * np.max(np.abs(K))
        V = abs(np.linalg.det((X[:3] - X[3]).T)) / 6
        assert abs(M.sum() - V) < 1e-14 * V
        # u = x'Ax + b.x + d is in the P2 space: its nodal values at the corners and edge midpoints interpolate it exactly
        A = RNG.standard_normal((3, 3)); A = A + A.T
        b, d = RNG.standard_normal(3), 0.3
        nodes = np.vstack([X] + [(X[i] + X[j])[None] / 2 for i, j in R.local_edges(4)])
        u = np.einsum("ni,ij,nj->n", nodes, A, nodes) + nodes @ b + d
        # int |grad u|^2 with grad u = 2Ax + b and  int x x' = V/20 (sum_i v_i v_i' + (sum_i v_i)(sum_i v_i)'),  int x = V * centroid
        s = X.sum(axis=0)
        Ixx = V / 20 * (X.T @ X + np.outer(s, s))
        energy = 4 * np.trace(A @ A @ Ixx) + 4 * b @ A @ (V * s / 4) + b @ b * V
        assert abs(u @ K @ u + c * c * energy) < 1e-12 * c * c * energy


def test_kuhn_cube_counts_and_global_sums():
    for n in (1, 2, 3):
        pts, tets, top = R.kuhn_cube(n)
        edges, t10, t6 = R.connectivity(len(pts), tets, top)
        assert len(pts) == (n + 1) ** 3 and len(tets) == 6 * n ** 3 and len(top) == 2 * n ** 2
        # axis-parallel edges, face diagonals, body diagonals
        assert len(edges) == 3 * n * (n + 1) ** 2 + 3 * n * n * (n + 1) + n ** 3
        assert t10.shape == (len(tets), 10) and t6.shape == (len(top), 6)
        assert t10[:, 4:].min() == len(pts) and t10[:, 4:].max() == len(pts) + len(edges) - 1
        dets = [np.linalg.det((pts[t[:3]] - pts[t[3]]).T) for t in tets]
        assert abs(np.sum(np.abs(dets)) / 6 - 1) < 1e-14 and min(dets) < 0 < max(dets)
    pts, tets, top = R.kuhn_cube(2)
    M, K = R.assemble(pts, tets)
    one = np.ones(M.shape[0])
    assert abs(one @ (M @ one) - 1) < 1e-14 and np.max(np.abs(K @ one)) < 1e-12 * np.max(np.abs(K.data))
    C = R.assemble_boundary(pts, tets, top)
    assert np.all(C.data.real == 0) and abs((one @ (C @ one)).imag + 1) < 1e-14          # C = -i b, the face has area 1


def test_flame_operator_of_the_reference():
    """Q = S (x) g: its row sums over the flame are volume * g, and sum_b g_b = 0 (the gradients of a partition of unity)"""
    pts, tets, _ = R.kuhn_cube(2)
    flame = [0, 1, 2, 7]
    Q, vol = R.assemble_flame(pts, tets, flame, 40, pts[tets[40]].mean(axis=0) + 0.01, [0.0, 0.0, 1.0], 2.5)
    assert abs(vol - 4 / 48) < 1e-15
    one = np.ones(Q.shape[0])
    assert np.max(np.abs(Q @ one)) < 1e-12 * np.max(np.abs(Q.data))
    col = np.asarray(Q.sum(axis=0)).ravel()
    g = -(2.5 / vol) * (R.basis_gradients_at(pts[tets[40]], pts[tets[40]].mean(axis=0) + 0.01) @ [0.0, 0.0, 1.0])
    _, t10, _ = R.connectivity(len(pts), tets)
    assert np.max(np.abs(col[t10[40]] - vol * g)) < 1e-13 * np.max(np.abs(g)) * vol


def test_p2_converges_faster_than_p1_on_the_unit_cube():
    """smallest non-zero eigenvalue of the Neumann cube (exact: pi^2), 4^3 Kuhn cells: O(h^4) against O(h^2)"""
    pts, tets, _ = R.kuhn_cube(4)
    e1 = abs(R.smallest_nonzero_eigenvalue(*R.assemble_p1(pts, tets)) - np.pi ** 2)
    e2 = abs(R.smallest_nonzero_eigenvalue(*R.assemble(pts, tets)) - np.pi ** 2)
    print(f"|w2_P1 - pi^2| = {e1:.3e}   |w2_P2 - pi^2| = {e2:.3e}")
    assert e2 < e1
