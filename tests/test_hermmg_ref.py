"""The host reference of the Hermite p-hierarchy (tests/_hermmgref.py) pinned by properties, on the CPU.

Tolerances.  P_face against the DoF vectors of the quadratics: 1e-13 of the vector's largest entry.  The other figures are sums of at most
~100 products per row with a few roundings each: 100 x 4 x 1.1e-16 = 4.4e-14 of the row's |P| |u|, so 1e-13 holds for them as well.
A seeded defect must miss the property it breaks by more than 1e10 times the intact figure (an exact 0 counted as 1e-17).

The spectral estimate: WAE_WEIGHT_POWER_STEPS = 40 power steps must land in [0.9 lambda, lambda (1 + 1e-10)] on every level of the Hermite
Rijke hierarchy and of the Hermite Kuhn cube, in the caller's numbering and in a shuffled one (the library renumbers its rows)."""
import numpy as np
import pytest
import scipy.sparse as sp

import _hermmgref as G
import _hermref as R

TOL = 1e-13
W340 = 2 * np.pi * 340.0


@pytest.fixture(scope="module")
def prolongators():
    return {name: (G.p_face_ref(*G.mesh(name)), G.p_lin_ref(*G.mesh(name)[:2])) for name in G.SHAPES}


@pytest.mark.parametrize("name", G.SHAPES)
def test_the_prolongators_have_their_properties(prolongators, name):
    pts, tets, tris = G.mesh(name)
    Pf, Pl = prolongators[name]
    N = len(pts)
    assert Pf.shape == (R.connectivity(N, tets, tris)[3], 4 * N) and Pl.shape == (4 * N, N)
    assert np.all(np.diff(Pf.indptr)[4 * N:] == 12) and np.all(np.diff(Pf.indptr)[:4 * N] == 1)
    fig = G.properties(pts, tets, tris, Pf, Pl)
    print(name, {k: f"{v:.2e}" for k, v in fig.items()})
    for k, v in fig.items():
        assert v <= TOL, (k, v)


def test_the_fitted_centroid_weights_are_a_third_and_an_eighteenth():
    """the 9 x 9 fit gives 1/3 on the values and 1/18 on each of the two edge derivatives of a point: 1/18 ((a_q - a_p) + (a_r - a_p)) =
    (x_f - x_p) / 6, the closed form the product writes down"""
    w = G.centroid_weights()
    assert np.allclose(w[:3], 1 / 3, rtol=0, atol=1e-15) and np.allclose(w[3:], 1 / 18, rtol=0, atol=1e-15)


@pytest.mark.parametrize("defect, broken", [("sixth", "quad"), ("unweighted", "volume"), ("signed", "volume")])
def test_a_seeded_defect_breaks_a_property(prolongators, defect, broken):
    """on `two`: tetrahedra of different volume, one of them with det J < 0.  A mean of P1 gradients reproduces linear functions whatever
    its weights, and its rows sum to 0: what tells the volume-weighted mean from the others is the identity
    sum_p W_p (P_lin u)_p = 4 sum_t |det J_t| grad u_t  (`volume`)."""
    pts, tets, tris = G.mesh("two")
    Pf, Pl = prolongators["two"]
    good = G.properties(pts, tets, tris, Pf, Pl)
    if defect == "sixth":
        Pf = G.p_face_ref(pts, tets, tris, defect=defect)
    else:
        Pl = G.p_lin_ref(pts, tets, defect=defect)
    bad = G.properties(pts, tets, tris, Pf, Pl)
    factor = bad[broken] / max(good[broken], 1e-17)
    print(f"{defect}: {broken} {good[broken]:.2e} -> {bad[broken]:.2e}, factor {factor:.1e}")
    assert factor > 1e10
    for k in good:
        if k != broken and not (defect == "signed" and k in ("lin", "grad_rows")):      # (negative weights cancel: those two lose digits, no more)
            assert bad[k] <= TOL, (k, bad[k])


@pytest.fixture(scope="module")
def rijke():
    A = G.rijke_operator(W340)
    pts, tets, tris = G.mesh("rijke")
    Ps = G.hierarchy(A, [G.p_face_ref(pts, tets, tris), G.p_lin_ref(pts, tets)])
    return A, Ps, G.level_operators(A, Ps)


def test_hierarchy_drops_a_column_that_only_penalty_rows_use():
    """4 fine rows, row 3 a penalty row and the only user of coarse column 2: the column leaves level 1, and with it row 2 of the next
    prolongator, whose column 1 nobody uses any more either"""
    A = sp.diags([1.0, 2.0, 1.5, 1e12]).tocsr()
    P0 = sp.csr_matrix(np.array([[1.0, 0, 0], [0.5, 0.5, 0], [0, 1.0, 0], [0, 0, 1.0]]))
    P1 = sp.csr_matrix(np.array([[1.0, 0], [1.0, 0], [0, 1.0]]))
    Q0, Q1 = G.hierarchy(A, [P0, P1])
    assert Q0.shape == (4, 2) and Q1.shape == (2, 1)
    assert np.array_equal(Q0.toarray(), np.array([[1.0, 0], [0.5, 0.5], [0, 1.0], [0, 0]])) and np.array_equal(Q1.toarray(), np.array([[1.0], [1.0]]))
    ops = G.level_operators(A, [Q0, Q1])
    assert [B.shape[0] for B in ops] == [4, 2, 1]


def cube_levels():
    pts, tets, top = R.kuhn_cube(4)
    M, K = R.assemble(pts, tets, top)
    A = sp.csr_matrix(9.0 * M + K)
    Ps = [G.p_face_ref(pts, tets, top), G.p_lin_ref(pts, tets)]
    return G.level_operators(A, Ps)


def test_forty_power_steps_reach_the_top_of_the_spectrum(rijke):
    for what, ops in (("rijke", rijke[2]), ("cube", cube_levels())):
        for l, A in enumerate(ops[:-1]):
            lam = G.lambda_max(A)
            est = G.power_estimate(A)
            shuffled = G.power_estimate(A, perm=np.random.default_rng(7).permutation(A.shape[0]))
            print(f"{what} level {l}: n = {A.shape[0]}, lambda_max(D^-1 Re A) = {lam:.6f}, {G.POWER_STEPS} steps {est:.6f} ({est / lam:.4f}), "
                  f"shuffled {shuffled / lam:.4f}, 0.8 lambda = {0.8 * lam:.3f}, scale {G.scale_of(est):.4f}")
            for e in (est, shuffled):
                assert 0.9 * lam <= e <= lam * (1 + 1e-10)
            assert 0.9 * G.scale_of(est) * lam < 2.0                # the largest scaled weight contracts


def test_the_cycle_needs_the_scaled_weights(rijke):
    """Hermite Rijke family at 340 Hz, one random right-hand side, GMRES(30) to 1e-10 on the preconditioned residual.  With the scaled
    weights: 67 iterations; with 0.8 / 0.9 as they are: 3.5e-4 after 300 (lambda_max = 5.79 and 4.88: 0.8 lambda > 2 on both levels)."""
    A, Ps, ops = rijke
    scales = [G.scale_of(G.power_estimate(B)) for B in ops[:-1]]
    b = G.rhs(A.shape[0], 1)[:, 0]
    _, its, rel = G.gmres_left(A, G.Cycle(ops, Ps, scales).apply, b)
    print(f"scaled weights {scales}: {its} iterations, preconditioned residual {rel:.2e}")
    assert its < 300 and rel <= 1e-10
    _, its1, rel1 = G.gmres_left(A, G.Cycle(ops, Ps, [1.0, 1.0]).apply, b)
    print(f"weights 0.8 / 0.9: {its1} iterations, preconditioned residual {rel1:.2e}")
    assert its1 == 300 and not rel1 <= 1e-10
