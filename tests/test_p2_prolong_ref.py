"""CPU tests of the P2 prolongation between octosplit levels: the host form of ``RefinedMesh.prolongator(l, order="quad")`` (the combinatorial
rule the device follows) against the geometric reference tests/_p2proref.py, which shares nothing with it, on the four small meshes of
tests/_octoref.py, two levels each; and the host form of ``p2_embedding``.

Tolerances: values 1e-14 (the reference solves a 3 x 3 system per row: 3.0e-15 measured); quadratic reproduction 1e-13 of the largest sample
(3.3e-16 measured); the Galerkin identity 1e-13 of the largest entry, the project's assembly tolerance (2.2e-15 measured); the embedding 1e-14."""
import numpy as np
import pytest
import scipy.sparse as sp

import _octoref as O
import _p2proref as R
import _p2ref as P2
from wae_amd.helmholtz.assemble import p2_embedding_host
from wae_amd.helmholtz.refine import RefinedMesh

SMALL = ["one", "two", "sheared", "cube"]
WEIGHTS = {1.0, 0.375, -0.125, 0.75, 0.5, 0.25}
KINDS = {"sheared": [(196, 360, 48), (1208, 2592, 384)]}


def host_mesh(name):
    H = R.hierarchy(name)
    return RefinedMesh(None, 0, [l.points for l in H], [l.tets for l in H], [l.tris for l in H], [l.parents for l in H],
                       [l.tet_labels for l in H], [l.tri_labels for l in H])


@pytest.mark.parametrize("frm", [0, 1])
@pytest.mark.parametrize("name", SMALL)
def test_host_prolongator_equals_the_geometric_reference(name, frm):
    Rm = host_mesh(name)
    P, G = Rm.prolongator(frm, order="quad"), R.prolongator(name, frm)
    assert sp.issparse(P) and P.format == "csr" and P.shape == G.shape == (Rm.ndof(frm + 1, "quad"), Rm.ndof(frm, "quad"))
    assert P.indptr.dtype == np.int32 and P.indices.dtype == np.int32 and P.data.dtype == np.float64
    assert np.array_equal(P.indptr, G.indptr) and np.array_equal(P.indices, G.indices), "pattern"
    err = float(np.max(np.abs(P.data - G.data)))
    print(f"{name} step {frm}: {P.shape[0]} x {P.shape[1]}, {P.nnz} entries, max |rule - geometry| = {err:.2e}")
    assert err <= 1e-14
    for i in range(P.shape[0]):
        assert np.all(np.diff(P.indices[P.indptr[i]:P.indptr[i + 1]]) > 0), (i, "columns not ascending")
    assert set(np.unique(P.data).tolist()) <= WEIGHTS
    assert np.array_equal(np.asarray(P.sum(axis=1)).ravel(), np.ones(P.shape[0]))       # (dyadic weights: the sums are exact)
    n_f = len(Rm.points[frm + 1])
    length = np.diff(P.indptr)
    assert np.all(length[:n_f] == 1) and set(np.unique(length[n_f:]).tolist()) <= {3, 5, 10}
    if name in KINDS:
        assert tuple(int(np.sum(length[n_f:] == k)) for k in (3, 5, 10)) == KINDS[name][frm]


def test_sizes_of_the_sheared_cube():
    Rm = host_mesh("sheared")
    assert [Rm.ndof(l, "quad") for l in range(3)] == [125, 729, 4913] and [Rm.ndof(l) for l in range(3)] == [27, 125, 729]
    assert Rm.ndof(order="quad") == 4913 and Rm.ndof(-1, "lin") == 729


@pytest.mark.parametrize("name", SMALL)
def test_quadratic_reproduction(name):
    Rm, H = host_mesh(name), R.hierarchy(name)
    for frm in (0, 1):
        xc, xf = R.locations(H[frm]), R.locations(H[frm + 1])
        want = R.quadratic(xf, seed=frm)
        got = Rm.prolongator(frm, order="quad") @ R.quadratic(xc, seed=frm)
        err = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
        print(f"{name} step {frm}: quadratic reproduced to {err:.2e} of the largest sample")
        assert err <= 1e-13


@pytest.mark.parametrize("name", SMALL)
def test_galerkin_identity_with_the_p2_assembly(name):
    Rm, H = host_mesh(name), R.hierarchy(name)
    nt0 = len(H[0].tets)
    c0 = 1.0 + 0.1 * np.arange(nt0) / nt0
    for frm in (0, 1):
        P = Rm.prolongator(frm, order="quad")
        Mc, Kc = P2.assemble(H[frm].points, H[frm].tets, O.carry_field(H, c0, "tet", frm))
        Mf, Kf = P2.assemble(H[frm + 1].points, H[frm + 1].tets, O.carry_field(H, c0, "tet", frm + 1))
        for what, Af, Ac in (("M", Mf, Mc), ("K", Kf, Kc)):
            err = float(np.max(np.abs((P.T @ Af @ P - Ac).toarray())) / np.max(np.abs(Ac.toarray())))
            print(f"{name} step {frm}, {what}: max|P^T A P - assembled| = {err:.2e} of the largest entry")
            assert err <= 1e-13, (name, frm, what)


@pytest.mark.parametrize("name", SMALL)
def test_embedding_host_form_samples_an_affine_function(name):
    H = R.hierarchy(name)
    for lvl in (0, 1):
        edges, _, _ = P2.connectivity(len(H[lvl].points), H[lvl].tets)
        E = p2_embedding_host(len(H[lvl].points), edges)
        n, ne = len(H[lvl].points), len(edges)
        assert E.shape == (n + ne, n) and E.nnz == n + 2 * ne and E.indptr.dtype == np.int32 and E.indices.dtype == np.int32
        assert all(np.all(np.diff(E.indices[E.indptr[i]:E.indptr[i + 1]]) > 0) for i in range(n + ne))
        want = R.affine(R.locations(H[lvl]))
        err = float(np.max(np.abs(E @ R.affine(H[lvl].points) - want)) / np.max(np.abs(want)))
        assert err <= 1e-14, (name, lvl, err)


def test_p_first_list_without_a_device():
    Rm, H = host_mesh("two"), R.hierarchy("two")
    Ps = Rm.prolongators(order="quad", p_first=True)
    assert [P.shape for P in Ps] == [(Rm.ndof(2, "quad"), Rm.ndof(2)), (Rm.ndof(2), Rm.ndof(1)), (Rm.ndof(1), Rm.ndof(0))]
    edges, _, _ = P2.connectivity(len(H[2].points), H[2].tets)
    assert (Ps[0] != p2_embedding_host(len(H[2].points), edges)).nnz == 0
    for P, l in zip(Ps[1:], (1, 0)):
        assert (P != Rm.prolongator(l)).nnz == 0
    assert [P.shape for P in Rm.prolongators(order="quad", p_first=True, coarsest=2)] == [(Rm.ndof(2, "quad"), Rm.ndof(2))]
    Hs = Rm.prolongators(order="quad")
    assert [P.shape for P in Hs] == [(Rm.ndof(2, "quad"), Rm.ndof(1, "quad")), (Rm.ndof(1, "quad"), Rm.ndof(0, "quad"))]
    assert (Hs[1] != Rm.prolongator(0, order="quad")).nnz == 0
    assert [P.shape for P in Rm.prolongators(1, order="quad")] == [(Rm.ndof(1, "quad"), Rm.ndof(0, "quad"))]


def test_argument_refusals():
    Rm = host_mesh("one")
    before = Rm.prolongator(0, order="quad")
    lin = Rm.prolongator(0)
    cases = {
        "an unknown order (prolongator)": lambda: Rm.prolongator(0, order="cubic"),
        "an unknown order (prolongators)": lambda: Rm.prolongators(order="herm"),
        "an unknown order (ndof)": lambda: Rm.ndof(0, "P2"),
        "an unknown order (prolong)": lambda: Rm.prolong(np.ones(4), 0, 1, order=2),
        "p_first without quad": lambda: Rm.prolongators(p_first=True),
        "p_first that is no flag": lambda: Rm.prolongators(order="quad", p_first=1),
        "the last level": lambda: Rm.prolongator(2, order="quad"),
        "a level out of range": lambda: Rm.prolongator(3, order="quad"),
        "a level that is no integer": lambda: Rm.prolongator(0.0, order="quad"),
        "ndof of a level out of range": lambda: Rm.ndof(3, "quad"),
        "coarsest = to_level without p_first": lambda: Rm.prolongators(1, coarsest=1, order="quad"),
        "coarsest above to_level": lambda: Rm.prolongators(1, coarsest=2, order="quad", p_first=True),
        "from >= to": lambda: Rm.prolong(np.ones(Rm.ndof(1, "quad")), 1, 1, order="quad"),
        "X of the P1 size": lambda: Rm.prolong(np.ones(Rm.ndof(0)), 0, 1, order="quad"),
        "X with no columns": lambda: Rm.prolong(np.ones((Rm.ndof(0, "quad"), 0)), 0, 1, order="quad"),
        "X of strings": lambda: Rm.prolong(np.array(["a"] * Rm.ndof(0, "quad")), 0, 1, order="quad"),
        "prolong without a device handle": lambda: Rm.prolong(np.ones(Rm.ndof(0, "quad")), 0, 1, order="quad"),
    }
    for what, f in cases.items():
        with pytest.raises(ValueError) as e:
            f()
        assert str(e.value), what
        print(f"{what}: {e.value}")
    after = Rm.prolongator(0, order="quad")
    assert (after != before).nnz == 0 and np.array_equal(after.data, before.data)
    assert (Rm.prolongator(0) != lin).nnz == 0
