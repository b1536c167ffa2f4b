"""Pins tests/_blochref.py, the CPU reference of the Bloch unit cell with point and edge DoFs (no GPU): the numbering rule on the wedge
with an axis, the fold by cell_dof against the literal loop of src/Bloch.jl:4-112 on a layout with the reference's contiguity, and the
identity that ties cell and ring together, L_ring(w) E_b v = E_b (L_b(w) v), with the P2 operators of tests/_p2ref.py."""
import numpy as np
import pytest
import scipy.sparse as sp

import _blochref as B
import _p2ref as R
import wae_amd  # noqa: F401
from wae_amd.helmholtz import annulus

DOS, GRID = 12, (4, 12, 4)


def test_wedge_numbering():
    nb = B.numbering(B.WEDGE["npoints"], B.WEDGE_TETS, B.WEDGE["nsector"], B.WEDGE["naxis"])
    assert [tuple(e) for e in nb["edges"].tolist()] == [(0, 1), (0, 2), (0, 4), (1, 2), (1, 3), (1, 4), (1, 5), (2, 3), (2, 4), (3, 4), (3, 5),
                                                        (4, 5)]
    assert nb["twins"] == {(0, 4): (0, 2), (1, 4): (1, 2), (1, 5): (1, 3), (4, 5): (2, 3)}
    assert nb["nedges"] == 12 and nb["nimage_edges"] == 4 and nb["naxis_edges"] == 1 and nb["dim"] == 12
    assert nb["axis"].tolist() == [True, True] + [False] * 4 + [True] + [False] * 11
    image_edges = np.nonzero(nb["image"][6:])[0].tolist()
    assert image_edges == [2, 5, 6, 11] and image_edges != list(range(8, 12))          # not the tail of the sorted list
    # points: 4, 5 fold onto 2, 3; the 8 cell edges are numbered 4..11 in list order, image edges take their twin's number
    assert nb["cell_dof"].tolist() == [0, 1, 2, 3, 2, 3, 4, 5, 5, 6, 7, 6, 7, 8, 9, 10, 11, 8]
    assert B.numbering(6, B.WEDGE_TETS, 4, 2, order="lin")["cell_dof"].tolist() == [0, 1, 2, 3, 2, 3]
    with pytest.raises(ValueError, match="without a twin"):
        B.numbering(6, B.WEDGE_BROKEN_TETS, 4, 2)                                       # edge 02 is gone: 04 has no twin
    assert B.numbering(6, B.WEDGE_TETS[1:], 4, 2)["nimage_edges"] == 3                  # dropping a tetrahedron drops 02 AND 04: still periodic


@pytest.mark.parametrize("naxis", [0, 3])
def test_fold_by_cell_dof_equals_the_literal_loop(naxis):
    lay = B.reference_layout(naxis=naxis, nbody=11, nxbloch=6, nax_ln=2 if naxis else 0, nref_ln=7, nbody_ln=13)
    n = lay["n_ext"]
    A = sp.random(n, n, density=0.25, random_state=3) + 1j * sp.random(n, n, density=0.25, random_state=4)
    for axis in (True, False):
        mine, ref = B.fold(A, lay, axis=axis), B.loop_parts(A, lay, axis=axis)
        assert len(mine) == len(ref) == (6 if naxis else 3)
        for a, b in zip(mine, ref):
            assert a.shape == b.shape == (lay["dim"],) * 2
            assert abs(a - b).max() <= 1e-15 if (a.nnz or b.nnz) else True
            assert np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices)
        if naxis:
            assert all(p.nnz > 0 for p in mine[:3]) and all((p.nnz > 0) == axis for p in mine[3:])
        assert sum(p.nnz for p in mine) > 0


def _p2_terms(pts, mesh):
    M, K = R.assemble(pts, mesh["tets"], mesh["c_tet"])
    C = R.assemble_boundary(pts, mesh["tets"], mesh["outlet_tris"], mesh["outlet_c"])
    Q = sum(R.assemble_flame(pts, mesh["tets"], f["flame_tets"], f["ref_tet"], f["x_ref"], f["n_ref"], f["nglobal_scaled"])[0]
            for f in mesh["flames"])
    return M, K, C, sp.csr_matrix(Q)


def test_ring_identity_with_p2_reference_operators():
    cell = annulus.build_unit_cell(grid=GRID, DOS=DOS, tau=2e-4)
    ring = annulus.build(grid=(DOS * GRID[0], GRID[1], GRID[2]), n_sector=DOS, ref_offset="polar", tau=2e-4)
    cm, rm = cell["info"]["mesh"], ring["info"]["mesh"]
    nb = B.numbering(len(cell["points"]), cm["tets"], cell["nsector"])
    assert (len(cell["points"]), cell["nsector"], nb["nedges"], nb["nimage_edges"], nb["dim"]) == (240, 192, 1209, 113, 1288)
    w, Y, tau = 2 * np.pi * (420 + 13j), 1e15, 2e-4
    coef = (w * w, 1.0, w * Y, np.exp(-1j * w * tau))
    Lr = sum(c * T for c, T in zip(coef, _p2_terms(ring["points"], rm)))
    folded = [B.fold(T, nb) for T in _p2_terms(cell["points"], cm)]
    assert folded[3][1].nnz == 0 and folded[3][2].nnz == 0                                # the flame does not reach the seam
    rc, rs = B.annulus_ring_map(GRID, DOS, nb, R.edge_list(rm["tets"]))
    assert Lr.shape[0] == len(rc) and np.array_equal(np.bincount(rc, minlength=nb["dim"]), np.full(nb["dim"], DOS))
    rng = np.random.default_rng(11)
    for b in (0, 1, 5, 6, 11):
        Lb = sum(c * B.bloch_matrix(P, b, DOS) for c, P in zip(coef, folded))
        v = rng.standard_normal(nb["dim"]) + 1j * rng.standard_normal(nb["dim"])
        lhs = Lr @ B.expand(v, b, DOS, rc, rs)
        rhs = B.expand(Lb @ v, b, DOS, rc, rs)
        err = np.linalg.norm(lhs - rhs) / np.linalg.norm(lhs)
        print(f"b = {b}: relative error {err:.2e}")
        assert err <= 1e-13
