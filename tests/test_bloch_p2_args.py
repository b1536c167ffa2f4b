"""CPU checks of the Bloch numbering / device fold wrappers (helmholtz/bloch.py, helmholtz/annulus.py): bad arguments are rejected in
Python, before any library call (no GPU here: a library call would raise WaeError, not ValueError), the host helpers that need no device,
and the family built without a numbering is term for term what it was."""
import numpy as np
import pytest
import scipy.sparse as sp

import _blochref as B
import wae_amd  # noqa: F401
from wae_amd.helmholtz import annulus
from wae_amd.helmholtz.bloch import (SUFFIXES, BlochNumbering, bloch_expand, bloch_expand_dofs, bloch_family, bloch_numbering, bloch_terms,
                                     blochify, blochify_device, seam_terms)

DOS, GRID = 12, (4, 12, 4)


def _numbering(nb, order="quad"):
    """the product's numbering object filled from the CPU reference"""
    flags = nb["image"].astype(np.int32) + 2 * nb["axis"].astype(np.int32)
    return BlochNumbering(nb["npoints"], nb["nsector"], nb["naxis"], order, nb["cell_dof"], flags, nb["edges"], nb["dim"], nb["nimage_edges"],
                          nb["naxis_edges"])


def test_wrappers_reject_bad_arguments_before_the_library():
    nb = _numbering(B.numbering(6, B.WEDGE_TETS, 4, 2))
    assert nb.ndof == 18 and nb.nedges == 12 and nb.image.sum() == 6 and nb.axis_cell_dofs().tolist() == [0, 1, 4]
    with pytest.raises(ValueError, match="18 DoFs"):
        blochify_device(sp.identity(17, format="csr"), nb)                       # a numbering of the wrong length
    with pytest.raises(ValueError, match="square"):
        blochify_device(sp.csr_matrix(np.ones((18, 17))), nb)
    with pytest.raises(ValueError, match="one sparsity pattern"):
        blochify_device((sp.identity(18, format="csr"), sp.csr_matrix(np.ones((18, 18)))), nb)
    for order in ("herm", "cubic", 2):
        with pytest.raises(ValueError, match="order"):
            bloch_numbering(6, B.WEDGE_TETS, 4, 2, order=order)
    with pytest.raises(ValueError, match="nsector, naxis"):
        bloch_terms({"M": sp.identity(18), "K": sp.identity(18), "C": sp.identity(18)}, 5, DOS, 2, numbering=nb)


def test_bloch_expand_dofs_generalises_bloch_expand():
    rng = np.random.default_rng(2)
    v = rng.standard_normal((7, 3)) + 1j * rng.standard_normal((7, 3))
    naxis, nx, dos = 2, 5, 4
    cell = np.concatenate([np.arange(naxis)] + [naxis + np.arange(nx)] * dos)
    sector = np.concatenate([np.zeros(naxis, dtype=int)] + [np.full(nx, s) for s in range(dos)])
    for b in (0, 1, 3):
        assert np.allclose(bloch_expand_dofs(v, b, dos, cell, sector), bloch_expand(v, b, dos, nxsector=nx, naxis=naxis), rtol=0, atol=1e-15)
        assert np.allclose(bloch_expand_dofs(v[:, 0], b, dos, cell, sector), bloch_expand(v[:, 0], b, dos, nxsector=nx, naxis=naxis), rtol=0, atol=1e-15)


def test_ring_cell_map_equals_the_reference_map():
    import _p2ref as R
    cell = annulus.build_unit_cell(grid=GRID, DOS=DOS)
    tets_ring = annulus._mesh(DOS * GRID[0], GRID[1], GRID[2])[1]
    ref = B.numbering(len(cell["points"]), cell["info"]["mesh"]["tets"], cell["nsector"])
    edges = R.edge_list(tets_ring)
    rc, rs = annulus.ring_cell_map(GRID, DOS, _numbering(ref), edges)
    qc, qs = B.annulus_ring_map(GRID, DOS, ref, edges)
    assert np.array_equal(rc, qc) and np.array_equal(rs, qs)
    with pytest.raises(ValueError, match="unit cell of this grid"):
        annulus.ring_cell_map((5, 12, 4), DOS, _numbering(ref), edges)


def _same_terms(L, expected):
    assert [(t.symbol, t.operator) for t in L.terms] == [(s, o) for s, o, _ in expected]
    for t, (_, _, A) in zip(L.terms, expected):
        assert t.coeff.shape == A.shape and abs(t.coeff - A).max() == 0


def test_family_without_numbering_is_unchanged():
    cell = annulus.build_unit_cell(grid=GRID, DOS=DOS, tau=2e-4)
    T, ns = cell["terms_ext"], cell["nsector"]
    expected = []
    for name, txt in (("M", "ω^2"), ("K", ""), ("C", "ω*Y"), ("Q", "n*exp(-iωτ)")):
        expected += [(txt + suf, name, P) for P, suf in zip(blochify(T[name], ns), SUFFIXES) if P.nnz]
    expected.append(("-λ", "__aux__", -sum(blochify(T["M"], ns, axis=False))))
    L = bloch_family(cell, b=3)
    _same_terms(L, expected)
    assert L.params["b"] == 3 and seam_terms(L) == [k for k, (s, o, _) in enumerate(expected) if s.endswith(("+", "-")) and o != "__aux__"]
    assert len(seam_terms(L)) == 6                                                 # M, K, C cross the seam; Q does not
    # with an axis: six parts per operator, then D on the axis DoFs, then the auxiliary term
    n_ext, nsector, naxis = 60, 48, 5
    A = {k: sp.random(n_ext, n_ext, density=0.2, random_state=s) + sp.identity(n_ext) for s, k in enumerate("MKC")}
    syn = {"terms_ext": A, "nsector": nsector, "DOS": 8, "naxis": naxis, "params": {"Y": 1.0, "n": 1.0, "τ": 0.0}}
    expected = []
    for name, txt in (("M", "ω^2"), ("K", ""), ("C", "ω*Y")):
        expected += [(txt + suf, name, P) for P, suf in zip(blochify(A[name], nsector, naxis), SUFFIXES) if P.nnz]
    Mf = sum(blochify(A["M"], nsector, naxis, axis=False)[:3])
    D = sp.csr_matrix((1.0 / -Mf.diagonal()[:naxis], (np.arange(naxis),) * 2), shape=(nsector, nsector), dtype=complex)
    expected += [("(1-δ(b))", "D", D), ("-λ", "__aux__", -Mf)]
    _same_terms(bloch_family(syn, flame=False), expected)
