"""GPU tests of the Bloch unit cell with P2 elements: the device numbering (wae_bloch_numbering) and fold (wae_bloch_fold) against
tests/_blochref.py (pinned by tests/test_bloch_p2_ref.py), P1 through the same path against the host blochify, and the P2 cell family
against the P2 ring -- L_ring(w) E_b v = E_b (L_b(w) v) through both families' device SpMV, and one eigenpair of the cell verified on the
ring.  Meshes: the six-point wedge with an axis and the annulus sector at grid (4, 12, 4), DOS 12 (ring: 2304 points, 13 932 DoF)."""
import numpy as np
import pytest
import scipy.sparse as sp

import _blochref as B
from wae_amd import _lib
from wae_amd.helmholtz import annulus
from wae_amd.helmholtz.bloch import (BlochNumbering, bloch_expand_dofs, bloch_family, bloch_numbering, blochify, blochify_device, seam_terms)
from wae_amd.helmholtz.family import helmholtz_family
from wae_amd.nlevp import mslp

pytestmark = pytest.mark.gpu
DOS, GRID = 12, (4, 12, 4)
TAU = 2e-4


@pytest.fixture(scope="module")
def cell():
    """the P2 unit cell (device-assembled terms, device numbering) and the reference numbering of the same mesh"""
    c = annulus.build_unit_cell_p2(grid=GRID, DOS=DOS, tau=TAU)
    ref = B.numbering(len(c["points"]), c["info"]["mesh"]["tets"], c["nsector"])
    return c, ref


@pytest.fixture(scope="module")
def ring(cell):
    r = annulus.build_ring_p2(grid=GRID, DOS=DOS, tau=TAU)
    rc, rs = annulus.ring_cell_map(GRID, DOS, cell[0]["numbering"], r["edges"])
    Lf = helmholtz_family(r["terms"], tau=TAU)
    yield r, Lf, rc, rs
    Lf._drop_device()


@pytest.fixture(scope="module")
def cell_family(cell):
    Lb = bloch_family(cell[0])
    Lb.solver_ref = 2 * np.pi * 400.0
    yield Lb
    Lb._drop_device()


def _check_numbering(nb, ref):
    assert np.array_equal(nb.cell_dof, ref["cell_dof"]) and nb.cell_dof.dtype == np.int32
    assert np.array_equal(nb.image, ref["image"]) and np.array_equal(nb.axis, ref["axis"])
    assert np.array_equal(nb.edges, ref["edges"])
    assert (nb.dim, nb.nedges, nb.nimage_edges, nb.naxis_edges, nb.ndof) == (ref["dim"], ref["nedges"], ref["nimage_edges"], ref["naxis_edges"],
                                                                         len(ref["cell_dof"]))


def test_numbering_equals_reference(cell):
    c, ref = cell
    _check_numbering(bloch_numbering(6, B.WEDGE_TETS, 4, 2), B.numbering(6, B.WEDGE_TETS, 4, 2))
    _check_numbering(c["numbering"], ref)
    assert (ref["nedges"], ref["nimage_edges"], ref["dim"]) == (1209, 113, 1288) and c["dim"] == 1288 and c["d_ext"] == 240 + 1209
    tets, npts = c["info"]["mesh"]["tets"], len(c["points"])
    lin = bloch_numbering(npts, tets, c["nsector"], order="lin")
    _check_numbering(lin, B.numbering(npts, tets, c["nsector"], order="lin"))
    assert lin.dim == c["nsector"] and lin.nedges == 0


def test_invalid_numbering_inputs_return_err_invalid():
    """The issue's first case reads "the wedge without its first tetrahedron"; dropping that tetrahedron removes edge 04 together with 02
    and leaves a periodic mesh (tests/test_bloch_p2_ref.py), so the case is built as the issue describes its effect: the first tetrahedron
    takes r1 in the place of r0 -- edge 02 is gone, image edge 04 stays and has no twin."""
    good = B.numbering(6, B.WEDGE_TETS, 4, 2)
    bad_index = B.WEDGE_TETS.copy()
    bad_index[2, 3] = 6
    for kw, msg in ((dict(tets=B.WEDGE_BROKEN_TETS), "1 image edge"), (dict(nsector=4, naxis=5), "naxis"), (dict(nsector=7, naxis=2), "nsector"),
                    (dict(nsector=3, naxis=1), "image points"), (dict(tets=bad_index), "outside")):
        args = dict(npoints=6, tets=B.WEDGE_TETS, nsector=4, naxis=2)
        args.update(kw)
        with pytest.raises(_lib.WaeError) as e:
            bloch_numbering(**args)
        assert e.value.code == _lib.WAE_ERR_INVALID and msg in str(e.value), (kw, str(e.value))
        _check_numbering(bloch_numbering(6, B.WEDGE_TETS, 4, 2), good)           # a valid call afterwards still works


def _same_pattern(a, b):
    a, b = sp.csr_matrix(a), sp.csr_matrix(b)
    return a.shape == b.shape and np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices)


def _check_parts(dev, ref, tol):
    """patterns identical, values to tol * max|part|"""
    assert len(dev) == len(ref)
    for k, (a, b) in enumerate(zip(dev, ref)):
        assert a.has_sorted_indices or a.nnz == 0
        assert _same_pattern(a, b), k
        if b.nnz:
            err, scale = np.max(np.abs(a.data - b.data)), np.max(np.abs(b.data))
            print(f"part {k}: nnz {b.nnz}  max error {err:.2e}  max|part| {scale:.2e}")
            assert err <= tol * scale, (k, err, scale)


def test_fold_of_device_assembled_p2_operators(cell):
    """tolerance 1e-14 max|part|: the device sums the duplicates of an entry in input order, scipy in its own; a handful of terms each"""
    c, ref = cell
    T, nb = c["terms_ext"], c["numbering"]
    Mp, Kp = blochify_device((T["M"], T["K"]), nb)
    Cp, Qp = blochify_device(T["C"], nb), blochify_device(T["Q"], nb)
    for name, dev in (("M", Mp), ("K", Kp), ("C", Cp), ("Q", Qp)):
        assert len(dev) == 3 and all(P.shape == (1288, 1288) and P.dtype == np.complex128 for P in dev)
        _check_parts(dev, B.fold(T[name], ref), 1e-14)
    assert Qp[0].nnz > 0 and Qp[1].nnz == 0 and Qp[2].nnz == 0                       # empty parts are valid matrices
    assert all(P.nnz > 0 for P in Mp + Kp + Cp)
    assert np.all(Cp[0].data.real == 0) and np.any(Cp[0].data.imag != 0)             # C = -i b: the imaginary stream alone
    # the same bits on every call, and M alone as in the pair
    Mq, Kq = blochify_device((T["M"], T["K"]), nb)
    M1 = blochify_device(T["M"], nb)
    for a, b in zip(Mp + Kp, Mq + Kq):
        assert _same_pattern(a, b) and np.array_equal(a.data.view(np.uint64), b.data.view(np.uint64))
    for a, b in zip(Mp, M1):
        assert np.array_equal(a.data.view(np.uint64), b.data.view(np.uint64))
    for a, b in zip(Qp, blochify_device(T["Q"], nb)):
        assert np.array_equal(a.data.view(np.uint64), b.data.view(np.uint64))


def test_six_part_fold_equals_the_literal_loop():
    lay = B.reference_layout(naxis=3, nbody=11, nxbloch=6, nax_ln=2, nref_ln=7, nbody_ln=13)
    n = lay["n_ext"]
    A = sp.csr_matrix(sp.random(n, n, density=0.25, random_state=3) + 1j * sp.random(n, n, density=0.25, random_state=4))
    flags = lay["image"].astype(np.int32) * _lib.BLOCH_IMAGE + lay["axis"].astype(np.int32) * _lib.BLOCH_AXIS
    nb = BlochNumbering(lay["N_points"], lay["nsector"], lay["naxis"], "quad", lay["cell_dof"], flags, np.zeros((0, 2)), lay["dim"], 7, 2)
    six = blochify_device(A, nb)
    ref = B.loop_parts(A, lay)
    assert len(six) == 6 and all(P.nnz > 0 for P in ref)
    for a, b in zip(six, ref):
        assert _same_pattern(a, b) and abs(a - b).max() <= 1e-15
    three = blochify_device(A, nb, axis=False)
    ref3 = B.loop_parts(A, lay, axis=False)
    assert len(three) == 3 and all(P.nnz == 0 for P in ref3[3:])
    for a, b in zip(three, ref3[:3]):
        assert _same_pattern(a, b) and abs(a - b).max() <= 1e-15
    # a real (M, K) pair: two streams through one sort
    Mr, Kr = sp.csr_matrix(A.real), sp.csr_matrix(A.real)
    Kr.data = Kr.data * 3.0 - 1.0
    pm, pk = blochify_device((Mr, Kr), nb)
    for a, b in zip(pm + pk, B.loop_parts(Mr, lay) + B.loop_parts(Kr, lay)):
        assert _same_pattern(a, b) and abs(a - b).max() <= 1e-15


def test_p1_through_the_device_path_equals_host_blochify():
    c = annulus.build_unit_cell(grid=GRID, DOS=DOS, tau=TAU)
    nb = bloch_numbering(c["d_ext"], c["info"]["mesh"]["tets"], c["nsector"], order="lin")
    for name in ("M", "K", "C", "Q"):
        dev, host = blochify_device(c["terms_ext"][name], nb), blochify(c["terms_ext"][name], c["nsector"])
        assert len(dev) == len(host) == 3
        for a, b in zip(dev, host):
            assert _same_pattern(a, b)
            if b.nnz:
                assert np.max(np.abs(a.data - b.data)) <= 1e-15
    La, Lb = bloch_family(c, numbering=nb), bloch_family(c)
    assert [(t.symbol, t.operator) for t in La.terms] == [(t.symbol, t.operator) for t in Lb.terms] and seam_terms(La) == seam_terms(Lb)


def test_ring_identity_through_both_device_spmvs(cell, ring, cell_family):
    c, _ = cell
    r, Lf, rc, rs = ring
    Lb = cell_family
    assert r["d"] == len(rc) == 2304 + len(r["edges"]) and Lf.terms[0].coeff.shape[0] == r["d"]
    assert [t.symbol for t in Lb.terms] == ["ω^2", "ω^2+", "ω^2-", "", "+", "-", "ω*Y", "ω*Y+", "ω*Y-", "n*exp(-iωτ)", "-λ"]
    assert all(t.coeff.shape == (1288, 1288) for t in Lb.terms)
    z = 2 * np.pi * (420 + 13j)
    rng = np.random.default_rng(7)
    Af = Lf(z)
    for b in (0, 1, 5, 6, 11):
        Lb.params["b"] = b
        v = rng.standard_normal((1288, 2)) + 1j * rng.standard_normal((1288, 2))
        lhs = Af @ bloch_expand_dofs(v, b, DOS, rc, rs)
        rhs = bloch_expand_dofs(Lb(z) @ v, b, DOS, rc, rs)
        err = np.linalg.norm(lhs - rhs) / np.linalg.norm(lhs)
        print(f"b = {b}: relative error {err:.2e}")
        assert err <= 1e-13
        if b == 5:                                                             # the adjoint product
            lhs = Af.H @ bloch_expand_dofs(v, b, DOS, rc, rs)
            rhs = bloch_expand_dofs(Lb(z).H @ v, b, DOS, rc, rs)
            err = np.linalg.norm(lhs - rhs) / np.linalg.norm(lhs)
            print(f"b = {b}, adjoint: relative error {err:.2e}")
            assert err <= 1e-13


def test_one_p2_cell_eigenpair_verifies_on_the_p2_ring(cell, ring, cell_family):
    r, Lf, rc, rs = ring
    L1 = bloch_family(annulus.build_unit_cell(grid=GRID, DOS=DOS, tau=TAU), b=1)
    L1.solver_ref = 2 * np.pi * 400.0
    sol1, _, flag1 = mslp(L1, 2 * np.pi * 400.0, maxiter=10, tol=1e-9)
    L1._drop_device()
    assert flag1 in (0, 1, 2)
    w1 = sol1.params["ω"]
    Lb = cell_family
    Lb.params["b"] = 1
    sol, _, flag = mslp(Lb, w1, maxiter=10, tol=1e-9)
    w = sol.params["ω"]
    print(f"P1 cell: {w1 / (2 * np.pi):.4f} Hz   P2 cell: {w / (2 * np.pi):.4f} Hz   flag {flag}")
    assert flag in (0, 1, 2) and abs(w - w1) <= 0.1 * abs(w1)
    assert Lb.device().last_info["n_unconverged"] == 0
    Vx = bloch_expand_dofs(sol.v, 1, DOS, rc, rs)
    res = Lf.device().spmv(np.array([Lf.coefficients(w)]), np.asfortranarray(Vx[:, None]))[:, 0]
    T = r["terms"]
    dg = w * w * T["M"].diagonal() + T["K"].diagonal() + w * 1e15 * T["C"].diagonal()
    print(f"ring residual {np.linalg.norm(res / dg) / np.linalg.norm(Vx):.2e}")
    assert np.linalg.norm(res / dg) <= 1e-6 * np.linalg.norm(Vx)
