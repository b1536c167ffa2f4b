"""The multigrid preconditioner against a host reference: the coarse-level operators, the transfers, the dense level and the
composition of the V-cycle (include/waehip.h wae_debug_vcycle: ONE application of the solver's own vcycle()), none of which any
other test compares with anything but the library itself.

The hierarchy is RECOVERED from the device once per family: restriction, prolongation and every term of every sparse coarse level
are applied to identity columns through wae_debug_spmv (CSR kernels; products with 0 and 1 are exact, so this reads the stored
matrices bit for bit).  From the recovered matrices:
  1. R_l == P_l^T bitwise, the penalty rows of the family have no aggregate;
  2. every term of every coarse level is the Galerkin product R A P of the level above, entry by entry, to 1e-13 of |R||A||P|
     (tests/_mgref.galerkin, extended precision); the auxiliary term is -1 x the M term;
  3. every fused form of the operator product on every sparse coarse level, and both transfers, against scipy products of the
     recovered matrices (tests/_tilecheck.py);
  4. the dense level alone against numpy.linalg.solve of the Galerkin matrix (measure of test_dense_level: 64 n eps kappa_inf);
  5. the cycle from every level against tests/_mgref.vcycle_ref (the textbook recursion in extended precision);
  6. the refusals of the hook.

Families: A -- annulus "tiny", 1 152 DoF, max_coarse = 16, weights 0.7 / 0.9 / 0.5, sweeps 1 and 2 (two handles); B -- annulus
"small", 8 736 DoF, default options (fine level and level-0 transfers in tile form from 8 columns on); C -- the Bloch unit cell of
test_gpu_bloch.py (728 DoF, 11 terms, complex per-plane coefficients, seam terms out of the shape matrix, max_coarse = 16 for a sparse
coarse level; set up at b = 0, run at b = 5).  Every family has three levels, the last one dense.

Budget of the cycle comparisons (5): the reference is evaluated twice on the host, in clongdouble and in complex128 (scipy
products); their distance e64 -- per column, the larger of max|.| error / max|reference| over the penalty rows and over all other
rows -- is measured at test time, and the device gets 16 x e64, floored at 1e-13 (_tilecheck.TOL).  tests/test_mgref.py shows that
every defect of the composition this is meant to catch moves the reference by more than 10^4 budgets.
"""
import numpy as np
import pytest

import _mgref as M
import _vecref as R
from _hier import MASKS, OPS, RATIOS, SENT, Z_AB, LINE, Hier, family_a, family_c
from _tilecheck import MatrixProducts, assert_close, check_modes
from wae_amd import _lib
from wae_amd.helmholtz.family import annulus_family

pytestmark = pytest.mark.gpu


def drop(H):
    print(f"family {H.name} sweeps={H.nsweeps}: largest device error of the cycle comparisons {RATIOS.get(H.name, 0.0):.2f} units of max(e64, 1e-13 / 16); 16 allowed")
    H.L._drop_device()


@pytest.fixture(scope="module")
def fam_a1():
    H = family_a(1)
    yield H
    drop(H)


@pytest.fixture(scope="module")
def fam_a2():
    H = family_a(2)
    yield H
    drop(H)


@pytest.fixture(scope="module")
def fam_b():
    L, _ = annulus_family("small", tau=2e-4)
    L.solver_ref = 2 * np.pi * 500.0
    H = Hier("B", L, (0.8, 0.9, 0.5), 1, Z_AB, Z_AB + LINE, distinct=16)
    yield H
    drop(H)


@pytest.fixture(scope="module")
def fam_c():
    H = family_c()
    yield H
    drop(H)


FAMS = ["fam_a1", "fam_a2", "fam_b", "fam_c"]


# ----------------------------------------------------------------------------------------------------
# 1, 2: the stored hierarchy
# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fx", FAMS)
def test_transfers_and_galerkin_identity(fx, request):
    H = request.getfixturevalue(fx)
    print(f"family {H.name} sweeps={H.nsweeps}: levels {H.n} (the last one dense), {int(H.pen.sum())} penalty rows, {H.fam.T} terms")
    assert H.nl >= 3, H.n
    assert H.n[0] == H.fam.d and H.n[-1] <= (128 if H.name == "B" else 16)
    for l in range(H.nl - 1):
        Rm, Pm = H.Rm[l], H.Pm[l]
        assert np.all(Rm.data.imag == 0) and np.all(Pm.data.imag == 0)
        assert Rm.shape == (H.n[l + 1], H.n[l]) and Pm.shape == (H.n[l], H.n[l + 1])
        D = (Rm - Pm.T).tocsr()
        assert D.nnz == 0 or np.all(D.data == 0), (l, "R is not the transpose of P, bit for bit")
        assert Rm.nnz == Pm.nnz and np.all(np.diff(Rm.indptr) > 0), (l, "an aggregate without members")
    assert H.pen.any()
    assert np.all(np.diff(H.Pm[0].indptr)[H.pen] == 0), "a penalty row belongs to an aggregate"
    assert np.all(np.diff(H.Pm[0].indptr)[~H.pen] > 0), "a row that is no penalty row has no aggregate"
    iM = [k for k, t in enumerate(H.L.terms) if t.operator == "M"]
    iaux = [k for k, t in enumerate(H.L.terms) if t.operator == "__aux__"]
    S0 = H.terms[0][iaux[0]] + sum(H.terms[0][k] for k in iM)
    assert len(iaux) == 1 and iM and (S0.nnz == 0 or np.max(np.abs(S0.data)) <= 4 * R.EPS * np.max(np.abs(H.terms[0][iaux[0]].data)))
    worst = 0.0
    for l in range(1, H.nl - 1):
        for k in range(H.fam.T):
            G, bound = H.gal[(l, k)]
            A = np.asarray(H.terms[l][k].todense())
            assert not np.any((A != 0) & (bound == 0)), (l, k, "a stored entry where R A P has none")
            q = np.abs(A - G)[bound > 0] / bound[bound > 0]
            worst = max(worst, float(np.max(q)) if q.size else 0.0)
            assert np.all(np.abs(A - G) <= 1e-13 * bound), (l, k, float(np.max(q)))
        S = (H.terms[l][iaux[0]] + sum(H.terms[l][k] for k in iM)).tocsr()
        if len(iM) == 1:                                             # the annulus: -M shares the plane of M, scaled by -1
            assert S.nnz == 0 or np.all(S.data == 0), (l, "the auxiliary term is not -1 x the M term")
        else:                                                        # the unit cell: -M is the sum of the base and seam parts of M, negated
            bsum = H.gal[(l, iaux[0])][1] + sum(H.gal[(l, k)][1] for k in iM)
            assert np.all(np.abs(np.asarray(S.todense())) <= 1e-13 * bsum), (l, "the auxiliary term is not -1 x the sum of the M parts")
    print(f"family {H.name}: Galerkin identity, largest |A - R A P| / |R||A||P| = {worst:.2e}")


# ----------------------------------------------------------------------------------------------------
# 3: fused forms and transfers on the coarse levels
# ----------------------------------------------------------------------------------------------------
def check_transfers(H, l, r, cmask=None, no_tiles=False):
    rng = H.rng
    nf, nc = H.n[l], H.n[l + 1]
    Pr, Rr = H.transfers[l]
    act = np.ones(r, dtype=bool) if cmask is None else np.repeat(cmask, 8)[:r]
    on, off = np.nonzero(act)[0], np.nonzero(~act)[0]
    ct = H.ct1
    X = rng.standard_normal((nf, r)) + 1j * rng.standard_normal((nf, r))
    Y0 = np.full((nc, r), SENT)
    Y = H.fam.debug_spmv(ct, X, mode=0, level=l, which=1, cmask=cmask, Y0=Y0, no_tiles=no_tiles)
    assert_close(Y, Rr @ X, abs(Rr) @ np.abs(X), f"{H.name} restriction {l} r={r}", cols=on)
    assert np.array_equal(Y[:, off], Y0[:, off])
    Xc = rng.standard_normal((nc, r)) + 1j * rng.standard_normal((nc, r))
    Bf = rng.standard_normal((nf, r)) + 1j * rng.standard_normal((nf, r))
    Y = H.fam.debug_spmv(ct, Xc, mode=3, B=Bf, Y0=Bf, level=l, which=2, cmask=cmask, no_tiles=no_tiles)
    assert_close(Y, Bf + Pr @ Xc, np.abs(Bf) + abs(Pr) @ np.abs(Xc), f"{H.name} prolongation {l} r={r}", cols=on)
    assert np.array_equal(Y[:, off], Bf[:, off])


@pytest.mark.parametrize("fx", ["fam_a1", "fam_c"])
def test_fused_forms_on_the_coarse_levels(fx, request):
    H = request.getfixturevalue(fx)
    for l in range(1, H.nl - 1):
        for r in (1, 2, 3, 4, 8, 21):
            X = (H.rng.standard_normal((H.n[l], r)) + 1j * H.rng.standard_normal((H.n[l], r)))
            for op in ("N", "C"):
                tp = MatrixProducts(H.terms[l], X, op)
                for percol in (False, True):
                    check_modes(H.fam, tp, H.ct(percol, r), X, H.rng, f"{H.name} level {l} r={r} op {op} percol={percol}", op=OPS[op], level=l, jac_w=0.7)
                if r == 21:
                    check_modes(H.fam, tp, H.ct(True, r), X, H.rng, f"{H.name} level {l} r=21 op {op} masked", op=OPS[op], level=l, cmask=MASKS[21])
    for l in range(H.nl - 1):
        for r in (1, 2, 3, 4, 8, 21):
            check_transfers(H, l, r)
        check_transfers(H, l, 21, cmask=MASKS[21])


def test_level_one_and_transfers_in_tile_and_csr_form(fam_b):
    """family B: level 1 and the level-0 transfers take the tile kernels from 8 columns on; both storage forms against the reference"""
    H = fam_b
    for r in (8, 64):
        X = H.rng.standard_normal((H.n[1], r)) + 1j * H.rng.standard_normal((H.n[1], r))
        for op in ("N", "C"):
            tp = MatrixProducts(H.terms[1], X, op)
            for no_tiles in (False, True):
                check_modes(H.fam, tp, H.ct(r == 64, r), X, H.rng, f"B level 1 r={r} op {op} no_tiles={no_tiles}", op=OPS[op], level=1, no_tiles=no_tiles)
        for no_tiles in (False, True):
            check_transfers(H, 0, r, no_tiles=no_tiles)
            check_transfers(H, 1, r, no_tiles=no_tiles)
    check_transfers(H, 0, 64, cmask=MASKS[64])


# ----------------------------------------------------------------------------------------------------
# 4: the dense level alone
# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fx", ["fam_a1", "fam_b", "fam_c"])
def test_coarsest_level_alone(fx, request):
    H = request.getfixturevalue(fx)
    Ld = H.nl - 1
    lv, n = H.levels[Ld], H.n[Ld]
    eps = R.EPS
    for op in ("N", "T", "C"):
        for percol in (False, True):
            r = 5
            X = R.rand(H.rng, n, r)
            ct = H.ct(percol, r)
            Y = H.fam.debug_vcycle(ct, X, level=Ld, op=OPS[op], Y0=np.full((n, r), SENT))
            cj = M.Level.coeffs(ct, op, r)
            for j in range(r):
                A64 = np.asarray(lv.matrix(cj[j], op, M.LD), dtype=np.complex128)
                factor = 64 * n * eps * R.cond_inf(A64)
                inv64 = np.linalg.inv(A64)
                ref = np.linalg.solve(A64, X[:, j])
                tol = factor * np.linalg.norm(inv64, np.inf) * np.max(np.abs(X[:, j]))
                err = np.max(np.abs(Y[:, j] - ref))
                assert err <= tol, (H.name, op, percol, j, float(err / tol))


# ----------------------------------------------------------------------------------------------------
# 5: the cycle
# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("light", [False, True], ids=["full", "light"])
@pytest.mark.parametrize("percol", [False, True], ids=["one_system", "per_column"])
@pytest.mark.parametrize("op", ["N", "T", "C"])
@pytest.mark.parametrize("fx", ["fam_a1", "fam_a2"])
def test_cycle_from_every_level(fx, op, percol, light, request):
    """Family A (levels 1 152 / 136 / 8).  Largest device error observed on an MI355X: 3.8 x e64 (16 allowed), 5.9e-15 in absolute terms
    against the floor of 1e-13; e64 itself stayed below 4.5e-15."""
    H = request.getfixturevalue(fx)
    for level in range(H.nl - 2, -1, -1):
        for r in (1, 3, 8, 21, 64):
            for final_out in (False, True):
                H.check_cycle(level, op, percol, light, r, final_out=final_out)
            if r in MASKS:
                H.check_cycle(level, op, percol, light, r, final_out=(r == 64), masked=True)
    for r in (1, 8, 64):
        H.check_cycle(0, op, percol, light, r, fused=True, final_out=(r == 8))
    H.check_cycle(0, op, percol, light, 64, fused=True, masked=True)


@pytest.mark.parametrize("op,percol,light", [("N", False, False), ("N", True, True), ("C", True, False), ("C", False, True)])
@pytest.mark.parametrize("fx", ["fam_b", "fam_c"])
def test_cycle_of_the_tile_and_bloch_families(fx, op, percol, light, request):
    """Families B (levels 8 736 / 1 010 / 46) and C (728 / 94 / 8), from level 0 (C: from its sparse coarse level too).  Largest device
    error observed on an MI355X: B 1.7 x e64 (8.6e-15 absolute, e64 up to 9.3e-15), C 2.2 x e64 (1.4e-15 absolute); 16 x e64 allowed."""
    H = request.getfixturevalue(fx)
    if H.name == "C":
        for r in (3, 21):
            H.check_cycle(1, op, percol, light, r, final_out=(r == 3), masked=(r == 21))
    for r in (8, 64):
        H.check_cycle(0, op, percol, light, r, final_out=(r == 8))
        H.check_cycle(0, op, percol, light, r, fused=True, final_out=(r == 64))
    H.check_cycle(0, op, percol, light, 64, masked=True)
    H.check_cycle(0, op, percol, light, 64, fused=True, masked=True, final_out=True)


# ----------------------------------------------------------------------------------------------------
# 6: refusals
# ----------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable(fam_a1):
    H = fam_a1
    fam, n0, n1 = H.fam, H.n[0], H.n[1]

    def refused(**kw):
        args = dict(coeffs=H.ct1, B=H.B[0][:, :3], level=0)
        args.update(kw)
        with pytest.raises(_lib.WaeError) as e:
            fam.debug_vcycle(args.pop("coeffs"), args.pop("B"), **args)
        assert e.value.code == _lib.WAE_ERR_INVALID, e.value

    L2, _ = annulus_family("tiny", tau=2e-4)
    with pytest.raises(_lib.WaeError) as e:                           # no set-up
        L2.device().debug_vcycle(H.ct1, H.B[0][:, :3])
    assert e.value.code == _lib.WAE_ERR_INVALID
    L2._drop_device()
    refused(level=-1)
    refused(level=H.nl, B=H.B[H.nl - 1][:, :3])
    refused(B=np.zeros((n0, 0), dtype=np.complex128))                # r = 0
    refused(B=np.zeros((n0, 65), dtype=np.complex128))               # r > opts[6]
    refused(coeffs=H.ct64[:2])                                       # ncoef = 2, r = 3
    refused(op=3)
    refused(level=1, B=H.B[1][:, :3], fused=True)                    # flags bit 2 on a coarse level
    with pytest.raises(_lib.WaeError):
        fam.debug_spmv(H.ct1, H.B[H.nl - 1][:, :3], level=H.nl - 1)   # (wae_debug_spmv still refuses the dense level)
    H.check_cycle(0, "N", False, False, 3)
    assert n1 < n0
