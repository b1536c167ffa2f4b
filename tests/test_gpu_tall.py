"""The tall-matrix entries of the C ABI (wae_tall_*, include/waehip.h) one call at a time against numpy, then the eigenpair extraction
built on them (`moments2eigs_native`, `beyn_native`) against known answers and against the host path.  Tolerances are worst-case
rounding bounds of a sum of complex products (eps = 2^-52); an indexing error misses them by many orders."""
import ctypes as C

import numpy as np
import pytest

import wae_amd  # noqa: F401
from wae_amd import _lib
from wae_amd.nlevp import TallMatrix, beyn, beyn_native, moments2eigs_native
from wae_amd.nlevp.beyn import coefficient_table

import _tallcases as T

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
ROWS = [1, 63, 255, 257, 4099]            # one lane, a tail shorter than a wavefront, a tile edge from both sides, many workgroups
LOOP_ROWS = 64 * (768 + 5) + 3           # more 64-row tiles than tall_gram_kernel has workgroups: every workgroup prefetches and
                                         # re-stages a second tile, a few take a third, and the last tile is ragged


def cn(rng, *shape):
    return np.asfortranarray(rng.standard_normal(shape) + 1j * rng.standard_normal(shape))


def gram_ok(G, X, Y):
    ref = X.conj().T @ Y
    bound = 4 * X.shape[0] * EPS * (np.abs(X).T @ np.abs(Y))
    assert G.shape == ref.shape and np.all(np.isfinite(G))
    assert np.all(np.abs(G - ref) <= bound), float(np.max(np.abs(G - ref) / bound))


@pytest.mark.parametrize("na,nb", [(1, 1), (3, 5), (16, 16), (17, 2), (64, 64)])
@pytest.mark.parametrize("rows", ROWS)
def test_gram_parity(rows, na, nb):
    rng = np.random.default_rng(1000 * rows + 64 * na + nb)
    Xa, Xb = cn(rng, rows, na + 3), cn(rng, rows, nb + 2)
    Xa[:, 0] = np.nan                                        # outside the requested ranges: never read
    Xb[:, nb + 1] = np.nan
    A, B = TallMatrix.from_host(Xa), TallMatrix.from_host(Xb)
    G = A.gram(B, 2, na, 1, nb)
    gram_ok(G, Xa[:, 2:2 + na], Xb[:, 1:1 + nb])
    assert np.array_equal(G, A.gram(B, 2, na, 1, nb))        # fixed-order reduction: the same bits from call to call
    A.write(np.ones((rows, 1)), col0=0)
    B.write(np.ones((rows, 1)), col0=nb + 1)
    assert np.array_equal(G, A.gram(B, 2, na, 1, nb))        # what lay outside the ranges changed nothing
    # a == b: the same columns (X^H X, staged once) and two different ranges of one matrix
    w = max(na, nb)
    Xw = cn(rng, rows, w + 3)
    Wm = TallMatrix.from_host(Xw)
    Gs = Wm.gram(Wm, 2, na, 2, na)
    gram_ok(Gs, Xw[:, 2:2 + na], Xw[:, 2:2 + na])
    assert np.array_equal(Gs, Wm.gram(Wm, 2, na, 2, na))
    gram_ok(Wm.gram(Wm, 2, na, 1, nb), Xw[:, 2:2 + na], Xw[:, 1:1 + nb])
    for m in (A, B, Wm):
        m.destroy()


def test_gram_grid_stride_loop():
    """(16, 16) at LOOP_ROWS rows: the loop over tiles inside a workgroup, which the small row counts never enter"""
    rng = np.random.default_rng(77)
    X = cn(rng, LOOP_ROWS, 33)
    A = TallMatrix.from_host(X)
    G = A.gram(A, 1, 16, 1, 16)                              # X^H X, staged once
    gram_ok(G, X[:, 1:17], X[:, 1:17])
    assert np.array_equal(G, A.gram(A, 1, 16, 1, 16))
    G = A.gram(A, 1, 16, 17, 16)                             # two column ranges, both staged
    gram_ok(G, X[:, 1:17], X[:, 17:33])
    assert np.array_equal(G, A.gram(A, 1, 16, 17, 16))
    A.destroy()


ALPHA, BETA = 0.6 - 0.5j, -0.3 + 0.8j      # general complex, |alpha| < 1: the bound below carries no factor |alpha|


def mul_ok(out, S, Cm, D, alpha, beta):
    ld = np.clongdouble
    ref = alpha * (S.astype(ld) @ Cm.astype(ld)) + (beta * D.astype(ld) if beta != 0 else 0)
    bound = 4 * Cm.shape[0] * EPS * (np.abs(S) @ np.abs(Cm)) + (EPS * np.abs(beta * D) if beta != 0 else 0)
    assert np.all(np.isfinite(out))
    assert np.all(np.abs(out - ref) <= bound), float(np.max(np.abs(out - ref) / bound))


@pytest.mark.parametrize("ns,nc", [(1, 1), (5, 3), (16, 8), (64, 64)])
@pytest.mark.parametrize("rows", ROWS)
def test_mul_parity(rows, ns, nc):
    rng = np.random.default_rng(2000 * rows + 64 * ns + nc)
    Cm = cn(rng, ns, nc)
    # (1) source with more rows than the destination, src_row0 > 0 (the P = U[:d] Y case), destination columns inside a wider matrix
    Xs, Xd = cn(rng, rows + 3, ns + 1), cn(rng, rows, nc + 2)
    Sm, Dm = TallMatrix.from_host(Xs), TallMatrix.from_host(Xd)
    Dm.mul(Sm, Cm, dst_col0=1, src_col0=1, src_row0=2, alpha=ALPHA, beta=BETA)
    out = Dm.to_host()
    mul_ok(out[:, 1:1 + nc], Xs[2:2 + rows, 1:1 + ns], Cm, Xd[:, 1:1 + nc], ALPHA, BETA)
    assert np.array_equal(out[:, [0, nc + 1]], Xd[:, [0, nc + 1]])           # the other columns: untouched bit for bit
    # (2) beta = 0: the destination is not read
    Dm.write(np.full((rows, nc), complex(np.nan, np.nan)), col0=1)
    Dm.mul(Sm, Cm, dst_col0=1, src_col0=1, src_row0=2, alpha=ALPHA, beta=0.0)
    out = Dm.to_host()
    mul_ok(out[:, 1:1 + nc], Xs[2:2 + rows, 1:1 + ns], Cm, None, ALPHA, 0.0)
    assert np.array_equal(out[:, [0, nc + 1]], Xd[:, [0, nc + 1]])
    # (3) source and destination: two column ranges of one matrix
    Xo = cn(rng, rows, ns + nc + 1)
    Om = TallMatrix.from_host(Xo)
    Om.mul(Om, Cm, dst_col0=ns + 1, src_col0=1, alpha=ALPHA, beta=BETA)
    out = Om.to_host()
    mul_ok(out[:, ns + 1:], Xo[:, 1:1 + ns], Cm, Xo[:, ns + 1:], ALPHA, BETA)
    assert np.array_equal(out[:, :ns + 1], Xo[:, :ns + 1])
    # overlapping ranges are refused, nothing is written
    with pytest.raises(_lib.WaeError) as e:
        Om.mul(Om, Cm, dst_col0=ns, src_col0=1)
    assert e.value.code == _lib.WAE_ERR_INVALID and "overlap" in str(e.value)
    assert np.array_equal(Om.to_host(), out)
    for m in (Sm, Dm, Om):
        m.destroy()


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("K", [1, 2, 3])
def test_hankel_is_an_exact_gather(K, shift):
    d, l = 257, 3
    A = cn(np.random.default_rng(30 + K), d, l * 2 * K)
    M = TallMatrix.from_host(A)
    B = TallMatrix.create(d * K, l * K).hankel(M, l, K, shift)
    ref = np.vstack([np.hstack([A[:, (i + j + shift) * l:(i + j + shift + 1) * l] for j in range(K)]) for i in range(K)])
    assert np.array_equal(B.to_host(), ref)
    for bad in ((l + 1, K, shift), (l, K + 1, shift), (l, K, 2)):
        with pytest.raises(_lib.WaeError) as e:
            B.hankel(M, *bad)
        assert e.value.code == _lib.WAE_ERR_INVALID
    M.destroy()
    B.destroy()


def test_write_read_round_trip_and_ranges():
    rng = np.random.default_rng(4)
    X = cn(rng, 300, 7)
    M = TallMatrix.create(300, 7)
    assert M.ptr != 0 and np.array_equal(M.to_host(), np.zeros((300, 7)))   # zero-filled
    M.write(X)
    assert np.array_equal(M.to_host(), X)
    blk = cn(rng, 41, 3)
    M.write(blk, row0=17, col0=2)
    X[17:58, 2:5] = blk
    assert np.array_equal(M.to_host(), X)
    assert np.array_equal(M.to_host(row0=250, nrows=50, col0=6, ncols=1), X[250:, 6:])
    assert M.to_host(nrows=0).shape == (0, 7)                               # zero widths: no-ops
    for kw in (dict(row0=260, col0=0), dict(row0=0, col0=5)):
        with pytest.raises(_lib.WaeError) as e:
            M.write(blk, **kw)
        assert e.value.code == _lib.WAE_ERR_INVALID
    with pytest.raises(_lib.WaeError):
        M.to_host(row0=299, nrows=2)
    assert np.array_equal(M.to_host(), X)
    M.destroy()


def test_refusals_leave_a_message():
    L = _lib.lib()
    A, B = TallMatrix.create(100, 70), TallMatrix.create(99, 70)
    G = np.zeros((70, 70), dtype=np.complex128)
    one = np.ones(1, dtype=np.complex128)
    z = _lib.zptr
    calls = [lambda: L.wae_tall_gram(A.handle, 0, 65, A.handle, 0, 1, z(G)),
             lambda: L.wae_tall_gram(A.handle, 0, -1, A.handle, 0, 1, z(G)),
             lambda: L.wae_tall_gram(A.handle, 0, 4, B.handle, 0, 4, z(G)),                          # mismatched rows
             lambda: L.wae_tall_gram(None, 0, 4, A.handle, 0, 4, z(G)),
             lambda: L.wae_tall_gram(A.handle, 0, 4, A.handle, 0, 4, None),
             lambda: L.wae_tall_gram(A.handle, 68, 4, A.handle, 0, 4, z(G)),
             lambda: L.wae_tall_mul(B.handle, 0, A.handle, 0, 0, 65, z(G), 1, z(one), z(one)),
             lambda: L.wae_tall_mul(B.handle, 0, A.handle, 0, 0, 1, z(G), -1, z(one), z(one)),
             lambda: L.wae_tall_mul(A.handle, 0, B.handle, 0, 0, 2, z(G), 2, z(one), z(one)),       # destination taller than the source
             lambda: L.wae_tall_mul(B.handle, 0, A.handle, 2, 0, 2, z(G), 2, z(one), z(one)),       # source rows past the end
             lambda: L.wae_tall_mul(None, 0, A.handle, 0, 0, 2, z(G), 2, z(one), z(one)),
             lambda: L.wae_tall_hankel(A.handle, None, 1, 1, 0),
             lambda: L.wae_tall_info(None, None, None, None),
             lambda: L.wae_tall_create(None, 0, 10, 10),
             lambda: L.wae_tall_create(C.byref(C.c_void_p()), 0, 10, 0),
             lambda: L.wae_tall_write(None, 0, 1, 0, 1, z(G)),
             lambda: L.wae_tall_read(None, 0, 1, 0, 1, z(G))]
    for k, f in enumerate(calls):
        assert f() == _lib.WAE_ERR_INVALID, k
        assert len(L.wae_last_error()) > 10, k
    assert L.wae_tall_gram(A.handle, 0, 0, A.handle, 0, 4, None) == _lib.WAE_OK          # zero widths: no-ops
    assert L.wae_tall_mul(B.handle, 0, A.handle, 0, 0, 0, None, 0, None, None) == _lib.WAE_OK
    assert L.wae_tall_destroy(None) == _lib.WAE_OK
    A.destroy()
    B.destroy()


@pytest.mark.parametrize("l,K", [(5, 2), (8, 1)])
def test_extraction_known_answer(l, K):
    """exactly rank-6 moments (tests/_tallcases.py).  Observed on an MI355X: err_host 1.2e-15, native 0.7e-15 (l = 5, K = 2) and
    1.4e-15 (l = 8, K = 1), against the bound 10 err_host + 1e-13 max|lambda| = 1.3e-13; Sigma7 / Sigma6 7e-15."""
    A, _ = T.rank6_moments(l, K)
    d = A.shape[0]
    M = TallMatrix.from_host(A.reshape(d, -1, order="F"))
    info = {}
    Om, P, Sall = moments2eigs_native(M, (d, l, 2 * K), rel_tol=1e-6, info=info)
    assert info["stages"] == 1 and info["kept"] == 6
    assert np.array_equal(M.to_host(), A.reshape(d, -1, order="F"))         # K = 1 works on column ranges of M: read only
    T.check_rank6(Om, P.to_host(), Sall, l, K, f"device l={l} K={K}")
    # the uploaded form; with the opt-in pool the second run works in parked matrices that hold the first run's leftovers
    TallMatrix.POOL_LIMIT = 1 << 28
    try:
        for _ in range(2):
            Om2, P2, _ = moments2eigs_native(np.array(A), (d, l, 2 * K), rel_tol=1e-6)
            assert np.array_equal(Om, Om2) and np.array_equal(P.to_host(), P2.to_host())
            P2.release()
        assert TallMatrix._pool_bytes > 0
    finally:
        TallMatrix.POOL_LIMIT = 0
        TallMatrix.trim_pool()
    assert TallMatrix._pool_bytes == 0
    for m in (M, P):
        m.destroy()


def test_beyn_native_end_to_end_on_the_rijke_family():
    from oracle import fixtures as F
    from wae_amd.helmholtz.family import helmholtz_family
    Lp = helmholtz_family(F.rijke_terms(), n=0.0)
    Gam = np.array([150 + 5j, 150 - 5j, 1000 - 5j, 1000 + 5j]) * 2 * np.pi
    Lp.solver_ref = 2 * np.pi * 500
    Om, P, S, res = beyn_native(Lp, Gam, l=5, K=1, N=16)
    Om_h, P_h = beyn(Lp, Gam, l=5, K=1, N=16, tol=1e-6 * S[0])              # the same truncation, as an absolute threshold
    print("beyn_native:", Om / (2 * np.pi), "residuals", res)
    assert len(Om) == len(Om_h) and len(Om) >= 1 and P.shape == P_h.shape and len(S) == 5
    for w in Om_h:
        assert np.min(np.abs(Om - w)) <= 1e-8 * abs(w)
    # the residual test read P in HBM: the same numbers from the eigenvectors read back and passed as a host array
    res_h = Lp.ensure_solver().eig_residuals(coefficient_table(Lp, Om), P=P)
    assert np.all(np.abs(res - res_h) <= 1e-12 * np.abs(res_h))
    Lp._drop_device()
    TallMatrix.trim_pool()
