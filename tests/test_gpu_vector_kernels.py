"""Every streaming and reduction kernel under the lock-step GMRES, the snapshot basis, the Beyn accumulation, the batched
perturbation and the dense coarse level, ONE launch at a time (wae_debug_vec) against the extended-precision references of
tests/_vecref.py.  GMRES corrects itself: a dropped row, a skipped basis vector or a wrong pivot only costs iterations in the whole
solves the rest of the suite runs, so these are the tests that pin each kernel to its defining formula.  The recurrence kernels
between them (gmres_init, gmres_step, gmres_rescale, gmres_pair_coef, gmres_solve_y: Hessenberg columns, rotations, residual
estimates, chunk masks) are pinned the same way by tests/test_gpu_gmres_recurrence.py (wae_debug_gmres, tests/_gmresref.py).

Tolerances are rounding bounds of float64 arithmetic, not measured numbers:
  reductions   |gpu - ref| <= 2 (n + 4) eps sum_rows |v||w|                       per output entry
  updates      |gpu - ref| <= 4 (m + 2) eps (|base| + sum_i |c_i||v_i|)           per element, m summed terms
  fused norms  the reduction bound on the squared norm of the vector written, and against the reference vector's norm with the
               elements' own update bound carried into the sum (check_fused_norms); 1/||.||^2 under the same relative bounds
  dense level  ||A Ainv - I||_max <= 64 n eps kappa_inf(A);  ||Y - A^-1 X||_max within the same factor times ||A^-1||_inf ||X||_max
Inputs rho e^{i phi}, rho in [0.5, 2], seeded; every output buffer holds the sentinel 3+7j before the call.
Shapes: R = 256 // nb row groups per workgroup; n in {1, R-1, R, R+1, 37 R + 5} for every nb, and one size past the launcher's grid cap."""
import numpy as np
import pytest

import _vecref as R
from wae_amd import _lib

pytestmark = pytest.mark.gpu

EPS = R.EPS
NBS = (1, 2, 3, 8, 24, 63, 64, 65, 128, 200, 256)
INVALID = _lib.WAE_ERR_INVALID


def row_sizes(nb, per_group=None):
    r = per_group or 256 // nb
    return sorted({1, r - 1, r, r + 1, 37 * r + 5} - {0})


def capped(nb, G, per_group=None):
    r = per_group or 256 // nb
    return 2 * G * r + r + 1


def call(op, sizes, bufs, **kw):
    return _lib.debug_vec(op, sizes, bufs, **kw)


def chunk_mask(nb, dead_chunks):
    m = np.ones((nb + 7) // 8, dtype=bool)
    m[list(dead_chunks)] = False
    return m


class Cols:
    """which columns a case checks: `live` (cmask byte non-zero) and not the column poisoned with NaN"""

    def __init__(self, nb, cmask=None, nan_col=None):
        self.nb, self.cmask, self.nan_col = nb, cmask, nan_col
        self.live = np.ones(nb, dtype=bool) if cmask is None else np.asarray(cmask, dtype=bool)[np.arange(nb) >> 3]
        self.ok = self.live.copy()
        if nan_col is not None:
            self.ok[nan_col] = False

    def poison(self, *arrays):
        if self.nan_col is not None:
            for a in arrays:
                a[..., self.nan_col] = np.nan
        return arrays


def assert_close(got, ref, tol, cols, what):
    """|got - ref| <= tol on the last-axis columns `cols` (boolean)"""
    err = np.abs(got[..., cols].astype(R.LD) - ref[..., cols])
    t = np.asarray(tol)[..., cols]
    assert np.all(np.isfinite(got[..., cols])), what
    bad = err > t
    assert not np.any(bad), (what, float(np.max(err / t)))


def assert_untouched(got, cols, what):
    assert np.all(got[..., cols] == R.SENTINEL), what


def assert_zero(got, cols, what):
    assert np.all(got[..., cols] == 0), what


# ---------------------------------------------------------------------------------------------------------------------------------
# reductions
# ---------------------------------------------------------------------------------------------------------------------------------
def check_dots(rng, n, nb, nv, cmask=None, nan_col=None, scaled=False, stride_pad=0, one_vector=False):
    C = Cols(nb, cmask, nan_col)
    stride = 0 if one_vector else n * nb + stride_pad
    Vs = R.rand(rng, 1 if one_vector else nv, n * nb + stride_pad)
    V = Vs[:, :n * nb].reshape(-1, n, nb)
    W = R.rand(rng, n, nb)
    C.poison(V, W)
    scale = R.rand(rng, nv, nb) if scaled else None        # (only the real part is the scale: the imaginary part must be ignored)
    out = R.sentinel(nv, nb)
    call(_lib.VEC_DOTS, [n, nb, nv, stride], [Vs, W, out, scale], cmask=cmask)
    ref, mag = R.dots(V, W)
    if one_vector:
        ref, mag = np.repeat(ref, nv, axis=0), np.repeat(mag, nv, axis=0)
    if scaled:
        ref, mag = ref * scale.real, mag * np.abs(scale.real)
    what = f"dots n={n} nb={nb} nv={nv} scaled={scaled}"
    assert_close(out, ref, 2 * (n + 4) * EPS * mag, C.ok, what)
    assert_zero(out, ~C.live, what + ": masked columns are written as 0")


def check_norms(rng, n, nb, cmask=None, nan_col=None):
    C = Cols(nb, cmask, nan_col)
    X, = C.poison(R.rand(rng, n, nb))
    out = R.sentinel(nb)
    call(_lib.VEC_NORMS, [n, nb], [X, out], cmask=cmask)
    sq = R.sqnorms(X)
    what = f"norms n={n} nb={nb}"
    assert np.all(out.imag[C.live] == 0), what
    assert_close(out.real.astype(np.longdouble) ** 2, sq, 2 * (n + 4) * EPS * sq, C.ok, what)
    assert_zero(out, ~C.live, what)


def check_dots_multi(rng, n, nb, nv, nw, nan_col=None):
    C = Cols(nb, None, nan_col)
    sv, sw = n * nb + 3, n * nb + 16                       # distinct strides
    Vs, Ws = R.rand(rng, nv, sv), R.rand(rng, nw, sw)
    V, W = Vs[:, :n * nb].reshape(nv, n, nb), Ws[:, :n * nb].reshape(nw, n, nb)
    C.poison(V, W)
    out = R.sentinel(nv, nw, nb)
    call(_lib.VEC_DOTS_MULTI, [n, nb, nv, nw, sv, sw], [Vs, Ws, out])
    ref, mag = R.dots_multi(V, W)
    assert_close(out, ref, 2 * (n + 4) * EPS * mag, C.ok, f"dots_multi n={n} nb={nb} nv={nv} nw={nw}")


def check_dots2(rng, n, nb, nv, cmask=None, nan_col=None):
    C = Cols(nb, cmask, nan_col)
    V, W1, W2, scale = R.rand(rng, nv, n, nb), R.rand(rng, n, nb), R.rand(rng, n, nb), R.rand(rng, nv, nb)
    C.poison(V, W1, W2)
    o1, o2, gram = R.sentinel(nv, nb), R.sentinel(nv, nb), R.sentinel(3, nb)
    call(_lib.VEC_DOTS2, [n, nb, nv, n * nb], [V, W1, W2, o1, o2, gram, scale], cmask=cmask)
    what = f"dots2 n={n} nb={nb} nv={nv}"
    s = np.abs(scale.real)
    for o, W in ((o1, W1), (o2, W2)):
        ref, mag = R.dots(V, W)
        assert_close(o, ref * scale.real, 2 * (n + 4) * EPS * mag * s, C.ok, what)
        assert_zero(o, ~C.live, what)
    gref, gmag = R.dots(np.stack([W1, W1, W2]), W1)        # w1^H w1, w1^H w2, w2^H w2
    g12, m12 = R.dots(W1[None], W2)
    g22, m22 = R.dots(W2[None], W2)
    gref[1], gmag[1], gref[2], gmag[2] = g12[0], m12[0], g22[0], m22[0]
    assert_close(gram, gref, 2 * (n + 4) * EPS * gmag, C.ok, what + " gram")
    assert_zero(gram, ~C.live, what)


@pytest.mark.parametrize("nb", NBS)
def test_dots(nb):
    rng = np.random.default_rng(100 + nb)
    for n in row_sizes(nb):
        for nv in (1, 7, 8, 9, 16, 17, 32, 33, 40):
            check_dots(rng, n, nb, nv, scaled=(nv % 2 == 0), stride_pad=5 if nv == 9 else 0)
        check_norms(rng, n, nb)
    # Several rows per thread, and past the grid caps: 1024 workgroups with nv <= 16, 768 beyond.  The grid is a quarter of the row
    # steps, so only the doubled sizes (4 G R rows and more) reach a cap.  With 17 vectors such a size has more than 2^23 entries,
    # whatever nb: there the 17 vectors are one and the same (stride 0, as launch_norms passes it), and every output is its norm^2.
    if nb in (64, 200):
        check_dots(rng, capped(nb, 1024), nb, 8)
        check_dots(rng, capped(nb, 768), nb, 17)
        check_dots(rng, 2 * capped(nb, 1024), nb, 4)
        check_dots(rng, 2 * capped(nb, 768), nb, 17, one_vector=True)
        check_norms(rng, 2 * capped(nb, 1024), nb)
    if nb == 1:
        check_dots(rng, capped(nb, 1024), nb, 4)
        check_dots(rng, 2 * capped(nb, 1024), nb, 3, scaled=True)
        check_norms(rng, 2 * capped(nb, 1024), nb)


@pytest.mark.parametrize("nb", NBS)
def test_dots2(nb):
    rng = np.random.default_rng(200 + nb)
    for n in row_sizes(nb):
        for nv in (1, 16, 17, 33):
            check_dots2(rng, n, nb, nv)
    if nb in (64, 200):
        check_dots2(rng, capped(nb, 768), nb, 17)
        check_dots2(rng, 2 * capped(nb, 768), nb, 2)
    if nb == 1:
        check_dots2(rng, 2 * capped(nb, 768), nb, 3)


@pytest.mark.parametrize("nb", NBS)
def test_dots_multi(nb):
    rng = np.random.default_rng(300 + nb)
    for n in row_sizes(nb):
        for nv in (1, 8, 9, 17):
            for nw in (1, 3, 4):
                check_dots_multi(rng, n, nb, nv, nw)
    if nb in (64, 200):
        check_dots_multi(rng, capped(nb, 768), nb, 9, 3)
    if nb == 1:
        check_dots_multi(rng, capped(nb, 768), nb, 2, 2)


# ---------------------------------------------------------------------------------------------------------------------------------
# updates
# ---------------------------------------------------------------------------------------------------------------------------------
def upd_tol(mag, m):
    return 4 * (m + 2) * EPS * mag


def check_axpy(rng, op, n, nb, nv, cmask=None, nan_col=None):
    """axpy_neg: W -= V h | lincomb: Y = V y | lincomb_add: X += V y"""
    C = Cols(nb, cmask, nan_col)
    V, c = R.rand(rng, nv, n, nb), R.rand(rng, nv, nb)
    W = R.sentinel(n, nb) if op == _lib.VEC_LINCOMB else R.rand(rng, n, nb)
    C.poison(V, c, W)
    W0 = W.copy()
    call(op, [n, nb, nv, n * nb], [V, c, W], cmask=cmask)
    ref, mag = R.update(None if op == _lib.VEC_LINCOMB else W0, c, V, -1.0 if op == _lib.VEC_AXPY_NEG else 1.0)
    what = f"op {op} n={n} nb={nb} nv={nv}"
    assert_close(W, ref, upd_tol(mag, nv), C.ok, what)
    assert np.all(W[:, ~C.live] == W0[:, ~C.live]), what + ": masked columns keep their values"


def check_axpy_neg_norm(rng, n, nb, nv, with_base, with_inv, cmask=None, nan_col=None):
    C = Cols(nb, cmask, nan_col)
    V, h = R.rand(rng, nv, n, nb), R.rand(rng, nv, nb)
    base = R.rand(rng, n, nb) if with_base else None
    W = R.sentinel(n, nb) if with_base else R.rand(rng, n, nb)
    C.poison(V, h, W if base is None else base)
    W0 = W.copy()
    norms, inv = R.sentinel(nb), (R.sentinel(nb) if with_inv else None)
    call(_lib.VEC_AXPY_NEG_NORM, [n, nb, nv, n * nb], [V, h, W, norms, base, inv], cmask=cmask)
    ref, mag = R.update(W0 if base is None else base, h, V, -1.0)
    what = f"axpy_neg_norm n={n} nb={nb} nv={nv} base={with_base} inv={with_inv}"
    assert_close(W, ref, upd_tol(mag, nv), C.ok, what)
    assert np.all(W[:, ~C.live] == W0[:, ~C.live]), what
    check_fused_norms(norms, inv, W, ref, upd_tol(mag, nv), n, C, what)


def check_fused_norms(norms, inv, W, ref, delta, n, C, what):
    """norms[..., b] and inv[..., b] = 1/||.||^2 of the vector(s) the kernel wrote, W (..., n, nb), whose reference is `ref` within `delta`.
    Two comparisons, both on the squared norm:
      with the extended-precision norm of W itself, under the reduction bound 2 (n + 4) eps ||W||^2: this is the sum the kernel forms;
      with the reference norm of the reference vector, under that bound PLUS what the rounding of the elements themselves moves the
      sum by, sum_rows 2 |ref| delta + delta^2.  The reduction bound alone is no rounding bound for this second comparison: with one
      row the norm is the element, whose relative error is that of an update of m terms, and a float64 evaluation of the defining
      formula on the CPU misses 2 (n + 4) eps by factors of 1.0 to 3.5 at n = 1 (nv = 7 ... 40).  A lost row moves the sum by one part
      in n, 1e10 times either tolerance."""
    rel = 2 * (n + 4) * EPS
    sq_w = (np.abs(W.astype(R.LD)) ** 2).sum(axis=-2)
    sq = (np.abs(ref) ** 2).sum(axis=-2)
    tol = rel * sq + (2 * np.abs(ref) * delta + delta * delta).sum(axis=-2)
    assert np.all(norms.imag[..., C.live] == 0), what
    got = norms.real.astype(np.longdouble) ** 2
    assert_close(got, sq_w, rel * sq_w, C.ok, what + " norms (of the vector written)")
    assert_close(got, sq, tol, C.ok, what + " norms (of the reference vector)")
    assert_zero(norms, ~C.live, what)
    if inv is not None:
        assert np.all(inv.imag[..., C.live] == 0), what
        got = inv.real.astype(np.longdouble)
        assert_close(got, 1 / sq_w, rel / sq_w, C.ok, what + " 1/norm^2 (of the vector written)")
        assert_close(got, 1 / sq, tol / (sq * (sq - tol)), C.ok, what + " 1/norm^2 (of the reference vector)")
        assert_zero(inv, ~C.live, what)


AXPY_NVS = (0, 1, 7, 8, 9, 40)


@pytest.mark.parametrize("nb", NBS)
@pytest.mark.parametrize("op", [_lib.VEC_AXPY_NEG, _lib.VEC_LINCOMB, _lib.VEC_LINCOMB_ADD])
def test_axpy_lincomb(op, nb):
    rng = np.random.default_rng(400 + 7 * nb + op)
    for n in row_sizes(nb):
        for nv in AXPY_NVS:
            check_axpy(rng, op, n, nb, nv)
    if nb == 256:                                           # across the chunk of AX_MAXC / nb coefficients
        for nv in (16, 17):
            check_axpy(rng, op, 3, nb, nv)
    if nb == 64:
        for nv in (64, 65):
            check_axpy(rng, op, 9, nb, nv)
    if nb in (64, 200):
        check_axpy(rng, op, capped(nb, 2048), nb, 3)
    if nb == 1:
        check_axpy(rng, op, capped(nb, 2048), nb, 4)


@pytest.mark.parametrize("nb", NBS)
def test_axpy_neg_norm(nb):
    rng = np.random.default_rng(500 + nb)
    k = 0
    for n in row_sizes(nb):
        for nv in AXPY_NVS[1:]:
            k += 1
            check_axpy_neg_norm(rng, n, nb, nv, with_base=bool(k & 1), with_inv=bool(k & 2) and nv <= 4096 // nb)    # (beyond: the fallback)
        check_axpy_neg_norm(rng, n, nb, 0, with_base=bool(n & 1), with_inv=False)        # nv = 0: the two-kernel fallback
    if nb == 256:
        check_axpy_neg_norm(rng, 3, nb, 16, True, True)
        check_axpy_neg_norm(rng, 3, nb, 17, True, False)    # nv > 4096 / nb: fallback
    if nb == 64:
        check_axpy_neg_norm(rng, 9, nb, 64, False, True)
        check_axpy_neg_norm(rng, 9, nb, 65, False, False)
    if nb in (64, 200):
        check_axpy_neg_norm(rng, capped(nb, 1024), nb, 3, True, True)
    if nb == 1:
        check_axpy_neg_norm(rng, capped(nb, 1024), nb, 4, False, True)


def test_axpy_neg_norm_fallback_refuses_inverse_norms():
    rng = np.random.default_rng(5)
    for nb, nv in ((8, 0), (64, 65), (256, 17)):
        n = 5
        V, h, W = R.rand(rng, nv, n, nb), R.rand(rng, nv, nb), R.rand(rng, n, nb)
        code, _ = call(_lib.VEC_AXPY_NEG_NORM, [n, nb, nv, n * nb], [V, h, W, R.sentinel(nb), None, R.sentinel(nb)], raise_on_error=False)
        assert code == INVALID, (nb, nv)


def check_axpy_neg_multi(rng, n, nb, nv, cnt, nan_col=None):
    C = Cols(nb, None, nan_col)
    ws = n * nb + 7
    V, h, Ws = R.rand(rng, nv, n, nb), R.rand(rng, nv, cnt, nb), R.rand(rng, cnt, ws)
    W = Ws[:, :n * nb].reshape(cnt, n, nb)
    C.poison(V, h, W)
    W0, pad0 = W.copy(), Ws[:, n * nb:].copy()
    call(_lib.VEC_AXPY_NEG_MULTI, [n, nb, nv, n * nb, cnt, ws], [V, h, Ws])
    for j in range(cnt):
        ref, mag = R.update(W0[j], h[:, j], V, -1.0)
        assert_close(W[j], ref, upd_tol(mag, nv), C.ok, f"axpy_neg_multi n={n} nb={nb} nv={nv} cnt={cnt} j={j}")
    assert np.all(Ws[:, n * nb:] == pad0)


@pytest.mark.parametrize("nb", NBS)
def test_axpy_neg_multi(nb):
    rng = np.random.default_rng(600 + nb)
    for n in row_sizes(nb):
        for cnt in (1, 2, 3, 4):
            for nv in (1, 9):
                if nv * cnt * nb * 16 <= 60 * 1024:
                    check_axpy_neg_multi(rng, n, nb, nv, cnt)
    if nb in (64, 200):
        check_axpy_neg_multi(rng, capped(nb, 2048), nb, 2, 2)
    if nb == 1:
        check_axpy_neg_multi(rng, capped(nb, 2048), nb, 2, 2)
    # the coefficients of one launch are limited to 60 KB of LDS
    nv = 60 * 1024 // (16 * 4 * nb) + 1
    V, h, W = R.rand(rng, nv, 2, nb), R.rand(rng, nv, 4, nb), R.rand(rng, 4, 2, nb)
    code, _ = call(_lib.VEC_AXPY_NEG_MULTI, [2, nb, nv, 2 * nb, 4, 2 * nb], [V, h, W], raise_on_error=False)
    assert code == INVALID


def check_axpy2(rng, n, nb, nv, cmask=None, nan_col=None):
    """v1 = w1 - V c1,  v2 = w2 - alpha w1 - V c2m, with their norms and 1/norm^2"""
    C = Cols(nb, cmask, nan_col)
    V, c1, c2m, al = R.rand(rng, nv, n, nb), R.rand(rng, nv, nb), R.rand(rng, nv, nb), R.rand(rng, nb)
    W1, W2 = R.rand(rng, n, nb), R.rand(rng, n, nb)
    C.poison(V, c1, c2m, al, W1, W2)
    W10, W20 = W1.copy(), W2.copy()
    norms, inv = R.sentinel(2, nb), R.sentinel(2, nb)
    call(_lib.VEC_AXPY2, [n, nb, nv, n * nb], [V, c1, c2m, al, W1, W2, norms, inv], cmask=cmask)
    what = f"axpy2 n={n} nb={nb} nv={nv}"
    r1, m1 = R.update(W10, c1, V, -1.0)
    r2, m2 = R.update(W20, np.concatenate([al[None], c2m]), np.concatenate([W10[None], V]), -1.0)
    assert_close(W1, r1, upd_tol(m1, nv), C.ok, what + " v1")
    assert_close(W2, r2, upd_tol(m2, nv + 1), C.ok, what + " v2")
    assert np.all(W1[:, ~C.live] == W10[:, ~C.live]) and np.all(W2[:, ~C.live] == W20[:, ~C.live]), what
    check_fused_norms(norms, inv, np.stack([W1, W2]), np.stack([r1, r2]), np.stack([upd_tol(m1, nv), upd_tol(m2, nv + 1)]), n, C, what)


@pytest.mark.parametrize("nb", NBS)
def test_axpy2(nb):
    rng = np.random.default_rng(700 + nb)
    for n in row_sizes(nb, 256 // nb) + [512 // nb + 1]:
        for nv in (1, 7, 8, 9, 40):
            if 2 * nv * nb * 16 <= 150 * 1024:              # (what fits LDS)
                check_axpy2(rng, n, nb, nv)
    if nb == 64:
        check_axpy2(rng, 37, nb, 20)                        # 40 KB of coefficients: the last size of the 256-thread variant
        check_axpy2(rng, 37, nb, 21)                        # the 512-thread variant
        check_axpy2(rng, 9, nb, 75)                         # 150 KB: the last size that fits
        V, c, al, W = R.rand(rng, 76, 9, nb), R.rand(rng, 76, nb), R.rand(rng, nb), R.rand(rng, 9, nb)
        code, _ = call(_lib.VEC_AXPY2, [9, nb, 76, 9 * nb], [V, c, c.copy(), al, W, W.copy(), R.sentinel(2, nb), R.sentinel(2, nb)],
                       raise_on_error=False)
        assert code == INVALID                              # (the launcher refuses before its launch; a refused call copies nothing back)
    if nb in (24, 200):                                     # thread counts that nb does not divide, both variants
        check_axpy2(rng, 1000 // nb + 3, nb, 20 * 64 // nb)
        check_axpy2(rng, 1000 // nb + 3, nb, 20 * 64 // nb + 6)
    if nb in (64, 200):
        check_axpy2(rng, capped(nb, 1024), nb, 3)
    if nb == 200:                                           # the 512-thread variant past its cap of 512 workgroups
        check_axpy2(rng, capped(nb, 512, 512 // nb), nb, 7)
    if nb == 1:
        check_axpy2(rng, capped(nb, 1024), nb, 4)


def check_lincomb_rep(rng, n, nb, l, nv, nan_col=None):
    C = Cols(nb, None, nan_col)
    Q, y, X = R.rand(rng, nv, n, l), R.rand(rng, nv, nb), R.sentinel(n, nb)
    if nan_col is not None:                                 # a basis column feeds every system's column b % l
        y[:, nan_col] = np.nan
        Q[:, :, nan_col % l] = np.nan
        C.ok &= (np.arange(nb) % l) != nan_col % l
    call(_lib.VEC_LINCOMB_REP, [n, nb, nv, n * l, l], [Q, y, X])
    ref, mag = R.lincomb_rep(Q, y, nb, l)
    assert_close(X, ref, upd_tol(mag, nv), C.ok, f"lincomb_rep n={n} nb={nb} l={l} nv={nv}")


@pytest.mark.parametrize("l,nb", [(8, 64), (4, 4), (5, 15), (3, 12), (8, 128), (1, 7)])
def test_lincomb_rep(l, nb):
    """the first three take the kernel for at most 8 systems (one thread per row pair and probe column), the others the general one"""
    rng = np.random.default_rng(800 + nb)
    rep8 = l >= 4 and nb // l <= 8
    per = 2 * (256 // l) if rep8 else 256 // nb
    for n in sorted(set(row_sizes(nb, per) + [1, 2, 3, per + 2, 74 * (per // 2 or 1) + 3])):
        for nv in (1, 3, 4, 5, 40):
            check_lincomb_rep(rng, n, nb, l, nv)
    check_lincomb_rep(rng, 7, nb, l, 4096 // nb + 1)        # the accumulating second launch ((nb = 64, nv = 65) among them)
    if (l, nb) == (4, 4):                                   # past the grid cap of 4096 workgroups, 128 rows each
        check_lincomb_rep(rng, 4096 * 128 + 128 + 1, nb, l, 1)
    if (l, nb) == (3, 12):                                  # ... of 2048 workgroups
        check_lincomb_rep(rng, capped(nb, 2048), nb, l, 2)


def scale_inv_ref(X, alpha):
    """X[:, b] / alpha[b].real, zero where that is not positive"""
    a = alpha.real
    return X.astype(R.LD) / np.where(a > 1e-300, a, np.inf).astype(np.longdouble)[None, :]


def test_small_column_ops():
    rng = np.random.default_rng(9)
    for nb in NBS:
        for n in (1, 256 // nb + 1, 37 * (256 // nb) + 5):
            X, alpha, Y = R.rand(rng, n, nb), R.rand(rng, nb), R.sentinel(n, nb)
            alpha[0] = 0                                    # a tiny norm: the column is written as zero
            call(_lib.VEC_SCALE_INV, [n, nb], [X, alpha, Y])
            ref = scale_inv_ref(X, alpha)
            assert_close(Y, ref, 2 * EPS * np.abs(ref) + 0.0, np.ones(nb, dtype=bool), f"scale_inv n={n} nb={nb}")
            assert np.all(Y[:, 0] == 0)
            keep = (rng.uniform(size=nb) < 0.6).astype(np.complex128) + 5j     # (only the real part counts)
            X0 = X.copy()
            call(_lib.VEC_MASK_COLS, [n, nb], [X, keep])
            assert np.all(X[:, keep.real != 0] == X0[:, keep.real != 0]) and np.all(X[:, keep.real == 0] == 0)
            for off, l in {(0, 1), (nb - 1, 1), (0, nb), (nb // 3, nb - nb // 3 - nb // 4)}:
                out = R.sentinel(n, l)
                call(_lib.VEC_EXTRACT_COLS, [n, nb, off, l], [X0, out])
                assert np.all(out == X0[:, off:off + l]), (n, nb, off, l)
    n, nb = 4096 * 256 // 64 * 2 + 5, 64                     # past the grid cap of the three (4096 workgroups)
    X, alpha, Y = R.rand(rng, n, nb), R.rand(rng, nb), R.sentinel(n, nb)
    call(_lib.VEC_SCALE_INV, [n, nb], [X, alpha, Y])
    ref = scale_inv_ref(X, alpha)
    assert_close(Y, ref, 2 * EPS * np.abs(ref), np.ones(nb, dtype=bool), "scale_inv past the grid cap")
    out = R.sentinel(n, 5)
    call(_lib.VEC_EXTRACT_COLS, [n, nb, 7, 5], [X, out])
    assert np.all(out == X[:, 7:12])


# ---------------------------------------------------------------------------------------------------------------------------------
# Beyn accumulation, batched perturbation
# ---------------------------------------------------------------------------------------------------------------------------------
def check_beyn(rng, d, nb, l, nsys, npow, wide, permute):
    lA, c0 = (l + 5, 2) if wide else (l, 0)
    X, w = R.rand(rng, d, nb), R.rand(rng, nsys)
    z = (rng.uniform(0.8, 1.25, nsys) * np.exp(1j * rng.uniform(0, 2 * np.pi, nsys))).astype(np.complex128)
    A = R.rand(rng, npow, lA, d)                            # the moments accumulate
    A0 = A.copy()
    perm = rng.permutation(d) if permute else None
    call(_lib.VEC_BEYN_ACCUM, [d, nb, l, nsys, npow, lA if wide else 0, c0], [X, w, z, A], perm=perm)
    add, mag = R.beyn_accum(X, w, z, npow, l)
    if permute:                                             # internal row i is the caller's row perm[i]
        inv = np.argsort(perm)
        add, mag = add[:, :, inv], mag[:, :, inv]
    own = np.zeros(lA, dtype=bool)
    own[c0:c0 + l] = True
    what = f"beyn_accum d={d} nb={nb} l={l} nsys={nsys} npow={npow} wide={wide} perm={permute}"
    ref = A0[:, own].astype(R.LD) + add
    # terms |w_s||z_s|^p |x|, each the product of p + 2 factors: m = nsys terms of up to npow + 1 roundings each
    err = np.abs(A[:, own].astype(R.LD) - ref)
    tol = 4 * (nsys + 2) * EPS * (np.abs(A0[:, own]) + mag)
    assert np.all(err <= tol), (what, float(np.max(err / tol)))
    assert np.all(A[:, ~own] == A0[:, ~own]), what + ": the other columns keep their values bit for bit"


@pytest.mark.parametrize("nb,l,nsys", [(64, 8, 8), (64, 8, 5), (256, 16, 16), (3, 3, 1)])
def test_beyn_accum(nb, l, nsys):
    rng = np.random.default_rng(1000 + nb + nsys)
    tr = min(32, 2048 // (nb + 1))                          # rows per LDS tile
    k = 0
    for npow in (1, 2, 8, 9, 12):
        for d in (1, 31, 33, 5 * tr + 1):
            k += 1
            check_beyn(rng, d, nb, l, nsys, npow, wide=bool(k & 1), permute=bool(k & 2))
    check_beyn(rng, 5 * tr + 1, nb, l, nsys, 12, True, True)
    check_beyn(rng, 33, nb, l, nsys, 9, False, False)
    if nb == 3:                                             # past the grid cap of 4096 tiles
        check_beyn(rng, 2 * 4096 * tr + tr + 1, nb, l, nsys, 2, False, True)


def check_pt_gemm(rng, d, nb, k, T, nan_col=None, stride_pad=0):
    C = Cols(nb, None, nan_col)
    Vs, G, U = R.rand(rng, k, d * nb + stride_pad), R.rand(rng, k, T, nb), R.sentinel(d, T, nb)
    V = Vs[:, :d * nb].reshape(k, d, nb)
    C.poison(V, G)
    call(_lib.VEC_PT_GEMM_BATCH, [d, nb, k, d * nb + stride_pad, T], [Vs, G, U])
    ref, mag = R.pt_gemm(V, G)
    assert_close(U, ref, upd_tol(mag, k), C.ok, f"pt_gemm_batch d={d} nb={nb} k={k} T={T}")


@pytest.mark.parametrize("nb", [1, 3, 8, 64])
def test_pt_gemm_batch(nb):
    rng = np.random.default_rng(1100 + nb)
    r = 256 // nb
    for T in (1, 4, 5, 8, 9, 16, 17):
        for d, k in ((1, 3), (r + 1, 4), (37 * r + 5, 7), (r - 1 or 1, 1)):
            check_pt_gemm(rng, d, nb, k, T)
    if nb == 8:                                             # 3072 weights per launch: k = 24 fits at T = 16, k = 25 takes a second launch
        check_pt_gemm(rng, 45, nb, 24, 16)
        check_pt_gemm(rng, 45, nb, 25, 16)
        check_pt_gemm(rng, 45, nb, 25, 17)
    if nb == 64:
        check_pt_gemm(rng, 9, nb, 7, 16)                    # 1024 weights per vector: three vectors per launch
        check_pt_gemm(rng, capped(nb, 2048), nb, 3, 2)
    if nb == 1:                                             # one column: the shape of the single-pair calls wae_perturb / wae_perturb_slots
        check_pt_gemm(rng, capped(nb, 2048), nb, 2, 2)
        check_pt_gemm(rng, capped(nb, 2048), nb, 2, 5)
        check_pt_gemm(rng, 257, nb, 192, 16)                # 3072 weights per launch: k = 192 fits at T = 16, k = 193 takes a second launch
        check_pt_gemm(rng, 257, nb, 193, 16)
        check_pt_gemm(rng, 257, nb, 193, 17)
        for d in (1, 255, 257, 9477):                       # a series whose vectors lie further apart than their length
            for k in (1, 31):
                for T in (1, 5):
                    check_pt_gemm(rng, d, nb, k, T, stride_pad=3)


def check_pt_axpby(rng, d, nb, nan_col=None, dead=()):
    C = Cols(nb, None, nan_col)
    coef, x, y, out = R.rand(rng, 2, nb), R.rand(rng, d, nb), R.rand(rng, d, nb), R.sentinel(d, nb)
    C.poison(coef, x, y)
    for b in dead:                                          # both coefficients zero: written as exact zero whatever x and y hold
        coef[:, b] = 0
        x[:, b] = y[:, b] = np.nan
    call(_lib.VEC_PT_AXPBY_COLS, [d, nb], [coef, x, y, out])
    ref, mag = R.axpby_cols(coef, x, y)
    assert_close(out, ref, upd_tol(mag, 2), C.ok, f"pt_axpby_cols d={d} nb={nb}")
    assert np.all(out[:, list(dead)] == 0)


def check_pt_project(rng, d, nb, nd, nan_col=None):
    C = Cols(nb, None, nan_col)
    vk, v0, dts = R.rand(rng, d, nb), R.rand(rng, d, nb), R.rand(rng, nd, nb)
    C.poison(vk, v0, dts)
    vk0 = vk.copy()
    call(_lib.VEC_PT_PROJECT, [d, nb, nd], [vk, v0, dts])
    ref, mag = R.pt_project(vk0, v0, dts)
    assert_close(vk, ref, upd_tol(mag, nd + 1), C.ok, f"pt_project d={d} nb={nb} nd={nd}")


@pytest.mark.parametrize("nb", NBS)
def test_pt_axpby_cols_and_project(nb):
    rng = np.random.default_rng(1300 + nb)
    for d in row_sizes(nb):
        check_pt_axpby(rng, d, nb, dead=(nb // 2,))
        for nd in (1, 2, 31):
            check_pt_project(rng, d, nb, nd)
    if nb in (1, 64, 200):
        check_pt_axpby(rng, capped(nb, 4096), nb, dead=(0,))
        check_pt_project(rng, capped(nb, 4096), nb, 2)


# ---------------------------------------------------------------------------------------------------------------------------------
# dense coarse level
# ---------------------------------------------------------------------------------------------------------------------------------
def dense_planes(rng, targets, nplanes, op):
    """planes and coefficients with sum_q pc[s][q] op(plane_q) = targets[s]: the least-norm planes for a random full-rank pc"""
    nsys = len(targets)
    pc = R.rand(rng, nsys, nplanes)
    if nsys == nplanes == 1:
        planes = targets / pc[0, 0]
    else:
        planes = np.einsum("qs,sij->qij", np.linalg.pinv(pc), targets)
    if op != 0:
        planes = planes.transpose(0, 2, 1)
    if op == 2:                                             # conj(plane)^T with the coefficients arriving conjugated, as the solver passes them
        planes = planes.conj()
    return np.ascontiguousarray(planes), pc


def check_dense(rng, n, nsys, nplanes, op, targets, l=2, per_system=False, cmask=None, nan_col=None):
    planes, pc = dense_planes(rng, targets, nplanes, op)
    nb = nsys * l if per_system else max(l, 8 if cmask is not None else 1)
    C = Cols(nb, cmask, nan_col)
    cps = l if per_system else 1 << 30
    X, = C.poison(R.rand(rng, n, nb))
    Ainv, Y = R.sentinel(nsys, n, n), R.sentinel(n, nb)
    code, status = call(_lib.VEC_DENSE, [n, nb, nsys, nplanes, op, cps], [planes, pc, Ainv, X, Y], cmask=cmask)
    what = f"dense n={n} nsys={nsys} nplanes={nplanes} op={op} per_system={per_system}"
    assert code == 0 and status == 0, what
    A = R.dense_assemble(planes, pc, op)                    # what the device was asked to invert
    for s in range(nsys):
        A64 = np.asarray(A[s], dtype=np.complex128)
        assert 0.99e2 < np.linalg.cond(A64) < 1.01e4, (what, np.linalg.cond(A64))
        kappa = R.cond_inf(A64)
        factor = 64 * n * EPS * kappa
        resid = np.max(np.abs(A64 @ Ainv[s] - np.eye(n)))   # (its own rounding, n eps kappa, is 1/64 of the bound)
        assert resid <= factor, (what, s, float(resid / factor))
        cols = np.nonzero(C.ok & ((np.arange(nb) // cps) == s))[0]
        if len(cols):
            inv64 = np.linalg.inv(A64)
            tol = factor * np.linalg.norm(inv64, np.inf) * np.max(np.abs(X[:, cols]))
            err = np.max(np.abs(Y[:, cols] - inv64 @ X[:, cols]))
            assert err <= tol, (what, s, float(err / tol))
    assert_untouched(Y, ~C.live, what)


def zero_corner(A):
    """A G with a unitary G acting on the first two columns such that the corner entry vanishes: the singular values stay"""
    a, b = A[0, 0], A[0, 1]
    r = np.sqrt(abs(a) ** 2 + abs(b) ** 2)
    c0, c1 = A[:, 0].copy(), A[:, 1].copy()
    A[:, 0], A[:, 1] = (b * c0 - a * c1) / r, (np.conj(a) * c0 + np.conj(b) * c1) / r
    A[0, 0] = 0
    return A


def targets_for(rng, n, nsys, kind="plain"):
    out = []
    for s in range(nsys):
        kappa = 10.0 ** rng.uniform(2.2, 3.8) if n > 1 else 1.0
        if kind == "interior" and n >= 4:                   # block diagonal: the second block's zero corner is the pivot of step h exactly
            h = n // 2
            A = np.zeros((n, n), dtype=np.complex128)
            A[:h, :h] = R.unitary_scaled(rng, h, np.sqrt(kappa))
            A[h:, h:] = zero_corner(R.unitary_scaled(rng, n - h, kappa))
        else:
            A = R.unitary_scaled(rng, n, kappa) * (1.0 if n > 1 else 100.0)
            if kind == "first" and n >= 2:
                A = zero_corner(A)                          # step 0 must interchange rows
        out.append(A)
    return np.stack(out)


@pytest.mark.parametrize("n", [1, 2, 3, 37, 128, 200])
def test_dense_level(n):
    rng = np.random.default_rng(1400 + n)
    k = 0
    for nsys in (1, 3):
        for nplanes in (1, 4):
            if nsys > nplanes:
                continue                                    # (different matrices need as many planes as systems)
            for op in (0, 1, 2):
                for kind in ("plain", "first", "interior"):
                    if n == 1 and kind != "plain":
                        continue
                    k += 1
                    T = targets_for(rng, n, nsys, kind)
                    if n == 1:
                        check_dense_small(rng, T, nsys, nplanes, op)
                    else:
                        check_dense(rng, n, nsys, nplanes, op, T, l=3, per_system=bool(k & 1))


def check_dense_small(rng, T, nsys, nplanes, op):
    """n = 1: the inverse is a reciprocal (kappa = 1)"""
    planes, pc = dense_planes(rng, T, nplanes, op)
    nb = nsys * 2
    X, Ainv, Y = R.rand(rng, 1, nb), R.sentinel(nsys, 1, 1), R.sentinel(1, nb)
    code, status = call(_lib.VEC_DENSE, [1, nb, nsys, nplanes, op, 2], [planes, pc, Ainv, X, Y])
    assert status == 0
    A = R.dense_assemble(planes, pc, op)
    for s in range(nsys):
        assert abs(A[s, 0, 0] * Ainv[s, 0, 0] - 1) <= 64 * EPS
        ref = X[0, 2 * s:2 * s + 2] / np.complex128(A[s, 0, 0])
        assert np.all(np.abs(Y[0, 2 * s:2 * s + 2] - ref) <= 64 * EPS * np.abs(ref))


def test_dense_level_three_systems_of_one_plane_share_it():
    """nsys = 3 with one plane: the systems differ by their coefficient only"""
    rng = np.random.default_rng(15)
    for n in (3, 37):
        P = R.unitary_scaled(rng, n, 1e3)
        pc = R.rand(rng, 3, 1)
        X, Ainv, Y = R.rand(rng, n, 6), R.sentinel(3, n, n), R.sentinel(n, 6)
        code, status = call(_lib.VEC_DENSE, [n, 6, 3, 1, 0, 2], [P[None].copy(), pc, Ainv, X, Y])
        assert status == 0
        kappa = R.cond_inf(P)
        for s in range(3):
            A = pc[s, 0] * P
            assert np.max(np.abs(A.astype(R.LD) @ Ainv[s].astype(R.LD) - np.eye(n))) <= 64 * n * EPS * kappa
            inv64 = np.linalg.inv(A)
            tol = 64 * n * EPS * kappa * np.linalg.norm(inv64, np.inf) * np.max(np.abs(X))
            assert np.max(np.abs(Y[:, 2 * s:2 * s + 2] - inv64 @ X[:, 2 * s:2 * s + 2])) <= tol


def test_dense_singular_matrix_sets_the_status_word():
    rng = np.random.default_rng(16)
    for n, col in ((1, 0), (3, 1), (37, 20)):
        A = R.unitary_scaled(rng, n, 10.0)
        A[:, col] = 0
        good = R.unitary_scaled(rng, n, 10.0)
        planes = np.stack([A, good])
        pc = np.array([[1, 0], [0, 1]], dtype=np.complex128)
        code, status = call(_lib.VEC_DENSE, [n, 1, 2, 2, 0, 1 << 30], [planes, pc, R.sentinel(2, n, n)])
        assert code == 0 and status != 0, (n, status)
        code, status = call(_lib.VEC_DENSE, [n, 1, 1, 1, 0, 1 << 30], [good[None].copy(), pc[:1, :1].copy(), R.sentinel(1, n, n)])
        assert code == 0 and status == 0, (n, status)


def test_dense_inversion_at_the_size_limit_above_the_default_lds_limit(n=2048):
    """The inversion keeps a pivot row, a pivot column and the interchanges in LDS, 36 n bytes beside 12 KB of static: past n = 1478
    that is more than the 64 KB a kernel gets by default, and launch_dense_invert has to raise the kernel's limit.  n = 2048, 84 KB,
    is the largest size the launcher accepts and the only one that shows whether all of them launch; one workgroup needs about 5 s
    for it (8 s with the numpy inverse; n = 1500 took 3.4 s).  The matrix is diagonally dominant (kappa of a few units, computed below) with its rows
    rotated by one, so that every step interchanges rows."""
    rng = np.random.default_rng(n)
    B = R.rand(rng, n, n) * (0.1 / n)
    B[np.arange(n), np.arange(n)] = R.rand(rng, n)
    A = np.ascontiguousarray(np.roll(B, 1, axis=0))
    X, Ainv, Y = R.rand(rng, n, 2), R.sentinel(1, n, n), R.sentinel(n, 2)
    code, status = call(_lib.VEC_DENSE, [n, 2, 1, 1, 0, 1 << 30], [A[None].copy(), np.ones((1, 1), dtype=np.complex128), Ainv, X, Y])
    assert code == 0 and status == 0
    inv64 = np.linalg.inv(A)
    kappa = float(np.linalg.norm(A, np.inf) * np.linalg.norm(inv64, np.inf))
    assert kappa < 100
    factor = 64 * n * EPS * kappa
    resid = np.max(np.abs(A @ Ainv[0] - np.eye(n)))
    assert resid <= factor, float(resid / factor)
    err = np.max(np.abs(Y - inv64 @ X))
    assert err <= factor * np.linalg.norm(inv64, np.inf) * np.max(np.abs(X)), float(err)


def test_dense_size_limit_is_refused_not_launched():
    """n <= 2048 (kernels.hip launch_dense_invert; the hook refuses the same sizes before it uploads or launches anything)"""
    n = 2049
    planes = np.zeros((1, n, n), dtype=np.complex128)
    Ainv = R.sentinel(1, n, n)
    code, _ = call(_lib.VEC_DENSE, [n, 1, 1, 1, 0, 1 << 30], [planes, np.ones((1, 1), dtype=np.complex128), Ainv], raise_on_error=False)
    assert code == INVALID


# ---------------------------------------------------------------------------------------------------------------------------------
# the hook's own refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def test_hook_refuses_bad_sizes():
    rng = np.random.default_rng(17)
    V, W, out = R.rand(rng, 2, 5, 8), R.rand(rng, 5, 8), R.sentinel(2, 8)
    ok = [5, 8, 2, 40]
    assert call(_lib.VEC_DOTS, ok, [V, W, out])[0] == 0
    for sizes, bufs in (([5, 257, 2, 40], [V, W, out]), ([5, 0, 2, 40], [V, W, out]), ([0, 8, 2, 40], [V, W, out]), ([6, 8, 2, 48], [V, W, out]),
                        ([5, 8, 3, 40], [V, W, out]), ([5, 8, 2, 41], [V, W, out]), ([5, 8, 2, 40], [V, W, out[:1].copy()]),
                        ([5, 8, 2, 40], [V, None, out]), ([5, 8], [V, W, out]), ([-1, 8, 2, 40], [V, W, out])):
        assert call(_lib.VEC_DOTS, sizes, bufs, raise_on_error=False)[0] == INVALID, sizes
    assert call(99, ok, [V, W, out], raise_on_error=False)[0] == INVALID
    assert call(_lib.VEC_DOTS, ok, [V, W, out], device=1 << 20, raise_on_error=False)[0] == INVALID
    assert call(_lib.VEC_DOTS_MULTI, [5, 8, 2, 5, 40, 40], [V, W, out], raise_on_error=False)[0] == INVALID
    assert call(_lib.VEC_EXTRACT_COLS, [5, 8, 6, 3], [W, R.sentinel(5, 3)], raise_on_error=False)[0] == INVALID
    assert call(_lib.VEC_BEYN_ACCUM, [5, 8, 3, 3, 2, 0, 0], [W, V[0, 0, :3].copy(), V[0, 1, :3].copy(), R.sentinel(2, 3, 5)],
                raise_on_error=False)[0] == INVALID        # 3 systems of 3 columns do not fit 8
    assert call(_lib.VEC_BEYN_ACCUM, [5, 8, 2, 3, 2, 0, 0], [W, V[0, 0, :3].copy(), V[0, 1, :3].copy(), R.sentinel(2, 2, 5)],
                perm=[0, 1, 2, 3, 5], raise_on_error=False)[0] == INVALID


# ---------------------------------------------------------------------------------------------------------------------------------
# column independence and masks
# ---------------------------------------------------------------------------------------------------------------------------------
MASK_NBS = (8, 24, 64)


def masks_for(nb):
    """a mask with a dead chunk (the only chunk at nb = 8) and one with the last chunk dead"""
    nch = (nb + 7) // 8
    return [chunk_mask(nb, [0])] + ([chunk_mask(nb, [nch - 1]), chunk_mask(nb, range(0, nch, 2))] if nch > 1 else [])


@pytest.mark.parametrize("nb", MASK_NBS)
def test_masked_chunks_keep_vectors_and_zero_reductions(nb):
    rng = np.random.default_rng(1800 + nb)
    r = 256 // nb
    for cm in masks_for(nb):
        for n in (1, r + 1, 37 * r + 5):
            check_dots(rng, n, nb, 9, cmask=cm)
            check_dots(rng, n, nb, 33, cmask=cm, scaled=True)
            check_norms(rng, n, nb, cmask=cm)
            check_dots2(rng, n, nb, 17, cmask=cm)
            check_axpy(rng, _lib.VEC_AXPY_NEG, n, nb, 9, cmask=cm)
            check_axpy(rng, _lib.VEC_AXPY_NEG, n, nb, 4096 // nb + 1, cmask=cm)
            check_axpy_neg_norm(rng, n, nb, 9, True, True, cmask=cm)
            check_axpy_neg_norm(rng, n, nb, 9, False, False, cmask=cm)
            check_axpy_neg_norm(rng, n, nb, 0, False, False, cmask=cm)
            check_axpy2(rng, n, nb, 9, cmask=cm)
            check_axpy2(rng, n, nb, 25 * 64 // nb, cmask=cm)
            X, alpha, Y = R.rand(rng, n, nb), R.rand(rng, nb), R.sentinel(n, nb)
            call(_lib.VEC_SCALE_INV, [n, nb], [X, alpha, Y], cmask=cm)
            C = Cols(nb, cm)
            assert_untouched(Y, ~C.live, "scale_inv")
            ref = scale_inv_ref(X, alpha)
            assert_close(Y, ref, 2 * EPS * np.abs(ref), C.live, "scale_inv masked")
        T = targets_for(rng, 37, 1)
        check_dense(rng, 37, 1, 1, 0, T, l=nb, cmask=cm)


@pytest.mark.parametrize("nb", MASK_NBS)
def test_a_nan_column_changes_no_other_column(nb):
    rng = np.random.default_rng(1900 + nb)
    r = 256 // nb
    for nan_col in (0, nb // 2 + 1, nb - 1):
        for n in (r + 1, 37 * r + 5):
            check_dots(rng, n, nb, 9, nan_col=nan_col)
            check_dots(rng, n, nb, 33, nan_col=nan_col, scaled=True)
            check_norms(rng, n, nb, nan_col=nan_col)
            check_dots_multi(rng, n, nb, 9, 3, nan_col=nan_col)
            check_dots2(rng, n, nb, 17, nan_col=nan_col)
            for op in (_lib.VEC_AXPY_NEG, _lib.VEC_LINCOMB, _lib.VEC_LINCOMB_ADD):
                check_axpy(rng, op, n, nb, 9, nan_col=nan_col)
            check_axpy_neg_norm(rng, n, nb, 9, True, True, nan_col=nan_col)
            check_axpy_neg_norm(rng, n, nb, 9, False, False, nan_col=nan_col)
            check_axpy_neg_multi(rng, n, nb, 5, 3, nan_col=nan_col)
            check_axpy2(rng, n, nb, 9, nan_col=nan_col)
            check_axpy2(rng, n, nb, 25 * 64 // nb, nan_col=nan_col)
            check_lincomb_rep(rng, n, nb, 8, 5, nan_col=nan_col)
            check_lincomb_rep(rng, n, nb, 2, 5, nan_col=nan_col)
            check_pt_gemm(rng, n, nb, 5, 5, nan_col=nan_col)
            check_pt_axpby(rng, n, nb, nan_col=nan_col, dead=((nan_col + 3) % nb,))
            check_pt_project(rng, n, nb, 3, nan_col=nan_col)
        T = targets_for(rng, 37, 1)
        check_dense(rng, 37, 1, 1, 0, T, l=nb, nan_col=nan_col)
