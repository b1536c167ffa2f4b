"""The update kernel under `x += V y` and `w -= V h` (vec.hip axpy_neg_kernel) skips, lane by lane, every (vector, column) pair whose
coefficient is exactly (0, 0): it neither loads that entry of V nor adds to its sum.  ONE launch at a time through wae_debug_vec
(WAE_VEC_LINCOMB_ADD, WAE_VEC_AXPY_NEG), against tests/_vecref.update under the rounding bound tests/test_gpu_vector_kernels.py uses
for this kernel, 4 (m + 2) eps (|base| + sum_i |c_i||v_i|) per element.

Shape: 1 031 rows (no multiple of any row-group count 256 // nb), nb in {8, 19, 64}, nv in {1, 9, 33} (the loop of 8 vectors and
its tail).  Per column b the coefficients of the last k_b vectors are exact zeros, as vec.hip gmres_solve_y_kernel leaves them for
the steps beyond a column's own: the chunks with index 1 mod 3 have one k for their 8 columns (whole 128-byte segments of a vector
are skipped), the others a different k_b in every column (lanes of one segment go different ways).

  1. the result against the reference;
  2. the same bits when the skipped entries of V hold other finite values;
  3. the same bits, hence finite, when they hold NaN (a masked chunk of a Krylov slot keeps stale bits: 0 * NaN would poison the sum)."""
import numpy as np
import pytest

import _vecref as R
from wae_amd import _lib

pytestmark = pytest.mark.gpu

N = 1031


def zero_tail(nb, nv):
    """k_b per column, 0 <= k_b <= nv"""
    b = np.arange(nb)
    chunk = b >> 3
    mixed = (b * 3 + 1) % (nv + 1)
    uniform = np.minimum(nv, 2 + chunk)
    return np.where(chunk % 3 == 1, uniform, mixed)


def upd_tol(mag, m):
    return 4 * (m + 2) * R.EPS * mag


@pytest.mark.parametrize("nv", [1, 9, 33])
@pytest.mark.parametrize("nb", [8, 19, 64])
@pytest.mark.parametrize("op", [_lib.VEC_LINCOMB_ADD, _lib.VEC_AXPY_NEG], ids=["lincomb_add", "axpy_neg"])
def test_zero_coefficients_are_skipped(op, nb, nv):
    rng = np.random.default_rng(1000 * op + 10 * nb + nv)
    kb = zero_tail(nb, nv)
    skipped = np.arange(nv)[:, None] >= (nv - kb)[None, :]          # (nv, nb): coefficient exactly zero
    if nb > 8:
        per_chunk = [skipped[:, c0:c0 + 8] for c0 in range(0, nb, 8)]
        assert any(np.any(np.all(s, axis=1) & np.any(skipped, axis=1)) for s in per_chunk), "no chunk is entirely zero for a vector"
    assert np.any(np.any(skipped, axis=1) & ~np.all(skipped, axis=1)), "no vector has both zero and non-zero coefficients"
    assert len(set(kb[:8])) > 1
    V, c = R.rand(rng, nv, N, nb), R.rand(rng, nv, nb)
    c[skipped] = 0
    W0 = R.rand(rng, N, nb)
    sign = -1.0 if op == _lib.VEC_AXPY_NEG else 1.0
    ref, mag = R.update(W0, c, V, sign)
    hole = np.broadcast_to(skipped[:, None, :], V.shape)
    other = R.rand(rng, nv, N, nb) * 1e3

    def run(fill):
        Vr = V.copy()
        if fill is not None:
            Vr[hole] = fill if np.isscalar(fill) else fill[hole]
        W = W0.copy()
        _lib.debug_vec(op, [N, nb, nv, N * nb], [Vr, c.copy(), W])
        return W

    what = f"op {op} nb={nb} nv={nv}"
    W = run(None)
    assert np.all(np.isfinite(W)), what
    err = np.abs(W.astype(R.LD) - ref)
    tol = upd_tol(mag, nv)
    assert np.all(err <= tol), (what, float(np.max(err / tol)))
    W2 = run(other)
    assert np.array_equal(W.view(np.uint64), W2.view(np.uint64)), what + ": the result depends on entries with a zero coefficient"
    W3 = run(np.nan)
    assert np.all(np.isfinite(W3)), what + ": a NaN behind a zero coefficient reached the result"
    assert np.array_equal(W.view(np.uint64), W3.view(np.uint64)), what
    untouched = kb == nv                                             # every coefficient of the column is zero
    assert np.array_equal(W[:, untouched], W0[:, untouched]), what


def test_zero_coefficients_in_a_masked_update():
    """w -= V h with a chunk mask as the Gram-Schmidt steps pass it: the masked chunk keeps its values, the others skip their zeros"""
    nb, nv = 19, 9
    rng = np.random.default_rng(7)
    kb = zero_tail(nb, nv)
    skipped = np.arange(nv)[:, None] >= (nv - kb)[None, :]
    V, c = R.rand(rng, nv, N, nb), R.rand(rng, nv, nb)
    c[skipped] = 0
    V[np.broadcast_to(skipped[:, None, :], V.shape)] = np.nan
    cmask = np.array([1, 0, 1], dtype=bool)
    live = cmask[np.arange(nb) >> 3]
    W0 = R.rand(rng, N, nb)
    W = W0.copy()
    _lib.debug_vec(_lib.VEC_AXPY_NEG, [N, nb, nv, N * nb], [V, c, W], cmask=cmask)
    Vf = np.where(np.isnan(V), 0, V)
    ref, mag = R.update(W0, c, Vf, -1.0)
    assert np.all(np.isfinite(W))
    assert np.all(np.abs(W.astype(R.LD) - ref)[:, live] <= upd_tol(mag, nv)[:, live])
    assert np.array_equal(W[:, ~live], W0[:, ~live])
