"""The extended-precision references of tests/_vecref.py against a second formulation of each (float64 einsum / matmul), within the
float64 rounding bound of that second formulation: the references of the kernel tests are verified without a GPU."""
import numpy as np

import _vecref as R


def _close(ref, other, mag, m):
    assert ref.dtype == R.LD and ref.shape == other.shape
    err = np.abs(ref - other.astype(R.LD))
    assert np.all(err <= 2 * (m + 4) * R.EPS * mag), float(np.max(err / (R.EPS * mag)))


def test_longdouble_has_a_64_bit_mantissa():
    assert np.finfo(np.longdouble).eps < 1.1e-19


def test_inputs_are_never_small():
    x = R.rand(np.random.default_rng(0), 1000, 3)
    assert x.dtype == np.complex128 and np.all(np.abs(x) >= 0.5) and np.all(np.abs(x) <= 2.0)


def test_reductions():
    rng = np.random.default_rng(1)
    V, W = R.rand(rng, 5, 301, 7), R.rand(rng, 3, 301, 7)
    out, mag = R.dots(V, W[0])
    _close(out, np.einsum("irb,rb->ib", V.conj(), W[0]), mag, 301)
    assert np.allclose(np.asarray(mag, dtype=float), np.einsum("irb,rb->ib", np.abs(V), np.abs(W[0])))
    out, mag = R.dots_multi(V, W)
    _close(out, np.einsum("irb,jrb->ijb", V.conj(), W), mag, 301)
    sq = R.sqnorms(W[1])
    assert np.allclose(np.asarray(sq, dtype=float), np.linalg.norm(W[1], axis=0) ** 2, rtol=1e-13)


def test_updates():
    rng = np.random.default_rng(2)
    V, c, base = R.rand(rng, 9, 41, 6), R.rand(rng, 9, 6), R.rand(rng, 41, 6)
    out, mag = R.update(base, c, V, -1.0)
    _close(out, base - np.einsum("ib,irb->rb", c, V), mag, 9)
    out, mag = R.update(None, c, V)
    _close(out, np.einsum("ib,irb->rb", c, V), mag, 9)
    assert np.all(mag > 0)
    Q = R.rand(rng, 9, 41, 3)
    out, mag = R.lincomb_rep(Q, c, 6, 3)
    _close(out, np.einsum("ib,irb->rb", c, np.concatenate([Q, Q], axis=2)), mag, 9)
    G = R.rand(rng, 9, 4, 6)
    out, mag = R.pt_gemm(V, G)
    _close(out, np.einsum("itb,irb->rtb", G, V), mag, 9)
    coef = R.rand(rng, 2, 6)
    coef[:, 2] = 0
    x, y = R.rand(rng, 41, 6), R.rand(rng, 41, 6)
    x[:, 2] = np.nan
    out, mag = R.axpby_cols(coef, x, y)
    keep = np.arange(6) != 2
    _close(out[:, keep], (coef[0] * x + coef[1] * y)[:, keep], mag[:, keep], 2)
    assert np.all(out[:, 2] == 0)
    d = R.rand(rng, 4, 6)
    out, mag = R.pt_project(x[:, keep], y[:, keep], d[:, keep])
    _close(out, x[:, keep] + (-d[0] - 0.5 * d[1:].sum(axis=0))[keep] * y[:, keep], mag, 5)


def test_beyn_accum():
    rng = np.random.default_rng(3)
    l, nsys, npow, d = 3, 4, 5, 17
    X, w = R.rand(rng, d, 13), R.rand(rng, nsys)
    z = rng.uniform(0.8, 1.25, nsys) * np.exp(1j * rng.uniform(0, 6.28, nsys))
    out, mag = R.beyn_accum(X, w, z, npow, l)
    zp = z[None, :] ** np.arange(npow)[:, None]
    other = np.einsum("s,ps,rsc->pcr", w, zp, X[:, :nsys * l].reshape(d, nsys, l))
    _close(out, other, mag, nsys + npow)


def test_dense_helpers():
    rng = np.random.default_rng(4)
    planes, pc = R.rand(rng, 3, 5, 5), R.rand(rng, 2, 3)
    for op, f in ((0, lambda P: P), (1, lambda P: P.T), (2, lambda P: P.conj().T)):
        A = R.dense_assemble(planes, pc, op)
        other = np.stack([sum(pc[s, q] * f(planes[q]) for q in range(3)) for s in range(2)])
        assert np.max(np.abs(A - other)) < 1e-13
    A = R.unitary_scaled(rng, 37, 1e3)
    s = np.linalg.svd(A, compute_uv=False)
    assert abs(s[0] / s[-1] / 1e3 - 1) < 1e-8
    assert 1e2 < R.cond_inf(A) < 1e5
