"""Plain references of the streaming and reduction kernels (tests/test_gpu_vector_kernels.py), in numpy's extended precision
(clongdouble: 64-bit mantissa on x86-64), each written as its defining formula.  Every function returns the value and the sum of
the magnitudes of its terms, which the rounding bounds are built from.  tests/test_vecref.py checks each against a second
formulation (float64 einsum), so that the references are verified where no GPU is."""
import numpy as np

LD = np.clongdouble
EPS = float(np.finfo(np.float64).eps)
SENTINEL = 3 + 7j


def rand(rng, *shape):
    """entries rho e^{i phi}, rho uniform in [0.5, 2]: no entry is small, every row carries weight in every sum"""
    return (rng.uniform(0.5, 2.0, shape) * np.exp(1j * rng.uniform(0.0, 2 * np.pi, shape))).astype(np.complex128)


def sentinel(*shape):
    return np.full(shape, SENTINEL, dtype=np.complex128)


def dots(V, W):
    """out[i][b] = sum_rows conj(V_i[row][b]) W[row][b];  V: (nv, n, nb), W: (n, nb)"""
    Wl = W.astype(LD)
    aW = np.abs(Wl)
    out = np.zeros((V.shape[0], V.shape[2]), dtype=LD)
    mag = np.zeros(out.shape, dtype=np.longdouble)
    for i in range(V.shape[0]):
        Vi = V[i].astype(LD)
        out[i] = (np.conj(Vi) * Wl).sum(axis=0)
        mag[i] = (np.abs(Vi) * aW).sum(axis=0)
    return out, mag


def dots_multi(V, W):
    """out[i][j][b] = V_i[:, b]^H W_j[:, b]"""
    out = np.zeros((V.shape[0], W.shape[0], V.shape[2]), dtype=LD)
    mag = np.zeros(out.shape, dtype=np.longdouble)
    for j in range(W.shape[0]):
        out[:, j], mag[:, j] = dots(V, W[j])
    return out, mag


def sqnorms(X):
    """||X[:, b]||^2"""
    a = np.abs(X.astype(LD))
    return (a * a).sum(axis=0)


def update(base, c, V, sign=1.0):
    """base + sign * sum_i c[i][b] V_i[row][b];  base: (n, nb) or None, c: (nv, nb), V: (nv, n, nb)"""
    n, nb = V.shape[1], V.shape[2]
    out = np.zeros((n, nb), dtype=LD) if base is None else base.astype(LD)
    mag = np.abs(out)
    for i in range(V.shape[0]):
        ci, Vi = c[i].astype(LD)[None, :], V[i].astype(LD)
        out = out + sign * ci * Vi
        mag = mag + np.abs(ci) * np.abs(Vi)
    return out, mag


def lincomb_rep(Q, y, nb, l):
    """X[row][b] = sum_i y[i][b] Q_i[row][b % l];  Q: (nv, n, l), y: (nv, nb)"""
    cols = np.arange(nb) % l
    return update(None, y, Q[:, :, cols])


def beyn_accum(X, w, z, npow, l):
    """add[p][c][row] = sum_s w[s] z[s]^p X[row][s*l + c];  X: (d, nb), nsys = len(w)"""
    d = X.shape[0]
    Xl = X.astype(LD)
    out = np.zeros((npow, l, d), dtype=LD)
    mag = np.zeros(out.shape, dtype=np.longdouble)
    for s in range(len(w)):
        blk = Xl[:, s * l:(s + 1) * l].T
        for p in range(npow):
            f = LD(w[s]) * LD(z[s]) ** p
            out[p] += f * blk
            mag[p] += np.abs(f) * np.abs(blk)
    return out, mag


def pt_gemm(V, G):
    """U[row][t][b] = sum_i G[i][t][b] V_i[row][b];  V: (k, d, nb), G: (k, T, nb)"""
    k, d, nb = V.shape
    T = G.shape[1]
    out = np.zeros((d, T, nb), dtype=LD)
    mag = np.zeros(out.shape, dtype=np.longdouble)
    for i in range(k):
        Gi, Vi = G[i].astype(LD)[None, :, :], V[i].astype(LD)[:, None, :]
        out += Gi * Vi
        mag += np.abs(Gi) * np.abs(Vi)
    return out, mag


def axpby_cols(coef, x, y):
    """a[b] x + c[b] y per column, a column with a = c = 0 is exact zero;  coef: (2, nb)"""
    a, c = coef[0].astype(LD)[None, :], coef[1].astype(LD)[None, :]
    out = a * x.astype(LD) + c * y.astype(LD)
    mag = np.abs(a) * np.abs(x) + np.abs(c) * np.abs(y)
    dead = (coef[0] == 0) & (coef[1] == 0)
    out[:, dead] = 0
    mag[:, dead] = 0
    return out, mag


def pt_project(vk, v0, dots_):
    """vk + (-dots[0][b] - 1/2 sum_{j>=1} dots[j][b]) v0"""
    dl = dots_.astype(LD)
    c = -dl[0] - (dl[1:].sum(axis=0) / 2 if dl.shape[0] > 1 else 0)
    mc = np.abs(dl[0]) + np.abs(dl[1:]).sum(axis=0) / 2
    return vk.astype(LD) + c[None, :] * v0.astype(LD), np.abs(vk) + mc[None, :] * np.abs(v0)


def dense_assemble(planes, pc, op):
    """A_s = sum_q pc[s][q] op(plane_q); op 0: plane, 1: plane^T, 2: conj(plane)^T;  planes: (nplanes, n, n), pc: (nsys, nplanes)"""
    P = planes.astype(LD)
    if op != 0:
        P = P.transpose(0, 2, 1)
    if op == 2:
        P = np.conj(P)
    return (pc.astype(LD)[:, :, None, None] * P[None]).sum(axis=1)


def unitary_scaled(rng, n, kappa):
    """U diag(s) V^H with singular values log-spaced from 1 down to 1/kappa"""
    def unitary():
        q, r = np.linalg.qr(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))
        return q * (np.diag(r) / np.abs(np.diag(r)))[None, :]
    s = np.logspace(0.0, -np.log10(kappa), n) if n > 1 else np.ones(1)
    return (unitary() * s[None, :]) @ unitary().conj().T


def cond_inf(A):
    return float(np.linalg.norm(A, np.inf) * np.linalg.norm(np.linalg.inv(A), np.inf))
