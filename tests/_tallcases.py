"""Synthetic moment tensors with known eigenpairs, the checks of an extraction against them, and a numpy stand-in for the three
tall-matrix operations -- shared by tests/test_tall_host_logic.py (CPU) and tests/test_gpu_tall.py (device)."""
import functools

import numpy as np

from wae_amd.nlevp.beyn import moments2eigs

LAMBDA = np.array([1.2, -0.9 + 0.4j, 0.3 + 0.8j, -0.2 - 0.9j, 0.8 - 0.7j, -0.6 + 0.0j])
FACTOR = 10.0            # Gram stages against Householder QR: a different but backward-stable route
FLOOR = 1e-13


@functools.lru_cache(maxsize=None)
def rank6_moments(l, K, d=517, seed=20):
    """A_p = sum_m lambda_m^p v_m (w_m^H V), p < 2K: the moments of a problem with exactly six eigenvalues (beyn.jl:62-74 in exact
    arithmetic).  Returns (A (d, l, 2K), v (d, 6))."""
    mod = np.abs(LAMBDA)
    gap = np.abs(LAMBDA[:, None] - LAMBDA[None, :]) + 10.0 * np.eye(6)
    assert mod.min() >= 0.5 and mod.max() <= 1.5 and gap.min() >= 0.3
    rng = np.random.default_rng(seed)
    cn = lambda *s: rng.standard_normal(s) + 1j * rng.standard_normal(s)      # noqa: E731
    v, w, V = cn(d, 6), cn(d, 6), cn(d, l)
    wV = w.conj().T @ V
    A = np.stack([(v * LAMBDA ** p) @ wV for p in range(2 * K)], axis=2)
    A.setflags(write=False)
    return A, v


def hankel0(A):
    d, l, K2 = A.shape
    K = K2 // 2
    return np.vstack([np.hstack([A[:, :, i + j] for j in range(K)]) for i in range(K)])


def match(Om, P, v):
    """(largest distance of a lambda_m to its nearest computed eigenvalue, largest 1 - |cos| between v_m and that eigenvector)"""
    e_val, e_vec = 0.0, 0.0
    for m, lam in enumerate(LAMBDA):
        k = int(np.argmin(np.abs(Om - lam)))
        e_val = max(e_val, abs(Om[k] - lam))
        c = abs(np.vdot(v[:, m], P[:, k])) / (np.linalg.norm(v[:, m]) * np.linalg.norm(P[:, k]))
        e_vec = max(e_vec, abs(1.0 - c))
    return e_val, e_vec


@functools.lru_cache(maxsize=None)
def host_reference(l, K):
    """the package's host `moments2eigs` (the reference's algorithm, not code under test) on the rank-6 moments, directions above
    1e-6 sigma_1: (Sigma, eigenvalue error, eigenvector error)"""
    A, v = rank6_moments(l, K)
    s1 = np.linalg.svd(hankel0(A), compute_uv=False)[0]
    Om, P, S = moments2eigs(np.array(A), tol_sigma=1e-6 * s1, return_sigma=True)
    assert len(Om) == 6
    return (S,) + match(Om, P, v)


def check_rank6(Om, P, Sall, l, K, label):
    """the assertions both test files make on an extraction of the rank-6 moments (P: host array d x kept)"""
    _, v = rank6_moments(l, K)
    S_host, ev_host, evec_host = host_reference(l, K)
    e_val, e_vec = match(Om, P, v)
    bound = FACTOR * ev_host + FLOOR * np.abs(LAMBDA).max()
    print(f"{label}: err_host {ev_host:.2e} (vectors {evec_host:.2e})  native {e_val:.2e} (vectors {e_vec:.2e})  factor {FACTOR:g}  "
          f"bound {bound:.2e}  Sigma7/Sigma6 {Sall[6] / Sall[5]:.1e}")
    assert len(Om) == 6 and P.shape[1] == 6
    assert e_val <= bound, (e_val, bound)
    assert np.all(np.abs(Sall[:6] - S_host[:6]) <= bound * S_host[0]), (Sall[:6], S_host[:6])
    assert Sall[6] / Sall[5] < 1e-9
    assert e_vec <= FACTOR * evec_host + FLOOR, (e_vec, evec_host)


@functools.lru_cache(maxsize=None)
def two_group_moments(d=389, seed=21):
    """K = 1, l = 6: B0 = Q diag(s) Z^H with two groups of singular values twelve decades apart, B1 = B0 T.  Returns (A (d, 6, 2), s, T)."""
    rng = np.random.default_rng(seed)
    cn = lambda *s: rng.standard_normal(s) + 1j * rng.standard_normal(s)      # noqa: E731
    Q, _ = np.linalg.qr(cn(d, 6))
    Z, _ = np.linalg.qr(cn(6, 6))
    s = np.array([1.0, 0.5, 0.3, 1e-12, 5e-13, 2e-13])
    B0 = (Q * s) @ Z.conj().T
    T = cn(6, 6)
    A = np.stack([B0, B0 @ T], axis=2)
    A.setflags(write=False)
    return A, s, T


class NumpyTall:
    """the three operations of wae_amd.nlevp.tall on a numpy array; new() hands out NaNs, so reading scratch that was never
    written shows"""

    def __init__(self, a):
        self.a = np.array(a, dtype=np.complex128, order="F")
        self.a = self.a.reshape(self.a.shape[0], -1, order="F")

    rows = property(lambda self: self.a.shape[0])
    ncols = property(lambda self: self.a.shape[1])

    def new(self, rows, ncols):
        return NumpyTall(np.full((rows, ncols), complex(np.nan, np.nan)))

    def release(self):
        self.a = None

    def to_host(self):
        return self.a.copy()

    def gram(self, other=None, a_col0=0, na=None, b_col0=0, nb=None):
        other = self if other is None else other
        na = self.ncols - a_col0 if na is None else na
        nb = other.ncols - b_col0 if nb is None else nb
        return self.a[:, a_col0:a_col0 + na].conj().T @ other.a[:, b_col0:b_col0 + nb]

    def mul(self, src, Cm, dst_col0=0, src_col0=0, src_row0=0, alpha=1.0, beta=0.0):
        Cm = np.asarray(Cm, dtype=np.complex128)
        ns, nc = Cm.shape
        assert src is not self or dst_col0 + nc <= src_col0 or src_col0 + ns <= dst_col0
        upd = alpha * (src.a[src_row0:src_row0 + self.rows, src_col0:src_col0 + ns] @ Cm)
        if beta != 0:
            upd = upd + beta * self.a[:, dst_col0:dst_col0 + nc]
        self.a[:, dst_col0:dst_col0 + nc] = upd
        return self

    def hankel(self, moments, l, K, shift):
        d = moments.rows
        for i in range(K):
            for j in range(K):
                self.a[i * d:(i + 1) * d, j * l:(j + 1) * l] = moments.a[:, (i + j + shift) * l:(i + j + shift + 1) * l]
        return self
