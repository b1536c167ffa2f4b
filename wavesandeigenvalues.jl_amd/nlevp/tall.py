"""Tall matrices in HBM (``wae_tall_*`` of include/waehip.h) and the staged extraction of Beyn's eigenpairs written on them.

``TallMatrix`` wraps a library-owned column-major rows x ncols complex matrix.  The step that turns moments into eigenpairs
(beyn.jl:76-107, 289-323) needs three operations on such matrices, and ``staged_extract`` below uses nothing else:

    A.gram(B, a_col0, na, b_col0, nb)                    ->  numpy  A[:, a..]^H B[:, b..]
    D.mul(S, C, dst_col0, src_col0, src_row0, alpha, beta)   D[:, d..] = beta D[:, d..] + alpha S[r0.., s..] C
    D.hankel(M, l, K, shift)                             the block Hankel matrix B0 / B1 of the moments M
    A.new(rows, ncols)  /  A.release()                   scratch of the same kind (contents not to be relied on) / give it back

so any class with these methods (a numpy one, tests/test_tall_host_logic.py) runs the same algorithm on the CPU.  No torch.
"""
from __future__ import annotations

import ctypes as C
import threading

import numpy as np

from .. import _lib

MAXCOLS = _lib.TALL_MAXCOLS


def _z(a):
    return _lib.zptr(a)


class TallMatrix:
    """rows x ncols ComplexF64 in HBM, leading dimension rows, the caller's row numbering.  ``ptr`` is the raw device address:
    ``out_dev`` of the moment integrals, ``P_dev`` of ``eig_residuals``."""
    # Opt-in cache of released matrices (off by default: release() frees).  A caller that extracts again and again at one shape
    # (a sweep, a benchmark loop) sets ``TallMatrix.POOL_LIMIT`` to the bytes of HBM it is willing to leave parked between calls:
    # new() then reuses a released matrix of the same shape instead of paying hipMalloc, the zero fill of create and hipFree.
    # trim_pool() frees what is parked.
    _pool: dict = {}            # (device, rows, ncols) -> released handles
    _pool_bytes = 0
    _pool_lock = threading.Lock()
    POOL_LIMIT = 0

    def __init__(self, handle, rows, ncols, device):
        self.handle, self.rows, self.ncols, self.device = handle, int(rows), int(ncols), int(device)

    # -- life cycle ----------------------------------------------------------------------------------
    @classmethod
    def create(cls, rows, ncols, device=0):
        """zero-filled"""
        h = C.c_void_p()
        _lib.check(_lib.lib().wae_tall_create(C.byref(h), int(device), int(rows), int(ncols)))
        return cls(h, rows, ncols, device)

    @classmethod
    def from_host(cls, X, device=0):
        X = np.asarray(X, dtype=np.complex128)
        X = X.reshape(X.shape[0], -1, order="F")
        m = cls.create(X.shape[0], X.shape[1], device)
        m.write(X)
        return m

    def new(self, rows, ncols):
        """scratch on the same device, contents UNDEFINED where it comes from the pool (see POOL_LIMIT), zero otherwise"""
        key = (self.device, int(rows), int(ncols))
        with TallMatrix._pool_lock:
            free = TallMatrix._pool.get(key)
            h = free.pop() if free else None
            if h is not None:
                TallMatrix._pool_bytes -= 16 * int(rows) * int(ncols)
        return TallMatrix(h, rows, ncols, self.device) if h is not None else TallMatrix.create(rows, ncols, self.device)

    def release(self):
        """give the storage back: freed, or parked for the next new() of the same shape while the pool stays within POOL_LIMIT bytes"""
        if not self.handle:
            return
        nbytes = 16 * self.rows * self.ncols
        with TallMatrix._pool_lock:
            park = TallMatrix._pool_bytes + nbytes <= TallMatrix.POOL_LIMIT
            if park:
                TallMatrix._pool.setdefault((self.device, self.rows, self.ncols), []).append(self.handle)
                TallMatrix._pool_bytes += nbytes
                self.handle = None
        if not park:
            self.destroy()

    def destroy(self):
        if getattr(self, "handle", None):
            _lib.lib().wae_tall_destroy(self.handle)
        self.handle = None

    @classmethod
    def trim_pool(cls):
        with cls._pool_lock:
            pool, cls._pool, cls._pool_bytes = cls._pool, {}, 0
        for handles in pool.values():
            for h in handles:
                _lib.lib().wae_tall_destroy(h)

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass

    @property
    def ptr(self):
        p = C.c_uint64(0)
        _lib.check(_lib.lib().wae_tall_info(self.handle, None, None, C.byref(p)))
        return p.value

    # -- host copies ---------------------------------------------------------------------------------
    def write(self, X, row0=0, col0=0):
        X = np.asfortranarray(np.asarray(X, dtype=np.complex128))
        X = X.reshape(X.shape[0], -1, order="F")
        _lib.check(_lib.lib().wae_tall_write(self.handle, int(row0), X.shape[0], int(col0), X.shape[1], _z(X)))

    def to_host(self, row0=0, nrows=None, col0=0, ncols=None):
        nrows = self.rows - row0 if nrows is None else nrows
        ncols = self.ncols - col0 if ncols is None else ncols
        X = np.zeros((nrows, ncols), dtype=np.complex128, order="F")
        _lib.check(_lib.lib().wae_tall_read(self.handle, int(row0), int(nrows), int(col0), int(ncols), _z(X)))
        return X

    # -- the three operations --------------------------------------------------------------------------
    def gram(self, other=None, a_col0=0, na=None, b_col0=0, nb=None):
        """self[:, a_col0 : a_col0+na]^H other[:, b_col0 : b_col0+nb] (numpy, na x nb); blocks of MAXCOLS columns per call"""
        other = self if other is None else other
        na = self.ncols - a_col0 if na is None else na
        nb = other.ncols - b_col0 if nb is None else nb
        G = np.zeros((na, nb), dtype=np.complex128, order="F")
        L = _lib.lib()
        for i0 in range(0, na, MAXCOLS):
            wi = min(MAXCOLS, na - i0)
            for j0 in range(0, nb, MAXCOLS):
                wj = min(MAXCOLS, nb - j0)
                blk = np.zeros((wi, wj), dtype=np.complex128, order="F")
                _lib.check(L.wae_tall_gram(self.handle, a_col0 + i0, wi, other.handle, b_col0 + j0, wj, _z(blk)))
                G[i0:i0 + wi, j0:j0 + wj] = blk
        return G

    def mul(self, src, Cm, dst_col0=0, src_col0=0, src_row0=0, alpha=1.0, beta=0.0):
        """self[:, dst_col0 : +nc] = beta self[:, ...] + alpha src[src_row0 : src_row0+rows, src_col0 : +ns] Cm   (Cm: ns x nc, numpy)"""
        Cm = np.asarray(Cm, dtype=np.complex128)
        ns, nc = Cm.shape
        L = _lib.lib()
        al = np.array([alpha], dtype=np.complex128)
        one = np.array([1.0], dtype=np.complex128)
        for j0 in range(0, nc, MAXCOLS):
            wj = min(MAXCOLS, nc - j0)
            be = np.array([beta], dtype=np.complex128)
            for i0 in range(0, ns, MAXCOLS):                       # more than MAXCOLS source columns: accumulate block by block
                wi = min(MAXCOLS, ns - i0)
                blk = np.asfortranarray(Cm[i0:i0 + wi, j0:j0 + wj])
                _lib.check(L.wae_tall_mul(self.handle, dst_col0 + j0, src.handle, int(src_row0), src_col0 + i0, wi, _z(blk), wj, _z(al), _z(be)))
                be = one
        return self

    def hankel(self, moments, l, K, shift):
        _lib.check(_lib.lib().wae_tall_hankel(self.handle, moments.handle, int(l), int(K), int(shift)))
        return self


def staged_extract(B0, b0_col0, B1, b1_col0, d, n, rel_tol=0.0, tol_sigma=0.0, info=None):
    """Eigenpairs from the block Hankel matrices B0 = B0[:, b0_col0 : +n], B1 likewise (beyn.jl:92-107), tall parts through
    gram / mul only.  Thin SVD of B0 from Gram matrices by deflation in stages, so that every group of singular values comes out
    to full relative accuracy although a Gram matrix resolves only ~1e-8 of its largest: a stage takes the directions within six
    decades of the largest singular value of what is left (that group's Gram matrix loses nothing that matters), makes them
    orthonormal with a second Cholesky-QR pass, projects them out; the next stage starts from the remainder, until that is below
    rel_tol times the largest singular value of all (rel_tol = 0: until every direction is taken).  Then the exact SVD of U^H B0
    for the kept group, U^H B1 W S^-1, its eigenpairs, and P = U[:d] Y on the device.  tol_sigma > 0 drops kept directions with
    singular value <= tol_sigma (the reference's absolute `tol`, beyn.jl:92-95).
    Returns (Omega, P (d x kept, same kind as B0), all n singular values); info (a dict) receives 'stages' and 'kept'."""
    stage_span = 1e-6
    R = B0.rows
    rest, rc, own_rest = B0, b0_col0, False
    blocks, s_top, S, stages = [], None, None, 0
    for _ in range(8):                                              # 16 decades / 6 per stage: 3 suffice in double precision
        G = rest.gram(rest, rc, n, rc, n)
        lam, W = np.linalg.eigh(0.5 * (G + G.conj().T))
        lam, W = np.maximum(lam[::-1], 0.0), W[:, ::-1]
        S = np.sqrt(lam)
        if s_top is None:
            s_top = float(S[0])
        nkept = sum(b.ncols for b in blocks)
        if S[0] <= rel_tol * s_top or S[0] == 0.0 or nkept >= n:
            break
        k = min(int((S > max(rel_tol * s_top, stage_span * S[0])).sum()), n - nkept)
        stages += 1
        U = B0.new(R, k).mul(rest, W[:, :k] / S[:k], src_col0=rc)
        for Ub in blocks:                                           # (later stages: rounding left along the earlier blocks)
            U.mul(Ub, Ub.gram(U), alpha=-1.0, beta=1.0)
        G2 = U.gram(U)                                              # second pass of the same construction on U itself
        l2, W2 = np.linalg.eigh(0.5 * (G2 + G2.conj().T))
        U2 = B0.new(R, k).mul(U, (W2 / np.sqrt(l2)) @ W2.conj().T)  # U G2^{-1/2}: orthonormal to rounding
        U.release()
        blocks.append(U2)
        Cm = U2.gram(rest, 0, k, rc, n)
        if not own_rest:                                            # the first remainder: a copy, B0 itself is needed again below
            rest, rc, own_rest = B0.new(R, n).mul(rest, np.eye(n), src_col0=rc), 0, True
        rest.mul(U2, Cm, alpha=-1.0, beta=1.0)
    if own_rest:
        rest.release()
    if not blocks:
        raise ValueError("staged_extract: the matrix is zero")
    # the singular triplets of the kept group, exactly: B0 = U (U^H B0) + rest
    UhB0 = np.vstack([Ub.gram(B0, 0, Ub.ncols, b0_col0, n) for Ub in blocks])
    Uc, Sc, Whc = np.linalg.svd(UhB0, full_matrices=False)
    ktot = UhB0.shape[0]
    Sall = np.concatenate([Sc, S[:n - ktot]])
    if tol_sigma > 0:
        m = Sc > tol_sigma
        Uc, Sc, Whc = Uc[:, m], Sc[m], Whc[m, :]
    if len(Sc) == 0:
        raise ValueError("staged_extract: tol_sigma leaves no singular direction")
    UhB1 = np.vstack([Ub.gram(B1, 0, Ub.ncols, b1_col0, n) for Ub in blocks])
    Om, Y = np.linalg.eig((Uc.conj().T @ UhB1 @ Whc.conj().T) / Sc)
    P = B0.new(d, len(Sc))
    r0 = 0
    for i, Ub in enumerate(blocks):                                 # P = (U Uc)[:d] Y, block by block
        P.mul(Ub, Uc[r0:r0 + Ub.ncols, :] @ Y, beta=0.0 if i == 0 else 1.0)
        r0 += Ub.ncols
        Ub.release()
    if info is not None:
        info.update(stages=stages, kept=len(Sc))
    return Om, P, Sall
