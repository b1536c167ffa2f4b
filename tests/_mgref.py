"""Plain reference of the multigrid preconditioner (tests/test_gpu_multigrid.py, include/waehip.h wae_debug_vcycle), written from
per-level matrices as the textbook recursion, in numpy's extended precision (clongdouble: 64-bit mantissa on x86-64) or, for the
measured float64 distance `e64` the device budget is built from, in plain complex128 with scipy products.  tests/test_mgref.py
checks every function against a second formulation where no GPU is.

The cycle, restated from its documented behaviour (include/waehip.h opts[2], [3], [10], [11]):

  * A level l < L holds the term matrices A_{l,k}; its operator for a column with coefficient row c is A_l(c) = sum_k c_k A_{l,k}
    (op = T: every A_{l,k} transposed; op = C: transposed and conjugated, c conjugated too).  One coefficient row serves every
    column, or every column has its own.  P_l prolongs from level l+1 to l, R_l restricts; both are real and the same for every op.
  * On a level l < L, for the right-hand side b:  x = w b / D  (D the diagonal of A_l(c), the first damped-Jacobi sweep from a zero
    guess); nsweeps - 1 more sweeps x <- x + w (b - A x) / D;  the residual b - A x is restricted, the coarser level is solved
    approximately by the same recursion, its result prolonged and added to x;  then the post-smoothing sweeps, with the weight w_post.
  * The full cycle smooths with w = w_pre before and with w_post after the coarse correction, nsweeps sweeps each, on every level.
    The light cycle (the projected phase of a contour integral, where a solve takes a handful of steps) smooths with w = w_light and
    does no post-smoothing at all, on the fine level and on the coarse ones.
  * The last level L is solved exactly: a dense solve with sum_k c_k G_k, G_k the Galerkin product R A_{L-1,k} P of the level above.
"""
import numpy as np
import scipy.sparse as sp

LD = np.clongdouble
EPS = float(np.finfo(np.float64).eps)
TOL = 1e-13                      # tests/_tilecheck.py: the floor of the device budget
FACTOR = 16.0                    # device budget = FACTOR * e64, floored at TOL


# ----------------------------------------------------------------------------------------------------
# sparse products in extended precision
# ----------------------------------------------------------------------------------------------------
def csr_matmat(A, X, dtype=LD, data=None, mag=True):
    """(A X, |A| |X|) for a scipy CSR matrix A and a dense X, accumulated in `dtype` row by row.  data: the values of A's pattern in
    `dtype`, in place of A.data; mag=False: the second result is not formed.  (X is handled as interleaved real columns: numpy's
    extended complex product is several times slower than the real one.)"""
    A = A.tocsr()
    X = np.asarray(X)
    X2 = np.ascontiguousarray(X.reshape(X.shape[0], -1).astype(dtype))
    real = np.longdouble if dtype == LD else np.float64
    r = X2.shape[1]
    out = np.zeros((A.shape[0], r), dtype=dtype)
    amag = np.zeros(out.shape if mag else (), dtype=real)
    if A.nnz and r:
        Xr, outr = X2.view(real), out.view(real)               # (n, 2 r): re, im, re, im, ...
        rows = np.nonzero(np.diff(A.indptr) > 0)[0]            # (reduceat returns an entry, not 0, for an empty segment)
        starts = A.indptr[:-1][rows]
        step = 2 * max(1, (1 << 21) // max(A.nnz, 1))           # real columns per pass: the nnz x columns products stay below 64 MB each
        vals = (A.data if data is None else data).astype(dtype)
        vr, vi = np.ascontiguousarray(vals.real)[:, None], np.ascontiguousarray(vals.imag)[:, None]
        cplx_a = bool(np.any(vi != 0))
        va = np.abs(vals)[:, None] if mag else None
        for c0 in range(0, 2 * r, step):
            G = Xr[A.indices, c0:c0 + step]
            prod = vr * G
            if cplx_a:                                           # (vr + i vi)(gr + i gi): the pairs swapped, the new real part negated
                Gs = G.reshape(G.shape[0], -1, 2)[:, :, ::-1] * np.array([-1.0, 1.0], dtype=real)
                prod += vi * Gs.reshape(G.shape)
            outr[rows, c0:c0 + step] = np.add.reduceat(prod, starts, axis=0)
            if mag:
                aG = np.abs(G.view(dtype)) if G.flags.c_contiguous else np.abs(np.ascontiguousarray(G).view(dtype))
                amag[rows, c0 // 2:(c0 + step) // 2] = np.add.reduceat(va * aG, starts, axis=0)
    return out.reshape(A.shape[:1] + X.shape[1:]), (amag.reshape(A.shape[:1] + X.shape[1:]) if mag else amag)


def _spgemm(rows, cols, vals, B, dtype):
    """(rows, cols, vals) of a sparse matrix times the scipy CSR matrix B, as coalesced triplets: every product a_ik b_kj is formed
    and the products of one entry are summed in `dtype`"""
    lens = np.diff(B.indptr)[cols]
    total = int(lens.sum())
    offs = np.arange(total) - np.repeat(np.cumsum(lens) - lens, lens)
    idx = np.repeat(B.indptr[cols], lens) + offs
    key = np.repeat(rows, lens).astype(np.int64) * B.shape[1] + B.indices[idx]
    prod = np.repeat(vals, lens) * B.data[idx].astype(dtype)
    order = np.argsort(key, kind="stable")
    key, prod = key[order], prod[order]
    starts = np.nonzero(np.r_[True, key[1:] != key[:-1]])[0] if total else np.zeros(0, dtype=np.int64)
    key = key[starts]
    return key // B.shape[1], key % B.shape[1], (np.add.reduceat(prod, starts) if total else prod)


def galerkin(R, A, P, dtype=LD):
    """(R A P, |R| |A| |P|) as dense arrays, accumulated in `dtype` over the sparse patterns"""
    out = []
    for f in (lambda m: m, abs):
        Rc = f(sp.csr_matrix(R)).tocoo()
        i, j, v = _spgemm(Rc.row, Rc.col, Rc.data.astype(dtype), f(sp.csr_matrix(A)).tocsr(), dtype)
        i, j, v = _spgemm(i, j, v, f(sp.csr_matrix(P)).tocsr(), dtype)
        G = np.zeros((R.shape[0], P.shape[1]), dtype=dtype)
        G[i, j] = v
        out.append(G)
    return out[0], np.abs(out[1])


def dense_solve(A, B):
    """A \\ B by Gaussian elimination with partial pivoting, in the precision of A (numpy.linalg has no extended precision)"""
    A = np.array(A)
    X = np.array(B, dtype=A.dtype)
    n = A.shape[0]
    for k in range(n):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        if p != k:
            A[[k, p]] = A[[p, k]]
            X[[k, p]] = X[[p, k]]
        f = A[k + 1:, k] / A[k, k]
        A[k + 1:, k:] -= f[:, None] * A[k, k:][None, :]
        X[k + 1:] -= f[:, None] * X[k][None, :]
    for k in range(n - 1, -1, -1):
        X[k] = (X[k] - A[k, k + 1:] @ X[k + 1:]) / A[k, k]
    return X


# ----------------------------------------------------------------------------------------------------
# levels
# ----------------------------------------------------------------------------------------------------
class Level:
    """the term matrices of one sparse level; products with sum_k c_k op(A_k), one coefficient row per column or one for all"""

    def __init__(self, terms):
        self.terms = [sp.csr_matrix(A).astype(np.complex128) for A in terms]
        self.n = self.terms[0].shape[0]
        self._ops = {"N": self.terms}
        self._asm = {}

    def mats(self, op):
        if op not in self._ops:
            self._ops[op] = [(A.T if op == "T" else A.conj().T).tocsr() for A in self.terms]
        return self._ops[op]

    @staticmethod
    def coeffs(c, op, r):
        c = np.asarray(c, dtype=np.complex128).reshape(-1, np.shape(c)[-1])
        if op == "C":
            c = c.conj()
        return c if c.shape[0] == r else np.repeat(c[:1], r, axis=0)

    def diag(self, c, op, r, dtype=LD):
        cj = self.coeffs(c, op, r).astype(dtype)
        return sum(A.diagonal().astype(dtype)[:, None] * cj[None, :, k] for k, A in enumerate(self.mats(op)))

    def assembled(self, crow, op, dtype):
        """sum_k c_k op(A_k) for ONE coefficient row (already conjugated for op = C): the union pattern as a scipy matrix and its
        values in `dtype` (scipy holds no extended precision)"""
        key = (op, dtype, crow.tobytes())
        if self._asm.get("key") != key:
            mats = [(ck, A.tocoo()) for ck, A in zip(crow, self.mats(op)) if ck != 0]
            keys = np.concatenate([A.row.astype(np.int64) * self.n + A.col for _, A in mats])
            vals = np.concatenate([dtype(ck) * A.data.astype(dtype) for ck, A in mats])
            order = np.argsort(keys, kind="stable")
            keys, vals = keys[order], vals[order]
            starts = np.nonzero(np.r_[True, keys[1:] != keys[:-1]])[0]
            keys, vals = keys[starts], np.add.reduceat(vals, starts)
            pat = sp.csr_matrix((np.ones(len(keys)), (keys // self.n, keys % self.n)), shape=(self.n, self.n))
            pat.sort_indices()                                       # (row-major order of the keys = CSR order of the pattern)
            self._asm = {"key": key, "pat": pat, "vals": vals}
        return self._asm["pat"], self._asm["vals"]

    def apply(self, c, op, X, dtype=LD):
        cj = self.coeffs(c, op, X.shape[1])
        if dtype == LD and np.all(cj == cj[:1]):                     # one system: one product with the assembled operator
            pat, vals = self.assembled(cj[0], op, dtype)
            return csr_matmat(pat, X, dtype, data=vals, mag=False)[0]
        out = np.zeros(X.shape, dtype=dtype)
        for k, A in enumerate(self.mats(op)):
            if not np.any(cj[:, k] != 0):
                continue
            AX = csr_matmat(A, X, dtype, mag=False)[0] if dtype == LD else A @ X
            out = out + AX * cj[None, :, k].astype(dtype)
        return out


class DenseLevel:
    """the last level: dense term matrices G_k (the Galerkin products of the level above), solved exactly"""

    def __init__(self, terms):
        self.terms = [np.asarray(G) for G in terms]
        self.n = self.terms[0].shape[0]

    def matrix(self, crow, op, dtype=LD):
        """sum_k c_k op(G_k) for ONE coefficient row (already conjugated for op = C)"""
        return sum(dtype(ck) * (G if op == "N" else (G.T if op == "T" else G.conj().T)).astype(dtype) for ck, G in zip(crow, self.terms) if ck != 0)

    def solve(self, c, op, B, dtype=LD):
        cj = Level.coeffs(c, op, B.shape[1])
        out = np.zeros(B.shape, dtype=dtype)
        same = np.all(cj == cj[:1])
        for j in ([0] if same else range(B.shape[1])):
            A = self.matrix(cj[j], op, dtype)
            cols = slice(None) if same else slice(j, j + 1)
            out[:, cols] = dense_solve(A, B[:, cols].astype(dtype)) if dtype == LD else np.linalg.solve(A, B[:, cols])
        return out


def dense_level(R, terms, P, dtype=LD):
    """the DenseLevel below a sparse level with term matrices `terms`"""
    return DenseLevel([galerkin(R, A, P, dtype)[0] for A in terms])


# ----------------------------------------------------------------------------------------------------
# the cycle
# ----------------------------------------------------------------------------------------------------
def default_post(level, light, nsweeps):
    """post-smoothing sweeps of a level: none anywhere in the light cycle, nsweeps on every level of the full cycle"""
    return 0 if light else nsweeps


def vcycle_ref(levels, transfers, b, coeffs, level=0, op="N", w_pre=0.8, w_post=0.9, w_light=0.5, nsweeps=1, light=False,
               post=default_post, dtype=LD, mutate=()):
    """M_level^-1 b.  levels: Level objects, the last one a DenseLevel; transfers[l] = (P_l, R_l) scipy matrices; coeffs: (1, T) or
    (r, T).  `mutate` names deliberate defects (tests/test_mgref.py: what a comparison with this reference must be able to see):
    'restrict_b' restricts b instead of the residual; 'level1_unconjugated' runs level 1 with op T under op C; 'level1_neighbour'
    gives column j of level 1 the coefficient row of column j + 1; 'early_return' returns the iterate before the last sweep."""
    L = len(levels) - 1
    b = np.asarray(b)
    r = b.shape[1]
    top = level

    def mul(P, X):
        return csr_matmat(P, X, dtype, mag=False)[0] if dtype == LD else P @ X

    def cyc(l, b):
        c, o = coeffs, op
        if l == 1 and "level1_neighbour" in mutate:
            c = np.roll(Level.coeffs(coeffs, "N", r), -1, axis=0)
        if l == 1 and "level1_unconjugated" in mutate and op == "C":
            o = "T"
        if l == L:
            return levels[l].solve(c, o, b, dtype)
        A = levels[l]
        D = A.diag(c, o, r, dtype)
        w = dtype(w_light if light else w_pre)
        npost = post(l, light, nsweeps)
        x = w * b / D
        prev = x
        for s in range(1, nsweeps):
            prev = x
            x = x + w * (b - A.apply(c, o, x, dtype)) / D
        if l == top and npost == 0 and "early_return" in mutate:
            x = prev
        res = b if "restrict_b" in mutate else b - A.apply(c, o, x, dtype)
        P, R = transfers[l]
        x = x + mul(P, cyc(l + 1, mul(R, res)))
        for s in range(npost):
            prev = x
            x = x + dtype(w_post) * (b - A.apply(c, o, x, dtype)) / D
        if l == top and npost > 0 and "early_return" in mutate:
            x = prev
        return x

    return cyc(level, b.astype(dtype))


# ----------------------------------------------------------------------------------------------------
# error measure and budget of the device comparisons
# ----------------------------------------------------------------------------------------------------
def column_errors(got, ref, groups):
    """per column: the largest over the row groups of max|got - ref| / max|ref| within the group (the penalty rows' values are ~1e-15
    of the others': one max-norm over all rows would not see them).  groups: boolean row masks; empty groups are skipped."""
    out = np.zeros(ref.shape[1])
    for g in groups:
        if not np.any(g):
            continue
        err = np.max(np.abs(got[g] - ref[g]), axis=0).astype(np.float64)
        scl = np.max(np.abs(ref[g]), axis=0).astype(np.float64)
        out = np.maximum(out, err / np.maximum(scl, 1e-300))
    return out


def budget(e64):
    """what the device may differ from the extended-precision reference by, per column: FACTOR x the distance of the float64
    evaluation of the same reference, floored at TOL"""
    return np.maximum(FACTOR * np.asarray(e64), TOL)
