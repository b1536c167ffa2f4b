"""The recovered multigrid hierarchy of a small family and the families the GPU tests of the preconditioner and of the solve drivers
run on (tests/test_gpu_multigrid.py, tests/test_gpu_solve_driver.py).

The hierarchy is RECOVERED from the device once per family: restriction, prolongation and every term of every sparse coarse level
are applied to identity columns through wae_debug_spmv (CSR kernels; products with 0 and 1 are exact, so this reads the stored
matrices bit for bit).  tests/test_gpu_multigrid.py holds the recovered matrices to the Galerkin identity and the cycle built from
them to tests/_mgref.vcycle_ref; what is built on top of them here rests on those tests."""
import numpy as np
import scipy.sparse as sp

import _mgref as M
from wae_amd.helmholtz import annulus
from wae_amd.helmholtz.bloch import bloch_family, seam_terms
from wae_amd.helmholtz.family import annulus_family

OPS = {"N": 0, "T": 1, "C": 2}
SENT = 3 + 7j
MASKS = {21: np.array([1, 0, 1], dtype=bool), 64: np.array([1, 0, 1, 1, 0, 0, 1, 1], dtype=bool)}
RATIOS = {}                                  # family -> largest device error in units of max(e64, TOL / 16), printed when a family is dropped


# ----------------------------------------------------------------------------------------------------
# the recovered hierarchy
# ----------------------------------------------------------------------------------------------------
def recover(fam, which, level, n_in, n_out, k=None):
    """the stored matrix of a level operator's term k (which = 0), a restriction (1) or a prolongation (2), read 256 columns at a time"""
    blocks = []
    ct = np.zeros((1, fam.T), dtype=np.complex128)
    if k is not None:
        ct[0, k] = 1.0
    for c0 in range(0, n_in, 256):
        w = min(256, n_in - c0)
        X = np.zeros((n_in, w), dtype=np.complex128)
        X[np.arange(c0, c0 + w), np.arange(w)] = 1.0
        if which == 2:
            Y = fam.debug_spmv(ct, X, mode=3, B=np.zeros((n_out, w), dtype=np.complex128), level=level, which=2, no_tiles=True)
        else:
            Y = fam.debug_spmv(ct, X, mode=0, level=level, which=which, no_tiles=True)
        blocks.append(sp.csc_matrix(Y))
    return sp.hstack(blocks).tocsr()


class Hier:
    def __init__(self, name, L, weights, nsweeps, zref, zs, distinct=64):
        """distinct: the 64 columns (right-hand sides and coefficient rows) are this many distinct ones, repeated -- the extended-precision
        reference of the 8 736-DoF family is evaluated on 16 columns; a column that took its neighbour's coefficients still differs"""
        self.name, self.L, self.fam = name, L, L.ensure_solver()
        fam = self.fam
        self.w = dict(zip(("w_pre", "w_post", "w_light"), weights))
        self.nsweeps = nsweeps
        xf = sorted((lv, ni, no) for w, lv, ni, no in fam.level_sizes() if w == 1)
        self.nl = len(xf) + 1                                        # levels, the dense one included
        self.n = [xf[0][1]] + [no for _, _, no in xf]
        T = fam.T
        self.Rm = [recover(fam, 1, l, self.n[l], self.n[l + 1]) for l in range(self.nl - 1)]
        self.Pm = [recover(fam, 2, l, self.n[l + 1], self.n[l]) for l in range(self.nl - 1)]
        self.terms = [[sp.csr_matrix(t.coeff).astype(np.complex128) for t in L.terms]]
        for l in range(1, self.nl - 1):
            self.terms.append([recover(fam, 0, l, self.n[l], self.n[l], k) for k in range(T)])
        Pr = [P.real.tocsr() for P in self.Pm]
        Rr = [Rm.real.tocsr() for Rm in self.Rm]
        self.transfers = list(zip(Pr, Rr))
        self.gal = {}                                                # (level, term) -> (R A P, |R||A||P|) of the level above
        for l in range(1, self.nl):
            for k in range(T):
                self.gal[(l, k)] = M.galerkin(Rr[l - 1], self.terms[l - 1][k], Pr[l - 1])
        self.levels = [M.Level(t) for t in self.terms] + [M.DenseLevel([self.gal[(self.nl - 1, k)][0] for k in range(T)])]
        # penalty rows, by the set-up's documented rule: |a_ii| > 1e8 x the median, at the reference coefficients
        dg = np.abs(sum(c * t.coeff.diagonal() for c, t in zip(L.coefficients(L.solver_ref), L.terms)))
        self.pen = dg > 1e8 * np.median(dg)
        # one system (zref) and one system per column (a line through zref)
        self.ct1 = np.array([L.coefficients(zref)])
        self.distinct, rep = distinct, 64 // distinct
        self.ct64 = np.tile(np.array([L.coefficients(z) for z in zs[::rep]]), (rep, 1))
        rng = np.random.default_rng(len(name) + 100 * nsweeps)
        self.rng = rng
        self.B = [np.tile(rng.standard_normal((n, distinct)) + 1j * rng.standard_normal((n, distinct)), (1, rep)) for n in self.n]
        d0 = np.abs(self.levels[0].diag(self.ct1, "N", 1, np.complex128))
        self.V = self.B[0].copy()                                    # (input of the fused entry: a Krylov vector, rows of one size)
        self.B[0] = self.B[0] * np.maximum(d0, 1.0)                  # right-hand sides of the size of the rows they meet
        self._ref = {}

    def groups(self, level):
        return (self.pen, ~self.pen) if level == 0 else (np.ones(self.n[level], dtype=bool),)

    def ct(self, percol, r=64):
        return self.ct64[:r] if percol else self.ct1

    def reference(self, level, op, percol, light, fused=False):
        """(reference in extended precision, e64 per column) of the 64-column case; narrower batches are its first columns"""
        key = (level, op, percol, light, fused)
        if key not in self._ref:
            out = []
            nd, ct = self.distinct, self.ct(percol, self.distinct)
            for dt in (M.LD, np.complex128):
                b = self.levels[0].apply(ct, op, self.V[:, :nd], dt) if fused else self.B[level][:, :nd]
                out.append(M.vcycle_ref(self.levels, self.transfers, b, ct, level=level, op=op, nsweeps=self.nsweeps, light=light, dtype=dt, **self.w))
            e64 = M.column_errors(out[1], out[0], self.groups(level))
            self._ref[key] = (np.tile(out[0], (1, 64 // nd)), np.tile(e64, 64 // nd))
        return self._ref[key]

    def check_cycle(self, level, op, percol, light, r, final_out=False, fused=False, masked=False):
        ref, e64 = self.reference(level, op, percol, light, fused)
        cm = MASKS[r] if masked else None
        Bin = (self.V if fused else self.B[level])[:, :r]
        Y0 = np.full((self.n[level], r), SENT)
        Y = self.fam.debug_vcycle(self.ct(percol, r), Bin, level=level, Y0=Y0, op=OPS[op], light=light, final_out=final_out, fused=fused, cmask=cm)
        act = np.ones(r, dtype=bool) if cm is None else np.repeat(cm, 8)[:r]
        what = f"{self.name} sweeps={self.nsweeps} level={level} op={op} percol={percol} light={light} r={r} final_out={final_out} fused={fused} masked={masked}"
        assert np.array_equal(Y[:, ~act], Y0[:, ~act]), what + ": a masked chunk was written"
        err = M.column_errors(Y[:, :r], ref[:, :r], self.groups(level))[act]
        unit = np.maximum(e64[:r][act], M.TOL / M.FACTOR)
        ratio = float(np.max(err / unit))
        RATIOS[self.name] = max(RATIOS.get(self.name, 0.0), ratio)
        print(f"cycle {what}: e64 {np.max(e64[:r][act]):.2e} device {np.max(err):.2e} ratio {ratio:.2f}")
        assert np.all(err <= M.budget(e64[:r][act])), f"{what}: device {np.max(err):.2e}, e64 {np.max(e64[:r][act]):.2e}, {ratio:.1f} units of 16 allowed"


Z_AB = 2 * np.pi * (430 + 15j)
Z_C = 2 * np.pi * (410 + 20j)
LINE = 2 * np.pi * np.linspace(-60, 60, 64) * (1 + 0.1j)



def family_a_operator(sweeps, **solver_opts):
    """the annulus "tiny" with the set-up options of family A, no hierarchy recovered (the child processes of the solve-driver tests)"""
    L, _ = annulus_family("tiny", tau=2e-4)
    L.solver_ref = 2 * np.pi * 500.0
    L.solver_opts = {"max_coarse": 16, "jacobi_weight": 0.7, "jacobi_weight_post": 0.9, "jacobi_weight_light": 0.5, "sweeps": sweeps}
    L.solver_opts.update(solver_opts)
    return L


def family_a(sweeps, distinct=64, **solver_opts):
    """max_coarse = 16 gives the annulus "tiny" its three levels (asserted in tests/test_gpu_multigrid.py); solver_opts: further
    options of the set-up (batch, restart) for the solve-driver tests"""
    return Hier("A", family_a_operator(sweeps, **solver_opts), (0.7, 0.9, 0.5), sweeps, Z_AB, Z_AB + LINE, distinct=distinct)


def family_c(distinct=64, **solver_opts):
    """the Bloch unit cell of tests/test_gpu_bloch.py: set up at b = 0, run at b = 5"""
    cell = annulus.build_unit_cell(grid=(4, 26, 7), DOS=12, tau=2e-4)
    L = bloch_family(cell)
    L.solver_ref = 2 * np.pi * 400.0
    L.solver_opts = {"shape_exclude": seam_terms(L), "max_coarse": 16}      # (the default, 128, leaves 728 -> 94 unknowns: no sparse coarse level)
    L.solver_opts.update(solver_opts)
    L.params["b"] = 0
    L.ensure_solver()                                                # the hierarchy of b = 0 ...
    L.params["b"] = 5                                                # ... serves b = 5: only coefficients change
    H = Hier("C", L, (0.8, 0.9, 0.5), 1, Z_C, Z_C + LINE, distinct=distinct)
    assert np.any(np.abs(H.ct1.imag) > 0) and len(L.terms) >= 11 and len(seam_terms(L)) > 0
    return H
