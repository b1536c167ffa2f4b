"""The forms of the prolongation kernels (kernels.hip prolong_add_kernel / prolong_tiles_kernel and their norm variants): out of
place, Y = X + P Xc with Y another multivector (the light cycle writes its result straight into a Krylov slot); in place, Y == X, the
same bits; with the column norms of Y from the same launch; and the norms alone, nothing written.  ONE launch at a time through
wae_debug_spmv (which = 2; B and Y the same array: in place) and wae_debug_prolong.

Families, as in tests/test_gpu_multigrid.py: the annulus "tiny" (1 152 DoF, max_coarse = 16: the CSR kernel) and "small" (8 736 DoF,
default options: the tile kernel from 8 columns on, the CSR kernel on request).  P of level 0 is recovered from the device as that
file recovers it (tests/_hier.recover: the CSR kernel on identity columns, exact), the reference is scipy's X + P Xc.

  results   tests/_tilecheck.assert_close: 1e-13 per column in the max-norm and element-wise of |X| + |P||Xc|;
  norms     |norm - numpy.linalg.norm(reference column)| within 16 x the distance between a float64 and a longdouble evaluation of the
            reference norm, measured here, floored at 1e-13, relative to the norm: the rule of tests/test_gpu_multigrid.py;
  masks     r in {8, 16, 19} with one 8-column chunk switched off: its columns of Y keep a sentinel, their norms are 0."""
import ctypes as C

import numpy as np
import pytest

from _hier import SENT, family_a_operator, recover
from _tilecheck import TOL, assert_close
from wae_amd import _lib
from wae_amd._lib import check, zptr
from wae_amd.helmholtz.family import annulus_family

pytestmark = pytest.mark.gpu

MASKS = {8: np.array([0], dtype=bool), 16: np.array([1, 0], dtype=bool), 19: np.array([1, 0, 1], dtype=bool)}
WIDTHS = (8, 16, 19)


class Fam:
    def __init__(self, name, L):
        self.name, self.L, self.fam = name, L, L.ensure_solver()
        _, _, self.nf, self.nc = next((w, lv, ni, no) for w, lv, ni, no in self.fam.level_sizes() if w == 1 and lv == 0)
        self.P = recover(self.fam, 2, 0, self.nc, self.nf).real.tocsr()
        assert self.P.shape == (self.nf, self.nc) and self.P.nnz > self.nc
        rng = np.random.default_rng(len(name))
        self.Xc = rng.standard_normal((self.nc, 19)) + 1j * rng.standard_normal((self.nc, 19))
        self.X = rng.standard_normal((self.nf, 19)) + 1j * rng.standard_normal((self.nf, 19))
        self.ref = self.X + self.P @ self.Xc
        self.bound = np.abs(self.X) + abs(self.P) @ np.abs(self.Xc)
        self.ct = np.zeros((1, self.fam.T), dtype=np.complex128)
        # norms of the reference columns in float64 and in extended precision: their distance is the unit of the norm budget
        ld = self.X.astype(np.clongdouble)
        Pc = self.P.tocoo()
        np.add.at(ld, Pc.row, Pc.data.astype(np.longdouble)[:, None] * self.Xc.astype(np.clongdouble)[Pc.col])
        a = np.abs(ld)
        self.norm_ld = np.sqrt((a * a).sum(axis=0))
        self.norm64 = np.linalg.norm(self.ref, axis=0)
        e64 = np.abs(self.norm64.astype(np.longdouble) - self.norm_ld) / self.norm_ld
        self.norm_budget = np.maximum(16 * e64.astype(np.float64), TOL)

    def cases(self):
        """(r, cmask, no_tiles)"""
        for r in WIDTHS:
            for cm in (None, MASKS[r]):
                for no_tiles in ((False, True) if self.name == "small" else (False,)):
                    yield r, cm, no_tiles

    def out_of_place(self, r, cm, no_tiles):
        return self.fam.debug_spmv(self.ct, self.Xc[:, :r], mode=3, B=self.X[:, :r], Y0=np.full((self.nf, r), SENT), level=0, which=2, cmask=cm,
                                   no_tiles=no_tiles)

    def in_place(self, r, cm, no_tiles):
        """wae_debug_spmv with B and Y the same array"""
        Xf = np.asfortranarray(self.Xc[:, :r])
        Y = np.asfortranarray(self.X[:, :r].copy())
        cmask = None if cm is None else (C.c_uint8 * ((r + 7) // 8))(*[1 if x else 0 for x in cm])
        nin, nout = C.c_int64(0), C.c_int64(0)
        check(_lib.lib().wae_debug_spmv(self.fam.handle, 2, 0, 3, zptr(self.ct), 1, zptr(Xf), zptr(Y), zptr(Y), None, r, 0, 0.0, cmask,
                                        1 if no_tiles else 0, C.byref(nin), C.byref(nout)))
        return Y


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def active(r, cm):
    return np.ones(r, dtype=bool) if cm is None else np.repeat(cm, 8)[:r]


@pytest.fixture(scope="module")
def tiny():
    F = Fam("tiny", family_a_operator(1))
    yield F
    F.L._drop_device()


@pytest.fixture(scope="module")
def small():
    L, _ = annulus_family("small", tau=2e-4)
    L.solver_ref = 2 * np.pi * 500.0
    F = Fam("small", L)
    yield F
    F.L._drop_device()


@pytest.mark.parametrize("fx", ["tiny", "small"])
def test_out_of_place_and_in_place(fx, request):
    F = request.getfixturevalue(fx)
    for r, cm, no_tiles in F.cases():
        what = f"{F.name} r={r} masked={cm is not None} no_tiles={no_tiles}"
        act = active(r, cm)
        on = np.nonzero(act)[0]
        Y = F.out_of_place(r, cm, no_tiles)
        assert_close(Y, F.ref[:, :r], F.bound[:, :r], what + " (out of place)", cols=on)
        assert np.all(Y[:, ~act] == SENT), what + ": a masked chunk of Y was written"
        Yi = F.in_place(r, cm, no_tiles)
        assert np.array_equal(bits(Yi[:, act]), bits(Y[:, act])), what + ": in place and out of place differ"
        assert np.array_equal(Yi[:, ~act], F.X[:, :r][:, ~act]), what + ": a masked chunk was written in place"


@pytest.mark.parametrize("fx", ["tiny", "small"])
def test_norms_from_the_prolongation(fx, request):
    F = request.getfixturevalue(fx)
    worst = 0.0
    for r, cm, no_tiles in F.cases():
        what = f"{F.name} r={r} masked={cm is not None} no_tiles={no_tiles}"
        act = active(r, cm)
        Y0 = np.full((F.nf, r), SENT)
        Y, nrm = F.fam.debug_prolong(F.Xc[:, :r], F.X[:, :r], Y0=Y0, cmask=cm, no_tiles=no_tiles)
        Yo = F.out_of_place(r, cm, no_tiles)
        assert np.array_equal(bits(Y), bits(Yo)), what + ": the result with norms is not the result without"
        rel = np.abs(nrm - F.norm64[:r]) / F.norm64[:r]
        print(f"norms {what}: largest error {np.max(rel[act], initial=0.0):.2e}, budget {np.min(F.norm_budget[:r]):.2e}")
        worst = max(worst, float(np.max(rel[act] / F.norm_budget[:r][act], initial=0.0)))
        assert np.all(rel[act] <= F.norm_budget[:r][act]), (what, float(np.max(rel[act])))
        assert np.all(nrm[~act] == 0), what + ": the norm of a masked column is not 0"
        Y2, nrm2 = F.fam.debug_prolong(F.Xc[:, :r], F.X[:, :r], Y0=Y0, cmask=cm, no_tiles=no_tiles)
        assert np.array_equal(nrm, nrm2) and np.array_equal(bits(Y), bits(Y2)), what + ": two runs differ"
        Yn, nrm_only = F.fam.debug_prolong(F.Xc[:, :r], F.X[:, :r], Y0=Y0, cmask=cm, no_tiles=no_tiles, norms_only=True)
        assert np.all(Yn == SENT), what + ": the norm-only form wrote to Y"
        assert np.array_equal(nrm_only, nrm), what + ": the norm-only form gives other norms"
    print(f"family {F.name}: largest norm error {worst:.2f} budgets")
