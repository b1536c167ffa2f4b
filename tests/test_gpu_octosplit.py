"""GPU tests (-m gpu) of the uniform mesh refinement on the device -- wae_octosplit, _info, _get, _prolong, _free through
helmholtz/refine.py -- against tests/_octoref.py (pinned by tests/test_octoref.py), and of the chain "coarse solve -> refine -> carry the
eigenpair over -> re-solve" on the tutorial Rijke tube.

Tolerances: the refinement and the prolongation are compared with array_equal (the device and the reference round every operation alike);
assembled values within 1e-13 * max|entry| of the oracle's (the project's assembly tolerance); the eigenvalue 1e-10 relative (the project's
bound for G1 and G5)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sp

import _octoref as O
from oracle import fixtures as F
from oracle import helmholtz_p1 as OH
from oracle import solvers as OS
from wae_amd import _lib
from wae_amd.helmholtz import RefinedMesh, octosplit
from wae_amd.helmholtz.assemble import assemble_p1, assemble_p1_boundary, assemble_p1_flame
from wae_amd.helmholtz.family import helmholtz_family
from wae_amd.nlevp import householder

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIELDS = ("points", "tets", "tris", "parents", "tet_labels", "tri_labels")


@functools.lru_cache(maxsize=None)
def reference(name):
    return O.refine(*O.mesh(name), levels=2)


@functools.lru_cache(maxsize=None)
def refined(name):
    return octosplit(*O.mesh(name), levels=2)


def same_level(R, l, ref, what):
    for f in FIELDS:
        a, b = getattr(R, f)[l], getattr(ref, f)
        assert a.shape == b.shape and a.dtype == b.dtype, (what, f, a.shape, b.shape, a.dtype, b.dtype)
        assert np.array_equal(a, b), (what, f, int(np.sum(a != b)))


def flame_inputs():
    fl = np.load(os.path.join(GOLDEN, "rijke_flame.npz"))
    return fl["flame_tets"], int(fl["ref_tet"]), fl["x_ref"], fl["n_ref"], float(fl["nglobal_scaled"]), float(fl["volume"])


# ---- 1. equality with the reference -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", O.MESHES)
def test_levels_equal_the_reference(name):
    H = reference(name)
    R1 = octosplit(*O.mesh(name), levels=1)
    assert isinstance(R1, RefinedMesh) and R1.levels == 1 and len(R1.points) == 2 and R1.parents[0] is None and R1.tet_labels[0] is None
    same_level(R1, 1, H[1], f"{name} levels=1")
    R2 = refined(name)
    for f, g in (("points", "points"), ("tets", "tets"), ("tris", "tris")):
        assert np.array_equal(getattr(R2, f)[0], getattr(H[0], g))                     # level 0 is the input
    same_level(R2, 1, H[1], f"{name} levels=2, level 1")
    same_level(R2, 2, H[2], f"{name} levels=2, level 2")
    # one call with levels=2 equals two calls with levels=1
    Rb = octosplit(R1.points[1], R1.tets[1], R1.tris[1], levels=1)
    for f in FIELDS:
        assert np.array_equal(getattr(Rb, f)[1], getattr(R2, f)[2]), f
    print(f"{name}: points {[len(p) for p in R2.points]}, tetrahedra {[len(t) for t in R2.tets]}, triangles {[len(t) for t in R2.tris]}")


def test_without_triangles_and_the_counts_of_the_rijke_tube():
    pts, tets, _ = O.mesh("cube")
    R = octosplit(pts, tets, levels=1)
    assert R.tris[0].shape == (0, 3) and R.tris[1].shape == (0, 3) and R.tri_labels[1].shape == (0, 4)
    assert np.array_equal(R.tets[1], reference("cube")[1].tets)
    R = refined("rijke")
    assert [len(p) for p in R.points] == [1006, 6172, 42507] and [len(t) for t in R.tets] == [3380, 27040, 216320]


# ---- 2. prolongation -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["two", "sheared", "rijke"])
def test_prolongation_equals_the_reference(name):
    H, R = reference(name), refined(name)
    rng = np.random.default_rng(5)
    for frm, to in ((0, 1), (1, 2), (0, 2)):
        n = len(H[frm].points)
        for ncols in (1, 3, 8):
            X = rng.standard_normal((n, ncols)) + 1j * rng.standard_normal((n, ncols))
            Y = R.prolong(X, frm, to)
            assert Y.shape == (len(H[to].points), ncols) and Y.dtype == np.complex128
            assert np.array_equal(Y, O.prolong(H, X, frm, to)), (frm, to, ncols)
        x = rng.standard_normal(n)                                                     # a real field, one-dimensional
        y = R.prolong(x, frm, to)
        assert y.shape == (len(H[to].points),) and y.dtype == np.float64 and np.array_equal(y, O.prolong(H, x, frm, to))
        z = R.prolong(x + 2j * x, frm, to)
        assert z.ndim == 1 and np.array_equal(z, O.prolong(H, x + 2j * x, frm, to))
    assert np.array_equal(R.prolong(H[0].points[:, :2]), O.prolong(H, H[0].points[:, :2]))      # defaults: level 0 to the last
    assert np.array_equal(R.prolong(H[0].points[:, 0], to_level=-2), O.prolong(H, H[0].points[:, 0], 0, 1))


# ---- 3. carriers -----------------------------------------------------------------------------------------------------------------------
def test_fields_domains_and_the_reference_tetrahedron_are_carried():
    H, R = reference("rijke"), refined("rijke")
    z = np.load(os.path.join(GOLDEN, "rijke_mesh.npz"))
    flame, ref_tet, x_ref, _, _, vol = flame_inputs()
    for to in (1, 2):
        assert np.array_equal(R.tet_field(z["c_tet"], to), O.carry_field(H, z["c_tet"], "tet", to))
        assert np.array_equal(R.tri_field(z["outlet_c"], to), O.carry_field(H, z["outlet_c"], "tri", to))
        fl = R.tet_domain(flame, to)
        assert np.array_equal(fl, O.carry_domain(H, flame, "tet", to)) and np.all(np.diff(fl) > 0) and len(fl) == len(flame) * 8 ** to
        assert np.array_equal(R.tri_domain([3, 0, 7], to), O.carry_domain(H, [3, 0, 7], "tri", to))
        v = O.volumes(R.points[to], R.tets[to][fl]).sum()
        print(f"flame volume at level {to}: {v:.17g}, level 0: {vol:.17g}, relative difference {abs(v - vol) / vol:.2e}")
        assert abs(v - vol) <= 1e-13 * vol
        r = R.reference_tet(ref_tet, x_ref, to)
        assert r == O.first_containing(H[to].points, H[to].tets, x_ref)
    ids = np.arange(len(R.tets[0]))
    assert np.array_equal(R.tet_field(ids, 1)[R.tet_labels[1]], np.repeat(ids[:, None], 8, axis=1))
    with pytest.raises(ValueError):
        R.tet_field(z["c_tet"][:-1])
    with pytest.raises(ValueError):
        R.tet_domain([len(R.tets[0])])


# ---- 4. error returns ---------------------------------------------------------------------------------------------------------------------
def test_errors_are_reported_and_the_next_call_works():
    pts, tets, tris = O.mesh("cube")
    good = reference("cube")[1]

    def works():
        R = octosplit(pts, tets, tris)
        assert np.array_equal(R.tets[1], good.tets) and np.array_equal(R.tris[1], good.tris)

    with pytest.raises(_lib.WaeError):
        octosplit(pts, tets + len(pts), tris)                                          # an index outside the points
    works()
    with pytest.raises(_lib.WaeError):
        octosplit(pts, tets, np.array([[0, 1, len(pts)]], dtype=np.int32))
    works()
    with pytest.raises(_lib.WaeError):
        octosplit(pts, np.vstack([tets, tets[:1]]), tris)                               # a tetrahedron listed twice
    works()
    with pytest.raises(_lib.WaeError):
        octosplit(pts, tets, np.vstack([tris, tris[2:3, ::-1]]))                        # a triangle listed twice, its points reversed
    works()
    with pytest.raises(_lib.WaeError):
        octosplit(pts, tets, np.array([[0, 1, 26]], dtype=np.int32))                    # (0, 1) is an edge, (0, 26) and (1, 26) are not
    works()
    # levels = 0: helmholtz/refine.py refuses it before the library is called, so the library is asked directly
    L = _lib.lib()
    p, t = np.ascontiguousarray(pts), np.ascontiguousarray(tets, dtype=np.int32)
    h = C.c_void_p()
    code = L.wae_octosplit(0, len(p), p.ctypes.data_as(C.POINTER(C.c_double)), len(t), t.ctypes.data_as(C.POINTER(C.c_int32)), 0, None, 0, C.byref(h))
    assert code == _lib.WAE_ERR_INVALID and not h.value
    with pytest.raises(_lib.WaeError):
        _lib.check(code)
    works()
    R = octosplit(pts, tets, tris)
    x = np.zeros(len(pts), dtype=np.complex128)
    y = np.zeros(len(R.points[1]), dtype=np.complex128)
    assert L.wae_octosplit_prolong(R._h, 1, 1, 1, _lib.zptr(x), _lib.zptr(y)) == _lib.WAE_ERR_INVALID
    assert L.wae_octosplit_prolong(R._h, 0, 2, 1, _lib.zptr(x), _lib.zptr(y)) == _lib.WAE_ERR_INVALID
    assert L.wae_octosplit_info(R._h, 2, None, None, None) == _lib.WAE_ERR_INVALID
    lab = np.zeros(8 * len(tets), dtype=np.int32)
    assert L.wae_octosplit_get(R._h, 0, None, None, None, None, lab.ctypes.data_as(C.POINTER(C.c_int32)), None) == _lib.WAE_ERR_INVALID
    works()


# ---- 5. end to end on the Rijke tube, level 1 (d = 6 172) -------------------------------------------------------------------------------------
def oracle_family_on(level, c_tet, flame, x_ref, n_ref, nglobal_scaled, n=0.01, tau=0.001):
    """the oracle's `discretize` (order=:lin) on a hand-built Mesh of the reference's refined arrays, descriptor as the tutorial's"""
    m = OH.Mesh()
    m.points = level.points
    m.tetrahedra = level.tets.astype(np.int64)
    m.triangles = level.tris.astype(np.int64)
    m.domains = {"Interior": {"dimension": 3, "simplices": list(range(len(level.tets)))},
                 "Outlet": {"dimension": 2, "simplices": list(range(len(level.tris)))},
                 "Flame": {"dimension": 3, "simplices": [int(i) for i in flame]}}
    # nlocal = (gamma - 1) / rho * nglobal / V: gamma = 2, rho = 1 pass nglobal_scaled through unchanged
    dscrp = {"Interior": ("interior", ()), "Outlet": ("admittance", ("Y", 1e15)),
             "Flame": ("flame", (2.0, 1.0, nglobal_scaled, list(x_ref), list(n_ref), "n", "τ", n, tau))}
    return OH.discretize_p1(m, dscrp, np.asarray(c_tet, dtype=float))


def test_rijke_tube_refined_once_end_to_end():
    H, R = reference("rijke"), refined("rijke")
    z = np.load(os.path.join(GOLDEN, "rijke_mesh.npz"))
    flame, ref_tet, x_ref, n_ref, ngs, _ = flame_inputs()
    # the coarse eigenpair: the device solve of the golden family at G1
    w_G1 = complex(*F.golden()["G1"]["omega"])
    L0 = helmholtz_family(F.rijke_terms(), n=0.01, tau=0.001)
    L0.solver_ref = 340 * 2 * np.pi
    sol0, _, flag0 = householder(L0, 340 * 2 * np.pi, maxiter=20, tol=1e-11)
    assert flag0 in (0, 1) and abs(sol0.params["ω"] - w_G1) < 1e-10 * abs(w_G1)
    L0._drop_device()
    # assembly from the refined arrays and the carried data, on the device
    pts, tets, tris = R.points[1], R.tets[1], R.tris[1]
    c1, oc1, fl1, ref1 = R.tet_field(z["c_tet"], 1), R.tri_field(z["outlet_c"], 1), R.tet_domain(flame, 1), R.reference_tet(ref_tet, x_ref, 1)
    M, K = assemble_p1(pts, tets, c1)
    Cm = assemble_p1_boundary(pts, tris, oc1)
    Q, _ = assemble_p1_flame(pts, tets, fl1, ref1, n_ref, ngs)
    Lo = oracle_family_on(H[1], O.carry_field(H, z["c_tet"], "tet", 1), O.carry_domain(H, flame, "tet", 1), x_ref, n_ref, ngs)
    assert Lo.size() == 6172
    for A, name in ((M, "M"), (K, "K"), (Cm, "C"), (Q, "Q")):
        B = next(t.coeff for t in Lo.terms if t.operator == name)
        A, B = sp.csr_matrix(A), sp.csr_matrix(B)
        A.sort_indices(); B.sort_indices()
        assert np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices), name
        err, scale = np.max(np.abs(A.data - B.data)), np.max(np.abs(B.data))
        print(f"{name}: nnz {A.nnz}, max|diff| = {err:.3e} = {err / scale:.3e} * max|entry|")
        assert err <= 1e-13 * scale, name
    # re-solve from the prolonged pair
    L1 = helmholtz_family({"M": M, "K": K, "C": Cm, "Q": Q}, n=0.01, tau=0.001)
    L1.solver_ref = 340 * 2 * np.pi
    sol1, n1, flag1 = householder(L1, w_G1, v0=R.prolong(sol0.v, 0, 1), v0_adj=R.prolong(sol0.v_adj, 0, 1), maxiter=20, tol=1e-11)
    L1._drop_device()
    solo, no, flago = OS.inveriter(Lo, w_G1, maxiter=40, tol=1e-9)
    w1, wo = sol1.params["ω"], solo.params["ω"]
    print(f"refined Rijke tube: device householder {w1:.12f} in {n1} steps (flag {flag1}), oracle inveriter {wo:.12f} in {no} steps (flag {flago}), "
          f"relative difference {abs(w1 - wo) / abs(wo):.2e}; tutorial mesh {w_G1:.12f}")
    assert flag1 in (0, 1) and no < 40
    assert abs(w1 - wo) < 1e-10 * abs(wo)
    assert abs(w1 - w_G1) < 1e-2 * abs(w_G1)              # the same mode as on the tutorial mesh: its neighbours are hundreds of Hz away
