"""GPU tests (-m gpu) of the device assembly with a NODAL speed of sound -- wae_p1_assemble_cpoint, wae_p1_assemble_boundary_cpoint,
wae_p2_assemble_cpoint, wae_p2_assemble_boundary_cpoint through the c_point= keyword of helmholtz/assemble.py -- against
tests/_nodalref.py (pinned by tests/test_nodal_ref.py), and of the P2 Rijke family built on the nodal K and C.

Tolerances: assembled values within 1e-13 * max|entry| of the reference (the assembly tolerance of tests/test_gpu_p2.py); symmetry
|a_ij - a_ji| <= 1e-14 * min(s_i, s_j), s_i the largest off-diagonal magnitude of row i (the criterion of wae_family_create_opts with
the opts[0] the Helmholtz wrappers pass); analytic sums 1e-12; fused SpMV-sum 1e-13, linear solve 1e-8, mslp eigenvalue 1e-10
relative, as the P2 family tests of tests/test_gpu_p2.py."""
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import _nodalref as N
import _p2ref as R
from oracle import solvers as OS
from oracle.nlevp import LinearOperatorFamily as OracleFamily, Term as OTerm, exp_delay as o_exp_delay, pow1 as o_pow1, pow2 as o_pow2
from wae_amd import _lib
from wae_amd.helmholtz.assemble import (assemble_p1, assemble_p1_boundary, assemble_p2, assemble_p2_boundary, assemble_p2_flame,
                                        speed_of_sound_kind)
from wae_amd.helmholtz.family import helmholtz_family
from wae_amd.nlevp import mslp

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RNG = np.random.default_rng(5)
SHAPES = ["one", "two", "cube", "rijke"]
CASES = [(name, order) for name in SHAPES for order in (1, 2)]


@functools.lru_cache(maxsize=None)
def mesh(name):
    """(points, tets, tris, c_tet, c_point): the meshes of tests/test_gpu_p2.py and a nodal field on each"""
    rng = np.random.default_rng(11)
    if name == "one":
        pts = np.array([[0.0, 0.0, 0.0], [1.0, 0.1, 0.0], [0.2, 0.9, 0.1], [0.1, 0.2, 0.8]])
        return pts, np.array([[0, 1, 2, 3]], dtype=np.int32), np.array([[0, 1, 2], [3, 1, 0]], dtype=np.int32), None, rng.uniform(0.5, 2.0, 4)
    if name == "two":                  # two tetrahedra on the face (3, 1, 4), listed so that one has det J < 0; points not in ascending order
        pts = np.array([[0.1, 0.2, 1.1], [1.0, 0.0, 0.1], [0.3, 0.1, -0.9], [0.0, 0.0, 0.0], [0.1, 1.2, 0.0]])
        tets = np.array([[3, 1, 4, 0], [3, 1, 4, 2]], dtype=np.int32)
        dets = [np.linalg.det((pts[t[:3]] - pts[t[3]]).T) for t in tets]
        assert dets[0] * dets[1] < 0
        return pts, tets, np.array([[4, 1, 0], [2, 3, 1]], dtype=np.int32), np.array([1.5, 0.5]), rng.uniform(0.5, 2.0, 5)
    if name == "cube":
        pts, tets, top = R.kuhn_cube(2)
        return pts, tets, top, None, 1.0 + pts[:, 0]
    z = np.load(os.path.join(GOLDEN, "rijke_mesh.npz"))
    pts = z["points"]
    lo, hi = np.unique(z["c_tet"])                                    # the cold and the hot gas of the fixture
    s = (pts[:, 2] - pts[:, 2].min()) / (pts[:, 2].max() - pts[:, 2].min())
    return pts, z["tetrahedra"], z["outlet_triangles"], z["c_tet"], lo + (hi - lo) * s * s * (3.0 - 2.0 * s)


@functools.lru_cache(maxsize=None)
def reference(name, order):
    pts, tets, tris, _, cp = mesh(name)
    return {"K": N.stiffness(pts, tets, cp, order), "C": N.boundary(pts, tets, tris, cp, order)}


@functools.lru_cache(maxsize=None)
def device(name, order):
    """(M, K, C) of the nodal entries"""
    pts, tets, tris, _, cp = mesh(name)
    if order == 1:
        return assemble_p1(pts, tets, c_point=cp) + (assemble_p1_boundary(pts, tris, c_point=cp),)
    return assemble_p2(pts, tets, c_point=cp) + (assemble_p2_boundary(pts, tets, tris, c_point=cp),)


def same_pattern(A, B):
    return A.shape == B.shape and np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices)


def close(A, B, what):
    err, scale = np.max(np.abs(A.data - B.data)), np.max(np.abs(B.data))
    print(f"{what}: max|diff| = {err:.3e} = {err / scale:.3e} * max|entry|")
    return err <= 1e-13 * scale


def relerr(a, b):
    return np.max(np.abs(a - b)) / np.max(np.abs(b))


# ---- 1. K and C against the reference ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,order", CASES)
def test_stiffness_and_boundary_match_the_reference(name, order):
    pts, tets, tris, c_tet, cp = mesh(name)
    M, K, Cm = device(name, order)
    ref = reference(name, order)
    assert same_pattern(K, ref["K"]) and same_pattern(M, K) and same_pattern(Cm, ref["C"])
    assert np.all(K.data.imag == 0) and np.all(Cm.data.real == 0)
    ok_k, ok_c = close(K, ref["K"], f"{name} P{order} K"), close(Cm, ref["C"], f"{name} P{order} C")
    assert ok_k and ok_c
    M0 = (assemble_p1 if order == 1 else assemble_p2)(pts, tets, c_tet)[0]                    # M does not depend on c: the per-simplex entry's bits
    assert same_pattern(M, M0) and np.array_equal(M.data, M0.data)
    if order == 1:
        M2, K2 = assemble_p1(pts, tets, c_point=cp)
        C2 = assemble_p1_boundary(pts, tris, c_point=cp)
    else:
        M2, K2 = assemble_p2(pts, tets, c_point=cp)
        C2 = assemble_p2_boundary(pts, tets, tris, c_point=cp)
    assert same_pattern(K2, K) and same_pattern(C2, Cm)
    assert np.array_equal(M2.data, M.data) and np.array_equal(K2.data, K.data) and np.array_equal(C2.data, Cm.data)     # deterministic: same bits


# ---- 2. symmetry ---------------------------------------------------------------------------------------------------------------------
def asymmetry(A):
    """max over the stored entries of |a_ij - a_ji| / min(s_i, s_j), s_i = the largest off-diagonal magnitude of row i"""
    A = sp.csr_matrix(A)
    off = abs(A - sp.diags(A.diagonal())).tocsr()
    s = np.asarray(off.max(axis=1).todense()).ravel()
    D = abs(A - A.T).tocoo()
    keep = D.row != D.col
    if not keep.any():
        return 0.0
    return float(np.max(D.data[keep] / np.minimum(s[D.row[keep]], s[D.col[keep]])))


@pytest.mark.parametrize("name,order", CASES)
def test_stiffness_and_boundary_are_symmetric(name, order):
    _, K, Cm = device(name, order)
    K, b = K.real.tocsr(), (1j * Cm).real.tocsr()
    for what, A in (("K", K), ("b", b)):
        assert same_pattern(A, A.T.tocsr())
        r = asymmetry(A)
        print(f"{name} P{order} {what}: max |a_ij - a_ji| / min(s_i, s_j) = {r:.3e}")
        if name == "one":
            assert np.array_equal(A.toarray(), A.toarray().T)                                  # the local matrix itself: bit for bit
        else:
            assert r <= 1e-14


# ---- 3. the feature is not a relabelling ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [1, 2])
def test_nodal_differs_from_centroid_values_and_integrates_polynomials_exactly(order):
    """c = 1 + x on the unit cube (tests/test_nodal_ref.py): u = x gives -7/3, u = x^2 (P2) -62/15, K 1 = 0; top face: 1' b 1 = 3/2,
    u = x (P2) gives 7/12.  The per-tetrahedron K from the centroid values of c is another discretisation."""
    pts, tets, top, _, cp = mesh("cube")
    _, K, Cm = device("cube", order)
    K, b = K.real.tocsr(), (1j * Cm).real.tocsr()
    Kc = (assemble_p1 if order == 1 else assemble_p2)(pts, tets, cp[tets].mean(axis=1))[1].real
    assert same_pattern(K, Kc)
    d = np.max(np.abs(K.data - Kc.data)) / np.max(np.abs(K.data))
    print(f"P{order}: max|K_nodal - K_centroid| = {d:.3e} * max|entry|")
    assert d > 1e-3
    x = N.dof_points(pts, tets, order)[:, 0]
    one = np.ones(K.shape[0])
    sums = {"x'Kx": (x @ (K @ x), -7 / 3), "1'b1": (one @ (b @ one), 3 / 2)}
    if order == 2:
        sums["x2'Kx2"] = ((x * x) @ (K @ (x * x)), -62 / 15)
        sums["x'bx"] = (x @ (b @ x), 7 / 12)
    for what, (got, want) in sums.items():
        print(f"P{order} {what} = {got!r}, exact {want!r}")
    for what, (got, want) in sums.items():
        assert abs(got - want) <= 1e-12 * abs(want), what
    assert np.max(np.abs(K @ one)) <= 1e-12 * np.max(np.abs(K.data))


# ---- 4. errors -----------------------------------------------------------------------------------------------------------------------
def entries():
    pts, tets, top, _, cp = mesh("cube")
    return [lambda c, t=tets, **kw: assemble_p1(pts, t, c_point=c, **kw), lambda c, t=top, **kw: assemble_p1_boundary(pts, t, c_point=c, **kw),
            lambda c, t=tets, **kw: assemble_p2(pts, t, c_point=c, **kw), lambda c, t=top, **kw: assemble_p2_boundary(pts, tets, t, c_point=c, **kw)]


def test_bad_arguments_are_refused():
    pts, tets, top, _, cp = mesh("cube")
    bad = cp.copy(); bad[7] = np.nan
    inf = cp.copy(); inf[0] = np.inf
    for k, f in enumerate(entries()):
        for c in (bad, inf):
            with pytest.raises((_lib.WaeError, ValueError)):
                f(c)
        for c in (cp[:-1], np.append(cp, 1.0), np.ones(len(tets))):
            with pytest.raises((_lib.WaeError, ValueError)):
                f(c)
        with pytest.raises((_lib.WaeError, ValueError)):
            f(cp, **({"c_tri": np.ones(len(top))} if k % 2 else {"c_tet": np.ones(len(tets))}))
        with pytest.raises((_lib.WaeError, ValueError)):
            f(cp, t=(top if k % 2 else tets) + len(pts))
        f(cp)                                                           # and the good call still works after the refusals
    # the C entries themselves: a missing c_point is WAE_ERR_INVALID
    import ctypes as C
    L = _lib.lib()
    h = C.c_void_p()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    p64, t32 = np.ascontiguousarray(pts, dtype=np.float64), np.ascontiguousarray(tets, dtype=np.int32)
    for entry in (L.wae_p1_assemble_cpoint, L.wae_p2_assemble_cpoint):
        assert entry(0, len(p64), p64.ctypes.data_as(dp), len(t32), t32.ctypes.data_as(ip), None, C.byref(h)) == _lib.WAE_ERR_INVALID
        assert not h.value


# ---- 5. dispatch ---------------------------------------------------------------------------------------------------------------------
def test_speed_of_sound_kind():
    assert speed_of_sound_kind(np.ones(48), 27, 48) == "tet"
    assert speed_of_sound_kind(np.ones(27), 27, 48) == "point"
    assert speed_of_sound_kind(np.ones(5), 5, 5) == "tet"                # the tetrahedron count is tested first
    for n in (0, 26, 49):
        with pytest.raises(ValueError):
            speed_of_sound_kind(np.ones(n), 27, 48)


# ---- 6. the P2 Rijke family on the nodal K and C -------------------------------------------------------------------------------------
def oracle_family(t, n, tau, Y=1e15):
    """oracle/fixtures.py rijke_family on the given terms"""
    L = OracleFamily(["ω", "λ"], [0.0, complex(np.inf, 0)])
    L.push(OTerm(sp.csc_matrix(t["M"]), (o_pow2,), (("ω",),), "ω^2", "M"))
    L.push(OTerm(sp.csc_matrix(t["K"]), (), (), "", "K"))
    L.params["Y"] = complex(Y)
    L.push(OTerm(sp.csc_matrix(t["C"]), (o_pow1, o_pow1), (("ω",), ("Y",)), "ω*Y", "C"))
    L.params["n"] = complex(n)
    L.params["τ"] = complex(tau)
    L.push(OTerm(sp.csc_matrix(t["Q"]), (o_pow1, o_exp_delay), (("n",), ("ω", "τ")), "n*exp(-iωτ)", "Q"))
    L.push(OTerm(sp.csc_matrix(-t["M"]), (o_pow1,), (("λ",),), "-λ", "__aux__"))
    return L


@pytest.fixture(scope="module")
def nodal_rijke():
    pts, tets, tris, _, _ = mesh("rijke")
    fl = np.load(os.path.join(GOLDEN, "rijke_flame.npz"))
    M, K, Cm = device("rijke", 2)
    Q = assemble_p2_flame(pts, tets, fl["flame_tets"], int(fl["ref_tet"]), np.array([0.0, 0.0, -0.00101]), fl["n_ref"], float(fl["nglobal_scaled"]))[0]
    t = {"M": M, "K": K, "C": Cm, "Q": Q}
    Lp = helmholtz_family(t, n=1.0, tau=0.001)
    Lp.solver_ref = 340 * 2 * np.pi
    yield oracle_family(t, 1.0, 0.001), Lp
    Lp._drop_device()


def test_nodal_family_spmv_sum(nodal_rijke):
    Lo, Lp = nodal_rijke
    d = Lo.size()
    X = RNG.standard_normal((d, 8)) + 1j * RNG.standard_normal((d, 8))
    z = 1500.0 + 40j
    Ao, Ap = Lo(z), Lp(z)
    e, eh = relerr(Ap @ X, Ao @ X), relerr(Ap.H @ X, Ao.conj().T @ X)
    print(f"nodal P2 Rijke spmv: {e:.3e}, adjoint {eh:.3e}")
    assert e < 1e-13 and eh < 1e-13


def test_nodal_family_solve(nodal_rijke):
    Lo, Lp = nodal_rijke
    d = Lo.size()
    z = 340 * 2 * np.pi
    B = RNG.standard_normal((d, 8)) + 1j * RNG.standard_normal((d, 8))
    Xo = spla.splu(sp.csc_matrix(Lo(z))).solve(B)
    X = Lp(z).solve(B, tol=1e-12)
    info = Lp.device().last_info
    print(f"nodal P2 Rijke solve: {info}, error {relerr(X, Xo):.3e}")
    assert info["n_unconverged"] == 0
    assert relerr(X, Xo) < 1e-8


def test_nodal_family_mslp(nodal_rijke):
    Lo, Lp = nodal_rijke
    sol, n, flag = mslp(Lp, 340 * 2 * np.pi, maxiter=20, tol=1e-11)
    solo, no, flago = OS.mslp(Lo, 340 * 2 * np.pi, maxiter=20, tol=1e-11)
    w, wo = sol.params["ω"], solo.params["ω"]
    print(f"mslp device {w!r} in {n} iterations (flag {flag}); oracle {wo!r} in {no} (flag {flago}); last solve {Lp.device().last_info}")
    assert flag in (0, 1)
    assert abs(w - wo) < 1e-10 * abs(wo)
