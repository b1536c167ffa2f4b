"""GPU tests (-m gpu) of the P2 (second-order) assembly on the device -- wae_p2_connectivity, wae_p2_assemble, _boundary, _flame
through helmholtz/assemble.py -- against tests/_p2ref.py (pinned by tests/test_p2_ref.py), and of the P2 Rijke family they produce on the
existing operator and solver path.

Tolerances: assembled values within 1e-13 * max|entry| of the reference (the project's P1 assembly tolerance); fused SpMV-sum 1e-13,
linear solves 1e-8, mslp eigenvalue 1e-10 relative, as tests/test_gpu_parity.py."""
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import _p2ref as R
from oracle import solvers as OS
from oracle.nlevp import LinearOperatorFamily as OracleFamily, Term as OTerm, exp_delay as o_exp_delay, pow1 as o_pow1, pow2 as o_pow2
from wae_amd import _lib
from wae_amd.helmholtz.assemble import assemble_p1, assemble_p2, assemble_p2_boundary, assemble_p2_flame, p2_connectivity
from wae_amd.helmholtz.family import helmholtz_family
from wae_amd.nlevp import mslp

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RNG = np.random.default_rng(2)
SHAPES = ["one", "two", "cube", "rijke"]


@functools.lru_cache(maxsize=None)
def mesh(name):
    """(points, tets, tris, c_tet, c_tri)"""
    if name == "one":
        pts = np.array([[0.0, 0.0, 0.0], [1.0, 0.1, 0.0], [0.2, 0.9, 0.1], [0.1, 0.2, 0.8]])
        return pts, np.array([[0, 1, 2, 3]], dtype=np.int32), np.array([[0, 1, 2], [3, 1, 0]], dtype=np.int32), None, None
    if name == "two":                  # two tetrahedra on the face (3, 1, 4), listed so that one has det J < 0; points not in ascending order
        pts = np.array([[0.1, 0.2, 1.1], [1.0, 0.0, 0.1], [0.3, 0.1, -0.9], [0.0, 0.0, 0.0], [0.1, 1.2, 0.0]])
        tets = np.array([[3, 1, 4, 0], [3, 1, 4, 2]], dtype=np.int32)
        dets = [np.linalg.det((pts[t[:3]] - pts[t[3]]).T) for t in tets]
        assert dets[0] * dets[1] < 0
        return pts, tets, np.array([[4, 1, 0], [2, 3, 1]], dtype=np.int32), np.array([1.5, 0.5]), np.array([2.0, 3.0])
    if name == "cube":
        pts, tets, top = R.kuhn_cube(2)
        return pts, tets, top, None, None
    z = np.load(os.path.join(GOLDEN, "rijke_mesh.npz"))
    return z["points"], z["tetrahedra"], z["outlet_triangles"], z["c_tet"], z["outlet_c"]


@functools.lru_cache(maxsize=None)
def reference(name):
    pts, tets, tris, c_tet, c_tri = mesh(name)
    M, K = R.assemble(pts, tets, c_tet)
    return {"conn": R.connectivity(len(pts), tets, tris), "M": M, "K": K, "C": R.assemble_boundary(pts, tets, tris, c_tri)}


def flame_inputs():
    fl = np.load(os.path.join(GOLDEN, "rijke_flame.npz"))
    return fl["flame_tets"], int(fl["ref_tet"]), np.array([0.0, 0.0, -0.00101]), fl["n_ref"], float(fl["nglobal_scaled"]), float(fl["volume"])


def same_pattern(A, B):
    return A.shape == B.shape and np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices)


def close(A, B, what):
    err, scale = np.max(np.abs(A.data - B.data)), np.max(np.abs(B.data))
    print(f"{what}: max|diff| = {err:.3e} = {err / scale:.3e} * max|entry|")
    return err <= 1e-13 * scale


def relerr(a, b):
    return np.max(np.abs(a - b)) / np.max(np.abs(b))


# ---- 1. connectivity ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SHAPES)
def test_connectivity_equals_the_reference(name):
    pts, tets, tris, _, _ = mesh(name)
    edges, t10, t6 = p2_connectivity(pts, tets, tris)
    re, rt10, rt6 = reference(name)["conn"]
    assert edges.shape == re.shape and np.array_equal(edges, re)
    assert np.array_equal(t10, rt10) and np.array_equal(t6, rt6)
    e2, t10b, t6b = p2_connectivity(len(pts), tets)                    # no triangles; the point count alone
    assert np.array_equal(e2, re) and np.array_equal(t10b, rt10) and t6b.shape == (0, 6)


def test_connectivity_rejects_a_triangle_edge_that_no_tetrahedron_has_and_bad_indices():
    pts, tets, _, _, _ = mesh("cube")
    with pytest.raises(_lib.WaeError):
        p2_connectivity(pts, tets, np.array([[0, 1, 26]], dtype=np.int32))          # (0, 1) is an edge, (0, 26) and (1, 26) are not
    with pytest.raises(_lib.WaeError):
        assemble_p2_boundary(pts, tets, np.array([[0, 1, 26]], dtype=np.int32))
    with pytest.raises(_lib.WaeError):
        p2_connectivity(pts, tets + len(pts))
    with pytest.raises(_lib.WaeError):
        assemble_p2(pts, tets + len(pts))
    with pytest.raises(_lib.WaeError):
        p2_connectivity(pts, tets, np.array([[0, 1, len(pts)]], dtype=np.int32))


# ---- 2. mass and stiffness -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SHAPES)
def test_mass_and_stiffness_match_the_reference(name):
    pts, tets, _, c_tet, _ = mesh(name)
    M, K = assemble_p2(pts, tets, c_tet)
    ref = reference(name)
    assert same_pattern(M, ref["M"]) and same_pattern(K, ref["K"])
    assert np.all(M.data.imag == 0) and np.all(K.data.imag == 0)
    assert close(M, ref["M"], f"{name} M") and close(K, ref["K"], f"{name} K")
    one = np.ones(M.shape[0])
    vol = sum(abs(np.linalg.det((pts[t[:3]] - pts[t[3]]).T)) for t in tets) / 6
    # every entry carries a few rounding errors and the sum of nnz of them a few more: 1e-13 of the sum of the magnitudes bounds both
    assert abs((one @ (M @ one)).real - vol) <= 1e-13 * np.abs(M.data).sum()
    assert np.max(np.abs(K @ one)) < 1e-12 * np.max(np.abs(K.data))
    M2, K2 = assemble_p2(pts, tets, c_tet)
    assert same_pattern(M2, M) and np.array_equal(M2.data, M.data) and np.array_equal(K2.data, K.data)          # deterministic: same bits
    print(f"{name}: dim {M.shape[0]}, nnz {M.nnz}, nonzeros per row max {np.diff(M.indptr).max()} mean {M.nnz / M.shape[0]:.1f}")


# ---- 3. boundary mass ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cube", "rijke", "two"])
def test_boundary_mass_matches_the_reference(name):
    pts, tets, tris, _, c_tri = mesh(name)
    Cm = assemble_p2_boundary(pts, tets, tris, c_tri)
    ref = reference(name)["C"]
    assert same_pattern(Cm, ref)
    assert np.all(Cm.data.real == 0)
    assert close(Cm, ref, f"{name} C")
    assert np.array_equal(assemble_p2_boundary(pts, tets, tris, c_tri).data, Cm.data)


# ---- 4. flame --------------------------------------------------------------------------------------------------------------------------
def test_flame_operator_matches_the_reference():
    pts, tets, _, _, _ = mesh("rijke")
    flame_tets, ref_tet, x_ref, n_ref, ngs, volume = flame_inputs()
    Q, vol = assemble_p2_flame(pts, tets, flame_tets, ref_tet, x_ref, n_ref, ngs)
    Qr, volr = R.assemble_flame(pts, tets, flame_tets, ref_tet, x_ref, n_ref, ngs)
    assert same_pattern(Q, Qr) and close(Q, Qr, "Q")
    print(f"flame volume {vol!r}, fixture {volume!r}, reference {volr!r}")
    assert abs(vol - volume) <= 1e-13 * volume
    assert np.array_equal(assemble_p2_flame(pts, tets, flame_tets, ref_tet, x_ref, n_ref, ngs)[0].data, Q.data)
    for bad in (-1, len(tets)):
        with pytest.raises(_lib.WaeError):
            assemble_p2_flame(pts, tets, flame_tets, bad, x_ref, n_ref, ngs)
    with pytest.raises(_lib.WaeError):
        assemble_p2_flame(pts, tets, [0, len(tets)], ref_tet, x_ref, n_ref, ngs)


# ---- 5. convergence order ----------------------------------------------------------------------------------------------------------------
def test_p2_is_closer_to_the_exact_eigenvalue_than_p1():
    """Smallest non-zero eigenvalue of (-K) u = w^2 M u on the unit cube with Neumann walls, c = 1, 4^3 Kuhn cells: exactly pi^2.
    Theory: O(h^4) for P2 against O(h^2) for P1.  tests/_p2ref.py on the CPU: |w2_P1 - pi^2| = 4.599e-01, |w2_P2 - pi^2| = 4.293e-03."""
    pts, tets, _ = R.kuhn_cube(4)
    e1 = abs(R.smallest_nonzero_eigenvalue(*assemble_p1(pts, tets)) - np.pi ** 2)
    e2 = abs(R.smallest_nonzero_eigenvalue(*assemble_p2(pts, tets)) - np.pi ** 2)
    print(f"|w2_P1 - pi^2| = {e1:.3e}   |w2_P2 - pi^2| = {e2:.3e}")
    assert e2 < e1


# ---- 6. the P2 Rijke family on the operator and solver path ---------------------------------------------------------------------------------
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
def p2_rijke():
    pts, tets, tris, c_tet, c_tri = mesh("rijke")
    flame_tets, ref_tet, x_ref, n_ref, ngs, _ = flame_inputs()
    M, K = assemble_p2(pts, tets, c_tet)
    t = {"M": M, "K": K, "C": assemble_p2_boundary(pts, tets, tris, c_tri),
         "Q": assemble_p2_flame(pts, tets, flame_tets, ref_tet, x_ref, n_ref, ngs)[0]}
    Lp = helmholtz_family(t, n=1.0, tau=0.001)
    Lp.solver_ref = 340 * 2 * np.pi
    nzr = np.diff((abs(M) + abs(t["C"]) + abs(t["Q"])).tocsr().indptr)
    print(f"P2 Rijke family: d = {M.shape[0]}, nonzeros per row of M/K max {np.diff(M.indptr).max()} mean {M.nnz / M.shape[0]:.1f}; "
          f"of the summed operator max {nzr.max()}")
    yield oracle_family(t, 1.0, 0.001), Lp
    Lp._drop_device()


@pytest.mark.parametrize("r", [1, 8, 19])
def test_p2_family_spmv_sum(p2_rijke, r):
    Lo, Lp = p2_rijke
    d = Lo.size()
    X = RNG.standard_normal((d, r)) + 1j * RNG.standard_normal((d, r))
    z = 1500.0 + 40j
    Ao, Ap = Lo(z), Lp(z)
    assert relerr(Ap @ X, Ao @ X) < 1e-13
    assert relerr(Ap.H @ X, Ao.conj().T @ X) < 1e-13


def test_p2_family_solve(p2_rijke):
    Lo, Lp = p2_rijke
    d = Lo.size()
    z = 340 * 2 * np.pi
    B = RNG.standard_normal((d, 8)) + 1j * RNG.standard_normal((d, 8))
    Xo = spla.splu(sp.csc_matrix(Lo(z))).solve(B)
    X = Lp(z).solve(B, tol=1e-12)
    info = Lp.device().last_info
    print(f"P2 Rijke solve, default hierarchy: {info}")
    assert info["n_unconverged"] == 0
    assert relerr(X, Xo) < 1e-8


def test_p2_family_mslp(p2_rijke):
    """mslp on the device against the oracle's mslp on the same scipy terms, relative 1e-10 as test_G5_mslp_active_flame.  Three CPU oracle
    runs on the reference-assembled P2 terms (start vector of ones, and two with 1e-3 noise on it) agree to 1.8e-14 relative, below 1e-11, so the 1e-10 stands."""
    Lo, Lp = p2_rijke
    sol, n, flag = mslp(Lp, 340 * 2 * np.pi, maxiter=20, tol=1e-11)
    solo, no, flago = OS.mslp(Lo, 340 * 2 * np.pi, maxiter=20, tol=1e-11)
    w, wo = sol.params["ω"], solo.params["ω"]
    print(f"mslp device {w!r} in {n} iterations (flag {flag}); oracle {wo!r} in {no} (flag {flago}); last solve {Lp.device().last_info}")
    assert flag in (0, 1)
    assert abs(w - wo) < 1e-10 * abs(wo)
