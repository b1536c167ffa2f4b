"""GPU tests (-m gpu) of the Hermite (cubic) assembly on the device -- wae_herm_connectivity, wae_herm_assemble, _boundary, _flame through
helmholtz/assemble.py -- against tests/_hermref.py (pinned by tests/test_herm_ref.py), and of the Hermite Rijke family they produce on the
existing operator path.

Tolerance of the assembled values: 1e-13 * max|entry| (the project's assembly tolerance), applied block by block: the DoF classes value,
derivative and face scale with different powers of h, so every one of the nine (row class, column class) blocks is measured against its
own largest entry.  tests/test_herm_ref.py measures the float64 error of the reference itself: up to 9.2e-14 of a block's largest entry on
the Rijke mesh (value-face block of M), more than a quarter of the tolerance.  The device is therefore compared with the reference
evaluated in numpy.longdouble (rounded to float64 at the end); the tolerance stays 1e-13.

The polynomial identities use the bound those 1e-13 imply: with E_ab <= 1e-13 * max|block(a, b)| on the pattern,
|u^T E v| <= 1e-13 * |u|^T Bmax |v|, plus 1e-14 * |u|^T |A| |v| for the rounding of the product and of the direct integration."""
import ctypes as C
import functools
import os
from fractions import Fraction

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import _hermref as R
import _p2ref as P2
from oracle.nlevp import LinearOperatorFamily as OracleFamily, Term as OTerm, exp_delay as o_exp_delay, pow1 as o_pow1, pow2 as o_pow2
from wae_amd import _lib
from wae_amd.helmholtz.assemble import (assemble_herm, assemble_herm_boundary, assemble_herm_flame, assemble_p1, assemble_p2, assemble_p2_boundary,
                                        assemble_p2_flame, assemble_p1_boundary, assemble_p1_flame, herm_connectivity, herm_dof_count, herm_dofs)
from wae_amd.helmholtz.family import helmholtz_family

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RNG = np.random.default_rng(3)
SHAPES = ["one", "two", "cube", "rijke"]
LD = np.longdouble
TOL = 1e-13
INT_MAX = 2 ** 31 - 1


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
    if name == "cube":                 # 48 tetrahedra; only the top face is listed: the other boundary faces are numbered by rank
        pts, tets, top = R.kuhn_cube(2)
        return pts, tets, top, None, None
    z = np.load(os.path.join(GOLDEN, "rijke_mesh.npz"))
    return z["points"], z["tetrahedra"], z["outlet_triangles"], z["c_tet"], z["outlet_c"]


@functools.lru_cache(maxsize=None)
def reference(name):
    """connectivity, and M, K, C evaluated in longdouble"""
    pts, tets, tris, c_tet, c_tri = mesh(name)
    M, K = R.assemble(pts, tets, tris, c_tet, dtype=LD)
    Cm, stray = R.assemble_boundary(pts, tets, tris, c_tri, dtype=LD)
    assert stray < 1e-15
    return {"conn": R.connectivity(len(pts), tets, tris), "M": M, "K": K, "C": Cm}


def flame_inputs():
    fl = np.load(os.path.join(GOLDEN, "rijke_flame.npz"))
    return fl["flame_tets"], int(fl["ref_tet"]), np.array([0.0, 0.0, -0.00101]), fl["n_ref"], float(fl["nglobal_scaled"]), float(fl["volume"])


def same_pattern(A, B):
    return A.shape == B.shape and np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices)


def close_blockwise(A, B, npoints, what):
    """every (row class, column class) block of A within TOL * max|block of B| of B; prints the figures first"""
    d = R.blockwise_distance(sp.csr_matrix(A.real if np.all(A.data.imag == 0) else A.imag), sp.csr_matrix(B.real if np.all(B.data.imag == 0) else B.imag),
                             npoints)
    print(f"{what}: blockwise max|diff| / max|block| = " + ", ".join(f"{k}: {v:.2e}" for k, v in sorted(d.items())))
    return max(d.values()) <= TOL


def block_max_matrix(A, npoints):
    """the pattern of A with every entry replaced by the largest |entry| of its (row class, column class) block"""
    A = sp.csr_matrix(A)
    rc = R.dof_class(np.repeat(np.arange(A.shape[0]), np.diff(A.indptr)), npoints)
    cc = R.dof_class(A.indices, npoints)
    data = np.zeros(A.nnz)
    for r in range(3):
        for c in range(3):
            sel = (rc == r) & (cc == c)
            if sel.any():
                data[sel] = np.max(np.abs(A.data[sel]))
    return sp.csr_matrix((data, A.indices.copy(), A.indptr.copy()), shape=A.shape)


def form_bound(A, u, v, npoints):
    return TOL * (np.abs(u) @ (block_max_matrix(A, npoints) @ np.abs(v))) + 1e-14 * (np.abs(u) @ (abs(A) @ np.abs(v)))


def polynomials(n=3, seed=11):
    """n polynomials of degree <= 3 with random rational coefficients: (f, grad f), both taking (m, 3) positions"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        co = [float(Fraction(int(rng.integers(-5, 6)), int(rng.integers(1, 5)))) for _ in R.EXPONENTS]

        def f(x, co=co):
            return sum(c * x[:, 0] ** a * x[:, 1] ** b * x[:, 2] ** d for c, (a, b, d) in zip(co, R.EXPONENTS))

        def g(x, co=co):
            out = np.zeros((len(x), 3))
            for c, (a, b, d) in zip(co, R.EXPONENTS):
                if a:
                    out[:, 0] += c * a * x[:, 0] ** (a - 1) * x[:, 1] ** b * x[:, 2] ** d
                if b:
                    out[:, 1] += c * b * x[:, 0] ** a * x[:, 1] ** (b - 1) * x[:, 2] ** d
                if d:
                    out[:, 2] += c * d * x[:, 0] ** a * x[:, 1] ** b * x[:, 2] ** (d - 1)
            return out
        out.append((f, g))
    return out


def volume_integrals(pts, tets, c_tet, f, g):
    """(int f^2, int c^2 |grad f|^2) over the mesh by a degree-6 rule per tetrahedron, no basis involved"""
    lam, w = R.tet_rule(6, np.float64)
    X = pts[tets]
    adet = np.abs(np.linalg.det(np.transpose(X[:, :3] - X[:, 3:4], (0, 2, 1))))
    x = np.einsum("qk,tkd->tqd", lam, X).reshape(-1, 3)
    c2 = np.ones(len(tets)) if c_tet is None else np.asarray(c_tet) ** 2
    f2 = (f(x) ** 2).reshape(len(tets), -1) @ w
    g2 = (g(x) ** 2).sum(axis=1).reshape(len(tets), -1) @ w
    return float(adet @ f2), float((c2 * adet) @ g2)


def surface_integral(pts, tris, c_tri, f):
    lam, w = R.tri_rule(6, np.float64)
    q = pts[tris]
    a2 = np.linalg.norm(np.cross(q[:, 0] - q[:, 2], q[:, 1] - q[:, 2]), axis=1)
    x = np.einsum("qk,tkd->tqd", lam, q).reshape(-1, 3)
    cc = np.ones(len(tris)) if c_tri is None else np.asarray(c_tri)
    return float((cc * a2) @ ((f(x) ** 2).reshape(len(tris), -1) @ w))


# ---- 1. connectivity ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SHAPES)
def test_connectivity_equals_the_reference(name):
    pts, tets, tris, _, _ = mesh(name)
    faces, t20, t13, ndof = herm_connectivity(pts, tets, tris)
    rf, rt20, rt13, rn = reference(name)["conn"]
    assert ndof == rn == herm_dof_count(pts, tets, tris)
    assert faces.shape == rf.shape and np.array_equal(faces, rf)
    assert np.array_equal(t20, rt20) and np.array_equal(t13, rt13)
    f2, t20b, t13b, n2 = herm_connectivity(len(pts), tets)             # no triangles; the point count alone
    rf2, rt20b, _, rn2 = R.connectivity(len(pts), tets)
    assert n2 == rn2 == ndof and np.array_equal(f2, rf2) and np.array_equal(t20b, rt20b) and t13b.shape == (0, 13)
    f3, t20c, t13c, _ = herm_connectivity(pts, tets, tris)             # the same bits on every call
    assert np.array_equal(f3, faces) and np.array_equal(t20c, t20) and np.array_equal(t13c, t13)


def test_connectivity_rejections():
    """every rejection of wae_herm_connectivity, each on the smallest mesh that has it; nothing is written"""
    pts1, tets1, tris1, _, _ = mesh("one")
    pts2, tets2, tris2, _, _ = mesh("two")

    def rejected(npoints, tets, tris, text):
        with pytest.raises(_lib.WaeError) as e:
            herm_connectivity(npoints, tets, tris)
        assert e.value.code == _lib.WAE_ERR_INVALID and text in str(e.value), str(e.value)

    rejected(4, tets1 + 1, None, "tetrahedron refers to a point outside")
    rejected(4, tets1, np.array([[0, 1, 4]], dtype=np.int32), "triangle refers to a point outside")
    rejected(5, tets2, np.array([[0, 1, 2]], dtype=np.int32), "no tetrahedron's face")                    # three points of the mesh, no face
    rejected(4, tets1, np.array([[0, 1, 2], [2, 0, 1]], dtype=np.int32), "listed twice")
    three = np.array([[0, 1, 2, 3], [0, 1, 2, 4], [0, 1, 2, 5]], dtype=np.int32)                          # the face (0, 1, 2) in three tetrahedra
    rejected(6, three, None, "more than two tetrahedra")
    rejected(2 ** 21 + 1, tets1, None, "too many points")
    L, ip, h = _lib.lib(), C.POINTER(C.c_int32), C.c_void_p()                      # the 32-bit limits: counts alone, the lists are not read
    for nt, ns in ((INT_MAX // 400 + 1, 0), (1, INT_MAX // 169 + 1)):
        code = L.wae_herm_connectivity(0, 4, nt, tets1.ctypes.data_as(ip), ns, tris1.ctypes.data_as(ip), C.byref(h))
        assert code == _lib.WAE_ERR_INVALID and "mesh too large" in L.wae_last_error().decode() and h.value is None
    with pytest.raises(_lib.WaeError):
        assemble_herm(pts2, tets2, np.array([[0, 1, 2]], dtype=np.int32))
    with pytest.raises(_lib.WaeError):
        assemble_herm_boundary(pts1, tets1, np.array([[0, 1, 2], [2, 0, 1]], dtype=np.int32))
    faces, _, _, ndof = herm_connectivity(2 ** 21, tets1, tris1)                                            # the largest point count goes through
    assert ndof == 4 * 2 ** 21 + 4 and len(faces) == 2


# ---- 2. mass and stiffness -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SHAPES)
def test_mass_and_stiffness_match_the_reference(name):
    pts, tets, tris, c_tet, _ = mesh(name)
    N = len(pts)
    M, K = assemble_herm(pts, tets, tris, c_tet)
    ref = reference(name)
    assert same_pattern(M, ref["M"]) and same_pattern(K, ref["K"])
    assert np.all(M.data.imag == 0) and np.all(K.data.imag == 0)
    okm, okk = close_blockwise(M, ref["M"], N, f"{name} M"), close_blockwise(K, ref["K"], N, f"{name} K")
    assert okm and okk
    M2, K2 = assemble_herm(pts, tets, tris, c_tet)
    assert same_pattern(M2, M) and np.array_equal(M2.data, M.data) and np.array_equal(K2.data, K.data)          # deterministic: same bits
    print(f"{name}: dim {M.shape[0]}, nnz {M.nnz}, nonzeros per row max {np.diff(M.indptr).max()} mean {M.nnz / M.shape[0]:.1f}")


@pytest.mark.parametrize("name", SHAPES)
def test_polynomial_identities_hold_on_the_device_matrices(name):
    """u = herm_dofs(p, grad p) of a cubic p represents p exactly: u^T M u = int p^2, u^T (-K) u = int c^2 |grad p|^2, u^T b u = c int_boundary p^2,
    K u_const = 0, u_const^T M u_const = the volume -- each against a direct integration of the polynomial"""
    pts, tets, tris, c_tet, c_tri = mesh(name)
    N = len(pts)
    faces, _, _, ndof = herm_connectivity(pts, tets, tris)
    M, K = (A.real.tocsr() for A in assemble_herm(pts, tets, tris, c_tet))
    b = (1j * assemble_herm_boundary(pts, tets, tris, c_tri)).real.tocsr()
    for f, g in polynomials():
        u = herm_dofs(pts, faces, tris, f, g)
        assert u.shape == (ndof,) and np.array_equal(u, R.dofs(pts, faces, tris, f, g))
        i_m, i_k = volume_integrals(pts, tets, c_tet, f, g)
        i_b = surface_integral(pts, tris, c_tri, f)
        e_m, e_k, e_b = abs(u @ (M @ u) - i_m), abs(-(u @ (K @ u)) - i_k), abs(u @ (b @ u) - i_b)
        print(f"{name}: |uMu - int p^2| = {e_m:.2e} (bound {form_bound(M, u, u, N):.2e}), K: {e_k:.2e} ({form_bound(K, u, u, N):.2e}), "
              f"b: {e_b:.2e} ({form_bound(b, u, u, N):.2e})")
        assert e_m <= form_bound(M, u, u, N) and e_k <= form_bound(K, u, u, N) and e_b <= form_bound(b, u, u, N)
    one = herm_dofs(pts, faces, tris, lambda x: np.ones(len(x)), lambda x: np.zeros((len(x), 3)))
    vol = float(np.abs(np.linalg.det(np.transpose(pts[tets][:, :3] - pts[tets][:, 3:4], (0, 2, 1)))).sum() / 6)
    assert abs(one @ (M @ one) - vol) <= form_bound(M, one, one, N)
    bound = TOL * (block_max_matrix(K, N) @ one) + 1e-14 * (abs(K) @ one)
    assert np.all(np.abs(K @ one) <= bound)


# ---- 3. boundary mass ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cube", "rijke", "two"])
def test_boundary_mass_matches_the_reference(name):
    pts, tets, tris, _, c_tri = mesh(name)
    Cm = assemble_herm_boundary(pts, tets, tris, c_tri)
    ref = reference(name)["C"]
    assert same_pattern(Cm, ref)
    assert np.all(Cm.data.real == 0)
    assert close_blockwise(Cm, ref, len(pts), f"{name} C")
    assert np.array_equal(assemble_herm_boundary(pts, tets, tris, c_tri).data, Cm.data)


# ---- 4. flame --------------------------------------------------------------------------------------------------------------------------
def test_flame_operator_matches_the_reference():
    pts, tets, tris, _, _ = mesh("rijke")
    flame_tets, ref_tet, x_ref, n_ref, ngs, volume = flame_inputs()
    Q, vol = assemble_herm_flame(pts, tets, tris, flame_tets, ref_tet, x_ref, n_ref, ngs)
    Qr, volr, _, _ = R.assemble_flame(pts, tets, tris, flame_tets, ref_tet, x_ref, n_ref, ngs, dtype=LD)
    assert same_pattern(Q, Qr) and np.all(Q.data.imag == 0)
    assert close_blockwise(Q, Qr, len(pts), "Q")
    print(f"flame volume {vol!r}, fixture {volume!r}, reference {volr!r}")
    assert abs(vol - volume) <= 1e-13 * volume
    assert np.array_equal(assemble_herm_flame(pts, tets, tris, flame_tets, ref_tet, x_ref, n_ref, ngs)[0].data, Q.data)
    for bad in (-1, len(tets)):
        with pytest.raises(_lib.WaeError):
            assemble_herm_flame(pts, tets, tris, flame_tets, bad, x_ref, n_ref, ngs)
    for bad in ([0, len(tets)], [-1, 0]):
        with pytest.raises(_lib.WaeError):
            assemble_herm_flame(pts, tets, tris, bad, ref_tet, x_ref, n_ref, ngs)


# ---- 5. convergence ----------------------------------------------------------------------------------------------------------------------
def test_hermite_is_closer_to_the_exact_eigenvalue_than_p1():
    """Smallest non-zero eigenvalue of (-K) u = w^2 M u on the unit cube with Neumann walls, c = 1, 4^3 Kuhn cells: exactly pi^2.
    On the CPU, with tests/_p2ref.py and tests/_hermref.py:  |w2_P1 - pi^2| = 4.599e-01,  |w2_P2 - pi^2| = 4.293e-03,
    |w2_Hermite - pi^2| = 2.814e-05.  Hermite is 150 times closer than P2 at this size, more than the factor 2 that the comparison asks for
    before it is asserted (the two spaces are not nested, so the order is no theorem), so both inequalities are asserted."""
    pts, tets, _ = R.kuhn_cube(4)
    e1 = abs(P2.smallest_nonzero_eigenvalue(*assemble_p1(pts, tets)) - np.pi ** 2)
    e2 = abs(P2.smallest_nonzero_eigenvalue(*assemble_p2(pts, tets)) - np.pi ** 2)
    e3 = abs(R.smallest_nonzero_eigenvalue(*assemble_herm(pts, tets)) - np.pi ** 2)
    print(f"|w2_P1 - pi^2| = {e1:.3e}   |w2_P2 - pi^2| = {e2:.3e}   |w2_Hermite - pi^2| = {e3:.3e}")
    assert e3 < e1
    assert e3 < e2


# ---- 6. the Hermite Rijke family on the operator path --------------------------------------------------------------------------------------
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


@functools.lru_cache(maxsize=None)
def rijke_terms(order):
    pts, tets, tris, c_tet, c_tri = mesh("rijke")
    flame_tets, ref_tet, x_ref, n_ref, ngs, _ = flame_inputs()
    if order == "herm":
        M, K = assemble_herm(pts, tets, tris, c_tet)
        return {"M": M, "K": K, "C": assemble_herm_boundary(pts, tets, tris, c_tri),
                "Q": assemble_herm_flame(pts, tets, tris, flame_tets, ref_tet, x_ref, n_ref, ngs)[0]}
    if order == "quad":
        M, K = assemble_p2(pts, tets, c_tet)
        return {"M": M, "K": K, "C": assemble_p2_boundary(pts, tets, tris, c_tri),
                "Q": assemble_p2_flame(pts, tets, flame_tets, ref_tet, x_ref, n_ref, ngs)[0]}
    M, K = assemble_p1(pts, tets, c_tet)
    return {"M": M, "K": K, "C": assemble_p1_boundary(pts, tris, c_tri), "Q": assemble_p1_flame(pts, tets, flame_tets, ref_tet, n_ref, ngs)[0]}


@pytest.fixture(scope="module")
def herm_rijke():
    t = rijke_terms("herm")
    Lp = helmholtz_family(t, n=1.0, tau=0.001)
    print(f"Hermite Rijke family: d = {t['M'].shape[0]}, nonzeros per row of M/K max {np.diff(t['M'].indptr).max()} mean {t['M'].nnz / t['M'].shape[0]:.1f}")
    yield oracle_family(t, 1.0, 0.001), Lp
    Lp._drop_device()


def relerr(a, b):
    return np.max(np.abs(a - b)) / np.max(np.abs(b))


@pytest.mark.parametrize("r", [1, 8, 19])
def test_herm_family_spmv_sum(herm_rijke, r):
    Lo, Lp = herm_rijke
    d = Lo.size()
    X = RNG.standard_normal((d, r)) + 1j * RNG.standard_normal((d, r))
    z = 1500.0 + 40j
    Ao, Ap = Lo(z), Lp(z)
    assert relerr(Ap @ X, Ao @ X) < 1e-13
    assert relerr(Ap.H @ X, Ao.conj().T @ X) < 1e-13


def passive_mode(t, sigma=340 * 2 * np.pi):
    """the eigenvalue w nearest sigma of the passive pencil (w^2 M + w Y C + K) v = 0 with Y = 1e15 (the outlet is a pressure node): the
    pencil is small, so scipy shift-invert on -(K + w Y C) v = w^2 M v, w under the penalty term taken from the step before (it hardly
    matters there: four steps reach 1e-9 on the CPU references)"""
    M, K, Cm = (sp.csc_matrix(t[k]).astype(complex) for k in ("M", "K", "C"))
    w = complex(sigma)
    for _ in range(4):
        lam = spla.eigs(-(K + w * 1e15 * Cm), k=3, M=M, sigma=w * w, which="LM", return_eigenvectors=False, v0=np.ones(M.shape[0]))
        w = np.sqrt(lam[np.argmin(np.abs(lam - w * w))])
    return w


def test_herm_passive_mode_lies_near_the_p2_one():
    """A sanity bound, not a pin: the passive Rijke mode of the device-assembled Hermite matrices lies within the distance P2-to-P1 of the
    P2 value (the higher-order spaces agree with each other better than either does with P1).  With the CPU references: P1 1709.4299,
    P2 1709.1090, Hermite 1709.0640 rad/s; |P2 - P1| = 0.321, |Hermite - P2| = 0.045."""
    w1, w2, w3 = (passive_mode(rijke_terms(o)) for o in ("lin", "quad", "herm"))
    print(f"passive mode: P1 {w1!r}, P2 {w2!r}, Hermite {w3!r}; |P2 - P1| = {abs(w2 - w1):.3e}, |Hermite - P2| = {abs(w3 - w2):.3e}")
    assert abs(w3 - w2) < abs(w2 - w1)
