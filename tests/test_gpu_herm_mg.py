"""GPU tests (-m gpu) of the Hermite p-hierarchy: the two prolongators of wae_hermite_prolongators against tests/_hermmgref.py (pinned by
tests/test_hermmg_ref.py), the per-level weight scale of the set-up (opts[12]) against scipy's eigenvalues of the recovered levels, the
solve of the Hermite Rijke family that the scale makes converge, and householder on that family.

Tolerance of the prolongators: 1e-13 of the largest entry of the row class (identity rows and face rows of P_face; value rows and
gradient rows of P_lin); the figures per (row class, column class) are printed beside it.

The solve.  maxit = 4 x the iteration count of the reference restatement (tests/_hermmgref.py: exact P1 solve, one column): a cap, the
device runs an aggregation cycle below P1.  The result is held to what tests/test_gpu_nested_mg.py demands of its solves, the
preconditioned residual ||M^-1 (b - A x)|| / ||M^-1 b|| <= 1e-10, recomputed here: the residual b - A x on the host with scipy's
matrices, M^-1 by one application of the solver's own cycle (wae_debug_vcycle).  That figure leans on the device's M, so X is also held
to scipy's spsolve, for op N and op H, within kappa(M^-1 A) x 1e-10 with kappa from the host restatement's own count (spsolve_bound).
MI355X: reference restatement 67 iterations; device 71 (op N and H), recomputed residuals 5.4e-11..6.8e-11, distance to spsolve 7.9e-10."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import _hermmgref as G
from _hier import recover
from wae_amd import _lib
from wae_amd.helmholtz.assemble import herm_prolongators
from wae_amd.helmholtz.family import helmholtz_family, herm_hierarchy
from wae_amd.nlevp import householder

pytestmark = pytest.mark.gpu
TOL = 1e-13
W340 = 2 * np.pi * 340.0
W_ORACLE = 2 * np.pi * (169.74501497 + 59.01432702j)                # OS.householder on the oracle family from 1709.0640 rad/s, n = 1, tau = 1e-3


# ---- 1. prolongators -------------------------------------------------------------------------------------------------------------------
def row_classes(P, N):
    """(name, row mask) of the row classes of P_face (ndof x 4N) or P_lin (4N x N)"""
    r = np.arange(P.shape[0])
    if P.shape[1] == 4 * N:
        return [("identity", r < 4 * N), ("face", r >= 4 * N)]
    return [("value", r < N), ("gradient", r >= N)]


@pytest.mark.parametrize("name", G.SHAPES)
def test_prolongators_match_the_reference(name):
    pts, tets, tris = G.mesh(name)
    N = len(pts)
    got = herm_prolongators(pts, tets, tris)
    ref = [G.p_face_ref(pts, tets, tris), G.p_lin_ref(pts, tets)]
    for P, Rf, what in zip(got, ref, ("P_face", "P_lin")):
        assert P.shape == Rf.shape and P.dtype == np.float64
        assert np.array_equal(P.indptr, Rf.indptr) and np.array_equal(P.indices, Rf.indices), what
        assert np.all(np.diff(P.indices)[np.setdiff1d(np.arange(P.nnz - 1), P.indptr[1:-1] - 1)] > 0)        # columns ascending, no duplicates
        rows = np.repeat(np.arange(P.shape[0]), np.diff(P.indptr))
        for cls, mask in row_classes(P, N):
            sel = mask[rows]
            err, big = np.max(np.abs(P.data[sel] - Rf.data[sel])), np.max(np.abs(Rf.data[sel]))
            vcol = P.indices[sel] < N
            parts = ", ".join(f"{lab} {np.max(np.abs(P.data[sel][m] - Rf.data[sel][m])) / np.max(np.abs(Rf.data[sel][m])):.1e}"
                              for lab, m in (("value columns", vcol), ("gradient columns", ~vcol)) if m.any() and np.max(np.abs(Rf.data[sel][m])) > 0)
            print(f"{name} {what} {cls} rows: max|diff| {err:.2e}, largest entry {big:.2e}; relative by column class: {parts}")
            assert err <= TOL * big, (what, cls)
    again = herm_prolongators(pts, tets, tris)
    for P, Q in zip(got, again):
        assert np.array_equal(P.indptr, Q.indptr) and np.array_equal(P.indices, Q.indices) and np.array_equal(P.data.view(np.uint64), Q.data.view(np.uint64))
    if name in ("two", "cube"):                                       # no triangles listed: another numbering of the faces, the same P_lin
        none = herm_prolongators(pts, tets)
        ref0 = G.p_face_ref(pts, tets, None)
        assert np.array_equal(none[0].indices, ref0.indices) and np.max(np.abs(none[0].data - ref0.data)) <= TOL
        assert np.array_equal(none[1].data.view(np.uint64), got[1].data.view(np.uint64))


def test_prolongator_refusals():
    """what wae_herm_connectivity refuses, carried through; a point of no tetrahedron; a point whose tetrahedra are all degenerate"""
    pts1, tets1, tris1 = G.mesh("one")
    pts2, tets2, _ = G.mesh("two")

    def rejected(pts, tets, tris, text):
        with pytest.raises(_lib.WaeError) as e:
            herm_prolongators(pts, tets, tris)
        assert e.value.code == _lib.WAE_ERR_INVALID and text in str(e.value), str(e.value)

    rejected(pts1, tets1 + 1, None, "tetrahedron refers to a point outside")
    rejected(pts1, tets1, np.array([[0, 1, 4]], dtype=np.int32), "triangle refers to a point outside")
    rejected(pts2, tets2, np.array([[0, 1, 2]], dtype=np.int32), "no tetrahedron's face")
    rejected(pts1, tets1, np.array([[0, 1, 2], [2, 0, 1]], dtype=np.int32), "listed twice")
    three = np.array([[0, 1, 2, 3], [0, 1, 2, 4], [0, 1, 2, 5]], dtype=np.int32)
    rejected(np.vstack([pts2, [[0.5, 0.5, 0.5]]]), three, None, "more than two tetrahedra")
    rejected(np.vstack([pts1, [[2.0, 2.0, 2.0]]]), tets1, None, "belongs to no tetrahedron")
    flat = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [1.0, 1.0, 0.0]])                  # four points in a plane: det J = 0
    rejected(flat, tets1, None, "have no volume")
    L, ip, dp, h = _lib.lib(), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_void_p()      # the limits: counts alone, the lists are not read
    p, t, s = pts1.ctypes.data_as(dp), tets1.ctypes.data_as(ip), tris1.ctypes.data_as(ip)
    for npts, nt, ns, text in ((2 ** 21 + 1, 1, 0, "too many points"), (4, (2 ** 31 - 1) // 400 + 1, 0, "mesh too large"),
                               (4, 1, (2 ** 31 - 1) // 169 + 1, "mesh too large")):
        assert L.wae_hermite_prolongators(0, npts, p, nt, t, ns, s, C.byref(h)) == _lib.WAE_ERR_INVALID
        assert text in L.wae_last_error().decode() and h.value is None
    assert L.wae_hermite_prolongators(0, 4, None, 1, t, 0, None, C.byref(h)) == _lib.WAE_ERR_INVALID and h.value is None
    assert L.wae_hermite_prolongators(0, 4, p, 1, t, 0, None, C.byref(h)) == 0
    try:
        n = C.c_int64(0)
        for which in (-1, 2):
            assert L.wae_hermite_prolongators_info(h, which, C.byref(n), None, None) == _lib.WAE_ERR_INVALID
            assert L.wae_hermite_prolongators_get(h, which, None, None, None) == _lib.WAE_ERR_INVALID
        assert L.wae_hermite_prolongators_info(h, 0, C.byref(n), None, None) == 0 and n.value == 20
    finally:
        L.wae_hermite_prolongators_free(h)


# ---- 2. level weights --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def herm_terms():
    from test_gpu_herm import rijke_terms
    return rijke_terms("herm")


@pytest.fixture(scope="module")
def herm_family(herm_terms):
    pts, tets, tris = G.mesh("rijke")
    Lp = herm_hierarchy(helmholtz_family(herm_terms, n=1.0, tau=0.001), pts, tets, tris)
    Lp.solver_ref = W340
    yield Lp
    Lp._drop_device()


@pytest.fixture(scope="module")
def reference_count():
    """iterations of the host restatement with scaled weights, one column (printed: the yardstick of the cap)"""
    A = G.rijke_operator(W340)
    pts, tets, tris = G.mesh("rijke")
    Ps = G.hierarchy(A, [G.p_face_ref(pts, tets, tris), G.p_lin_ref(pts, tets)])
    ops = G.level_operators(A, Ps)
    scales = [G.scale_of(G.power_estimate(B)) for B in ops[:-1]]
    _, its, rel = G.gmres_left(A, G.Cycle(ops, Ps, scales).apply, G.rhs(A.shape[0], 1)[:, 0])
    print(f"reference restatement: {its} iterations to {rel:.2e}")
    assert rel <= 1e-10
    return its


def test_level_weights_follow_the_spectrum(herm_family):
    Lp = herm_family
    fam = Lp.ensure_solver()
    lam, scale = fam.level_weights()
    sizes = sorted((lv, ni) for w, lv, ni, no in fam.level_sizes() if w == 0)
    assert len(lam) == len(scale) == len(sizes) and len(sizes) >= 3 and sizes[1][1] <= 4024 and sizes[2][1] <= 1006
    c = Lp.coefficients(W340)
    for (l, n), lm, sc in zip(sizes, lam, scale):
        terms = [sp.csr_matrix(t.coeff) for t in Lp.terms] if l == 0 else [recover(fam, 0, l, n, n, k) for k in range(fam.T)]
        A = sum(ck * t for ck, t in zip(c, terms) if ck != 0)
        true = G.lambda_max(A)
        print(f"level {l}: n = {n}, lambda_max(D^-1 Re A) = {true:.6f}, device estimate {lm:.6f} ({lm / true:.4f}), scale {sc:.6f}")
        assert 0.9 * true <= lm <= true * (1 + 1e-10)
        assert sc == min(1.0, 5.0 / (3.0 * 1.1 * lm))
    lam2, scale2 = fam.level_weights()
    fam.solver_ready = False
    fam2 = Lp.ensure_solver()                                          # a second set-up: the same bits
    lam3, scale3 = fam2.level_weights()
    assert np.array_equal(lam, lam3) and np.array_equal(scale, scale3) and np.array_equal(lam, lam2) and np.array_equal(scale, scale2)


def test_the_switch_is_off_by_default(herm_terms):
    Lp = helmholtz_family(herm_terms, n=1.0, tau=0.001)
    Lp.solver_ref = W340
    try:
        lam, scale = Lp.ensure_solver().level_weights()
        assert len(scale) >= 1 and np.all(scale == 1.0) and np.all(lam == 0.0)
        fam = Lp.device()
        c = np.ascontiguousarray(Lp.coefficients(W340), dtype=np.complex128)
        opts = np.zeros(13)
        opts[12] = 2.0
        assert _lib.lib().wae_solver_setup(fam.handle, _lib.zptr(c), opts.ctypes.data_as(C.POINTER(C.c_double)), 13) == _lib.WAE_ERR_INVALID
        assert "opts[12]" in _lib.lib().wae_last_error().decode()
    finally:
        Lp._drop_device()


def test_switch_off_gives_the_bits_of_a_handle_without_the_option():
    """the nested solve of the P2 Rijke p-hierarchy: 12 options (a caller that never heard of opts[12]) against 13 with opts[12] = 0"""
    from test_gpu_p2_prolong import P2_SMOOTHER, device_mesh, rijke_p2_family
    Rm = device_mesh("rijke")
    Ps = Rm.prolongators(to_level=0, order="quad", p_first=True)
    B = G.rhs(Rm.ndof(0, "quad"), 8)
    out = []
    for nopts in (12, 13):
        L = rijke_p2_family(0)
        try:
            fam = L.device()
            c = np.ascontiguousarray(L.coefficients(W340), dtype=np.complex128)
            opts = np.array([0.02, 128, P2_SMOOTHER["jacobi_weight"], 1, 30, 1e8, 64, 0.0, 0.0, 0.0, P2_SMOOTHER["jacobi_weight_post"],
                             P2_SMOOTHER["jacobi_weight_light"], 0.0])
            from wae_amd.nlevp.linopfam import _check_prolongators
            mats = _check_prolongators(Ps, fam.d)
            n = len(mats)
            keep = [(np.ascontiguousarray(P.indptr, dtype=np.int32), np.ascontiguousarray(P.indices, dtype=np.int32), np.ascontiguousarray(P.data)) for P in mats]
            arr = [(C.c_void_p * n)(*[k[j].ctypes.data for k in keep]) for j in range(3)]
            rows, cols = (C.c_int64 * n)(*[P.shape[0] for P in mats]), (C.c_int64 * n)(*[P.shape[1] for P in mats])
            _lib.check(_lib.lib().wae_solver_setup_nested(fam.handle, _lib.zptr(c), opts.ctypes.data_as(C.POINTER(C.c_double)), nopts, n, rows, cols,
                                                          arr[0], arr[1], arr[2]))
            fam.solver_ready, fam.batch = True, 64
            X = fam.solve(c, B, tol=1e-10, maxit=300, strict=False, quiet=True)
            lam, scale = fam.level_weights()
            assert np.all(scale == 1.0) and np.all(lam == 0.0)
            out.append((X.copy(), dict(fam.last_info)))
        finally:
            L._drop_device()
    print(f"P2 Rijke p-hierarchy, 8 columns: {out[0][1]}")
    assert out[0][1]["n_unconverged"] == 0
    assert np.array_equal(out[0][0].view(np.float64).view(np.uint64), out[1][0].view(np.float64).view(np.uint64))
    assert all(out[0][1][k] == out[1][1][k] for k in out[0][1] if k != "seconds")


def spsolve_bound(reference_count, tol=1e-10):
    """The distance to scipy's spsolve that a solve stopped at `tol` may show.  The driver bounds the PRECONDITIONED residual, so
    x - x* = (M^-1 A)^-1 M^-1 (b - A x) and |x - x*| / |x*| <= kappa(M^-1 A) tol.  kappa is taken from the host restatement, which knows
    nothing of the device: it needs `reference_count` iterations for `tol`, a mean contraction q = tol^(1 / count) per iteration, and the
    Krylov rate of an operator of condition kappa is (sqrt(kappa) - 1) / (sqrt(kappa) + 1) = q.  67 iterations: q = 0.709, kappa = 34.5,
    bound 3.5e-9 (measured 7.9e-10).  The check is independent of the device's own cycle: scipy factorises the operator, penalty rows
    of 1e15 included."""
    q = tol ** (1.0 / reference_count)
    return ((1 + q) / (1 - q)) ** 2 * tol


# ---- 3. the solve ----------------------------------------------------------------------------------------------------------------------------
def test_the_hermite_solve_converges(herm_family, herm_terms, reference_count):
    """MI355X: iters_max 71 for both orientations against 67 of the reference restatement"""
    import warnings
    Lp = herm_family
    fam = Lp.ensure_solver()
    d = Lp.size()
    B = G.rhs(d, 8)
    c = np.ascontiguousarray(Lp.coefficients(W340), dtype=np.complex128)
    A = sp.csc_matrix(sum(ck * sp.csr_matrix(t.coeff) for ck, t in zip(c, Lp.terms) if ck != 0))
    lu = spla.splu(A)
    maxit = 4 * reference_count
    for op, name in ((0, "N"), (2, "H")):
        Aop = A if op == 0 else A.conj().T.tocsc()
        with warnings.catch_warnings():
            warnings.simplefilter("error")                            # a stagnation or iteration-limit warning fails the test
            X = fam.solve(c, B, op=op, tol=1e-10, maxit=maxit)
        info, code = dict(fam.last_info), fam.last_code
        Xs = lu.solve(B) if op == 0 else lu.solve(B, trans="H")
        res = B - Aop @ X
        MB = fam.debug_vcycle(c, B, op=op)
        MR = fam.debug_vcycle(c, np.asarray(res, dtype=np.complex128), op=op)
        rho = np.linalg.norm(MR, axis=0) / np.linalg.norm(MB, axis=0)
        dist = np.max(np.linalg.norm(X - Xs, axis=0) / np.linalg.norm(Xs, axis=0))
        print(f"Hermite Rijke, op {name}, 8 columns, tol 1e-10, maxit {maxit} (reference {reference_count}): code {code}, info {info}, iters_max "
              f"{info['iters_max']}, recomputed preconditioned residuals {rho.min():.2e}..{rho.max():.2e}, distance to spsolve {dist:.2e}")
        assert code == 0 and info["n_unconverged"] == 0
        assert info["iters_max"] <= maxit
        assert np.all(rho <= 1e-10), rho
        assert dist <= spsolve_bound(reference_count), (dist, spsolve_bound(reference_count))


# ---- 4. end to end ----------------------------------------------------------------------------------------------------------------------------
def test_householder_on_the_hermite_rijke_family(herm_family, herm_terms):
    """From the passive mode as guess (1709.0640 rad/s, the CPU figure of tests/test_gpu_herm.py).  The reference is the oracle family's
    householder (sparse LU on the CPU), at the tolerance of the P2 counterpart (tests/test_gpu_p2_prolong.py): the iterations stopped at
    1e-11 |w|, the eigenvalues compared to 1e-10 relative.  A step of the oracle (sparse LU of the 11 565 unknowns and its Arnoldi runs)
    takes 3.5 s on the host, so it does not repeat the walk from the passive mode (there it uses all 20 steps: with Y = 1e15 its own
    steps stay at 1e-10 |w|, above the stopping tolerance): it starts from the device's eigenvalue rounded to whole rad/s and converges on
    its own from there, at most 6 steps.  MI355X: device 169.74501497 + 59.01432701i Hz in 6 steps, flag 1; relative difference to the
    oracle's walk from the passive mode 2.2e-11.  The test takes 13 s, nearly all of it the oracle.
    Which mode is found must not hang on the device either: W_ORACLE is what the oracle's own walk from the passive mode returned (20
    steps, 70 s on the host, run once), and the device's eigenvalue is held to it at 1e-8 -- its digits beyond that are the oracle's
    round-off with Y = 1e15, which is what the short walk pins."""
    from oracle import solvers as OS
    from test_gpu_herm import oracle_family
    w0 = 1709.0640
    tol = 1e-11 * abs(w0)
    sol, n, flag = householder(herm_family, w0, maxiter=20, tol=tol)
    w = sol.params["ω"]
    start = complex(round(w.real), round(w.imag))
    solo, no, flago = OS.householder(oracle_family(herm_terms, 1.0, 0.001), start, maxiter=6, tol=tol)
    wo = solo.params["ω"]
    print(f"Hermite Rijke tube: passive mode {w0 / (2 * np.pi):.6f} Hz, device householder {w / (2 * np.pi):.8f} Hz in {n} steps (flag {flag}), "
          f"oracle from {start} {wo / (2 * np.pi):.8f} Hz in {no} steps (flag {flago}), relative difference {abs(w - wo) / abs(wo):.2e}")
    assert flag in (0, 1)
    assert abs(w - W_ORACLE) < 1e-8 * abs(W_ORACLE)                   # the mode the oracle reaches from the passive one, not another
    assert abs(start - w) > 1e-6 * abs(w)
    assert abs(w - wo) < 1e-10 * abs(wo)
