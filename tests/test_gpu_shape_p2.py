"""GPU tests (-m gpu) of the discrete-adjoint shape sensitivity for P2 elements and for a nodal speed of sound -- wae_p2_shape_sensitivity,
wae_p1_shape_sensitivity_cpoint, wae_p2_shape_sensitivity_cpoint, wae_p2_shape_sensitivity_flame through helmholtz/assemble.py and
helmholtz/shape.py -- against tests/_shaperef.py (pinned by tests/test_shape_ref.py; cases and shared references: tests/_shapecases.py).

Bounds.  The kernels only contract, so wherever no eigenpair is needed random complex vectors go in as v_ext=.  At h = 1e-5 the device must
be within 10 * e64 + 1e-13 of the reference, per point and relative to max|want| of that point: e64 is the distance of the float64 restatement
from the extended-precision evaluation of the same central difference, measured on the CPU when the references are built (tiny meshes:
the extended evaluation is the reference, all points; Rijke tube: the float64 evaluation is the reference and e64 comes from the extended
route on 16 of the 783 surface points; flame: extended route on all 14 points).  The factor 10 covers another order of operations and
fused multiply-adds; a logic error (sign, missing pair, wrong node or weight) is O(1) in that unit.  Measured e64 (tests/test_shape_ref.py):
    one 1.3e-11 / 1.5e-11 / 2.2e-11   two 3.2e-11 / 4.1e-11 / 3.8e-11   cube 3.2e-11 / 2.7e-11 / 1.3e-11   (P2 c per simplex / P2 nodal c / P1 nodal c)
    Rijke tube 1.6e-12 (per simplex), 1.6e-12 (nodal), with the flame 1.0e-12  -- there h = 1e-5 is 1e-3 of an element, not 1e-5 of it.
Measured on one MI355X the device lies at 0.5 - 1.7 e64 in every case, and at 7e-8 - 4e-7 of the scale at h = 1e-9.
At the default h = 1e-9 the bound is the 2e-5 * scale of the P1 test (tests/test_gpu_parity.py), for the reason given there: both sides then
agree to the rounding of that difference, not better.  The end-to-end bounds 2e-3 (h = 1e-6) and 2e-2 (h = 1e-7, flame) are those of the two
P1 tests of the same cross-check and rest on the same second-order term of the linearised family."""
import os

import numpy as np
import pytest

import _shapecases as SC
import _shaperef as S
from wae_amd import _lib
from wae_amd.helmholtz import shape as SH
from wae_amd.helmholtz.assemble import (assemble_p1, assemble_p1_boundary, assemble_p2, assemble_p2_boundary, assemble_p2_flame,
                                        discrete_adjoint_shape_sensitivity)
from wae_amd.helmholtz.family import helmholtz_family
from wae_amd.nlevp import Solution, householder

pytestmark = pytest.mark.gpu


def device(pb, sp, h=SC.H, bnd=True, **kw):
    """the product on the inputs of a _shaperef.Problem"""
    sol = Solution({"ω": pb.omega}, None, None, "ω")
    flame = None if pb.flame is None else {**pb.flame, "coeff": pb.coeff}
    return discrete_adjoint_shape_sensitivity(pb.points, pb.tets, pb.c_tet, sp, sol, None, bnd_tris=pb.tris if bnd else None, bnd_c=pb.c_tri if bnd else None,
                                              Y=pb.Y, h=h, v_ext=(pb.u, pb.w), order="lin" if pb.order == 1 else "quad", c_point=pb.c_point,
                                              **{"flame": flame, **kw})


def worst(got, want):
    """max over the points of |got - want| / max|want of the point|"""
    return float(np.max(np.abs(got - want).max(axis=0) / np.abs(want).max(axis=0)))


# ---- 1. parity with the reference on the tiny meshes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SC.CASES)
@pytest.mark.parametrize("name", SC.TINY)
def test_parity_with_the_reference(name, case):
    pb, sp = SC.problem(name, case)
    _, want, e64 = SC.references(name, case)
    assert SC.scale_is_not_tiny(pb, want)
    got = device(pb, sp)
    err = worst(got, want)
    print(f"{name} {case}: h = {SC.H:g}: device {err:.3e}, e64 {e64:.3e}, bound {10 * e64 + SC.EPS:.3e}")
    assert err <= 10 * e64 + SC.EPS
    want9 = S.sensitivity_ext(pb, sp, 1e-9)
    err9 = worst(device(pb, sp, h=1e-9), want9)
    print(f"{name} {case}: h = 1e-9: device {err9:.3e} (bound 2e-5)")
    assert err9 <= 2e-5
    assert np.array_equal(device(pb, sp), got)                                            # the same bits on every call


# ---- 2. Rijke tube: several blocks, a launch tail ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["p2", "p2_nodal"])
def test_rijke_tube_all_surface_points(case):
    pb, sp = SC.rijke_problem(case)
    faces, _ = SH.boundary_triangles(pb.tets)
    assert np.array_equal(SH.get_surface_points(faces, pb.tets)[0], sp)
    npair = int(np.isin(pb.tets, sp).sum())
    assert npair > 4 * 256 and npair % 256 != 0 and (3 * npair) % 256 != 0, npair
    want, e64 = SC.rijke_references(case)
    got = device(pb, sp)
    err = worst(got, want)
    print(f"rijke {case}: {len(sp)} points, {npair} pairs: device {err:.3e}, e64 {e64:.3e}, bound {10 * e64 + SC.EPS:.3e}")
    assert np.all(np.abs(want).max(axis=0) > 0)
    assert err <= 10 * e64 + SC.EPS
    assert np.array_equal(device(pb, sp), got)


# ---- 3. operator identity against the device assembly of the whole mesh -------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["p2", "p2_nodal"])
def test_operator_identity_against_the_assembly(case):
    """independent of the pair lists: -w^H [om^2 (M+ - M-) + (K+ - K-) + om Y (C+ - C-)] u / (2h) with the matrices of assemble_p2 /
    assemble_p2_boundary of the WHOLE cube at +-h.  Points: the corner 0, the midpoint (0, 0, 1/2) of a cube edge, the centre (1/2, 1/2, 1) of
    the top face (the one with boundary triangles)."""
    pb, _ = SC.problem("cube", case)
    _, _, e64 = SC.references("cube", case)
    pick = np.array([0, 1, 14])
    assert np.allclose(pb.points[pick], [[0, 0, 0], [0, 0, 0.5], [0.5, 0.5, 1.0]])
    got = device(pb, pick)
    want = np.zeros_like(got)
    for k, p in enumerate(pick):
        for crd in range(3):
            L = []
            for d in (SC.H, -SC.H):
                ph = pb.points.copy()
                ph[p, crd] += d
                M, K = assemble_p2(ph, pb.tets, pb.c_tet, c_point=pb.c_point)
                L.append(pb.omega ** 2 * M + K + pb.omega * pb.Y * assemble_p2_boundary(ph, pb.tets, pb.tris, pb.c_tri, c_point=pb.c_point))
            want[crd, k] = -np.vdot(pb.w, (L[0] - L[1]) @ pb.u) / (2 * SC.H)
    err = worst(got, want)
    print(f"cube {case}: against the assembly: {err:.3e}, e64 {e64:.3e}")
    assert SC.scale_is_not_tiny(pb, want)
    assert err <= 10 * e64 + SC.EPS


# ---- 4. flame ---------------------------------------------------------------------------------------------------------------------------------
def test_flame_part_on_the_rijke_tube():
    pb, sp = SC.flame_problem()
    assert len(sp) == 14 and len(set(sp.tolist())) == 14
    want = S.sensitivity(pb, sp, SC.H)
    e64 = S.yardstick(want, S.sensitivity_ext(pb, sp, SC.H))
    plain = S.Problem(pb.points, pb.tets, pb.u, pb.w, pb.omega, "quad", c_tet=pb.c_tet, c_tri=pb.c_tri, tris=pb.tris, Y=pb.Y)
    want_plain = S.sensitivity(plain, sp, SC.H)
    got, none = device(pb, sp), device(pb, sp, flame=None)
    err, err0 = worst(got, want), worst(none, want_plain)
    print(f"flame: device {err:.3e}, without flame {err0:.3e}, e64 {e64:.3e}, bound {10 * e64 + SC.EPS:.3e}")
    assert err <= 10 * e64 + SC.EPS and err0 <= 10 * e64 + SC.EPS
    has = np.abs(want - want_plain).max(axis=0) > 0
    assert has.sum() >= 8 and (~has).sum() >= 2                                            # ... and two vertices of the reference tetrahedron touch no flame tetrahedron
    assert np.array_equal(np.abs(got - none).max(axis=0) > 0, has)
    part = np.abs(want - want_plain).max(axis=0)
    assert np.all(part[has] > 1e-3 * np.abs(want).max(axis=0)[has])                        # the flame term is a real share of the gradient there
    assert np.array_equal(device(pb, sp), got)


# ---- 5. end to end: the reference's own cross-check -------------------------------------------------------------------------------------------
def test_p2_adjoint_gradient_against_the_re_solved_eigenvalue():
    """nev = 1: the device-resident iteration of householder.  With the cross-check's default nev = 3 the block shift-invert solves at the
    eigenvalue itself do not converge on the P2 family (8 columns unconverged, relative residual 5e-4) and householder gives up with flag -4;
    forward_finite_differences_shape_sensitivity now raises in that case instead of returning zeros.  maxiter = 3: the re-solve starts at the
    eigenvalue and its second step already moves it by less than 1e-10."""
    pts, tets, tris, c_tet, c_tri = SC.mesh("rijke")
    fl = SC.flame_inputs()
    M, K = assemble_p2(pts, tets, c_tet)
    t = {"M": M, "K": K, "C": assemble_p2_boundary(pts, tets, tris, c_tri),
         "Q": assemble_p2_flame(pts, tets, fl["flame_tets"], fl["ref_tet"], fl["x_ref"], fl["n_ref"], fl["nglobal_scaled"])[0]}
    Lp = helmholtz_family(t, n=1.0, tau=0.001)
    Lp.solver_ref = 340 * 2 * np.pi
    sol, n, flag = householder(Lp, 1066.8 + 370.8j, maxiter=10, tol=1e-9)           # the active-flame mode that mslp finds from 340 Hz (tests/test_gpu_p2.py)
    assert flag == 1
    w0 = complex(sol.params["ω"])
    assert abs(w0 - (1066.7823089382373 + 370.75427745433393j)) < 1e-6
    g = np.load(os.path.join(SC.GOLDEN, "rijke_shape_flame.npz"))
    wall = g["surface_points"][g["in_flame"] & ~g["in_ref"]][0]
    outlet = np.unique(tris)[0]
    Lp.solver_ref = w0.real
    kw = dict(bnd_tris=tris, bnd_c=c_tri, flame=fl, order="quad")
    for p, h, bound in ((outlet, 1e-6, 2e-3), (wall, 1e-7, 2e-2)):
        adj = SH.discrete_adjoint_shape_sensitivity(pts, tets, c_tet, [p], sol, Lp, Y=1e15, **kw)
        fd = SH.forward_finite_differences_shape_sensitivity(pts, tets, c_tet, [p], Lp, sol, h=h, nev=1, maxiter=3, **kw)
        scale = np.abs(adj).max()
        gap = np.abs(fd - adj).max() / scale
        print(f"P2 end to end: omega {w0!r}, point {p}, h = {h:g}: |fd - adj| / scale = {gap:.3e} (bound {bound:g}); adj {adj.ravel()}, fd {fd.ravel()}")
        assert scale > 1.0
        assert gap <= bound
    Lp._drop_device()


def test_p1_nodal_adjoint_gradient_against_the_re_solved_eigenvalue():
    """passive mode, speed of sound given on the points: cold below the flame sheet, hot above, linear in between"""
    pts, tets, tris, _, _ = SC.mesh("rijke")
    c_point = np.interp(pts[:, 2], [-0.02, 0.02], [347.2, 694.4])
    M, K = assemble_p1(pts, tets, c_point=c_point)
    Lp = helmholtz_family({"M": M, "K": K, "C": assemble_p1_boundary(pts, tris, c_point=c_point)}, n=0.0, flame=False)
    Lp.solver_ref = 270 * 2 * np.pi
    sol, n, flag = householder(Lp, 270 * 2 * np.pi, maxiter=20, tol=1e-9)
    w0 = complex(sol.params["ω"])
    # the oracle's householder on the matrices of tests/_nodalref.py (CPU, tol 1e-11): 1735.1616536712256 + 7e-13i
    assert flag == 1 and abs(w0 - 1735.1616536712256) < 1e-6, (w0, n, flag)
    p = np.unique(tris)[0]
    kw = dict(bnd_tris=tris, c_point=c_point)
    adj = SH.discrete_adjoint_shape_sensitivity(pts, tets, None, [p], sol, Lp, Y=1e15, **kw)
    fd = SH.forward_finite_differences_shape_sensitivity(pts, tets, None, [p], Lp, sol, h=1e-6, nev=1, **kw)
    scale = np.abs(adj).max()
    gap = np.abs(fd - adj).max() / scale
    print(f"P1 nodal end to end: omega {w0!r}, point {p}: |fd - adj| / scale = {gap:.3e} (bound 2e-3); adj {adj.ravel()}, fd {fd.ravel()}")
    assert scale > 1.0
    assert gap <= 2e-3
    Lp._drop_device()


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------------------
def raw(pb, sp, order, outputs=False, **over):
    """the C entry behind `device`, with single arguments replaced: returns the code, or (code, out_t, out_s)"""
    import ctypes as C
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    a = dict(points=np.ascontiguousarray(pb.points), tets=pb.tets.astype(np.int32), tris=pb.tris.astype(np.int32), c_point=pb.c_point,
             pair_pt_t=np.array([pb.tets[0, 0]], dtype=np.int32), pair_tet=np.zeros(1, dtype=np.int32),
             pair_pt_s=np.array([pb.tris[0, 0]], dtype=np.int32), pair_tri=np.zeros(1, dtype=np.int32), h=1e-5, nv=len(pb.u), npoints=len(pb.points))
    a.update(over)
    P = lambda x, t: None if x is None else np.ascontiguousarray(x).ctypes.data_as(t)          # noqa: E731
    keep = [np.ascontiguousarray(a[k]) for k in ("points", "tets", "tris", "pair_pt_t", "pair_tet", "pair_pt_s", "pair_tri")]
    out_t, out_s = np.full(3, 7 + 7j), np.full(3, 7 + 7j)                              # sentinels: the library writes every entry
    om = np.array([1.0, 0.1])
    u, w = np.ascontiguousarray(pb.u), np.ascontiguousarray(pb.w)
    nodal = a["c_point"] is not None
    cpt = None if not nodal else np.ascontiguousarray(a["c_point"], dtype=np.float64)
    L = _lib.lib()
    entry = getattr(L, f"wae_{'p2' if order == 'quad' else 'p1'}_shape_sensitivity" + ("_cpoint" if nodal else ""))
    args = [0, a["npoints"], P(keep[0], dp), P(keep[1], ip), P(cpt, dp), len(keep[3]), P(keep[3], ip), P(keep[4], ip), P(keep[2], ip)]
    if not nodal:
        args.append(None)
    args += [len(keep[5]), P(keep[5], ip), P(keep[6], ip), len(keep[1]), len(keep[2]), P(om, dp), P(om, dp)]
    if order == "quad":
        args.append(a["nv"])
    args += [P(u.view(np.float64), dp), P(w.view(np.float64), dp), a["h"], P(out_t.view(np.float64), dp), P(out_s.view(np.float64), dp)]
    code = entry(*args)
    return (code, out_t, out_s) if outputs else code


@pytest.mark.parametrize("case", SC.CASES)
def test_refusals(case):
    pb, sp = SC.problem("cube", case)
    order = "lin" if pb.order == 1 else "quad"
    npts, nt, ns = len(pb.points), len(pb.tets), len(pb.tris)
    bad_tets, bad_tris = pb.tets.copy(), pb.tris.copy()
    bad_tets[3, 2] = npts
    bad_tris[1, 0] = -1
    cases = [dict(tets=bad_tets), dict(tris=bad_tris), dict(pair_tet=np.array([nt], dtype=np.int32)), dict(pair_tet=np.array([-1], dtype=np.int32)),
             dict(pair_pt_t=np.array([npts], dtype=np.int32)), dict(pair_tri=np.array([ns], dtype=np.int32)),
             dict(pair_pt_s=np.array([-2], dtype=np.int32)), dict(h=0.0), dict(h=-1e-5), dict(h=np.inf), dict(h=np.nan)]
    if order == "quad":
        cases += [dict(nv=len(pb.u) - 1), dict(nv=len(pb.u) + 1), dict(nv=npts)]
    if pb.c_point is not None:
        for v in (np.nan, np.inf):
            c = pb.c_point.copy()
            c[5] = v
            cases.append(dict(c_point=c))
    assert raw(pb, sp, order) == _lib.WAE_OK
    for over in cases:
        code = raw(pb, sp, order, **over)
        msg = _lib.lib().wae_last_error().decode()
        assert code == _lib.WAE_ERR_INVALID and msg, (over, code, msg)
        with pytest.raises(_lib.WaeError):
            _lib.check(code)
        assert raw(pb, sp, order) == _lib.WAE_OK                                          # a valid call still works
    # a pair whose point is no corner of its simplex contributes zero, and empty pair lists return zeros
    far = int(np.setdiff1d(np.arange(npts), pb.tets[0])[0])
    far_s = int(np.setdiff1d(np.arange(npts), pb.tris[0])[0])
    code, out_t, out_s = raw(pb, sp, order, outputs=True)
    assert code == _lib.WAE_OK and np.all(np.abs(out_t) > 0) and np.all(out_t != 7 + 7j) and np.all(out_s != 7 + 7j)
    code, out_t, out_s = raw(pb, sp, order, outputs=True, pair_pt_t=np.array([far], dtype=np.int32), pair_pt_s=np.array([far_s], dtype=np.int32))
    assert code == _lib.WAE_OK and np.all(out_t == 0) and np.all(out_s == 0)
    empty = np.zeros(0, dtype=np.int32)
    none_kw = dict(pair_pt_t=empty, pair_tet=empty, pair_pt_s=empty, pair_tri=empty)
    assert raw(pb, sp, order, **none_kw) == _lib.WAE_OK
    if order == "quad":                                                                   # nv is checked even when nothing is launched
        assert raw(pb, sp, order, nv=len(pb.u) + 1, **none_kw) == _lib.WAE_ERR_INVALID
    none = device(pb, np.zeros(0, dtype=np.int64))
    assert none.shape == (3, 0)
    inner = np.array([13])                                                                # the cube's centre: tetrahedra, no boundary triangle
    assert np.array_equal(device(pb, inner), device(pb, inner, bnd=False))


def raw_flame(pb, **over):
    """wae_p2_shape_sensitivity_flame with one pair of each list and single arguments replaced: returns the code"""
    import ctypes as C
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    fl = pb.flame
    t0, ref = int(fl["flame_tets"][0]), int(fl["ref_tet"])
    a = dict(pair_pt=int(pb.tets[t0, 0]), pair_tet=t0, ref_tet=ref, pair_pt_r=int(pb.tets[ref, 0]), h=1e-5, nv=len(pb.u))
    a.update(over)
    pts, tets = np.ascontiguousarray(pb.points), np.ascontiguousarray(pb.tets, dtype=np.int32)
    pp, pt, pr = (np.array([a[k]], dtype=np.int32) for k in ("pair_pt", "pair_tet", "pair_pt_r"))
    xr, nr = np.ascontiguousarray(fl["x_ref"], dtype=np.float64), np.ascontiguousarray(fl["n_ref"], dtype=np.float64)
    u, w = np.ascontiguousarray(pb.u), np.ascontiguousarray(pb.w)
    det_pm, ssum, g_pm, g0 = np.zeros(6), np.zeros(2), np.zeros(12), np.zeros(2)
    return _lib.lib().wae_p2_shape_sensitivity_flame(
        0, len(pts), pts.ctypes.data_as(dp), len(tets), tets.ctypes.data_as(ip), 1, pp.ctypes.data_as(ip), pt.ctypes.data_as(ip), a["ref_tet"], 1,
        pr.ctypes.data_as(ip), xr.ctypes.data_as(dp), nr.ctypes.data_as(dp), a["nv"], u.view(np.float64).ctypes.data_as(dp),
        w.view(np.float64).ctypes.data_as(dp), a["h"], det_pm.ctypes.data_as(dp), ssum.ctypes.data_as(dp), g_pm.ctypes.data_as(dp), g0.ctypes.data_as(dp))


def test_flame_refusals():
    pb, sp = SC.flame_problem()
    nt, npts = len(pb.tets), len(pb.points)
    assert raw_flame(pb) == _lib.WAE_OK
    for over in (dict(ref_tet=-1), dict(ref_tet=nt), dict(pair_tet=nt), dict(pair_tet=-1), dict(pair_pt=npts), dict(pair_pt_r=-1), dict(h=0.0),
                 dict(h=np.nan), dict(h=np.inf), dict(nv=len(pb.u) - 1), dict(nv=npts)):
        code = raw_flame(pb, **over)
        msg = _lib.lib().wae_last_error().decode()
        assert code == _lib.WAE_ERR_INVALID and msg, (over, code, msg)
        with pytest.raises(_lib.WaeError):
            _lib.check(code)
        assert raw_flame(pb) == _lib.WAE_OK                                               # a valid call still works
    # points that touch no flame tetrahedron and are no vertex of the reference tetrahedron: both pair lists empty, the flame part is zero
    lone = sp[-2:]
    assert np.array_equal(device(pb, lone), device(pb, lone, flame=None))
