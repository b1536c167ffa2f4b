"""Pins tests/_shaperef.py, the CPU reference of the GPU tests of the shape sensitivity (tests/test_gpu_shape_p2.py), without a device:

* in its P1 / per-simplex-c mode it reproduces the oracle's recorded gradients, tests/golden/rijke_shape.npz and rijke_shape_flame.npz
  (oracle/shape.py: full re-discretisations, h = 1e-9), within the 2e-5 * scale of the GPU test of the same fixtures: pairing, sign, the
  reduced flame volume and the normalisation are the oracle's;
* its float64 and its extended-precision evaluation agree on the tiny meshes, for P1 and P2, per-simplex and nodal c;
* it measures the rounding yardstick  e64(mesh, h) = max|ref64 - ref_ext| / scale  that bounds the device in the GPU tests, and prints it.

Measured (h = 1e-5; cases P2 per-simplex c / P2 nodal c / P1 nodal c):
    one 1.3e-11 / 1.5e-11 / 2.2e-11     two 3.2e-11 / 4.1e-11 / 3.8e-11     cube 3.2e-11 / 2.7e-11 / 1.3e-11
    Rijke tube, 16 of the surface points: P2 per-simplex c and P2 nodal c 1.6e-12 (h is 1e-3 of an element there, not 1e-5), with flame 1.0e-12."""
import os

import numpy as np
import pytest

import _shapecases as SC
import _shaperef as S
from oracle import fixtures as F

GOLDEN = F.GOLDEN_DIR


def _normalised(Lo, w0, v, v_adj):
    """v'v = 1, v_adj' L'(w0) v = 1  (shape_sensitivity.jl:40-47)"""
    v0 = v / np.sqrt(np.vdot(v, v))
    saved = (Lo.active, Lo.mode, dict(Lo.params))
    Lo.active, Lo.mode = [Lo.eigval], "all"
    va = v_adj / np.conj(np.vdot(v_adj, Lo(w0, 1) @ v0))
    Lo.active, Lo.mode, Lo.params = saved
    return v0, va


def test_p1_mode_reproduces_the_oracle_fixture():
    m = np.load(os.path.join(GOLDEN, "rijke_mesh.npz"))
    g = np.load(os.path.join(GOLDEN, "rijke_shape.npz"))
    w0 = complex(g["omega"][0])
    u, w = _normalised(F.rijke_family(n=0.0), w0, g["v"], g["v_adj"])
    pb = S.Problem(m["points"], m["tetrahedra"], u, w, w0, "lin", c_tet=m["c_tet"], tris=m["outlet_triangles"], c_tri=m["outlet_c"], Y=1e15)
    # Both sides difference with h = 1e-9 and agree to the rounding of that difference, not better.  Measured: 1.96e-5 of the scale at the
    # worst point (scale 18, the smallest gradient of the fixture), 1e-8 at the outlet points.  The fixture's own distance from the exact
    # central difference (sensitivity_ext) at that point is 2.09e-5: the bound of the GPU test is the rounding of the fixture itself.
    got = S.sensitivity(pb, g["surface_points"], 1e-9)
    want = g["sens"]
    scale = np.abs(want).max(axis=0)
    err = np.abs(got - want).max(axis=0)
    print("passive mode: max err / scale per point", np.max(err / scale), " fixture against the exact central difference:",
          np.max(np.abs(S.sensitivity_ext(pb, g["surface_points"], 1e-9) - want).max(axis=0) / scale))
    assert np.all(err <= 2e-5 * scale + 1e-9)
    assert np.abs(want).max() > 1.0


def test_p1_mode_reproduces_the_oracle_fixture_with_the_flame():
    m = np.load(os.path.join(GOLDEN, "rijke_mesh.npz"))
    fl = np.load(os.path.join(GOLDEN, "rijke_flame.npz"))
    g = np.load(os.path.join(GOLDEN, "rijke_shape_flame.npz"))
    w0 = complex(g["omega"][0])
    n, tau = 1.0, 1e-3
    u, w = _normalised(F.rijke_family(n=n, tau=tau), w0, g["v"], g["v_adj"])
    flame = {"flame_tets": fl["flame_tets"], "ref_tet": int(fl["ref_tet"]), "n_ref": fl["n_ref"], "nglobal_scaled": float(fl["nglobal_scaled"])}
    kw = dict(c_tet=m["c_tet"], tris=m["outlet_triangles"], c_tri=m["outlet_c"], Y=1e15)
    pb = S.Problem(m["points"], m["tetrahedra"], u, w, w0, "lin", flame=flame, coeff=n * np.exp(-1j * w0 * tau), **kw)
    got = S.sensitivity(pb, g["surface_points"], 1e-9)
    want = g["sens"]
    scale = np.abs(want).max(axis=0)
    err = np.abs(got - want).max(axis=0)
    print("active flame: max err / scale per point", np.max(err / scale))
    assert np.all(err <= 2e-5 * scale + 1e-6)
    none = S.sensitivity(S.Problem(m["points"], m["tetrahedra"], u, w, w0, "lin", **kw), g["surface_points"], 1e-9)
    assert np.all(np.abs(none - g["sens_without_flame"]).max(axis=0) <= 2e-5 * np.abs(g["sens_without_flame"]).max(axis=0) + 1e-6)
    assert np.array_equal(np.abs(got - none).max(axis=0) > 0, g["in_flame"])


@pytest.mark.parametrize("case", SC.CASES + ["p1"])
@pytest.mark.parametrize("name", SC.TINY)
def test_float64_and_extended_agree_and_the_yardstick(name, case):
    """The two evaluations share the bookkeeping of `Problem` and nothing else.  At h = 1e-5 the float64 one carries the cancellation of the
    central difference, about eps * |L| / h = 1e-11 relative, the extended one none: they must agree to 1e-9 of the per-point scale (a wrong
    weight, node or sign in either is O(1)), and at h = 1e-2, where truncation is the same for both and rounding is 1e-14, to 1e-12."""
    pb, sp = SC.problem(name, case)
    assert SC.scale_is_not_tiny(pb, S.sensitivity_ext(pb, sp, SC.H))
    for h, tol in ((SC.H, 1e-9), (1e-2, 1e-12)):
        w64, wext = S.sensitivity(pb, sp, h), S.sensitivity_ext(pb, sp, h)
        e64 = S.yardstick(w64, wext)
        print(f"e64({name}, {case}, h = {h:g}) = {e64:.3e}")
        assert e64 <= tol


def test_flame_float64_and_extended_agree_on_the_rijke_points():
    pb, sp = SC.flame_problem()
    w64, wext = S.sensitivity(pb, sp, SC.H), S.sensitivity_ext(pb, sp, SC.H)
    e64 = S.yardstick(w64, wext)
    print(f"e64(rijke flame points, h = {SC.H:g}) = {e64:.3e}")
    assert e64 <= 1e-9
