"""CPU tests of the Hermite rows of the point locator: tests/_hermlocref.py (the reference of tests/test_gpu_herm_locate.py) reproduces
cubics, its transliteration of the device formula agrees with it and loses that under three seeded defects; the argument checks of
helmholtz/locate.py for order="herm" come before the library; the new C entry is exported, declared, bound and called from Julia."""
import os
import re

import numpy as np
import pytest

import _hermlocref as HL
import _hermref as H
import _octoref as O
from wae_amd import _lib
from wae_amd.helmholtz import Locator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MESHES = ["one", "sheared", "cube"]
GPU_MESHES = ["two", "sheared", "cube", "rijke"]
LD = np.longdouble


def points_in(pts, tets, seed=3):
    """per tetrahedron: its vertices, edge midpoints, face centroids, centroid and four random interior points -> (X, tet)"""
    rng = np.random.default_rng(seed)
    lam = [np.eye(4)[k] for k in range(4)]
    lam += [(np.eye(4)[i] + np.eye(4)[j]) / 2 for i in range(4) for j in range(i + 1, 4)]
    lam += [(1 - np.eye(4)[k]) / 3 for k in range(4)] + [np.full(4, 0.25)]
    lam = np.concatenate([np.array(lam), rng.dirichlet(np.ones(4), 4)])
    X = np.einsum("qk,tkd->tqd", lam, pts[tets]).reshape(-1, 3)
    return X, np.repeat(np.arange(len(tets)), len(lam))


def reproduction(name, rows_of, dtype):
    """the largest |rows . herm_dofs(cubic) - cubic| / sum |row| |dofs| over three cubics, both kinds and all points of points_in"""
    pts, tets, tris = O.mesh(name)
    X, t = points_in(pts, tets)
    faces, t20, _, ndof = H.connectivity(len(pts), tets, tris)
    worst = 0.0
    for k in range(3):
        f, grad = HL.mesh_cubic(pts, k)
        u = H.dofs(pts.astype(dtype), faces, tris, f, grad)
        assert u.shape == (ndof,) and u.dtype == dtype
        for kind in (0, 1):
            w = rows_of(pts, tets, X, t, kind, HL.N_DIR)
            got = np.sum(w.astype(dtype) * u[t20[t]], axis=1)
            want = f(X.astype(dtype)) if kind == 0 else grad(X.astype(dtype)) @ HL.N_DIR.astype(dtype)
            mag = np.sum(np.abs(w.astype(dtype)) * np.abs(u[t20[t]]), axis=1)
            worst = max(worst, float(np.max(np.abs(got - want) / mag)))
    return worst


def test_the_meshes_hold_a_reflected_tetrahedron_with_a_non_symmetric_jacobian():
    pts, tets, _ = O.mesh("sheared")
    P = pts[tets]
    J = np.transpose(P[:, :3] - P[:, 3:4], (0, 2, 1))
    bad = (np.linalg.det(J) < 0) & (np.abs(J - np.transpose(J, (0, 2, 1))).max(axis=(1, 2)) > 0.1)
    assert bad.sum() >= 10


@pytest.mark.parametrize("name", MESHES)
def test_longdouble_rows_reproduce_cubics(name):
    """rows . herm_dofs(cubic) = p(x) and = n . grad p(x) with the numbering of _hermref.connectivity.  The rows come out of a 20 x 20
    inverse refined in longdouble (eps 1e-19 times a condition of up to 1e4 in the scaled coordinates): 1e-15 of sum |w| |u|, four digits
    below what float64 rows can reach."""
    e = reproduction(name, lambda *a: HL.weight_rows_herm(*a, dtype=LD), LD)
    print(f"{name}: longdouble rows reproduce the cubics to {e:.1e} of sum |w| |u|")
    assert e <= 1e-15


@pytest.mark.parametrize("name", MESHES)
def test_float64_reference_and_transliteration_reproduce_cubics(name):
    """the same in float64: the reference rows to 1e-11 of sum |w| |u| (eps 2e-16 times the condition of the 20 x 20 inverse, up to 1e4, and a
    factor 5), the transliteration of the device formula to 1e-12 (eps times kappa(J) <= 30 on these meshes times the 20 terms of a
    function with coefficients up to 33)"""
    e1 = reproduction(name, lambda *a: HL.weight_rows_herm(*a, dtype=np.float64), np.float64)
    e2 = reproduction(name, HL.device_rows_herm, np.float64)
    print(f"{name}: float64 reference {e1:.1e}, transliteration {e2:.1e}")
    assert e1 <= 1e-11 and e2 <= 1e-12


@pytest.mark.parametrize("defect", ["transposed", "lambda3", "faces"])
def test_seeded_defects_break_the_reproduction(defect):
    """each defect in the transliteration misses the reproduction by more than 1e-6 of sum |w| |u| (in fact by O(1)) on `one` and on `sheared`,
    whose reflected tetrahedra have a non-symmetric J"""
    errs = {name: reproduction(name, lambda *a: HL.device_rows_herm(*a, defect=defect), np.float64) for name in MESHES}
    print(defect, {k: f"{v:.1e}" for k, v in errs.items()})
    assert errs["sheared"] > 1e-6 and errs["one"] > 1e-6
    assert max(errs.values()) > 1e-3


def test_measured_ratio_of_the_transliteration():
    """the figure that sets the tolerance of tests/test_gpu_herm_locate.py::test_weight_rows: |transliteration - longdouble| / (eps kappa s)
    on the located points of that test.  Measured here: two 1.68, sheared 3.08, cube 2.44, rijke 4.01."""
    r = {name: HL.measured_herm_ratio(name) for name in GPU_MESHES}
    print("measured_herm_ratio:", {k: round(v, 2) for k, v in r.items()})
    import test_gpu_herm_locate as G
    assert max(r.values()) <= G.C_MEASURED                               # the constant written into the GPU test is not below the measurement
    assert G.C_WEIGHTS == 8 * G.C_MEASURED


# ---- the argument checks of helmholtz/locate.py ----------------------------------------------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    """any call into the library fails the test: the checks below must come first"""
    def boom():
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "lib", boom)


def bare_locator(name="cube"):
    """a Locator without a device handle and without the attributes this order adds: what the argument checks see"""
    pts, tets, _ = O.mesh(name)
    loc = object.__new__(Locator)
    loc._h, loc.device, loc._tets10 = None, 0, None
    loc.points, loc.tets = np.ascontiguousarray(pts), np.ascontiguousarray(tets, dtype=np.int32)
    return loc


def test_herm_calls_check_their_arguments_before_the_library(no_library):
    loc = bare_locator()
    pts, tets, tris = O.mesh("cube")
    _, t20, _, ndof = H.connectivity(len(pts), tets, tris)
    X = np.full((5, 3), 0.3)
    V = np.zeros((ndof, 2), dtype=complex)
    t5 = np.zeros(5, dtype=np.int32)
    with pytest.raises(ValueError, match="herm_connectivity"):
        loc.weights(X, "herm", tet=t5)
    with pytest.raises(ValueError, match="herm_connectivity"):
        loc.sample(V, X, "herm", tet=t5)
    with pytest.raises(ValueError, match="herm_connectivity"):
        loc.observers(X, "herm")
    with pytest.raises(ValueError, match="herm_connectivity"):
        loc.interpolation(X, order="herm")
    with pytest.raises(ValueError, match="herm_connectivity"):
        loc.herm_transfer(V, pts, tets, tris)
    for bad in (t20[:, :19], t20[1:], t20.ravel(), t20.astype(float), t20[None], -t20 - 1):
        with pytest.raises(ValueError, match="tets20"):
            loc.weights(X, "herm", tet=t5, tets20=bad)
        with pytest.raises(ValueError, match="tets20"):
            loc.sample(V, X, "herm", tet=t5, tets20=bad)
        with pytest.raises(ValueError, match="tets20"):
            loc.interpolation(X, order="herm", tets20=bad)
        with pytest.raises(ValueError, match="tets20"):
            loc.herm_transfer(V, pts, tets, tris, tets20=bad)
    for bad in (V[1:], np.zeros((ndof + 1, 1)), np.zeros(len(pts)), V[:, :, None], np.array(["a"] * ndof)):
        with pytest.raises(ValueError, match="V "):
            loc.sample(bad, X, "herm", tet=t5, tets20=t20)
        with pytest.raises(ValueError, match="V "):
            loc.herm_transfer(bad, pts, tets, tris, tets20=t20)
    for bad in (tets[:, :3], tets.astype(float), tets.ravel(), np.zeros((0, 4), dtype=np.int32), tets + len(pts)):
        with pytest.raises(ValueError):
            loc.herm_transfer(V, pts, bad, tris, tets20=t20)
    for bad in (pts[:, :2], pts.astype(complex)):
        with pytest.raises(ValueError):
            loc.herm_transfer(V, bad, tets, tris, tets20=t20)
    with pytest.raises(ValueError):
        loc.herm_transfer(V, pts, tets, tris[:, :2], tets20=t20)
    # the checks that the other orders had still hold with the new order and keyword
    for kw in (dict(kind="grad"), dict(outside="ignore"), dict(n=[0.0, 0.0, 1.0]), dict(kind="n_grad_p"), dict(tet=np.zeros(4, dtype=np.int32))):
        with pytest.raises(ValueError):
            loc.weights(X, "herm", tets20=t20, **kw)
    with pytest.raises(ValueError, match="closed"):
        loc.weights(X, "herm", tet=t5, tets20=t20)                          # well-formed: only now the handle is asked for
    # the lin path reads no attribute of the Hermite order: it gets as far as the library
    assert not hasattr(loc, "_tets20")
    with pytest.raises(AssertionError, match="the library was called"):
        loc.weights(X, "lin", tet=t5)


def test_the_new_entry_is_exported_declared_bound_and_called_from_julia():
    hdr = open(os.path.join(ROOT, "include", "waehip.h")).read()
    jl = open(os.path.join(ROOT, "julia", "WAEHip.jl"), encoding="utf-8").read()
    n = "wae_hermite_locator_set"
    assert n in _lib.EXPORTS
    L = _lib.lib()
    assert len(getattr(L, n).argtypes) == 3
    assert re.search(r"\bint\s+" + n + r"\s*\(void \*locator, int64_t ndof, const int32_t \*tets20\);", hdr)
    assert f"ccall((:{n}, libwaehip), Cint, (Ptr{{Cvoid}}, Int64, Ptr{{Int32}})" in jl
    for fn in ("function locator_set_herm!(", "order == :herm"):
        assert fn in jl, fn
    body = jl[jl.index("function locator_set_herm!("):]
    body = body[:body.index("\nend\n")]
    assert "t20_0 = " in body and ".- Int32(1)" in body                     # 1-based in, 0-based to the library
    assert L.wae_hermite_locator_set(None, 0, None) == _lib.WAE_ERR_INVALID and L.wae_last_error().decode() == "null handle"
