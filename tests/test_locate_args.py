"""CPU tests of the host side of the point locator (helmholtz/locate.py): every argument error is a ValueError raised before the library is
touched, and the new entry points are declared in the header, bound in ctypes and called from Julia."""
import os
import re

import numpy as np
import pytest

import _octoref as O
from wae_amd import _lib
from wae_amd.helmholtz import Locator, locate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["wae_locator_create", "wae_locator_info", "wae_locator_find", "wae_locator_set_p2", "wae_locator_weights", "wae_locator_sample",
         "wae_locator_free"]


@pytest.fixture
def no_library(monkeypatch):
    """any call into the library fails the test: the checks below must come first"""
    def boom():
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "lib", boom)


def bare_locator(name="cube"):
    """a Locator without a device handle: what the argument checks see"""
    pts, tets, _ = O.mesh(name)
    loc = object.__new__(Locator)
    loc._h, loc.device, loc._tets10 = None, 0, None
    loc.points, loc.tets = np.ascontiguousarray(pts), np.ascontiguousarray(tets, dtype=np.int32)
    return loc


def test_constructor_checks_its_arguments_before_the_library(no_library):
    pts, tets, _ = O.mesh("cube")
    for bad in (pts[:, :2], pts.ravel(), np.zeros((0, 3)), pts.astype(complex), np.array([["a"] * 3] * 4)):
        with pytest.raises(ValueError):
            Locator(bad, tets)
    for bad in (tets[:, :3], tets.ravel(), tets.astype(float), np.zeros((0, 4), dtype=np.int32), tets.astype(np.int64) + 2 ** 32):
        with pytest.raises(ValueError):
            Locator(pts, bad)
    for bad in (-1, 1.0, 2.5, None, True, "8"):
        with pytest.raises(ValueError):
            Locator(pts, tets, cell_target=bad)


def test_queries_check_their_arguments_before_the_library(no_library):
    loc = bare_locator()
    X = np.full((5, 3), 0.3)
    V = np.zeros((len(loc.points), 2), dtype=complex)
    for bad in (X[:, :2], X.ravel(), X[None], X.astype(complex), np.zeros((5, 4))):
        with pytest.raises(ValueError):
            loc.find(bad)
        for call in (loc.weights, loc.observers, loc.interpolation, lambda x: loc.sample(V, x)):
            with pytest.raises(ValueError):
                call(bad)
    for tol in (-1e-9, 2e-6, np.nan, None, "0", True):
        with pytest.raises(ValueError):
            loc.find(X, tol=tol)
    for kw in (dict(order="cubic"), dict(order=1), dict(kind="grad"), dict(kind=0), dict(outside="ignore"), dict(outside=None),
               dict(n=[0.0, 0.0, 1.0]),                                        # a direction without kind="n_grad_p"
               dict(kind="n_grad_p"),                                          # ... and the other way round
               dict(kind="n_grad_p", n=[0.0, 1.0]), dict(kind="n_grad_p", n=np.zeros((4, 3))), dict(kind="n_grad_p", n=np.zeros((5, 3, 1))),
               dict(tet=np.zeros(4, dtype=np.int32)), dict(tet=np.zeros(5)), dict(tet=np.zeros((5, 1), dtype=np.int32))):
        with pytest.raises(ValueError):
            loc.weights(X, **kw)
        with pytest.raises(ValueError):
            loc.sample(V, X, **kw)
    for bad in (np.zeros((5, 9), dtype=np.int32), np.zeros((len(loc.tets), 10)), np.zeros(len(loc.tets) * 10, dtype=np.int32)):
        with pytest.raises(ValueError):
            loc.weights(X, order="quad", tets10=bad, tet=np.zeros(5, dtype=np.int32))
    for bad in (V[1:], V[:, :0], V[:, :, None], np.array(["a"] * len(V)), np.zeros(())):
        with pytest.raises(ValueError):
            loc.sample(bad, X, tet=np.zeros(5, dtype=np.int32))
    with pytest.raises(ValueError):
        loc.interpolation(X, order="hermite")
    with pytest.raises(ValueError):
        loc.find(X)                                                          # well-formed, but this object holds no device handle


def test_new_entry_points_are_declared_bound_and_called_from_julia():
    hdr = open(os.path.join(ROOT, "include", "waehip.h")).read()
    jl = open(os.path.join(ROOT, "julia", "WAEHip.jl"), encoding="utf-8").read()
    L = _lib.lib()
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", hdr), n
        assert n in _lib.EXPORTS and f"ccall((:{n}, libwaehip)" in jl, n
        assert getattr(L, n).argtypes is not None, n
    assert [len(getattr(L, n).argtypes) for n in NAMES] == [7, 6, 6, 3, 9, 11, 1]
    for fn in ("function locator(", "function find_tetrahedra(", "get_p(loc::PointLocator", "function get_n_grad_p("):
        assert fn in jl, fn
    # the index bases of the order=:quad path: the locator keeps its tetrahedra 0-based, p2_connectivity takes and returns 1-based ones,
    # wae_locator_set_p2 wants 0-based unknowns
    body = jl[jl.index("function _locator_p2!("):jl.index("function _locator_sample(")]
    assert "p2_connectivity(loc.npoints, loc.tets .+ Int32(1)" in body and "t10_0 = t10 .- Int32(1)" in body
    assert re.search(r":wae_locator_set_p2, libwaehip\).*loc\.handle, ndof, t10_0\)", body)
    assert "t0 = _zero_based(hcat(mesh.tetrahedra...))" in jl[jl.index("function locator("):jl.index("function find_tetrahedra(")]
    assert "Meshutils.jl:800-815" in hdr and locate.Locator is Locator
    mk = open(os.path.join(ROOT, "wavesandeigenvalues.jl_amd", "csrc", "Makefile")).read()
    assert "locate.o" in mk
