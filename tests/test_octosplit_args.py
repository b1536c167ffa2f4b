"""CPU tests of the host side of the uniform mesh refinement (helmholtz/refine.py): the argument checks raise ValueError before any library
call, the carriers that need no device (fields, domains, the reference tetrahedron) agree with tests/_octoref.py, and the new entry points
are declared in the header, bound in ctypes and called from Julia."""
import os
import re

import numpy as np
import pytest

import _octoref as O
from wae_amd import _lib
from wae_amd.helmholtz import RefinedMesh, octosplit, refine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["wae_octosplit", "wae_octosplit_info", "wae_octosplit_get", "wae_octosplit_prolong", "wae_octosplit_free"]


@pytest.fixture
def no_library(monkeypatch):
    """any call into the library fails the test: the checks below must come first"""
    def boom():
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "lib", boom)


def host_mesh(name, levels=2):
    """a RefinedMesh without a device handle, from the reference's arrays"""
    H = O.refine(*O.mesh(name), levels=levels)
    rest = lambda f: [None] + [getattr(L, f) for L in H[1:]]
    return H, RefinedMesh(None, 0, [L.points for L in H], [L.tets for L in H], [L.tris for L in H], rest("parents"), rest("tet_labels"),
                          rest("tri_labels"))


def test_octosplit_checks_its_arguments_before_the_library(no_library):
    pts, tets, tris = O.mesh("cube")
    for bad in (pts[:, :2], pts.ravel(), np.zeros((0, 3))):
        with pytest.raises(ValueError):
            octosplit(bad, tets, tris)
    for bad in (tets[:, :3], tets.ravel(), tets.astype(float), np.zeros((0, 4), dtype=np.int32), tets.astype(np.int64) + 2 ** 32):
        with pytest.raises(ValueError):
            octosplit(pts, bad, tris)
    for bad in (tris[:, :2], tris.ravel(), tris.astype(float)):
        with pytest.raises(ValueError):
            octosplit(pts, tets, bad)
    for bad in (0, -1, 1.0, 1.5, None, True, "2"):
        with pytest.raises(ValueError):
            octosplit(pts, tets, tris, levels=bad)


def test_prolong_checks_its_arguments_before_the_library(no_library):
    H, R = host_mesh("two")
    n0, n1 = len(H[0].points), len(H[1].points)
    for frm, to in ((1, 1), (2, 1), (1, 0), (0, 0), (2, 2), (2, -1), (-1, -1), (0, 3), (-4, 1), (3, 4)):
        with pytest.raises(ValueError):
            R.prolong(np.zeros(len(H[min(max(frm, 0), 2)].points)), frm, to)
    for X in (np.zeros(n0 + 1), np.zeros((n0, 2, 2)), np.zeros(()), np.zeros((n0, 0)), np.array(["a"] * n0), np.zeros((2, n0))):
        with pytest.raises(ValueError):
            R.prolong(X)
    with pytest.raises(ValueError):
        R.prolong(np.zeros(n0), 1, 2)                                    # level 1 has n1 points
    with pytest.raises(ValueError):
        R.prolong(np.zeros(n1), 1, 2)                                    # well-formed, but this object holds no device levels


@pytest.mark.parametrize("name", ["two", "cube", "rijke"])
def test_host_carriers_agree_with_the_reference(name):
    H, R = host_mesh(name)
    rng = np.random.default_rng(3)
    c_tet, c_tri = rng.standard_normal(len(H[0].tets)), rng.standard_normal((len(H[0].tris), 2))
    some = rng.permutation(len(H[0].tets))[:max(1, len(H[0].tets) // 7)]
    for to in (1, 2, -1):
        lvl = to % 3
        assert np.array_equal(R.tet_field(c_tet, to), O.carry_field(H, c_tet, "tet", lvl))
        assert np.array_equal(R.tri_field(c_tri, to), O.carry_field(H, c_tri, "tri", lvl))
        d = R.tet_domain(some, to)
        assert np.array_equal(d, O.carry_domain(H, some, "tet", lvl)) and len(d) == len(some) * 8 ** lvl and np.all(np.diff(d) > 0)
        assert np.array_equal(R.tri_domain([1, 0], to), O.carry_domain(H, [1, 0], "tri", lvl))
        # children inherit: the volume-weighted mean of a field is unchanged
        v0, v1 = O.volumes(H[0].points, H[0].tets), O.volumes(H[lvl].points, H[lvl].tets)
        assert abs(v1 @ R.tet_field(c_tet, to) - v0 @ c_tet) <= 1e-13 * (v0 @ np.abs(c_tet))
    assert np.array_equal(R.tet_field(c_tet, 0), c_tet) and np.array_equal(R.tet_domain([0], 0), [0])
    for call in (lambda: R.tet_field(c_tet[1:]), lambda: R.tri_field(c_tri[1:]), lambda: R.tet_domain([-1]), lambda: R.tri_domain([len(H[0].tris)]),
                 lambda: R.tet_field(c_tet, 3), lambda: R.tet_field(1.0)):
        with pytest.raises(ValueError):
            call()


def test_reference_tetrahedron_is_the_first_in_list_order_that_contains_the_point():
    H, R = host_mesh("rijke")
    fl = np.load(os.path.join(ROOT, "tests", "golden", "rijke_flame.npz"))
    ref, x_ref = int(fl["ref_tet"]), fl["x_ref"]
    assert O.first_containing(H[0].points, H[0].tets, x_ref) == ref
    for to in (1, 2):
        r = R.reference_tet(ref, x_ref, to)
        assert r == O.first_containing(H[to].points, H[to].tets, x_ref) and r in R.tet_domain([ref], to).tolist()
    assert R.reference_tet(ref, x_ref, 0) == ref
    # points inside other tetrahedra, in an inner and in a corner child; the faces of the children of both levels lie where a barycentric
    # coordinate or the sum of two is a multiple of 1/4, and these points keep away from them
    for t in (0, 17, 1234):
        X = H[0].points[H[0].tets[t]]
        for lam in ([0.33, 0.27, 0.22, 0.18], [0.7, 0.12, 0.1, 0.08], [0.05, 0.07, 0.3, 0.58]):
            x = np.asarray(lam) @ X
            for to in (1, 2):
                assert R.reference_tet(t, x, to) == O.first_containing(H[to].points, H[to].tets, x)
    # on a face of the parent the whole level is searched: the answer contains the point, whoever owns it
    X = H[0].points[H[0].tets[ref]]
    x = np.array([0.5, 0.3, 0.2, 0.0]) @ X
    r = R.reference_tet(ref, x, 1)
    Xr = H[1].points[H[1].tets[r]]
    lam = np.linalg.solve(np.vstack([Xr.T, np.ones(4)]), np.append(x, 1.0))
    assert lam.min() > -1e-10
    with pytest.raises(ValueError):
        R.reference_tet(len(H[0].tets), x_ref)
    with pytest.raises(ValueError):
        R.reference_tet(ref, x_ref[:2])
    with pytest.raises(ValueError):
        R.reference_tet(ref, X[0] + 100.0)                              # outside the mesh


def test_new_entry_points_are_declared_bound_and_called_from_julia():
    hdr = open(os.path.join(ROOT, "include", "waehip.h")).read()
    jl = open(os.path.join(ROOT, "julia", "WAEHip.jl"), encoding="utf-8").read()
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", hdr), n
        assert n in _lib.EXPORTS
        assert f"ccall((:{n}, libwaehip)" in jl, n
    L = _lib.lib()
    for n in NAMES:
        assert getattr(L, n).argtypes is not None, n
    assert len(L.wae_octosplit.argtypes) == 9 and len(L.wae_octosplit_get.argtypes) == 8 and len(L.wae_octosplit_prolong.argtypes) == 6
    for fn in ("function octosplit_device(", "function prolong("):
        assert fn in jl, fn
    assert "Meshutils.jl:589-747" in hdr and refine.octosplit is octosplit
    # edge_keys.h keeps the (smaller, larger) key of the P2 numbering and gains the (larger, smaller) one beside it
    ek = open(os.path.join(ROOT, "wavesandeigenvalues.jl_amd", "csrc", "edge_keys.h")).read()
    assert "p2_edge_key" in ek and "octo_edge_key" in ek
    mk = open(os.path.join(ROOT, "wavesandeigenvalues.jl_amd", "csrc", "Makefile")).read()
    assert "octosplit.o" in mk
