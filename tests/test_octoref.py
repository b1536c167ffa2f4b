"""CPU tests that pin tests/_octoref.py, the host reference of the uniform mesh refinement (`octosplit`, src/Meshutils.jl:589-747), on the five
meshes the GPU tests use: one tetrahedron, two sharing a face, the dyadic Kuhn cube (exact arithmetic: every tetrahedron ties and takes the
second diagonal), the same cube sheared (no ties, all take the third) and the tutorial Rijke tube (all three choices)."""
import functools
from itertools import combinations

import numpy as np
import pytest

import _octoref as O


@functools.lru_cache(maxsize=None)
def hier(name):
    return O.refine(*O.mesh(name), levels=2)


def face_keys(tets):
    """(4 ntets, 3) sorted point triples of the faces of the tetrahedra"""
    t = np.asarray(tets, dtype=np.int64)
    return np.sort(np.concatenate([t[:, list(f)] for f in combinations(range(4), 3)]), axis=1)


def package_keys(simplices):
    """the package's sort key of every simplex: its points sorted descending (sorter.jl:9-31), as tuples"""
    return [tuple(r) for r in (-np.sort(-np.asarray(simplices, dtype=np.int64), axis=1)).tolist()]


@pytest.mark.parametrize("name", O.MESHES)
def test_counts_points_and_parents(name):
    H = hier(name)
    for lo, hi in zip(H[:-1], H[1:]):
        N = len(lo.points)
        edges = {(max(t[i], t[j]), min(t[i], t[j])) for t in lo.tets.tolist() for i in range(4) for j in range(i + 1, 4)}
        assert len(hi.points) == N + len(edges) and len(hi.tets) == 8 * len(lo.tets) and len(hi.tris) == 4 * len(lo.tris)
        assert np.array_equal(hi.points[:N], lo.points)                         # a hierarchy: the first N points are the old ones
        assert [tuple(p) for p in hi.parents.tolist()] == sorted(edges)         # mesh.lines order: ascending by (larger, smaller)
        assert np.array_equal(hi.points[N:], (lo.points[hi.parents[:, 0]] + lo.points[hi.parents[:, 1]]) * 0.5)
        assert hi.tets.min() == 0 and hi.tets.max() == len(hi.points) - 1


def test_counts_of_the_rijke_tube():
    H = hier("rijke")
    assert [len(L.points) for L in H] == [1006, 6172, 42507] and [len(L.tets) for L in H] == [3380, 27040, 216320]
    assert [len(L.tris) for L in H] == [34, 136, 544]


@pytest.mark.parametrize("name", O.MESHES)
def test_volume_is_conserved_and_every_parent_is_filled_by_its_children(name):
    H = hier(name)
    for lo, hi in zip(H[:-1], H[1:]):
        v0, v1 = O.volumes(lo.points, lo.tets), O.volumes(hi.points, hi.tets)
        assert abs(v1.sum() - v0.sum()) <= 1e-14 * v0.sum()
        assert np.all(v1 > 0)
        assert np.max(np.abs(v1[hi.tet_labels].sum(axis=1) - v0)) <= 1e-13 * v0.max()


@pytest.mark.parametrize("name", O.MESHES)
def test_faces_are_shared_by_at_most_two_children_and_the_boundary_is_kept(name):
    H = hier(name)
    for lo, hi in zip(H[:-1], H[1:]):
        def boundary(tets):
            f, cnt = np.unique(face_keys(tets), axis=0, return_counts=True)
            assert cnt.max() <= 2
            return f[cnt == 1]
        b0, b1 = boundary(lo.tets), boundary(hi.tets)
        N = len(lo.points)
        lines = {tuple(p): N + e for e, p in enumerate(hi.parents.tolist())}
        mid = lambda u, v: lines[(max(u, v), min(u, v))]
        kids = []
        for A, B, C in b0.tolist():
            AB, AC, BC = mid(A, B), mid(A, C), mid(B, C)
            kids += [sorted(f) for f in ((A, AB, AC), (B, AB, BC), (C, AC, BC), (AB, AC, BC))]
        assert sorted(kids) == sorted(b1.tolist())                              # exactly the children of the old boundary faces
        if len(lo.tris):                                                        # ... and the listed triangles stay on the boundary
            have = {tuple(f) for f in b1.tolist()}
            assert all(tuple(sorted(t)) in have for t in hi.tris.tolist())


@pytest.mark.parametrize("name", O.MESHES)
def test_lists_are_strictly_increasing_in_the_package_order_and_labels_are_permutations(name):
    H = hier(name)
    for lo, hi in zip(H[:-1], H[1:]):
        for simplices, labels, nchild in ((hi.tets, hi.tet_labels, 8), (hi.tris, hi.tri_labels, 4)):
            keys = package_keys(simplices) if len(simplices) else []
            assert all(a < b for a, b in zip(keys[:-1], keys[1:]))
            assert labels.shape[1] == nchild and np.array_equal(np.sort(labels.ravel()), np.arange(len(simplices)))
        # the first four children of a tetrahedron start at its corners, in order; the inner four share their first two points
        t1 = hi.tets[hi.tet_labels]
        assert np.array_equal(t1[:, :4, 0], lo.tets)
        assert np.all(t1[:, 4:, 0] == t1[:, 4:5, 0]) and np.all(t1[:, 4:, 1] == t1[:, 4:5, 1]) and np.all(t1[:, 4:, :2] >= len(lo.points))
        if len(lo.tris):
            assert np.array_equal(hi.tris[hi.tri_labels][:, :3, 0], lo.tris)


def test_diagonal_choices():
    assert np.all(hier("cube")[1].diagonal == 1)                     # dyadic: the three diagonals are compared exactly; AC-BD ties and wins
    pts, tets, _ = O.mesh("cube")
    L = hier("cube")[1]
    m = lambda u, v: (pts[u] + pts[v]) * 0.5
    d = np.array([[np.sum((m(t[0], t[1]) - m(t[2], t[3])) ** 2), np.sum((m(t[0], t[2]) - m(t[1], t[3])) ** 2),
                   np.sum((m(t[0], t[3]) - m(t[1], t[2])) ** 2)] for t in tets])
    assert np.all(d[:, 1] == d[:, 2]) and np.all(d[:, 0] > d[:, 1])  # the tie is between the second and the third, the first is longer
    assert np.all(L.tets[L.tet_labels[:, 4:]][:, :, 0] == L.tets[L.tet_labels[:, 2:3]][:, :, 1])        # the inner children start at AC
    assert np.all(hier("sheared")[1].diagonal == 2)                  # no ties, all take AD-BC
    assert np.bincount(hier("rijke")[1].diagonal, minlength=3).tolist() == [1118, 1067, 1195]


@pytest.mark.parametrize("name", O.MESHES)
def test_prolongation_reproduces_an_affine_function(name):
    H = hier(name)
    g, c = np.array([0.7, -1.3, 0.45]), 0.2
    f = lambda P: P @ g + c
    for frm, to in ((0, 1), (1, 2), (0, 2)):
        y = O.prolong(H, f(H[frm].points), frm, to)
        exact = f(H[to].points)
        assert y.shape == exact.shape and np.array_equal(y[:len(H[frm].points)], f(H[frm].points))
        # a few roundings of terms of size |g||x| + |c| per level, on both sides
        scale = np.abs(H[to].points) @ np.abs(g) + abs(c)
        assert np.all(np.abs(y - exact) <= 8 * np.finfo(float).eps * scale)
    Z = np.stack([f(H[0].points) * (1 + 2j), H[0].points[:, 0] - 1j * H[0].points[:, 2]], axis=1)
    Y = O.prolong(H, Z, 0, 2)
    assert Y.shape == (len(H[2].points), 2) and np.array_equal(Y, O.prolong(H, O.prolong(H, Z, 0, 1), 1, 2))


@pytest.mark.parametrize("name", O.MESHES)
def test_level_two_is_level_one_applied_twice(name):
    H = hier(name)
    L1 = O.split(*O.mesh(name))
    L2 = O.split(L1.points, L1.tets, L1.tris)
    for a, b in ((L1, H[1]), (L2, H[2])):
        for f in ("points", "tets", "tris", "parents", "tet_labels", "tri_labels"):
            assert np.array_equal(getattr(a, f), getattr(b, f)), f


def test_carriers_and_errors():
    H = hier("rijke")
    c = np.arange(len(H[0].tets), dtype=float)
    c2 = O.carry_field(H, c)
    assert np.array_equal(c2[H[2].tet_labels[H[1].tet_labels[7]].ravel()], np.full(64, 7.0))
    dom = O.carry_domain(H, [3, 5], to_level=1)
    assert np.array_equal(dom, np.sort(np.concatenate([H[1].tet_labels[3], H[1].tet_labels[5]])))
    pts, tets, tris = O.mesh("cube")
    with pytest.raises(ValueError):
        O.split(pts, np.vstack([tets, tets[:1]]), tris)                         # a tetrahedron listed twice
    with pytest.raises(ValueError):
        O.split(pts, tets, np.array([[0, 1, 26]]))                              # (0, 26) is no edge
    with pytest.raises(ValueError):
        O.split(pts, tets + len(pts), tris)
