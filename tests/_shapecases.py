"""The cases shared by tests/test_shape_ref.py (CPU) and tests/test_gpu_shape_p2.py (device): meshes, vectors, coefficients and the two
references of tests/_shaperef.py, each computed once per process.

Meshes: `one`, `two`, `cube` of tests/test_gpu_p2.py (restated: a single tetrahedron; two tetrahedra with det J of opposite sign, points not
ascending, c per simplex given; kuhn_cube(2)) with every point a surface point and every listed boundary triangle, and the Rijke tube of
tests/golden.  Vectors: random complex u (right) and w (left), seeded per mesh and case.  Nodal speed of sound: 1 + 0.3x - 0.2y + 0.1z."""
import functools
import os

import numpy as np

import _p2ref as R
import _shaperef as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TINY = ["one", "two", "cube"]
CASES = ["p2", "p2_nodal", "p1_nodal"]          # element order, and the form of the speed of sound
H = 1e-5
OMEGA, Y = 2.5 + 0.3j, 0.7 - 0.2j
EPS = 1e-13          # rounding of the per-point sum itself: up to ~60 pairs, each a few eps of the sum of the magnitudes


@functools.lru_cache(maxsize=None)
def mesh(name):
    """(points, tets, tris, c_tet, c_tri)"""
    if name == "one":
        pts = np.array([[0.0, 0.0, 0.0], [1.0, 0.1, 0.0], [0.2, 0.9, 0.1], [0.1, 0.2, 0.8]])
        return pts, np.array([[0, 1, 2, 3]], dtype=np.int32), np.array([[0, 1, 2], [3, 1, 0]], dtype=np.int32), None, None
    if name == "two":
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


def nodal_c(pts, base=1.0):
    return base * (1.0 + 0.3 * pts[:, 0] - 0.2 * pts[:, 1] + 0.1 * pts[:, 2])


def dimension(name, order):
    pts, tets, _, _, _ = mesh(name)
    return len(pts) + (len(R.edge_list(tets)) if order == "quad" else 0)


@functools.lru_cache(maxsize=None)
def vectors(name, case):
    order = "lin" if case.startswith("p1") else "quad"
    rng = np.random.default_rng([TINY.index(name) if name in TINY else 7, len(case), sum(map(ord, case))])
    d = dimension(name, order)
    return rng.standard_normal(d) + 1j * rng.standard_normal(d), rng.standard_normal(d) + 1j * rng.standard_normal(d)


@functools.lru_cache(maxsize=None)
def problem(name, case):
    """(_shaperef.Problem, surface points) of a tiny mesh: all points, all listed triangles"""
    pts, tets, tris, c_tet, c_tri = mesh(name)
    order = "lin" if case.startswith("p1") else "quad"
    u, w = vectors(name, case)
    kw = dict(c_point=nodal_c(pts)) if case.endswith("nodal") else dict(c_tet=c_tet, c_tri=c_tri)
    return S.Problem(pts, tets, u, w, OMEGA, order, tris=tris, Y=Y, **kw), np.arange(len(pts))


def scale_is_not_tiny(pb, want):
    """every point has a gradient far above rounding, so that a device that returned zeros could not pass"""
    return bool(np.all(np.abs(want).max(axis=0) > 1e-3 * np.linalg.norm(pb.u) * np.linalg.norm(pb.w) * (abs(pb.omega) ** 2 + 1)))


@functools.lru_cache(maxsize=None)
def references(name, case, h=H):
    """(float64 reference, extended reference, e64) of a tiny mesh"""
    pb, sp = problem(name, case)
    w64, wext = S.sensitivity(pb, sp, h), S.sensitivity_ext(pb, sp, h)
    return w64, wext, S.yardstick(w64, wext)


# ---- Rijke tube ---------------------------------------------------------------------------------------------------------------------------
RIJKE_OMEGA, RIJKE_Y = 1.0e5 + 3.0e3j, 0.7 + 0.1j          # not a mode: chosen so that om^2 M and om Y C carry a few per cent of what K does


def rijke_surface():
    """(all surface points, all boundary triangles) of the Rijke tube: faces that belong to one tetrahedron"""
    _, tets, _, _, _ = mesh("rijke")
    tt = np.asarray(tets, dtype=np.int64)
    faces = np.sort(np.concatenate([tt[:, [0, 1, 2]], tt[:, [0, 1, 3]], tt[:, [0, 2, 3]], tt[:, [1, 2, 3]]]), axis=1)
    uniq, count = np.unique(faces, axis=0, return_counts=True)
    return np.unique(uniq[count == 1])


@functools.lru_cache(maxsize=None)
def rijke_problem(case):
    """P2 Rijke tube, admittance boundary on the outlet; (Problem, all surface points)"""
    pts, tets, tris, c_tet, c_tri = mesh("rijke")
    u, w = vectors("rijke", case)
    kw = dict(c_point=nodal_c(pts, 347.0)) if case.endswith("nodal") else dict(c_tet=c_tet, c_tri=c_tri)
    return S.Problem(pts, tets, u, w, RIJKE_OMEGA, "quad", tris=tris, Y=RIJKE_Y, **kw), rijke_surface()


@functools.lru_cache(maxsize=None)
def rijke_references(case):
    """(float64 reference at all surface points, e64 on 16 of them by the extended route)"""
    pb, sp = rijke_problem(case)
    w64 = S.sensitivity(pb, sp, H)
    pick = np.linspace(0, len(sp) - 1, 16).astype(int)
    wext = S.sensitivity_ext(pb, sp[pick], H)
    return w64, S.yardstick(w64[:, pick], wext)


def flame_inputs():
    fl = np.load(os.path.join(GOLDEN, "rijke_flame.npz"))
    return {"flame_tets": fl["flame_tets"], "ref_tet": int(fl["ref_tet"]), "x_ref": np.array([0.0, 0.0, -0.00101]), "n_ref": fl["n_ref"],
            "nglobal_scaled": float(fl["nglobal_scaled"])}


FLAME_COEFF = 0.8 * np.exp(-1j * 0.9)


@functools.lru_cache(maxsize=None)
def flame_problem():
    """P2 Rijke tube with the flame; points: the 8 wall points of rijke_shape_flame.npz that touch flame tetrahedra, the 4 vertices of the
    reference tetrahedron, and two points whose reduced flame domain is empty"""
    pts, tets, tris, c_tet, c_tri = mesh("rijke")
    g = np.load(os.path.join(GOLDEN, "rijke_shape_flame.npz"))
    sp, in_flame, in_ref = g["surface_points"], g["in_flame"], g["in_ref"]
    pick = np.concatenate([sp[in_flame & ~in_ref][:8], sp[in_ref], sp[~in_flame & ~in_ref][:2]])
    u, w = vectors("rijke", "p2_flame")
    pb = S.Problem(pts, tets, u, w, RIJKE_OMEGA, "quad", c_tet=c_tet, c_tri=c_tri, tris=tris, Y=RIJKE_Y, flame=flame_inputs(), coeff=FLAME_COEFF)
    return pb, pick
