"""The argument and limit checks of the Hermite entries of libwaehip.so (assemble_herm.hip), pinned through the C ABI on a machine without
a device, the way tests/test_mesh_entry_args.py pins the other mesh entries: every check that an entry makes before it touches the device,
with its return code and the exact text of wae_last_error(), and -- by calls that break two rules at once -- the order of the checks.  The
mesh is the five-point mesh of that file: two tetrahedra and one triangle.  The checks that need the face list (a triangle that is no
face, one listed twice, a face of three tetrahedra) run on the device and are covered by tests/test_gpu_herm.py.

A call that passes every check goes on to hipSetDevice and fails there without a device (with one it succeeds):
test_valid_calls_reach_the_device.  The Python
layer's NotImplementedError for a speed of sound per mesh point is covered at the end."""
import ctypes as C

import numpy as np
import pytest

from wae_amd import _lib
from wae_amd.helmholtz import assemble as A

INV, HIP = _lib.WAE_ERR_INVALID, _lib.WAE_ERR_HIP

PTS = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 1.0, 1.0]])
TETS = np.array([[0, 1, 2, 3], [1, 2, 3, 4]], dtype=np.int32)
TRIS = np.array([[0, 1, 2]], dtype=np.int32)
NP, NT, NS = 5, 2, 1
INT_MAX = 2 ** 31 - 1
MAX_POINTS = 2 ** 21


def i32(*a):
    return np.array(a, dtype=np.int32)


def changed(a, pos, value):
    b = np.array(a).copy()
    b.reshape(-1)[pos] = value
    return b


TETS_LO, TETS_HI = changed(TETS, 6, -1), changed(TETS, 5, NP)
TRIS_LO, TRIS_HI = changed(TRIS, 0, -1), changed(TRIS, 2, NP)
OUT = np.zeros(8)
HANDLE = "handle"
N_REF = np.array([0.0, 0.0, 1.0])
X_REF = np.array([0.25, 0.25, 0.25])

BAD = "bad argument"
TET_RANGE = "tetrahedron refers to a point outside 0..npoints-1"
TRI_RANGE = "triangle refers to a point outside 0..npoints-1"
POINTS_BIG = "too many points: a face key holds three point numbers in 64 bits, npoints <= 2^21"
MESH_BIG = "mesh too large: 400*ntets and 169*ntris triplets must fit a 32-bit count"
FLAME_BIG = "too many flame tetrahedra: 400*nflame triplets must fit a 32-bit count"
REF = "reference tetrahedron out of range"
FLAME = "flame tetrahedron out of range"
NULL_HANDLE = "null handle"

MESH = [("device", 0), ("npoints", NP), ("points", PTS), ("ntets", NT), ("tets", TETS), ("ntris", NS), ("tris", TRIS)]
SPEC = {
    "wae_herm_connectivity": [("device", 0), ("npoints", NP), ("ntets", NT), ("tets", TETS), ("ntris", NS), ("tris", TRIS), ("out", HANDLE)],
    "wae_herm_assemble": MESH + [("c", None), ("out", HANDLE)],
    "wae_herm_assemble_boundary": MESH + [("c", None), ("out", HANDLE)],
    "wae_herm_assemble_flame": MESH + [("nflame", 1), ("flame_tets", i32(0)), ("ref_tet", 1), ("x_ref", X_REF), ("n_ref", N_REF), ("nglobal", 1.0),
                                       ("out", HANDLE), ("volume_out", OUT)],
}


def call(name, **over):
    """the entry with the arguments of its valid call, `over` replacing some (None: a null pointer); returns (code, message, handles)"""
    L = _lib.lib()
    fn = getattr(L, name)
    spec = SPEC[name]
    unknown = set(over) - {k for k, _ in spec}
    assert not unknown, unknown
    assert len(spec) == len(fn.argtypes), name
    args, keep = [], []
    handles = (C.c_void_p * 2)()
    for (key, value), ctype in zip(spec, fn.argtypes):
        value = over.get(key, value)
        if isinstance(value, str):
            assert value == HANDLE
            args.append(C.cast(handles, ctype))
        elif isinstance(value, np.ndarray):
            value = np.ascontiguousarray(value).copy()
            keep.append(value)
            args.append(value.ctypes.data_as(ctype))
        else:
            args.append(value)
    code = fn(*args)
    return code, L.wae_last_error().decode(), handles


# herm_check_mesh: bad argument, the point limit of the face key, the 32-bit limits, the index ranges of the tetrahedra, then of the triangles
MESH_ROWS = [({"npoints": 0}, BAD), ({"npoints": -1}, BAD), ({"ntets": 0}, BAD), ({"ntets": -1}, BAD), ({"tets": None}, BAD), ({"ntris": -1}, BAD),
             ({"tris": None}, BAD), ({"npoints": MAX_POINTS + 1}, POINTS_BIG), ({"npoints": INT_MAX + 1}, POINTS_BIG),
             ({"ntets": INT_MAX // 400 + 1}, MESH_BIG), ({"ntris": INT_MAX // 169 + 1}, MESH_BIG),
             ({"npoints": MAX_POINTS + 1, "ntets": INT_MAX // 400 + 1}, POINTS_BIG), ({"ntets": INT_MAX // 400 + 1, "tets": None}, BAD),
             ({"ntris": INT_MAX // 169 + 1, "tets": TETS_LO}, MESH_BIG), ({"tets": TETS_LO}, TET_RANGE), ({"tets": TETS_HI}, TET_RANGE),
             ({"tris": TRIS_LO}, TRI_RANGE), ({"tris": TRIS_HI}, TRI_RANGE), ({"tets": TETS_HI, "tris": TRIS_LO}, TET_RANGE),
             ({"npoints": MAX_POINTS + 1, "tets": TETS_HI}, POINTS_BIG)]
ASSEMBLY_ROWS = [({"points": None}, BAD), ({"out": None}, BAD), ({"out": None, "tets": TETS_HI}, BAD), ({"points": None, "npoints": MAX_POINTS + 1}, BAD)]
TABLE = {
    "wae_herm_connectivity": [({"out": None}, BAD), ({"out": None, "tets": TETS_HI}, BAD)] + MESH_ROWS,
    "wae_herm_assemble": ASSEMBLY_ROWS + MESH_ROWS,
    "wae_herm_assemble_boundary": ASSEMBLY_ROWS + MESH_ROWS + [({"ntris": 0}, BAD), ({"ntris": 0, "tris": None}, BAD), ({"ntris": 0, "tets": TETS_HI}, BAD)],
    "wae_herm_assemble_flame": ASSEMBLY_ROWS + MESH_ROWS + [
        ({"nflame": 0}, BAD), ({"nflame": -1}, BAD), ({"flame_tets": None}, BAD), ({"x_ref": None}, BAD), ({"n_ref": None}, BAD),
        ({"nflame": 0, "tets": TETS_HI}, BAD), ({"nflame": INT_MAX // 400 + 1}, FLAME_BIG), ({"nflame": INT_MAX // 400 + 1, "ref_tet": NT}, FLAME_BIG),
        ({"nflame": INT_MAX // 400 + 1, "tets": TETS_HI}, TET_RANGE), ({"ref_tet": -1}, REF), ({"ref_tet": NT}, REF), ({"flame_tets": i32(-1)}, FLAME),
        ({"flame_tets": i32(NT)}, FLAME), ({"ref_tet": NT, "flame_tets": i32(NT)}, REF), ({"ref_tet": NT, "tris": TRIS_HI}, TRI_RANGE)],
}
CASES = [pytest.param(name, over, msg, id=f"{name}-{i}") for name, rows in TABLE.items() for i, (over, msg) in enumerate(rows)]


@pytest.mark.parametrize("name, over, msg", CASES)
def test_rejected_before_the_device(name, over, msg):
    code, text, handles = call(name, **over)
    assert (code, text) == (INV, msg)
    assert handles[0] is None                         # nothing written


def test_null_handles():
    L = _lib.lib()
    assert L.wae_herm_connectivity_info(None, None, None, None, None) == INV and L.wae_last_error().decode() == NULL_HANDLE
    assert L.wae_herm_connectivity_get(None, None, None, None) == INV and L.wae_last_error().decode() == NULL_HANDLE
    assert L.wae_herm_connectivity_free(None) == 0


def test_every_hermite_entry_is_covered():
    herm = {s for s in _lib.EXPORTS if s.startswith("wae_herm_")}
    assert herm == set(SPEC) | {"wae_herm_connectivity_info", "wae_herm_connectivity_get", "wae_herm_connectivity_free"}


VALID = [(name, {}) for name in SPEC] + [
    ("wae_herm_connectivity", {"ntris": 0, "tris": None}), ("wae_herm_connectivity", {"npoints": MAX_POINTS}), ("wae_herm_assemble", {"ntris": 0, "tris": None}),
    ("wae_herm_assemble", {"c": np.ones(NT)}), ("wae_herm_assemble_boundary", {"c": np.ones(NS)}), ("wae_herm_assemble_flame", {"ntris": 0, "tris": None}),
    ("wae_herm_assemble_flame", {"volume_out": None}),
]


@pytest.mark.parametrize("name, over", [pytest.param(n, o, id=f"{n}-{i}") for i, (n, o) in enumerate(VALID)])
def test_valid_calls_reach_the_device(name, over):
    """every check passes: without a device the call fails at hipSetDevice, with one it succeeds and returns a handle"""
    L = _lib.lib()
    code, text, handles = call(name, **over)
    if code == 0:
        assert handles[0] is not None
        (L.wae_herm_connectivity_free if name == "wae_herm_connectivity" else L.wae_p1_free)(C.c_void_p(handles[0]))
    else:
        assert code == HIP and text.startswith("hipSetDevice(device)"), (code, text)


# ---- the generated tables -------------------------------------------------------------------------------------------------------------------
def test_the_generator_reproduces_the_committed_header(tmp_path):
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("gen_herm_tables", os.path.join(root, "dev", "gen_herm_tables.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    out = tmp_path / "herm_tables.h"
    gen.main(out=str(out))
    with open(os.path.join(root, "wavesandeigenvalues.jl_amd", "csrc", "herm_tables.h"), "rb") as f:
        assert out.read_bytes() == f.read()


# ---- the Python layer ---------------------------------------------------------------------------------------------------------------------
def test_a_nodal_speed_of_sound_is_not_implemented():
    c_point = np.ones(NP)
    for fn, args in ((A.assemble_herm, (PTS, TETS, TRIS)), (A.assemble_herm_boundary, (PTS, TETS, TRIS))):
        with pytest.raises(NotImplementedError, match="c_point"):
            fn(*args, c_point=c_point)


def test_the_length_of_c_is_checked_before_the_library_is_called():
    with pytest.raises(ValueError, match="c_tet"):
        A.assemble_herm(PTS, TETS, TRIS, c_tet=np.ones(NT + 1))
    with pytest.raises(ValueError, match="c_tri"):
        A.assemble_herm_boundary(PTS, TETS, TRIS, c_tri=np.ones(NS + 1))


def test_dof_count_and_dofs_on_the_host():
    assert A.herm_dof_count(PTS, TETS) == A.herm_dof_count(NP, TETS, TRIS) == 4 * NP + 7             # 8 faces, one shared
    faces = np.array([[1, 2, 3], [0, 1, 3]])
    u = A.herm_dofs(PTS, faces, TRIS, lambda x: x[:, 0] + 2 * x[:, 1] ** 2, lambda x: np.stack([np.ones(len(x)), 4 * x[:, 1], np.zeros(len(x))], axis=1))
    assert u.shape == (4 * NP + 3,)
    assert np.array_equal(u[:NP], PTS[:, 0] + 2 * PTS[:, 1] ** 2) and np.array_equal(u[NP:2 * NP], np.ones(NP)) and np.array_equal(u[2 * NP:3 * NP], 4 * PTS[:, 1])
    assert not u[3 * NP:4 * NP].any()
    cen = np.array([PTS[[0, 1, 2]].mean(axis=0), PTS[[1, 2, 3]].mean(axis=0), PTS[[0, 1, 3]].mean(axis=0)])
    assert np.allclose(u[4 * NP:], cen[:, 0] + 2 * cen[:, 1] ** 2, rtol=0, atol=1e-15)
