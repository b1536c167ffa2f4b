"""The argument checks of the mesh-side entries of libwaehip.so (assemble.hip, assemble_p2.hip, bloch.hip, octosplit.hip, locate.hip), pinned
through the C ABI on a machine without a device: every check that an entry makes before it touches the device, with its return code and
the exact text of wae_last_error(), and -- by calls that break two rules at once -- the order of the checks.  The mesh is the five-point
mesh of tests/test_shape_args.py: two tetrahedra and one triangle.  Where the P1 and the P2 entries answer the same mistake differently
(a step h that is not finite, negative pair counts), each is recorded as it is.

The entries that take a handle (info, get, free, and the queries of a refinement or a locator) are called with a null handle here: no
handle exists without a device.  The checks behind the handle (order, kind and tol of the locator's queries among them) are pinned in the
same way by the two tests at the end, which are marked gpu.

A call that passes every check goes on to hipSetDevice and fails there without a device: test_valid_calls_reach_the_device.
"""
import ctypes as C

import numpy as np
import pytest

from wae_amd import _lib

INV, HIP = _lib.WAE_ERR_INVALID, _lib.WAE_ERR_HIP

PTS = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 1.0, 1.0]])
TETS = np.array([[0, 1, 2, 3], [1, 2, 3, 4]], dtype=np.int32)
TRIS = np.array([[0, 1, 2]], dtype=np.int32)
NP, NT, NS, NE = 5, 2, 1, 9
NV = NP + NE


def i32(*a):
    return np.array(a, dtype=np.int32)


def changed(a, pos, value):
    b = np.array(a).copy()
    b.reshape(-1)[pos] = value
    return b


TETS_LO, TETS_HI = changed(TETS, 6, -1), changed(TETS, 5, NP)
TRIS_LO, TRIS_HI = changed(TRIS, 0, -1), changed(TRIS, 2, NP)
C_POINT = np.linspace(1.0, 2.0, NP)
C_NAN, C_INF = changed(C_POINT, 3, np.nan), changed(C_POINT, 0, np.inf)
PTS_NAN = changed(PTS, 7, np.nan)
ONES = np.ones(2 * NV)                           # a complex vector of the P2 space (its first 2 NP doubles: of the P1 space)
OUT = np.zeros(64)                               # room for every array result of a call that goes through
HANDLE = "handle"                                # a void* to receive a handle
OM = np.array([3.0, 0.5])
N_REF = np.array([0.0, 0.0, 1.0])
X_REF = np.array([0.5, 0.5, 0.5])
# the surface points 0 and 4 with their tetrahedra, point 0 with its triangle
PAIR_PT_T, PAIR_TET, PAIR_PT_S, PAIR_TRI = i32(0, 4), i32(0, 1), i32(0), i32(0)
# a 3 x 3 CSR matrix with 4 entries, folded to dimension 2
ROWPTR, COL, VALS, CELL, FLAGS = i32(0, 2, 3, 4), i32(0, 2, 1, 2), np.ones(4), i32(0, 1, 0), i32(0, 0, 1)

BAD = "bad argument"
TET_RANGE = "tetrahedron refers to a point outside 0..npoints-1"
TRI_RANGE = "triangle refers to a point outside 0..npoints-1"
CP_NULL = "c_point is required: one speed of sound per mesh point"
CP_FIN = "c_point holds a value that is not finite"
REF = "reference tetrahedron out of range"
FLAME = "flame tetrahedron out of range"
PAIR = "pair index out of range"
H_STEP = "the step h must be finite and positive"
T_PAIRS, S_PAIRS = "bad tetrahedron pair arguments", "bad triangle pair arguments"
F_PAIRS, R_PAIRS = "bad flame pair arguments", "bad reference pair arguments"
P1_BIG = "too many tetrahedra for 32-bit triplet indices"
SRC_BIG = "too many triangles for a 32-bit pair count"
P2_BIG = "mesh too large: 100*ntets and 36*ntris triplets must fit a 32-bit count"
FLAME_BIG = "too many flame tetrahedra: 100*nflame triplets must fit a 32-bit count"
PAIRS3_BIG, PAIRS6_BIG = "too many pairs: 3*npair must fit a 32-bit count", "too many pairs: 6*npair must fit a 32-bit count"
NV_MSG = "nv is not npoints + nedges"
NULL_HANDLE = "null handle"
INT_MAX = 2 ** 31 - 1

# ---- the entries: argument names with the values of a valid call ---------------------------------------------------------------------
MESH = [("device", 0), ("npoints", NP), ("points", PTS), ("ntets", NT), ("tets", TETS)]
SPEC = {
    "wae_p1_assemble": MESH + [("c", None), ("out", HANDLE)],
    "wae_p1_assemble_cpoint": MESH + [("c", C_POINT), ("out", HANDLE)],
    "wae_p1_assemble_boundary": MESH[:3] + [("ntris", NS), ("tris", TRIS), ("c", None), ("out", HANDLE)],
    "wae_p1_assemble_boundary_cpoint": MESH[:3] + [("ntris", NS), ("tris", TRIS), ("c", C_POINT), ("out", HANDLE)],
    "wae_p1_assemble_source": MESH[:3] + [("ntris", NS), ("tris", TRIS), ("c", None), ("out", OUT)],
    "wae_p1_assemble_source_cpoint": MESH[:3] + [("ntris", NS), ("tris", TRIS), ("c", C_POINT), ("out", OUT)],
    "wae_p1_assemble_flame": MESH + [("nflame", 1), ("flame_tets", i32(0)), ("ref_tet", 1), ("n_ref", N_REF), ("nglobal", 1.0), ("out", HANDLE),
                                     ("volume_out", OUT)],
    "wae_p1_shape_sensitivity": MESH[:3] + [("tets", TETS), ("c_tet", None), ("npair_t", 2), ("pair_pt_t", PAIR_PT_T), ("pair_tet", PAIR_TET),
                                            ("tris", TRIS), ("c_tri", np.ones(NS)), ("npair_s", 1), ("pair_pt_s", PAIR_PT_S), ("pair_tri", PAIR_TRI),
                                            ("ntets", NT), ("ntris", NS), ("omega", OM), ("omegaY", OM), ("v", ONES), ("v_adj", ONES), ("h", 1e-6),
                                            ("out_t", OUT), ("out_s", OUT)],
    "wae_p1_shape_sensitivity_cpoint": MESH[:3] + [("tets", TETS), ("c_point", C_POINT), ("npair_t", 2), ("pair_pt_t", PAIR_PT_T),
                                                   ("pair_tet", PAIR_TET), ("tris", TRIS), ("npair_s", 1), ("pair_pt_s", PAIR_PT_S),
                                                   ("pair_tri", PAIR_TRI), ("ntets", NT), ("ntris", NS), ("omega", OM), ("omegaY", OM), ("v", ONES),
                                                   ("v_adj", ONES), ("h", 1e-6), ("out_t", OUT), ("out_s", OUT)],
    "wae_p1_shape_sensitivity_flame": MESH + [("npair", 2), ("pair_pt", PAIR_PT_T), ("pair_tet", PAIR_TET), ("ref_tet", 1), ("npair_r", 1),
                                              ("pair_pt_r", i32(4)), ("n_ref", N_REF), ("v", ONES), ("v_adj", ONES), ("h", 1e-6), ("det_pm", OUT),
                                              ("ssum", OUT), ("g_pm", OUT), ("g0", OUT)],
    "wae_p2_connectivity": [("device", 0), ("npoints", NP), ("ntets", NT), ("tets", TETS), ("ntris", NS), ("tris", TRIS), ("out", HANDLE)],
    "wae_p2_assemble": MESH + [("c", None), ("out", HANDLE)],
    "wae_p2_assemble_cpoint": MESH + [("c", C_POINT), ("out", HANDLE)],
    "wae_p2_assemble_boundary": MESH + [("ntris", NS), ("tris", TRIS), ("c", None), ("out", HANDLE)],
    "wae_p2_assemble_boundary_cpoint": MESH + [("ntris", NS), ("tris", TRIS), ("c", C_POINT), ("out", HANDLE)],
    "wae_p2_assemble_source": MESH + [("ntris", NS), ("tris", TRIS), ("c", None), ("out", OUT), ("nout", NV)],
    "wae_p2_assemble_source_cpoint": MESH + [("ntris", NS), ("tris", TRIS), ("c", C_POINT), ("out", OUT), ("nout", NV)],
    "wae_p2_assemble_flame": MESH + [("nflame", 1), ("flame_tets", i32(0)), ("ref_tet", 1), ("x_ref", X_REF), ("n_ref", N_REF), ("nglobal", 1.0),
                                     ("out", HANDLE), ("volume_out", OUT)],
    "wae_p2_shape_sensitivity": MESH[:3] + [("tets", TETS), ("c_tet", None), ("npair_t", 2), ("pair_pt_t", PAIR_PT_T), ("pair_tet", PAIR_TET),
                                            ("tris", TRIS), ("c_tri", None), ("npair_s", 1), ("pair_pt_s", PAIR_PT_S), ("pair_tri", PAIR_TRI),
                                            ("ntets", NT), ("ntris", NS), ("omega", OM), ("omegaY", OM), ("nv", NV), ("v", ONES), ("v_adj", ONES),
                                            ("h", 1e-6), ("out_t", OUT), ("out_s", OUT)],
    "wae_p2_shape_sensitivity_cpoint": MESH[:3] + [("tets", TETS), ("c_point", C_POINT), ("npair_t", 2), ("pair_pt_t", PAIR_PT_T),
                                                   ("pair_tet", PAIR_TET), ("tris", TRIS), ("npair_s", 1), ("pair_pt_s", PAIR_PT_S),
                                                   ("pair_tri", PAIR_TRI), ("ntets", NT), ("ntris", NS), ("omega", OM), ("omegaY", OM), ("nv", NV),
                                                   ("v", ONES), ("v_adj", ONES), ("h", 1e-6), ("out_t", OUT), ("out_s", OUT)],
    "wae_p2_shape_sensitivity_flame": MESH + [("npair", 2), ("pair_pt", PAIR_PT_T), ("pair_tet", PAIR_TET), ("ref_tet", 1), ("npair_r", 1),
                                              ("pair_pt_r", i32(4)), ("x_ref", X_REF), ("n_ref", N_REF), ("nv", NV), ("v", ONES), ("v_adj", ONES),
                                              ("h", 1e-6), ("det_pm", OUT), ("ssum", OUT), ("g_pm", OUT), ("g0", OUT)],
    "wae_bloch_numbering": [("device", 0), ("npoints", NP), ("ntets", NT), ("tets", TETS), ("nsector", 4), ("naxis", 1), ("order", 2),
                            ("out", HANDLE)],
    "wae_bloch_fold": [("device", 0), ("n", 3), ("rowptr", ROWPTR), ("col", COL), ("v0", VALS), ("v1", None), ("cell_dof", CELL), ("flags", FLAGS),
                       ("dim", 2), ("nparts", 3), ("out", HANDLE)],
    "wae_octosplit": MESH + [("ntris", NS), ("tris", TRIS), ("levels", 2), ("out", HANDLE)],
    "wae_locator_create": MESH + [("cell_target", 0), ("out", HANDLE)],
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
    handles = (C.c_void_p * 6)()
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


# ---- the tables: (arguments replaced, return code, message) ------------------------------------------------------------------------------
def p1_mesh_rows(count, array, lo, hi, range_msg, nodal, big=None):
    """the checks shared by the P1 interior / boundary drivers: bad argument, c_point, the 32-bit limit, the index range"""
    rows = [({"npoints": 0}, BAD), ({"npoints": -1}, BAD), ({count: 0}, BAD), ({count: -3}, BAD), ({"points": None}, BAD), ({array: None}, BAD),
            ({"out": None}, BAD), ({array: lo}, range_msg), ({array: hi}, range_msg),
            ({"points": None, array: hi}, BAD)]
    if big:
        rows += [({count: big[0]}, big[1]), ({count: big[0], "out": None}, BAD)]
    if nodal:
        rows += [({"c": None}, CP_NULL), ({"c": C_NAN}, CP_FIN), ({"c": C_INF}, CP_FIN), ({"c": None, array: hi}, CP_NULL), ({"c": C_NAN, array: lo}, CP_FIN),
                 ({"c": None, "npoints": 0}, BAD)]
        if big:
            rows += [({"c": C_NAN, count: big[0]}, CP_FIN)]
    return rows


def p1_source_rows(nodal):
    rows = [r for r in p1_mesh_rows("ntris", "tris", TRIS_LO, TRIS_HI, TRI_RANGE, nodal, (1 << 30, SRC_BIG)) if r[0] != {"ntris": 0}]
    return rows + [({"ntris": 0, "tris": None, "out": None}, BAD), ({"ntris": 0, "npoints": 0}, BAD)]


def p2_mesh_rows(with_tris):
    """p2_check_mesh: bad argument, the 32-bit limits, the index ranges of the tetrahedra, then of the triangles"""
    rows = [({"npoints": 0}, BAD), ({"npoints": -1}, BAD), ({"ntets": 0}, BAD), ({"ntets": -1}, BAD), ({"tets": None}, BAD),
            ({"npoints": INT_MAX + 1}, P2_BIG), ({"ntets": INT_MAX // 100 + 1}, P2_BIG), ({"tets": TETS_LO}, TET_RANGE), ({"tets": TETS_HI}, TET_RANGE),
            ({"ntets": INT_MAX // 100 + 1, "tets": None}, BAD)]
    if with_tris:
        rows += [({"ntris": -1}, BAD), ({"tris": None}, BAD), ({"ntris": INT_MAX // 36 + 1}, P2_BIG), ({"tris": TRIS_LO}, TRI_RANGE),
                 ({"tris": TRIS_HI}, TRI_RANGE), ({"tets": TETS_HI, "tris": TRIS_LO}, TET_RANGE), ({"ntris": INT_MAX // 36 + 1, "tets": TETS_LO}, P2_BIG)]
    return rows


def p2_assembly_rows(with_tris, nodal):
    rows = [({"points": None}, BAD), ({"out": None}, BAD), ({"out": None, "tets": TETS_HI}, BAD), ({"points": None, "ntets": INT_MAX // 100 + 1}, BAD)]
    rows += p2_mesh_rows(with_tris)
    if nodal:
        rows += [({"c": None}, CP_NULL), ({"c": C_NAN}, CP_FIN), ({"c": C_INF}, CP_FIN), ({"c": None, "tets": TETS_HI}, TET_RANGE),
                 ({"c": C_NAN, "npoints": 0}, BAD)]
    return rows


P1_SHAPE = [({"npoints": 0}, BAD), ({"points": None}, BAD), ({"v": None}, BAD), ({"v_adj": None}, BAD), ({"omega": None}, BAD),
            ({"h": 0.0}, BAD), ({"h": -1e-6}, BAD), ({"h": np.nan}, BAD), ({"h": 0.0, "tets": None}, BAD),
            ({"tets": None}, T_PAIRS), ({"pair_pt_t": None}, T_PAIRS), ({"pair_tet": None}, T_PAIRS), ({"out_t": None}, T_PAIRS), ({"ntets": 0}, T_PAIRS),
            ({"ntets": -1}, T_PAIRS),
            ({"tris": None}, S_PAIRS), ({"pair_pt_s": None}, S_PAIRS), ({"pair_tri": None}, S_PAIRS), ({"out_s": None}, S_PAIRS),
            ({"omegaY": None}, S_PAIRS), ({"ntris": 0}, S_PAIRS), ({"tets": None, "tris": None}, T_PAIRS),
            ({"pair_tet": i32(0, -1)}, PAIR), ({"pair_tet": i32(NT, 1)}, PAIR), ({"pair_pt_t": i32(-1, 4)}, PAIR), ({"pair_pt_t": i32(0, NP)}, PAIR),
            ({"pair_tri": i32(-1)}, PAIR), ({"pair_tri": i32(NS)}, PAIR), ({"pair_pt_s": i32(-1)}, PAIR), ({"pair_pt_s": i32(NP)}, PAIR),
            ({"tets": TETS_LO}, TET_RANGE), ({"tets": TETS_HI}, TET_RANGE), ({"tris": TRIS_LO}, TRI_RANGE), ({"tris": TRIS_HI}, TRI_RANGE),
            ({"tets": TETS_HI, "tris": TRIS_HI}, TET_RANGE), ({"tets": TETS_HI, "pair_tri": i32(NS)}, PAIR), ({"pair_tet": i32(0, NT), "out_s": None}, S_PAIRS)]
P2_SHAPE = [({"points": None}, BAD), ({"v": None}, BAD), ({"v_adj": None}, BAD), ({"omega": None}, BAD), ({"npair_t": -1}, BAD), ({"npair_s": -1}, BAD),
            ({"h": 0.0}, H_STEP), ({"h": -1e-6}, H_STEP), ({"h": np.inf}, H_STEP), ({"h": np.nan}, H_STEP), ({"h": 0.0, "points": None}, BAD),
            ({"h": np.nan, "pair_tet": None}, H_STEP),
            ({"pair_pt_t": None}, T_PAIRS), ({"pair_tet": None}, T_PAIRS), ({"out_t": None}, T_PAIRS),
            ({"tris": None}, S_PAIRS), ({"pair_pt_s": None}, S_PAIRS), ({"pair_tri": None}, S_PAIRS), ({"out_s": None}, S_PAIRS),
            ({"omegaY": None}, S_PAIRS), ({"ntris": 0}, S_PAIRS), ({"out_t": None, "out_s": None}, T_PAIRS), ({"out_s": None, "npoints": 0}, S_PAIRS),
            ({"npoints": 0}, BAD), ({"ntets": 0}, BAD), ({"tets": None}, BAD), ({"ntets": INT_MAX // 100 + 1}, P2_BIG),
            ({"ntris": INT_MAX // 36 + 1}, P2_BIG), ({"tets": TETS_LO}, TET_RANGE), ({"tets": TETS_HI}, TET_RANGE), ({"tris": TRIS_LO}, TRI_RANGE),
            ({"tris": TRIS_HI}, TRI_RANGE), ({"tets": TETS_HI, "pair_tet": i32(0, NT)}, TET_RANGE),
            ({"npair_t": INT_MAX // 3 + 1}, PAIRS3_BIG), ({"npair_s": INT_MAX // 3 + 1}, PAIRS3_BIG), ({"npair_t": INT_MAX // 3 + 1, "tris": TRIS_HI}, TRI_RANGE),
            ({"pair_tet": i32(0, -1)}, PAIR), ({"pair_tet": i32(NT, 1)}, PAIR), ({"pair_pt_t": i32(-1, 4)}, PAIR), ({"pair_pt_t": i32(0, NP)}, PAIR),
            ({"pair_tri": i32(-1)}, PAIR), ({"pair_tri": i32(NS)}, PAIR), ({"pair_pt_s": i32(-1)}, PAIR), ({"pair_pt_s": i32(NP)}, PAIR),
            ({"npair_t": 0, "npair_s": 0, "nv": NV - 1}, NV_MSG), ({"npair_t": 0, "npair_s": 0, "nv": NP}, NV_MSG),
            ({"npair_t": 0, "npair_s": 0, "nv": NV + 1, "tris": TRIS_HI}, NV_MSG)]
P1_SHAPE_FLAME = [({"npoints": 0}, BAD), ({"ntets": 0}, BAD), ({"points": None}, BAD), ({"tets": None}, BAD), ({"n_ref": None}, BAD), ({"v": None}, BAD),
                  ({"v_adj": None}, BAD), ({"g0": None}, BAD), ({"h": 0.0}, BAD), ({"h": -1.0}, BAD), ({"h": np.nan}, BAD),
                  ({"pair_pt": None}, F_PAIRS), ({"pair_tet": None}, F_PAIRS), ({"det_pm": None}, F_PAIRS), ({"ssum": None}, F_PAIRS),
                  ({"pair_pt_r": None}, R_PAIRS), ({"g_pm": None}, R_PAIRS), ({"ssum": None, "g_pm": None}, F_PAIRS), ({"g_pm": None, "g0": None}, BAD),
                  ({"ref_tet": -1}, REF), ({"ref_tet": NT}, REF), ({"ref_tet": NT, "g_pm": None}, R_PAIRS),
                  ({"pair_tet": i32(0, -1)}, PAIR), ({"pair_tet": i32(NT, 1)}, PAIR), ({"pair_pt": i32(-1, 4)}, PAIR), ({"pair_pt": i32(0, NP)}, PAIR),
                  ({"pair_pt_r": i32(-1)}, PAIR), ({"pair_pt_r": i32(NP)}, PAIR), ({"pair_pt_r": i32(NP), "ref_tet": -1}, REF),
                  ({"tets": TETS_LO}, TET_RANGE), ({"tets": TETS_HI}, TET_RANGE), ({"tets": TETS_HI, "pair_pt": i32(0, NP)}, PAIR)]
P2_SHAPE_FLAME = [({"points": None}, BAD), ({"x_ref": None}, BAD), ({"n_ref": None}, BAD), ({"v": None}, BAD), ({"v_adj": None}, BAD), ({"g0": None}, BAD),
                  ({"npair": -1}, BAD), ({"npair_r": -1}, BAD), ({"h": 0.0}, H_STEP), ({"h": -1.0}, H_STEP), ({"h": np.inf}, H_STEP), ({"h": np.nan}, H_STEP),
                  ({"h": np.inf, "g0": None}, BAD),
                  ({"pair_pt": None}, F_PAIRS), ({"pair_tet": None}, F_PAIRS), ({"det_pm": None}, F_PAIRS), ({"ssum": None}, F_PAIRS),
                  ({"pair_pt_r": None}, R_PAIRS), ({"g_pm": None}, R_PAIRS), ({"ssum": None, "g_pm": None}, F_PAIRS), ({"ssum": None, "h": 0.0}, H_STEP),
                  ({"g_pm": None, "tets": None}, R_PAIRS)] + p2_mesh_rows(False) + [
                  ({"npair": INT_MAX // 6 + 1}, PAIRS6_BIG), ({"npair_r": INT_MAX // 6 + 1}, PAIRS6_BIG), ({"npair": INT_MAX // 6 + 1, "tets": TETS_HI}, TET_RANGE),
                  ({"ref_tet": -1}, REF), ({"ref_tet": NT}, REF), ({"ref_tet": NT, "npair_r": INT_MAX // 6 + 1}, PAIRS6_BIG),
                  ({"pair_tet": i32(0, -1)}, FLAME), ({"pair_tet": i32(NT, 1)}, FLAME), ({"pair_pt": i32(-1, 4)}, PAIR), ({"pair_pt": i32(0, NP)}, PAIR),
                  ({"pair_tet": i32(0, NT), "pair_pt": i32(NP, 4)}, PAIR), ({"pair_tet": i32(NT, 1), "pair_pt": i32(NP, 4)}, FLAME),
                  ({"pair_pt_r": i32(-1)}, PAIR), ({"pair_pt_r": i32(NP)}, PAIR), ({"pair_pt_r": i32(NP), "ref_tet": -1}, REF)]
P1_FLAME = [({"npoints": 0}, BAD), ({"ntets": 0}, BAD), ({"nflame": 0}, BAD), ({"nflame": -1}, BAD), ({"points": None}, BAD), ({"tets": None}, BAD),
            ({"flame_tets": None}, BAD), ({"n_ref": None}, BAD), ({"out": None}, BAD), ({"ref_tet": -1}, REF), ({"ref_tet": NT}, REF),
            ({"flame_tets": i32(-1)}, FLAME), ({"flame_tets": i32(NT)}, FLAME), ({"tets": TETS_LO}, TET_RANGE), ({"tets": TETS_HI}, TET_RANGE),
            ({"ref_tet": NT, "flame_tets": i32(NT)}, REF), ({"flame_tets": i32(NT), "tets": TETS_HI}, FLAME), ({"ref_tet": -1, "out": None}, BAD)]
P2_FLAME = [({"points": None}, BAD), ({"out": None}, BAD), ({"nflame": 0}, BAD), ({"nflame": -1}, BAD), ({"flame_tets": None}, BAD), ({"x_ref": None}, BAD),
            ({"n_ref": None}, BAD), ({"x_ref": None, "tets": TETS_HI}, BAD)] + p2_mesh_rows(False) + [
            ({"nflame": INT_MAX // 100 + 1}, FLAME_BIG), ({"nflame": INT_MAX // 100 + 1, "tets": TETS_HI}, TET_RANGE),
            ({"nflame": INT_MAX // 100 + 1, "ref_tet": -1}, FLAME_BIG), ({"ref_tet": -1}, REF), ({"ref_tet": NT}, REF), ({"flame_tets": i32(-1)}, FLAME),
            ({"flame_tets": i32(NT)}, FLAME), ({"ref_tet": NT, "flame_tets": i32(NT)}, REF), ({"ref_tet": NT, "tets": TETS_LO}, TET_RANGE)]
ORDER_MSG = "order must be 1 (lin) or 2 (quad)"
BLOCH_NUMBERING = [({"out": None}, BAD), ({"order": 0}, ORDER_MSG), ({"order": 3}, ORDER_MSG), ({"order": 3, "out": None}, BAD),
                   ({"order": 0, "npoints": 0}, ORDER_MSG)] + p2_mesh_rows(False) + [
                   ({"naxis": -1}, "naxis must lie in 0..nsector"), ({"naxis": 5}, "naxis must lie in 0..nsector"),
                   ({"naxis": -1, "tets": TETS_HI}, TET_RANGE), ({"nsector": NP + 1}, "nsector exceeds the number of points"),
                   ({"nsector": NP + 1, "naxis": NP + 2}, "naxis must lie in 0..nsector"),
                   ({"nsector": 2, "naxis": 0}, "more image points (3) than points off the axis (2): an image point would have no twin"),
                   ({"nsector": 3, "naxis": 2}, "more image points (2) than points off the axis (1): an image point would have no twin")]
DIM_MSG = "dim must lie in 1..n, and n and nparts * dim must fit a 32-bit index"
BLOCH_FOLD = [({"n": 0}, BAD), ({"n": -1}, BAD), ({"rowptr": None}, BAD), ({"cell_dof": None}, BAD), ({"flags": None}, BAD), ({"v0": None}, BAD),
              ({"out": None}, BAD), ({"nparts": 0}, "nparts must be 3 or 6"), ({"nparts": 4}, "nparts must be 3 or 6"), ({"nparts": 4, "v0": None}, BAD),
              ({"dim": 0}, DIM_MSG), ({"dim": -2}, DIM_MSG), ({"dim": 4}, DIM_MSG), ({"n": INT_MAX + 1}, DIM_MSG), ({"n": INT_MAX, "dim": INT_MAX // 3 + 1}, DIM_MSG),
              ({"dim": 0, "nparts": 5}, "nparts must be 3 or 6"),
              ({"rowptr": i32(1, 2, 3, 4)}, "rowptr does not start at 0"), ({"rowptr": i32(0, 2, 1, 4)}, "rowptr decreases"),
              ({"rowptr": i32(1, 0, 3, 4)}, "rowptr does not start at 0"), ({"rowptr": i32(1, 2, 3, 4), "dim": 0}, DIM_MSG),
              ({"col": None}, BAD), ({"col": None, "rowptr": i32(0, 2, 1, 4)}, "rowptr decreases"),
              ({"col": i32(0, 2, -1, 2)}, "column index outside 0..n-1"), ({"col": i32(0, 3, 1, 2)}, "column index outside 0..n-1"),
              ({"cell_dof": i32(0, -1, 0)}, "cell_dof holds an index outside 0..dim-1"), ({"cell_dof": i32(0, 1, 2)}, "cell_dof holds an index outside 0..dim-1"),
              ({"flags": i32(0, 4, 1)}, "flags holds an unknown bit"), ({"flags": i32(-1, 0, 1)}, "flags holds an unknown bit"),
              ({"cell_dof": i32(0, 1, 2), "flags": i32(0, 4, 1)}, "flags holds an unknown bit"),
              ({"cell_dof": i32(2, 1, 0), "flags": i32(0, 4, 1)}, "cell_dof holds an index outside 0..dim-1"),
              ({"col": i32(0, 3, 1, 2), "cell_dof": i32(2, 1, 0)}, "column index outside 0..n-1")]
LEVELS_BIG = "8^levels * ntets or 4^levels * ntris does not fit a 32-bit index"
OCTOSPLIT = [({"out": None}, BAD), ({"points": None}, BAD), ({"npoints": 0}, BAD), ({"npoints": -1}, BAD), ({"ntets": 0}, BAD), ({"ntets": -1}, BAD),
             ({"tets": None}, BAD), ({"ntris": -1}, BAD), ({"tris": None}, BAD), ({"levels": 0}, "levels must be at least 1"),
             ({"levels": -1}, "levels must be at least 1"), ({"levels": 0, "tets": None}, BAD),
             ({"npoints": INT_MAX + 1}, "npoints does not fit a 32-bit index"), ({"npoints": INT_MAX + 1, "levels": 0}, "levels must be at least 1"),
             ({"levels": 11}, LEVELS_BIG), ({"levels": 16, "ntets": 1, "ntris": 0, "tris": None}, LEVELS_BIG), ({"ntets": INT_MAX // 8 + 1}, LEVELS_BIG),
             ({"ntris": INT_MAX // 4 + 1}, LEVELS_BIG), ({"levels": 11, "npoints": INT_MAX + 1}, "npoints does not fit a 32-bit index"),
             ({"levels": 11, "tets": TETS_HI}, LEVELS_BIG),
             ({"tets": TETS_LO}, TET_RANGE), ({"tets": TETS_HI}, TET_RANGE), ({"tris": TRIS_LO}, TRI_RANGE), ({"tris": TRIS_HI}, TRI_RANGE),
             ({"tets": TETS_HI, "tris": TRIS_LO}, TET_RANGE)]
NEGATIVE = "a count is negative"
LOC_BIG = "npoints or 32*ntets does not fit a 32-bit index"
LOCATOR_CREATE = [({"npoints": -1}, NEGATIVE), ({"ntets": -1}, NEGATIVE), ({"cell_target": -1}, NEGATIVE), ({"cell_target": -1, "points": None}, NEGATIVE),
                  ({"out": None}, BAD), ({"points": None}, BAD), ({"tets": None}, BAD), ({"npoints": 0}, BAD), ({"ntets": 0}, BAD),
                  ({"npoints": INT_MAX + 1}, LOC_BIG), ({"ntets": INT_MAX // 32 + 1}, LOC_BIG), ({"ntets": INT_MAX // 32 + 1, "out": None}, BAD),
                  ({"tets": TETS_LO}, TET_RANGE), ({"tets": TETS_HI}, TET_RANGE), ({"points": PTS_NAN}, "points holds a coordinate that is not finite"),
                  ({"points": changed(PTS, 14, -np.inf)}, "points holds a coordinate that is not finite"), ({"points": PTS_NAN, "tets": TETS_HI}, TET_RANGE)]

TABLE = {
    "wae_p1_assemble": p1_mesh_rows("ntets", "tets", TETS_LO, TETS_HI, TET_RANGE, False, (1 << 28, P1_BIG)),
    "wae_p1_assemble_cpoint": p1_mesh_rows("ntets", "tets", TETS_LO, TETS_HI, TET_RANGE, True, (1 << 28, P1_BIG)),
    "wae_p1_assemble_boundary": p1_mesh_rows("ntris", "tris", TRIS_LO, TRIS_HI, TRI_RANGE, False),
    "wae_p1_assemble_boundary_cpoint": p1_mesh_rows("ntris", "tris", TRIS_LO, TRIS_HI, TRI_RANGE, True),
    "wae_p1_assemble_source": p1_source_rows(False),
    "wae_p1_assemble_source_cpoint": p1_source_rows(True),
    "wae_p1_assemble_flame": P1_FLAME,
    # h = inf and negative pair counts pass the checks of the per-simplex entry (test_valid_calls_reach_the_device), not of the nodal one
    "wae_p1_shape_sensitivity": P1_SHAPE + [({"c_tri": None}, S_PAIRS)],
    "wae_p1_shape_sensitivity_cpoint": P1_SHAPE + [({"h": np.inf}, H_STEP), ({"h": np.inf, "npair_t": -1}, H_STEP), ({"npair_t": -1}, BAD), ({"npair_s": -2}, BAD),
                                                   ({"c_point": None}, CP_NULL), ({"c_point": C_NAN}, CP_FIN), ({"npair_t": -1, "c_point": None}, BAD),
                                                   ({"c_point": None, "out_t": None}, CP_NULL), ({"c_point": C_INF, "tets": TETS_HI}, CP_FIN),
                                                   ({"h": np.nan, "c_point": None}, BAD)],
    "wae_p1_shape_sensitivity_flame": P1_SHAPE_FLAME,
    "wae_p2_connectivity": [({"out": None}, BAD), ({"out": None, "tets": TETS_HI}, BAD)] + p2_mesh_rows(True),
    "wae_p2_assemble": p2_assembly_rows(False, False),
    "wae_p2_assemble_cpoint": p2_assembly_rows(False, True),
    "wae_p2_assemble_boundary": p2_assembly_rows(True, False) + [({"ntris": 0}, BAD), ({"ntris": 0, "tets": TETS_HI}, BAD)],
    "wae_p2_assemble_boundary_cpoint": p2_assembly_rows(True, True) + [({"ntris": 0}, BAD), ({"c": None, "tris": TRIS_HI}, TRI_RANGE)],
    "wae_p2_assemble_source": p2_assembly_rows(True, False) + [({"nout": 0}, BAD), ({"nout": -1}, BAD), ({"nout": 0, "tets": TETS_HI}, BAD)],
    "wae_p2_assemble_source_cpoint": p2_assembly_rows(True, True) + [({"nout": 0}, BAD), ({"nout": 0, "c": None}, BAD)],
    "wae_p2_assemble_flame": P2_FLAME,
    "wae_p2_shape_sensitivity": P2_SHAPE,
    "wae_p2_shape_sensitivity_cpoint": P2_SHAPE + [({"c_point": None}, CP_NULL), ({"c_point": C_NAN}, CP_FIN), ({"c_point": C_INF}, CP_FIN),
                                                   ({"c_point": None, "tets": TETS_HI}, TET_RANGE), ({"c_point": None, "pair_tet": i32(0, NT)}, CP_NULL),
                                                   ({"c_point": C_NAN, "npair_t": INT_MAX // 3 + 1}, PAIRS3_BIG),
                                                   ({"c_point": C_NAN, "npair_t": 0, "npair_s": 0, "nv": 0}, CP_FIN)],
    "wae_p2_shape_sensitivity_flame": P2_SHAPE_FLAME,
    "wae_bloch_numbering": BLOCH_NUMBERING,
    "wae_bloch_fold": BLOCH_FOLD,
    "wae_octosplit": OCTOSPLIT,
    "wae_locator_create": LOCATOR_CREATE,
}
assert set(TABLE) == set(SPEC)
ROWS = [pytest.param(name, over, msg, id=f"{name}-{i}") for name, rows in TABLE.items() for i, (over, msg) in enumerate(rows)]


@pytest.mark.parametrize("name, over, msg", ROWS)
def test_bad_call(name, over, msg):
    code, text, _ = call(name, **over)
    assert (code, text) == (INV, msg)


# ---- calls that end before the device is touched, with success ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["wae_p1_assemble_source", "wae_p1_assemble_source_cpoint"])
def test_the_empty_speaker_is_the_zero_vector_without_a_device(name):
    L = _lib.lib()
    out = np.full(NP, 7.0)
    c = C_POINT if name.endswith("cpoint") else None
    dp = C.POINTER(C.c_double)
    code = getattr(L, name)(0, NP, PTS.ctypes.data_as(dp), 0, None, None if c is None else c.ctypes.data_as(dp), out.ctypes.data_as(dp))
    assert code == 0 and not out.any()


@pytest.mark.parametrize("name", ["wae_p2_shape_sensitivity", "wae_p2_shape_sensitivity_cpoint"])
def test_p2_shape_with_empty_pair_lists_checks_nv_on_the_host(name):
    code, _, _ = call(name, npair_t=0, npair_s=0)
    assert code == 0
    code, _, _ = call(name, npair_t=0, npair_s=0, pair_pt_t=None, pair_tet=None, out_t=None, tris=None, pair_pt_s=None, pair_tri=None, out_s=None, omegaY=None)
    assert code == 0


@pytest.mark.parametrize("nparts", [3, 6])
def test_fold_of_an_empty_matrix_returns_empty_parts_without_a_device(nparts):
    L = _lib.lib()
    code, _, handles = call("wae_bloch_fold", rowptr=i32(0, 0, 0, 0), col=None, nparts=nparts)
    assert code == 0
    try:
        for p in range(nparts):
            n, nnz = C.c_int64(-1), C.c_int64(-1)
            assert L.wae_p1_info(C.c_void_p(handles[p]), C.byref(n), C.byref(nnz)) == 0 and (n.value, nnz.value) == (2, 0)
            rowptr = np.full(3, -1, dtype=np.int32)
            assert L.wae_p1_get(C.c_void_p(handles[p]), rowptr.ctypes.data_as(C.POINTER(C.c_int32)), None, None, None) == 0 and not rowptr.any()
    finally:
        for p in range(nparts):
            L.wae_p1_free(C.c_void_p(handles[p]))


# ---- the entries that take a handle: a null handle ---------------------------------------------------------------------------------------------
def null_handle_calls():
    L = _lib.lib()
    one = np.ones(40)
    d, i = one.ctypes.data_as(C.POINTER(C.c_double)), np.zeros(40, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    return {
        "wae_p1_info": lambda: L.wae_p1_info(None, None, None),
        "wae_p1_get": lambda: L.wae_p1_get(None, None, None, None, None),
        "wae_p2_connectivity_info": lambda: L.wae_p2_connectivity_info(None, None, None, None),
        "wae_p2_connectivity_get": lambda: L.wae_p2_connectivity_get(None, None, None, None),
        "wae_p2_embedding": lambda: L.wae_p2_embedding(None, NP, i, i, d),
        "wae_bloch_numbering_info": lambda: L.wae_bloch_numbering_info(None, None, None, None, None, None),
        "wae_bloch_numbering_get": lambda: L.wae_bloch_numbering_get(None, None, None, None),
        "wae_octosplit_info": lambda: L.wae_octosplit_info(None, 0, None, None, None),
        "wae_octosplit_get": lambda: L.wae_octosplit_get(None, 0, None, None, None, None, None, None),
        "wae_octosplit_prolong": lambda: L.wae_octosplit_prolong(None, 0, 1, 1, d, d),
        "wae_octosplit_prolongator": lambda: L.wae_octosplit_prolongator(None, 0, i, i, d),
        "wae_octosplit_p2_info": lambda: L.wae_octosplit_p2_info(None, 0, None, None, None),
        "wae_octosplit_prolongator_p2": lambda: L.wae_octosplit_prolongator_p2(None, 0, i, i, d),
        "wae_octosplit_prolong_p2": lambda: L.wae_octosplit_prolong_p2(None, 0, 1, 1, d, d),
        "wae_locator_info": lambda: L.wae_locator_info(None, None, None, None, None, None),
        "wae_locator_find": lambda: L.wae_locator_find(None, 1, d, 0.0, i, d),
        "wae_locator_set_p2": lambda: L.wae_locator_set_p2(None, NV, i),
        "wae_locator_weights": lambda: L.wae_locator_weights(None, 1, 0, 1, d, i, None, i, d),
        "wae_locator_sample": lambda: L.wae_locator_sample(None, 1, 0, 1, d, i, None, NP, 1, d, d),
    }, (one,)


NULL_HANDLE_ENTRIES = ["wae_p1_info", "wae_p1_get", "wae_p2_connectivity_info", "wae_p2_connectivity_get", "wae_p2_embedding", "wae_bloch_numbering_info",
                       "wae_bloch_numbering_get", "wae_octosplit_info", "wae_octosplit_get", "wae_octosplit_prolong", "wae_octosplit_prolongator",
                       "wae_octosplit_p2_info", "wae_octosplit_prolongator_p2", "wae_octosplit_prolong_p2", "wae_locator_info", "wae_locator_find",
                       "wae_locator_set_p2", "wae_locator_weights", "wae_locator_sample"]


@pytest.mark.parametrize("name", NULL_HANDLE_ENTRIES)
def test_null_handle(name):
    calls, _keep = null_handle_calls()
    assert set(calls) == set(NULL_HANDLE_ENTRIES)
    assert calls[name]() == INV
    assert _lib.lib().wae_last_error().decode() == NULL_HANDLE


@pytest.mark.parametrize("name", ["wae_p1_free", "wae_p2_connectivity_free", "wae_bloch_numbering_free", "wae_octosplit_free", "wae_locator_free"])
def test_free_of_a_null_handle_is_ok(name):
    assert getattr(_lib.lib(), name)(None) == 0


def test_every_mesh_side_entry_is_covered():
    mesh_side = [s for s in _lib.EXPORTS if s.startswith(("wae_p1_", "wae_p2_", "wae_bloch_", "wae_octosplit", "wae_locator_"))]
    covered = set(SPEC) | set(NULL_HANDLE_ENTRIES) | {"wae_p1_free", "wae_p2_connectivity_free", "wae_bloch_numbering_free", "wae_octosplit_free",
                                                     "wae_locator_free"}
    assert set(mesh_side) == covered


# ---- valid calls: every check passes, the device is missing ------------------------------------------------------------------------------------
VALID = [(name, {}) for name in SPEC] + [
    ("wae_p1_assemble", {"c": np.ones(NT)}), ("wae_p1_assemble_boundary", {"c": np.ones(NS)}), ("wae_p1_assemble_source", {"c": np.ones(NS)}),
    ("wae_p1_assemble_flame", {"volume_out": None}),
    # the per-simplex P1 entry tests h > 0 alone, and no pair count: today these go through
    ("wae_p1_shape_sensitivity", {"h": np.inf}), ("wae_p1_shape_sensitivity", {"npair_t": -1}), ("wae_p1_shape_sensitivity", {"npair_s": -1}),
    ("wae_p1_shape_sensitivity", {"npair_t": 0, "tets": None, "pair_pt_t": None, "pair_tet": None, "out_t": None, "ntets": 0}),
    ("wae_p1_shape_sensitivity", {"npair_s": 0, "tris": None, "c_tri": None, "pair_pt_s": None, "pair_tri": None, "out_s": None, "omegaY": None, "ntris": 0}),
    ("wae_p1_shape_sensitivity", {"c_tet": np.ones(NT)}),
    ("wae_p1_shape_sensitivity_flame", {"h": np.inf}), ("wae_p1_shape_sensitivity_flame", {"npair": 0, "pair_pt": None, "pair_tet": None, "det_pm": None, "ssum": None}),
    ("wae_p1_shape_sensitivity_flame", {"npair_r": 0, "pair_pt_r": None, "g_pm": None}), ("wae_p1_shape_sensitivity_flame", {"npair": -1, "npair_r": -1}),
    ("wae_p2_connectivity", {"ntris": 0, "tris": None}), ("wae_p2_assemble_source", {"ntris": 0, "tris": None}), ("wae_p2_assemble_source", {"nout": 1}),
    ("wae_p2_shape_sensitivity", {"nv": 1}), ("wae_p2_shape_sensitivity", {"c_tet": np.ones(NT), "c_tri": np.ones(NS)}),
    ("wae_p2_shape_sensitivity", {"npair_s": 0, "tris": None, "pair_pt_s": None, "pair_tri": None, "out_s": None, "omegaY": None, "ntris": 0}),
    ("wae_p2_shape_sensitivity", {"npair_s": 0, "tris": TRIS_HI}),
    ("wae_p2_shape_sensitivity_flame", {"npair": 0, "npair_r": 0, "pair_pt": None, "pair_tet": None, "det_pm": None, "ssum": None, "pair_pt_r": None, "g_pm": None}),
    ("wae_bloch_numbering", {"order": 1}), ("wae_bloch_numbering", {"nsector": NP, "naxis": 0}), ("wae_bloch_fold", {"v1": VALS, "nparts": 6}),
    ("wae_octosplit", {"ntris": 0, "tris": None, "levels": 9}), ("wae_locator_create", {"cell_target": 3}),
]


@pytest.mark.parametrize("name, over", [pytest.param(n, o, id=f"{n}-{i}") for i, (n, o) in enumerate(VALID)])
def test_valid_calls_reach_the_device(name, over):
    n = C.c_int(0)
    if _lib.lib().wae_device_count(C.byref(n)) == 0 and n.value > 0:
        pytest.skip("GPU present")
    code, text, _ = call(name, **over)
    assert code == HIP and text.startswith("hipSetDevice(device)"), (code, text)


# ---- behind a handle: the checks of the locator's and the refinement's queries (these need a device) ------------------------------------------
def _pinned(L, rows):
    for i, (fn, code, msg) in enumerate(rows):
        got = fn()
        text = L.wae_last_error().decode()
        assert got == code and (code == 0 or text == msg), (i, got, text)


@pytest.mark.gpu
def test_locator_queries_behind_the_handle():
    L = _lib.lib()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    code, text, handles = call("wae_locator_create")
    assert code == 0, text
    h = C.c_void_p(handles[0])
    x = np.array([[0.1, 0.1, 0.1], [0.9, 0.9, 0.8]])
    x_nan = changed(x, 4, np.nan)
    tet, tet_lo, tet_hi = i32(0, 1), i32(-2, 1), i32(0, NT)
    n = np.ones((2, 3))
    t10 = np.arange(NT * 10, dtype=np.int32) % NV
    V, out = np.ones(2 * NV * 2), np.zeros(64)
    idx = np.zeros(64, dtype=np.int32)
    X, XN, T, TL, TH, N, T10, VV, O, I = (x.ctypes.data_as(dp), x_nan.ctypes.data_as(dp), tet.ctypes.data_as(ip), tet_lo.ctypes.data_as(ip),
                                          tet_hi.ctypes.data_as(ip), n.ctypes.data_as(dp), t10.ctypes.data_as(ip), V.ctypes.data_as(dp),
                                          out.ctypes.data_as(dp), idx.ctypes.data_as(ip))
    TOL, ORDER, KIND = "tol must lie in [0, 1e-6]", "order must be 1 or 2", "kind must be 0 (p) or 1 (n.grad p)"
    X_FIN, TET_RANGE_Q = "x holds a coordinate that is not finite", "tet holds an index outside -1..ntets-1"
    try:
        _pinned(L, [
            (lambda: L.wae_locator_find(h, -1, X, 0.0, I, O), INV, "nq is negative"), (lambda: L.wae_locator_find(h, -1, X, -1.0, I, O), INV, "nq is negative"),
            (lambda: L.wae_locator_find(h, 2, X, -1e-9, I, O), INV, TOL), (lambda: L.wae_locator_find(h, 2, X, 2e-6, I, O), INV, TOL),
            (lambda: L.wae_locator_find(h, 2, X, np.nan, I, O), INV, TOL), (lambda: L.wae_locator_find(h, 0, None, 2e-6, None, None), INV, TOL),
            (lambda: L.wae_locator_find(h, 0, None, 0.0, None, None), 0, ""), (lambda: L.wae_locator_find(h, 2, None, 0.0, I, O), INV, BAD),
            (lambda: L.wae_locator_find(h, 2, X, 0.0, None, O), INV, BAD), (lambda: L.wae_locator_find(h, 2, XN, 0.0, I, O), INV, X_FIN),
            (lambda: L.wae_locator_find(h, 2, XN, 0.0, None, O), INV, BAD), (lambda: L.wae_locator_find(h, 2, X, 1e-6, I, None), 0, ""),
            (lambda: L.wae_locator_weights(h, 1, 0, -1, X, T, None, I, O), INV, "nq is negative"), (lambda: L.wae_locator_weights(h, 3, 0, 0, X, T, None, I, O), 0, ""),
            (lambda: L.wae_locator_weights(h, 0, 0, 2, X, T, None, I, O), INV, ORDER), (lambda: L.wae_locator_weights(h, 3, 2, 2, X, T, None, I, O), INV, ORDER),
            (lambda: L.wae_locator_weights(h, 1, -1, 2, X, T, None, I, O), INV, KIND), (lambda: L.wae_locator_weights(h, 2, 2, 2, X, T, None, I, O), INV, KIND),
            (lambda: L.wae_locator_weights(h, 2, 1, 2, X, T, None, I, O), INV, "order 2 needs wae_locator_set_p2 first"),
            (lambda: L.wae_locator_weights(h, 1, 1, 2, None, T, None, I, O), INV, "kind 1 needs the directions n"),
            (lambda: L.wae_locator_weights(h, 1, 0, 2, None, T, None, I, O), INV, BAD), (lambda: L.wae_locator_weights(h, 1, 0, 2, X, None, None, I, O), INV, BAD),
            (lambda: L.wae_locator_weights(h, 1, 0, 2, XN, TH, None, I, O), INV, X_FIN), (lambda: L.wae_locator_weights(h, 1, 0, 2, X, TL, None, I, O), INV, TET_RANGE_Q),
            (lambda: L.wae_locator_weights(h, 1, 0, 2, X, TH, None, None, O), INV, TET_RANGE_Q), (lambda: L.wae_locator_weights(h, 1, 0, 2, X, T, None, None, O), INV, BAD),
            (lambda: L.wae_locator_weights(h, 1, 1, 2, X, T, N, I, None), INV, BAD), (lambda: L.wae_locator_weights(h, 1, 1, 2, X, T, N, I, O), 0, ""),
            (lambda: L.wae_locator_sample(h, 1, 0, -1, X, T, None, NP, 1, VV, O), INV, NEGATIVE), (lambda: L.wae_locator_sample(h, 1, 0, 2, X, T, None, -1, 1, VV, O), INV, NEGATIVE),
            (lambda: L.wae_locator_sample(h, 1, 0, 2, X, T, None, NP, -1, VV, O), INV, NEGATIVE), (lambda: L.wae_locator_sample(h, 0, 0, 0, X, T, None, 1, 0, None, None), 0, ""),
            (lambda: L.wae_locator_sample(h, 0, 0, 2, X, T, None, 1, 0, None, None), INV, ORDER),
            (lambda: L.wae_locator_sample(h, 1, 0, 2, X, TH, None, NP + 1, 1, VV, O), INV, TET_RANGE_Q),
            (lambda: L.wae_locator_sample(h, 1, 0, 2, X, T, None, NP + 1, 0, None, O), INV, "d must be npoints (order 1) or ndof (order 2)"),
            (lambda: L.wae_locator_sample(h, 1, 0, 2, X, T, None, NP, 1, None, O), INV, BAD), (lambda: L.wae_locator_sample(h, 1, 0, 2, X, T, None, NP, 1, VV, None), INV, BAD),
            (lambda: L.wae_locator_sample(h, 1, 0, 2, X, T, None, NP, 0, VV, O), INV, BAD), (lambda: L.wae_locator_sample(h, 1, 0, 2, X, T, None, NP, 2, VV, O), 0, ""),
            (lambda: L.wae_locator_set_p2(h, -1, None), INV, "ndof is negative"), (lambda: L.wae_locator_set_p2(h, NV, None), INV, BAD),
            (lambda: L.wae_locator_set_p2(h, 0, T10), INV, BAD), (lambda: L.wae_locator_set_p2(h, INT_MAX + 1, T10), INV, BAD),
            (lambda: L.wae_locator_set_p2(h, NV - 1, T10), INV, "tets10 holds an entry outside 0..ndof-1"), (lambda: L.wae_locator_set_p2(h, NV, T10), 0, ""),
            (lambda: L.wae_locator_sample(h, 2, 0, 2, X, T, None, NP, 1, VV, O), INV, "d must be npoints (order 1) or ndof (order 2)"),
            (lambda: L.wae_locator_sample(h, 2, 1, 2, X, T, N, NV, 2, VV, O), 0, ""), (lambda: L.wae_locator_weights(h, 2, 0, 2, X, T, None, I, O), 0, ""),
        ])
    finally:
        L.wae_locator_free(h)


@pytest.mark.gpu
def test_refinement_queries_behind_the_handle():
    L = _lib.lib()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    code, text, handles = call("wae_octosplit")                     # two levels
    assert code == 0, text
    h = C.c_void_p(handles[0])
    buf, ibuf = np.ones(8192), np.zeros(8192, dtype=np.int32)
    D, I = buf.ctypes.data_as(dp), ibuf.ctypes.data_as(ip)
    LEVEL, LAST, ORDERED = "level outside 0..levels", "from_level must be below the last level", "prolongation needs from_level < to_level"
    try:
        _pinned(L, [
            (lambda: L.wae_octosplit_info(h, -1, None, None, None), INV, LEVEL), (lambda: L.wae_octosplit_info(h, 3, None, None, None), INV, LEVEL),
            (lambda: L.wae_octosplit_info(h, 2, None, None, None), 0, ""), (lambda: L.wae_octosplit_get(h, 3, D, I, I, I, I, I), INV, LEVEL),
            (lambda: L.wae_octosplit_get(h, 0, None, None, None, I, None, None), INV, "level 0 is the input: it has no parents and no labels"),
            (lambda: L.wae_octosplit_get(h, 0, None, None, None, None, None, I), INV, "level 0 is the input: it has no parents and no labels"),
            (lambda: L.wae_octosplit_get(h, 0, D, I, I, None, None, None), 0, ""), (lambda: L.wae_octosplit_get(h, 1, None, None, None, I, I, I), 0, ""),
            (lambda: L.wae_octosplit_prolong(h, 3, 1, 1, D, D), INV, LEVEL), (lambda: L.wae_octosplit_prolong(h, 0, 3, 1, D, D), INV, LEVEL),
            (lambda: L.wae_octosplit_prolong(h, 1, 1, 1, D, D), INV, ORDERED), (lambda: L.wae_octosplit_prolong(h, 2, 1, 0, None, D), INV, ORDERED),
            (lambda: L.wae_octosplit_prolong(h, 0, 1, 1, None, D), INV, BAD), (lambda: L.wae_octosplit_prolong(h, 0, 1, 1, D, None), INV, BAD),
            (lambda: L.wae_octosplit_prolong(h, 0, 1, 0, D, D), INV, BAD), (lambda: L.wae_octosplit_prolong(h, 0, 2, 2, D, D), 0, ""),
            (lambda: L.wae_octosplit_prolongator(h, -1, I, I, D), INV, LEVEL), (lambda: L.wae_octosplit_prolongator(h, 2, I, I, D), INV, LAST),
            (lambda: L.wae_octosplit_prolongator(h, 2, None, I, D), INV, LAST), (lambda: L.wae_octosplit_prolongator(h, 1, None, I, D), INV, BAD),
            (lambda: L.wae_octosplit_prolongator(h, 1, I, None, D), INV, BAD), (lambda: L.wae_octosplit_prolongator(h, 1, I, I, None), INV, BAD),
            (lambda: L.wae_octosplit_prolongator(h, 1, I, I, D), 0, ""),
            (lambda: L.wae_octosplit_p2_info(h, 3, None, None, None), INV, LEVEL), (lambda: L.wae_octosplit_p2_info(h, 2, None, None, None), 0, ""),
            (lambda: L.wae_octosplit_prolongator_p2(h, 3, I, I, D), INV, LEVEL), (lambda: L.wae_octosplit_prolongator_p2(h, 2, None, I, D), INV, LAST),
            (lambda: L.wae_octosplit_prolongator_p2(h, 0, None, I, D), INV, BAD), (lambda: L.wae_octosplit_prolongator_p2(h, 0, I, I, None), INV, BAD),
            (lambda: L.wae_octosplit_prolongator_p2(h, 0, I, I, D), 0, ""),
            (lambda: L.wae_octosplit_prolong_p2(h, 0, 3, 1, D, D), INV, LEVEL), (lambda: L.wae_octosplit_prolong_p2(h, 2, 2, 1, D, D), INV, ORDERED),
            (lambda: L.wae_octosplit_prolong_p2(h, 0, 1, 1, None, D), INV, BAD), (lambda: L.wae_octosplit_prolong_p2(h, 0, 1, 0, D, D), INV, BAD),
            (lambda: L.wae_octosplit_prolong_p2(h, 0, 2, 2, D, D), 0, ""),
        ])
    finally:
        L.wae_octosplit_free(h)
