"""The Python entries of the Hermite p-hierarchy refuse bad arguments with ValueError before the library is touched: on a machine without
a device a call that reached libwaehip.so would fail with a WaeError from hipSetDevice instead.  What the library itself refuses (indices
out of range, triangles that are no face, the size limits of wae_herm_connectivity) is covered on the device by tests/test_gpu_herm_mg.py."""
import numpy as np
import pytest

from wae_amd import _lib
from wae_amd.helmholtz import assemble as A
from wae_amd.helmholtz.family import helmholtz_family, herm_hierarchy
from wae_amd.nlevp.linopfam import DeviceFamily, LinearOperatorFamily

PTS = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 1.0, 1.0]])
TETS = np.array([[0, 1, 2, 3], [1, 2, 3, 4]], dtype=np.int32)
TRIS = np.array([[0, 1, 2]], dtype=np.int32)

BAD_MESHES = {
    "points with two columns": (PTS[:, :2], TETS, TRIS, "points"),
    "points as a flat vector": (PTS.reshape(-1), TETS, TRIS, "points"),
    "no points": (np.zeros((0, 3)), TETS, TRIS, "points"),
    "complex points": (PTS.astype(complex), TETS, TRIS, "points"),
    "points that are strings": (PTS.astype(str), TETS, TRIS, "points"),
    "a point that is not finite": (np.where(np.arange(15).reshape(5, 3) == 4, np.nan, PTS), TETS, TRIS, "points"),
    "tets with three columns": (PTS, TETS[:, :3], TRIS, "tets"),
    "tets as floats": (PTS, TETS.astype(np.float64), TRIS, "tets"),
    "tets as a flat vector": (PTS, TETS.reshape(-1), TRIS, "tets"),
    "no tets": (PTS, np.zeros((0, 4), dtype=np.int32), TRIS, "tets"),
    "a tet index beyond 32 bits": (PTS, TETS.astype(np.int64) + 2 ** 31, TRIS, "tets"),
    "tris with four columns": (PTS, TETS, TETS, "tris"),
    "tris as floats": (PTS, TETS, TRIS.astype(np.float32), "tris"),
    "tris as booleans": (PTS, TETS, TRIS.astype(bool), "tris"),
}


@pytest.mark.parametrize("what", list(BAD_MESHES))
def test_herm_prolongators_refuses_bad_arrays(what):
    pts, tets, tris, name = BAD_MESHES[what]
    with pytest.raises(ValueError, match=name):
        A.herm_prolongators(pts, tets, tris)


@pytest.mark.parametrize("bad", ["Spectral", "spectral ", "", b"spectral", 1, 1.0, True, False, ("spectral",), ["spectral"], 0])
def test_level_weights_is_none_or_spectral(bad):
    fam = DeviceFamily.__new__(DeviceFamily)            # no handle: the check comes before anything that would need one
    with pytest.raises(ValueError, match="level_weights"):
        fam.setup_solver(np.ones(3, dtype=complex), level_weights=bad)
    with pytest.raises(ValueError, match="level_weights"):
        fam.setup_solver(np.ones(3, dtype=complex), prolongators="nonsense", level_weights=bad)      # ... and before the prolongators' own


def test_nothing_is_switched_on_by_default():
    L = LinearOperatorFamily(["ω"], [0.0])
    assert L.solver_level_weights is None and L.solver_prolongators is None
    import scipy.sparse as sp
    I = sp.identity(4, format="csr", dtype=complex)
    Lh = helmholtz_family({"M": I, "K": I, "C": I, "Q": I})
    assert Lh.solver_level_weights is None and Lh.solver_prolongators is None


def test_herm_hierarchy_checks_the_mesh_first():
    L = LinearOperatorFamily(["ω"], [0.0])
    with pytest.raises(ValueError, match="tets"):
        herm_hierarchy(L, PTS, TETS[:, :3], TRIS)
    assert L.solver_level_weights is None and L.solver_prolongators is None


def test_the_new_entries_are_exported():
    for s in ("wae_hermite_prolongators", "wae_hermite_prolongators_info", "wae_hermite_prolongators_get", "wae_hermite_prolongators_free",
              "wae_solver_level_weights"):
        assert s in _lib.EXPORTS and hasattr(_lib.lib(), s)
    L = _lib.lib()
    assert L.wae_hermite_prolongators_info(None, 0, None, None, None) == _lib.WAE_ERR_INVALID and L.wae_last_error().decode() == "null handle"
    assert L.wae_hermite_prolongators_get(None, 0, None, None, None) == _lib.WAE_ERR_INVALID and L.wae_last_error().decode() == "null handle"
    assert L.wae_hermite_prolongators_free(None) == 0
    assert L.wae_solver_level_weights(None, 0, None, None, None) == _lib.WAE_ERR_INVALID
