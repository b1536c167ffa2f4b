"""The Python side of the nodal speed of sound (helmholtz/assemble.py), as far as it runs without a device: how the length of a
speed-of-sound array picks its meaning (the rule of `discretize`, Helmholtz.jl:59-74), and the argument checks of the c_point= keyword,
which refuse before the library is touched."""
import numpy as np
import pytest

from wae_amd.helmholtz.assemble import assemble_p1, assemble_p1_boundary, assemble_p2, assemble_p2_boundary, speed_of_sound_kind

PTS = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 1.0, 1.0]])
TETS = np.array([[0, 1, 2, 3], [1, 2, 3, 4]], dtype=np.int32)
TRIS = np.array([[0, 1, 2]], dtype=np.int32)


def test_speed_of_sound_kind():
    assert speed_of_sound_kind(np.ones(2), 5, 2) == "tet"
    assert speed_of_sound_kind(np.ones(5), 5, 2) == "point"
    assert speed_of_sound_kind([1.0] * 4, 4, 4) == "tet"                 # the tetrahedron count is tested first
    for n in (0, 3, 6):
        with pytest.raises(ValueError):
            speed_of_sound_kind(np.ones(n), 5, 2)


@pytest.mark.parametrize("call", [lambda **kw: assemble_p1(PTS, TETS, **kw), lambda **kw: assemble_p2(PTS, TETS, **kw)])
def test_interior_arguments(call):
    with pytest.raises(ValueError):
        call(c_point=np.ones(5), c_tet=np.ones(2))
    for n in (2, 4, 6):
        with pytest.raises(ValueError):
            call(c_point=np.ones(n))


@pytest.mark.parametrize("call", [lambda **kw: assemble_p1_boundary(PTS, TRIS, **kw), lambda **kw: assemble_p2_boundary(PTS, TETS, TRIS, **kw)])
def test_boundary_arguments(call):
    with pytest.raises(ValueError):
        call(c_point=np.ones(5), c_tri=np.ones(1))
    for n in (1, 4, 6):
        with pytest.raises(ValueError):
            call(c_point=np.ones(n))
