"""The keywords order= and c_point= of the shape sensitivity (helmholtz/assemble.py, helmholtz/shape.py), as far as they run without a device:
every wrong combination is a ValueError raised before the library is touched -- `_lib.lib` is replaced by a function that fails the test."""
import numpy as np
import pytest

from wae_amd import _lib
from wae_amd.helmholtz import shape as SH
from wae_amd.helmholtz.assemble import discrete_adjoint_shape_sensitivity, p2_edge_count
from wae_amd.nlevp import Solution

PTS = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 1.0, 1.0]])
TETS = np.array([[0, 1, 2, 3], [1, 2, 3, 4]], dtype=np.int32)
TRIS = np.array([[0, 1, 2]], dtype=np.int32)
NP, NE = 5, 9                      # 6 + 6 edges, 3 of them shared
FLAME = {"flame_tets": [0], "ref_tet": 1, "n_ref": [0.0, 0.0, 1.0], "nglobal_scaled": 1.0, "coeff": 1.0}


@pytest.fixture(autouse=True)
def no_library(monkeypatch):
    def touched():
        raise AssertionError("the library was touched before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", touched)


def sol(n):
    return Solution({"ω": 1.0 + 0j}, np.ones(n, dtype=complex), np.ones(n, dtype=complex), "ω")


def adjoint(n=NP, **kw):
    kw.setdefault("v_ext", (np.ones(n, dtype=complex), np.ones(n, dtype=complex)))
    return discrete_adjoint_shape_sensitivity(PTS, TETS, kw.pop("c_tet", None), [0, 4], sol(n), None, **kw)


def forward(n=NP, **kw):
    return SH.forward_finite_differences_shape_sensitivity(PTS, TETS, kw.pop("c_tet", None), [0, 4], None, sol(n), **kw)


def test_edge_count():
    assert p2_edge_count(TETS) == NE and p2_edge_count(TETS[:1]) == 6


@pytest.mark.parametrize("call", [adjoint, forward])
def test_order_must_be_lin_or_quad(call):
    for bad in ("cubic", "P2", None, ""):
        with pytest.raises(ValueError):
            call(order=bad)


@pytest.mark.parametrize("call", [adjoint, forward])
@pytest.mark.parametrize("order", ["lin", "quad"])
def test_c_point_excludes_the_per_simplex_forms_and_has_one_value_per_point(call, order):
    n = NP + (NE if order == "quad" else 0)
    with pytest.raises(ValueError):
        call(n, order=order, c_point=np.ones(NP), c_tet=np.ones(2))
    with pytest.raises(ValueError):
        call(n, order=order, c_point=np.ones(NP), bnd_tris=TRIS, bnd_c=np.ones(1))
    for m in (2, NP - 1, NP + 1, NP + NE):
        with pytest.raises(ValueError):
            call(n, order=order, c_point=np.ones(m))


@pytest.mark.parametrize("order, good", [("lin", NP), ("quad", NP + NE)])
def test_vector_lengths(order, good):
    for n in (NP - 1, NP + 1, NP + NE - 1, NP + NE + 1, NP if order == "quad" else NP + NE):
        with pytest.raises(ValueError):
            adjoint(n, order=order)                                              # v_ext of the wrong length
        with pytest.raises(ValueError):
            adjoint(n, order=order, v_ext=None)                                  # sol.v, sol.v_adj of the wrong length
        with pytest.raises(ValueError):
            forward(n, order=order)
    one = np.ones(good, dtype=complex)
    with pytest.raises(ValueError):
        adjoint(good, order=order, v_ext=(one, one[:-1]))
    with pytest.raises(ValueError):
        adjoint(good, order=order, v_ext=(one[:-1], one))
    with pytest.raises(AssertionError, match="touched"):                         # right lengths: the call goes on to the library
        adjoint(good, order=order)


@pytest.mark.parametrize("call", [adjoint, forward])
def test_the_p2_flame_needs_x_ref(call):
    with pytest.raises(ValueError, match="x_ref"):
        call(NP + NE, order="quad", flame=FLAME)
    with pytest.raises(ValueError, match="x_ref"):
        call(NP + NE, order="quad", flame={**FLAME, "x_ref": None})


def test_an_integer_order_of_the_cross_check_is_still_the_order_of_householder():
    with pytest.raises(ValueError):
        forward(NP + NE, order=3)                                                # P1 elements: the vector is too long
