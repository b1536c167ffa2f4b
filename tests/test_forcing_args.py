"""The Python side of the forced response (helmholtz/assemble.py, helmholtz/probe.py, nlevp/forcing.py), as far as it runs without a device:
the argument errors of the wrappers, each raised before the library is entered."""
import numpy as np
import pytest
import scipy.sparse as sp

from wae_amd.helmholtz.assemble import assemble_p1_source, assemble_p2_source
from wae_amd.helmholtz.family import helmholtz_family, speaker_source
from wae_amd.helmholtz.probe import find_tetrahedron, probe_n_grad_p, probe_p
from wae_amd.nlevp import forced_response
from wae_amd.nlevp.algebra import pow1

PTS = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 1.0, 1.0]])
TETS = np.array([[0, 1, 2, 3], [1, 2, 3, 4]], dtype=np.int32)
TRIS = np.array([[0, 1, 2]], dtype=np.int32)
D = 5


@pytest.mark.parametrize("call", [lambda **kw: assemble_p1_source(PTS, TRIS, **kw), lambda **kw: assemble_p2_source(PTS, TETS, TRIS, **kw)])
def test_source_arguments(call):
    with pytest.raises(ValueError):
        call(c_point=np.ones(5), c_tri=np.ones(1))
    for n in (1, 4, 6):
        with pytest.raises(ValueError):
            call(c_point=np.ones(n))
    for n in (0, 2, 5):
        with pytest.raises(ValueError):
            call(c_tri=np.ones(n))


def families():
    eye = sp.identity(D, dtype=np.complex128, format="csr")
    L = helmholtz_family({"M": eye, "K": eye, "C": eye, "Q": eye})
    m = sp.csc_matrix(([1.0 - 2.0j, 0.5j], ([1, 3], [0, 0])), shape=(D, 1))
    return L, speaker_source(m, Y=2.0, A=3.0)


def test_speaker_source_is_the_rhs_family_of_the_reference():
    L, rhs = families()
    assert rhs.eigval == "ω" and rhs.auxval == "" and list(rhs.params) == ["ω", "Y", "A"]
    (term,) = rhs.terms
    assert term.func == (pow1, pow1, pow1) and term.params == (("ω",), ("Y",), ("A",)) and (term.symbol, term.operator) == ("speaker", "m")
    rhs.active, rhs.mode = ["ω"], "all"
    assert rhs.coefficients(7.0)[0] == 7.0 * 2.0 * 3.0
    assert L._fam is None                                             # helmholtz_family is untouched, no device yet


@pytest.mark.parametrize("kw", [
    dict(observers=[(np.array([0, D]), np.ones(2))]),                 # an observer index beyond d
    dict(observers=[(np.array([-1]), np.ones(1))]),
    dict(observers=[(np.array([0, 1]), np.ones(3))]),                 # wrong shapes
    dict(observers=[(np.array([[0, 1]]), np.ones((1, 2)))]),
    dict(observers=[(np.array([0.5]), np.ones(1))]),
    dict(observers=[(np.array([0]), np.array([np.nan]))]),
    dict(observers=[np.arange(3)]),
    dict(keep=[1, 0]),                                                # a keep that is not ascending
    dict(keep=[0, 0]),
    dict(keep=[3]),
    dict(keep=[-1]),
    dict(),                                                           # nothing asked for
])
def test_forced_response_arguments(kw):
    L, rhs = families()
    kw.setdefault("keep", [0] if "observers" in kw else [])
    with pytest.raises(ValueError):
        forced_response(L, rhs, [1.0, 2.0, 3.0], **kw)
    assert L._fam is None and rhs._fam is None                        # refused before a device handle was made


def test_forced_response_refuses_a_source_of_the_wrong_size():
    L, _ = families()
    rhs = speaker_source(sp.csc_matrix((D + 1, 1), dtype=np.complex128))
    with pytest.raises(ValueError):
        forced_response(L, rhs, [1.0], keep=[0])
    with pytest.raises(ValueError):
        forced_response(L, families()[1], np.ones((2, 2)), keep=[0])
    assert L._fam is None


def test_forced_response_restores_the_families():
    L, rhs = families()
    L.params["ω"], L.active, L.mode = 5.0 + 0j, ["ω", "λ"], "compact"
    saved = dict(L.params), list(L.active), L.mode, dict(rhs.params)
    with pytest.raises(ValueError):
        forced_response(L, rhs, [1.0, 2.0], keep=[1, 1])
    assert (dict(L.params), list(L.active), L.mode, dict(rhs.params)) == saved


def test_probe_arguments():
    with pytest.raises(ValueError):
        find_tetrahedron(PTS, TETS, [5.0, 5.0, 5.0])                  # outside the mesh
    with pytest.raises(ValueError):
        find_tetrahedron(PTS, TETS, [0.1, 0.1])
    with pytest.raises(ValueError):
        probe_p(PTS, TETS, [0.1, 0.1, 0.1], order="herm")
    with pytest.raises(ValueError):
        probe_p(PTS, TETS, [0.1, 0.1, 0.1], tet=2)
    with pytest.raises(ValueError):
        probe_n_grad_p(PTS, TETS, [0.1, 0.1, 0.1], [1.0, 0.0])
    assert find_tetrahedron(PTS, TETS, [0.1, 0.1, 0.1]) == 0 and find_tetrahedron(PTS, TETS, [0.6, 0.6, 0.6]) == 1
    idx, w = probe_p(PTS, TETS, [0.1, 0.2, 0.3])
    assert idx.tolist() == [0, 1, 2, 3] and np.allclose(w, [0.4, 0.1, 0.2, 0.3], atol=1e-15)
