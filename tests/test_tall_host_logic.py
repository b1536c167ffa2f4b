"""The host half of `moments2eigs_native` (wae_amd.nlevp.tall.staged_extract: deflation in stages, second Cholesky-QR pass, exact
SVD of the kept group, U^H B1 W S^-1, eig) on a numpy stand-in for the three tall-matrix operations: pins the algorithm where no GPU
exists; tests/test_gpu_tall.py then only has to show that the device primitives are right."""
import numpy as np
import pytest

import wae_amd  # noqa: F401
from wae_amd.nlevp.beyn import moments2eigs, moments2eigs_native

import _tallcases as T


@pytest.mark.parametrize("l,K", [(5, 2), (8, 1)])
def test_rank6_known_answer_on_the_numpy_stand_in(l, K):
    """(5, 2): l < 6 forces the Hankel path; (8, 1): B0 and B1 are column ranges of the moments themselves"""
    A, _ = T.rank6_moments(l, K)
    d = A.shape[0]
    M = T.NumpyTall(A.reshape(d, -1, order="F"))
    before = M.a.copy()
    info = {}
    Om, P, Sall = moments2eigs_native(M, (d, l, 2 * K), rel_tol=1e-6, info=info)
    assert info["stages"] == 1 and info["kept"] == 6 and len(Sall) == l * K
    assert np.array_equal(M.a, before)                      # the moments are read, never written (K = 1: B0 is M itself)
    T.check_rank6(Om, P.to_host(), Sall, l, K, f"numpy stand-in l={l} K={K}")


def test_two_groups_twelve_decades_apart_need_two_stages():
    A, s, Tm = T.two_group_moments()
    d = A.shape[0]
    info = {}
    Om, P, Sall = moments2eigs_native(T.NumpyTall(A.reshape(d, -1, order="F")), (d, 6, 2), rel_tol=0.0, info=info)
    assert info["stages"] == 2 and info["kept"] == 6 and P.ncols == 6 and len(Om) == 6
    # the large group to rounding; the small one as well as 1e-12-sized singular values of a matrix of norm 1 are defined at all
    # (perturbations of eps = 2e-16 of the matrix move them by 2e-4 relative)
    assert np.allclose(Sall[:3], s[:3], rtol=1e-12) and np.allclose(Sall[3:], s[3:], rtol=1e-2)
    Om_h, _ = moments2eigs(np.array(A))
    want = np.linalg.eigvals(Tm)
    err = lambda X: max(np.min(np.abs(X - w)) for w in want) / np.abs(want).max()      # noqa: E731
    print(f"two groups: eigenvalue error native {err(Om):.2e} host {err(Om_h):.2e}")
    assert err(Om) <= T.FACTOR * err(Om_h) + 1e-3            # (both routes see the small group through a 1e-4 perturbation)


def test_tol_sigma_and_the_uploaded_form_agree_with_the_handle_form():
    """tol_sigma (absolute, the reference's `tol`) on top of rel_tol = 0 keeps the same six directions"""
    A, _ = T.rank6_moments(5, 2)
    d = A.shape[0]
    s1 = T.host_reference(5, 2)[0][0]
    Om, P, Sall = moments2eigs_native(T.NumpyTall(A.reshape(d, -1, order="F")), (d, 5, 4), rel_tol=0.0, tol_sigma=1e-6 * s1)
    T.check_rank6(Om, P.to_host(), Sall, 5, 2, "numpy stand-in tol_sigma")
    with pytest.raises(ValueError):
        moments2eigs_native(T.NumpyTall(A.reshape(d, -1, order="F")), (d, 4, 4))
