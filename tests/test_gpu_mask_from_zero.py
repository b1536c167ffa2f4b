"""The device recurrence of the lock-step GMRES masks converged 8-column chunks in solves from a ZERO guess too (csrc/gmres.hip
run_device): a system that has finished is skipped by every kernel while the slower ones of its batch go on, and the update x += V y
never reads the stale basis entries of its chunk (tests/test_gpu_zero_coef_skip.py).

One batch of 16 columns on the annulus "small" (8 736 DoF, three levels), every column with its own coefficients: columns 0-7 at a
shift far from the spectrum, 2 pi (500 + 400i), columns 8-15 near it, 2 pi (1000 - 20i); zero guess, tol 1e-10.  The solution is
compared with SuperLU (scipy.sparse.linalg.splu of the assembled operator) at the tolerance tests/test_gpu_parity.py
test_solve_many_systems_in_lockstep uses, 1e-8 of the column's largest entry.  That a chunk really is masked while the other runs is
shown by the step counts: the same right-hand sides solved with all 16 columns at the far shift, and with all 16 at the near one,
give the per-group counts; the far group has to finish at least 4 steps before the near one's fastest column, and the mixed batch has to
report the sum of the two groups' own counts, not lock-step counts.  Step counts are per column with or without the mask, so the mask
itself is pinned by a second run of the mixed batch in a child process with WAE_GMRES_MASK0=0 (the switch is read once per process):
skipping the finished chunk may not move one bit of the solution, nor a count."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse.linalg as spla

from wae_amd.helmholtz.family import annulus_family

pytestmark = pytest.mark.gpu

Z_FAR, Z_NEAR = 2 * np.pi * (500 + 400j), 2 * np.pi * (1000 - 20j)
TOL, MAXIT = 1e-10, 300


def relerr(a, b):
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def mixed_case():
    L, _ = annulus_family("small", tau=2e-4)
    L.solver_ref = 2 * np.pi * 500.0
    fam = L.ensure_solver()
    rng = np.random.default_rng(5)
    B = rng.standard_normal((fam.d, 16)) + 1j * rng.standard_normal((fam.d, 16))
    c_far, c_near = L.coefficients(Z_FAR), L.coefficients(Z_NEAR)
    return L, fam, B, c_far, c_near


CHILD = """
import json, sys
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np
import wae_amd  # noqa: F401
import test_gpu_mask_from_zero as T
L, fam, B, c_far, c_near = T.mixed_case()
X = fam.solve(np.array([c_far] * 8 + [c_near] * 8), B, tol=T.TOL, maxit=T.MAXIT)
np.save({out!r}, np.ascontiguousarray(X))
info = dict(fam.last_info)
info.pop("seconds", None)
print("INFO " + json.dumps(info))
"""


def test_mixed_batch_from_a_zero_guess(tmp_path):
    L, fam, B, c_far, c_near = mixed_case()
    ct = np.array([c_far] * 8 + [c_near] * 8)

    X = fam.solve(ct, B, tol=TOL, maxit=MAXIT)
    mixed = dict(fam.last_info)
    fam.solve(np.array([c_far] * 16), B, tol=TOL, maxit=MAXIT)
    far = dict(fam.last_info)
    fam.solve(np.array([c_near] * 16), B, tol=TOL, maxit=MAXIT)
    near = dict(fam.last_info)
    print(f"mixed {mixed}\nfar   {far}\nnear  {near}")
    L._drop_device()

    assert mixed["n_unconverged"] == 0 and far["n_unconverged"] == 0 and near["n_unconverged"] == 0
    for z, cols in ((Z_FAR, range(0, 8)), (Z_NEAR, range(8, 16))):
        A = sum(c * t.coeff for c, t in zip(L.coefficients(z), L.terms) if c != 0).tocsc()
        lu = spla.splu(A)
        for j in cols:
            e = relerr(X[:, j], lu.solve(B[:, j]))
            assert e < 1e-8, (j, e)
    # the two shifts separate: every far column is done at least 4 steps before the average near column
    assert far["iters_max"] + 4 <= near["iters_total"] / 16, (far, near)
    # ... and in the mixed batch the far group stopped at its own counts while the near group ran on
    assert mixed["iters_max"] >= far["iters_max"] + 4, (mixed, far)
    assert mixed["iters_total"] <= 8 * far["iters_max"] + 8 * mixed["iters_max"], (mixed, far)
    # the same batch without the mask from a zero guess: the same bits, the same counts
    out = str(tmp_path / "x_unmasked.npy")
    env = dict(os.environ, WAE_GMRES_MASK0="0")
    r = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), out=out)], env=env, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    unmasked = json.loads(next(ln for ln in r.stdout.split("\n") if ln.startswith("INFO "))[5:])
    Xu = np.load(out)
    assert np.array_equal(np.ascontiguousarray(X).view(np.uint64), Xu.view(np.uint64)), "the mask from a zero guess moves the solution"
    assert all(mixed[k] == unmasked[k] for k in unmasked), (mixed, unmasked)
