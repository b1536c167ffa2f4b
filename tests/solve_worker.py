"""Child process of tests/test_gpu_solve_driver.py::test_variants: the switches of the solve drivers (WAE_GMRES_DEVICE, WAE_GMRES_PAIR,
WAE_GMRES_SYNC, WAE_NARROW_PAIR) are read once per process, so every variant gets a process of its own, with the switch in its
environment.  Runs the truncated table for r = 16 and r = 8 on the handle batch 16 / restart 6 and the converged solve of 64 columns
on the handle batch 64, prints a summary line per solve and leaves X (.npy) and info (.json) in the directory given.

usage: solve_worker.py DIR   (DIR holds B16.npy, ct16.npy, ct1.npy, written by the parent)"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

import _solveref as S  # noqa: E402
from _hier import OPS, family_a_operator  # noqa: E402


def main(out):
    B16, ct16, ct1 = (np.load(os.path.join(out, f"{n}.npy")) for n in ("B16", "ct16", "ct1"))
    done = {}

    def solve(fam, name, r, percol, tol, maxit):
        B, ct = S.columns(B16, ct16, ct1, r, percol)
        X = fam.solve(ct, B, op=OPS["N"], tol=tol, maxit=maxit, strict=False, quiet=True)
        info = dict(fam.last_info, code=int(fam.last_code))
        np.save(os.path.join(out, name + ".npy"), X)
        done[name] = info
        print(f"{name}: sum|X| {np.abs(X).sum():.15e} max|X| {np.abs(X).max():.6e} info {info}", flush=True)

    L = family_a_operator(1, batch=S.NB_SMALL, restart=S.RESTART_SMALL)
    fam = L.ensure_solver()
    for r in (16, 8):
        for k in S.ks_for(r):
            for percol in (False, True):
                solve(fam, f"trunc_r{r}_k{k}_p{int(percol)}", r, percol, 1e-300, k)
    L._drop_device()
    L = family_a_operator(1, batch=S.NB_WIDE)
    solve(L.ensure_solver(), "conv_r64", 64, True, S.TOL, S.MAXIT)
    L._drop_device()
    with open(os.path.join(out, "info.json"), "w") as f:
        json.dump(done, f)


if __name__ == "__main__":
    main(sys.argv[1])
