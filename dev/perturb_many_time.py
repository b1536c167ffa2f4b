#!/usr/bin/env python3
"""C5 (500k-DoF annulus): the eigenpairs of 8 start values, each expanded to order N in tau -- (a) one perturb_fast_ call per pair, one
after the other (the single-pair path, wae_perturb), against (b) ONE perturb_many (wae_perturb_batch).  Same process, both warmed up,
alternating a/b/a/b, each timed run ending in a device synchronise.  Prints one JSON object (and writes it to --out).

    python dev/perturb_many_time.py --out profiles/perturb_many_C5.json
    WAE_PERTURB_PAD=0 python dev/perturb_many_time.py --nsys 4 --order 10 --reps 2      # the padding decision for narrow batches
    python dev/perturb_many_time.py --only-batch --reps 1                                # under rocprofv3 --kernel-trace --stats
"""
import argparse
import json
import os
import re
import sys
import tempfile
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
os.environ.setdefault("WAE_PERTURB_DEBUG", "1")          # the per-order lock-step iteration counts (one stderr line per batch call)
import numpy as np
import torch
import wae_amd  # noqa
from wae_amd.helmholtz.family import annulus_family
from wae_amd.nlevp import householder_many, perturb_fast_, perturb_many

ap = argparse.ArgumentParser()
ap.add_argument("--preset", default="C5")
ap.add_argument("--nsys", type=int, default=8)
ap.add_argument("--order", type=int, default=30)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--only-batch", action="store_true")
ap.add_argument("--out", default="")
a = ap.parse_args()

# the modes of the annulus inside the benchmark contour (BENCH: eigenvalues_hz of the C3 pass), as start values
STARTS_HZ = [195.42 + 8.89j, 735.18 + 3.23j, 428.64 + 9.45j, 774.18 + 9.94j, 843.81 + 13.50j, 428.65 + 9.47j, 774.20 + 9.98j, 843.82 + 13.54j]
tau0 = 2e-4
t0 = time.time()
L, pb = annulus_family(a.preset, tau=tau0)
L.solver_tol = 1e-12
L.solver_ref = 2 * np.pi * 500.0
L.solver_opts = {"batch": 16, "restart": 40, "sweeps": 1}
fam = L.ensure_solver()
starts = [2 * np.pi * z for z in STARTS_HZ[:a.nsys]]
sols = [s for s, _, _ in householder_many(L, starts, maxiter=12, tol=1e-11)]
print("built, set up, %d eigenpairs refined: %.1f s" % (len(sols), time.time() - t0), [complex(np.round(s.params["ω"] / 2 / np.pi, 3)) for s in sols],
      file=sys.stderr, flush=True)
N = a.order


def sync():
    torch.cuda.synchronize()


def run_a():
    sync(); t = time.perf_counter()
    its = 0
    for s in sols:
        perturb_fast_(s, L, "τ", N)
        its += fam.last_info["iters_total"]
    sync()
    return time.perf_counter() - t, its


def run_b():
    sync(); t = time.perf_counter()
    st = perturb_many(sols, L, "τ", N, kind="fast")
    sync()
    return time.perf_counter() - t, dict(fam.last_info), [int(x) for x in st]


def captured_stderr(fn):
    """fn() with the process's stderr (the library's debug line) captured"""
    sys.stderr.flush()
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        saved = os.dup(2)
        os.dup2(tmp.fileno(), 2)
        try:
            out = fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        return out, tmp.read().decode(errors="replace")


res = {"preset": a.preset, "d": int(pb["d"]), "nsys": len(sols), "order": N, "pad_env": os.environ.get("WAE_PERTURB_PAD", "(default 0)"),
       "eigenvalues_hz": [[float(np.real(s.params["ω"]) / 2 / np.pi), float(np.imag(s.params["ω"]) / 2 / np.pi)] for s in sols]}
if not a.only_batch:
    lam_a = []
    run_a()                                               # warm-up of both
    lam_a = [np.array(s.eigval_pert["τ/Taylor"]) for s in sols]
    run_b()
    lam_b = [np.array(s.eigval_pert["τ/Taylor"]) for s in sols]
    res["max_rel_diff_lambda_1_to_10_batch_vs_single"] = float(max(np.max(np.abs(x[1:11] - y[1:11]) / np.abs(x[1:11])) for x, y in zip(lam_a, lam_b)))
    ta, tb = [], []
    for _ in range(a.reps):
        t, its_a = run_a(); ta.append(t)
        t, info_b, st_b = run_b(); tb.append(t)
    res.update({"a_seconds": ta, "b_seconds": tb, "a_median": float(np.median(ta)), "b_median": float(np.median(tb)),
                "a_spread": float(max(ta) - min(ta)), "b_spread": float(max(tb) - min(tb)),
                "speedup_median": float(np.median(ta) / np.median(tb)), "a_column_iterations": int(its_a), "b_info": info_b, "b_status": st_b,
                "a": "%d successive perturb_fast_ calls (wae_perturb, one pair each)" % len(sols), "b": "one perturb_many (wae_perturb_batch)"})
(out, err) = captured_stderr(run_b)
m = re.search(r"\[perturb_batch\] nsys=(\d+) nb=(\d+) N=(\d+) lock-step iterations per order:([ 0-9]*)", err)
if m:
    res["batch_columns"] = int(m.group(2))
    res["lockstep_iterations_per_order"] = [int(x) for x in m.group(4).split()]
res["b_seconds_last"] = out[0]
line = json.dumps(res)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
