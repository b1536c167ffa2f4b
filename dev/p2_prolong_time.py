#!/usr/bin/env python3
"""The P2 prolongation and the two nested hierarchies of a P2 family on the tutorial Rijke tube refined once.

The tube's mesh (tests/golden) is refined once on the device (wae_octosplit); M, K, C and Q are assembled with the P2 entries on level 1
from the carried fields (about 45k unknowns).  Recorded:
  - the seconds of one ``prolong(order="quad")`` of 8 complex columns 0 -> 1 (wae_octosplit_prolong_p2: host to host, the copies
    included): the first call, which numbers the edges and builds the step in HBM, and the median of --reps later calls;
  - for three set-ups of the same family in one process -- default (smoothed aggregation, wae_solver_setup), the h-hierarchy
    (``prolongators(order="quad")``: the P2 space of level 0, then aggregation) and the p-hierarchy (``p_first=True``: the P1 space of
    level 1, the P1 space of level 0, then aggregation) -- the set-up seconds (wall, the call alone, median of --reps), the levels, and
    iters_total / iters_max of a solve of 8 columns at tol 1e-10 at the shift 500 + 20i Hz of tests/test_gpu_nested_mg.py.
    Each set-up twice: with the library's Jacobi weights (0.8 / 0.9 / 0.5), and with 0.6 for all three -- damped Jacobi contracts only
    below 2 / lambda_max(D^-1 A), which for P2 operators lies under 0.9.
No threshold is attached.  Prints one JSON object (and writes it to --out).

    python dev/p2_prolong_time.py --out profiles/p2_prolong.json
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np
import torch
import wae_amd  # noqa
from wae_amd.helmholtz import octosplit
from wae_amd.helmholtz.assemble import assemble_p2, assemble_p2_boundary, assemble_p2_flame
from wae_amd.helmholtz.family import helmholtz_family

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default="")
a = ap.parse_args()
assert torch.cuda.is_available(), "this measurement needs the GPU"

GOLDEN = os.path.join(ROOT, "tests", "golden")
Z = 2 * np.pi * (500 + 20j)

z = np.load(os.path.join(GOLDEN, "rijke_mesh.npz"))
fl = np.load(os.path.join(GOLDEN, "rijke_flame.npz"))
R = octosplit(z["points"], z["tetrahedra"], z["outlet_triangles"], levels=1)
pts, tets, tris = R.points[1], R.tets[1], R.tris[1]
M, K = assemble_p2(pts, tets, R.tet_field(z["c_tet"], 1))
Cm = assemble_p2_boundary(pts, tets, tris, R.tri_field(z["outlet_c"], 1))
Q, _ = assemble_p2_flame(pts, tets, R.tet_domain(fl["flame_tets"], 1), R.reference_tet(int(fl["ref_tet"]), fl["x_ref"], 1), fl["x_ref"], fl["n_ref"],
                         float(fl["nglobal_scaled"]))
L = helmholtz_family({"M": M, "K": K, "C": Cm, "Q": Q}, n=0.01, tau=0.001)
L.solver_ref = 340 * 2 * np.pi

rng = np.random.default_rng(1)
res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "unknowns": [R.ndof(0, "quad"), R.ndof(1, "quad")],
       "points": [len(p) for p in R.points], "entries_per_row_fine": float(M.nnz / M.shape[0])}

# ---- the prolongation: a fresh handle, so that the first call pays for the cache
R2 = octosplit(z["points"], z["tetrahedra"], z["outlet_triangles"], levels=1)
X = rng.standard_normal((res["unknowns"][0], 8)) + 1j * rng.standard_normal((res["unknowns"][0], 8))
times = []
for rep in range(a.reps + 1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    Y = R2.prolong(X, 0, 1, order="quad")
    times.append(time.perf_counter() - t0)
P = R2.prolongator(0, order="quad")
res["prolong_8_columns"] = {"first_call_seconds": times[0], "later_calls_seconds": times[1:], "median_later_seconds": float(np.median(times[1:])),
                            "prolongator_nnz": int(P.nnz), "max_error_against_scipy": float(np.max(np.abs(Y - P @ X)))}
del R2

# ---- the three set-ups
B = rng.standard_normal((L.size(), 8)) + 1j * rng.standard_normal((L.size(), 8))
SETUPS = [("default", "smoothed aggregation (wae_solver_setup)", None),
          ("h", "nested, prolongators(order='quad'): P2 of level 0, then aggregation", R.prolongators(order="quad")),
          ("p_first", "nested, prolongators(order='quad', p_first=True): P1 of level 1, P1 of level 0, then aggregation",
           R.prolongators(order="quad", p_first=True))]
WEIGHTS = [("library_weights", {}), ("weights_0.6", {"jacobi_weight": 0.6, "jacobi_weight_post": 0.6, "jacobi_weight_light": 0.6})]
for wkey, opts in WEIGHTS:
    res[wkey] = {"solver_opts": opts}
    for key, what, Ps in SETUPS:
        L.solver_prolongators = Ps
        L.solver_opts = dict(opts)
        setup, solves = [], []
        for rep in range(a.reps):
            L._drop_device()
            fam = L.device()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            L.ensure_solver()
            torch.cuda.synchronize()
            setup.append(time.perf_counter() - t0)
            fam.solve(L.coefficients(Z), B, tol=1e-10, maxit=300, strict=False, quiet=True)
            solves.append(dict(fam.last_info, code=fam.last_code))
        sizes = sorted((lv, ni, no) for w, lv, ni, no in fam.level_sizes() if w == 1)
        res[wkey][key] = {"setup": what, "supplied_levels": [] if Ps is None else [int(P.shape[1]) for P in Ps],
                          "setup_seconds": setup, "median_setup_seconds": float(np.median(setup)), "levels": solves[-1]["levels"],
                          "level_unknowns": [int(sizes[0][1])] + [int(no) for _, _, no in sizes], "iters_total": solves[-1]["iters_total"],
                          "iters_max": solves[-1]["iters_max"], "n_unconverged": solves[-1]["n_unconverged"], "code": solves[-1]["code"],
                          "relres_max": solves[-1]["relres_max"], "solve_seconds": [s["seconds"] for s in solves],
                          "median_solve_seconds": float(np.median([s["seconds"] for s in solves])),
                          "iters_total_all_reps": [s["iters_total"] for s in solves]}
        L._drop_device()
del R
print(json.dumps(res), flush=True)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
