#!/usr/bin/env python3
"""Smoothed aggregation against the nested set-up (wae_solver_setup_nested) on a refined annulus: the same family, set up both ways in
one process, smoothed aggregation first.

The annulus mesh of helmholtz/annulus.py is refined once on the device (wae_octosplit); M, K, C and the flames' Q are assembled on the
device from the carried fields; the nested set-up takes the one prolongator of that refinement, so its level 1 is the unrefined mesh and
smoothed aggregation continues from there.  Recorded for each set-up, as the median of --reps runs: set-up seconds (wall, the call alone),
level sizes and stored entries per row of every sparse level (term 0), iterations per solve of 8 columns at tol 1e-10 over one fixed list
of shifts, and the seconds of one Beyn pass (contour 150..1000 Hz x +-150 Hz, N points per edge, l probe columns, automatic snapshots).
No threshold is attached.  Prints one JSON object per mesh (and writes the list to --out).

    python dev/nested_mg_time.py --out profiles/nested_mg.json [--grids 80,40,8 144,64,14]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np
import scipy.sparse as sp
import torch
import wae_amd  # noqa
from wae_amd.helmholtz import annulus, octosplit
from wae_amd.helmholtz.assemble import assemble_p1, assemble_p1_boundary, assemble_p1_flame
from wae_amd.helmholtz.family import helmholtz_family
from wae_amd.nlevp import compute_moment_matrices

ap = argparse.ArgumentParser()
ap.add_argument("--grids", nargs="+", default=["80,40,8"], help="nth,nz,nr of the UNREFINED annulus: 80,40,8 refines to ~190k points, 144,64,14 to ~1M")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--N", type=int, default=16)
ap.add_argument("--l", type=int, default=8)
ap.add_argument("--out", default="")
a = ap.parse_args()
assert torch.cuda.is_available(), "this measurement needs the GPU"

SHIFTS_HZ = [272 + 10j, 450 + 15j, 640 - 20j, 900 + 10j]
GAMMA = np.array([150 - 150j, 1000 - 150j, 1000 + 150j, 150 + 150j]) * 2 * np.pi


def refined_family(grid):
    """the family on the once-refined mesh, assembled on the device, and the refinement"""
    pb = annulus.build(grid=grid, tau=2e-4)
    m = pb["info"]["mesh"]
    R = octosplit(pb["points"], m["tets"], m["outlet_tris"], levels=1)
    pts, tets, tris = R.points[1], R.tets[1], R.tris[1]
    M, K = assemble_p1(pts, tets, R.tet_field(m["c_tet"], 1))
    Cm = assemble_p1_boundary(pts, tris, R.tri_field(m["outlet_c"], 1))
    Q = None
    for f in m["flames"]:
        Qf, _ = assemble_p1_flame(pts, tets, R.tet_domain(f["flame_tets"], 1), R.reference_tet(f["ref_tet"], f["x_ref"], 1), f["n_ref"],
                                  f["nglobal_scaled"])
        Q = Qf if Q is None else Q + Qf
    p = pb["params"]
    L = helmholtz_family({"M": M, "K": K, "C": Cm, "Q": sp.csr_matrix(Q)}, Y=p["Y"], n=p["n"], tau=p["τ"])
    L.solver_ref = 2 * np.pi * 500.0
    L.solver_tol = 1e-10
    return L, R


def levels_of(L):
    """[(unknowns, stored entries per row of the first plane)] of the coarse levels, from the [setup] lines of one more, untimed set-up
    with WAE_SETUP_DEBUG (the library prints every level's size and entries per plane to stderr)"""
    import re
    import tempfile
    L._drop_device()
    L.device()
    sys.stderr.flush()
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        saved = os.dup(2)
        os.dup2(tmp.fileno(), 2)
        os.environ["WAE_SETUP_DEBUG"] = "1"
        try:
            L.ensure_solver()
        finally:
            del os.environ["WAE_SETUP_DEBUG"]
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        text = tmp.read().decode(errors="replace")
    out = []
    for m in re.finditer(r"\[setup\] level (\d+)[^:]*: n=(\d+) P nnz=(\d+) nnz/plane: (\d+)", text):
        lv, n, pnnz, nnz = (int(x) for x in m.groups())
        if lv >= 1:
            out.append({"level": lv, "unknowns": n, "entries_per_row": nnz / n, "P_nnz": pnnz})
    return out


def measure(L, what):
    rng = np.random.default_rng(1)
    d = L.size()
    B = rng.standard_normal((d, 8)) + 1j * rng.standard_normal((d, 8))
    setup, iters, passes, lv = [], [], [], None
    for rep in range(a.reps):
        L._drop_device()
        fam = L.device()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        L.ensure_solver()
        torch.cuda.synchronize()
        setup.append(time.perf_counter() - t0)
        it = []
        for hz in SHIFTS_HZ:
            fam.solve(L.coefficients(2 * np.pi * hz), B, tol=1e-10, maxit=300, strict=False, quiet=True)
            it.append({"hz": [hz.real, hz.imag], "iters_max": fam.last_info["iters_max"], "n_unconverged": fam.last_info["n_unconverged"],
                       "relres_max": fam.last_info["relres_max"]})
        iters.append(it)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        compute_moment_matrices(L, GAMMA, l=a.l, K=1, N=a.N)
        torch.cuda.synchronize()
        passes.append(time.perf_counter() - t0)
    lv = levels_of(L)
    L._drop_device()
    return {"setup": what, "setup_seconds": setup, "median_setup_seconds": float(np.median(setup)), "levels": lv, "solves": iters[-1],
            "iters_max_per_shift_all_reps": [[s["iters_max"] for s in it] for it in iters],
            "beyn_pass_seconds": passes, "median_beyn_pass_seconds": float(np.median(passes))}


results = []
for g in a.grids:
    grid = tuple(int(x) for x in g.split(","))
    L, R = refined_family(grid)
    P = R.prolongators()
    res = {"device": torch.cuda.get_device_name(0), "grid_unrefined": list(grid), "points": [len(p) for p in R.points], "unknowns": L.size(),
           "reps": a.reps, "beyn": {"N": a.N, "l": a.l}, "entries_per_row_fine": float(sp.csr_matrix(L.terms[1].coeff).nnz / L.size()),
           "entries_per_row_unrefined_mesh": float((P[0].T @ sp.csr_matrix(abs(L.terms[1].coeff)) @ P[0]).nnz / P[0].shape[1])}
    L.solver_prolongators = None
    res["aggregation"] = measure(L, "smoothed aggregation (wae_solver_setup)")
    L.solver_prolongators = P
    res["nested"] = measure(L, "nested (wae_solver_setup_nested), one supplied level")
    print(json.dumps(res), flush=True)
    results.append(res)
    del L, R, P
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(results, f, indent=1)
