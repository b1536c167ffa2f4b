#!/usr/bin/env python3
"""Time of the uniform mesh refinement on the device (wae_octosplit) for 1 to 4 levels of the tutorial Rijke tube (tests/golden/
rijke_mesh.npz) and one level of the C2 annulus mesh, each beside the numpy restatement of tests/_octoref.py timed in the same run, and of
a 64-column prolongation onto the last level of the 4-level Rijke hierarchy.

The device figure is the time between two HIP events on the null stream around one wae_octosplit call: upload of the mesh, every level,
the count and flag read-backs; the copies of the levels back to the host (wae_octosplit_get) are not in it.  The prolongation call moves
its multivectors over the bus, which dominates it: the call's event time is given with the bytes that cross the bus, and --kernel-stats takes
the kernel_stats CSV of a separate `rocprofv3 --kernel-trace --stats -- python dev/octosplit_time.py --prolong-only` run for the kernel alone.
No threshold is attached.  Prints one JSON object (and writes it to --out).

    python dev/octosplit_time.py --out profiles/octosplit.json [--kernel-stats CSV]
"""
import argparse
import csv
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import wae_amd  # noqa
from wae_amd import _lib
from wae_amd.helmholtz import annulus, octosplit
import _octoref

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--max-levels", type=int, default=4)
ap.add_argument("--ncols", type=int, default=64)
ap.add_argument("--prolong-only", action="store_true")
ap.add_argument("--kernel-stats", default="")
ap.add_argument("--out", default="")
a = ap.parse_args()

assert torch.cuda.is_available(), "this measurement needs the GPU"
torch.cuda.init()
L = _lib.lib()
dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)


def device_call(pts, tets, tris, levels):
    """(event seconds, wall seconds, counts of the last level) of one wae_octosplit call"""
    pts, tets = np.ascontiguousarray(pts, dtype=np.float64), np.ascontiguousarray(tets, dtype=np.int32)
    tris = None if tris is None or not len(tris) else np.ascontiguousarray(tris, dtype=np.int32)
    h = C.c_void_p()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    _lib.check(L.wae_octosplit(0, len(pts), pts.ctypes.data_as(dp), len(tets), tets.ctypes.data_as(ip), 0 if tris is None else len(tris),
                               None if tris is None else tris.ctypes.data_as(ip), levels, C.byref(h)))
    e1.record()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    n, nt, ns = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    _lib.check(L.wae_octosplit_info(h, levels, C.byref(n), C.byref(nt), C.byref(ns)))
    L.wae_octosplit_free(h)
    return e0.elapsed_time(e1) * 1e-3, wall, (n.value, nt.value, ns.value)


def case(name, pts, tets, tris, levels):
    device_call(pts, tets, tris, levels)                                           # warm-up
    ev, wall = [], []
    for _ in range(a.reps):
        e, w, counts = device_call(pts, tets, tris, levels)
        ev.append(e); wall.append(w)
    t0 = time.perf_counter()
    H = _octoref.refine(pts, tets, tris, levels)
    t_np = time.perf_counter() - t0
    assert (len(H[-1].points), len(H[-1].tets), len(H[-1].tris)) == counts
    del H
    return {"mesh": name, "levels": levels, "input": [len(pts), len(tets), 0 if tris is None else len(tris)], "last_level": list(counts),
            "seconds_device_events": ev, "median_device_events": float(np.median(ev)), "median_device_wall": float(np.median(wall)),
            "seconds_numpy_reference": t_np}


def prolongation(pts, tets, tris, levels):
    R = octosplit(pts, tets, tris, levels=levels)
    nold, nnew = len(R.points[-2]), len(R.points[-1])
    rng = np.random.default_rng(0)
    X = np.asfortranarray(rng.standard_normal((nold, a.ncols)) + 1j * rng.standard_normal((nold, a.ncols)))
    Y = np.zeros((nnew, a.ncols), dtype=np.complex128, order="F")
    xp, yp = X.ctypes.data_as(dp), Y.ctypes.data_as(dp)
    ev = []
    for rep in range(a.reps + 1):                                                   # the first is the warm-up
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        _lib.check(L.wae_octosplit_prolong(R._h, levels - 1, levels, a.ncols, xp, yp))
        e1.record()
        torch.cuda.synchronize()
        if rep:
            ev.append(e0.elapsed_time(e1) * 1e-3)
    par = R.parents[-1]
    ends = [0, a.ncols - 1]                                                         # two columns: the check is not the measurement
    assert np.array_equal(Y[nold:, ends], (X[par[:, 0]][:, ends] + X[par[:, 1]][:, ends]) * 0.5) and np.array_equal(Y[:nold], X)
    # what the kernel has to move: every row of the old level read once, every row of the new level written, one parent pair per new point.
    # It ASKS for more -- a new point reads two old rows, and an old row is the end of many edges -- and the caches serve those repeats.
    kernel_bytes = 16 * a.ncols * (nold + nnew) + 8 * (nnew - nold)
    kernel_requested_bytes = 16 * a.ncols * (nold + 2 * (nnew - nold) + nnew) + 8 * (nnew - nold)
    bus_bytes = 16 * a.ncols * (nold + nnew)
    t = float(np.median(ev))
    return {"mesh": "rijke", "from_level": levels - 1, "to_level": levels, "ncols": a.ncols, "points_from": nold, "points_to": nnew,
            "seconds_call_events": ev, "median_call_events": t, "kernel_bytes": kernel_bytes, "kernel_requested_bytes": kernel_requested_bytes,
            "bus_bytes": bus_bytes, "bus_bytes_per_second_of_the_call": bus_bytes / t}


z = np.load(os.path.join(ROOT, "tests", "golden", "rijke_mesh.npz"))
rij = (z["points"], z["tetrahedra"], z["outlet_triangles"])
res = {"device": torch.cuda.get_device_name(0)}
if not a.prolong_only:
    res["refinement"] = [case("rijke", *rij, levels) for levels in range(1, a.max_levels + 1)]
    apts, atets, _ = annulus._mesh(*annulus.PRESETS["C2"])
    res["refinement"].append(case("annulus C2", apts, atets.astype(np.int32), None, 1))
res["prolongation"] = prolongation(*rij, a.max_levels)
if a.kernel_stats:
    r = next(r for r in csv.DictReader(open(a.kernel_stats)) if "octo_prolong_kernel" in r["Name"])
    p = res["prolongation"]
    p["kernel_average_ns"], p["kernel_min_ns"], p["kernel_calls"] = float(r["AverageNs"]), float(r["MinNs"]), int(r["Calls"])
    p["kernel_bytes_per_second"] = p["kernel_bytes"] / (p["kernel_average_ns"] * 1e-9)
    p["kernel_source"] = "rocprofv3 --kernel-trace --stats of a separate --prolong-only run"
print(json.dumps(res))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
