#!/usr/bin/env python3
"""Time of the point locator on the device (wae_locator_*) on the C3 annulus mesh (annulus._mesh at the benchmark grid, 995 328 points,
5.7 M tetrahedra): the build, `find` for 10^4 and 10^6 random points of the bounding box, `sample` of 8 columns at those points, beside
`probe.find_tetrahedron` (one host pass over all tetrahedra per point) timed on 16 of the same points and scaled.

The device figures are the times between two HIP events on the null stream around one C-ABI call.  A call moves its arguments and results
over the bus (find: 24 B per point in, 4 B out; sample: 28 B per point in, 16 B per point and column out, and the 8 columns of V in), so
the call time is given with those bytes; --kernel-stats takes the kernel_stats CSV of a separate `rocprofv3 --kernel-trace --stats --
python dev/locate_time.py` run for the kernels alone.  No threshold is attached.  Prints one JSON object (and writes it to --out).

    python dev/locate_time.py --out profiles/locate_C3.json [--kernel-stats CSV]
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
import numpy as np
import torch
import wae_amd  # noqa
from wae_amd import _lib
from wae_amd.helmholtz import Locator, annulus, probe

ap = argparse.ArgumentParser()
ap.add_argument("--preset", default="C3")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--ncols", type=int, default=8)
ap.add_argument("--host-points", type=int, default=16)
ap.add_argument("--kernel-stats", default="")
ap.add_argument("--out", default="")
a = ap.parse_args()

assert torch.cuda.is_available(), "this measurement needs the GPU"
torch.cuda.init()


def timed(call, reps=a.reps):
    """(event seconds of every repetition after a warm-up, the last result)"""
    ev, out = [], None
    for rep in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        out = call()
        e1.record()
        torch.cuda.synchronize()
        if rep:
            ev.append(e0.elapsed_time(e1) * 1e-3)
    return ev, out


pts, tets, _ = annulus._mesh(*annulus.PRESETS[a.preset])
tets = np.ascontiguousarray(tets, dtype=np.int32)
res = {"device": torch.cuda.get_device_name(0), "mesh": f"annulus {a.preset}", "npoints": len(pts), "ntets": len(tets)}
ev, loc = timed(lambda: Locator(pts, tets))
res["build"] = {"seconds_call_events": ev, "median_call_events": float(np.median(ev)), "dims": list(loc.dims), "nrefs": loc.nrefs,
                "refs_per_tet": loc.nrefs / len(tets), "max_per_cell": loc.max_per_cell,
                "mean_per_cell": loc.nrefs / float(np.prod(loc.dims)), "bus_bytes": 24 * len(pts) + 16 * len(tets)}
rng = np.random.default_rng(0)
lo, hi = pts.min(axis=0), pts.max(axis=0)
V = np.asfortranarray(rng.standard_normal((len(pts), a.ncols)) + 1j * rng.standard_normal((len(pts), a.ncols)))
res["queries"] = []
for nq in (10 ** 4, 10 ** 6):
    X = lo + rng.uniform(0.0, 1.0, (nq, 3)) * (hi - lo)
    ev_f, tet = timed(lambda: loc.find(X))
    ev_s, P = timed(lambda: loc.sample(V, X, tet=tet, outside="nan"))
    inside = tet >= 0
    assert np.array_equal(np.isnan(P[:, 0].real), ~inside)
    # the answers of the first host points: the host pass takes the tetrahedron with the largest smallest coordinate, the device the
    # first that holds the point; both hold it
    k = a.host_points
    if not res["queries"]:                                                  # (timed once: the cost of a point does not depend on nq)
        t0 = time.perf_counter()
        host = []
        for x in X[:k]:
            try:
                host.append(probe.find_tetrahedron(pts, tets, x, tol=0.0))
            except ValueError:
                host.append(-1)
        t_host = (time.perf_counter() - t0) / k
        agree = int(np.sum((np.array(host) >= 0) == inside[:k]))
    tf, ts = float(np.median(ev_f)), float(np.median(ev_s))
    res["queries"].append({
        "nq": nq, "inside_fraction": float(inside.mean()),
        "find_seconds_call_events": ev_f, "find_median": tf, "find_points_per_second": nq / tf, "find_bus_bytes": 28 * nq,
        "sample_ncols": a.ncols, "sample_seconds_call_events": ev_s, "sample_median": ts, "sample_bus_bytes": 28 * nq + 16 * a.ncols * (nq + len(pts)),
        "host_find_tetrahedron_seconds_per_point": t_host, "host_points_timed": k, "host_seconds_scaled_to_nq": t_host * nq,
        "host_over_device_find": t_host * nq / tf, "host_and_device_agree_on_inside": f"{agree} of {k}"})
if a.kernel_stats:
    rows = list(csv.DictReader(open(a.kernel_stats)))
    ks = {}
    for key in ("loc_find_kernel", "loc_sample_kernel", "loc_fill_kernel", "loc_count_kernel", "loc_ptr_kernel", "loc_box_kernel"):
        for r in rows:
            if key + "(" in r["Name"] or key + "<" in r["Name"]:
                ks[key] = {"calls": int(r["Calls"]), "average_ns": float(r["AverageNs"]), "min_ns": float(r["MinNs"]), "max_ns": float(r["MaxNs"])}
    res["kernels"] = ks
    res["kernel_source"] = "rocprofv3 --kernel-trace --stats of a separate run of this script (the figures mix the 10^4 and the 10^6 calls: max_ns is a 10^6 one)"
print(json.dumps(res))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
