#!/usr/bin/env python3
"""Time of `Locator.sample` for Hermite vectors (order "herm", csrc/locate.hip loc_sample_kernel<20>) beside P2 vectors (order "quad",
loc_sample_kernel<10>) on the same mesh and points: the octosplit Rijke tube (--levels refinements of tests/golden/rijke_mesh.npz), about
10^6 uniform points of its bounding box, 8 columns, kinds "p" and "n_grad_p", the tetrahedra found once and passed in.

The call figures are the times between two HIP events on the null stream around one C-ABI call.  A call moves its arguments and results
over the bus (28 B per point in, 24 more for the directions of n_grad_p, 16 B per point and column out, and the columns of V in), which
is most of it; --kernel-trace takes the kernel_trace CSV of a separate `rocprofv3 --kernel-trace -- python dev/herm_sample_time.py`
run (same --reps) for the kernels alone: its loc_sample_kernel dispatches, in order, are the four timed groups of reps + 1 calls.  The
bytes a kernel asks for per point (not what reaches HBM: the gathers of neighbouring points hit the same lines) are 28 [+ 24] for the point, 16 + 96 for the tetrahedron and its corners, 4 NW for the unknowns,
16 NW ncols for the gathered entries and 16 ncols for the result, NW = 20 or 10.  No threshold is attached: the P2 time of the same run is
the yardstick.  Prints one JSON object (and writes it to --out).

    python dev/herm_sample_time.py --out profiles/herm_sample.json [--kernel-trace CSV]
"""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np
import torch
import wae_amd  # noqa
from wae_amd.helmholtz import Locator, octosplit
from wae_amd.helmholtz.assemble import herm_connectivity, p2_connectivity

ap = argparse.ArgumentParser()
ap.add_argument("--levels", type=int, default=2)
ap.add_argument("--nq", type=int, default=10 ** 6)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--ncols", type=int, default=8)
ap.add_argument("--kernel-trace", default="")
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


def kernel_bytes_per_point(nw, kind):
    return 28 + (24 if kind else 0) + 16 + 96 + 4 * nw + 16 * nw * a.ncols + 16 * a.ncols


z = np.load(os.path.join(ROOT, "tests", "golden", "rijke_mesh.npz"))
Rm = octosplit(z["points"], z["tetrahedra"], z["outlet_triangles"], levels=a.levels)
pts, tets = np.ascontiguousarray(Rm.points[a.levels]), np.ascontiguousarray(Rm.tets[a.levels], dtype=np.int32)
del Rm                                                                  # (frees the levels in HBM now, not at interpreter exit)
t10 = p2_connectivity(pts, tets)[1]
t20, ndof20 = herm_connectivity(pts, tets)[1::2]
ndof10 = int(t10.max()) + 1
res = {"device": torch.cuda.get_device_name(0), "mesh": f"rijke, octosplit level {a.levels}", "npoints": len(pts), "ntets": len(tets),
       "ndof_quad": ndof10, "ndof_herm": int(ndof20), "ncols": a.ncols}
loc = Locator(pts, tets)
rng = np.random.default_rng(0)
lo, hi = pts.min(axis=0), pts.max(axis=0)
X = lo + rng.uniform(0.0, 1.0, (a.nq, 3)) * (hi - lo)
tet = loc.find(X)
X, tet = np.ascontiguousarray(X[tet >= 0]), np.ascontiguousarray(tet[tet >= 0])       # the tube fills part of its box: the located points only
n = np.array([0.3, -0.5, 0.8])
res["nq"] = len(X)
V = {"quad": np.asfortranarray(rng.standard_normal((ndof10, a.ncols)) + 1j * rng.standard_normal((ndof10, a.ncols))),
     "herm": np.asfortranarray(rng.standard_normal((ndof20, a.ncols)) + 1j * rng.standard_normal((ndof20, a.ncols)))}
res["sample"] = {}
for order, nw, kw in (("quad", 10, dict(tets10=t10)), ("herm", 20, dict(tets20=t20))):
    for kind in ("p", "n_grad_p"):
        ev, P = timed(lambda: loc.sample(V[order], X, order, kind, n=n if kind != "p" else None, tet=tet, **kw))
        assert P.shape == (len(X), a.ncols) and np.all(np.isfinite(P.real))
        res["sample"][f"{order}_{kind}"] = {
            "seconds_call_events": ev, "median_call_events": float(np.median(ev)),
            "bus_bytes": (28 + (24 if kind != "p" else 0) + 16 * a.ncols) * len(X) + 16 * a.ncols * V[order].shape[0],
            "kernel_bytes_per_point": kernel_bytes_per_point(nw, kind != "p")}
for kind in ("p", "n_grad_p"):
    res["sample"][f"herm_over_quad_call_{kind}"] = res["sample"][f"herm_{kind}"]["median_call_events"] / res["sample"][f"quad_{kind}"]["median_call_events"]
    res["sample"][f"herm_over_quad_kernel_bytes_{kind}"] = kernel_bytes_per_point(20, kind != "p") / kernel_bytes_per_point(10, kind != "p")
if a.kernel_trace:
    rows = [r for r in csv.DictReader(open(a.kernel_trace)) if "loc_sample_kernel" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    assert len(rows) == 4 * (a.reps + 1), (len(rows), a.reps)
    ks = {}
    for g, label in enumerate(("quad_p", "quad_n_grad_p", "herm_p", "herm_n_grad_p")):
        grp = rows[g * (a.reps + 1):(g + 1) * (a.reps + 1)]
        nw = "20" if label.startswith("herm") else "10"
        assert all(f"<{nw}>" in r["Kernel_Name"] or f"ILi{nw}E" in r["Kernel_Name"] for r in grp), label
        ns = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in grp[1:]]                 # (the first is the warm-up)
        ks[label] = {"kernel_ns": ns, "median_ns": float(np.median(ns)),
                     "requested_bytes_per_second": res["sample"][label]["kernel_bytes_per_point"] * len(X) / (np.median(ns) * 1e-9)}
    for kind in ("p", "n_grad_p"):
        ks[f"herm_over_quad_{kind}"] = ks[f"herm_{kind}"]["median_ns"] / ks[f"quad_{kind}"]["median_ns"]
    res["kernels"] = ks
    res["kernel_source"] = "rocprofv3 --kernel-trace of a separate run of this script with the same seed and sizes"
print(json.dumps(res))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
