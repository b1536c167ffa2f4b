#!/usr/bin/env python3
"""Wall time of the P2 discrete-adjoint shape sensitivity on the Rijke tube (tests/golden/rijke_mesh.npz, all surface points, interior and
admittance parts): the device call, discrete_adjoint_shape_sensitivity(..., order="quad"), against the only route there was before it, a host
loop of 2 x 3 re-discretisations of the whole mesh with assemble_p2 / assemble_p2_boundary per point and -w^H (L+ - L-) u / 2h from the
matrices -- timed for --points points and scaled to all of them.  Same process, one warm-up of each.  Random vectors: the kernel only
contracts.  Prints one JSON object (and writes it to --out).

    python dev/shape_p2_time.py --out profiles/shape_p2.json
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import wae_amd  # noqa
from wae_amd.helmholtz import shape as SH
from wae_amd.helmholtz.assemble import assemble_p2, assemble_p2_boundary, discrete_adjoint_shape_sensitivity, p2_edge_count
from wae_amd.nlevp import Solution

ap = argparse.ArgumentParser()
ap.add_argument("--points", type=int, default=16)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--h", type=float, default=1e-5)
ap.add_argument("--out", default="")
a = ap.parse_args()

z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "rijke_mesh.npz"))
pts, tets, tris, c_tet, c_tri = z["points"], z["tetrahedra"], z["outlet_triangles"], z["c_tet"], z["outlet_c"]
sp = SH.get_surface_points(SH.boundary_triangles(tets)[0], tets)[0]
dim = len(pts) + p2_edge_count(tets)
rng = np.random.default_rng(0)
u, w = (rng.standard_normal(dim) + 1j * rng.standard_normal(dim) for _ in range(2))
om, Y = 1.0e5 + 3.0e3j, 0.7 + 0.1j
sol = Solution({"ω": om}, None, None, "ω")


def device(points):
    return discrete_adjoint_shape_sensitivity(pts, tets, c_tet, points, sol, None, bnd_tris=tris, bnd_c=c_tri, Y=Y, h=a.h, v_ext=(u, w), order="quad")


def host_loop(points):
    out = np.zeros((3, len(points)), dtype=complex)
    for k, p in enumerate(points):
        for crd in range(3):
            L = []
            for d in (a.h, -a.h):
                ph = pts.copy()
                ph[p, crd] += d
                M, K = assemble_p2(ph, tets, c_tet)
                L.append(om ** 2 * M + K + om * Y * assemble_p2_boundary(ph, tets, tris, c_tri))
            out[crd, k] = -np.vdot(w, (L[0] - L[1]) @ u) / (2 * a.h)
    return out


pick = sp[np.linspace(0, len(sp) - 1, a.points).astype(int)]
device(sp); host_loop(pick[:1])                                          # warm-up
t_dev = []
for _ in range(a.reps):
    t0 = time.perf_counter()
    got = device(sp)
    t_dev.append(time.perf_counter() - t0)
t0 = time.perf_counter()
ref = host_loop(pick)
t_host = time.perf_counter() - t0
pos = np.searchsorted(sp, pick)
gap = float(np.max(np.abs(got[:, pos] - ref).max(axis=0) / np.abs(ref).max(axis=0)))
res = {"mesh": "rijke_mesh.npz", "npoints": len(pts), "ntets": len(tets), "dim": dim, "surface_points": len(sp), "h": a.h,
       "seconds_device_all_points": t_dev, "median_device_all_points": float(np.median(t_dev)),
       "host_loop_points": len(pick), "seconds_host_loop": t_host, "host_loop_scaled_to_all_points": t_host / len(pick) * len(sp),
       "ratio": t_host / len(pick) * len(sp) / float(np.median(t_dev)), "max_relative_gap_on_the_timed_points": gap}
print(json.dumps(res))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
