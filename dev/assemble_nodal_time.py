#!/usr/bin/env python3
"""Wall time of the P2 interior assembly with a nodal speed of sound, assemble_p2(..., c_point=...), against the per-tetrahedron form,
assemble_p2(..., c_tet=...), on the Kuhn triangulation of the unit cube with n^3 cells (n = 48: 663 552 tetrahedra).  Same process, one
warm-up call of each, then alternating a/b/a/b; every call ends with the matrices on the host, so the clock covers the whole entry
(upload, edge numbering, element kernel, sort, reduce, download).  Prints one JSON object (and writes it to --out).

    python dev/assemble_nodal_time.py --out profiles/assemble_nodal_kuhn48.json
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import wae_amd  # noqa
from wae_amd.helmholtz.assemble import assemble_p2

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=48)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--out", default="")
a = ap.parse_args()


def kuhn_cube(n):
    """points ((n+1)^3, 3) and tetrahedra (6 n^3, 4): per cell one tetrahedron for every order of the axes"""
    g = np.arange(n + 1) / n
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    ijk = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    stride = np.array([(n + 1) ** 2, n + 1, 1])
    tets = []
    for perm in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
        p = ijk.copy()
        cols = [p @ stride]
        for ax in perm:
            p[:, ax] += 1
            cols.append(p @ stride)
        tets.append(np.stack(cols, axis=1))
    return pts, np.concatenate(tets).astype(np.int32)


pts, tets = kuhn_cube(a.n)
c_point = 1.0 + pts[:, 0]
c_tet = c_point[tets].mean(axis=1)
times = {"c_tet": [], "c_point": []}
for rep in range(a.reps + 1):                                           # rep 0: warm-up
    for kind, kw in (("c_tet", {"c_tet": c_tet}), ("c_point", {"c_point": c_point})):
        t0 = time.perf_counter()
        M, K = assemble_p2(pts, tets, dtype=np.float64, **kw)
        dt = time.perf_counter() - t0
        if rep:
            times[kind].append(dt)
res = {"mesh": f"kuhn_cube({a.n})", "npoints": len(pts), "ntets": len(tets), "dim": M.shape[0], "nnz": int(M.nnz), "reps": a.reps,
       "seconds_c_tet": times["c_tet"], "seconds_c_point": times["c_point"],
       "median_c_tet": float(np.median(times["c_tet"])), "median_c_point": float(np.median(times["c_point"]))}
print(json.dumps(res))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
