#!/usr/bin/env python3
"""Wall time of the Bloch fold of the P2 mass and stiffness matrices at the C4 unit cell (annulus preset C4: grid 20 x 200 x 50, DOS 32;
extended cell 210 000 points): the device route -- bloch_numbering + blochify_device((M, K)) -- against a host scipy fold that uses the
same cell_dof map (COO arrays, one csr_matrix per part), timed in the same run.  M and K come from assemble_p2 on the device (not timed).
No threshold is attached: the case for the device fold is that it exists in the assembly pipeline, not a factor.  Prints one JSON object
(and writes it to --out).

    python dev/bloch_p2_time.py --out profiles/bloch_p2_C4.json
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import scipy.sparse as sp
import wae_amd  # noqa
from wae_amd.helmholtz import annulus
from wae_amd.helmholtz.assemble import assemble_p2
from wae_amd.helmholtz.bloch import bloch_numbering, blochify_device

ap = argparse.ArgumentParser()
ap.add_argument("--grid", default="20,200,50")
ap.add_argument("--dos", type=int, default=32)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--out", default="")
a = ap.parse_args()

nthc, nz, nr = (int(x) for x in a.grid.split(","))
pts, tets, _ = annulus._mesh(nthc, nz, nr, sector_of=a.dos)
tets = tets.astype(np.int32)
c_tet = np.where(pts[tets].mean(axis=1)[:, 2] < annulus.Z_JUMP, annulus.C_COLD, annulus.C_HOT)
nsector = nthc * nz * nr
M, K = assemble_p2(pts, tets, c_tet)


def device():
    nb = bloch_numbering(len(pts), tets, nsector)
    return nb, blochify_device((M, K), nb)


def host(nb):
    cell, image = nb.cell_dof.astype(np.int64), nb.image
    out = []
    for A in (M, K):
        A = A.tocoo()
        i_img, j_img = image[A.row], image[A.col]
        I, J = cell[A.row], cell[A.col]
        parts = []
        for sel in (i_img == j_img, ~i_img & j_img, i_img & ~j_img):
            P = sp.csr_matrix((A.data[sel], (I[sel], J[sel])), shape=(nb.dim, nb.dim))
            P.sum_duplicates()
            P.sort_indices()
            parts.append(P)
        out.append(parts)
    return out


nb, got = device()                                                             # warm-up
t_dev, t_host = [], []
for _ in range(a.reps):
    t0 = time.perf_counter()
    nb, got = device()
    t_dev.append(time.perf_counter() - t0)
for _ in range(a.reps):
    t0 = time.perf_counter()
    ref = host(nb)
    t_host.append(time.perf_counter() - t0)
gap = max(float(np.max(np.abs(g.data - r.data)) / np.max(np.abs(r.data))) for G, R in zip(got, ref) for g, r in zip(G, R) if r.nnz)
same = all(np.array_equal(g.indptr, r.indptr) and np.array_equal(g.indices, r.indices) for G, R in zip(got, ref) for g, r in zip(G, R))
res = {"grid": [nthc, nz, nr], "DOS": a.dos, "extended_points": len(pts), "ntets": len(tets), "nedges": nb.nedges, "nimage_edges": nb.nimage_edges,
       "extended_dofs": nb.ndof, "dim": nb.dim, "nnz_extended": int(M.nnz), "nnz_parts": [int(p.nnz) for p in got[0]],
       "seconds_device_numbering_and_fold": t_dev, "median_device": float(np.median(t_dev)),
       "seconds_host_scipy_fold": t_host, "median_host": float(np.median(t_host)),
       "patterns_equal": bool(same), "max_relative_gap": gap}
print(json.dumps(res))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
