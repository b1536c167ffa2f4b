#!/usr/bin/env python3
"""Wall time and PCIe traffic of a frequency sweep of the forced problem on the annular combustor (preset C2 by default, 199 680 DoF): the outlet
as a :speaker boundary, 4 point probes, --nfreq excitation frequencies between --f0 and --f1 Hz,

  a) through nlevp.forced_response (wae_forced_response): right-hand sides built and observers applied in HBM;
  b) through DeviceFamily.solve with a dense d x nfreq host right-hand side and one coefficient set per column, the probes applied on the
     host to the dense solution that comes back -- the only way before wae_forced_response existed.

Same process, same handle and solver set-up, one warm-up sweep of 2 x batch frequencies through each path, then a, b, a, b.  Both paths end
with their results on the host, so the clock covers the whole call.  Bytes: what each call moves over PCIe, counted from the array sizes.
Prints one JSON object (and writes it to --out).

    python dev/forced_sweep_time.py --out profiles/forced_sweep_C2.json
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import wae_amd  # noqa
from wae_amd.helmholtz.assemble import assemble_p1_source
from wae_amd.helmholtz.family import annulus_family, speaker_source
from wae_amd.helmholtz.probe import probe_p
from wae_amd.nlevp import forced_response
from wae_amd.nlevp.forcing import _coefficient_table

ap = argparse.ArgumentParser()
ap.add_argument("--preset", default="C2")
ap.add_argument("--nfreq", type=int, default=256)
ap.add_argument("--f0", type=float, default=50.0)
ap.add_argument("--f1", type=float, default=600.0)
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--tol", type=float, default=1e-10)
ap.add_argument("--reps", type=int, default=2)
ap.add_argument("--out", default="")
a = ap.parse_args()

L, pb = annulus_family(a.preset, n=0.01)
mesh = pb["info"]["mesh"]
pts, tets = pb["points"], mesh["tets"]
d = pb["d"]
L.solver_ref = 2 * np.pi * 300.0
L.solver_opts = {"batch": a.batch}
L.solver_tol = a.tol
rhs = speaker_source(assemble_p1_source(pts, mesh["outlet_tris"], c_tri=mesh["outlet_c"]), Y=pb["params"]["Y"], A=1.0)
probes = [probe_p(pts, tets, np.array([0.15 * np.cos(t), 0.15 * np.sin(t), z])) for t, z in ((0.1, 0.05), (1.7, 0.2), (3.3, 0.35), (5.0, 0.45))]
W = np.zeros((len(probes), d), dtype=np.complex128)
for q, (idx, val) in enumerate(probes):
    np.add.at(W[q], idx, val)
m = np.asarray(rhs.terms[0].coeff.todense()).ravel()
fam = L.ensure_solver()


def sweep_device(omegas):
    t0 = time.perf_counter()
    res = forced_response(L, rhs, omegas, observers=probes)
    return time.perf_counter() - t0, res.H, res.info


def sweep_host(omegas):
    t0 = time.perf_counter()
    ct, sc = _coefficient_table(L, omegas), _coefficient_table(rhs, omegas)
    B = np.asfortranarray(m[:, None] * sc[:, 0][None, :])
    X = fam.solve(ct, B, tol=a.tol, maxit=L.solver_maxit)
    H = W @ X
    return time.perf_counter() - t0, H, fam.last_info


omegas = 2 * np.pi * np.linspace(a.f0, a.f1, a.nfreq)
warm = omegas[:: max(1, a.nfreq // (2 * a.batch))][: 2 * a.batch]
sweep_device(warm); sweep_host(warm)
times = {"device": [], "host": []}
for rep in range(a.reps):
    for kind, f in (("device", sweep_device), ("host", sweep_host)):
        dt, H, info = f(omegas)
        times[kind].append(dt)
        if kind == "device":
            Hd, info_d = H, info
        else:
            Hh, info_h = H, info
nsrc_nnz, nobs_nnz, T = int(np.count_nonzero(m)), sum(len(i) for i, _ in probes), len(L.terms)
bytes_device = 16 * a.nfreq * (T + 1) + (16 + 4) * (nsrc_nnz + nobs_nnz) + 16 * len(probes) * a.nfreq
bytes_host = 16 * a.nfreq * T + 2 * 16 * d * a.nfreq
res = {"preset": a.preset, "d": d, "nfreq": a.nfreq, "hz": [a.f0, a.f1], "batch": a.batch, "tol": a.tol, "reps": a.reps,
       "seconds_forced_response": times["device"], "seconds_dense_solve": times["host"],
       "pcie_bytes_forced_response": bytes_device, "pcie_bytes_dense_solve": bytes_host,
       "max_abs_H_difference_over_max_abs_H": float(np.max(np.abs(Hd - Hh)) / np.max(np.abs(Hh))), "max_abs_H": float(np.max(np.abs(Hh))),
       "info_forced_response": info_d, "info_dense_solve": info_h}
print(json.dumps(res))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
