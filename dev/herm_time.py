#!/usr/bin/env python3
"""Wall time of the Hermite entries -- herm_connectivity, assemble_herm, assemble_herm_boundary, assemble_herm_flame -- on the Rijke mesh of
tests/golden and on the Kuhn triangulation of the unit cube with n^3 cells (n = 26: 105 456 tetrahedra).  Same process, one warm-up call of
each, then `reps` timed calls; every call ends with its result on the host, so the host clock covers the whole entry (upload, face
numbering, element kernels, sort, reduce, download) and ends behind a device synchronise.  Beside the times: the bytes the triplet sort of
the interior assembly has to move at least once, 400 keys and 800 values of 8 bytes per tetrahedron, and that traffic over the entry's time
as a fraction of the device triad rate (wae_bench_triad, the figure bench.py reports) -- an end-to-end rate, not a kernel's share of peak.

    python dev/herm_time.py --out profiles/herm_assembly.json
    python dev/herm_time.py --solve --out profiles/herm_solve.json      # one Lp(z).solve of the Hermite Rijke family, default set-up
    python dev/herm_time.py --solve --hierarchy --out profiles/herm_solve_hierarchy.json
                                                                        # ... with herm_hierarchy: p-hierarchy and per-level weight scaling,
                                                                        # on the Rijke family and on w^2 M + K of kuhn_cube(n)

There is no threshold and no parent to compare with: the numbers are a record."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np
import wae_amd  # noqa
from wae_amd import _lib
from wae_amd.helmholtz.assemble import assemble_herm, assemble_herm_boundary, assemble_herm_flame, herm_connectivity

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=26)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--solve", action="store_true")
ap.add_argument("--hierarchy", action="store_true")
ap.add_argument("--out", default="")
a = ap.parse_args()
GOLDEN = os.path.join(ROOT, "tests", "golden")


def kuhn_cube(n):
    """points, tetrahedra (6 n^3: per cell one for every order of the axes) and the boundary triangles of the face z = 1"""
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
    tets = np.concatenate(tets).astype(np.int32)
    top = pts[:, 2] == 1.0
    faces = np.concatenate([tets[:, [b for b in range(4) if b != k]] for k in range(4)])
    return pts, tets, faces[top[faces].all(axis=1)].astype(np.int32)


def rijke():
    z = np.load(os.path.join(GOLDEN, "rijke_mesh.npz"))
    fl = np.load(os.path.join(GOLDEN, "rijke_flame.npz"))
    flame = (fl["flame_tets"], int(fl["ref_tet"]), np.array([0.0, 0.0, -0.00101]), fl["n_ref"], float(fl["nglobal_scaled"]))
    return z["points"], z["tetrahedra"], z["outlet_triangles"], z["c_tet"], z["outlet_c"], flame


def timed(fn, reps):
    fn()                                                                # warm-up
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return out


def measure(name, pts, tets, tris, c_tet, c_tri, flame, triad):
    calls = {"connectivity": lambda: herm_connectivity(pts, tets, tris), "assemble": lambda: assemble_herm(pts, tets, tris, c_tet, dtype=np.float64),
             "boundary": lambda: assemble_herm_boundary(pts, tets, tris, c_tri), "flame": lambda: assemble_herm_flame(pts, tets, tris, *flame)}
    M, _ = assemble_herm(pts, tets, tris, c_tet, dtype=np.float64)
    res = {"mesh": name, "npoints": len(pts), "ntets": len(tets), "ntris": len(tris), "nflame": len(flame[0]), "ndof": M.shape[0], "nnz": int(M.nnz)}
    for key, fn in calls.items():
        t = timed(fn, a.reps)
        res[f"seconds_{key}"] = t
        res[f"median_{key}"] = float(np.median(t))
    sort_bytes = len(tets) * (400 + 800) * 8
    res["sort_bytes_interior"] = sort_bytes
    res["sort_GBps_over_entry_time"] = sort_bytes / res["median_assemble"] / 1e9
    res["fraction_of_triad"] = res["sort_GBps_over_entry_time"] / triad if triad else None
    return res


def solve_once():
    """one Lp(z).solve of the Hermite Rijke family with the default set-up: an observation, whatever it does"""
    from wae_amd.helmholtz.family import helmholtz_family
    pts, tets, tris, c_tet, c_tri, flame = rijke()
    M, K = assemble_herm(pts, tets, tris, c_tet)
    t = {"M": M, "K": K, "C": assemble_herm_boundary(pts, tets, tris, c_tri), "Q": assemble_herm_flame(pts, tets, tris, *flame)[0]}
    Lp = helmholtz_family(t, n=1.0, tau=0.001)
    Lp.solver_ref = 340 * 2 * np.pi
    z = 340 * 2 * np.pi
    rng = np.random.default_rng(0)
    B = rng.standard_normal((M.shape[0], 8)) + 1j * rng.standard_normal((M.shape[0], 8))
    res = {"family": "Hermite Rijke, n = 1, tau = 1e-3", "d": M.shape[0], "z": z, "columns": 8, "tol": 1e-12}
    try:
        X = Lp(z).solve(B, tol=1e-12)
        info = dict(Lp.device().last_info)
        res.update(info={k: (float(v) if isinstance(v, float) else int(v)) for k, v in info.items()}, finite=bool(np.all(np.isfinite(X))))
    except Exception as e:                                              # noqa: BLE001 -- the observation is what happened
        res["error"] = f"{type(e).__name__}: {e}"
    Lp._drop_device()
    return res


def solve_hierarchy():
    """Lp(z).solve with the set-up of helmholtz.family.herm_hierarchy: iterations, levels, lambda_l, s_l and seconds (set-up apart)"""
    from wae_amd.helmholtz.assemble import herm_prolongators
    from wae_amd.helmholtz.family import helmholtz_family, herm_hierarchy
    from wae_amd.nlevp.algebra import pow2
    from wae_amd.nlevp.linopfam import LinearOperatorFamily, Term
    out = []
    pts, tets, tris, c_tet, c_tri, flame = rijke()
    M, K = assemble_herm(pts, tets, tris, c_tet)
    t = {"M": M, "K": K, "C": assemble_herm_boundary(pts, tets, tris, c_tri), "Q": assemble_herm_flame(pts, tets, tris, *flame)[0]}
    cases = [("Hermite Rijke, n = 1, tau = 1e-3", helmholtz_family(t, n=1.0, tau=0.001), (pts, tets, tris), 340 * 2 * np.pi)]
    kp, kt, ks = kuhn_cube(a.n)
    Mc, Kc = assemble_herm(kp, kt, ks)
    Lc = LinearOperatorFamily(["ω"], [0.0])
    Lc.symmetry_tol = 1e-14
    Lc.push(Term(Mc, (pow2,), (("ω",),), "ω^2", "M"))
    Lc.push(Term(Kc, (), (), "", "K"))
    cases.append((f"w^2 M + K on kuhn_cube({a.n}), Neumann walls", Lc, (kp, kt, ks), 3.0 * (1 + 0.02j)))
    for name, Lp, mesh, z in cases:
        d = Lp.size()
        rng = np.random.default_rng(0)
        B = rng.standard_normal((d, 8)) + 1j * rng.standard_normal((d, 8))
        res = {"family": name, "d": d, "z": [z.real, z.imag] if isinstance(z, complex) else z, "columns": 8, "tol": 1e-10}
        try:
            t0 = time.perf_counter()
            Ps = herm_prolongators(*mesh)
            res["seconds_prolongators"] = time.perf_counter() - t0
            herm_hierarchy(Lp, *mesh)
            Lp.solver_ref = z
            t0 = time.perf_counter()
            fam = Lp.ensure_solver()
            res["seconds_setup"] = time.perf_counter() - t0
            lam, scale = fam.level_weights()
            res.update(prolongator_shapes=[list(P.shape) for P in Ps], lambda_l=[float(x) for x in lam], s_l=[float(x) for x in scale])
            X = Lp(z).solve(B, tol=1e-10)
            info = dict(fam.last_info)
            res.update(info={k: (float(v) if isinstance(v, float) else int(v)) for k, v in info.items()}, finite=bool(np.all(np.isfinite(X))))
            R = B - Lp(z) @ X
            res["plain_relres_max"] = float(np.max(np.linalg.norm(R, axis=0) / np.linalg.norm(B, axis=0)))
        except Exception as e:                                          # noqa: BLE001 -- the observation is what happened
            res["error"] = f"{type(e).__name__}: {e}"
        Lp._drop_device()
        out.append(res)
    return {"cases": out}


if a.solve and a.hierarchy:
    res = solve_hierarchy()
elif a.solve:
    res = solve_once()
else:
    tri = C.c_double(0.0)
    _lib.check(_lib.lib().wae_bench_triad(0, 1 << 27, 20, C.byref(tri)))
    pts, tets, tris, c_tet, c_tri, flame = rijke()
    kp, kt, ks = kuhn_cube(a.n)
    mid = np.nonzero(np.abs(kp[kt].mean(axis=1)[:, 2] - 0.5) < 1.0 / a.n)[0].astype(np.int32)           # a slab of flame tetrahedra
    kflame = (mid, int(mid[0]), kp[kt[mid[0]]].mean(axis=0), np.array([0.0, 0.0, 1.0]), 1.0)
    res = {"triad_GBps": tri.value, "reps": a.reps,
           "meshes": [measure("rijke", pts, tets, tris, c_tet, c_tri, flame, tri.value),
                      measure(f"kuhn_cube({a.n})", kp, kt, ks, None, None, kflame, tri.value)]}
print(json.dumps(res))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
