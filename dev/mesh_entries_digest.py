#!/usr/bin/env python3
"""SHA-256 of the raw bytes of everything the mesh-side entries return (assemble.hip, assemble_p2.hip, assemble_herm.hip, bloch.hip,
octosplit.hip, locate.hip), called through the wrappers of helmholtz/ on small fixed meshes: the Kuhn cube with 3^3 cells (64 points,
162 tetrahedra) with its boundary triangles, two levels of octosplit, the cube as a periodic cell (3 parts) and the six-point wedge with an axis
(6 parts).  Every variant is called: speed of sound per simplex and per point, P1 and P2, flame, source (also the empty speaker), both
shape sensitivities with their flame forms, Bloch numbering and fold, P1 and P2 prolongators and prolongation, the locator's find,
weights and sample for both orders and kinds; the Hermite entries; and, keys *_jit, assembly, flame and shape sensitivities of every
order on the cube with jittered points.

The kernels, their launch order and the hipCUB calls fix every bit of these arrays, so two builds of the library that differ only in
host code, or in where a kernel's expressions are written down, must print the same digests.  Prints one JSON object (and writes it
to --out).

    python dev/mesh_entries_digest.py --out profiles/mesh_entries_digest.json
"""
import argparse
import hashlib
import json
import os
import sys
from itertools import permutations

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import scipy.sparse as sp
import wae_amd  # noqa
from wae_amd.helmholtz import Locator, octosplit
from wae_amd.helmholtz import assemble as A
from wae_amd.helmholtz import bloch as B
from wae_amd.helmholtz.shape import boundary_triangles
from wae_amd.nlevp import Solution

ap = argparse.ArgumentParser()
ap.add_argument("--out", default="")
a = ap.parse_args()


def kuhn_cube(n):
    idx = lambda i, j, k: (i * (n + 1) + j) * (n + 1) + k
    g = np.arange(n + 1) / n
    pts = np.array([[g[i], g[j], g[k]] for i in range(n + 1) for j in range(n + 1) for k in range(n + 1)])
    tets = []
    for i in range(n):
        for j in range(n):
            for k in range(n):
                for perm in permutations(range(3)):
                    p = [i, j, k]
                    tet = [idx(*p)]
                    for ax in perm:
                        p[ax] += 1
                        tet.append(idx(*p))
                    tets.append(tet)
    return pts, np.array(tets, dtype=np.int32)


def sha(x):
    return hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()


res = {}


def put(name, *arrays):
    """arrays, scipy matrices (pattern and values) and numbers, each under its own key"""
    k = 0
    for x in arrays:
        if sp.issparse(x):
            x = sp.csr_matrix(x) if not sp.isspmatrix_csc(x) else x
            for part in (x.indptr, x.indices, x.data):
                res[f"{name}/{k}"] = sha(part)
                k += 1
        else:
            res[f"{name}/{k}"] = sha(np.asarray(x))
            k += 1


pts, tets = kuhn_cube(3)
tris = boundary_triangles(tets)[0].astype(np.int32)
assert pts.shape == (64, 3) and tets.shape == (162, 4)
NP, NT, NS = len(pts), len(tets), len(tris)
c_point = 1.0 + 0.5 * pts[:, 0] + 0.25 * pts[:, 1] * pts[:, 2]
c_tet = c_point[tets].mean(axis=1)
c_tri = c_point[tris].mean(axis=1)
speaker = tris[::3]
flame_tets = np.arange(40, 70, dtype=np.int32)
ref_tet, n_ref = 5, np.array([0.0, 0.6, 0.8])
x_ref = pts[tets[ref_tet]].mean(axis=0)
NE = A.p2_edge_count(tets)

# ---- assembly -----------------------------------------------------------------------------------------------------------------------
put("p1_assemble", *A.assemble_p1(pts, tets, dtype=np.float64))
put("p1_assemble_c_tet", *A.assemble_p1(pts, tets, c_tet, dtype=np.float64))
put("p1_assemble_cpoint", *A.assemble_p1(pts, tets, c_point=c_point, dtype=np.float64))
put("p1_boundary", A.assemble_p1_boundary(pts, tris))
put("p1_boundary_c_tri", A.assemble_p1_boundary(pts, tris, c_tri))
put("p1_boundary_cpoint", A.assemble_p1_boundary(pts, tris, c_point=c_point))
put("p1_flame", *A.assemble_p1_flame(pts, tets, flame_tets, ref_tet, n_ref, 1.75))
put("p1_source", A.assemble_p1_source(pts, speaker))
put("p1_source_c_tri", A.assemble_p1_source(pts, speaker, c_tri[::3]))
put("p1_source_cpoint", A.assemble_p1_source(pts, speaker, c_point=c_point))
put("p1_source_empty", A.assemble_p1_source(pts, np.zeros((0, 3), dtype=np.int32)))
put("p2_connectivity", *A.p2_connectivity(pts, tets, tris))
put("p2_embedding", A.p2_embedding(pts, tets))
put("p2_assemble", *A.assemble_p2(pts, tets, dtype=np.float64))
put("p2_assemble_c_tet", *A.assemble_p2(pts, tets, c_tet, dtype=np.float64))
put("p2_assemble_cpoint", *A.assemble_p2(pts, tets, c_point=c_point, dtype=np.float64))
put("p2_boundary", A.assemble_p2_boundary(pts, tets, tris))
put("p2_boundary_c_tri", A.assemble_p2_boundary(pts, tets, tris, c_tri))
put("p2_boundary_cpoint", A.assemble_p2_boundary(pts, tets, tris, c_point=c_point))
put("p2_flame", *A.assemble_p2_flame(pts, tets, flame_tets, ref_tet, x_ref, n_ref, 1.75))
put("p2_source", A.assemble_p2_source(pts, tets, speaker))
put("p2_source_c_tri", A.assemble_p2_source(pts, tets, speaker, c_tri[::3]))
put("p2_source_cpoint", A.assemble_p2_source(pts, tets, speaker, c_point=c_point))
put("p2_source_empty", A.assemble_p2_source(pts, tets, np.zeros((0, 3), dtype=np.int32)))

# ---- shape sensitivities --------------------------------------------------------------------------------------------------------------
rng = np.random.default_rng(7)
surface = np.unique(tris)[::2]
flame = {"flame_tets": flame_tets, "ref_tet": ref_tet, "n_ref": n_ref, "x_ref": x_ref, "nglobal_scaled": 1.75, "coeff": 0.3 - 0.2j}
for order, dim in (("lin", NP), ("quad", NP + NE)):
    v = rng.standard_normal(dim) + 1j * rng.standard_normal(dim)
    va = rng.standard_normal(dim) + 1j * rng.standard_normal(dim)
    sol = Solution({"ω": 3.0 + 0.4j}, v, va, "ω")
    kw = dict(v_ext=(v, va), order=order, h=1e-6, Y=0.7 - 0.1j)
    put(f"shape_{order}", A.discrete_adjoint_shape_sensitivity(pts, tets, None, surface, sol, None, bnd_tris=tris, bnd_c=c_tri, **kw))
    put(f"shape_{order}_c_tet", A.discrete_adjoint_shape_sensitivity(pts, tets, c_tet, surface, sol, None, **kw))
    put(f"shape_{order}_cpoint", A.discrete_adjoint_shape_sensitivity(pts, tets, None, surface, sol, None, bnd_tris=tris, c_point=c_point, **kw))
    put(f"shape_{order}_flame", A.discrete_adjoint_shape_sensitivity(pts, tets, c_tet, np.unique(tets[flame_tets])[::2], sol, None, flame=flame, **kw))

# ---- Bloch cells ---------------------------------------------------------------------------------------------------------------------------
# the cube as a cell periodic in x: the points of the face x = 1 are the last 16, in the order of their twins on x = 0, the first 16
M2, K2 = A.assemble_p2(pts, tets, c_tet)
M1, K1 = A.assemble_p1(pts, tets, c_tet)
C2 = A.assemble_p2_boundary(pts, tets, tris, c_tri)
for order, mats in (("lin", (M1, K1)), ("quad", (M2, K2))):
    N = B.bloch_numbering(NP, tets, 48, 0, order=order)
    put(f"bloch_numbering_{order}", N.cell_dof, N.flags, N.edges, [N.dim, N.nimage_edges, N.naxis_edges])
    for i, parts in enumerate(B.blochify_device(mats, N, axis=False)):
        assert len(parts) == 3
        put(f"bloch_fold3_{order}_{i}", *parts)
N = B.bloch_numbering(NP, tets, 48, 0, order="quad")
put("bloch_fold3_complex", *B.blochify_device(C2 + 1j * C2.T, N, axis=False))
wedge_pts = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.1], [1.0, 0.0, 1.1], [0.6, 0.8, 0.1], [0.6, 0.8, 1.1]])
wedge_tets = np.array([[0, 1, 2, 4], [1, 2, 3, 4], [1, 3, 4, 5]], dtype=np.int32)
for order, asm in (("lin", A.assemble_p1), ("quad", A.assemble_p2)):
    N = B.bloch_numbering(6, wedge_tets, 4, 2, order=order)
    put(f"bloch_wedge_numbering_{order}", N.cell_dof, N.flags, N.edges, [N.dim, N.nimage_edges, N.naxis_edges])
    for i, parts in enumerate(B.blochify_device(asm(wedge_pts, wedge_tets), N, axis=True)):
        assert len(parts) == 6
        put(f"bloch_wedge_fold6_{order}_{i}", *parts)

# ---- octosplit ---------------------------------------------------------------------------------------------------------------------------
R = octosplit(pts, tets, tris, levels=2)
for l in range(3):
    put(f"octosplit_level{l}", R.points[l], R.tets[l], R.tris[l])
    if l:
        put(f"octosplit_labels{l}", R.parents[l], R.tet_labels[l], R.tri_labels[l])
for order in ("lin", "quad"):
    for l in range(2):
        put(f"octosplit_prolongator_{order}_{l}", R.prolongator(l, order))
    n0 = R.ndof(0, order)
    X = rng.standard_normal((n0, 3)) + 1j * rng.standard_normal((n0, 3))
    put(f"octosplit_prolong_{order}_0_2", R.prolong(X, 0, 2, order))
    put(f"octosplit_prolong_{order}_1_2", R.prolong(R.prolong(X[:, 0].real, 0, 1, order), 1, 2, order))
put("octosplit_prolongators_p_first", *R.prolongators(order="quad", p_first=True))

# ---- locator ---------------------------------------------------------------------------------------------------------------------------------
Q = np.concatenate([rng.uniform(-0.1, 1.1, (200, 3)), pts[::5], pts[tets[::9]].mean(axis=1)])
dirs = rng.standard_normal(Q.shape)
for target in (0, 2):
    loc = Locator(pts, tets, cell_target=target)
    put(f"locator_grid_{target}", [*loc.dims, loc.nrefs, loc.max_per_cell])
    tet, lam = loc.find(Q, tol=1e-9, barycentric=True)
    put(f"locator_find_{target}", tet, lam, loc.find(Q))
    for order, dim in (("lin", NP), ("quad", NP + NE)):
        V = rng.standard_normal((dim, 3)) + 1j * rng.standard_normal((dim, 3))
        for kind, n in (("p", None), ("n_grad_p", dirs)):
            put(f"locator_weights_{target}_{order}_{kind}", *loc.weights(Q, order, kind, n, outside="nan", tol=1e-9))
            put(f"locator_sample_{target}_{order}_{kind}", loc.sample(V, Q, order, kind, n, outside="nan", tol=1e-9))
    loc.close()

# ---- Hermite entries (added after the keys above; nothing above depends on them) --------------------------------------------------------
put("herm_connectivity", *A.herm_connectivity(pts, tets))
put("herm_connectivity_tris", *A.herm_connectivity(pts, tets, tris))
for tag, tr in (("", None), ("_tris", tris)):
    put(f"herm_assemble{tag}", *A.assemble_herm(pts, tets, tr, dtype=np.float64))
    put(f"herm_assemble{tag}_c_tet", *A.assemble_herm(pts, tets, tr, c_tet, dtype=np.float64))
put("herm_boundary", A.assemble_herm_boundary(pts, tets, tris))
put("herm_boundary_c_tri", A.assemble_herm_boundary(pts, tets, tris, c_tri))
put("herm_flame", *A.assemble_herm_flame(pts, tets, tris, flame_tets, ref_tet, x_ref, n_ref, 1.75))
put("herm_prolongators", *A.herm_prolongators(pts, tets, tris))

# ---- the jittered cube: generic Jacobians (on the Kuhn cube they hold only 0 and +-1/3, most products vanish and a different FMA
# contraction cannot show).  Every point moves by a fixed vector of amplitude 0.05, a sixth of the cell: no tetrahedron inverts.
ptsj = pts + np.random.default_rng(11).uniform(-0.05, 0.05, pts.shape)


def det_j(p):
    return np.linalg.det(np.transpose(p[tets[:, :3]] - p[tets[:, 3:4]], (0, 2, 1)))


assert np.all(np.sign(det_j(ptsj)) == np.sign(det_j(pts))) and np.all(np.abs(det_j(ptsj)) > 1e-3)
x_refj = ptsj[tets[ref_tet]].mean(axis=0)
put("p1_assemble_c_tet_jit", *A.assemble_p1(ptsj, tets, c_tet, dtype=np.float64))
put("p1_assemble_cpoint_jit", *A.assemble_p1(ptsj, tets, c_point=c_point, dtype=np.float64))
put("p2_assemble_c_tet_jit", *A.assemble_p2(ptsj, tets, c_tet, dtype=np.float64))
put("p2_assemble_cpoint_jit", *A.assemble_p2(ptsj, tets, c_point=c_point, dtype=np.float64))
put("herm_assemble_c_tet_jit", *A.assemble_herm(ptsj, tets, tris, c_tet, dtype=np.float64))
put("p1_flame_jit", *A.assemble_p1_flame(ptsj, tets, flame_tets, ref_tet, n_ref, 1.75))
put("p2_flame_jit", *A.assemble_p2_flame(ptsj, tets, flame_tets, ref_tet, x_refj, n_ref, 1.75))
put("herm_flame_jit", *A.assemble_herm_flame(ptsj, tets, tris, flame_tets, ref_tet, x_refj, n_ref, 1.75))
rngj = np.random.default_rng(13)
flamej = dict(flame, x_ref=x_refj)
for order, dim in (("lin", NP), ("quad", NP + NE)):
    v = rngj.standard_normal(dim) + 1j * rngj.standard_normal(dim)
    va = rngj.standard_normal(dim) + 1j * rngj.standard_normal(dim)
    sol = Solution({"ω": 3.0 + 0.4j}, v, va, "ω")
    kw = dict(v_ext=(v, va), order=order, h=1e-6, Y=0.7 - 0.1j)
    put(f"shape_{order}_jit", A.discrete_adjoint_shape_sensitivity(ptsj, tets, c_tet, surface, sol, None, bnd_tris=tris, bnd_c=c_tri, **kw))
    put(f"shape_{order}_cpoint_jit", A.discrete_adjoint_shape_sensitivity(ptsj, tets, None, surface, sol, None, bnd_tris=tris, c_point=c_point, **kw))
    put(f"shape_{order}_flame_jit",
        A.discrete_adjoint_shape_sensitivity(ptsj, tets, c_tet, np.unique(tets[flame_tets])[::2], sol, None, flame=flamej, **kw))

print(json.dumps(res))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
