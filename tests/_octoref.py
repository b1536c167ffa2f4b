"""Host reference of the uniform mesh refinement (`octosplit`, src/Meshutils.jl:589-747 of the reference) in numpy, sharing no code with the
product (csrc/octosplit.hip, helmholtz/refine.py); pinned by tests/test_octoref.py.  Everything is 0-based.

One level:
 - the unique tetrahedron edges in the order of the reference's mesh.lines (src/Mesh/sorter.jl:9-31): ascending by (larger point, smaller
   point); the old points keep their numbers, the midpoint of edge e is point N + e = (x_a + x_b) * 0.5;
 - a tetrahedron (A,B,C,D) gives [A,AB,AC,AD] [B,AB,BC,BD] [C,AC,BC,CD] [D,AD,BD,CD] and four children of the inner octahedron, cut along the
   shortest of the diagonals AB-CD, AC-BD, AD-BC (<= tie-breaks in that order, Meshutils.jl:620-640), lengths compared by
   d2 = (dx*dx + dy*dy) + dz*dz in float64 on the stored midpoints (numpy rounds every operation on its own);
 - a triangle (A,B,C) gives [A,AB,AC] [B,AB,BC] [C,AC,BC] [AB,AC,BC];
 - the children are listed ascending by "vertices sorted descending, compared lexicographically", their own vertex order kept; the labels
   are the positions of a parent's children in that list."""
import numpy as np

_INNER = {            # diagonal -> the four inner children in terms of the midpoints (Meshutils.jl:625-640)
    0: (("AB", "CD", "AC", "AD"), ("AB", "CD", "AD", "BD"), ("AB", "CD", "BD", "BC"), ("AB", "CD", "BC", "AC")),
    1: (("AC", "BD", "AB", "AD"), ("AC", "BD", "AD", "CD"), ("AC", "BD", "CD", "BC"), ("AC", "BD", "BC", "AB")),
    2: (("AD", "BC", "AC", "CD"), ("AD", "BC", "CD", "BD"), ("AD", "BC", "BD", "AB"), ("AD", "BC", "AB", "AC")),
}


class Level:
    """points (n, 3), tets (nt, 4), tris (ns, 3); from the level below: parents (new points, 2) = (larger, smaller) end, tet_labels
    (nt / 8, 8), tri_labels (ns / 4, 4), diagonal (nt / 8,) = 0, 1, 2 for AB-CD, AC-BD, AD-BC"""

    def __init__(self, points, tets, tris, parents=None, tet_labels=None, tri_labels=None, diagonal=None):
        self.points, self.tets, self.tris = points, tets, tris
        self.parents, self.tet_labels, self.tri_labels, self.diagonal = parents, tet_labels, tri_labels, diagonal


def _sorted_children(children):
    """(the children in the package's list order, labels with labels[i] = position of child i); ValueError on two equal children"""
    key = -np.sort(-children.astype(np.int64), axis=1)                 # vertices descending
    order = np.lexsort(tuple(key[:, k] for k in range(key.shape[1] - 1, -1, -1)))
    ks = key[order]
    if len(ks) > 1 and np.any(np.all(ks[1:] == ks[:-1], axis=1)):
        raise ValueError("two equal children: a simplex is listed twice")
    labels = np.empty(len(children), dtype=np.int32)
    labels[order] = np.arange(len(children), dtype=np.int32)
    return children[order], labels


def split(points, tets, tris=None):
    """one refinement of (points, tets, tris) -> Level"""
    points = np.asarray(points, dtype=np.float64)
    tets = np.asarray(tets, dtype=np.int64).reshape(-1, 4)
    tris = np.zeros((0, 3), dtype=np.int64) if tris is None else np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    N = len(points)
    if tets.min() < 0 or tets.max() >= N or (len(tris) and (tris.min() < 0 or tris.max() >= N)):
        raise ValueError("an index outside the points")
    pairs = np.concatenate([tets[:, [i, j]] for i in range(4) for j in range(i + 1, 4)])
    lines = np.unique(pairs.max(axis=1) * N + pairs.min(axis=1))        # ascending by (larger, smaller)
    a, b = lines // N, lines % N
    P = np.vstack([points, (points[a] + points[b]) * 0.5])

    def mid(u, v):
        k = np.maximum(u, v) * N + np.minimum(u, v)
        e = np.searchsorted(lines, k)
        if np.any(e >= len(lines)) or np.any(lines[np.minimum(e, len(lines) - 1)] != k):
            raise ValueError("an edge that is no tetrahedron's edge")
        return N + e

    A, B, C, D = tets.T
    m = {"A": A, "B": B, "C": C, "D": D, "AB": mid(A, B), "AC": mid(A, C), "AD": mid(A, D), "BC": mid(B, C), "BD": mid(B, D), "CD": mid(C, D)}

    def d2(p, q):
        d = P[p] - P[q]
        return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]

    ab_cd, ac_bd, ad_bc = d2(m["AB"], m["CD"]), d2(m["AC"], m["BD"]), d2(m["AD"], m["BC"])
    diagonal = np.where((ab_cd <= ac_bd) & (ab_cd <= ad_bc), 0, np.where((ac_bd <= ab_cd) & (ac_bd <= ad_bc), 1, 2))
    kids = np.empty((len(tets), 8, 4), dtype=np.int64)
    for k, names in enumerate((("A", "AB", "AC", "AD"), ("B", "AB", "BC", "BD"), ("C", "AC", "BC", "CD"), ("D", "AD", "BD", "CD"))):
        kids[:, k] = np.stack([m[n] for n in names], axis=1)
    for dg, table in _INNER.items():
        sel = diagonal == dg
        for k, names in enumerate(table):
            kids[sel, 4 + k] = np.stack([m[n][sel] for n in names], axis=1)
    new_tets, tl = _sorted_children(kids.reshape(-1, 4))
    if len(tris):
        A, B, C = tris.T
        AB, AC, BC = mid(A, B), mid(A, C), mid(B, C)
        tk = np.stack([np.stack(c, axis=1) for c in ((A, AB, AC), (B, AB, BC), (C, AC, BC), (AB, AC, BC))], axis=1)
        new_tris, sl = _sorted_children(tk.reshape(-1, 3))
    else:
        new_tris, sl = np.zeros((0, 3), dtype=np.int64), np.zeros(0, dtype=np.int32)
    return Level(P, new_tets.astype(np.int32), new_tris.astype(np.int32), np.stack([a, b], axis=1).astype(np.int32), tl.reshape(-1, 8),
                 sl.reshape(-1, 4), diagonal)


def refine(points, tets, tris=None, levels=1):
    """[level 0 (the input), level 1, ..., level `levels`]"""
    tets = np.asarray(tets, dtype=np.int32).reshape(-1, 4)
    tris = np.zeros((0, 3), dtype=np.int32) if tris is None else np.asarray(tris, dtype=np.int32).reshape(-1, 3)
    out = [Level(np.asarray(points, dtype=np.float64), tets, tris)]
    for _ in range(levels):
        out.append(split(out[-1].points, out[-1].tets, out[-1].tris))
    return out


def prolong(hier, X, from_level=0, to_level=None):
    """nested P1 embedding: old rows copied, the row of a new point = (x[a] + x[b]) * 0.5, level by level"""
    to_level = len(hier) - 1 if to_level is None else to_level
    X = np.asarray(X)
    for l in range(from_level + 1, to_level + 1):
        par = hier[l].parents
        X = np.concatenate([X, (X[par[:, 0]] + X[par[:, 1]]) * 0.5], axis=0)
    return X


def carry_field(hier, values, kind="tet", to_level=None):
    """children inherit the parent's value"""
    to_level = len(hier) - 1 if to_level is None else to_level
    v = np.asarray(values)
    for l in range(1, to_level + 1):
        lab = hier[l].tet_labels if kind == "tet" else hier[l].tri_labels
        out = np.empty((lab.size,) + v.shape[1:], dtype=v.dtype)
        for k in range(lab.shape[1]):
            out[lab[:, k]] = v
        v = out
    return v


def carry_domain(hier, idx, kind="tet", to_level=None):
    """the sorted list of the children of the listed simplices (Meshutils.jl:724-740)"""
    to_level = len(hier) - 1 if to_level is None else to_level
    d = np.asarray(idx, dtype=np.int64)
    for l in range(1, to_level + 1):
        lab = hier[l].tet_labels if kind == "tet" else hier[l].tri_labels
        d = np.sort(np.concatenate([lab[i] for i in d]).astype(np.int64))
    return d


def volumes(points, tets):
    X = points[np.asarray(tets, dtype=np.int64)]
    return np.abs(np.linalg.det(X[:, :3] - X[:, 3:4])) / 6.0


def first_containing(points, tets, x):
    """find_tetrahedron_containing_point (Meshutils.jl:800-816): the first tetrahedron in list order with all barycentric coordinates of
    x in [0, 1]; -1 if none"""
    X = points[np.asarray(tets, dtype=np.int64)]
    J = np.transpose(X[:, :3] - X[:, 3:4], (0, 2, 1))
    xi = np.linalg.solve(J, (np.asarray(x, dtype=np.float64) - X[:, 3])[:, :, None])[:, :, 0]
    xi = np.concatenate([xi, 1.0 - xi.sum(axis=1, keepdims=True)], axis=1)
    hit = np.nonzero(np.all((xi >= 0) & (xi <= 1), axis=1))[0]
    return int(hit[0]) if len(hit) else -1


# ---- the five meshes of the tests ------------------------------------------------------------------------------------------------------
SHEAR = np.array([[1.0, 0.3, 0.1], [0.0, 1.0, 0.45], [0.0, 0.0, 1.0]])
MESHES = ["one", "two", "cube", "sheared", "rijke"]


def mesh(name):
    """(points, tets, tris)"""
    import os

    import _p2ref
    if name == "one":
        pts = np.array([[0.0, 0.0, 0.0], [1.0, 0.1, 0.0], [0.2, 0.9, 0.1], [0.1, 0.2, 0.8]])
        return pts, np.array([[0, 1, 2, 3]], dtype=np.int32), np.array([[0, 1, 2], [3, 1, 0]], dtype=np.int32)
    if name == "two":                  # two tetrahedra on the face (3, 1, 4), one with det J < 0; points not in ascending order
        pts = np.array([[0.1, 0.2, 1.1], [1.0, 0.0, 0.1], [0.3, 0.1, -0.9], [0.0, 0.0, 0.0], [0.1, 1.2, 0.0]])
        return pts, np.array([[3, 1, 4, 0], [3, 1, 4, 2]], dtype=np.int32), np.array([[4, 1, 0], [2, 3, 1]], dtype=np.int32)
    if name in ("cube", "sheared"):
        pts, tets, top = _p2ref.kuhn_cube(2, 1.0)
        return (pts if name == "cube" else pts @ SHEAR.T), tets, top
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rijke_mesh.npz"))
    return z["points"], z["tetrahedra"], z["outlet_triangles"]
