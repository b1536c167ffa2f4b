"""Geometric reference of the P2 prolongation between two octosplit levels, for tests only: it shares nothing with the combinatorial rule of
the product (helmholtz/refine.py ``_p2_step``, csrc/octosplit.hip).

A row of the prolongator is the coarse P2 basis evaluated where the fine unknown sits.  For every fine unknown: its location (a point of the
fine level, or the midpoint of a fine edge numbered by ``_p2ref.connectivity``), a fine tetrahedron that holds it, that tetrahedron's parent
through ``tet_labels``, the barycentric coordinates of the location in the parent from a 3 x 3 solve, and ``_p2ref.basis(4)`` there.  A
location on a face or an edge shared by several parents gets the same row from each of them: the basis functions of the nodes off the face
vanish on it.  Values below DROP in magnitude are roundings of such zeros (the coordinates are multiples of 1/4 up to a few ulp, the
smallest weight of a row is 1/8) and are not stored."""
import functools

import numpy as np
import scipy.sparse as sp

import _octoref as O
import _p2ref as P2

DROP = 1e-9


@functools.lru_cache(maxsize=None)
def hierarchy(name, levels=2):
    return O.refine(*O.mesh(name), levels=levels)


def locations(level):
    """(ndof, 3): the points, then the midpoints of the edges in the P2 order"""
    edges, _, _ = P2.connectivity(len(level.points), level.tets)
    return np.vstack([level.points, (level.points[edges[:, 0]] + level.points[edges[:, 1]]) * 0.5])


def _basis_at(lam):
    return np.array([P2._value(f, lam) for f in P2.basis(4)])


@functools.lru_cache(maxsize=None)
def prolongator(name, frm):
    """csr_matrix (ndof(frm + 1), ndof(frm)) of the step frm -> frm + 1 of mesh `name`, columns ascending"""
    H = hierarchy(name)
    Lc, Lf = H[frm], H[frm + 1]
    _, c10, _ = P2.connectivity(len(Lc.points), Lc.tets)
    _, f10, _ = P2.connectivity(len(Lf.points), Lf.tets)
    x = locations(Lf)
    parent_of = np.empty(len(Lf.tets), dtype=np.int64)
    for k in range(8):
        parent_of[Lf.tet_labels[:, k]] = np.arange(len(Lc.tets))
    holder = np.full(len(x), -1, dtype=np.int64)              # a fine tetrahedron that has the unknown among its 10 nodes
    holder[f10.ravel()] = np.repeat(np.arange(len(f10)), 10)
    assert np.all(holder >= 0)
    rows, cols, vals = [], [], []
    for i in range(len(x)):
        t = parent_of[holder[i]]
        X = Lc.points[c10[t, :4]]
        lam3 = np.linalg.solve((X[:3] - X[3]).T, x[i] - X[3])
        phi = _basis_at(np.append(lam3, 1.0 - lam3.sum()))
        keep = np.abs(phi) > DROP
        rows.append(np.full(int(keep.sum()), i)); cols.append(c10[t][keep]); vals.append(phi[keep])
    A = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(len(x), len(Lc.points) + len(P2.edge_list(Lc.tets))))
    A = A.tocsr()
    A.sort_indices()
    return A


def quadratic(x, seed=0):
    """a quadratic polynomial with complex coefficients at the locations x (n, 3)"""
    rng = np.random.default_rng(seed)
    c = rng.standard_normal(10) + 1j * rng.standard_normal(10)
    X, Y, Z = x.T
    return c[0] + c[1] * X + c[2] * Y + c[3] * Z + c[4] * X * X + c[5] * Y * Y + c[6] * Z * Z + c[7] * X * Y + c[8] * X * Z + c[9] * Y * Z


def affine(x, seed=0):
    rng = np.random.default_rng(seed)
    c = rng.standard_normal(4) + 1j * rng.standard_normal(4)
    return c[0] + x @ c[1:]
