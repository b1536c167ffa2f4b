"""Point probes of a finite-element solution as sparse functionals: the host side of ``get_p`` / ``get_n_grad_p`` of the reference
(src/FEM/helmholtz_getters.jl:7-45).  Each probe returns ``(idx, val)`` with  p(x) = Σ_i val[i]·v[idx[i]]  resp.  n·∇p(x) = Σ_i val[i]·v[idx[i]]
for every solution vector v of the space -- the observers of ``nlevp.forced_response``, which applies them on the device."""
from __future__ import annotations

import numpy as np

_EDGES = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))          # local edge order of p2_connectivity


def _barycentric(X, x):
    """(l (4,), grad l (4, 3)) of the point x in the tetrahedron with corners X (4, 3); corner 4 is the origin of the local coordinates"""
    J = (X[:3] - X[3]).T
    Ji = np.linalg.inv(J)
    l3 = Ji @ (np.asarray(x, dtype=np.float64) - X[3])
    return np.append(l3, 1.0 - l3.sum()), np.vstack([Ji, -Ji.sum(axis=0)])


def find_tetrahedron(points, tets, x, tol=1e-10):
    """Index of a tetrahedron that contains the point x (find_tetrahedron_containing_point): the one in which the smallest barycentric
    coordinate of x is largest; ValueError if that is below -tol, i.e. x lies outside the mesh."""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    tt = np.asarray(tets, dtype=np.int64).reshape(-1, 4)
    x = np.asarray(x, dtype=np.float64)
    if x.shape != (3,):
        raise ValueError(f"a point has 3 coordinates, got shape {x.shape}")
    X = pts[tt]                                                       # (ntets, 4, 3)
    J = np.transpose(X[:, :3] - X[:, 3:4], (0, 2, 1))
    l3 = np.linalg.solve(J, (x - X[:, 3])[:, :, None])[:, :, 0]
    lmin = np.minimum(l3.min(axis=1), 1.0 - l3.sum(axis=1))
    t = int(np.argmax(lmin))
    if not lmin[t] >= -tol:
        raise ValueError(f"the point {x.tolist()} lies in no tetrahedron of the mesh")
    return t


def _element(points, tets, x, order, tet, tets10):
    if order not in ("lin", "quad"):
        raise ValueError(f"order must be 'lin' or 'quad', got {order!r}")
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    tt = np.asarray(tets, dtype=np.int64).reshape(-1, 4)
    t = find_tetrahedron(pts, tt, x) if tet is None else int(tet)
    if not 0 <= t < len(tt):
        raise ValueError(f"tetrahedron {t} is outside 0..{len(tt) - 1}")
    lam, G = _barycentric(pts[tt[t]], x)
    if order == "lin":
        return tt[t].astype(np.int32), lam, G
    if tets10 is None:
        from .assemble import p2_connectivity
        tets10 = p2_connectivity(len(pts), tt)[1]
    return np.asarray(tets10)[t].astype(np.int32), lam, G


def probe_p(points, tets, x, order="lin", tet=None, tets10=None):
    """get_p as a functional: (idx, val) with p(x) = Σ val·v[idx].  order "lin": the barycentric coordinates on the 4 points of the
    tetrahedron; "quad": l_i(2l_i-1) on the points and 4·l_i·l_j on the edges, edge DoFs as numbered by ``p2_connectivity`` (``tets10``: its
    second result, if the caller has it already).  ``tet``: the tetrahedron that holds x, if known (else ``find_tetrahedron``)."""
    idx, lam, _ = _element(points, tets, x, order, tet, tets10)
    if order == "lin":
        return idx, lam
    return idx, np.concatenate([lam * (2.0 * lam - 1.0), [4.0 * lam[i] * lam[j] for i, j in _EDGES]])


def probe_n_grad_p(points, tets, x, n, order="lin", tet=None, tets10=None):
    """get_n_grad_p as a functional: (idx, val) with n·∇p(x) = Σ val·v[idx]; val_b = n·∇φ_b(x), the weights of the ``g`` of the flame
    operator (``assemble_p1_flame`` / ``assemble_p2_flame``) without its factor -nlocal."""
    n = np.asarray(n, dtype=np.float64)
    if n.shape != (3,):
        raise ValueError(f"a direction has 3 components, got shape {n.shape}")
    idx, lam, G = _element(points, tets, x, order, tet, tets10)
    gn = G @ n                                                        # n·∇l_i
    if order == "lin":
        return idx, gn
    return idx, np.concatenate([(4.0 * lam - 1.0) * gn, [4.0 * (lam[j] * gn[i] + lam[i] * gn[j]) for i, j in _EDGES]])
