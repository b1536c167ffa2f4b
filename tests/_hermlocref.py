"""Host reference of the Hermite rows of the point locator (csrc/locate.hip, order 3), for tests only; pinned by tests/test_herm_locate_ref.py.

 - ``weight_rows_herm``: the 20 weights of p(x) (kind 0) or n . grad p(x) (kind 1) from ``_hermref.Elements`` -- the dual basis built on
   the physical element by inverting the functional-by-monomial matrix, in np.longdouble or np.float64.  It uses neither the reference-element
   table nor J, so it is another route than the device's, and it is what the device is compared with.
 - ``device_rows_herm``: a float64 transliteration of the device formula, operation for operation: the coordinates of ``_locref.bary`` as
   xi, the monomials of csrc/herm_tables.h (read from that file), psi_a = sum_m coef[a][m] xi^exp[m] with the zero coefficients left out,
   and the recombination w[4 (1 + i) + k] = sum_j J[i][j] psi[4 (1 + j) + k].  It sets the tolerance of the GPU tests and carries the
   seeded defects that tests/test_herm_locate_ref.py must catch:
       "transposed"  J[j][i] in the recombination (passes wherever J is symmetric);
       "lambda3"     the fourth barycentric coordinate in the place of xi_3;
       "faces"       the four face functions shifted by one: face k takes the function of a face that holds point k, not the one opposite."""
import functools
import os
import re

import numpy as np

import _hermref as H
import _locref as R

EPS = np.finfo(np.float64).eps
N_DIR = np.array([0.3, -0.5, 0.8])


@functools.lru_cache(maxsize=None)
def tables():
    """(exp (20, 3) int, coef (20, 20) float64) of csrc/herm_tables.h"""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "wavesandeigenvalues.jl_amd", "csrc", "herm_tables.h")
    src = open(path).read()
    num = r"[-+]?\d+(?:\.\d*)?(?:[eE][-+]?\d+)?"
    e = re.search(r"kHermExp\[20\]\[3\]\s*=\s*\{(.*?)\};", src, re.S).group(1)
    c = re.search(r"kHermCoef\[20\]\[20\]\s*=\s*\{(.*?)\};", src, re.S).group(1)
    exp = np.array([int(v) for v in re.findall(r"\d+", e)]).reshape(20, 3)
    coef = np.array([float(v) for v in re.findall(num, c)]).reshape(20, 20)
    return exp, coef


def weight_rows_herm(points, tets, X, tet, kind=0, n=None, dtype=np.longdouble):
    """val (nq, 20) of the functionals at the points X in their tetrahedra tet (all >= 0), in the local order of tets20"""
    P = np.asarray(points).astype(dtype)[np.asarray(tets, dtype=np.int64)[np.asarray(tet, dtype=np.int64)]]
    E = H.Elements(P)
    x = np.asarray(X).astype(dtype)[:, None, :]
    if kind == 0:
        return E.values(x)[:, 0]
    nn = np.broadcast_to(np.asarray(n).astype(dtype), np.shape(X))
    return np.einsum("qi,qia->qa", nn, E.gradients(x)[:, 0])


def device_rows_herm(points, tets, X, tet, kind=0, n=None, defect=None):
    """the device formula in float64, every operation rounded on its own, in the device's order"""
    exp, coef = tables()
    P = np.asarray(points, dtype=np.float64)[np.asarray(tets, dtype=np.int64)[np.asarray(tet, dtype=np.int64)]]
    X = np.asarray(X, dtype=np.float64)
    if kind == 0:
        l = R.bary(P, X)
        g = None
    else:
        l, g = R.bary(P, X, n=np.broadcast_to(np.asarray(n, dtype=np.float64), X.shape))
    xi = [l[:, 0], l[:, 1], l[:, 3] if defect == "lambda3" else l[:, 2]]
    gg = None if g is None else [g[:, 0], g[:, 1], g[:, 3] if defect == "lambda3" else g[:, 2]]
    one = np.ones(len(X))
    pw = [[one, xi[j], xi[j] * xi[j], (xi[j] * xi[j]) * xi[j]] for j in range(3)]
    mono = []
    for m in range(20):
        e = exp[m]
        if kind == 0:
            mono.append((pw[0][e[0]] * pw[1][e[1]]) * pw[2][e[2]])
            continue
        d = np.zeros(len(X))
        for j in range(3):
            if e[j] == 0:
                continue
            term = float(e[j]) * one
            for i in range(3):
                term = term * pw[i][e[i] - 1 if i == j else e[i]]
            d = d + gg[j] * term
        mono.append(d)
    psi = []
    for a in range(20):
        acc = np.zeros(len(X))
        for m in range(20):
            if coef[a, m] != 0.0:
                acc = acc + coef[a, m] * mono[m]
        psi.append(acc)
    J = np.transpose(P[:, :3] - P[:, 3:4], (0, 2, 1))                 # J[:, i, j] = (p_j - p_3)_i
    if defect == "transposed":
        J = np.transpose(J, (0, 2, 1))
    w = [None] * 20
    for k in range(4):
        w[k] = psi[k]
        w[16 + k] = psi[16 + (k + 1) % 4] if defect == "faces" else psi[16 + k]
        for i in range(3):
            w[4 * (1 + i) + k] = (J[:, i, 0] * psi[4 + k] + J[:, i, 1] * psi[8 + k]) + J[:, i, 2] * psi[12 + k]
    return np.stack(w, axis=1)


def row_bound(points, tets, tet, kind, n=None):
    """eps kappa_inf(J) s per weight, (nq, 20): s = 1 for the value and face weights, ||J||_inf for the weights of the gradient unknowns; for
    kind 1 times ||J^-1||_inf ||n||.  The unit in which the rows are compared: c times this is the tolerance."""
    kap, jinv = R.conditioning(points, tets, tet)
    s = np.ones((len(kap), 20))
    s[:, 4:16] = (kap / jinv)[:, None]
    b = EPS * kap[:, None] * s
    return b * (jinv * np.linalg.norm(n))[:, None] if kind else b


def located_points(name, count=600):
    """the selection of tests/test_gpu_locate.py: a seeded share of its located queries with their reference tetrahedra"""
    import test_gpu_locate as G
    return G.located_points(name, count)


def mesh(name):
    import test_gpu_locate as G
    return G.mesh(name)


@functools.lru_cache(maxsize=None)
def measured_herm_ratio(name):
    """the largest |float64 transliteration - longdouble| / row_bound over the located points of one mesh, both kinds"""
    pts, tets = mesh(name)
    X, t = located_points(name)
    worst = 0.0
    for kind in (0, 1):
        d = np.abs(device_rows_herm(pts, tets, X, t, kind, N_DIR).astype(np.longdouble) - weight_rows_herm(pts, tets, X, t, kind, N_DIR))
        worst = max(worst, float(np.max(d.astype(np.float64) / row_bound(pts, tets, t, kind, N_DIR))))
    return worst


# ---- cubics with every monomial class ---------------------------------------------------------------------------------------------------
def cubic(k, scale=1.0, centre=(0.0, 0.0, 0.0)):
    """(f, grad f) of the k-th test cubic in y = (x - centre) * scale; each has an x^3, an x^2 y and an x y z term; generic in the dtype of x"""
    A = [dict(c3=(0.7, -0.4, 0.9), c21=(0.5, -0.8, 0.3, 0.6, -0.2, 0.4), cxyz=1.1, q=(0.3, -0.2, 0.5), lin=(0.4, 0.1, -0.6), c0=0.25),
         dict(c3=(-1.2, 0.8, 0.3), c21=(0.9, 0.2, -0.7, -0.5, 0.6, 0.1), cxyz=-0.9, q=(-0.4, 0.7, 0.2), lin=(-0.3, 0.8, 0.2), c0=-0.5),
         dict(c3=(0.2, 1.1, -0.6), c21=(-0.3, 0.7, 0.8, 0.4, -0.9, -0.6), cxyz=0.6, q=(0.6, 0.1, -0.8), lin=(0.9, -0.5, 0.3), c0=1.0)][k]
    pairs = [(0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1)]          # y_a^2 y_b

    def parts(x):
        x = np.asarray(x)
        return (x - np.asarray(centre).astype(x.dtype)) * x.dtype.type(scale)

    def f(x):
        y = parts(x)
        out = A["c0"] + sum(A["lin"][i] * y[:, i] + A["q"][i] * y[:, i] ** 2 + A["c3"][i] * y[:, i] ** 3 for i in range(3))
        out = out + sum(c * y[:, a] ** 2 * y[:, b] for c, (a, b) in zip(A["c21"], pairs))
        return out + A["cxyz"] * y[:, 0] * y[:, 1] * y[:, 2]

    def grad(x):
        y = parts(x)
        g = [A["lin"][i] + 2 * A["q"][i] * y[:, i] + 3 * A["c3"][i] * y[:, i] ** 2 for i in range(3)]
        for c, (a, b) in zip(A["c21"], pairs):
            g[a] = g[a] + 2 * c * y[:, a] * y[:, b]
            g[b] = g[b] + c * y[:, a] ** 2
        g[0] = g[0] + A["cxyz"] * y[:, 1] * y[:, 2]
        g[1] = g[1] + A["cxyz"] * y[:, 0] * y[:, 2]
        g[2] = g[2] + A["cxyz"] * y[:, 0] * y[:, 1]
        return np.stack(g, axis=1) * y.dtype.type(scale)

    return f, grad


def mesh_cubic(points, k):
    """the k-th cubic in coordinates centred on the mesh and scaled to its extent (O(1) values on every mesh)"""
    pts = np.asarray(points, dtype=np.float64)
    return cubic(k, 1.0 / float(np.max(pts.max(axis=0) - pts.min(axis=0))), tuple(pts.mean(axis=0)))
