"""CPU reference of the discrete-adjoint shape sensitivity (src/shape_sensitivity.jl:16-141 of the reference), for tests only: it shares no
code with the product.  For a surface point p, a coordinate and given vectors u (right) and w (left, adjoint):

    sens = -w^H (L+ - L-)/(2h) u,      L = om^2 M + K + om Y C + coeff Q

with L+-, the operator re-discretised on the simplices that touch p -- the tetrahedra, the boundary triangles and the flame domain REDUCED
to the tetrahedra at p, its volume included -- with p moved by +h and -h along the coordinate.  Two evaluations of the same number:

* ``sensitivity``: float64, through the pinned references.  The reduced mesh is assembled at +h and at -h (L+ - L- entry by entry, then the
  contraction, as the reference does) with _p2ref.assemble /
  assemble_boundary / assemble_flame / assemble_p1 and, for a nodal speed of sound, _nodalref.stiffness / boundary; a reduced P2 mesh numbers
  its own edges, so its matrices are contracted with the entries of u and w that belong to those edges in the numbering of the whole mesh
  (_p2ref.connectivity of both).  The two P1 pieces that the pinned files do not hold are written out here from their formulas: the boundary
  mass c |(x0-x2) x (x1-x2)| (1 + delta_ab)/24 and the flame operator S (x) g, S_a = |det J|/24, g_b = -nlocal grad l_b . n_ref.

* ``sensitivity_ext``: the same central difference in extended precision, for rounding yardsticks.  The geometry is rational in the coordinates:
  with the basis polynomials of _p2ref (basis, _diff, _mul, _integral; Fractions) the forms w^H M u, w^H K u, w^H C u, w^H Q u are products of
  geometry-free rational numbers with |det J|, |det J| grad l_i . grad l_j, |(x0-x2) x (x1-x2)| and 1/volume, all evaluated exactly from
  the (binary, hence rational) coordinates at +-h; only the square root of the boundary part is taken in ``decimal`` (60 digits)."""
import functools
from decimal import Decimal, getcontext
from fractions import Fraction

import numpy as np
import scipy.sparse as sp

import _nodalref as N
import _p2ref as R

getcontext().prec = 60


# ---- shared bookkeeping -------------------------------------------------------------------------------------------------------------------
class Problem:
    """everything that does not depend on the point: mesh, vectors, coefficients"""

    def __init__(self, points, tets, u, w, omega, order, c_tet=None, c_point=None, tris=None, c_tri=None, Y=0.0, flame=None, coeff=0.0):
        self.points = np.asarray(points, dtype=float)
        self.tets = np.asarray(tets, dtype=np.int64).reshape(-1, 4)
        self.tris = None if tris is None else np.asarray(tris, dtype=np.int64).reshape(-1, 3)
        self.order = {"lin": 1, "quad": 2}[order]
        self.np = len(self.points)
        self.c_tet = None if c_tet is None else np.asarray(c_tet, dtype=float)
        self.c_tri = None if c_tri is None else np.asarray(c_tri, dtype=float)
        self.c_point = None if c_point is None else np.asarray(c_point, dtype=float)
        assert self.c_point is None or (self.c_tet is None and self.c_tri is None)
        self.omega, self.Y, self.coeff = complex(omega), complex(Y), complex(coeff)
        self.flame = flame                      # dict(flame_tets, ref_tet, n_ref, nglobal_scaled[, x_ref])
        self.u, self.w = np.asarray(u, dtype=complex), np.asarray(w, dtype=complex)
        if self.order == 2:
            edges, _, _ = R.connectivity(self.np, self.tets)
            self.number = {(int(a), int(b)): self.np + k for k, (a, b) in enumerate(edges)}
            dim = self.np + len(edges)
        else:
            self.number, dim = None, self.np
        assert self.u.shape == (dim,) and self.w.shape == (dim,)

    def touching(self, p):
        tsel = np.nonzero((self.tets == p).any(axis=1))[0]
        ssel = np.zeros(0, dtype=np.int64) if self.tris is None else np.nonzero((self.tris == p).any(axis=1))[0]
        fsel = np.zeros(0, dtype=np.int64) if self.flame is None else np.intersect1d(np.asarray(self.flame["flame_tets"], dtype=np.int64), tsel)
        return tsel, ssel, fsel

    def dofs_of(self, sub_tets):
        """numbers, in the whole mesh, of the DoFs of the mesh made of sub_tets alone (which numbers its edges by itself)"""
        if self.order == 1:
            return np.arange(self.np)
        edges, _, _ = R.connectivity(self.np, sub_tets)
        return np.concatenate([np.arange(self.np), np.array([self.number[(int(a), int(b))] for a, b in edges], dtype=np.int64)])

    def local_nodes(self, corners):
        """DoFs of one simplex in local order: corners, then the edges in the order of _p2ref.local_edges"""
        corners = [int(x) for x in corners]
        if self.order == 1:
            return corners
        return corners + [self.number[(min(corners[i], corners[j]), max(corners[i], corners[j]))] for i, j in R.local_edges(len(corners))]


def _moved(points, p, crd, d):
    out = points.copy()
    out[p, crd] += d
    return out


# ---- float64, through the pinned references --------------------------------------------------------------------------------------------------
def _p1_boundary(points, tris, c_tri):
    """C = -i b,  b_ab = c |(x0-x2) x (x1-x2)| (1 + delta_ab)/24 on the 3-node triangles, dense bookkeeping by (rows, cols, values)"""
    rows, cols, vals = [], [], []
    for t, nodes in enumerate(tris):
        X = points[nodes]
        det = np.linalg.norm(np.cross(X[0] - X[2], X[1] - X[2]))
        rows.append(np.repeat(nodes, 3)); cols.append(np.tile(nodes, 3))
        vals.append(((1.0 if c_tri is None else float(c_tri[t])) * det * (1.0 + np.eye(3)) / 24.0).ravel())
    return np.concatenate(rows), np.concatenate(cols), -1j * np.concatenate(vals)


def _form(pb, A, dofs):
    """w^H A u for a matrix in the numbering `dofs` of a reduced mesh"""
    return np.vdot(pb.w[dofs], A @ pb.u[dofs])


def _flame_difference(pb, p, crd, h, fsel):
    """w^H (Q+ - Q-) u of the flame domain reduced to the tetrahedra fsel"""
    fl = pb.flame
    ref, n_ref, ngs = int(fl["ref_tet"]), np.asarray(fl["n_ref"], dtype=float), float(fl["nglobal_scaled"])
    plus, minus = _moved(pb.points, p, crd, +h), _moved(pb.points, p, crd, -h)
    if pb.order == 2:
        fsub = np.vstack([pb.tets[fsel], pb.tets[ref:ref + 1]])                        # the reduced flame domain and the reference tetrahedron
        Qp, _ = R.assemble_flame(plus, fsub, np.arange(len(fsel)), len(fsel), fl["x_ref"], n_ref, ngs)
        Qm, _ = R.assemble_flame(minus, fsub, np.arange(len(fsel)), len(fsel), fl["x_ref"], n_ref, ngs)
        return _form(pb, Qp - Qm, pb.dofs_of(fsub))

    def form(points):
        dets = np.array([abs(R.barycentric_gradients(points[pb.tets[t]])[1]) for t in fsel])
        G, _ = R.barycentric_gradients(points[pb.tets[ref]])
        g = -(ngs / (dets.sum() / 6.0)) * (G @ n_ref)
        return sum(det / 24.0 * np.conj(pb.w[pb.tets[t]]).sum() for t, det in zip(fsel, dets)) * np.dot(g, pb.u[pb.tets[ref]])
    return form(plus) - form(minus)


def _stacked_differences(pb, pts_chunk, h):
    """w^H (L+ - L-) u, L = om^2 M + K + om Y C, for every point of the chunk and every coordinate.  The reduced mesh of a point -- its
    simplices, with their own copy of their points -- is one piece; the pieces of all points and coordinates are laid side by side as ONE
    mesh of disjoint pieces, once with the points moved by +h and once by -h, and each of the two is assembled by one call of the pinned
    references per operator.  The two assemblies have the same pattern, so L+ - L- is formed entry by entry, as the reference forms
    D = (L+(om) - L-(om))/2h, and a piece's block is contracted with the entries of u and w that its points and edges have in the whole
    mesh.  Returns (len(pts_chunk), 3) complex."""
    Pp, Pm, T, S3, ct, cs, cp, gid, piece = [], [], [], [], [], [], [], [], []
    off = 0
    for k, p in enumerate(pts_chunk):
        tsel, ssel, _ = pb.touching(int(p))
        ids = np.unique(pb.tets[tsel])
        loc = {int(g): a for a, g in enumerate(ids)}
        lt = np.array([[loc[int(x)] for x in t] for t in pb.tets[tsel]], dtype=np.int64).reshape(-1, 4)
        ls = np.array([[loc[int(x)] for x in t] for t in pb.tris[ssel]], dtype=np.int64).reshape(-1, 3) if len(ssel) else np.zeros((0, 3), dtype=np.int64)
        for crd in range(3):
            for stack, d in ((Pp, h), (Pm, -h)):
                X = pb.points[ids].copy()
                X[loc[int(p)], crd] += d
                stack.append(X)
            T.append(lt + off); S3.append(ls + off)
            gid.append(ids); piece.append(np.full(len(ids), k * 3 + crd))
            if pb.c_tet is not None:
                ct.append(pb.c_tet[tsel])
            if pb.c_tri is not None:
                cs.append(pb.c_tri[ssel])
            if pb.c_point is not None:
                cp.append(pb.c_point[ids])
            off += len(ids)
    T, S3, gid, piece = np.vstack(T), np.vstack(S3), np.concatenate(gid), np.concatenate(piece)
    ct = np.concatenate(ct) if ct else None
    cs = np.concatenate(cs) if cs else None
    cp = np.concatenate(cp) if cp else None
    if pb.order == 2:                                                                   # the stacked mesh's edges, in the whole mesh's numbers
        edges, _, _ = R.connectivity(len(gid), T)
        ga, gb = gid[edges[:, 0]], gid[edges[:, 1]]
        dofs = np.concatenate([gid, np.array([pb.number[(min(a, b), max(a, b))] for a, b in zip(ga.tolist(), gb.tolist())], dtype=np.int64)])
        piece = np.concatenate([piece, piece[edges[:, 0]]])
    else:
        dofs = gid

    def operator(P):
        P = np.vstack(P)
        M, K = (R.assemble if pb.order == 2 else R.assemble_p1)(P, T, ct)
        if cp is not None:
            K = N.stiffness(P, T, cp, pb.order)
        L = pb.omega ** 2 * M + K
        if len(S3):
            if cp is not None:
                L = L + pb.omega * pb.Y * N.boundary(P, T, S3, cp, pb.order)
            elif pb.order == 2:
                L = L + pb.omega * pb.Y * R.assemble_boundary(P, T, S3, cs)
            else:
                r, c, v = _p1_boundary(P, S3, cs)
                L = L + pb.omega * pb.Y * sp.coo_matrix((v, (r, c)), shape=L.shape).tocsr()
        return L
    rows = np.conj(pb.w[dofs]) * ((operator(Pp) - operator(Pm)) @ pb.u[dofs])
    n = len(pts_chunk) * 3
    return (np.bincount(piece, weights=rows.real, minlength=n) + 1j * np.bincount(piece, weights=rows.imag, minlength=n)).reshape(-1, 3)


def sensitivity(pb, surface_points, h, chunk=64):
    """(3, len(surface_points)) complex, float64"""
    pts = np.asarray(surface_points, dtype=np.int64)
    diff = np.concatenate([_stacked_differences(pb, pts[i:i + chunk], h) for i in range(0, len(pts), chunk)])
    if pb.flame is not None:
        for k, p in enumerate(pts):
            _, _, fsel = pb.touching(int(p))
            if len(fsel):
                for crd in range(3):
                    diff[k, crd] += pb.coeff * _flame_difference(pb, p, crd, h, fsel)
    return (-diff / (2 * h)).T


# ---- extended precision --------------------------------------------------------------------------------------------------------------------
def _F(x):
    return Fraction(float(x))


def _cF(z):
    z = complex(z)
    return (_F(z.real), _F(z.imag))


def _cmul(a, b):
    return (a[0] * b[0] - a[1] * b[1], a[0] * b[1] + a[1] * b[0])


def _cadd(a, b):
    return (a[0] + b[0], a[1] + b[1])


def _cscale(a, s):
    return (a[0] * s, a[1] * s)


def _linear(p):
    """the four coefficients (re, im) of an affine complex polynomial in l_1..l_4 written as a linear form, using 1 = sum_k l_k"""
    out = []
    for k in range(4):
        e = tuple(1 if x == k else 0 for x in range(4))
        assert all(sum(x) <= 1 for q in p for x in q)
        out.append(tuple(q.get(e, Fraction(0)) + q.get((0, 0, 0, 0), Fraction(0)) for q in p))
    return out


def _exact_gradients(X):
    """(grad l_a (4 x 3 Fractions), det J) of the tetrahedron with corner rows X (Fractions), corner 4 the origin: inverse by cofactors"""
    J = [[X[a][r] - X[3][r] for a in range(3)] for r in range(3)]          # J[r][a]: column a = x_a - x_4
    cof = [[J[(r + 1) % 3][(a + 1) % 3] * J[(r + 2) % 3][(a + 2) % 3] - J[(r + 1) % 3][(a + 2) % 3] * J[(r + 2) % 3][(a + 1) % 3] for a in range(3)]
           for r in range(3)]
    det = sum(J[0][a] * cof[0][a] for a in range(3))
    G = [[cof[r][a] / det for r in range(3)] for a in range(3)]            # inverse = transposed cofactors / det: row a = grad l_a
    G.append([-(G[0][k] + G[1][k] + G[2][k]) for k in range(3)])
    return G, det


def _corners(pb, nodes, p, crd, d):
    X = [[_F(pb.points[n, k]) for k in range(3)] for n in nodes]
    for a, n in enumerate(nodes):
        if n == p:
            X[a][crd] += d
    return X


@functools.lru_cache(maxsize=None)
def _mass(nv, order):
    """int phi_a phi_b on the reference simplex, Fractions"""
    fs = N.functions(nv, order)
    return [[R._integral(R._mul(a, b), nv) for b in fs] for a in fs]


@functools.lru_cache(maxsize=None)
def _mass_l(order):
    """T[p][a][b] = int l_p phi_a phi_b on the reference triangle, Fractions"""
    fs = N.functions(3, order)
    return [[[R._integral(R._mul(R._mul(a, b), N._unit(3, p)), 3) for b in fs] for a in fs] for p in range(3)]


@functools.lru_cache(maxsize=None)
def _source(order):
    return [R._integral(f, 4) for f in N.functions(4, order)]


def _bilinear(A, w, u):
    """sum_ab conj(w_a) A_ab u_b for a real rational matrix and lists of (re, im) Fractions"""
    acc = (Fraction(0), Fraction(0))
    for a, row in enumerate(A):
        t = (sum(m * x[0] for m, x in zip(row, u)), sum(m * x[1] for m, x in zip(row, u)))
        acc = _cadd(acc, _cmul((w[a][0], -w[a][1]), t))
    return acc


def _exp2(xs):
    """the smallest e for which x 2^e is an integer for every float x"""
    return max([Fraction(float(x)).denominator.bit_length() - 1 for x in xs] + [0])


def _ints(xs, e):
    """the floats xs times 2^e as Python integers (exact)"""
    out = [Fraction(float(x)) * (1 << e) for x in xs]
    assert all(x.denominator == 1 for x in out)
    return [x.numerator for x in out]


@functools.lru_cache(maxsize=None)
def _dlin(order):
    """D[b][i][k]: d phi_b / d l_i is affine in l; with 1 = sum_k l_k it is the linear form sum_k D[b][i][k] l_k (integers)"""
    out = []
    for f in N.functions(4, order):
        rows = []
        for i in range(4):
            lin = _linear((R._diff(f, i), {}))
            assert all(x[0].denominator == 1 for x in lin)
            rows.append([x[0].numerator for x in lin])
        out.append(rows)
    return out


@functools.lru_cache(maxsize=None)
def _quartic():
    """Q[k][m][p][q] = 7! int l_k l_m l_p l_q on the reference tetrahedron (integers)"""
    l = [N._unit(4, i) for i in range(4)]
    out = [[[[R._integral(R._mul(R._mul(l[k], l[m]), R._mul(l[p], l[q])), 4) * 5040 for q in range(4)] for p in range(4)] for m in range(4)] for k in range(4)]
    assert all(x.denominator == 1 for a in out for b in a for c in b for x in c)
    return [[[[x.numerator for x in c] for c in b] for b in a] for a in out]


def _icmul(a, b):
    return (a[0] * b[0] - a[1] * b[1], a[0] * b[1] + a[1] * b[0])


class _TetForms:
    """geometry-free rational forms of one tetrahedron: mq = w^H Mhat u and S[i][j] = int c^2 conj(d_i w) (d_j u) with d_i = d/dl_i,
    so that  w^H M u = |det J| mq  and  w^H K u = -|det J| sum_ij S_ij grad l_i . grad l_j.  The floats are dyadic, so S is kept as
    integers S_int over one power-of-two-times-7! denominator DS: no greatest common divisors in the inner loops."""

    def __init__(self, pb, t):
        corners = pb.tets[t]
        nodes = pb.local_nodes(corners)
        uf, wf = pb.u[nodes], pb.w[nodes]
        self.mq = _bilinear(_mass(4, pb.order), [_cF(z) for z in wf], [_cF(z) for z in uf])
        self.src = functools.reduce(_cadd, [_cscale((_F(z.real), -_F(z.imag)), m) for z, m in zip(wf, _source(pb.order))])     # sum_a conj(w_a) int phi_a
        # c(x) = sum_p c_p l_p; a constant c is the case of four equal corner values (sum_p l_p = 1)
        c4 = pb.c_point[corners] if pb.c_point is not None else [1.0 if pb.c_tet is None else pb.c_tet[t]] * 4
        qc, qu = _exp2(c4), _exp2(list(uf.real) + list(uf.imag) + list(wf.real) + list(wf.imag))
        ci = _ints(c4, qc)
        u = list(zip(_ints(uf.real, qu), _ints(uf.imag, qu)))
        wc = list(zip(_ints(wf.real, qu), _ints(-wf.imag, qu)))                             # conj(w)
        Q, D = _quartic(), _dlin(pb.order)
        W = [[sum(ci[p] * ci[q] * Q[k][m][p][q] for p in range(4) for q in range(4)) for m in range(4)] for k in range(4)]      # 7! int c^2 l_k l_m
        au = [[(sum(D[b][i][k] * u[b][0] for b in range(len(nodes))), sum(D[b][i][k] * u[b][1] for b in range(len(nodes)))) for k in range(4)]
              for i in range(4)]
        aw = [[(sum(D[b][i][k] * wc[b][0] for b in range(len(nodes))), sum(D[b][i][k] * wc[b][1] for b in range(len(nodes)))) for k in range(4)]
              for i in range(4)]
        Z = [[(sum(W[k][m] * au[j][m][0] for m in range(4)), sum(W[k][m] * au[j][m][1] for m in range(4))) for k in range(4)] for j in range(4)]
        self.S_int = [[tuple(map(sum, zip(*[_icmul(aw[i][k], Z[j][k]) for k in range(4)]))) for j in range(4)] for i in range(4)]
        self.DS = 5040 << (2 * qc + 2 * qu)


def _int_cofactors(X):
    """for integer corner rows X: (c_a = det J * grad l_a as integer vectors, a = 1..4, and det J); corner 4 is the origin"""
    J = [[X[a][r] - X[3][r] for a in range(3)] for r in range(3)]
    cof = [[J[(r + 1) % 3][(a + 1) % 3] * J[(r + 2) % 3][(a + 2) % 3] - J[(r + 1) % 3][(a + 2) % 3] * J[(r + 2) % 3][(a + 1) % 3] for a in range(3)]
           for r in range(3)]
    det = sum(J[0][a] * cof[0][a] for a in range(3))
    c = [[cof[r][a] for r in range(3)] for a in range(3)]
    c.append([-(c[0][k] + c[1][k] + c[2][k]) for k in range(3)])
    return c, det


def _ref_gradient_form(pb, X, p, crd, d):
    """sum_b (grad phi_b(x_ref) . n_ref) u_b on the reference tetrahedron with p moved by d; x_ref stays where it is"""
    fl = pb.flame
    corners = pb.tets[int(fl["ref_tet"])]
    nodes = pb.local_nodes(corners)
    G, _ = _exact_gradients(X)
    n_ref = [_F(x) for x in fl["n_ref"]]
    gn = [sum(G[i][k] * n_ref[k] for k in range(3)) for i in range(4)]
    if pb.order == 2:
        xr = [_F(x) for x in fl["x_ref"]]
        lam = [sum(G[a][k] * (xr[k] - X[3][k]) for k in range(3)) for a in range(3)]
        lam.append(1 - sum(lam))
    else:
        lam = [Fraction(0)] * 4                                                            # the gradients are constant
    fs = N.functions(4, pb.order)
    acc = (Fraction(0), Fraction(0))
    for b, n in enumerate(nodes):
        gb = Fraction(0)
        for i in range(4):
            val = Fraction(0)
            for e, c in R._diff(fs[b], i).items():
                term = c
                for l, x in zip(lam, e):
                    term *= l ** x
                val += term
            gb += val * gn[i]
        acc = _cadd(acc, _cscale(_cF(pb.u[n]), gb))
    return acc


def _dec(c):
    return (Decimal(c[0].numerator) / Decimal(c[0].denominator), Decimal(c[1].numerator) / Decimal(c[1].denominator))


def sensitivity_ext(pb, surface_points, h):
    """(3, len(surface_points)) complex: the central difference of ``sensitivity`` evaluated exactly (one square root in 60 digits) and
    rounded once at the end"""
    hF = _F(h)
    om, Y, coeff = _cF(pb.omega), _cF(pb.Y), _cF(pb.coeff)
    om2, omY = _cmul(om, om), _cmul(om, Y)
    forms = functools.lru_cache(maxsize=None)(lambda t: _TetForms(pb, int(t)))
    om2mq = functools.lru_cache(maxsize=None)(lambda t: _cmul(om2, forms(t).mq))
    K0 = _exp2(list(pb.points.ravel()) + [h])
    ih = _ints([h], K0)[0]
    ipts = functools.lru_cache(maxsize=None)(lambda n: tuple(_ints(pb.points[n], K0)))
    out = np.zeros((3, len(surface_points)), dtype=complex)
    for k, p in enumerate(surface_points):
        p = int(p)
        tsel, ssel, fsel = pb.touching(p)
        tri_forms = []
        for s in ssel:                                                                      # w^H Bhat u, Bhat = int c phi_a phi_b
            corners = pb.tris[s]
            nodes = pb.local_nodes(corners)
            wl, ul = [_cF(pb.w[n]) for n in nodes], [_cF(pb.u[n]) for n in nodes]
            if pb.c_point is not None:
                T = _mass_l(pb.order)
                cc = [_F(pb.c_point[n]) for n in corners]
                B = [[sum(cc[q] * T[q][a][b] for q in range(3)) for b in range(len(nodes))] for a in range(len(nodes))]
            else:
                cval = _F(1.0 if pb.c_tri is None else pb.c_tri[s])
                B = [[cval * m for m in row] for row in _mass(3, pb.order)]
            tri_forms.append(_bilinear(B, wl, ul))
        for crd in range(3):
            rational = {}
            area = {}
            for sgn in (+1, -1):
                d = sgn * hF
                acc = (Fraction(0), Fraction(0))
                for t in tsel:                                                              # integers: coordinates times 2^K0
                    f = forms(int(t))
                    X = [list(ipts(int(n))) for n in pb.tets[t]]
                    for a, n in enumerate(pb.tets[t]):
                        if n == p:
                            X[a][crd] += sgn * ih
                    c, det = _int_cofactors(X)
                    adet = abs(det)                                                         # |det J| 2^(3 K0); c_a = det J grad l_a 2^(2 K0)
                    acc = _cadd(acc, _cscale(om2mq(int(t)), Fraction(adet, 1 << (3 * K0))))
                    nr = ni = 0
                    for i in range(4):
                        for j in range(4):
                            g = c[i][0] * c[j][0] + c[i][1] * c[j][1] + c[i][2] * c[j][2]
                            nr += f.S_int[i][j][0] * g
                            ni += f.S_int[i][j][1] * g
                    den = (f.DS * adet) << K0                                               # |det J| grad l_i . grad l_j = c_i . c_j / (|det J| 2^K0)
                    acc = (acc[0] - Fraction(nr, den), acc[1] - Fraction(ni, den))
                if len(fsel):
                    fl = pb.flame
                    a, vol = (Fraction(0), Fraction(0)), Fraction(0)
                    for t in fsel:
                        adet = abs(_exact_gradients(_corners(pb, pb.tets[t], p, crd, d))[1])
                        a = _cadd(a, _cscale(forms(int(t)).src, adet))
                        vol += adet / 6
                    gu = _ref_gradient_form(pb, _corners(pb, pb.tets[int(fl["ref_tet"])], p, crd, d), p, crd, d)
                    acc = _cadd(acc, _cmul(coeff, _cscale(_cmul(a, gu), -_F(fl["nglobal_scaled"]) / vol)))
                rational[sgn] = acc
                tot = (Decimal(0), Decimal(0))
                for s, bq in zip(ssel, tri_forms):
                    X = _corners(pb, pb.tris[s], p, crd, d)
                    e1, e2 = [X[0][x] - X[2][x] for x in range(3)], [X[1][x] - X[2][x] for x in range(3)]
                    n = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
                    nn = sum(x * x for x in n)
                    root = (Decimal(nn.numerator) / Decimal(nn.denominator)).sqrt()
                    z = _dec(_cmul(omY, _cmul((Fraction(0), Fraction(-1)), bq)))            # om Y (-i) w^H Bhat u
                    tot = (tot[0] + z[0] * root, tot[1] + z[1] * root)
                area[sgn] = tot
            diff = _dec((rational[+1][0] - rational[-1][0], rational[+1][1] - rational[-1][1]))
            two_h = Decimal(2) * Decimal(hF.numerator) / Decimal(hF.denominator)
            re = -(diff[0] + area[+1][0] - area[-1][0]) / two_h
            im = -(diff[1] + area[+1][1] - area[-1][1]) / two_h
            out[crd, k] = complex(float(re), float(im))
    return out


def yardstick(want64, want_ext):
    """e64 = max over points of |ref64 - ref_ext| / max|ref_ext of the point|: the float64 restatement's own rounding, the unit of the
    bounds of the GPU tests"""
    scale = np.abs(want_ext).max(axis=0)
    return float(np.max(np.abs(want64 - want_ext).max(axis=0) / scale))
