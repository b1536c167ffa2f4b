"""Bloch-periodic operator families on the unit cell of a discrete-rotationally-symmetric domain (config C4).

Restates what the reference does when ``discretize`` meets a mesh with a degree of symmetry (``mesh.dos``):

* ``blochify`` (src/Bloch.jl:4-113) sorts the assembled triplets of every operator by whether the row / the column
  lies on the image boundary (the rotated copy of the reference boundary).  Image DoFs are folded onto their
  reference twins; entries that couple across the seam go to separate matrices that are later multiplied by the phase
  factors exp(±i·b·2π/DOS) (src/Helmholtz.jl:89-91,508-513), b being the Bloch wave number, a parameter of the family.
* DoFs on the symmetry axis (``naxis`` > 0) only carry the b = 0 wave: their entries go to three more matrices that
  are multiplied by the discrete delta filter δ(b) = (1/DOS)·Σ_k exp(2πi·k·b/DOS) (src/Helmholtz.jl:92-98), and a
  diagonal term (1-δ(b))·D pins them for b ≠ 0 (src/Helmholtz.jl:551-568).
* the auxiliary mass term -λ·M is the folded mass matrix WITHOUT phase factors (src/Helmholtz.jl:543-549; the
  reference's own TODO notes that).
* ``bloch_expand`` (src/Bloch.jl:118-143) unfolds a unit-cell vector onto the full ring.

P1 point DoFs fold by a constant index shift (``blochify``, host scipy).  The line DoFs of the quadratic element order
(P2) have no such shift here -- the edges are numbered by sorted point pairs, not in the reference's generator order -- so
their twins are found: ``bloch_numbering`` numbers the cell DoFs on the device (wae_bloch_numbering) and
``blochify_device`` folds an operator by that numbering (wae_bloch_fold: sorted triplets, no atomics); with
``order="lin"`` the same path serves P1.  Hermite elements are not handled.  The device sees the result as an ordinary
multi-term family whose coefficients depend on (ω, b, ...).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import scipy.sparse as sp

from .. import _lib
from ..nlevp.algebra import (exp_delay, generate_1_gz, generate_exp_az, generate_gz_hz, generate_Sigma_y_exp_ikx, pow1,
                             pow2)
from ..nlevp.linopfam import LinearOperatorFamily, Term

SUFFIXES = ("", "+", "-", "δ", "δ+", "δ-")


def blochify(A, nsector, naxis=0, axis=True):
    """Split one operator assembled on the extended numbering (image DoFs = indices >= nsector, 0-based) into the
    (base, plus, minus[, axis, axis_plus, axis_minus]) matrices of dimension nsector.  src/Bloch.jl:4-113."""
    A = sp.coo_matrix(A)
    A.sum_duplicates()
    shift = nsector - naxis
    i, j, v = A.row.astype(np.int64), A.col.astype(np.int64), A.data.astype(complex)
    i_img, j_img = i >= nsector, j >= nsector
    i = np.where(i_img, i - shift, i)
    j = np.where(j_img, j - shift, j)
    on_axis = ((i < naxis) | (j < naxis)) if (axis and naxis > 0) else np.zeros(len(i), dtype=bool)
    same = i_img == j_img
    plus = ~i_img & j_img
    minus = i_img & ~j_img
    out = []
    for ax in ((False, True) if naxis > 0 else (False,)):
        for sel in (same, plus, minus):
            m = sel & (on_axis == ax)
            out.append(sp.csr_matrix((v[m], (i[m], j[m])), shape=(nsector, nsector)))
    for M in out:
        M.sum_duplicates()
        M.sort_indices()
    return tuple(out)


def phase_functions(DOS):
    """exp_plus, exp_minus, bloch_filt, anti_bloch_filt, bloch_exp_plus, bloch_exp_minus -- src/Helmholtz.jl:89-98."""
    dphi = 2 * np.pi / DOS

    exp_plus = generate_exp_az(1j * dphi)        # = exp_az(z, Δϕ·i, k), written so that operator files can name it
    exp_minus = generate_exp_az(-1j * dphi)
    y = np.zeros(DOS, dtype=complex)
    y[0] = 1.0 / DOS
    bloch_filt = generate_Sigma_y_exp_ikx(np.fft.fft(y))
    return {
        "exp_plus": exp_plus, "exp_minus": exp_minus, "bloch_filt": bloch_filt,
        "anti_bloch_filt": generate_1_gz(bloch_filt),
        "bloch_exp_plus": generate_gz_hz(bloch_filt, exp_plus),
        "bloch_exp_minus": generate_gz_hz(bloch_filt, exp_minus),
    }


class BlochNumbering:
    """Cell numbering of an extended unit-cell mesh (``bloch_numbering``): per extended DoF (points, then the P2 edges) ``cell_dof``
    (int32) and the flag arrays ``image`` / ``axis`` (bool; ``flags`` holds the bits), ``edges`` (nedges, 2), ``dim`` and the counts."""

    def __init__(self, npoints, nsector, naxis, order, cell_dof, flags, edges, dim, nimage_edges, naxis_edges):
        self.npoints, self.nsector, self.naxis, self.order = int(npoints), int(nsector), int(naxis), order
        self.cell_dof = np.ascontiguousarray(cell_dof, dtype=np.int32)
        self.flags = np.ascontiguousarray(flags, dtype=np.int32)
        self.edges = np.ascontiguousarray(edges, dtype=np.int32).reshape(-1, 2)
        self.dim, self.nimage_edges, self.naxis_edges = int(dim), int(nimage_edges), int(naxis_edges)

    image = property(lambda self: (self.flags & _lib.BLOCH_IMAGE) != 0)
    axis = property(lambda self: (self.flags & _lib.BLOCH_AXIS) != 0)
    nedges = property(lambda self: self.edges.shape[0])
    ndof = property(lambda self: self.cell_dof.shape[0])

    def axis_cell_dofs(self):
        """cell DoFs that carry only the b = 0 wave: the axis points and the axis edges, ascending"""
        return np.unique(self.cell_dof[self.axis])


_ORDERS = {"lin": 1, "quad": 2}


def bloch_numbering(npoints, tets, nsector, naxis=0, order="quad", device=0):
    """Number the DoFs of a Bloch unit cell on the device (wae_bloch_numbering).  ``tets`` (ntets, 4), 0-based, is the EXTENDED cell
    mesh: points < naxis on the symmetry axis, points >= nsector image points whose twin is p - (nsector - naxis).  Edge DoFs as in
    ``p2_connectivity``; an edge whose endpoints are all image or axis points (one image point at least) is an image edge and takes the
    cell DoF of its twin, which is searched in the sorted edge list; the others are renumbered densely after the points.  ``order``:
    "quad" (P2) or "lin" (no edges: the point rule alone)."""
    order = str(order)
    if order not in _ORDERS:
        raise ValueError(f"order must be 'lin' or 'quad', not {order!r}")
    tt = np.ascontiguousarray(tets, dtype=np.int32).reshape(-1, 4)
    L = _lib.lib()
    ip, lp = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    h = C.c_void_p()
    _lib.check(L.wae_bloch_numbering(int(device), int(npoints), tt.shape[0], tt.ctypes.data_as(ip), int(nsector), int(naxis), _ORDERS[order],
                                     C.byref(h)))
    try:
        nd, dim, ne, ni, na = (C.c_int64(0) for _ in range(5))
        _lib.check(L.wae_bloch_numbering_info(h, C.byref(nd), C.byref(dim), C.byref(ne), C.byref(ni), C.byref(na)))
        cell = np.zeros(nd.value, dtype=np.int32)
        flags = np.zeros(nd.value, dtype=np.int32)
        edges = np.zeros((ne.value, 2), dtype=np.int32)
        _lib.check(L.wae_bloch_numbering_get(h, cell.ctypes.data_as(ip), flags.ctypes.data_as(ip), edges.ctypes.data_as(ip)))
    finally:
        L.wae_bloch_numbering_free(h)
    return BlochNumbering(npoints, nsector, naxis, order, cell, flags, edges, dim.value, ni.value, na.value)


def _real_streams(A):
    """the real value streams of a CSR matrix: [re] or [re, im]"""
    if np.iscomplexobj(A.data) and np.any(A.data.imag):
        return [np.ascontiguousarray(A.data.real), np.ascontiguousarray(A.data.imag)]
    return [np.ascontiguousarray(A.data.real, dtype=np.float64)]


def _fold_streams(rowptr, col, streams, numbering, nparts, device):
    """wae_bloch_fold on one pattern with any number of real value streams (two per call) -> (patterns [(rowptr, col)] per part, values
    [stream][part])"""
    L = _lib.lib()
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    n = len(rowptr) - 1
    pats, vals = None, []
    for s0 in range(0, len(streams), 2):
        pair = streams[s0:s0 + 2]
        hs = (C.c_void_p * nparts)()
        _lib.check(L.wae_bloch_fold(int(device), n, rowptr.ctypes.data_as(ip), col.ctypes.data_as(ip), pair[0].ctypes.data_as(dp),
                                    pair[1].ctypes.data_as(dp) if len(pair) > 1 else None, numbering.cell_dof.ctypes.data_as(ip),
                                    numbering.flags.ctypes.data_as(ip), numbering.dim, nparts, hs))
        got = [[] for _ in pair]
        new_pats = []
        try:
            for p in range(nparts):
                h = C.c_void_p(hs[p])
                d, nnz = C.c_int64(0), C.c_int64(0)
                _lib.check(L.wae_p1_info(h, C.byref(d), C.byref(nnz)))
                rp = np.zeros(d.value + 1, dtype=np.int32)
                cc = np.zeros(nnz.value, dtype=np.int32)
                a = np.zeros(nnz.value, dtype=np.float64)
                b = np.zeros(nnz.value, dtype=np.float64)
                _lib.check(L.wae_p1_get(h, rp.ctypes.data_as(ip), cc.ctypes.data_as(ip), a.ctypes.data_as(dp), b.ctypes.data_as(dp)))
                new_pats.append((rp, cc))
                got[0].append(a)
                if len(pair) > 1:
                    got[1].append(b)
        finally:
            for p in range(nparts):
                L.wae_p1_free(C.c_void_p(hs[p]))
        pats = pats or new_pats
        vals += got
    return pats, vals


def blochify_device(A, numbering, axis=True, device=0):
    """``blochify`` on the device, by the cell numbering of ``bloch_numbering`` (points and P2 edges): the tuple of scipy CSR parts
    (base, plus, minus[, axis, axis_plus, axis_minus]) of dimension ``numbering.dim`` -- six if ``axis`` and the cell has axis points,
    else three.  ``A``: a scipy matrix on the extended numbering, or an (M, K) pair sharing one pattern (folded in one pass; returns
    the pair of tuples).  Complex values are split into real streams for the device, as in the assembly wrappers."""
    pair = isinstance(A, (tuple, list))
    mats = [sp.csr_matrix(X) for X in (A if pair else (A,))]
    n = numbering.ndof
    for X in mats:
        if X.shape[0] != X.shape[1]:
            raise ValueError(f"blochify_device needs a square matrix, got {X.shape}")
        if X.shape[0] != n:
            raise ValueError(f"the numbering has {n} DoFs, the matrix {X.shape[0]} rows")
    if pair and (len(mats) != 2 or mats[0].nnz != mats[1].nnz or not (np.array_equal(mats[0].indptr, mats[1].indptr)
                                                                    and np.array_equal(mats[0].indices, mats[1].indices))):
        raise ValueError("an (M, K) pair must be two matrices with one sparsity pattern")
    nparts = 6 if (axis and numbering.naxis > 0) else 3
    rowptr = np.ascontiguousarray(mats[0].indptr, dtype=np.int32)
    col = np.ascontiguousarray(mats[0].indices, dtype=np.int32)
    streams, owner = [], []
    for X in mats:
        st = _real_streams(X)
        streams += st
        owner.append(len(st))
    pats, vals = _fold_streams(rowptr, col, streams, numbering, nparts, device)
    out, k = [], 0
    for cnt in owner:
        parts = []
        for p, (rp, cc) in enumerate(pats):
            v = vals[k][p].astype(complex) if cnt == 1 else vals[k][p] + 1j * vals[k + 1][p]
            parts.append(sp.csr_matrix((v, cc.copy(), rp.copy()), shape=(numbering.dim, numbering.dim)))
        out.append(tuple(parts))
        k += cnt
    return tuple(out) if pair else out[0]


def bloch_terms(terms_ext, nsector, DOS, naxis=0, b="b", flame=True, numbering=None, device=0):
    """Term list of the Bloch family in the reference's push order: for every operator its base / plus / minus
    (/ axis) parts (src/Helmholtz.jl:508-513), then D (if there is an axis), then the auxiliary mass term last.
    With a ``numbering`` (``bloch_numbering``: P2 cells, or P1 through the same path) the parts come from ``blochify_device`` and D covers
    the axis points and the axis edges (Helmholtz.jl:551-567)."""
    pf = phase_functions(DOS)
    extra = [((), ()), ((pf["exp_plus"],), ((b,),)), ((pf["exp_minus"],), ((b,),)),
             ((pf["bloch_filt"],), ((b,),)), ((pf["bloch_exp_plus"],), ((b,),)), ((pf["bloch_exp_minus"],), ((b,),))]
    ops = [("M", (pow2,), (("ω",),), "ω^2"), ("K", (), (), ""), ("C", (pow1, pow1), (("ω",), ("Y",)), "ω*Y")]
    if flame and "Q" in terms_ext:
        ops.append(("Q", (pow1, exp_delay), (("n",), ("ω", "τ")), "n*exp(-iωτ)"))
    if numbering is None:
        dim, axis_idx = nsector, np.arange(naxis)

        def fold(A, axis=True):
            return blochify(A, nsector, naxis, axis)
    else:
        if (numbering.nsector, numbering.naxis) != (nsector, naxis):
            raise ValueError(f"the numbering was made for nsector, naxis = {numbering.nsector}, {numbering.naxis}, not {nsector}, {naxis}")
        dim, axis_idx = numbering.dim, numbering.axis_cell_dofs()

        def fold(A, axis=True):
            return blochify_device(A, numbering, axis, device)
    out = []
    for name, func, arg, txt in ops:
        for part, (f, a), suf in zip(fold(terms_ext[name]), extra, SUFFIXES):
            if part.nnz:
                out.append(Term(part, (*func, *f), (*arg, *a), txt + suf, name))
    Mparts = fold(terms_ext["M"], axis=False)
    Mfold = sp.csr_matrix(Mparts[0] + Mparts[1] + Mparts[2])
    if naxis > 0:
        dv = 1.0 / (-Mfold.diagonal()[axis_idx])            # DV = 1/M[idx,idx] with M = -mass  (Helmholtz.jl:549,558-560)
        D = sp.csr_matrix((dv, (axis_idx, axis_idx)), shape=(dim, dim), dtype=complex)
        out.append(Term(D, (pf["anti_bloch_filt"],), ((b,),), "(1-δ(b))", "D"))
    out.append(Term(-Mfold, (pow1,), (("λ",),), "-λ", "__aux__"))
    return out


def bloch_family(cell, b=0, device=0, flame=True, b_symbol="b", numbering=None):
    """Device-backed family of a unit cell produced by annulus.build_unit_cell (or any dict with terms_ext, nsector,
    DOS, params[, naxis]).  ``L.params['b']`` is the Bloch wave number; change it freely between solves -- only the
    scalar coefficients change, the device copy of the matrices and the multigrid hierarchy are reused.
    ``numbering`` (default: ``cell["numbering"]`` if the cell carries one, as annulus.build_unit_cell_p2's does): fold by the device
    numbering of ``bloch_numbering`` -- required for P2 cells."""
    L = LinearOperatorFamily(["ω", "λ"], [0.0, complex(np.inf, 0)], device=device)
    L.symmetry_tol = 1e-14          # (the base parts of M, K, C are symmetric to assembly rounding; helmholtz/family.py)
    p = cell["params"]
    L.params["Y"] = complex(p["Y"])
    if flame:
        L.params["n"] = complex(p["n"])
        L.params["τ"] = complex(p["τ"])
    if numbering is None:
        numbering = cell.get("numbering")
    for T in bloch_terms(cell["terms_ext"], cell["nsector"], cell["DOS"], cell.get("naxis", 0), b_symbol, flame, numbering, device):
        L.push(T)
    L.params[b_symbol] = complex(b)
    return L


def seam_terms(L):
    """indices of the seam parts (the "+"/"-" terms) of a Bloch family.  ``L.solver_opts["shape_exclude"] = seam_terms(L)``
    keeps them out of the multigrid shape matrix, so that no aggregate spans the seam: measured at C4 (d = 200 000,
    DOS = 32) this halves the iterations for wave numbers near DOS/2 (b = 16: 53 -> 26, b = 5: 60 -> 50), where the
    solution is close to antiperiodic, and quadruples them near b = 0 (21 -> 93, b = 1: 34 -> 91), where it is smooth
    across the seam -- hence off by default; one hierarchy serves a whole sweep."""
    return [k for k, t in enumerate(L.terms) if t.symbol.endswith(("+", "-")) and t.operator != "__aux__"]


def bloch_expand(v, b, DOS, nxsector=None, naxis=0):
    """Unit-cell vector -> vector on the full ring: sector s carries v·exp(+2πi·b·s/DOS); axis DoFs are copied once.
    src/Bloch.jl:118-143."""
    v = np.asarray(v)
    if nxsector is None:
        nxsector = v.shape[0] - naxis
    out = np.zeros((naxis + nxsector * DOS,) + v.shape[1:], dtype=complex)
    out[:naxis] = v[:naxis]
    for s in range(DOS):
        out[naxis + s * nxsector:naxis + (s + 1) * nxsector] = v[naxis:naxis + nxsector] * np.exp(2j * np.pi / DOS * b * s)
    return out


def bloch_expand_dofs(v, b, DOS, ring_cell_dof, ring_sector):
    """``bloch_expand`` for any DoF layout: ring DoF k carries v[ring_cell_dof[k]]·exp(+2πi·b·ring_sector[k]/DOS).  The two maps come
    with the ring (annulus.ring_cell_map for P2: edges have no contiguous per-sector blocks); axis DoFs have sector 0."""
    v = np.asarray(v)
    ph = np.exp(2j * np.pi / DOS * b * np.asarray(ring_sector))
    return v[np.asarray(ring_cell_dof)] * ph.reshape((-1,) + (1,) * (v.ndim - 1))
