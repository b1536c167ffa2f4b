"""Test-only CPU reference of the Bloch unit cell with point and edge DoFs; shares no code with the product.

* ``blochify_loop``: `blochify` of src/Bloch.jl:4-112 as its literal loop over the triplets, on the reference's 1-based contiguous layout
  (naxis, nxbloch, nsector, naxis_ln, nsector_ln, N_points).
* ``numbering``: the cell numbering rule (include/waehip.h, "Bloch unit cells") with dictionaries and Python loops.
* ``fold``: an operator on the extended numbering -> its parts, by cell_dof and the flags.
* the six-point wedge, the reference-layout generator and the ring map of the annulus that the tests share.
"""
import numpy as np
import scipy.sparse as sp

# the wedge with an axis: a0, a1 on the axis; r0, r1 on the reference plane; i0, i1 their rotated images
WEDGE_TETS = np.array([[0, 1, 2, 4], [1, 2, 3, 4], [1, 3, 4, 5]], dtype=np.int32)
WEDGE = dict(npoints=6, nsector=4, naxis=2)
# not periodic: the first tetrahedron takes r1 instead of r0, so edge 02 is gone while image edge 04 stays and has no twin
WEDGE_BROKEN_TETS = np.array([[0, 1, 3, 4], [1, 2, 3, 4], [1, 3, 4, 5]], dtype=np.int32)


def blochify_loop(ii, jj, mm, naxis, nxbloch, nsector, naxis_ln, nsector_ln, N_points, axis=True):
    """1-based triplets -> (II, JJ, MM), each a tuple of 3 (naxis == 0) or 6 lists: base, plus, minus[, axis, axis plus, axis minus]"""
    shift, shift_ln = nsector - naxis, nsector_ln - naxis_ln
    II, JJ, MM = ([[] for _ in range(6)] for _ in range(3))
    for i, j, m in zip(ii, jj, mm):
        if i <= N_points:
            i_img = i > nsector
            if i_img:
                i -= shift
        else:
            i_img = i > nsector_ln
            if i_img:
                i -= shift_ln
        if j <= N_points:
            j_img = j > nsector
            if j_img:
                j -= shift
        else:
            j_img = j > nsector_ln
            if j_img:
                j -= shift_ln
        on_axis = axis and (i <= naxis or j <= naxis or N_points < i <= naxis_ln or N_points < j <= naxis_ln)
        if i > N_points:
            i -= nxbloch
        if j > N_points:
            j -= nxbloch
        if i_img == j_img:
            k = 0
        elif j_img:
            k = 1
        else:
            k = 2
        k += 3 if on_axis else 0
        II[k].append(i); JJ[k].append(j); MM[k].append(m)
    n = 3 if naxis == 0 else 6
    return tuple(II[:n]), tuple(JJ[:n]), tuple(MM[:n])


def loop_parts(A, lay, axis=True):
    """blochify_loop on a scipy matrix given on the 0-based extended numbering of layout ``lay`` -> tuple of CSR parts of dimension dim"""
    A = sp.coo_matrix(A)
    II, JJ, MM = blochify_loop((A.row + 1).tolist(), (A.col + 1).tolist(), A.data.tolist(), lay["naxis"], lay["nxbloch"], lay["nsector"],
                               lay["naxis_ln"], lay["nsector_ln"], lay["N_points"], axis=axis)
    d = lay["dim"]
    return tuple(_csr(np.array(M, dtype=complex), np.array(I, dtype=np.int64) - 1, np.array(J, dtype=np.int64) - 1, d) for I, J, M in zip(II, JJ, MM))


def _csr(v, i, j, d):
    M = sp.csr_matrix((v, (i, j)), shape=(d, d))
    M.sum_duplicates()
    M.sort_indices()
    return M


def reference_layout(naxis, nbody, nxbloch, nax_ln, nref_ln, nbody_ln):
    """A layout with the reference's contiguity.  Points: axis, reference plane (nxbloch), body, image (nxbloch).  Lines: axis lines, reference
    plane lines, body lines, image lines (as many as reference-plane lines).  Returns the 1-based layout numbers of blochify and the 0-based
    cell_dof / image / axis arrays the numbering rule gives for it (non-image lines keep their order behind the points)."""
    nsector = naxis + nxbloch + nbody
    N_points = nsector + nxbloch
    naxis_ln = N_points + nax_ln
    nsector_ln = naxis_ln + nref_ln + nbody_ln
    n_ext = nsector_ln + nref_ln
    d = np.arange(n_ext)
    point = d < N_points
    image = np.where(point, d >= nsector, d >= nsector_ln)
    axis = np.where(point, d < naxis, d < naxis_ln)
    cell = np.where(point, np.where(image, d - (nsector - naxis), d),
                    np.where(image, d - (nsector_ln - naxis_ln), d) - nxbloch)
    return dict(naxis=naxis, nxbloch=nxbloch, nsector=nsector, naxis_ln=naxis_ln, nsector_ln=nsector_ln, N_points=N_points, n_ext=n_ext,
                dim=nsector + nsector_ln - N_points, cell_dof=cell.astype(np.int32), image=image, axis=axis)


def numbering(npoints, tets, nsector, naxis=0, order="quad"):
    """The cell numbering rule in plain Python.  Returns a dict: cell_dof (int32), image, axis (bool), edges, twins {image edge: twin edge},
    dim, nedges, nimage_edges, naxis_edges.  ValueError where the library returns WAE_ERR_INVALID."""
    tets = np.asarray(tets, dtype=np.int64).reshape(-1, 4)
    if naxis > nsector or nsector > npoints or npoints - nsector > nsector - naxis:
        raise ValueError("bad point counts")
    if tets.min() < 0 or tets.max() >= npoints:
        raise ValueError("point index out of range")
    shift = nsector - naxis
    edges = []
    if order == "quad":
        edges = sorted({(min(t[a], t[b]), max(t[a], t[b])) for t in tets.tolist() for a in range(4) for b in range(a + 1, 4)})
    elif order != "lin":
        raise ValueError("order")
    index = {e: k for k, e in enumerate(edges)}
    is_img = lambda p: p >= nsector        # noqa: E731
    is_ax = lambda p: p < naxis            # noqa: E731
    image_edge = [all(is_img(p) or is_ax(p) for p in e) and any(is_img(p) for p in e) for e in edges]
    twins, missing = {}, 0
    for e, im in zip(edges, image_edge):
        if im:
            t = tuple(sorted(p - shift if is_img(p) else p for p in e))
            if t not in index:
                missing += 1
            elif image_edge[index[t]]:
                raise ValueError("a twin is an image edge")
            twins[e] = t
    if missing:
        raise ValueError(f"{missing} image edges without a twin")
    cell = [p - shift if is_img(p) else p for p in range(npoints)]
    own, count = {}, 0
    for e, im in zip(edges, image_edge):
        if not im:
            own[e] = nsector + count
            count += 1
    cell += [own[twins[e]] if im else own[e] for e, im in zip(edges, image_edge)]
    image = [is_img(p) for p in range(npoints)] + image_edge
    axis = [is_ax(p) for p in range(npoints)] + [is_ax(e[0]) and is_ax(e[1]) for e in edges]
    return dict(cell_dof=np.array(cell, dtype=np.int32), image=np.array(image, dtype=bool), axis=np.array(axis, dtype=bool),
                edges=np.array(edges, dtype=np.int32).reshape(-1, 2), twins=twins, dim=nsector + count, nedges=len(edges),
                nimage_edges=len(edges) - count, naxis_edges=int(sum(axis[npoints:])), naxis=naxis, nsector=nsector, npoints=npoints)


def fold(A, nb, axis=True):
    """A (scipy, extended numbering) -> tuple of CSR parts of dimension nb["dim"]: 3 if the cell has no axis DoF, else 6 (Bloch.jl:107-111;
    with axis=False the three axis parts stay empty)"""
    A = sp.coo_matrix(A)
    cell, image, ax = nb["cell_dof"].astype(np.int64), nb["image"], nb["axis"]
    i, j, v = A.row, A.col, A.data.astype(complex)
    part = np.where(image[i] == image[j], 0, np.where(image[j], 1, 2))
    if axis:
        part = part + 3 * (ax[i] | ax[j])
    n = 6 if ax.any() else 3
    return tuple(_csr(v[part == k], cell[i[part == k]], cell[j[part == k]], nb["dim"]) for k in range(n))


def bloch_matrix(parts, b, DOS):
    """base + exp(+2 pi i b/DOS) plus + exp(-2 pi i b/DOS) minus of one operator without axis DoFs"""
    assert len(parts) == 3
    ph = np.exp(2j * np.pi * b / DOS)
    return parts[0] + ph * parts[1] + parts[2] / ph


def annulus_ring_map(grid, DOS, nb, ring_edges):
    """ring DoF -> (cell DoF, sector) for the ring of DOS sectors of grid = (nthc, nz, nr) whose points are numbered plane by plane:
    written with a dictionary of the cell's edges, one ring edge at a time"""
    nthc, nz, nr = grid
    ns = nthc * nz * nr
    npc = ns + nz * nr
    number = {(int(u), int(v)): npc + k for k, (u, v) in enumerate(nb["edges"])}
    cell, sector = [], []
    for p in range(DOS * ns):
        cell.append(int(nb["cell_dof"][p % ns])); sector.append(p // ns)
    for u, v in np.asarray(ring_edges).tolist():
        su, sv = u // ns, v // ns
        if su == sv:
            s, lu, lv = su, u % ns, v % ns
        elif (su + 1) % DOS == sv:
            s, lu, lv = su, u % ns, ns + v % ns
        else:
            assert (sv + 1) % DOS == su
            s, lu, lv = sv, ns + u % ns, v % ns
        d = number[(min(lu, lv), max(lu, lv))]
        cell.append(int(nb["cell_dof"][d])); sector.append((s + 1) % DOS if nb["image"][d] else s)
    return np.array(cell), np.array(sector)


def expand(v, b, DOS, ring_cell, ring_sector):
    return v[ring_cell] * np.exp(2j * np.pi * b * ring_sector / DOS)
