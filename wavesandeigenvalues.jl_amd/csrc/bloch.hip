// Bloch unit cells on the device: the numbering of the cell DoFs (points and P2 edges) and the fold of an operator assembled on the
// extended numbering into its base / plus / minus (/ axis) parts -- `blochify` of the reference (src/Bloch.jl:4-112) with
// Helmholtz.jl:107-113 for the dimension.
//
//   1. Numbering.  Points < naxis lie on the symmetry axis, points >= nsector are image points, the twin of image point p is
//      p - (nsector - naxis).  The edges are those of assemble_p2.hip (sorted by (smaller point, larger point), DoF of edge e = npoints + e).
//      An edge is an image edge if every endpoint is an image or an axis point and at least one is an image point; its twin is the edge
//      with the image endpoints shifted, found by binary search in the sorted keys, one thread per edge.  The other edges are numbered
//      nsector + (number of non-image edges before them) by an exclusive scan (hipCUB); image DoFs take the cell DoF of their twin.
//   2. Fold.  One thread per stored entry (i, j) of the CSR input: I = cell_dof[i], J = cell_dof[j], part = base / plus / minus by the
//      image bits of i and j (+3 if an axis bit is set and the axis parts are asked for), key = (part * dim + I) * (nparts * dim) + J.
//      triplets_to_csr (assemble.hip) sorts all parts at once (stable radix sort), sums the duplicates that folding creates in input
//      order (reduce-by-key) -- no atomics, the same bits on every call -- and returns one CSR of nparts * dim rows, which the host cuts
//      into the parts.
#include <climits>
#include <memory>
#include <vector>

#include "edge_keys.h"
#include "mesh_host.h"

namespace {

typedef unsigned long long u64;

struct BlochNumbering {
    int64_t npoints = 0, ndof = 0, dim = 0, nedges = 0, nimage_edges = 0, naxis_edges = 0;
    std::vector<int> cell_dof, flags, edges;
};

// one thread per edge: its two points, whether it is an image / an axis edge, and the position of its twin in the sorted list.
// keep[e] = 1 for an edge that gets a cell DoF of its own; twin[e] = -1: no image edge, -2: twin missing, -3: the twin is an image edge itself
__global__ __launch_bounds__(256) void bloch_edge_kernel(const u64 *__restrict__ ek, int64_t ne, u64 np, int nsector, int naxis, int *__restrict__ edges,
                                                         int *__restrict__ keep, int *__restrict__ twin, int *__restrict__ eflags,
                                                         int *__restrict__ nmissing, int *__restrict__ nimgtwin, int *__restrict__ nax) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < ne; e += (int64_t)gridDim.x * 256) {
        const u64 k = ek[e], lo = k / np;
        const int u = (int)lo, v = (int)(k - lo * np);
        edges[e * 2] = u;
        edges[e * 2 + 1] = v;
        const bool iu = u >= nsector, iv = v >= nsector, au = u < naxis, av = v < naxis;
        const bool image = (iu || au) && (iv || av) && (iu || iv);
        const bool axis = au && av;
        int t = -1, missing = 0, imgtwin = 0;
        if (image) {
            const int shift = nsector - naxis;
            const int tu = iu ? u - shift : u, tv = iv ? v - shift : v;
            t = p2_find_edge(ek, ne, np, tu, tv);
            if (t < 0) { t = -2; missing = 1; }
            else if (tu >= nsector || tv >= nsector) { t = -3; imgtwin = 1; }          // (cannot happen once the point counts are checked)
        }
        keep[e] = image ? 0 : 1;
        twin[e] = t;
        eflags[e] = (image ? WAE_BLOCH_IMAGE : 0) | (axis ? WAE_BLOCH_AXIS : 0);
        nmissing[e] = missing;
        nimgtwin[e] = imgtwin;
        nax[e] = axis ? 1 : 0;
    }
}

// one thread per extended DoF: points by the point rule, edges from the scan of keep (rank = number of non-image edges before an edge)
__global__ __launch_bounds__(256) void bloch_number_kernel(int64_t npoints, int64_t ne, int nsector, int naxis, const int *__restrict__ rank,
                                                           const int *__restrict__ twin, const int *__restrict__ eflags,
                                                           int *__restrict__ cell_dof, int *__restrict__ flags) {
    const int64_t n = npoints + ne;
    for (int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x; d < n; d += (int64_t)gridDim.x * 256) {
        if (d < npoints) {
            const bool image = d >= nsector;
            cell_dof[d] = image ? (int)d - (nsector - naxis) : (int)d;
            flags[d] = (image ? WAE_BLOCH_IMAGE : 0) | (d < naxis ? WAE_BLOCH_AXIS : 0);
        } else {
            const int64_t e = d - npoints;
            const int t = twin[e];
            cell_dof[d] = nsector + rank[t >= 0 ? t : e];
            flags[d] = eflags[e];
        }
    }
}

// row index of every stored entry of a CSR matrix, one thread per row
__global__ __launch_bounds__(256) void bloch_expand_rows_kernel(const int *__restrict__ rowptr, int64_t n, int *__restrict__ rowidx) {
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (int64_t)gridDim.x * 256)
        for (int e = rowptr[r]; e < rowptr[r + 1]; ++e) rowidx[e] = (int)r;
}

// key of every stored entry: (part * dim + I) * (nparts * dim) + J
__global__ __launch_bounds__(256) void bloch_fold_keys_kernel(const int *__restrict__ rowidx, const int *__restrict__ col, size_t nnz,
                                                              const int *__restrict__ cell_dof, const int *__restrict__ flags, u64 dim, int nparts,
                                                              u64 *__restrict__ keys) {
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < nnz; e += (size_t)gridDim.x * 256) {
        const int i = rowidx[e], j = col[e];
        const int fi = flags[i], fj = flags[j];
        const bool ii = fi & WAE_BLOCH_IMAGE, ij = fj & WAE_BLOCH_IMAGE;
        int part = ii == ij ? 0 : (ij ? 1 : 2);
        if (nparts == 6 && ((fi | fj) & WAE_BLOCH_AXIS)) part += 3;
        keys[e] = ((u64)part * dim + (u64)cell_dof[i]) * ((u64)nparts * dim) + (u64)cell_dof[j];
    }
}

}  // namespace

extern "C" {

int wae_bloch_numbering(int32_t device, int64_t npoints, int64_t ntets, const int32_t *tets, int64_t nsector, int64_t naxis, int32_t order, void **out) {
    return wae_guarded([&]() {
        if (!out) throw WaeError(WAE_ERR_INVALID, "bad argument");
        if (order != 1 && order != 2) throw WaeError(WAE_ERR_INVALID, "order must be 1 (lin) or 2 (quad)");
        p2_check_tets(npoints, ntets, tets);
        if (naxis < 0 || naxis > nsector) throw WaeError(WAE_ERR_INVALID, "naxis must lie in 0..nsector");
        if (nsector > npoints) throw WaeError(WAE_ERR_INVALID, "nsector exceeds the number of points");
        if (npoints - nsector > nsector - naxis)
            throw WaeError(WAE_ERR_INVALID, "more image points (" + std::to_string(npoints - nsector) + ") than points off the axis (" +
                                                std::to_string(nsector - naxis) + "): an image point would have no twin");
        HIP_CHECK(hipSetDevice(device));
        std::unique_ptr<BlochNumbering> H(new BlochNumbering);
        H->npoints = npoints;
        Dev<int> dtets(tets, order == 2 ? (size_t)ntets * 4 : 0);
        Dev<u64> ek((size_t)ntets * 6);
        int64_t ne = 0;
        if (order == 2) {
            ne = p2_edge_list(npoints, ntets, dtets.p, ek);                 // (checks npoints + nedges <= INT_MAX)
        }
        const int64_t ndof = npoints + ne;
        Dev<int> edges((size_t)ne * 2), keep((size_t)ne), rank((size_t)ne), twin((size_t)ne), eflags((size_t)ne), cnt((size_t)ne * 3);
        Dev<int> cell((size_t)ndof), flags((size_t)ndof);
        int nkeep = 0;
        if (ne > 0) {
            hipLaunchKernelGGL(bloch_edge_kernel, grid_for((size_t)ne, GRID_STRIDE_CAP), dim3(256), 0, 0, ek.p, ne, (u64)npoints, (int)nsector, (int)naxis, edges.p,
                               keep.p, twin.p, eflags.p, cnt.p, cnt.p + ne, cnt.p + 2 * ne);
            HIP_CHECK(hipGetLastError());
            const int nmissing = device_sum(cnt.p, (int)ne), nimgtwin = device_sum(cnt.p + ne, (int)ne);
            if (nmissing)
                throw WaeError(WAE_ERR_INVALID, "the cell is not periodic: " + std::to_string(nmissing) + " image edge(s) whose twin is no edge of the mesh");
            if (nimgtwin) throw WaeError(WAE_ERR_INVALID, std::to_string(nimgtwin) + " image edge(s) whose twin is an image edge itself");
            H->naxis_edges = device_sum(cnt.p + 2 * ne, (int)ne);
            DevBuf<char> tmp;
            exclusive_sum(keep.p, rank.p, (int)ne, tmp);
            nkeep = device_sum(keep.p, (int)ne);
        }
        hipLaunchKernelGGL(bloch_number_kernel, grid_for((size_t)ndof, GRID_STRIDE_CAP), dim3(256), 0, 0, npoints, ne, (int)nsector, (int)naxis, rank.p, twin.p,
                           eflags.p, cell.p, flags.p);
        HIP_CHECK(hipGetLastError());
        H->ndof = ndof; H->nedges = ne; H->nimage_edges = ne - nkeep; H->dim = nsector + nkeep;
        H->cell_dof.resize((size_t)ndof); H->flags.resize((size_t)ndof); H->edges.resize((size_t)ne * 2);
        cell.to_host(H->cell_dof.data(), (size_t)ndof);
        flags.to_host(H->flags.data(), (size_t)ndof);
        edges.to_host(H->edges.data(), (size_t)ne * 2);
        *out = H.release();
        return WAE_OK;
    });
}

int wae_bloch_numbering_info(const void *handle, int64_t *ndof, int64_t *dim, int64_t *nedges, int64_t *nimage_edges, int64_t *naxis_edges) {
    return wae_guarded([&]() {
        if (!handle) throw WaeError(WAE_ERR_INVALID, "null handle");
        const BlochNumbering *H = (const BlochNumbering *)handle;
        if (ndof) *ndof = H->ndof;
        if (dim) *dim = H->dim;
        if (nedges) *nedges = H->nedges;
        if (nimage_edges) *nimage_edges = H->nimage_edges;
        if (naxis_edges) *naxis_edges = H->naxis_edges;
        return WAE_OK;
    });
}

int wae_bloch_numbering_get(const void *handle, int32_t *cell_dof, int32_t *flags, int32_t *edges) {
    return wae_guarded([&]() {
        if (!handle) throw WaeError(WAE_ERR_INVALID, "null handle");
        const BlochNumbering *H = (const BlochNumbering *)handle;
        if (cell_dof) memcpy(cell_dof, H->cell_dof.data(), H->cell_dof.size() * sizeof(int));
        if (flags) memcpy(flags, H->flags.data(), H->flags.size() * sizeof(int));
        if (edges) memcpy(edges, H->edges.data(), H->edges.size() * sizeof(int));
        return WAE_OK;
    });
}

int wae_bloch_numbering_free(void *handle) {
    delete (BlochNumbering *)handle;
    return WAE_OK;
}

int wae_bloch_fold(int32_t device, int64_t n, const int32_t *rowptr, const int32_t *col, const double *v0, const double *v1, const int32_t *cell_dof,
                   const int32_t *flags, int64_t dim, int32_t nparts, void **out) {
    return wae_guarded([&]() {
        if (!(n > 0 && rowptr && cell_dof && flags && v0 && out)) throw WaeError(WAE_ERR_INVALID, "bad argument");
        if (nparts != 3 && nparts != 6) throw WaeError(WAE_ERR_INVALID, "nparts must be 3 or 6");
        if (n > INT_MAX || dim <= 0 || dim > n || dim * nparts > INT_MAX)
            throw WaeError(WAE_ERR_INVALID, "dim must lie in 1..n, and n and nparts * dim must fit a 32-bit index");
        if (rowptr[0] != 0) throw WaeError(WAE_ERR_INVALID, "rowptr does not start at 0");
        for (int64_t r = 0; r < n; ++r)
            if (rowptr[r + 1] < rowptr[r]) throw WaeError(WAE_ERR_INVALID, "rowptr decreases");
        const size_t nnz = (size_t)rowptr[n];
        if (nnz && !col) throw WaeError(WAE_ERR_INVALID, "bad argument");
        check_indices(col, (int64_t)nnz, n, "column index outside 0..n-1");
        for (int64_t d = 0; d < n; ++d) {
            if (cell_dof[d] < 0 || cell_dof[d] >= dim) throw WaeError(WAE_ERR_INVALID, "cell_dof holds an index outside 0..dim-1");
            if (flags[d] & ~(WAE_BLOCH_IMAGE | WAE_BLOCH_AXIS)) throw WaeError(WAE_ERR_INVALID, "flags holds an unknown bit");
        }
        std::vector<std::unique_ptr<P1Handle>> parts;
        for (int p = 0; p < nparts; ++p) {
            parts.emplace_back(new P1Handle);
            parts.back()->np = dim;
            parts.back()->rowptr.assign((size_t)dim + 1, 0);
        }
        if (nnz) {
            HIP_CHECK(hipSetDevice(device));
            Dev<int> drow(rowptr, (size_t)n + 1), dcol(col, nnz), didx(nnz), dcell(cell_dof, (size_t)n), dflags(flags, (size_t)n);
            Dev<double> a(v0, nnz), b(v1, v1 ? nnz : 0);
            Dev<u64> keys(nnz);
            hipLaunchKernelGGL(bloch_expand_rows_kernel, grid_for((size_t)n, GRID_STRIDE_CAP), dim3(256), 0, 0, drow.p, n, didx.p);
            hipLaunchKernelGGL(bloch_fold_keys_kernel, grid_for(nnz, GRID_STRIDE_CAP), dim3(256), 0, 0, didx.p, dcol.p, nnz, dcell.p, dflags.p, (u64)dim, (int)nparts,
                               keys.p);
            HIP_CHECK(hipGetLastError());
            std::unique_ptr<P1Handle> all(triplets_to_csr(dim * nparts, nnz, keys, a, v1 ? &b : nullptr));
            for (int p = 0; p < nparts; ++p) {                               // rows p*dim .. (p+1)*dim-1 of the stacked matrix are part p
                P1Handle &P = *parts[(size_t)p];
                const int e0 = all->rowptr[(size_t)p * dim], e1 = all->rowptr[(size_t)(p + 1) * dim];
                P.nnz = e1 - e0;
                for (int64_t r = 0; r <= dim; ++r) P.rowptr[(size_t)r] = all->rowptr[(size_t)(p * dim + r)] - e0;
                P.col.assign(all->col.begin() + e0, all->col.begin() + e1);
                P.m.assign(all->m.begin() + e0, all->m.begin() + e1);
                P.k.assign(all->k.begin() + e0, all->k.begin() + e1);
            }
        }
        for (int p = 0; p < nparts; ++p) out[p] = parts[(size_t)p].release();
        return WAE_OK;
    });
}

}  // extern "C"
