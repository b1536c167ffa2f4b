// Point location in a tetrahedral mesh and sampling of P1 / P2 / Hermite vectors at the located points, on the device: the counterpart of
// find_tetrahedron_containing_point (src/Meshutils.jl:800-815) and of get_p / get_n_grad_p (src/FEM/helmholtz_getters.jl:7-45) for many
// points at once.  One handle keeps the mesh, a uniform cell grid over it and (once set) the P2 and the Hermite connectivity in HBM.
//
// Containment.  The barycentric coordinates of x in the tetrahedron (p1, p2, p3, p4) by Cramer's rule on J = [a b c] = [p1-p4, p2-p4, p3-p4],
// r = x - p4 (loc_bary; every operation rounded on its own, contract(off), so that a float64 host restatement gets the same bits):
//      bc = b x c, det = a . bc, l1 = (r . bc) / det, l2 = (a . (r x c)) / det, l3 = (a . (b x r)) / det, l4 = 1 - ((l1 + l2) + l3)
// with u . w = (u0 w0 + u1 w1) + u2 w2.  The quotients carry the sign of det J, so the orientation of the tetrahedron does not matter.  A
// tetrahedron contains x if all four are >= -tol; the answer is the lowest such index, -1 if there is none.
//
// Cell grid.  Bounding box of the points (block reduction), dims cells per axis (host: about ntets / cell_target cells, as cubical as the
// box allows, at most 1024 per axis so that the cell number fits 31 bits).  The cell of a coordinate on one axis is
//      clamp(floor((x - lo) * inv), 0, dim - 1),  inv = dim / (hi - lo)  (0 on an axis without extent)
// for a query point and for the corners of a tetrahedron's box alike (loc_axis_cell).  Every tetrahedron is listed in the cells that its
// bounding box, grown on every side by pad = (4 tol_max + 2^-30) * (hi - lo), overlaps.  In exact arithmetic a point with all coordinates >=
// -tol lies within 3 tol times the tetrahedron's extent of that box, and the expression above is monotone in x under rounding (a
// subtraction, a product with a non-negative number, floor, clamp), so the list of a point's cell holds every tetrahedron that can accept
// it; the 2^-30 share covers coordinates that rounding moves across zero.  A point outside the box grown by the same pad can be in no
// tetrahedron and is answered -1 without a look at the cells; a point in the rim between the two boxes, or on an upper face of the box,
// is clamped into the first or last cell of the axis.  The (cell, tet) pairs are written in tetrahedron order, a stable
// radix sort by cell groups them, the tetrahedra ascending inside a cell: the first hit in the list is the answer.  More than 32 ntets
// pairs (elongated elements): every dim is halved and the pairs are counted again, down to one cell.  No atomics anywhere.
//
// Query: one lane per point.  The lists hold a few dozen candidates at the default target, a walk ends at its first hit (half the list on
// average), the points outside the box leave at once, and a million points fill the device without any sharing of a point among lanes;
// the lanes of a wavefront that fall into the same cell read the same candidates (one fetch).  A wavefront per point with a ballot over 64
// candidates would test the whole list every time and idle most lanes on lists shorter than 64.
//
// Hermite rows (order 3).  The 20 weights of a point in the local order of tets20 (assemble_herm.hip): with x = p4 + J xi the
// coordinates l1..l3 of loc_bary ARE xi, and g1..g3 = n . grad xi.  The reference functions psi_a = sum_m kHermCoef[a][m] xi^kHermExp[m]
// (herm_tables.h) are evaluated from the twenty monomials (kind 1: from their derivatives along n, sum_j g_j d/dxi_j) held in registers;
// the functions of the physical gradients at p_k are recombined as in the assembly, w[4 (1 + i) + k] = sum_j J[i][j] psi_{4 (1 + j) + k}.
// All loops are unrolled, so the exponents and the (integer) coefficients are compile-time operands and the zero coefficients cost nothing.
#include <climits>
#include <memory>
#include <vector>

#include "herm_tables.h"
#include "mesh_host.h"

namespace {

constexpr double LOC_TOL_MAX = 1e-6;
constexpr double LOC_PAD = 4.0 * LOC_TOL_MAX + 9.313225746154785e-10;          // 4 tol_max + 2^-30
constexpr int LOC_DIM_MAX = 1024;
constexpr int64_t LOC_CELLS_PER_TET = 8;                                        // at most this many cells per tetrahedron
constexpr int LOC_BOX_BLOCKS = 256;

struct LocGrid {
    double lo[3], hi[3], inv[3], pad[3];
    int dims[3];
};

__device__ inline int loc_axis_cell(double x, double lo, double inv, int dim) {
#pragma clang fp contract(off)
    const double f = floor((x - lo) * inv);
    return f < 0.0 ? 0 : (f >= (double)dim ? dim - 1 : (int)f);
}

__device__ inline double loc_dot(double u0, double u1, double u2, double w0, double w1, double w2) {
#pragma clang fp contract(off)
    return (u0 * w0 + u1 * w1) + u2 * w2;
}

// the coordinates l[4] of x in tetrahedron t; n != null: also g[i] = n . grad l_i; J != null: also J[3 i + j] = (p_{j+1} - p4)_i
__device__ inline void loc_bary(const double *__restrict__ pts, const int *__restrict__ tets, int64_t t, const double *x, const double *n, double *l,
                                double *g, double *J = nullptr) {
#pragma clang fp contract(off)
    const int *v = tets + t * 4;
    const double *p1 = pts + (size_t)v[0] * 3, *p2 = pts + (size_t)v[1] * 3, *p3 = pts + (size_t)v[2] * 3, *p4 = pts + (size_t)v[3] * 3;
    const double a0 = p1[0] - p4[0], a1 = p1[1] - p4[1], a2 = p1[2] - p4[2];
    const double b0 = p2[0] - p4[0], b1 = p2[1] - p4[1], b2 = p2[2] - p4[2];
    const double c0 = p3[0] - p4[0], c1 = p3[1] - p4[1], c2 = p3[2] - p4[2];
    const double r0 = x[0] - p4[0], r1 = x[1] - p4[1], r2 = x[2] - p4[2];
    const double bc0 = b1 * c2 - b2 * c1, bc1 = b2 * c0 - b0 * c2, bc2 = b0 * c1 - b1 * c0;
    const double det = loc_dot(a0, a1, a2, bc0, bc1, bc2);
    const double rc0 = r1 * c2 - r2 * c1, rc1 = r2 * c0 - r0 * c2, rc2 = r0 * c1 - r1 * c0;
    const double br0 = b1 * r2 - b2 * r1, br1 = b2 * r0 - b0 * r2, br2 = b0 * r1 - b1 * r0;
    l[0] = loc_dot(r0, r1, r2, bc0, bc1, bc2) / det;
    l[1] = loc_dot(a0, a1, a2, rc0, rc1, rc2) / det;
    l[2] = loc_dot(a0, a1, a2, br0, br1, br2) / det;
    l[3] = 1.0 - ((l[0] + l[1]) + l[2]);
    if (n) {
        const double ca0 = c1 * a2 - c2 * a1, ca1 = c2 * a0 - c0 * a2, ca2 = c0 * a1 - c1 * a0;
        const double ab0 = a1 * b2 - a2 * b1, ab1 = a2 * b0 - a0 * b2, ab2 = a0 * b1 - a1 * b0;
        g[0] = loc_dot(n[0], n[1], n[2], bc0, bc1, bc2) / det;
        g[1] = loc_dot(n[0], n[1], n[2], ca0, ca1, ca2) / det;
        g[2] = loc_dot(n[0], n[1], n[2], ab0, ab1, ab2) / det;
        g[3] = -((g[0] + g[1]) + g[2]);
    }
    if (J) {
        J[0] = a0; J[1] = b0; J[2] = c0;
        J[3] = a1; J[4] = b1; J[5] = c1;
        J[6] = a2; J[7] = b2; J[8] = c2;
    }
}

// the row of the probe functional: NW = 4 (P1) or 10 (P2) weights from l (and g for kind 1), in the order of probe_p / probe_n_grad_p
template <int NW> __device__ inline void loc_row(int kind, const double *l, const double *g, double *w) {
#pragma clang fp contract(off)
    constexpr int EI[6] = {0, 0, 0, 1, 1, 2}, EJ[6] = {1, 2, 3, 2, 3, 3};
    if constexpr (NW == 4) {
#pragma unroll
        for (int i = 0; i < 4; ++i) w[i] = kind ? g[i] : l[i];
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) w[i] = kind ? (4.0 * l[i] - 1.0) * g[i] : l[i] * (2.0 * l[i] - 1.0);
#pragma unroll
        for (int e = 0; e < 6; ++e) {
            const int i = EI[e], j = EJ[e];
            w[4 + e] = kind ? 4.0 * (l[j] * g[i] + l[i] * g[j]) : (4.0 * l[i]) * l[j];
        }
    }
}

// psi_a from the monomials (or their directional derivatives): the terms in the order of m, the zero coefficients left out
__device__ inline double loc_herm_psi(int a, const double *mono) {
#pragma clang fp contract(off)
    double acc = 0.0;
#pragma unroll
    for (int m = 0; m < 20; ++m)
        if (kHermCoef[a][m] != 0.0) acc = acc + kHermCoef[a][m] * mono[m];
    return acc;
}

// the Hermite row: 20 weights from xi = l[0..2] (kind 1: and g[0..2] = n . grad xi) and J, in the local order of tets20
__device__ inline void loc_row_herm(int kind, const double *l, const double *g, const double *J, double *w) {
#pragma clang fp contract(off)
    double pw[3][4], mono[20];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        pw[j][0] = 1.0;
        pw[j][1] = l[j];
        pw[j][2] = l[j] * l[j];
        pw[j][3] = pw[j][2] * l[j];
    }
    if (!kind) {
#pragma unroll
        for (int m = 0; m < 20; ++m) mono[m] = (pw[0][kHermExp[m][0]] * pw[1][kHermExp[m][1]]) * pw[2][kHermExp[m][2]];
    } else {
#pragma unroll
        for (int m = 0; m < 20; ++m) {                               // sum_j g_j d(xi^e)/dxi_j, j ascending
            double d = 0.0;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                if (kHermExp[m][j] == 0) continue;
                double term = (double)kHermExp[m][j];
#pragma unroll
                for (int i = 0; i < 3; ++i) term = term * pw[i][i == j ? kHermExp[m][i] - 1 : kHermExp[m][i]];
                d = d + g[j] * term;
            }
            mono[m] = d;
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        w[k] = loc_herm_psi(k, mono);
        w[16 + k] = loc_herm_psi(16 + k, mono);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {                                    // one vertex at a time: three reference functions live, not twelve
        const double p0 = loc_herm_psi(4 + k, mono), p1 = loc_herm_psi(8 + k, mono), p2 = loc_herm_psi(12 + k, mono);
#pragma unroll
        for (int i = 0; i < 3; ++i) w[4 * (1 + i) + k] = loc_dot(J[3 * i], J[3 * i + 1], J[3 * i + 2], p0, p1, p2);
    }
}

// ---- bounding box ----------------------------------------------------------------------------------------------------------------------
// partial[6 * block + k]: k < 3 the minimum, k >= 3 the maximum of axis k % 3 over the block's share of the points
__global__ __launch_bounds__(256) void loc_box_kernel(const double *__restrict__ pts, int64_t np, double *__restrict__ partial) {
    __shared__ double sm[6][256];
    double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < np; i += (int64_t)gridDim.x * 256)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double v = pts[i * 3 + k];
            mn[k] = fmin(mn[k], v);
            mx[k] = fmax(mx[k], v);
        }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        sm[k][threadIdx.x] = mn[k];
        sm[3 + k][threadIdx.x] = mx[k];
    }
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                sm[k][threadIdx.x] = fmin(sm[k][threadIdx.x], sm[k][threadIdx.x + s]);
                sm[3 + k][threadIdx.x] = fmax(sm[3 + k][threadIdx.x], sm[3 + k][threadIdx.x + s]);
            }
        __syncthreads();
    }
    if (threadIdx.x < 6) partial[(size_t)blockIdx.x * 6 + threadIdx.x] = sm[threadIdx.x][0];
}

__global__ __launch_bounds__(64) void loc_box_final_kernel(const double *__restrict__ partial, int nblk, double *__restrict__ box) {
    const int k = threadIdx.x;
    if (k >= 6) return;
    double v = partial[k];
    for (int b = 1; b < nblk; ++b) v = k < 3 ? fmin(v, partial[(size_t)b * 6 + k]) : fmax(v, partial[(size_t)b * 6 + k]);
    box[k] = v;
}

// ---- cell lists ------------------------------------------------------------------------------------------------------------------------
// the cell range [c0, c1] per axis of the grown bounding box of tetrahedron t
__device__ inline void loc_tet_range(const LocGrid &G, const double *__restrict__ pts, const int *__restrict__ tets, int64_t t, int *c0, int *c1) {
#pragma clang fp contract(off)
    const int *v = tets + t * 4;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double x0 = pts[(size_t)v[0] * 3 + k], x1 = pts[(size_t)v[1] * 3 + k], x2 = pts[(size_t)v[2] * 3 + k], x3 = pts[(size_t)v[3] * 3 + k];
        const double mn = fmin(fmin(x0, x1), fmin(x2, x3)), mx = fmax(fmax(x0, x1), fmax(x2, x3));
        c0[k] = loc_axis_cell(mn - G.pad[k], G.lo[k], G.inv[k], G.dims[k]);
        c1[k] = loc_axis_cell(mx + G.pad[k], G.lo[k], G.inv[k], G.dims[k]);
    }
}

// len[t] = cells that tetrahedron t is listed in, len[nt] = 0: the exclusive scan of nt + 1 values ends with the pair count
__global__ __launch_bounds__(256) void loc_count_kernel(LocGrid G, const double *__restrict__ pts, const int *__restrict__ tets, int64_t nt,
                                                        long long *__restrict__ len) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t > nt) return;
    if (t == nt) { len[t] = 0; return; }
    int c0[3], c1[3];
    loc_tet_range(G, pts, tets, t, c0, c1);
    len[t] = (long long)(c1[0] - c0[0] + 1) * (long long)(c1[1] - c0[1] + 1) * (long long)(c1[2] - c0[2] + 1);
}

// the pairs of tetrahedron t at off[t] ...: key = cell, value = t
__global__ __launch_bounds__(256) void loc_fill_kernel(LocGrid G, const double *__restrict__ pts, const int *__restrict__ tets, int64_t nt,
                                                       const long long *__restrict__ off, unsigned *__restrict__ key, int *__restrict__ val) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= nt) return;
    int c0[3], c1[3];
    loc_tet_range(G, pts, tets, t, c0, c1);
    long long p = off[t];
    for (int z = c0[2]; z <= c1[2]; ++z)
        for (int y = c0[1]; y <= c1[1]; ++y)
            for (int x = c0[0]; x <= c1[0]; ++x) {
                key[p] = (unsigned)((z * G.dims[1] + y) * G.dims[0] + x);
                val[p] = (int)t;
                ++p;
            }
}

// ptr[c] = the first position of the sorted keys that is not below c, c = 0..ncells; len[c] = the length of cell c's list
__global__ __launch_bounds__(256) void loc_ptr_kernel(const unsigned *__restrict__ key, int nrefs, int64_t ncells, int *__restrict__ ptr) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c > ncells) return;
    int lo = 0, hi = nrefs;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if ((int64_t)key[mid] < c) lo = mid + 1;
        else hi = mid;
    }
    ptr[c] = lo;
}

__global__ __launch_bounds__(256) void loc_len_kernel(const int *__restrict__ ptr, int64_t ncells, int *__restrict__ len) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c < ncells) len[c] = ptr[c + 1] - ptr[c];
}

// ---- queries ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void loc_find_kernel(LocGrid G, const double *__restrict__ pts, const int *__restrict__ tets,
                                                       const int *__restrict__ cell_ptr, const int *__restrict__ cell_tet, int64_t nq,
                                                       const double *__restrict__ xq, double tol, int *__restrict__ out, double *__restrict__ lam) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= nq) return;
    const double x[3] = {xq[q * 3], xq[q * 3 + 1], xq[q * 3 + 2]};
    int found = -1;
    double l[4] = {NAN, NAN, NAN, NAN};
    bool inside = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) inside = inside && x[k] >= G.lo[k] - G.pad[k] && x[k] <= G.hi[k] + G.pad[k];
    if (inside) {
        const int cx = loc_axis_cell(x[0], G.lo[0], G.inv[0], G.dims[0]), cy = loc_axis_cell(x[1], G.lo[1], G.inv[1], G.dims[1]);
        const int cz = loc_axis_cell(x[2], G.lo[2], G.inv[2], G.dims[2]);
        const int64_t cell = ((int64_t)cz * G.dims[1] + cy) * G.dims[0] + cx;
        const int e = cell_ptr[cell + 1];
        const double mt = -tol;
        for (int p = cell_ptr[cell]; p < e; ++p) {
            const int t = cell_tet[p];
            double m[4];
            loc_bary(pts, tets, t, x, nullptr, m, nullptr);
            if (m[0] >= mt && m[1] >= mt && m[2] >= mt && m[3] >= mt) {
                found = t;
                l[0] = m[0]; l[1] = m[1]; l[2] = m[2]; l[3] = m[3];
                break;
            }
        }
    }
    out[q] = found;
    if (lam) {
        lam[q * 4] = l[0]; lam[q * 4 + 1] = l[1]; lam[q * 4 + 2] = l[2]; lam[q * 4 + 3] = l[3];
    }
}

// the row of point q: NW weights and the unknowns they act on (nodes: tets for P1, tets10 for P2, tets20 for Hermite); false for tet[q] == -1
template <int NW>
__device__ inline bool loc_point_row(const double *__restrict__ pts, const int *__restrict__ tets, const int *__restrict__ nodes, int kind, int64_t q,
                                     const double *__restrict__ xq, const int *__restrict__ tet, const double *__restrict__ nq3, int *idx, double *w) {
    const int t = tet[q];
    if (t < 0) return false;
    const double x[3] = {xq[q * 3], xq[q * 3 + 1], xq[q * 3 + 2]};
    double n[3] = {0.0, 0.0, 0.0}, l[4], g[4] = {0.0, 0.0, 0.0, 0.0};
    if (kind) { n[0] = nq3[q * 3]; n[1] = nq3[q * 3 + 1]; n[2] = nq3[q * 3 + 2]; }
    if constexpr (NW == 20) {
        double J[9];
        loc_bary(pts, tets, t, x, kind ? n : nullptr, l, g, J);
        loc_row_herm(kind, l, g, J, w);
    } else {
        loc_bary(pts, tets, t, x, kind ? n : nullptr, l, g);
        loc_row<NW>(kind, l, g, w);
    }
#pragma unroll
    for (int i = 0; i < NW; ++i) idx[i] = nodes[(size_t)t * NW + i];
    return true;
}

template <int NW>
__global__ __launch_bounds__(256) void loc_weights_kernel(const double *__restrict__ pts, const int *__restrict__ tets, const int *__restrict__ nodes,
                                                          int kind, int64_t nq, const double *__restrict__ xq, const int *__restrict__ tet,
                                                          const double *__restrict__ nq3, int *__restrict__ idx, double *__restrict__ val) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= nq) return;
    int id[NW];
    double w[NW];
    const bool ok = loc_point_row<NW>(pts, tets, nodes, kind, q, xq, tet, nq3, id, w);
#pragma unroll
    for (int i = 0; i < NW; ++i) {
        idx[q * NW + i] = ok ? id[i] : 0;
        val[q * NW + i] = ok ? w[i] : 0.0;
    }
}

// out[q, c] = sum_i w_i V[idx_i, c], i ascending, every product and sum rounded on its own; the lanes of a wave on consecutive points, so
// the store of a column coalesces; the row stays in registers over the columns
template <int NW>
__global__ __launch_bounds__(256) void loc_sample_kernel(const double *__restrict__ pts, const int *__restrict__ tets, const int *__restrict__ nodes,
                                                         int kind, int64_t nq, const double *__restrict__ xq, const int *__restrict__ tet,
                                                         const double *__restrict__ nq3, int64_t d, int ncols, const cplx *__restrict__ V,
                                                         cplx *__restrict__ out) {
#pragma clang fp contract(off)
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= nq) return;
    int id[NW];
    double w[NW];
    const bool ok = loc_point_row<NW>(pts, tets, nodes, kind, q, xq, tet, nq3, id, w);
    for (int c = 0; c < ncols; ++c) {
        double re = NAN, im = NAN;
        if (ok) {
            const cplx *v = V + (size_t)c * d;
            re = w[0] * v[id[0]].x;
            im = w[0] * v[id[0]].y;
#pragma unroll
            for (int i = 1; i < NW; ++i) {
                const cplx z = v[id[i]];
                re = re + w[i] * z.x;
                im = im + w[i] * z.y;
            }
        }
        out[(size_t)c * nq + q] = cplx{re, im};
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------
struct Locator {
    int device = 0;
    int64_t np = 0, nt = 0, ndof = 0, ndof20 = 0, nrefs = 0, maxlen = 0;
    LocGrid G;
    DevBuf<double> pts;
    DevBuf<int> tets, tets10, tets20, cell_ptr, cell_tet;
};

// about `want` cells over the box, as cubical as it allows: the axes with an extent share the cells, the others have one
void loc_dims(const double *lo, const double *hi, double want, int *dims) {
    double vol = 1.0;
    int nax = 0;
    for (int k = 0; k < 3; ++k)
        if (hi[k] > lo[k]) { vol *= hi[k] - lo[k]; ++nax; }
    for (int k = 0; k < 3; ++k) dims[k] = 1;
    if (!nax || !(want > 1.0)) return;
    const double h = std::pow(vol / want, 1.0 / nax);
    for (int k = 0; k < 3; ++k)
        if (hi[k] > lo[k]) {
            const double n = std::ceil((hi[k] - lo[k]) / h);
            dims[k] = n >= LOC_DIM_MAX ? LOC_DIM_MAX : (n >= 1.0 ? (int)n : 1);
        }
}

void loc_set_dims(LocGrid &G, const int *dims) {
    for (int k = 0; k < 3; ++k) {
        G.dims[k] = dims[k];
        G.inv[k] = G.hi[k] > G.lo[k] ? (double)dims[k] / (G.hi[k] - G.lo[k]) : 0.0;
    }
}

void loc_build(Locator &H, int64_t cell_target) {
    const int64_t np = H.np, nt = H.nt;
    {
        const int nblk = (int)std::min<int64_t>(LOC_BOX_BLOCKS, (np + 255) / 256);
        Dev<double> partial((size_t)nblk * 6), box(6);
        hipLaunchKernelGGL(loc_box_kernel, dim3(nblk), dim3(256), 0, 0, H.pts.p, np, partial.p);
        HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(loc_box_final_kernel, dim3(1), dim3(64), 0, 0, partial.p, nblk, box.p);
        HIP_CHECK(hipGetLastError());
        double hb[6];
        box.to_host(hb, 6);
        for (int k = 0; k < 3; ++k) {
            H.G.lo[k] = hb[k];
            H.G.hi[k] = hb[3 + k];
            H.G.pad[k] = LOC_PAD * (hb[3 + k] - hb[k]);
        }
    }
    int dims[3];
    loc_dims(H.G.lo, H.G.hi, (double)nt / (double)(cell_target > 0 ? cell_target : 8), dims);
    // the cell arrays stay proportional to the mesh: the per-axis clamp alone allows 2^30 cells (a small cell_target on a large mesh, or
    // the rounding up of the axes of a thin box)
    while ((int64_t)dims[0] * dims[1] * dims[2] > LOC_CELLS_PER_TET * nt)
        for (int k = 0; k < 3; ++k) dims[k] = (dims[k] + 1) / 2;
    Dev<long long> len((size_t)nt + 1), off((size_t)nt + 1);
    DevBuf<char> tmp;                                                // (allocated by the first scan, kept for the others)
    long long nrefs = 0;
    for (;;) {
        loc_set_dims(H.G, dims);
        hipLaunchKernelGGL(loc_count_kernel, grid_for(nt + 1), dim3(256), 0, 0, H.G, H.pts.p, H.tets.p, nt, len.p);
        HIP_CHECK(hipGetLastError());
        exclusive_sum(len.p, off.p, (int)(nt + 1), tmp);
        off.to_host(&nrefs, 1, (size_t)nt);
        if (nrefs < nt) throw WaeError(WAE_ERR_HIP, "locator: the scan returned an impossible pair count");
        if (nrefs <= 32 * nt || (dims[0] == 1 && dims[1] == 1 && dims[2] == 1)) break;
        for (int k = 0; k < 3; ++k) dims[k] = (dims[k] + 1) / 2;
    }
    const int64_t ncells = (int64_t)dims[0] * dims[1] * dims[2];
    const int cnt = (int)nrefs;                                      // <= 32 ntets <= INT_MAX (checked by the caller)
    Dev<unsigned> k0((size_t)nrefs), k1((size_t)nrefs);
    Dev<int> v0((size_t)nrefs);
    H.cell_tet.alloc((size_t)nrefs);
    H.cell_ptr.alloc((size_t)ncells + 1);
    hipLaunchKernelGGL(loc_fill_kernel, grid_for(nt), dim3(256), 0, 0, H.G, H.pts.p, H.tets.p, nt, off.p, k0.p, v0.p);
    HIP_CHECK(hipGetLastError());
    const int bits = key_bits((uint64_t)ncells);                     // (at most 31: ncells <= 2^30)
    Dev<int> lens((size_t)ncells), dmax(1);
    auto sort = [&](void *t, size_t &b) { return hipcub::DeviceRadixSort::SortPairs(t, b, k0.p, k1.p, v0.p, H.cell_tet.p, cnt, 0, bits); };
    auto longest = [&](void *t, size_t &b) { return hipcub::DeviceReduce::Max(t, b, lens.p, dmax.p, (int)ncells); };
    DevBuf<char> tmp2;
    cub_reserve(tmp2, sort, longest);
    cub_run(sort, tmp2);
    hipLaunchKernelGGL(loc_ptr_kernel, grid_for(ncells + 1), dim3(256), 0, 0, k1.p, cnt, ncells, H.cell_ptr.p);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(loc_len_kernel, grid_for(ncells), dim3(256), 0, 0, H.cell_ptr.p, ncells, lens.p);
    HIP_CHECK(hipGetLastError());
    cub_run(longest, tmp2);
    int hmax = 0;
    dmax.to_host(&hmax, 1);
    H.nrefs = nrefs;
    H.maxlen = hmax;
}

const Locator &loc_handle(const void *h) {
    if (!h) throw WaeError(WAE_ERR_INVALID, "null handle");
    return *(const Locator *)h;
}

void loc_check_finite(const double *x, int64_t count, const char *what) {
    for (int64_t i = 0; i < count; ++i)
        if (!std::isfinite(x[i])) throw WaeError(WAE_ERR_INVALID, std::string(what) + " holds a coordinate that is not finite");
}

// the checks shared by wae_locator_weights and wae_locator_sample; returns the node table (tets, tets10 or tets20)
const int *loc_check_rows(const Locator &H, int32_t order, int32_t kind, int64_t nq, const double *x, const int32_t *tet, const double *n) {
    // order 3 exists on a handle once its table is set; before that it is refused like any unknown order, with the words of that refusal
    if (order != 1 && order != 2 && !(order == 3 && H.tets20.p)) throw WaeError(WAE_ERR_INVALID, "order must be 1 or 2");
    if (kind != 0 && kind != 1) throw WaeError(WAE_ERR_INVALID, "kind must be 0 (p) or 1 (n.grad p)");
    if (order == 2 && !H.tets10.p) throw WaeError(WAE_ERR_INVALID, "order 2 needs wae_locator_set_p2 first");
    if (kind == 1 && !n) throw WaeError(WAE_ERR_INVALID, "kind 1 needs the directions n");
    if (!(x && tet)) throw WaeError(WAE_ERR_INVALID, "bad argument");
    loc_check_finite(x, nq * 3, "x");
    for (int64_t q = 0; q < nq; ++q)
        if (tet[q] < -1 || tet[q] >= H.nt) throw WaeError(WAE_ERR_INVALID, "tet holds an index outside -1..ntets-1");
    return order == 1 ? H.tets.p : (order == 2 ? H.tets10.p : H.tets20.p);
}

struct LocQuery {                       // the per-point inputs of a weights / sample call in HBM
    DevBuf<double> x, n;
    DevBuf<int> tet;
    LocQuery(int64_t nq, const double *hx, const int32_t *ht, const double *hn) {
        x.from_host(hx, (size_t)nq * 3);
        tet.from_host(ht, (size_t)nq);
        if (hn) n.from_host(hn, (size_t)nq * 3);
    }
};

}  // namespace

extern "C" {

int wae_locator_create(int32_t device, int64_t npoints, const double *points, int64_t ntets, const int32_t *tets, int64_t cell_target, void **out) {
    return wae_guarded([&]() {
        if (npoints < 0 || ntets < 0 || cell_target < 0) throw WaeError(WAE_ERR_INVALID, "a count is negative");
        if (!(out && points && tets && npoints > 0 && ntets > 0)) throw WaeError(WAE_ERR_INVALID, "bad argument");
        if (npoints > INT_MAX || ntets > INT_MAX / 32) throw WaeError(WAE_ERR_INVALID, "npoints or 32*ntets does not fit a 32-bit index");
        check_tets(tets, ntets, npoints);
        loc_check_finite(points, npoints * 3, "points");
        HIP_CHECK(hipSetDevice(device));
        std::unique_ptr<Locator> H(new Locator);
        H->device = device;
        H->np = npoints;
        H->nt = ntets;
        H->pts.from_host(points, (size_t)npoints * 3);
        H->tets.from_host(tets, (size_t)ntets * 4);
        loc_build(*H, cell_target);
        *out = H.release();
        return WAE_OK;
    });
}

int wae_locator_info(const void *h, int64_t *npoints, int64_t *ntets, int64_t *dims, int64_t *nrefs, int64_t *max_per_cell) {
    return wae_guarded([&]() {
        const Locator &H = loc_handle(h);
        if (npoints) *npoints = H.np;
        if (ntets) *ntets = H.nt;
        if (dims)
            for (int k = 0; k < 3; ++k) dims[k] = H.G.dims[k];
        if (nrefs) *nrefs = H.nrefs;
        if (max_per_cell) *max_per_cell = H.maxlen;
        return WAE_OK;
    });
}

int wae_locator_find(const void *h, int64_t nq, const double *x, double tol, int32_t *tet, double *lambda) {
    return wae_guarded([&]() {
        const Locator &H = loc_handle(h);
        if (nq < 0) throw WaeError(WAE_ERR_INVALID, "nq is negative");
        if (!(tol >= 0.0 && tol <= LOC_TOL_MAX)) throw WaeError(WAE_ERR_INVALID, "tol must lie in [0, 1e-6]");
        if (nq == 0) return WAE_OK;
        if (!(x && tet)) throw WaeError(WAE_ERR_INVALID, "bad argument");
        loc_check_finite(x, nq * 3, "x");
        HIP_CHECK(hipSetDevice(H.device));
        DevBuf<double> dx, dl;
        DevBuf<int> dt;
        dx.from_host(x, (size_t)nq * 3);
        dt.alloc((size_t)nq);
        if (lambda) dl.alloc((size_t)nq * 4);
        hipLaunchKernelGGL(loc_find_kernel, grid_for(nq), dim3(256), 0, 0, H.G, H.pts.p, H.tets.p, H.cell_ptr.p, H.cell_tet.p, nq, dx.p, tol, dt.p, dl.p);
        HIP_CHECK(hipGetLastError());
        dt.to_host(tet, (size_t)nq);
        dl.to_host(lambda, (size_t)nq * 4);
        return WAE_OK;
    });
}

int wae_locator_set_p2(void *h, int64_t ndof, const int32_t *tets10) {
    return wae_guarded([&]() {
        Locator &H = const_cast<Locator &>(loc_handle(h));
        if (ndof < 0) throw WaeError(WAE_ERR_INVALID, "ndof is negative");
        if (!tets10 || ndof < 1 || ndof > INT_MAX) throw WaeError(WAE_ERR_INVALID, "bad argument");
        check_indices(tets10, H.nt * 10, ndof, "tets10 holds an entry outside 0..ndof-1");
        HIP_CHECK(hipSetDevice(H.device));
        DevBuf<int> t10;
        t10.from_host(tets10, (size_t)H.nt * 10);
        H.tets10 = std::move(t10);
        H.ndof = ndof;
        return WAE_OK;
    });
}

int wae_hermite_locator_set(void *h, int64_t ndof, const int32_t *tets20) {
    return wae_guarded([&]() {
        Locator &H = const_cast<Locator &>(loc_handle(h));
        if (!tets20) throw WaeError(WAE_ERR_INVALID, "tets20 is null");
        if (ndof < 4 * H.np || ndof > INT_MAX) throw WaeError(WAE_ERR_INVALID, "ndof must be at least 4*npoints and fit a 32-bit index");
        HIP_CHECK(hipSetDevice(H.device));
        std::vector<int> tets((size_t)H.nt * 4);
        H.tets.to_host(tets.data(), tets.size());
        for (int64_t t = 0; t < H.nt; ++t) {
            const int32_t *r = tets20 + t * 20;
            for (int b = 0; b < 4; ++b)
                for (int k = 0; k < 4; ++k)
                    if ((int64_t)r[4 * b + k] != b * H.np + tets[(size_t)t * 4 + k])
                        throw WaeError(WAE_ERR_INVALID, "tets20: entry 4 b + k of a tetrahedron is not b * npoints + its point k");
            for (int k = 16; k < 20; ++k)
                if (r[k] < 4 * H.np || r[k] >= ndof) throw WaeError(WAE_ERR_INVALID, "tets20 holds a face unknown outside 4*npoints..ndof-1");
        }
        DevBuf<int> t20;
        t20.from_host(tets20, (size_t)H.nt * 20);
        H.tets20 = std::move(t20);
        H.ndof20 = ndof;
        return WAE_OK;
    });
}

int wae_locator_weights(const void *h, int32_t order, int32_t kind, int64_t nq, const double *x, const int32_t *tet, const double *n, int32_t *idx,
                        double *val) {
    return wae_guarded([&]() {
        const Locator &H = loc_handle(h);
        if (nq < 0) throw WaeError(WAE_ERR_INVALID, "nq is negative");
        if (nq == 0) return WAE_OK;
        const int *nodes = loc_check_rows(H, order, kind, nq, x, tet, n);
        if (!(idx && val)) throw WaeError(WAE_ERR_INVALID, "bad argument");
        HIP_CHECK(hipSetDevice(H.device));
        const int nw = order == 1 ? 4 : (order == 2 ? 10 : 20);
        LocQuery Q(nq, x, tet, kind ? n : nullptr);
        DevBuf<int> di;
        DevBuf<double> dv;
        di.alloc((size_t)nq * nw);
        dv.alloc((size_t)nq * nw);
        if (order == 1)
            hipLaunchKernelGGL(loc_weights_kernel<4>, grid_for(nq), dim3(256), 0, 0, H.pts.p, H.tets.p, nodes, (int)kind, nq, Q.x.p, Q.tet.p, Q.n.p, di.p, dv.p);
        else if (order == 2)
            hipLaunchKernelGGL(loc_weights_kernel<10>, grid_for(nq), dim3(256), 0, 0, H.pts.p, H.tets.p, nodes, (int)kind, nq, Q.x.p, Q.tet.p, Q.n.p, di.p, dv.p);
        else
            hipLaunchKernelGGL(loc_weights_kernel<20>, grid_for(nq), dim3(256), 0, 0, H.pts.p, H.tets.p, nodes, (int)kind, nq, Q.x.p, Q.tet.p, Q.n.p, di.p, dv.p);
        HIP_CHECK(hipGetLastError());
        di.to_host(idx, (size_t)nq * nw);
        dv.to_host(val, (size_t)nq * nw);
        return WAE_OK;
    });
}

int wae_locator_sample(const void *h, int32_t order, int32_t kind, int64_t nq, const double *x, const int32_t *tet, const double *n, int64_t d,
                       int32_t ncols, const double *V, double *out) {
    return wae_guarded([&]() {
        const Locator &H = loc_handle(h);
        if (nq < 0 || d < 0 || ncols < 0) throw WaeError(WAE_ERR_INVALID, "a count is negative");
        if (nq == 0) return WAE_OK;
        const int *nodes = loc_check_rows(H, order, kind, nq, x, tet, n);
        if (order != 3 && d != (order == 1 ? H.np : H.ndof)) throw WaeError(WAE_ERR_INVALID, "d must be npoints (order 1) or ndof (order 2)");
        if (order == 3 && d != H.ndof20) throw WaeError(WAE_ERR_INVALID, "d must be the ndof given to wae_hermite_locator_set (order 3)");
        if (!(V && out) || ncols < 1) throw WaeError(WAE_ERR_INVALID, "bad argument");
        HIP_CHECK(hipSetDevice(H.device));
        LocQuery Q(nq, x, tet, kind ? n : nullptr);
        DevBuf<cplx> dV, dO;
        dV.from_host((const cplx *)V, (size_t)d * (size_t)ncols);
        dO.alloc((size_t)nq * (size_t)ncols);
        if (order == 1)
            hipLaunchKernelGGL(loc_sample_kernel<4>, grid_for(nq), dim3(256), 0, 0, H.pts.p, H.tets.p, nodes, (int)kind, nq, Q.x.p, Q.tet.p, Q.n.p, d,
                               (int)ncols, dV.p, dO.p);
        else if (order == 2)
            hipLaunchKernelGGL(loc_sample_kernel<10>, grid_for(nq), dim3(256), 0, 0, H.pts.p, H.tets.p, nodes, (int)kind, nq, Q.x.p, Q.tet.p, Q.n.p, d,
                               (int)ncols, dV.p, dO.p);
        else
            hipLaunchKernelGGL(loc_sample_kernel<20>, grid_for(nq), dim3(256), 0, 0, H.pts.p, H.tets.p, nodes, (int)kind, nq, Q.x.p, Q.tet.p, Q.n.p, d,
                               (int)ncols, dV.p, dO.p);
        HIP_CHECK(hipGetLastError());
        dO.to_host((cplx *)out, (size_t)nq * (size_t)ncols);
        return WAE_OK;
    });
}

int wae_locator_free(void *h) {
    if (h) (void)hipSetDevice(((Locator *)h)->device);
    delete (Locator *)h;
    return WAE_OK;
}

}  // extern "C"
