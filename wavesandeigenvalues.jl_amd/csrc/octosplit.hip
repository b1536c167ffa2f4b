// Uniform refinement of a tetrahedral mesh on the device: `octosplit` of the reference (src/Meshutils.jl:589-747), every tetrahedron split
// into 8 and every boundary triangle into 4, with the nested P1 prolongation between the levels.  One handle keeps every level in HBM.
//
// One level, from (points, tets, tris) of the level below:
//   1. Midpoints.  One kernel writes the six keys max(u,v)*npoints + min(u,v) of every tetrahedron (octo_edge_key, edge_keys.h), a radix
//      sort and a unique pass (hipCUB) leave the edges in the order of the reference's mesh.lines (src/Mesh/sorter.jl:9-31: ascending by
//      (larger point, smaller point)).  The old points keep their numbers, the midpoint of edge e is point npoints + e = (x_a + x_b) * 0.5,
//      and parents[e] = (a, b) with a > b.
//   2. Children.  One thread per tetrahedron (A,B,C,D) finds its six midpoints by binary search and writes
//          [A,AB,AC,AD] [B,AB,BC,BD] [C,AC,BC,CD] [D,AD,BD,CD]
//      and the four children of the inner octahedron, cut along the shortest of its diagonals AB-CD, AC-BD, AD-BC (Meshutils.jl:620-640;
//      the <= tie-breaks in that order):
//          AB-CD: [AB,CD,AC,AD] [AB,CD,AD,BD] [AB,CD,BD,BC] [AB,CD,BC,AC]
//          AC-BD: [AC,BD,AB,AD] [AC,BD,AD,CD] [AC,BD,CD,BC] [AC,BD,BC,AB]
//          AD-BC: [AD,BC,AC,CD] [AD,BC,CD,BD] [AD,BC,BD,AB] [AD,BC,AB,AC]
//      The vertex order inside a child is kept as listed (not sorted), so the orientation is mixed as in the reference; every assembly of
//      this library takes |det J|.  One thread per triangle (A,B,C) writes [A,AB,AC] [B,AB,BC] [C,AC,BC] [AB,AC,BC].
//      The diagonals are compared by d2 = (dx*dx + dy*dy) + dz*dz on the differences of the STORED midpoints, every operation rounded on its
//      own (contract(off) in that kernel): a host restatement in float64 gets the same bits, and the same children.  The reference compares
//      LinearAlgebra.norm of the same differences, whose rounding is not specified: on tetrahedra with two diagonals equal or within a
//      rounding of each other (35 + 50 of the 3380 of the tutorial Rijke tube) the package may cut along another diagonal.
//   3. List order.  The children are stored in the reference's sorted order (insert_smplx!, sorter.jl: ascending by "vertices sorted
//      descending, compared lexicographically"; find_smplx is a binary search over it).  The key of a child is its vertices sorted
//      descending, 31 bits each: two stable 64-bit radix sorts of (key, child number), low pair first.  The inverse permutation gives
//      tet_labels (8 per parent) and tri_labels (4 per parent): the positions of a parent's children, in the order listed above.
// No atomics, the same bits on every call.  Only the edge count and three flags of a level come back to the host before the next level starts.
//
// The P2 prolongation between the levels ("P2 prolongation between two levels" below): the first P2 entry called on a handle numbers the
// P2 edges of every level and builds every step as a CSR matrix in HBM; wae_octosplit_prolong_p2 applies it, wae_octosplit_prolongator_p2
// copies it out.
#include <climits>
#include <memory>
#include <vector>

#include "edge_keys.h"
#include "mesh_host.h"

namespace {

typedef unsigned long long u64;

__global__ __launch_bounds__(256) void octo_edge_keys_kernel(const int *__restrict__ tets, int64_t nt, u64 np, u64 *__restrict__ keys) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= nt) return;
    const int v0 = tets[t * 4], v1 = tets[t * 4 + 1], v2 = tets[t * 4 + 2], v3 = tets[t * 4 + 3];
    u64 *k = keys + t * 6;
    k[0] = octo_edge_key(v0, v1, np); k[1] = octo_edge_key(v0, v2, np); k[2] = octo_edge_key(v0, v3, np);
    k[3] = octo_edge_key(v1, v2, np); k[4] = octo_edge_key(v1, v3, np); k[5] = octo_edge_key(v2, v3, np);
}

// point np + e of the new level and its parents (larger, smaller); pts holds the np old points already
__global__ __launch_bounds__(256) void octo_midpoints_kernel(const u64 *__restrict__ ek, int64_t ne, u64 np, double *__restrict__ pts,
                                                             int *__restrict__ parents) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= ne) return;
    const u64 k = ek[e], a = k / np, b = k - a * np;
    parents[e * 2] = (int)a;
    parents[e * 2 + 1] = (int)b;
    double *o = pts + (np + (u64)e) * 3;
    o[0] = (pts[a * 3] + pts[b * 3]) * 0.5;
    o[1] = (pts[a * 3 + 1] + pts[b * 3 + 1]) * 0.5;
    o[2] = (pts[a * 3 + 2] + pts[b * 3 + 2]) * 0.5;
}

__device__ inline void octo_order2(int &a, int &b) {      // a >= b afterwards
    const int hi = max(a, b), lo = min(a, b);
    a = hi; b = lo;
}

// child c of a tetrahedron: the vertices as listed, and the two halves of its sort key (vertices sorted descending, 31 bits each)
__device__ inline void octo_put_tet(int *__restrict__ child, u64 *__restrict__ khi, u64 *__restrict__ klo, int64_t c, int a, int b, int d, int e) {
    int *o = child + c * 4;
    o[0] = a; o[1] = b; o[2] = d; o[3] = e;
    octo_order2(a, b); octo_order2(d, e); octo_order2(a, d); octo_order2(b, e); octo_order2(b, d);
    khi[c] = ((u64)a << 31) | (u64)b;
    klo[c] = ((u64)d << 31) | (u64)e;
}

__device__ inline void octo_put_tri(int *__restrict__ child, u64 *__restrict__ khi, u64 *__restrict__ klo, int64_t c, int a, int b, int d) {
    int *o = child + c * 3;
    o[0] = a; o[1] = b; o[2] = d;
    octo_order2(a, b); octo_order2(b, d); octo_order2(a, b);
    khi[c] = ((u64)a << 31) | (u64)b;
    klo[c] = (u64)d;
}

__device__ inline double octo_dist2(const double *__restrict__ pts, int p, int q) {
#pragma clang fp contract(off)
    const double dx = pts[(size_t)p * 3] - pts[(size_t)q * 3], dy = pts[(size_t)p * 3 + 1] - pts[(size_t)q * 3 + 1],
                 dz = pts[(size_t)p * 3 + 2] - pts[(size_t)q * 3 + 2];
    return (dx * dx + dy * dy) + dz * dz;
}

// threads 0..nt-1: the 8 children of a tetrahedron (child number 8 t + position in the list of the header comment);
// nt..nt+ns-1: the 4 children of a triangle.  pts: the points of the NEW level.  bad[0]: a triangle edge that is no tetrahedron's edge
// (its children are not written)
__global__ __launch_bounds__(256) void octo_children_kernel(const int *__restrict__ tets, int64_t nt, const int *__restrict__ tris, int64_t ns,
                                                            const u64 *__restrict__ ek, int64_t ne, u64 np, const double *__restrict__ pts,
                                                            int *__restrict__ tchild, u64 *__restrict__ thi, u64 *__restrict__ tlo,
                                                            int *__restrict__ schild, u64 *__restrict__ shi, u64 *__restrict__ slo,
                                                            int *__restrict__ bad) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int off = (int)np;
    if (i < nt) {
        const int A = tets[i * 4], B = tets[i * 4 + 1], Cc = tets[i * 4 + 2], D = tets[i * 4 + 3];
        // every edge of a tetrahedron is in the list it was made from
        const int AB = off + edge_key_position(ek, ne, octo_edge_key(A, B, np)), AC = off + edge_key_position(ek, ne, octo_edge_key(A, Cc, np));
        const int AD = off + edge_key_position(ek, ne, octo_edge_key(A, D, np)), BC = off + edge_key_position(ek, ne, octo_edge_key(B, Cc, np));
        const int BD = off + edge_key_position(ek, ne, octo_edge_key(B, D, np)), CD = off + edge_key_position(ek, ne, octo_edge_key(Cc, D, np));
        const int64_t c = i * 8;
        octo_put_tet(tchild, thi, tlo, c, A, AB, AC, AD);
        octo_put_tet(tchild, thi, tlo, c + 1, B, AB, BC, BD);
        octo_put_tet(tchild, thi, tlo, c + 2, Cc, AC, BC, CD);
        octo_put_tet(tchild, thi, tlo, c + 3, D, AD, BD, CD);
        const double ab_cd = octo_dist2(pts, AB, CD), ac_bd = octo_dist2(pts, AC, BD), ad_bc = octo_dist2(pts, AD, BC);
        if (ab_cd <= ac_bd && ab_cd <= ad_bc) {
            octo_put_tet(tchild, thi, tlo, c + 4, AB, CD, AC, AD);
            octo_put_tet(tchild, thi, tlo, c + 5, AB, CD, AD, BD);
            octo_put_tet(tchild, thi, tlo, c + 6, AB, CD, BD, BC);
            octo_put_tet(tchild, thi, tlo, c + 7, AB, CD, BC, AC);
        } else if (ac_bd <= ab_cd && ac_bd <= ad_bc) {
            octo_put_tet(tchild, thi, tlo, c + 4, AC, BD, AB, AD);
            octo_put_tet(tchild, thi, tlo, c + 5, AC, BD, AD, CD);
            octo_put_tet(tchild, thi, tlo, c + 6, AC, BD, CD, BC);
            octo_put_tet(tchild, thi, tlo, c + 7, AC, BD, BC, AB);
        } else {
            octo_put_tet(tchild, thi, tlo, c + 4, AD, BC, AC, CD);
            octo_put_tet(tchild, thi, tlo, c + 5, AD, BC, CD, BD);
            octo_put_tet(tchild, thi, tlo, c + 6, AD, BC, BD, AB);
            octo_put_tet(tchild, thi, tlo, c + 7, AD, BC, AB, AC);
        }
    } else if (i < nt + ns) {
        const int64_t s = i - nt;
        const int A = tris[s * 3], B = tris[s * 3 + 1], Cc = tris[s * 3 + 2];
        const int e0 = edge_key_position(ek, ne, octo_edge_key(A, B, np)), e1 = edge_key_position(ek, ne, octo_edge_key(A, Cc, np));
        const int e2 = edge_key_position(ek, ne, octo_edge_key(B, Cc, np));
        const int64_t c = s * 4;
        if ((e0 | e1 | e2) < 0) {
            bad[0] = 1;
            for (int k = 0; k < 4; ++k) {
                shi[c + k] = 0; slo[c + k] = 0;
                schild[(c + k) * 3] = schild[(c + k) * 3 + 1] = schild[(c + k) * 3 + 2] = 0;
            }
            return;
        }
        const int AB = off + e0, AC = off + e1, BC = off + e2;
        octo_put_tri(schild, shi, slo, c, A, AB, AC);
        octo_put_tri(schild, shi, slo, c + 1, B, AB, BC);
        octo_put_tri(schild, shi, slo, c + 2, Cc, AC, BC);
        octo_put_tri(schild, shi, slo, c + 3, AB, AC, BC);
    }
}

__global__ __launch_bounds__(256) void octo_iota_kernel(int *__restrict__ idx, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) idx[i] = (int)i;
}

__global__ __launch_bounds__(256) void octo_gather_keys_kernel(const u64 *__restrict__ key, const int *__restrict__ idx, int64_t n, u64 *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = key[idx[i]];
}

// position p of the sorted list takes child order[p]; labels[order[p]] = p; bad[flag]: two neighbours of the sorted list with equal keys
template <int NV>
__global__ __launch_bounds__(256) void octo_place_kernel(const int *__restrict__ child, const int *__restrict__ order, const u64 *__restrict__ hi_sorted,
                                                         const u64 *__restrict__ lo, int64_t n, int *__restrict__ out, int *__restrict__ labels,
                                                         int *__restrict__ bad, int flag) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const int c = order[p];
#pragma unroll
    for (int k = 0; k < NV; ++k) out[p * NV + k] = child[(int64_t)c * NV + k];
    labels[c] = (int)p;
    if (p > 0 && hi_sorted[p] == hi_sorted[p - 1] && lo[c] == lo[order[p - 1]]) bad[flag] = 1;
}

// one level of the nested P1 embedding on column-major multivectors: rows < nold are copied, row nold + e = (x[a] + x[b]) * 0.5
__global__ __launch_bounds__(256) void octo_prolong_kernel(const cplx *__restrict__ X, int64_t nold, const int *__restrict__ parents, int64_t nnew,
                                                           int ncols, cplx *__restrict__ Y) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nnew) return;
    int a = 0, b = 0;
    if (i >= nold) {
        a = parents[(i - nold) * 2];
        b = parents[(i - nold) * 2 + 1];
    }
    for (int c = 0; c < ncols; ++c) {
        const cplx *x = X + (size_t)c * nold;
        cplx y;
        if (i < nold) y = x[i];
        else {
            const cplx xa = x[a], xb = x[b];
            y = cplx{(xa.x + xb.x) * 0.5, (xa.y + xb.y) * 0.5};
        }
        Y[(size_t)c * nnew + i] = y;
    }
}

// the same embedding as a CSR matrix (nnew x nold): row i < nold holds (i, 1), row nold + e holds (b, 0.5) (a, 0.5) with b < a, columns
// ascending; one thread per row, every entry written once
__global__ __launch_bounds__(256) void octo_prolongator_kernel(int64_t nold, const int *__restrict__ parents, int64_t nnew, int *__restrict__ ptr,
                                                               int *__restrict__ col, double *__restrict__ val) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > nnew) return;
    const int64_t p = i < nold ? i : nold + 2 * (i - nold);
    ptr[i] = (int)p;
    if (i == nnew) return;
    if (i < nold) {
        col[p] = (int)i;
        val[p] = 1.0;
    } else {
        const int a = parents[(i - nold) * 2], b = parents[(i - nold) * 2 + 1];
        col[p] = min(a, b); col[p + 1] = max(a, b);
        val[p] = 0.5; val[p + 1] = 0.5;
    }
}

// ---- P2 prolongation between two levels ------------------------------------------------------------------------------------------------
// The P2 unknowns of a level are its points, then its edges ascending by (smaller point, larger point) (p2_edge_key: the numbering of
// wae_p2_assemble).  A row of the prolongator is the coarse basis -- l_i (2 l_i - 1) on the points, 4 l_i l_j on the edges -- at the place of
// the fine unknown.  nc / nf: points of the coarse / fine level; fine point nc + k is the midpoint of parents[k] = (larger, smaller).
//   fine unknown                                   entries
//   old point a < nc                               (a, 1)
//   new point, midpoint of the coarse edge AB      (edge AB, 1)
//   fine edge (A, AB)                              (A, 3/8) (B, -1/8) (edge AB, 3/4)
//   fine edge (AB, AC)                             (B, -1/8) (C, -1/8) (edge AB, 1/2) (edge AC, 1/2) (edge BC, 1/4); A has weight 0: not stored
//   fine edge (AB, CD), an inner diagonal          the four points -1/8, the six edges among them 1/4
// Only the two ends of the fine edge, the parents table and binary searches in the coarse edge list are read; one thread per row, every
// entry written once, columns ascending (points before edges, either kind sorted).

// entries of the fine row i (0 for a row that no refinement produces: flagged by the fill kernel)
__device__ inline int octo_p2_row_length(int64_t i, int64_t nc, int64_t nf, const u64 *__restrict__ ekf, const int *__restrict__ parents) {
    if (i < nf) return 1;
    const u64 k = ekf[i - nf], u = k / (u64)nf, v = k - u * (u64)nf;          // u < v
    if (v < (u64)nc) return 0;
    if (u < (u64)nc) return 3;
    const int a1 = parents[(u - nc) * 2], b1 = parents[(u - nc) * 2 + 1], a2 = parents[(v - nc) * 2], b2 = parents[(v - nc) * 2 + 1];
    return (a1 == a2 || a1 == b2 || b1 == a2 || b1 == b2) ? 5 : 10;
}

// len[i] for the ndof rows, len[ndof] = 0: the exclusive scan of ndof + 1 values ends with the entry count
__global__ __launch_bounds__(256) void octo_p2_count_kernel(int64_t nc, int64_t nf, int64_t ndof, const u64 *__restrict__ ekf,
                                                            const int *__restrict__ parents, long long *__restrict__ len) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > ndof) return;
    len[i] = i < ndof ? octo_p2_row_length(i, nc, nf, ekf, parents) : 0;
}

// M distinct columns with their weights, written in ascending column order (position = number of smaller columns)
template <int M> __device__ inline void octo_p2_put(int *__restrict__ col, double *__restrict__ val, const int (&c)[M], const double (&w)[M]) {
#pragma unroll
    for (int j = 0; j < M; ++j) {
        int r = 0;
#pragma unroll
        for (int k = 0; k < M; ++k) r += c[k] < c[j];
        col[r] = c[j];
        val[r] = w[j];
    }
}

// bad[0]: a pair of points that is no coarse edge, or a fine edge that no refinement produces (the row is then filled with column 0)
__global__ __launch_bounds__(256) void octo_p2_fill_kernel(int64_t nc, int64_t nf, int64_t ndof, const u64 *__restrict__ ekc, int64_t nec,
                                                           const u64 *__restrict__ ekf, const int *__restrict__ parents,
                                                           const long long *__restrict__ ptr64, int *__restrict__ ptr, int *__restrict__ col,
                                                           double *__restrict__ val, int *__restrict__ bad) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > ndof) return;
    const long long p = ptr64[i];
    ptr[i] = (int)p;
    if (i == ndof) return;
    int *cp = col + p;
    double *vp = val + p;
    auto edge = [&](int a, int b) {                     // the coarse unknown of edge (a, b)
        int e = p2_find_edge(ekc, nec, (u64)nc, a, b);
        if (e < 0) { bad[0] = 1; e = -(int)nc; }
        return (int)nc + e;
    };
    if (i < nc) {
        cp[0] = (int)i; vp[0] = 1.0;
        return;
    }
    if (i < nf) {
        cp[0] = edge(parents[(i - nc) * 2], parents[(i - nc) * 2 + 1]); vp[0] = 1.0;
        return;
    }
    const u64 k = ekf[i - nf], uu = k / (u64)nf, vv = k - uu * (u64)nf;
    if (vv < (u64)nc) { bad[0] = 1; return; }           // (its length is 0)
    const int a2 = parents[(vv - nc) * 2], b2 = parents[(vv - nc) * 2 + 1];
    if (uu < (u64)nc) {
        const int A = (int)uu, B = a2 == A ? b2 : a2;
        if (a2 != A && b2 != A) bad[0] = 1;
        const int c[3] = {A, B, edge(a2, b2)};
        const double w[3] = {0.375, -0.125, 0.75};
        octo_p2_put<3>(cp, vp, c, w);
        return;
    }
    const int a1 = parents[(uu - nc) * 2], b1 = parents[(uu - nc) * 2 + 1];
    if (a1 == a2 || a1 == b2 || b1 == a2 || b1 == b2) {
        const int A = (a1 == a2 || a1 == b2) ? a1 : b1, B = a1 + b1 - A, Cc = a2 + b2 - A;
        const int c[5] = {B, Cc, edge(A, B), edge(A, Cc), edge(B, Cc)};
        const double w[5] = {-0.125, -0.125, 0.5, 0.5, 0.25};
        octo_p2_put<5>(cp, vp, c, w);
        return;
    }
    const int c[10] = {a1, b1, a2, b2, edge(a1, b1), edge(a1, a2), edge(a1, b2), edge(b1, a2), edge(b1, b2), edge(a2, b2)};
    const double w[10] = {-0.125, -0.125, -0.125, -0.125, 0.25, 0.25, 0.25, 0.25, 0.25, 0.25};
    octo_p2_put<10>(cp, vp, c, w);
}

// Y = P X on column-major multivectors, P the real CSR step above (rows of 1, 3, 5 or 10 entries): one thread per fine row, the lanes
// of a wave on consecutive rows, so that the col / val reads and the store of a column coalesce; a thread reads its row once into
// registers and loops over the columns, gathering 16-byte values of X (the coarse vector is 1/8 of the fine one and stays in L2).
// Rows longer than 10 entries (no octosplit step has one) finish from memory.
constexpr int OCTO_P2_ROW = 10;
__global__ __launch_bounds__(256) void octo_p2_apply_kernel(const int *__restrict__ ptr, const int *__restrict__ col, const double *__restrict__ val,
                                                            int64_t nrow, int64_t nin, int ncols, const cplx *__restrict__ X, cplx *__restrict__ Y) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nrow) return;
    const int p0 = ptr[i], len = ptr[i + 1] - p0;
    int cj[OCTO_P2_ROW];
    double vj[OCTO_P2_ROW];
#pragma unroll
    for (int k = 0; k < OCTO_P2_ROW; ++k) {
        cj[k] = k < len ? col[p0 + k] : 0;
        vj[k] = k < len ? val[p0 + k] : 0.0;
    }
    for (int c = 0; c < ncols; ++c) {
        const cplx *x = X + (size_t)c * nin;
        double re = 0.0, im = 0.0;
#pragma unroll
        for (int k = 0; k < OCTO_P2_ROW; ++k)
            if (k < len) {
                const cplx xv = x[cj[k]];
                re = fma(vj[k], xv.x, re);
                im = fma(vj[k], xv.y, im);
            }
        for (int k = OCTO_P2_ROW; k < len; ++k) {
            const cplx xv = x[col[p0 + k]];
            re = fma(val[p0 + k], xv.x, re);
            im = fma(val[p0 + k], xv.y, im);
        }
        Y[(size_t)c * nrow + i] = cplx{re, im};
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
struct OctoLevel {
    int64_t np = 0, nt = 0, ns = 0;
    DevBuf<double> pts;
    DevBuf<int> tets, tris;
    DevBuf<int> parents, tet_labels, tri_labels;     // empty on level 0
};
// the P2 space of a level and the prolongator to the next one, made by the first P2 call on the handle (octo_p2_build)
struct OctoP2Level {
    int64_t ne = 0, ndof = 0, nnz = 0;               // edges; points + edges; entries of the step level -> level + 1 (0 on the last level)
    DevBuf<u64> ek;                                  // the edges: sorted keys smaller * npoints + larger
    DevBuf<int> ptr, col;                            // the step as CSR, ndof(level + 1) rows
    DevBuf<double> val;
};
struct Octo {
    int device = 0;
    std::vector<OctoLevel> lv;
    std::vector<OctoP2Level> p2;                     // empty until a P2 entry is called
};

// children (n of them, NV vertices each, with their keys) -> the sorted list `out` and the labels; bad[flag] set on equal neighbours
template <int NV>
void octo_sort_children(int64_t n, const int *child, u64 *hi, u64 *lo, int end_bit_hi, int end_bit_lo, int *out, int *labels, int *bad, int flag) {
    if (!n) return;
    const int cnt = (int)n;
    Dev<int> i0((size_t)n), i1((size_t)n), i2((size_t)n);
    Dev<u64> k1((size_t)n), k2((size_t)n);
    hipLaunchKernelGGL(octo_iota_kernel, grid_for(n), dim3(256), 0, 0, i0.p, n);
    HIP_CHECK(hipGetLastError());
    auto by_lo = [&](void *t, size_t &b) { return hipcub::DeviceRadixSort::SortPairs(t, b, lo, k1.p, i0.p, i1.p, cnt, 0, end_bit_lo); };
    auto by_hi = [&](void *t, size_t &b) { return hipcub::DeviceRadixSort::SortPairs(t, b, k2.p, k1.p, i1.p, i2.p, cnt, 0, end_bit_hi); };
    DevBuf<char> tmp;
    cub_reserve(tmp, by_lo, by_hi);
    cub_run(by_lo, tmp);
    hipLaunchKernelGGL(octo_gather_keys_kernel, grid_for(n), dim3(256), 0, 0, hi, i1.p, n, k2.p);
    HIP_CHECK(hipGetLastError());
    cub_run(by_hi, tmp);
    hipLaunchKernelGGL(octo_place_kernel<NV>, grid_for(n), dim3(256), 0, 0, child, i2.p, k1.p, lo, n, out, labels, bad, flag);
    HIP_CHECK(hipGetLastError());
}

void octo_refine(const OctoLevel &in, OctoLevel &out, int level) {
    const int64_t np = in.np, nt = in.nt, ns = in.ns;
    const std::string at = " (level " + std::to_string(level) + ")";
    if (nt * 8 > INT_MAX || ns * 4 > INT_MAX) throw WaeError(WAE_ERR_INVALID, "8*ntets or 4*ntris does not fit a 32-bit index" + at);
    const int nk = (int)(nt * 6);
    Dev<u64> k0((size_t)nk), ek((size_t)nk);
    Dev<int> bad(3);
    hipLaunchKernelGGL(octo_edge_keys_kernel, grid_for(nt), dim3(256), 0, 0, in.tets.p, nt, (u64)np, k0.p);
    HIP_CHECK(hipGetLastError());
    const int ne = sorted_unique_keys(k0, nk, key_bits((u64)np * (u64)np), ek);
    if (np + (int64_t)ne > INT_MAX) throw WaeError(WAE_ERR_INVALID, "npoints + nedges does not fit a 32-bit index" + at);
    out.np = np + ne; out.nt = nt * 8; out.ns = ns * 4;
    out.pts.alloc((size_t)out.np * 3);
    out.tets.alloc((size_t)out.nt * 4);
    out.tris.alloc((size_t)out.ns * 3);
    out.parents.alloc((size_t)ne * 2);
    out.tet_labels.alloc((size_t)out.nt);
    out.tri_labels.alloc((size_t)out.ns);
    HIP_CHECK(hipMemcpy(out.pts.p, in.pts.p, (size_t)np * 3 * sizeof(double), hipMemcpyDeviceToDevice));
    hipLaunchKernelGGL(octo_midpoints_kernel, grid_for(ne), dim3(256), 0, 0, ek.p, (int64_t)ne, (u64)np, out.pts.p, out.parents.p);
    HIP_CHECK(hipGetLastError());
    Dev<int> tchild((size_t)out.nt * 4), schild((size_t)out.ns * 3);
    Dev<u64> thi((size_t)out.nt), tlo((size_t)out.nt), shi((size_t)out.ns), slo((size_t)out.ns);
    HIP_CHECK(hipMemset(bad.p, 0, 3 * sizeof(int)));
    hipLaunchKernelGGL(octo_children_kernel, grid_for(nt + ns), dim3(256), 0, 0, in.tets.p, nt, in.tris.p, ns, ek.p, (int64_t)ne, (u64)np, out.pts.p,
                       tchild.p, thi.p, tlo.p, schild.p, shi.p, slo.p, bad.p);
    HIP_CHECK(hipGetLastError());
    const int vb = key_bits((u64)out.np);          // bits of a point number of the new level
    octo_sort_children<4>(out.nt, tchild.p, thi.p, tlo.p, 31 + vb, 31 + vb, out.tets.p, out.tet_labels.p, bad.p, 1);
    octo_sort_children<3>(out.ns, schild.p, shi.p, slo.p, 31 + vb, vb, out.tris.p, out.tri_labels.p, bad.p, 2);
    int hbad[3] = {0, 0, 0};
    bad.to_host(hbad, 3);
    if (hbad[0]) throw WaeError(WAE_ERR_INVALID, "a boundary triangle has an edge that is no tetrahedron's edge" + at);
    if (hbad[1]) throw WaeError(WAE_ERR_INVALID, "two children of the tetrahedra are equal: a tetrahedron is listed twice or repeats a point" + at);
    if (hbad[2]) throw WaeError(WAE_ERR_INVALID, "two children of the triangles are equal: a triangle is listed twice or repeats a point" + at);
}

const OctoLevel &octo_level(const void *h, int32_t level) {
    if (!h) throw WaeError(WAE_ERR_INVALID, "null handle");
    const Octo *H = (const Octo *)h;
    if (level < 0 || level >= (int32_t)H->lv.size()) throw WaeError(WAE_ERR_INVALID, "level outside 0..levels");
    return H->lv[(size_t)level];
}

// the step l -> l + 1: row lengths by kind, an exclusive scan, one thread per row to fill it
void octo_p2_step(const OctoLevel &F, const OctoLevel &T, const OctoP2Level &cf, const OctoP2Level &ct, OctoP2Level &out, int level) {
    const std::string at = " (P2 prolongator of level " + std::to_string(level) + ")";
    const int64_t nd = ct.ndof;
    if (nd + 1 > INT_MAX) throw WaeError(WAE_ERR_INVALID, "npoints + nedges + 1 does not fit a 32-bit index" + at);
    DevBuf<long long> len, ptr64;
    len.alloc((size_t)nd + 1); ptr64.alloc((size_t)nd + 1);
    hipLaunchKernelGGL(octo_p2_count_kernel, grid_for(nd + 1), dim3(256), 0, 0, F.np, T.np, nd, ct.ek.p, T.parents.p, len.p);
    HIP_CHECK(hipGetLastError());
    DevBuf<char> tmp;
    exclusive_sum(len.p, ptr64.p, (int)(nd + 1), tmp);
    long long nnz = 0;
    ptr64.to_host(&nnz, 1, (size_t)nd);
    if (nnz < nd || nnz > 10 * nd) throw WaeError(WAE_ERR_HIP, "P2 prolongator: the scan returned an impossible entry count" + at);
    if (nnz > INT_MAX) throw WaeError(WAE_ERR_INVALID, "the prolongator's entries do not fit a 32-bit index" + at);
    out.nnz = nnz;
    out.ptr.alloc((size_t)nd + 1); out.col.alloc((size_t)nnz); out.val.alloc((size_t)nnz);
    Dev<int> bad(1);
    HIP_CHECK(hipMemset(bad.p, 0, sizeof(int)));
    hipLaunchKernelGGL(octo_p2_fill_kernel, grid_for(nd + 1), dim3(256), 0, 0, F.np, T.np, nd, cf.ek.p, cf.ne, ct.ek.p, T.parents.p, ptr64.p,
                       out.ptr.p, out.col.p, out.val.p, bad.p);
    HIP_CHECK(hipGetLastError());
    int hbad = 0;
    bad.to_host(&hbad, 1);
    if (hbad) throw WaeError(WAE_ERR_HIP, "P2 prolongator: an edge of the finer level does not come from the coarser one" + at);
}

// The first P2 call on a handle: the edges of every level (keys, sort and unique pass of wae_p2_connectivity: p2_edge_list) and every
// step's prolongator, kept in HBM.  Nothing is kept if a level is refused.
const std::vector<OctoP2Level> &octo_p2(Octo *H) {
    if (!H->p2.empty()) return H->p2;
    const size_t nl = H->lv.size();
    std::vector<OctoP2Level> p2(nl);
    for (size_t l = 0; l < nl; ++l) {
        const OctoLevel &L = H->lv[l];
        if (L.nt > INT_MAX / 6) throw WaeError(WAE_ERR_INVALID, "6*ntets does not fit a 32-bit index (P2 edges of level " + std::to_string(l) + ")");
        Dev<u64> ek((size_t)L.nt * 6);
        p2[l].ne = p2_edge_list(L.np, L.nt, L.tets.p, ek);          // (refuses npoints + nedges beyond a 32-bit index)
        p2[l].ndof = L.np + p2[l].ne;
        p2[l].ek.alloc((size_t)p2[l].ne);
        HIP_CHECK(hipMemcpy(p2[l].ek.p, ek.p, (size_t)p2[l].ne * sizeof(u64), hipMemcpyDeviceToDevice));
    }
    for (size_t l = 0; l + 1 < nl; ++l) octo_p2_step(H->lv[l], H->lv[l + 1], p2[l], p2[l + 1], p2[l], (int)l);
    H->p2 = std::move(p2);
    return H->p2;
}

}  // namespace

extern "C" {

int wae_octosplit_p2_info(void *h, int32_t level, int64_t *nedges, int64_t *ndof, int64_t *prolongator_nnz) {
    return wae_guarded([&]() {
        (void)octo_level(h, level);
        Octo *H = (Octo *)h;
        HIP_CHECK(hipSetDevice(H->device));
        const OctoP2Level &P = octo_p2(H)[(size_t)level];
        if (nedges) *nedges = P.ne;
        if (ndof) *ndof = P.ndof;
        if (prolongator_nnz) *prolongator_nnz = P.nnz;
        return WAE_OK;
    });
}

int wae_octosplit_prolongator_p2(void *h, int32_t from_level, int32_t *ptr, int32_t *col, double *val) {
    return wae_guarded([&]() {
        (void)octo_level(h, from_level);
        Octo *H = (Octo *)h;
        if (from_level + 1 >= (int32_t)H->lv.size()) throw WaeError(WAE_ERR_INVALID, "from_level must be below the last level");
        if (!(ptr && col && val)) throw WaeError(WAE_ERR_INVALID, "bad argument");
        HIP_CHECK(hipSetDevice(H->device));
        const std::vector<OctoP2Level> &p2 = octo_p2(H);
        const OctoP2Level &P = p2[(size_t)from_level];
        P.ptr.to_host(ptr, (size_t)p2[(size_t)from_level + 1].ndof + 1);
        P.col.to_host(col, (size_t)P.nnz);
        P.val.to_host(val, (size_t)P.nnz);
        return WAE_OK;
    });
}

int wae_octosplit_prolong_p2(void *h, int32_t from_level, int32_t to_level, int32_t ncols, const double *X, double *Y) {
    return wae_guarded([&]() {
        (void)octo_level(h, from_level);
        (void)octo_level(h, to_level);
        if (from_level >= to_level) throw WaeError(WAE_ERR_INVALID, "prolongation needs from_level < to_level");
        if (!(X && Y) || ncols < 1) throw WaeError(WAE_ERR_INVALID, "bad argument");
        Octo *H = (Octo *)h;
        HIP_CHECK(hipSetDevice(H->device));
        const std::vector<OctoP2Level> &p2 = octo_p2(H);
        DevBuf<cplx> a, b;                                  // the intermediate levels stay here
        const size_t nin = (size_t)p2[(size_t)from_level].ndof * (size_t)ncols;
        a.from_host((const cplx *)X, nin);
        for (int32_t l = from_level; l < to_level; ++l) {
            const OctoP2Level &P = p2[(size_t)l];
            const int64_t nrow = p2[(size_t)l + 1].ndof;
            b.alloc((size_t)nrow * (size_t)ncols);
            hipLaunchKernelGGL(octo_p2_apply_kernel, grid_for(nrow), dim3(256), 0, 0, P.ptr.p, P.col.p, P.val.p, nrow, P.ndof, (int)ncols, a.p, b.p);
            HIP_CHECK(hipGetLastError());
            std::swap(a, b);
        }
        a.to_host((cplx *)Y, (size_t)p2[(size_t)to_level].ndof * (size_t)ncols);
        return WAE_OK;
    });
}

int wae_octosplit(int32_t device, int64_t npoints, const double *points, int64_t ntets, const int32_t *tets, int64_t ntris, const int32_t *tris,
                  int32_t levels, void **out) {
    return wae_guarded([&]() {
        if (!(out && points && npoints > 0 && ntets > 0 && tets && ntris >= 0 && (ntris == 0 || tris))) throw WaeError(WAE_ERR_INVALID, "bad argument");
        if (levels < 1) throw WaeError(WAE_ERR_INVALID, "levels must be at least 1");
        // the tetrahedron and triangle counts of every level are known in advance (the point counts are checked as the edges are counted):
        // nothing is allocated for a call that cannot finish
        if (npoints > INT_MAX) throw WaeError(WAE_ERR_INVALID, "npoints does not fit a 32-bit index");
        for (int64_t l = 0, nt = ntets, ns = ntris; l < levels; ++l, nt *= 8, ns *= 4)
            if (nt > INT_MAX / 8 || ns > INT_MAX / 4)
                throw WaeError(WAE_ERR_INVALID, "8^levels * ntets or 4^levels * ntris does not fit a 32-bit index");
        check_tets(tets, ntets, npoints);
        check_tris(tris, ntris, npoints);
        HIP_CHECK(hipSetDevice(device));
        std::unique_ptr<Octo> H(new Octo);
        H->device = device;
        H->lv.resize((size_t)levels + 1);
        OctoLevel &L0 = H->lv[0];
        L0.np = npoints; L0.nt = ntets; L0.ns = ntris;
        L0.pts.from_host(points, (size_t)npoints * 3);
        L0.tets.from_host(tets, (size_t)ntets * 4);
        L0.tris.from_host(tris, (size_t)ntris * 3);
        for (int32_t l = 1; l <= levels; ++l) octo_refine(H->lv[(size_t)l - 1], H->lv[(size_t)l], l);
        *out = H.release();
        return WAE_OK;
    });
}

int wae_octosplit_info(const void *h, int32_t level, int64_t *npoints, int64_t *ntets, int64_t *ntris) {
    return wae_guarded([&]() {
        const OctoLevel &L = octo_level(h, level);
        if (npoints) *npoints = L.np;
        if (ntets) *ntets = L.nt;
        if (ntris) *ntris = L.ns;
        return WAE_OK;
    });
}

int wae_octosplit_get(const void *h, int32_t level, double *points, int32_t *tets, int32_t *tris, int32_t *parents, int32_t *tet_labels,
                      int32_t *tri_labels) {
    return wae_guarded([&]() {
        const OctoLevel &L = octo_level(h, level);
        if (level == 0 && (parents || tet_labels || tri_labels)) throw WaeError(WAE_ERR_INVALID, "level 0 is the input: it has no parents and no labels");
        HIP_CHECK(hipSetDevice(((const Octo *)h)->device));
        L.pts.to_host(points, (size_t)L.np * 3);
        L.tets.to_host(tets, (size_t)L.nt * 4);
        L.tris.to_host(tris, (size_t)L.ns * 3);
        if (level > 0) {
            const OctoLevel &P = octo_level(h, level - 1);
            L.parents.to_host(parents, (size_t)(L.np - P.np) * 2);
            L.tet_labels.to_host(tet_labels, (size_t)L.nt);
            L.tri_labels.to_host(tri_labels, (size_t)L.ns);
        }
        return WAE_OK;
    });
}

int wae_octosplit_prolong(const void *h, int32_t from_level, int32_t to_level, int32_t ncols, const double *X, double *Y) {
    return wae_guarded([&]() {
        const OctoLevel &F = octo_level(h, from_level);
        const OctoLevel &T = octo_level(h, to_level);
        if (from_level >= to_level) throw WaeError(WAE_ERR_INVALID, "prolongation needs from_level < to_level");
        if (!(X && Y) || ncols < 1) throw WaeError(WAE_ERR_INVALID, "bad argument");
        const Octo *H = (const Octo *)h;
        HIP_CHECK(hipSetDevice(H->device));
        DevBuf<cplx> a, b;                                  // the intermediate levels stay here
        a.from_host((const cplx *)X, (size_t)F.np * (size_t)ncols);
        for (int32_t l = from_level + 1; l <= to_level; ++l) {
            const OctoLevel &P = H->lv[(size_t)l - 1], &L = H->lv[(size_t)l];
            b.alloc((size_t)L.np * (size_t)ncols);
            hipLaunchKernelGGL(octo_prolong_kernel, grid_for(L.np), dim3(256), 0, 0, a.p, P.np, L.parents.p, L.np, (int)ncols, b.p);
            HIP_CHECK(hipGetLastError());
            std::swap(a, b);
        }
        a.to_host((cplx *)Y, (size_t)T.np * (size_t)ncols);
        return WAE_OK;
    });
}

int wae_octosplit_prolongator(const void *h, int32_t from_level, int32_t *ptr, int32_t *col, double *val) {
    return wae_guarded([&]() {
        const OctoLevel &F = octo_level(h, from_level);
        if (from_level + 1 >= (int32_t)((const Octo *)h)->lv.size()) throw WaeError(WAE_ERR_INVALID, "from_level must be below the last level");
        const OctoLevel &T = octo_level(h, from_level + 1);
        if (!(ptr && col && val)) throw WaeError(WAE_ERR_INVALID, "bad argument");
        const int64_t nnz = 2 * T.np - F.np;
        if (nnz > INT_MAX) throw WaeError(WAE_ERR_INVALID, "the prolongator's entries do not fit a 32-bit index");
        HIP_CHECK(hipSetDevice(((const Octo *)h)->device));
        DevBuf<int> dptr, dcol;
        DevBuf<double> dval;
        dptr.alloc((size_t)T.np + 1); dcol.alloc((size_t)nnz); dval.alloc((size_t)nnz);
        hipLaunchKernelGGL(octo_prolongator_kernel, grid_for(T.np + 1), dim3(256), 0, 0, F.np, T.parents.p, T.np, dptr.p, dcol.p, dval.p);
        HIP_CHECK(hipGetLastError());
        dptr.to_host(ptr, (size_t)T.np + 1);
        dcol.to_host(col, (size_t)nnz);
        dval.to_host(val, (size_t)nnz);
        return WAE_OK;
    });
}

int wae_octosplit_free(void *h) {
    if (h) (void)hipSetDevice(((Octo *)h)->device);
    delete (Octo *)h;
    return WAE_OK;
}

}  // extern "C"
