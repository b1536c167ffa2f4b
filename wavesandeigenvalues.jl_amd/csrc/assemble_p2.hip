// P2 (second-order) tetrahedral assembly of the Helmholtz operators on the device: `discretize(...; order=:quad)` of the reference
// (src/Helmholtz.jl:36-54) for the interior, admittance-boundary and flame domains.
//
//   1. Edge numbering (aggregate_elements, src/FEM/FEM.jl:84-116; collect_lines!, Meshutils.jl:831-840): one kernel writes the six
//      keys min(v_i,v_j)*npoints + max(v_i,v_j) of every tetrahedron, a radix sort and a unique pass (hipCUB) leave the edge list
//      in lexicographic order, a second kernel finds every local edge of every tetrahedron and boundary triangle in it by binary
//      search.  DoF of edge e = npoints + e.
//   2. Element kernels, one thread per (simplex, local row): 10 (tetrahedron) or 6 (triangle) triplets of that row.  A thread keeps
//      no array that it indexes by its row number: what depends on the row is read from the basis tables in constant memory.
//   3. triplets_to_csr (assemble.hip): stable sort, reduce-by-key, row pointer -- deterministic, no atomics.
// The gradients of the barycentric coordinates, |det J| of the flame tetrahedra and the flame set-up: tet_geometry.h.
//
// Basis (barycentric coordinates l_1..l_n, n = 4 or 3): vertex functions l_i (2 l_i - 1), edge functions 4 l_i l_j, local order
// vertices first, then the edges (1,2), (1,3), (1,4), (2,3), (2,4), (3,4) resp. (1,2), (1,3), (2,3).  With sum l = 1 every function is
// a homogeneous quadratic form  phi_a = 1/2 sum_kl q2[a][k][l] l_k l_l  with integer q2, and the monomial formula
//     int l^alpha = |det J| prod(alpha_i!) / (|alpha| + n - 1)!
// gives every local matrix exactly: the tables below are made from it at compile time, none is copied from anywhere.
#include <algorithm>
#include <climits>
#include <memory>
#include <vector>

#include "edge_keys.h"
#include "tet_geometry.h"

namespace {

typedef unsigned long long u64;

template <int NV> struct P2Basis {
    static constexpr int NN = NV + NV * (NV - 1) / 2;
    double mass[NN][NN];      // int phi_a phi_b / |det J|
    double src[NN];           // int phi_a / |det J|
    double d[NN][NV][NV];     // d phi_a / d l_i = sum_k d[a][i][k] l_k
};

constexpr long long p2_factorial(int n) { return n <= 1 ? 1 : n * p2_factorial(n - 1); }

// phi_a = 1/2 sum_kl q2[a][k][l] l_k l_l
template <int NV> constexpr void p2_quadratic_forms(int (&q2)[NV + NV * (NV - 1) / 2][NV][NV]) {
    for (int a = 0; a < NV; ++a)                  // l_a (2 l_a - sum_k l_k) = l_a^2 - sum_{k != a} l_a l_k
        for (int k = 0; k < NV; ++k) {
            if (k == a) q2[a][a][a] = 2;
            else q2[a][a][k] = q2[a][k][a] = -1;
        }
    int a = NV;
    for (int i = 0; i < NV; ++i)
        for (int j = i + 1; j < NV; ++j, ++a) q2[a][i][j] = q2[a][j][i] = 4;      // 4 l_i l_j
}

template <int NV> constexpr P2Basis<NV> make_p2_basis() {
    constexpr int NN = P2Basis<NV>::NN;
    int q2[NN][NV][NV] = {};
    p2_quadratic_forms<NV>(q2);
    P2Basis<NV> B = {};
    for (int r = 0; r < NN; ++r) {
        long long s = 0;
        for (int k = 0; k < NV; ++k)
            for (int l = 0; l < NV; ++l) s += q2[r][k][l] * (k == l ? 2 : 1);
        B.src[r] = (double)s / (double)(2 * p2_factorial(NV + 1));
        for (int c = 0; c < NN; ++c) {
            long long num = 0;
            for (int k = 0; k < NV; ++k)
                for (int l = 0; l < NV; ++l)
                    for (int m = 0; m < NV; ++m)
                        for (int n = 0; n < NV; ++n) {
                            if (q2[r][k][l] == 0 || q2[c][m][n] == 0) continue;
                            int cnt[NV] = {};
                            ++cnt[k]; ++cnt[l]; ++cnt[m]; ++cnt[n];
                            long long mono = 1;
                            for (int v = 0; v < NV; ++v) mono *= p2_factorial(cnt[v]);
                            num += (long long)q2[r][k][l] * q2[c][m][n] * mono;
                        }
            B.mass[r][c] = (double)num / (double)(4 * p2_factorial(NV + 3));
        }
        for (int i = 0; i < NV; ++i)
            for (int k = 0; k < NV; ++k) B.d[r][i][k] = (double)q2[r][i][k];
    }
    return B;
}

constexpr P2Basis<4> kTet = make_p2_basis<4>();
constexpr P2Basis<3> kTri = make_p2_basis<3>();
__constant__ P2Basis<4> dTet = kTet;
__constant__ P2Basis<3> dTri = kTri;

// Tables of the nodal speed of sound, c(x) = sum_p c_p l_p on every simplex (the *_cpoint entries), from the same monomial formula.
//   quart[km][pq] = (2 - delta_pq) int l_k l_m l_p l_q / |det J|  on the tetrahedron (denominator 7!), the unordered pairs k <= m and
//                   p <= q numbered (0,0), (0,1), (0,2), (0,3), (1,1), (1,2), (1,3), (2,2), (2,3), (3,3):
//                   W_km = int c^2 l_k l_m / |det J| = sum_{p<=q} c_p c_q quart[km][pq]
//   tri[p][a][b]  = int l_p phi_a phi_b / |(x0-x2) x (x1-x2)|  on the 6-node triangle (degree 5, denominator 7!)
struct P2NodalC {
    double quart[10][10];
    double tri[3][6][6];
};

constexpr P2NodalC make_p2_nodal_c() {
    P2NodalC T = {};
    int km = 0;
    for (int k = 0; k < 4; ++k)
        for (int m = k; m < 4; ++m, ++km) {
            int pq = 0;
            for (int p = 0; p < 4; ++p)
                for (int q = p; q < 4; ++q, ++pq) {
                    int cnt[4] = {};
                    ++cnt[k]; ++cnt[m]; ++cnt[p]; ++cnt[q];
                    long long mono = p == q ? 1 : 2;
                    for (int v = 0; v < 4; ++v) mono *= p2_factorial(cnt[v]);
                    T.quart[km][pq] = (double)mono / (double)p2_factorial(7);
                }
        }
    int q2[6][3][3] = {};
    p2_quadratic_forms<3>(q2);
    for (int p = 0; p < 3; ++p)
        for (int r = 0; r < 6; ++r)
            for (int c = 0; c < 6; ++c) {
                long long num = 0;
                for (int k = 0; k < 3; ++k)
                    for (int l = 0; l < 3; ++l)
                        for (int m = 0; m < 3; ++m)
                            for (int n = 0; n < 3; ++n) {
                                int cnt[3] = {};
                                ++cnt[p]; ++cnt[k]; ++cnt[l]; ++cnt[m]; ++cnt[n];
                                long long mono = 1;
                                for (int v = 0; v < 3; ++v) mono *= p2_factorial(cnt[v]);
                                num += (long long)q2[r][k][l] * q2[c][m][n] * mono;
                            }
                T.tri[p][r][c] = (double)num / (double)(4 * p2_factorial(7));
            }
    return T;
}

constexpr P2NodalC kNodalC = make_p2_nodal_c();
__constant__ P2NodalC dNodalC = kNodalC;

// Speaker source vector with the nodal speed of sound:  srcc[p][a] = int l_p phi_a / |(x0-x2) x (x1-x2)|  on the 6-node triangle (degree 3,
// denominator 5!), from the same quadratic forms:  s_a = |..| sum_p c_p srcc[p][a]
struct P2SourceC {
    double tri[3][6];
};

constexpr P2SourceC make_p2_source_c() {
    P2SourceC S = {};
    int q2[6][3][3] = {};
    p2_quadratic_forms<3>(q2);
    for (int p = 0; p < 3; ++p)
        for (int a = 0; a < 6; ++a) {
            long long num = 0;
            for (int k = 0; k < 3; ++k)
                for (int l = 0; l < 3; ++l) {
                    int cnt[3] = {};
                    ++cnt[p]; ++cnt[k]; ++cnt[l];
                    long long mono = 1;
                    for (int v = 0; v < 3; ++v) mono *= p2_factorial(cnt[v]);
                    num += (long long)q2[a][k][l] * mono;
                }
            S.tri[p][a] = (double)num / (double)(2 * p2_factorial(5));
        }
    return S;
}

constexpr P2SourceC kSourceC = make_p2_source_c();
__constant__ P2SourceC dSourceC = kSourceC;

// grad phi = sum_k l_k w[k] with w[k] = sum_i d[i][k] grad l_i; s = sum_k w[k].  One fixed order of operations, so that the row's and
// the column's function get the same bits and K_ab == K_ba.
__host__ __device__ inline void p2_grad_coeffs(const double d[4][4], const double G[4][3], double w[4][3], double s[3]) {
    for (int c = 0; c < 3; ++c) s[c] = 0.0;
    for (int k = 0; k < 4; ++k)
        for (int c = 0; c < 3; ++c) {
            double x = d[0][k] * G[0][c];
            for (int i = 1; i < 4; ++i) x = fma(d[i][k], G[i][c], x);
            w[k][c] = x;
            s[c] += x;
        }
}

// ---- edge numbering ------------------------------------------------------------------------------------------------------------
// (p2_edge_key and p2_find_edge: edge_keys.h)
__global__ __launch_bounds__(256) void p2_edge_keys_kernel(const int *__restrict__ tets, int64_t nt, u64 np, u64 *__restrict__ keys) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= nt) return;
    const int v0 = tets[t * 4], v1 = tets[t * 4 + 1], v2 = tets[t * 4 + 2], v3 = tets[t * 4 + 3];
    u64 *k = keys + t * 6;
    k[0] = p2_edge_key(v0, v1, np); k[1] = p2_edge_key(v0, v2, np); k[2] = p2_edge_key(v0, v3, np);
    k[3] = p2_edge_key(v1, v2, np); k[4] = p2_edge_key(v1, v3, np); k[5] = p2_edge_key(v2, v3, np);
}

// threads 0..nt-1: 10-node connectivity of a tetrahedron; nt..nt+ns-1: 6-node connectivity of a boundary triangle.
// bad[0] / bad[1]: a tetrahedron / a triangle with an edge that is not in the list (its node is written as -1)
__global__ __launch_bounds__(256) void p2_connect_kernel(const int *__restrict__ tets, int64_t nt, const int *__restrict__ tris, int64_t ns,
                                                         const u64 *__restrict__ ek, int64_t ne, u64 np, int *__restrict__ t10,
                                                         int *__restrict__ s6, int *__restrict__ bad) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < nt) {
        const int v0 = tets[i * 4], v1 = tets[i * 4 + 1], v2 = tets[i * 4 + 2], v3 = tets[i * 4 + 3];
        const int e0 = p2_find_edge(ek, ne, np, v0, v1), e1 = p2_find_edge(ek, ne, np, v0, v2), e2 = p2_find_edge(ek, ne, np, v0, v3);
        const int e3 = p2_find_edge(ek, ne, np, v1, v2), e4 = p2_find_edge(ek, ne, np, v1, v3), e5 = p2_find_edge(ek, ne, np, v2, v3);
        int *o = t10 + i * 10;
        const int off = (int)np;
        o[0] = v0; o[1] = v1; o[2] = v2; o[3] = v3;
        o[4] = e0 < 0 ? -1 : off + e0; o[5] = e1 < 0 ? -1 : off + e1; o[6] = e2 < 0 ? -1 : off + e2;
        o[7] = e3 < 0 ? -1 : off + e3; o[8] = e4 < 0 ? -1 : off + e4; o[9] = e5 < 0 ? -1 : off + e5;
        if ((e0 | e1 | e2 | e3 | e4 | e5) < 0) bad[0] = 1;
    } else if (i < nt + ns) {
        const int64_t s = i - nt;
        const int v0 = tris[s * 3], v1 = tris[s * 3 + 1], v2 = tris[s * 3 + 2];
        const int e0 = p2_find_edge(ek, ne, np, v0, v1), e1 = p2_find_edge(ek, ne, np, v0, v2), e2 = p2_find_edge(ek, ne, np, v1, v2);
        int *o = s6 + s * 6;
        const int off = (int)np;
        o[0] = v0; o[1] = v1; o[2] = v2;
        o[3] = e0 < 0 ? -1 : off + e0; o[4] = e1 < 0 ? -1 : off + e1; o[5] = e2 < 0 ? -1 : off + e2;
        if ((e0 | e1 | e2) < 0) bad[1] = 1;
    }
}

__global__ __launch_bounds__(256) void p2_edge_pairs_kernel(const u64 *__restrict__ ek, int64_t ne, u64 np, int *__restrict__ edges) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= ne) return;
    const u64 k = ek[e], lo = k / np;
    edges[e * 2] = (int)lo;
    edges[e * 2 + 1] = (int)(k - lo * np);
}

// the embedding of the P1 space into the P2 space of the same mesh as CSR (np + ne rows, np columns): the row of point a holds (a, 1), the
// row of edge (a, b), a < b, holds (a, 1/2) (b, 1/2) -- a P1 function at the P2 nodes; one thread per row, and one for ptr[np + ne]
__global__ __launch_bounds__(256) void p2_embedding_kernel(int64_t np, const int *__restrict__ edges, int64_t ne, int *__restrict__ ptr,
                                                           int *__restrict__ col, double *__restrict__ val) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > np + ne) return;
    const int64_t p = i < np ? i : np + 2 * (i - np);
    ptr[i] = (int)p;
    if (i == np + ne) return;
    if (i < np) {
        col[p] = (int)i;
        val[p] = 1.0;
    } else {
        col[p] = edges[(i - np) * 2]; col[p + 1] = edges[(i - np) * 2 + 1];
        val[p] = 0.5; val[p + 1] = 0.5;
    }
}

// ---- element kernels -------------------------------------------------------------------------------------------------------------
// row a of the local matrices of tetrahedron t:  M_ab = |det J| int phi_a phi_b,   K_ab = -c^2 |det J| int grad phi_a . grad phi_b  with
// int l_k l_l = (1 + delta_kl)/120:   K_ab = -c^2 |det J|/120 (s_a . s_b + sum_k w_a[k] . w_b[k])
__global__ __launch_bounds__(256) void p2_local_kernel(const double *__restrict__ pts, const int *__restrict__ t10, const double *__restrict__ c_tet,
                                                       int64_t nt, u64 dim, u64 *__restrict__ keys, double *__restrict__ mv, double *__restrict__ kv) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= nt * 10) return;
    const int64_t t = e / 10;
    const int a = (int)(e - t * 10);
    int nd[10];
#pragma unroll
    for (int b = 0; b < 10; ++b) nd[b] = t10[t * 10 + b];
    double X[4][3], G[4][3];
#pragma unroll
    for (int v = 0; v < 4; ++v)
        for (int k = 0; k < 3; ++k) X[v][k] = pts[(size_t)nd[v] * 3 + k];
    const double adet = fabs(tet_gradients(X, G));
    const double c = c_tet ? c_tet[t] : 1.0;
    const double ks = -(c * c) * adet / 120.0;
    double wa[4][3], sa[3];
    p2_grad_coeffs(dTet.d[a], G, wa, sa);
    const u64 row = (u64)t10[t * 10 + a] * dim;
#pragma unroll
    for (int b = 0; b < 10; ++b) {
        double wb[4][3], sb[3];
        p2_grad_coeffs(dTet.d[b], G, wb, sb);
        double acc = sa[0] * sb[0];
        acc = fma(sa[1], sb[1], acc);
        acc = fma(sa[2], sb[2], acc);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            for (int x = 0; x < 3; ++x) acc = fma(wa[k][x], wb[k][x], acc);
        const size_t o = (size_t)e * 10 + b;
        keys[o] = row + (u64)nd[b];
        mv[o] = adet * dTet.mass[a][b];
        kv[o] = ks * acc;
    }
}

// row a of the boundary mass of triangle t: b_ab = c |(x0-x2) x (x1-x2)| int phi_a phi_b on the 6-node triangle
__global__ __launch_bounds__(256) void p2_boundary_kernel(const double *__restrict__ pts, const int *__restrict__ s6, const double *__restrict__ c_tri,
                                                          int64_t ns, u64 dim, u64 *__restrict__ keys, double *__restrict__ bv) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= ns * 6) return;
    const int64_t t = e / 6;
    const int a = (int)(e - t * 6);
    int nd[6];
#pragma unroll
    for (int b = 0; b < 6; ++b) nd[b] = s6[t * 6 + b];
    double X[3][3];
#pragma unroll
    for (int v = 0; v < 3; ++v)
        for (int k = 0; k < 3; ++k) X[v][k] = pts[(size_t)nd[v] * 3 + k];
    const double u0 = X[0][0] - X[2][0], u1 = X[0][1] - X[2][1], u2 = X[0][2] - X[2][2];
    const double w0 = X[1][0] - X[2][0], w1 = X[1][1] - X[2][1], w2 = X[1][2] - X[2][2];
    const double n0 = u1 * w2 - u2 * w1, n1 = u2 * w0 - u0 * w2, n2 = u0 * w1 - u1 * w0;
    const double cd = (c_tri ? c_tri[t] : 1.0) * sqrt(n0 * n0 + n1 * n1 + n2 * n2);
    const u64 row = (u64)s6[t * 6 + a] * dim;
#pragma unroll
    for (int b = 0; b < 6; ++b) {
        const size_t o = (size_t)e * 6 + b;
        keys[o] = row + (u64)nd[b];
        bv[o] = cd * dTri.mass[a][b];
    }
}

// ---- element kernels, speed of sound given at the mesh points ---------------------------------------------------------------------------
// c(x) = sum_p c_p l_p with the 4 (3) corner values of the simplex (generate_field(...; order=:lin); s43nv2nu2cc1 and s33v2u2c1 of the
// reference, Helmholtz.jl:59-74,120-171).  Every integral is a polynomial in l and exact: no quadrature.
//
// row a of tetrahedron t, M as in p2_local_kernel and, with grad phi_a = sum_k l_k w_a[k] and the symmetric W_km = int c^2 l_k l_m / |det J|,
//     K_ab = -|det J| sum_{k<=m} d_km W_km,   d_kk = w_a[k].w_b[k],   d_km = w_a[k].w_b[m] + w_a[m].w_b[k]  (k < m).
// Every dot product runs in one fixed order and d_km adds the two of a pair first, so K_ab and K_ba get the same bits -- as long as the
// compiler rounds where the source does.  Two contractions would break that, and both are shut out:
//  - of one dot product of a pair into the other's fma chain (fadd (fma x, y, (fmul u, v)), z -> fma x, y, (fma u, v, z)), which of the
//    two depending on the side: contract(off) in this kernel;
//  - of grad l_i = cofactor / det J into the sums of p2_grad_coeffs: for the column's function b is a constant, the compiler knows the
//    table entries (0, -1, 2, 4), turns fma(-1, G, x) into x - G and fuses the product that made G into it, while the row's function,
//    picked at run time, keeps the rounded G.  The gradients therefore pass through p2_opaque before they are used.
__device__ inline double p2_opaque(double x) {
    asm volatile("" : "+v"(x));          // no instruction: only hides where x came from
    return x;
}
__device__ inline double p2_dot3(const double x[3], const double y[3]) {
#pragma clang fp contract(off)
    return fma(x[2], y[2], fma(x[1], y[1], x[0] * y[0]));
}

__global__ __launch_bounds__(256) void p2_local_cpoint_kernel(const double *__restrict__ pts, const int *__restrict__ t10,
                                                              const double *__restrict__ c_point, int64_t nt, u64 dim, u64 *__restrict__ keys,
                                                              double *__restrict__ mv, double *__restrict__ kv) {
#pragma clang fp contract(off)
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= nt * 10) return;
    const int64_t t = e / 10;
    const int a = (int)(e - t * 10);
    int nd[10];
#pragma unroll
    for (int b = 0; b < 10; ++b) nd[b] = t10[t * 10 + b];
    double X[4][3], G[4][3], cc[10], W[10];
#pragma unroll
    for (int v = 0; v < 4; ++v)
        for (int k = 0; k < 3; ++k) X[v][k] = pts[(size_t)nd[v] * 3 + k];
    {
        double c[4];
#pragma unroll
        for (int v = 0; v < 4; ++v) c[v] = c_point[nd[v]];
        int pq = 0;
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int q = p; q < 4; ++q, ++pq) cc[pq] = c[p] * c[q];
    }
#pragma unroll
    for (int km = 0; km < 10; ++km) {
        double x = cc[0] * dNodalC.quart[km][0];
#pragma unroll
        for (int pq = 1; pq < 10; ++pq) x = fma(cc[pq], dNodalC.quart[km][pq], x);
        W[km] = x;
    }
    const double nadet = -fabs(tet_gradients(X, G));
#pragma unroll
    for (int v = 0; v < 4; ++v)
        for (int k = 0; k < 3; ++k) G[v][k] = p2_opaque(G[v][k]);
    double wa[4][3], sa[3];
    p2_grad_coeffs(dTet.d[a], G, wa, sa);
    const u64 row = (u64)t10[t * 10 + a] * dim;
#pragma unroll
    for (int b = 0; b < 10; ++b) {
        double wb[4][3], sb[3];
        p2_grad_coeffs(dTet.d[b], G, wb, sb);
        double acc = 0.0;
        int km = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int m = k; m < 4; ++m, ++km) {
                const double d = k == m ? p2_dot3(wa[k], wb[k]) : p2_dot3(wa[k], wb[m]) + p2_dot3(wa[m], wb[k]);
                acc = km == 0 ? d * W[0] : fma(d, W[km], acc);
            }
        const size_t o = (size_t)e * 10 + b;
        keys[o] = row + (u64)nd[b];
        mv[o] = -nadet * dTet.mass[a][b];
        kv[o] = nadet * acc;
    }
}

// row a of triangle t: b_ab = |(x0-x2) x (x1-x2)| sum_p c_p int l_p phi_a phi_b; the table is symmetric in (a, b) and p runs in one order
__global__ __launch_bounds__(256) void p2_boundary_cpoint_kernel(const double *__restrict__ pts, const int *__restrict__ s6,
                                                                 const double *__restrict__ c_point, int64_t ns, u64 dim, u64 *__restrict__ keys,
                                                                 double *__restrict__ bv) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= ns * 6) return;
    const int64_t t = e / 6;
    const int a = (int)(e - t * 6);
    int nd[6];
#pragma unroll
    for (int b = 0; b < 6; ++b) nd[b] = s6[t * 6 + b];
    double X[3][3];
#pragma unroll
    for (int v = 0; v < 3; ++v)
        for (int k = 0; k < 3; ++k) X[v][k] = pts[(size_t)nd[v] * 3 + k];
    const double c0 = c_point[nd[0]], c1 = c_point[nd[1]], c2 = c_point[nd[2]];
    const double u0 = X[0][0] - X[2][0], u1 = X[0][1] - X[2][1], u2 = X[0][2] - X[2][2];
    const double w0 = X[1][0] - X[2][0], w1 = X[1][1] - X[2][1], w2 = X[1][2] - X[2][2];
    const double n0 = u1 * w2 - u2 * w1, n1 = u2 * w0 - u0 * w2, n2 = u0 * w1 - u1 * w0;
    const double det = sqrt(n0 * n0 + n1 * n1 + n2 * n2);
    const u64 row = (u64)s6[t * 6 + a] * dim;
#pragma unroll
    for (int b = 0; b < 6; ++b) {
        const size_t o = (size_t)e * 6 + b;
        keys[o] = row + (u64)nd[b];
        bv[o] = det * fma(c2, dNodalC.tri[2][a][b], fma(c1, dNodalC.tri[1][a][b], c0 * dNodalC.tri[0][a][b]));
    }
}

// node a of the speaker source vector of triangle t (wallsrc of the reference divided by i, Helmholtz.jl:488-505):
//     s_a = |(x0-x2) x (x1-x2)| int c(x) phi_a,   c per triangle (c_tri, NULL = 1) or linear between the corner values (nodal).
// One (node, value) pair per thread, key = node * dim (column 0 of triplets_to_csr); p runs in one order.
__global__ __launch_bounds__(256) void p2_source_kernel(const double *__restrict__ pts, const int *__restrict__ s6, const double *__restrict__ c, int nodal,
                                                        int64_t ns, u64 dim, u64 *__restrict__ keys, double *__restrict__ sv) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= ns * 6) return;
    const int64_t t = e / 6;
    const int a = (int)(e - t * 6);
    int nd[3];
    double X[3][3];
#pragma unroll
    for (int v = 0; v < 3; ++v) {
        nd[v] = s6[t * 6 + v];
        for (int k = 0; k < 3; ++k) X[v][k] = pts[(size_t)nd[v] * 3 + k];
    }
    const double u0 = X[0][0] - X[2][0], u1 = X[0][1] - X[2][1], u2 = X[0][2] - X[2][2];
    const double w0 = X[1][0] - X[2][0], w1 = X[1][1] - X[2][1], w2 = X[1][2] - X[2][2];
    const double n0 = u1 * w2 - u2 * w1, n1 = u2 * w0 - u0 * w2, n2 = u0 * w1 - u1 * w0;
    const double det = sqrt(n0 * n0 + n1 * n1 + n2 * n2);
    keys[e] = (u64)s6[t * 6 + a] * dim;
    if (nodal) sv[e] = det * fma(c[nd[2]], dSourceC.tri[2][a], fma(c[nd[1]], dSourceC.tri[1][a], c[nd[0]] * dSourceC.tri[0][a]));
    else sv[e] = (c ? c[t] : 1.0) * det * dTri.src[a];
}

// Q triplets: (node a of flame tetrahedron i, node b of the reference tetrahedron) -> |det J_i| int phi_a * g_b
__global__ __launch_bounds__(256) void p2_flame_kernel(const int *__restrict__ t10, const int *__restrict__ list, int64_t n, const double *__restrict__ adet,
                                                       int ref_tet, const double *__restrict__ g, u64 dim, u64 *__restrict__ keys, double *__restrict__ qv) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n * 10) return;
    const int64_t i = e / 10;
    const int a = (int)(e - i * 10);
    const int64_t t = list[i];
    const double s = adet[i] * dTet.src[a];
    const u64 row = (u64)t10[t * 10 + a] * dim;
#pragma unroll
    for (int b = 0; b < 10; ++b) {
        const size_t o = (size_t)e * 10 + b;
        keys[o] = row + (u64)t10[(int64_t)ref_tet * 10 + b];
        qv[o] = s * g[b];
    }
}

// ---- discrete-adjoint shape sensitivity ------------------------------------------------------------------------------------------------
// -v_adj^H (L+ - L-)/(2h) v of src/shape_sensitivity.jl:16-141 for P2 elements, L+- the operator re-discretised with one corner of the
// simplex moved by +-h.  Straight-sided elements: everything but |det J| and the four grad l_i is independent of the geometry, so a thread
// contracts the element tensors with its 10 (6) vector entries once and differences only the geometric factors.  With x = v_loc,
// y = v_adj_loc, xi_ik = sum_b d[b][i][k] x_b (grad u = sum_k l_k sum_i xi_ik grad l_i), eta likewise for y, and the symmetric
// W_km = int c^2 l_k l_m / |det J|  (c per tetrahedron: c^2 (1 + delta_km)/120; nodal c: the quart table of p2_local_cpoint_kernel):
//     y^H M x = |det J| (y^H Mhat x),        y^H K x = -sum_ij T_ij (|det J| grad l_i . grad l_j),   T_ij = sum_km W_km conj(eta_ik) xi_jm
// Only p2_shape_geometry is evaluated at +-h.  Every array below is indexed by unrolled loop counters only: the moved corner a0 and the
// coordinate enter through selects, never through an index.
__device__ constexpr int p2_sym(int k, int m) { return k <= m ? k * 4 - k * (k - 1) / 2 + (m - k) : m * 4 - m * (m - 1) / 2 + (k - m); }

__device__ inline cplx p2_cmul(cplx a, cplx b) { return cplx{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }

// gg[p2_sym(i, j)] = |det J| grad l_i . grad l_j of the tetrahedron X with corner a0 moved by d along coordinate CRD; returns |det J|
template <int CRD> __device__ inline double p2_shape_geometry(const double X[4][3], int a0, double d, double gg[10]) {
    double Xd[4][3], G[4][3];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int k = 0; k < 3; ++k) Xd[a][k] = (k == CRD && a == a0) ? X[a][k] + d : X[a][k];
    const double adet = fabs(tet_gradients(Xd, G));
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = i; j < 4; ++j) gg[p2_sym(i, j)] = adet * fma(G[i][2], G[j][2], fma(G[i][1], G[j][1], G[i][0] * G[j][0]));
    return adet;
}

// -[w^2 mq (|det J|+ - |det J|-) - sum_ij Ts_ij (gg+ - gg-)_ij] / (2h) for one coordinate
template <int CRD> __device__ inline cplx p2_shape_tet_term(const double X[4][3], int a0, double h, cplx w2mq, const cplx Ts[10]) {
    double gp[10], gm[10];
    const double dp = p2_shape_geometry<CRD>(X, a0, h, gp), dm = p2_shape_geometry<CRD>(X, a0, -h, gm);
    const double dd = dp - dm;
    cplx acc = {w2mq.x * dd, w2mq.y * dd};
#pragma unroll
    for (int ij = 0; ij < 10; ++ij) {
        const double g = gp[ij] - gm[ij];
        acc.x = fma(-Ts[ij].x, g, acc.x);
        acc.y = fma(-Ts[ij].y, g, acc.y);
    }
    const double s = -1.0 / (2.0 * h);
    return cplx{acc.x * s, acc.y * s};
}

// one thread per (surface point, tetrahedron) pair: out[3 pr + crd], zero if the point is no corner of the tetrahedron.
// c: per tetrahedron (NULL = 1) or, NODAL, per mesh point
template <bool NODAL>
__global__ __launch_bounds__(256) void p2_shape_tet_kernel(const double *__restrict__ pts, const int *__restrict__ t10, const double *__restrict__ c,
                                                           int64_t npair, const int *__restrict__ pair_pt, const int *__restrict__ pair_tet, double wr,
                                                           double wi, const cplx *__restrict__ v, const cplx *__restrict__ vadj, double h,
                                                           cplx *__restrict__ out) {
    const int64_t pr = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (pr >= npair) return;
    const int64_t t = pair_tet[pr];
    const int p = pair_pt[pr];
    int nd[10];
#pragma unroll
    for (int b = 0; b < 10; ++b) nd[b] = t10[t * 10 + b];
    double X[4][3];
    int a0 = -1;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        if (nd[a] == p) a0 = a;
#pragma unroll
        for (int k = 0; k < 3; ++k) X[a][k] = pts[(size_t)nd[a] * 3 + k];
    }
    if (a0 < 0) {
        out[pr * 3] = out[pr * 3 + 1] = out[pr * 3 + 2] = cplx{0.0, 0.0};
        return;
    }
    double W[10];
    if (NODAL) {
        double c4[4], cc[10];
#pragma unroll
        for (int a = 0; a < 4; ++a) c4[a] = c[nd[a]];
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int m = k; m < 4; ++m) cc[p2_sym(k, m)] = c4[k] * c4[m];
#pragma unroll
        for (int km = 0; km < 10; ++km) {
            double s = cc[0] * dNodalC.quart[km][0];
#pragma unroll
            for (int pq = 1; pq < 10; ++pq) s = fma(cc[pq], dNodalC.quart[km][pq], s);
            W[km] = s;
        }
    } else {
        const double ct = c ? c[t] : 1.0;
        const double c2 = ct * ct / 120.0;
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int m = k; m < 4; ++m) W[p2_sym(k, m)] = k == m ? 2.0 * c2 : c2;
    }
    cplx x[10], yc[10];                                            // yc = conj(v_adj_loc)
#pragma unroll
    for (int b = 0; b < 10; ++b) {
        x[b] = v[nd[b]];
        const cplx y = vadj[nd[b]];
        yc[b] = cplx{y.x, -y.y};
    }
    cplx mq = {0.0, 0.0};                                          // y^H Mhat x
#pragma unroll
    for (int a = 0; a < 10; ++a) {
        cplx s = {0.0, 0.0};
#pragma unroll
        for (int b = 0; b < 10; ++b) {
            s.x = fma(dTet.mass[a][b], x[b].x, s.x);
            s.y = fma(dTet.mass[a][b], x[b].y, s.y);
        }
        const cplx q = p2_cmul(yc[a], s);
        mq.x += q.x; mq.y += q.y;
    }
    cplx eta[4][4], Z[4][4];                                       // conj(eta_ik);  Z_jk = sum_m W_km xi_jm
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        cplx xi[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            cplx sx = {0.0, 0.0}, sy = {0.0, 0.0};
#pragma unroll
            for (int b = 0; b < 10; ++b) {
                const double d = dTet.d[b][i][k];
                sx.x = fma(d, x[b].x, sx.x); sx.y = fma(d, x[b].y, sx.y);
                sy.x = fma(d, yc[b].x, sy.x); sy.y = fma(d, yc[b].y, sy.y);
            }
            xi[k] = sx;
            eta[i][k] = sy;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            cplx s = {0.0, 0.0};
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                s.x = fma(W[p2_sym(k, m)], xi[m].x, s.x);
                s.y = fma(W[p2_sym(k, m)], xi[m].y, s.y);
            }
            Z[i][k] = s;
        }
    }
    cplx Ts[10];                                                   // T_ij + T_ji (i < j), T_ii
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = i; j < 4; ++j) {
            cplx s = {0.0, 0.0};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const cplx q = p2_cmul(eta[i][k], Z[j][k]);
                s.x += q.x; s.y += q.y;
                if (i != j) {
                    const cplx r = p2_cmul(eta[j][k], Z[i][k]);
                    s.x += r.x; s.y += r.y;
                }
            }
            Ts[p2_sym(i, j)] = s;
        }
    const cplx w2mq = p2_cmul(cplx{wr * wr - wi * wi, 2.0 * wr * wi}, mq);
    out[pr * 3] = p2_shape_tet_term<0>(X, a0, h, w2mq, Ts);
    out[pr * 3 + 1] = p2_shape_tet_term<1>(X, a0, h, w2mq, Ts);
    out[pr * 3 + 2] = p2_shape_tet_term<2>(X, a0, h, w2mq, Ts);
}

// |(x0-x2) x (x1-x2)| of the triangle X with corner a0 moved by d along coordinate CRD
template <int CRD> __device__ inline double p2_shape_area2(const double X[3][3], int a0, double d) {
    double Xd[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int k = 0; k < 3; ++k) Xd[a][k] = (k == CRD && a == a0) ? X[a][k] + d : X[a][k];
    const double u0 = Xd[0][0] - Xd[2][0], u1 = Xd[0][1] - Xd[2][1], u2 = Xd[0][2] - Xd[2][2];
    const double w0 = Xd[1][0] - Xd[2][0], w1 = Xd[1][1] - Xd[2][1], w2 = Xd[1][2] - Xd[2][2];
    const double n0 = u1 * w2 - u2 * w1, n1 = u2 * w0 - u0 * w2, n2 = u0 * w1 - u1 * w0;
    return sqrt(n0 * n0 + n1 * n1 + n2 * n2);
}

// admittance boundary, operator term w Y C with C = -i b:  -(w Y)(-i) (y^H Bhat x) (|..|+ - |..|-)/(2h), Bhat = c int phi_a phi_b resp. the
// nodal table of p2_boundary_cpoint_kernel.  One thread per (surface point, triangle) pair.
template <bool NODAL>
__global__ __launch_bounds__(256) void p2_shape_tri_kernel(const double *__restrict__ pts, const int *__restrict__ s6, const double *__restrict__ c,
                                                           int64_t npair, const int *__restrict__ pair_pt, const int *__restrict__ pair_tri, double wyr,
                                                           double wyi, const cplx *__restrict__ v, const cplx *__restrict__ vadj, double h,
                                                           cplx *__restrict__ out) {
    const int64_t pr = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (pr >= npair) return;
    const int64_t t = pair_tri[pr];
    const int p = pair_pt[pr];
    int nd[6];
#pragma unroll
    for (int b = 0; b < 6; ++b) nd[b] = s6[t * 6 + b];
    double X[3][3];
    int a0 = -1;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (nd[a] == p) a0 = a;
#pragma unroll
        for (int k = 0; k < 3; ++k) X[a][k] = pts[(size_t)nd[a] * 3 + k];
    }
    if (a0 < 0) {
        out[pr * 3] = out[pr * 3 + 1] = out[pr * 3 + 2] = cplx{0.0, 0.0};
        return;
    }
    double c0 = 1.0, c1 = 1.0, c2 = 1.0, ct = 1.0;
    if (NODAL) { c0 = c[nd[0]]; c1 = c[nd[1]]; c2 = c[nd[2]]; }
    else if (c) ct = c[t];
    cplx bq = {0.0, 0.0};                                          // y^H Bhat x
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        cplx s = {0.0, 0.0};
#pragma unroll
        for (int b = 0; b < 6; ++b) {
            const double m = NODAL ? fma(c2, dNodalC.tri[2][a][b], fma(c1, dNodalC.tri[1][a][b], c0 * dNodalC.tri[0][a][b])) : dTri.mass[a][b];
            const cplx xb = v[nd[b]];
            s.x = fma(m, xb.x, s.x);
            s.y = fma(m, xb.y, s.y);
        }
        const cplx y = vadj[nd[a]];
        const cplx q = p2_cmul(cplx{y.x, -y.y}, s);
        bq.x += q.x; bq.y += q.y;
    }
    const double s = ct / (2.0 * h);
    const double d0 = (p2_shape_area2<0>(X, a0, h) - p2_shape_area2<0>(X, a0, -h)) * s;
    const double d1 = (p2_shape_area2<1>(X, a0, h) - p2_shape_area2<1>(X, a0, -h)) * s;
    const double d2 = (p2_shape_area2<2>(X, a0, h) - p2_shape_area2<2>(X, a0, -h)) * s;
    const cplx f = p2_cmul(cplx{-wyi, wyr}, bq);                   // -(w Y)(-i) (y^H Bhat x)
    out[pr * 3] = cplx{f.x * d0, f.y * d0};
    out[pr * 3 + 1] = cplx{f.x * d1, f.y * d1};
    out[pr * 3 + 2] = cplx{f.x * d2, f.y * d2};
}

// Flame part (the P2 form of shape_flame_kernel, assemble.hip): per (surface point, flame tetrahedron) pair |det J| with the point moved by
// +h and -h along every coordinate (det_pm[pair][3][2]), and ssum = sum_a (int phi_a / |det J|) conj(v_adj_a) over the 10 nodes
template <int CRD> __device__ inline double p2_shape_adet(const double X[4][3], int a0, double d) {
    double Xd[4][3], G[4][3];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int k = 0; k < 3; ++k) Xd[a][k] = (k == CRD && a == a0) ? X[a][k] + d : X[a][k];
    return fabs(tet_gradients(Xd, G));
}

__global__ __launch_bounds__(256) void p2_shape_flame_kernel(const double *__restrict__ pts, const int *__restrict__ t10, int64_t npair,
                                                             const int *__restrict__ pair_pt, const int *__restrict__ pair_tet,
                                                             const cplx *__restrict__ vadj, double h, double *__restrict__ det_pm,
                                                             cplx *__restrict__ ssum) {
    const int64_t pr = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (pr >= npair) return;
    const int64_t t = pair_tet[pr];
    const int p = pair_pt[pr];
    int nd[10];
#pragma unroll
    for (int b = 0; b < 10; ++b) nd[b] = t10[t * 10 + b];
    double X[4][3];
    int a0 = -1;                                                   // no corner: a0 matches nothing and the six values are the undisplaced |det J|
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        if (nd[a] == p) a0 = a;
#pragma unroll
        for (int k = 0; k < 3; ++k) X[a][k] = pts[(size_t)nd[a] * 3 + k];
    }
    cplx sa = {0.0, 0.0};
#pragma unroll
    for (int b = 0; b < 10; ++b) {
        const cplx y = vadj[nd[b]];
        sa.x = fma(dTet.src[b], y.x, sa.x);
        sa.y = fma(-dTet.src[b], y.y, sa.y);
    }
    ssum[pr] = sa;
    double *o = det_pm + pr * 6;
    o[0] = p2_shape_adet<0>(X, a0, h); o[1] = p2_shape_adet<0>(X, a0, -h);
    o[2] = p2_shape_adet<1>(X, a0, h); o[3] = p2_shape_adet<1>(X, a0, -h);
    o[4] = p2_shape_adet<2>(X, a0, h); o[5] = p2_shape_adet<2>(X, a0, -h);
}

// sum_b (grad phi_b(x_ref) . n_ref) v_b on the 10 nodes of the reference tetrahedron with corner a0 moved by d along CRD (a0 < 0: as it
// is).  x_ref stays where it is, so its barycentric coordinates move with the tetrahedron:
//     grad phi_b(x_ref) = sum_k lam_k sum_i d[b][i][k] grad l_i,    sum_b (..) v_b = sum_k lam_k sum_i (grad l_i . n_ref) xi_ik
template <int CRD> __device__ inline cplx p2_shape_ref_value(const double X[4][3], int a0, double d, const double xr[3], const double n[3],
                                                             const cplx xi[4][4]) {
    double Xd[4][3], G[4][3], lam[4], gn[4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int k = 0; k < 3; ++k) Xd[a][k] = (k == CRD && a == a0) ? X[a][k] + d : X[a][k];
    tet_gradients(Xd, G);
    lam[3] = 1.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        lam[a] = G[a][0] * (xr[0] - Xd[3][0]) + G[a][1] * (xr[1] - Xd[3][1]) + G[a][2] * (xr[2] - Xd[3][2]);
        lam[3] -= lam[a];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) gn[i] = G[i][0] * n[0] + G[i][1] * n[1] + G[i][2] * n[2];
    cplx acc = {0.0, 0.0};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        cplx s = {0.0, 0.0};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            s.x = fma(gn[i], xi[i][k].x, s.x);
            s.y = fma(gn[i], xi[i][k].y, s.y);
        }
        acc.x = fma(lam[k], s.x, acc.x);
        acc.y = fma(lam[k], s.y, acc.y);
    }
    return acc;
}

// thread pr < npair: the six displaced values of the listed corner pair_pt[pr] (g_pm[pr][3][2]); thread npair: the undisplaced value g0
__global__ __launch_bounds__(64) void p2_shape_ref_kernel(const double *__restrict__ pts, const int *__restrict__ t10, int ref_tet, int64_t npair,
                                                          const int *__restrict__ pair_pt, double xr0, double xr1, double xr2, double n0, double n1,
                                                          double n2, const cplx *__restrict__ v, double h, cplx *__restrict__ g_pm,
                                                          cplx *__restrict__ g0) {
    const int64_t pr = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (pr > npair) return;
    const int p = pr < npair ? pair_pt[pr] : -1;
    int nd[10];
    cplx x[10];
#pragma unroll
    for (int b = 0; b < 10; ++b) {
        nd[b] = t10[(int64_t)ref_tet * 10 + b];
        x[b] = v[nd[b]];
    }
    double X[4][3];
    int a0 = -1;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        if (nd[a] == p) a0 = a;
#pragma unroll
        for (int k = 0; k < 3; ++k) X[a][k] = pts[(size_t)nd[a] * 3 + k];
    }
    cplx xi[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            cplx s = {0.0, 0.0};
#pragma unroll
            for (int b = 0; b < 10; ++b) {
                s.x = fma(dTet.d[b][i][k], x[b].x, s.x);
                s.y = fma(dTet.d[b][i][k], x[b].y, s.y);
            }
            xi[i][k] = s;
        }
    const double xr[3] = {xr0, xr1, xr2}, nr[3] = {n0, n1, n2};
    if (pr == npair) {
        *g0 = p2_shape_ref_value<0>(X, -1, 0.0, xr, nr, xi);
        return;
    }
    cplx *o = g_pm + pr * 6;
    o[0] = p2_shape_ref_value<0>(X, a0, h, xr, nr, xi); o[1] = p2_shape_ref_value<0>(X, a0, -h, xr, nr, xi);
    o[2] = p2_shape_ref_value<1>(X, a0, h, xr, nr, xi); o[3] = p2_shape_ref_value<1>(X, a0, -h, xr, nr, xi);
    o[4] = p2_shape_ref_value<2>(X, a0, h, xr, nr, xi); o[5] = p2_shape_ref_value<2>(X, a0, -h, xr, nr, xi);
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
struct P2Conn {
    int device = 0;
    int64_t npoints = 0, nedges = 0, ntets = 0, ntris = 0;
    std::vector<int> edges, tets10, tris6;
};

void p2_check_mesh(int64_t npoints, int64_t ntets, const int32_t *tets, int64_t ntris, const int32_t *tris) {
    if (!(npoints > 0 && ntets > 0 && tets && ntris >= 0 && (ntris == 0 || tris))) throw WaeError(WAE_ERR_INVALID, "bad argument");
    if (npoints > INT_MAX || ntets > INT_MAX / 100 || ntris > INT_MAX / 36)
        throw WaeError(WAE_ERR_INVALID, "mesh too large: 100*ntets and 36*ntris triplets must fit a 32-bit count");
    check_tets(tets, ntets, npoints);
    check_tris(tris, ntris, npoints);
}

// Edge list and connectivities of a mesh whose 4-node tetrahedra (and 3-node triangles, ns may be 0) are on the device.
// ek: room for 6*nt keys, on return the nedges sorted unique keys; t10: 10*nt; s6: 6*ns.  Returns nedges.
int64_t p2_connect(int64_t npoints, int64_t nt, const int *dtets, int64_t ns, const int *dtris, Dev<u64> &ek, Dev<int> &t10, Dev<int> &s6) {
    const int nk = (int)(nt * 6);
    Dev<u64> k0((size_t)nk);
    Dev<int> bad(2);
    hipLaunchKernelGGL(p2_edge_keys_kernel, grid_for(nt), dim3(256), 0, 0, dtets, nt, (u64)npoints, k0.p);
    HIP_CHECK(hipGetLastError());
    const int ne = sorted_unique_keys(k0, nk, key_bits((u64)npoints * (u64)npoints), ek);
    if (npoints + (int64_t)ne > INT_MAX) throw WaeError(WAE_ERR_INVALID, "npoints + nedges does not fit a 32-bit index");
    HIP_CHECK(hipMemset(bad.p, 0, 2 * sizeof(int)));
    hipLaunchKernelGGL(p2_connect_kernel, grid_for(nt + ns), dim3(256), 0, 0, dtets, nt, dtris, ns, ek.p, (int64_t)ne, (u64)npoints,
                       t10.p, s6.p, bad.p);
    HIP_CHECK(hipGetLastError());
    int hbad[2] = {0, 0};
    bad.to_host(hbad, 2);
    if (hbad[0]) throw WaeError(WAE_ERR_HIP, "edge list: an edge of a tetrahedron was not found");
    if (hbad[1]) throw WaeError(WAE_ERR_INVALID, "a boundary triangle has an edge that is no tetrahedron's edge");
    return ne;
}

// number of distinct edges, counted on the host (the entries that launch nothing for empty pair lists still check nv)
int64_t p2_host_edge_count(int64_t npoints, int64_t nt, const int32_t *tets) {
    std::vector<u64> keys;
    keys.reserve((size_t)nt * 6);
    for (int64_t t = 0; t < nt; ++t)
        for (int i = 0; i < 4; ++i)
            for (int j = i + 1; j < 4; ++j) {
                const int u = tets[t * 4 + i], v = tets[t * 4 + j];
                keys.push_back((u64)std::min(u, v) * (u64)npoints + (u64)std::max(u, v));
            }
    std::sort(keys.begin(), keys.end());
    return (int64_t)(std::unique(keys.begin(), keys.end()) - keys.begin());
}

// the mesh on the device with its P2 connectivity
struct P2Mesh {
    Dev<double> pts;
    Dev<int> tets, tris, t10, s6;
    Dev<u64> ek;
    int64_t nedges = 0, dim = 0;
    P2Mesh(int64_t npoints, const double *points, int64_t nt, const int32_t *htets, int64_t ns, const int32_t *htris)
        : pts(points, points ? (size_t)npoints * 3 : 0), tets(htets, (size_t)nt * 4), tris(htris, (size_t)ns * 3), t10((size_t)nt * 10), s6((size_t)ns * 6),
          ek((size_t)nt * 6) {
        nedges = p2_connect(npoints, nt, tets.p, ns, tris.p, ek, t10, s6);
        dim = npoints + nedges;
    }
};

// One half of wae_p2_shape_sensitivity (10-node tetrahedra with omega, 6-node triangles with omega Y) on the mesh in HBM: the (point, simplex) pairs
// and, unless the nodal field c_nodal is on the device already, the speed of sound per simplex (c: nc values, NULL = 1) go up, `kernel` runs
// with a thread per pair, out receives the 3 npair complex numbers.
typedef void (*P2ShapeKernel)(const double *, const int *, const double *, int64_t, const int *, const int *, double, double, const cplx *, const cplx *,
                              double, cplx *);
void p2_shape_half(P2ShapeKernel kernel, const Dev<double> &pts, const Dev<int> &nodes, const double *c_nodal, const double *c, size_t nc, int64_t npair,
                   const int32_t *pair_pt, const int32_t *pair_simplex, const double *w, const Dev<cplx> &dv, const Dev<cplx> &dva, double h, double *out) {
    Dev<int> dpp(pair_pt, (size_t)npair), dps(pair_simplex, (size_t)npair);
    Dev<double> dc(c, !c_nodal && c ? nc : 0);
    Dev<cplx> dout((size_t)npair * 3);
    hipLaunchKernelGGL(kernel, grid_for(npair), dim3(256), 0, 0, pts.p, nodes.p, c_nodal ? c_nodal : c ? dc.p : nullptr, npair, dpp.p, dps.p, w[0], w[1], dv.p,
                       dva.p, h, dout.p);
    HIP_CHECK(hipGetLastError());
    dout.to_host((cplx *)out, (size_t)npair * 3);
}

}  // namespace

// (declared in mesh_host.h: octosplit.hip numbers the new points of a level with it)
int sorted_unique_keys(Dev<unsigned long long> &k0, int nk, int bits, Dev<unsigned long long> &ek) {
    Dev<unsigned long long> k1((size_t)nk);
    Dev<int> dnum(1);
    auto sort = [&](void *t, size_t &b) { return hipcub::DeviceRadixSort::SortKeys(t, b, k0.p, k1.p, nk, 0, bits); };
    auto unique = [&](void *t, size_t &b) { return hipcub::DeviceSelect::Unique(t, b, k1.p, ek.p, dnum.p, nk); };
    DevBuf<char> tmp;
    cub_reserve(tmp, sort, unique);
    cub_run(sort, tmp);
    cub_run(unique, tmp);
    int ne = 0;
    dnum.to_host(&ne, 1);
    if (ne <= 0 || ne > nk) throw WaeError(WAE_ERR_HIP, "edge list: unique pass returned an impossible count");
    return ne;
}

// the sorted unique edge keys of a mesh whose tetrahedra are on the device (declared in wae_internal.h: bloch.hip numbers unit cells with them)
int64_t p2_edge_list(int64_t npoints, int64_t nt, const int *dtets, Dev<unsigned long long> &ek) {
    Dev<int> t10((size_t)nt * 10), s6(1);
    return p2_connect(npoints, nt, dtets, 0, nullptr, ek, t10, s6);
}
void p2_check_tets(int64_t npoints, int64_t ntets, const int32_t *tets) { p2_check_mesh(npoints, ntets, tets, 0, nullptr); }

extern "C" {

int wae_p2_connectivity(int32_t device, int64_t npoints, int64_t ntets, const int32_t *tets, int64_t ntris, const int32_t *tris, void **out) {
    return wae_guarded([&]() {
        if (!out) throw WaeError(WAE_ERR_INVALID, "bad argument");
        p2_check_mesh(npoints, ntets, tets, ntris, tris);
        HIP_CHECK(hipSetDevice(device));
        P2Mesh m(npoints, nullptr, ntets, tets, ntris, tris);
        std::unique_ptr<P2Conn> H(new P2Conn);
        H->device = device; H->npoints = npoints; H->nedges = m.nedges; H->ntets = ntets; H->ntris = ntris;
        H->edges.resize((size_t)m.nedges * 2); H->tets10.resize((size_t)ntets * 10); H->tris6.resize((size_t)ntris * 6);
        Dev<int> de((size_t)m.nedges * 2);
        hipLaunchKernelGGL(p2_edge_pairs_kernel, grid_for(m.nedges), dim3(256), 0, 0, m.ek.p, m.nedges, (u64)npoints, de.p);
        HIP_CHECK(hipGetLastError());
        de.to_host(H->edges.data(), H->edges.size());
        m.t10.to_host(H->tets10.data(), H->tets10.size());
        m.s6.to_host(H->tris6.data(), H->tris6.size());
        *out = H.release();
        return WAE_OK;
    });
}

int wae_p2_connectivity_info(const void *handle, int64_t *nedges, int64_t *ntets, int64_t *ntris) {
    return wae_guarded([&]() {
        if (!handle) throw WaeError(WAE_ERR_INVALID, "null handle");
        const P2Conn *H = (const P2Conn *)handle;
        if (nedges) *nedges = H->nedges;
        if (ntets) *ntets = H->ntets;
        if (ntris) *ntris = H->ntris;
        return WAE_OK;
    });
}

int wae_p2_connectivity_get(const void *handle, int32_t *edges, int32_t *tets10, int32_t *tris6) {
    return wae_guarded([&]() {
        if (!handle) throw WaeError(WAE_ERR_INVALID, "null handle");
        const P2Conn *H = (const P2Conn *)handle;
        if (edges) memcpy(edges, H->edges.data(), H->edges.size() * sizeof(int));
        if (tets10) memcpy(tets10, H->tets10.data(), H->tets10.size() * sizeof(int));
        if (tris6) memcpy(tris6, H->tris6.data(), H->tris6.size() * sizeof(int));
        return WAE_OK;
    });
}

int wae_p2_connectivity_free(void *handle) {
    delete (P2Conn *)handle;
    return WAE_OK;
}

int wae_p2_embedding(const void *handle, int64_t npoints, int32_t *ptr, int32_t *col, double *val) {
    return wae_guarded([&]() {
        if (!handle) throw WaeError(WAE_ERR_INVALID, "null handle");
        const P2Conn *H = (const P2Conn *)handle;
        if (npoints != H->npoints) throw WaeError(WAE_ERR_INVALID, "npoints is not the point count the connectivity was numbered with");
        if (!(ptr && col && val)) throw WaeError(WAE_ERR_INVALID, "bad argument");
        const int64_t np = H->npoints, ne = H->nedges, nnz = np + 2 * ne;
        if (nnz > INT_MAX) throw WaeError(WAE_ERR_INVALID, "the embedding's entries do not fit a 32-bit index");
        HIP_CHECK(hipSetDevice(H->device));
        Dev<int> de(H->edges.data(), (size_t)ne * 2), dptr((size_t)(np + ne + 1)), dcol((size_t)nnz);
        Dev<double> dval((size_t)nnz);
        hipLaunchKernelGGL(p2_embedding_kernel, grid_for(np + ne + 1), dim3(256), 0, 0, np, de.p, ne, dptr.p, dcol.p, dval.p);
        HIP_CHECK(hipGetLastError());
        dptr.to_host(ptr, (size_t)(np + ne + 1));
        dcol.to_host(col, (size_t)nnz);
        dval.to_host(val, (size_t)nnz);
        return WAE_OK;
    });
}

// c: per tetrahedron (NULL = 1), or per mesh point (nodal; required)
static int p2_assemble_interior(int32_t device, int64_t npoints, const double *points, int64_t ntets, const int32_t *tets, const double *c, bool nodal,
                                void **out) {
    return wae_guarded([&]() {
        if (!(points && out)) throw WaeError(WAE_ERR_INVALID, "bad argument");
        p2_check_mesh(npoints, ntets, tets, 0, nullptr);
        if (nodal) check_c_point(npoints, c);
        HIP_CHECK(hipSetDevice(device));
        P2Mesh m(npoints, points, ntets, tets, 0, nullptr);
        const size_t ne = (size_t)ntets * 100;
        Dev<double> dc(c, c ? (size_t)(nodal ? npoints : ntets) : 0), mv(ne), kv(ne);
        Dev<u64> k0(ne);
        const dim3 grid = grid_for(ntets * 10);
        if (nodal) hipLaunchKernelGGL(p2_local_cpoint_kernel, grid, dim3(256), 0, 0, m.pts.p, m.t10.p, dc.p, ntets, (u64)m.dim, k0.p, mv.p, kv.p);
        else hipLaunchKernelGGL(p2_local_kernel, grid, dim3(256), 0, 0, m.pts.p, m.t10.p, c ? dc.p : nullptr, ntets, (u64)m.dim, k0.p, mv.p, kv.p);
        HIP_CHECK(hipGetLastError());
        *out = triplets_to_csr(m.dim, ne, k0, mv, &kv);
        return WAE_OK;
    });
}

static int p2_assemble_boundary(int32_t device, int64_t npoints, const double *points, int64_t ntets, const int32_t *tets, int64_t ntris,
                                const int32_t *tris, const double *c, bool nodal, void **out) {
    return wae_guarded([&]() {
        if (!(points && out && ntris > 0)) throw WaeError(WAE_ERR_INVALID, "bad argument");
        p2_check_mesh(npoints, ntets, tets, ntris, tris);
        if (nodal) check_c_point(npoints, c);
        HIP_CHECK(hipSetDevice(device));
        P2Mesh m(npoints, points, ntets, tets, ntris, tris);
        const size_t ne = (size_t)ntris * 36;
        Dev<double> dc(c, c ? (size_t)(nodal ? npoints : ntris) : 0), bv(ne);
        Dev<u64> k0(ne);
        const dim3 grid = grid_for(ntris * 6);
        if (nodal) hipLaunchKernelGGL(p2_boundary_cpoint_kernel, grid, dim3(256), 0, 0, m.pts.p, m.s6.p, dc.p, ntris, (u64)m.dim, k0.p, bv.p);
        else hipLaunchKernelGGL(p2_boundary_kernel, grid, dim3(256), 0, 0, m.pts.p, m.s6.p, c ? dc.p : nullptr, ntris, (u64)m.dim, k0.p, bv.p);
        HIP_CHECK(hipGetLastError());
        *out = triplets_to_csr(m.dim, ne, k0, bv, nullptr);
        return WAE_OK;
    });
}

// c: per triangle (NULL = 1), or per mesh point (nodal; required).  nout is checked against the edge count of the device numbering, before
// the element kernel is launched.
static int p2_assemble_source(int32_t device, int64_t npoints, const double *points, int64_t ntets, const int32_t *tets, int64_t ntris,
                              const int32_t *tris, const double *c, bool nodal, double *out, int64_t nout) {
    return wae_guarded([&]() {
        if (!(points && out && ntris >= 0 && nout > 0)) throw WaeError(WAE_ERR_INVALID, "bad argument");
        p2_check_mesh(npoints, ntets, tets, ntris, tris);
        if (nodal) check_c_point(npoints, c);
        HIP_CHECK(hipSetDevice(device));
        P2Mesh m(npoints, points, ntets, tets, ntris, tris);
        if (nout != m.dim) throw WaeError(WAE_ERR_INVALID, "nout is not npoints + nedges");
        if (ntris == 0) {                                                     // an empty speaker domain: the zero vector
            std::fill(out, out + nout, 0.0);
            return WAE_OK;
        }
        const size_t ne = (size_t)ntris * 6;
        Dev<double> dc(c, c ? (size_t)(nodal ? npoints : ntris) : 0), sv(ne);
        Dev<u64> k0(ne);
        hipLaunchKernelGGL(p2_source_kernel, grid_for(ntris * 6), dim3(256), 0, 0, m.pts.p, m.s6.p, c ? dc.p : nullptr, nodal ? 1 : 0, ntris, (u64)m.dim, k0.p,
                           sv.p);
        HIP_CHECK(hipGetLastError());
        pairs_to_dense(m.dim, ne, k0, sv, out);
        return WAE_OK;
    });
}

int wae_p2_assemble_source(int32_t device, int64_t npoints, const double *points, int64_t ntets, const int32_t *tets, int64_t ntris,
                           const int32_t *tris, const double *c_tri, double *out, int64_t nout) {
    return p2_assemble_source(device, npoints, points, ntets, tets, ntris, tris, c_tri, false, out, nout);
}

int wae_p2_assemble_source_cpoint(int32_t device, int64_t npoints, const double *points, int64_t ntets, const int32_t *tets, int64_t ntris,
                                  const int32_t *tris, const double *c_point, double *out, int64_t nout) {
    return p2_assemble_source(device, npoints, points, ntets, tets, ntris, tris, c_point, true, out, nout);
}

int wae_p2_assemble(int32_t device, int64_t npoints, const double *points, int64_t ntets, const int32_t *tets, const double *c_tet, void **out) {
    return p2_assemble_interior(device, npoints, points, ntets, tets, c_tet, false, out);
}

int wae_p2_assemble_cpoint(int32_t device, int64_t npoints, const double *points, int64_t ntets, const int32_t *tets, const double *c_point, void **out) {
    return p2_assemble_interior(device, npoints, points, ntets, tets, c_point, true, out);
}

int wae_p2_assemble_boundary(int32_t device, int64_t npoints, const double *points, int64_t ntets, const int32_t *tets, int64_t ntris,
                             const int32_t *tris, const double *c_tri, void **out) {
    return p2_assemble_boundary(device, npoints, points, ntets, tets, ntris, tris, c_tri, false, out);
}

int wae_p2_assemble_boundary_cpoint(int32_t device, int64_t npoints, const double *points, int64_t ntets, const int32_t *tets, int64_t ntris,
                                    const int32_t *tris, const double *c_point, void **out) {
    return p2_assemble_boundary(device, npoints, points, ntets, tets, ntris, tris, c_point, true, out);
}

int wae_p2_assemble_flame(int32_t device, int64_t npoints, const double *points, int64_t ntets, const int32_t *tets, int64_t nflame,
                          const int32_t *flame_tets, int32_t ref_tet, const double *x_ref, const double *n_ref, double nglobal_scaled, void **out,
                          double *volume_out) {
    return wae_guarded([&]() {
        if (!(points && out && nflame > 0 && flame_tets && x_ref && n_ref)) throw WaeError(WAE_ERR_INVALID, "bad argument");
        p2_check_mesh(npoints, ntets, tets, 0, nullptr);
        if (nflame > INT_MAX / 100) throw WaeError(WAE_ERR_INVALID, "too many flame tetrahedra: 100*nflame triplets must fit a 32-bit count");
        if (ref_tet < 0 || ref_tet >= ntets) throw WaeError(WAE_ERR_INVALID, "reference tetrahedron out of range");
        check_indices(flame_tets, nflame, ntets, "flame tetrahedron out of range");
        HIP_CHECK(hipSetDevice(device));
        P2Mesh m(npoints, points, ntets, tets, 0, nullptr);
        const size_t ne = (size_t)nflame * 100;
        Dev<double> qv(ne);
        Dev<u64> k0(ne);
        FlameSetup<10> f(m.pts.p, m.t10.p, nflame, flame_tets, nglobal_scaled, volume_out, points, tets, ref_tet);
        // g_b = -nlocal grad(phi_b)(x_ref) . n_ref on the 10 nodes of the reference tetrahedron (Helmholtz.jl:477-482): 10 numbers, on the host
        const double(&X)[4][3] = f.X;
        double G[4][3];
        if (tet_gradients(X, G) == 0.0) throw WaeError(WAE_ERR_INVALID, "degenerate reference tetrahedron");
        double lam[4];
        lam[3] = 1.0;
        for (int a = 0; a < 3; ++a) {
            lam[a] = G[a][0] * (x_ref[0] - X[3][0]) + G[a][1] * (x_ref[1] - X[3][1]) + G[a][2] * (x_ref[2] - X[3][2]);
            lam[3] -= lam[a];
        }
        double g[10];
        for (int b = 0; b < 10; ++b) {
            double w[4][3], s[3], acc = 0.0;
            p2_grad_coeffs(kTet.d[b], G, w, s);
            for (int k = 0; k < 4; ++k) acc += lam[k] * (w[k][0] * n_ref[0] + w[k][1] * n_ref[1] + w[k][2] * n_ref[2]);
            g[b] = -f.nlocal * acc;
        }
        Dev<double> dg(g, 10);
        hipLaunchKernelGGL(p2_flame_kernel, grid_for(nflame * 10), dim3(256), 0, 0, m.t10.p, f.list.p, nflame, f.adet.p, ref_tet, dg.p,
                           (u64)m.dim, k0.p, qv.p);
        HIP_CHECK(hipGetLastError());
        *out = triplets_to_csr(m.dim, ne, k0, qv, nullptr);
        return WAE_OK;
    });
}

// c_t / c_s: per tetrahedron / triangle (NULL = 1), or, nodal, both the one array per mesh point (required)
static int p2_shape_sensitivity(int32_t device, int64_t npoints, const double *points, const int32_t *tets, const double *c_t, int64_t npair_t,
                                const int32_t *pair_pt_t, const int32_t *pair_tet, const int32_t *tris, const double *c_s, bool nodal, int64_t npair_s,
                                const int32_t *pair_pt_s, const int32_t *pair_tri, int64_t ntets, int64_t ntris, const double *omega,
                                const double *omegaY, int64_t nv, const double *v, const double *v_adj, double h, double *out_t, double *out_s) {
    return wae_guarded([&]() {
        if (!(points && v && v_adj && omega && npair_t >= 0 && npair_s >= 0)) throw WaeError(WAE_ERR_INVALID, "bad argument");
        if (!(std::isfinite(h) && h > 0.0)) throw WaeError(WAE_ERR_INVALID, "the step h must be finite and positive");
        if (npair_t > 0 && !(pair_pt_t && pair_tet && out_t)) throw WaeError(WAE_ERR_INVALID, "bad tetrahedron pair arguments");
        if (npair_s > 0 && !(tris && pair_pt_s && pair_tri && out_s && omegaY && ntris > 0)) throw WaeError(WAE_ERR_INVALID, "bad triangle pair arguments");
        const int64_t ns = npair_s > 0 ? ntris : 0;                          // the triangles take part only if a pair names one
        p2_check_mesh(npoints, ntets, tets, ns, tris);
        if (npair_t > INT_MAX / 3 || npair_s > INT_MAX / 3) throw WaeError(WAE_ERR_INVALID, "too many pairs: 3*npair must fit a 32-bit count");
        if (nodal) check_c_point(npoints, c_t);
        check_indices(pair_tet, npair_t, ntets, "pair index out of range");
        check_indices(pair_pt_t, npair_t, npoints, "pair index out of range");
        check_indices(pair_tri, npair_s, ntris, "pair index out of range");
        check_indices(pair_pt_s, npair_s, npoints, "pair index out of range");
        if (npair_t == 0 && npair_s == 0) {                                  // empty lists: nothing is launched, nv is checked against a host count
            if (nv != npoints + p2_host_edge_count(npoints, ntets, tets)) throw WaeError(WAE_ERR_INVALID, "nv is not npoints + nedges");
            return (int)WAE_OK;
        }
        HIP_CHECK(hipSetDevice(device));
        P2Mesh m(npoints, points, ntets, tets, ns, tris);
        if (nv != m.dim) throw WaeError(WAE_ERR_INVALID, "nv is not npoints + nedges");
        Dev<cplx> dv((const cplx *)v, (size_t)nv), dva((const cplx *)v_adj, (size_t)nv);
        Dev<double> dcp(c_t, nodal ? (size_t)npoints : 0);                   // the nodal field serves both halves
        if (npair_t > 0)
            p2_shape_half(nodal ? p2_shape_tet_kernel<true> : p2_shape_tet_kernel<false>, m.pts, m.t10, nodal ? dcp.p : nullptr, c_t, (size_t)ntets, npair_t,
                          pair_pt_t, pair_tet, omega, dv, dva, h, out_t);
        if (npair_s > 0)
            p2_shape_half(nodal ? p2_shape_tri_kernel<true> : p2_shape_tri_kernel<false>, m.pts, m.s6, nodal ? dcp.p : nullptr, c_s, (size_t)ntris, npair_s,
                          pair_pt_s, pair_tri, omegaY, dv, dva, h, out_s);
        return (int)WAE_OK;
    });
}

int wae_p2_shape_sensitivity(int32_t device, int64_t npoints, const double *points, const int32_t *tets, const double *c_tet, int64_t npair_t,
                             const int32_t *pair_pt_t, const int32_t *pair_tet, const int32_t *tris, const double *c_tri, int64_t npair_s,
                             const int32_t *pair_pt_s, const int32_t *pair_tri, int64_t ntets, int64_t ntris, const double *omega,
                             const double *omegaY, int64_t nv, const double *v, const double *v_adj, double h, double *out_t, double *out_s) {
    return p2_shape_sensitivity(device, npoints, points, tets, c_tet, npair_t, pair_pt_t, pair_tet, tris, c_tri, false, npair_s, pair_pt_s, pair_tri, ntets,
                                ntris, omega, omegaY, nv, v, v_adj, h, out_t, out_s);
}

int wae_p2_shape_sensitivity_cpoint(int32_t device, int64_t npoints, const double *points, const int32_t *tets, const double *c_point, int64_t npair_t,
                                    const int32_t *pair_pt_t, const int32_t *pair_tet, const int32_t *tris, int64_t npair_s, const int32_t *pair_pt_s,
                                    const int32_t *pair_tri, int64_t ntets, int64_t ntris, const double *omega, const double *omegaY, int64_t nv,
                                    const double *v, const double *v_adj, double h, double *out_t, double *out_s) {
    return p2_shape_sensitivity(device, npoints, points, tets, c_point, npair_t, pair_pt_t, pair_tet, tris, c_point, true, npair_s, pair_pt_s, pair_tri, ntets,
                                ntris, omega, omegaY, nv, v, v_adj, h, out_t, out_s);
}

int wae_p2_shape_sensitivity_flame(int32_t device, int64_t npoints, const double *points, int64_t ntets, const int32_t *tets, int64_t npair,
                                   const int32_t *pair_pt, const int32_t *pair_tet, int32_t ref_tet, int64_t npair_r, const int32_t *pair_pt_r,
                                   const double *x_ref, const double *n_ref, int64_t nv, const double *v, const double *v_adj, double h, double *det_pm,
                                   double *ssum, double *g_pm, double *g0) {
    return wae_guarded([&]() {
        if (!(points && x_ref && n_ref && v && v_adj && g0 && npair >= 0 && npair_r >= 0)) throw WaeError(WAE_ERR_INVALID, "bad argument");
        if (!(std::isfinite(h) && h > 0.0)) throw WaeError(WAE_ERR_INVALID, "the step h must be finite and positive");
        if (npair > 0 && !(pair_pt && pair_tet && det_pm && ssum)) throw WaeError(WAE_ERR_INVALID, "bad flame pair arguments");
        if (npair_r > 0 && !(pair_pt_r && g_pm)) throw WaeError(WAE_ERR_INVALID, "bad reference pair arguments");
        p2_check_mesh(npoints, ntets, tets, 0, nullptr);
        if (npair > INT_MAX / 6 || npair_r > INT_MAX / 6) throw WaeError(WAE_ERR_INVALID, "too many pairs: 6*npair must fit a 32-bit count");
        if (ref_tet < 0 || ref_tet >= ntets) throw WaeError(WAE_ERR_INVALID, "reference tetrahedron out of range");
        for (int64_t i = 0; i < npair; ++i) {
            if (pair_tet[i] < 0 || pair_tet[i] >= ntets) throw WaeError(WAE_ERR_INVALID, "flame tetrahedron out of range");
            if (pair_pt[i] < 0 || pair_pt[i] >= npoints) throw WaeError(WAE_ERR_INVALID, "pair index out of range");
        }
        check_indices(pair_pt_r, npair_r, npoints, "pair index out of range");
        HIP_CHECK(hipSetDevice(device));
        P2Mesh m(npoints, points, ntets, tets, 0, nullptr);
        if (nv != m.dim) throw WaeError(WAE_ERR_INVALID, "nv is not npoints + nedges");
        Dev<cplx> dv((const cplx *)v, (size_t)nv), dva((const cplx *)v_adj, (size_t)nv);
        if (npair > 0) {
            Dev<int> dpp(pair_pt, (size_t)npair), dpt(pair_tet, (size_t)npair);
            Dev<double> ddet((size_t)npair * 6);
            Dev<cplx> dss((size_t)npair);
            hipLaunchKernelGGL(p2_shape_flame_kernel, grid_for(npair), dim3(256), 0, 0, m.pts.p, m.t10.p, npair, dpp.p, dpt.p, dva.p, h, ddet.p, dss.p);
            HIP_CHECK(hipGetLastError());
            ddet.to_host(det_pm, (size_t)npair * 6);
            dss.to_host((cplx *)ssum, (size_t)npair);
        }
        const size_t nr = (size_t)npair_r;
        Dev<int> dpr(pair_pt_r, nr);
        Dev<cplx> dg(nr * 6 + 1);
        hipLaunchKernelGGL(p2_shape_ref_kernel, dim3((unsigned)((nr + 1 + 63) / 64)), dim3(64), 0, 0, m.pts.p, m.t10.p, ref_tet, npair_r, dpr.p, x_ref[0], x_ref[1],
                           x_ref[2], n_ref[0], n_ref[1], n_ref[2], dv.p, h, dg.p, dg.p + nr * 6);
        HIP_CHECK(hipGetLastError());
        dg.to_host((cplx *)g_pm, nr * 6);
        dg.to_host((cplx *)g0, 1, nr * 6);
        return (int)WAE_OK;
    });
}

}  // extern "C"
