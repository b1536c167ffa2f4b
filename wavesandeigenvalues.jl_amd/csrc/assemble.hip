// P1 tetrahedral assembly of the Helmholtz mass and stiffness matrices on the device.
//
// Replaces the element loops of `discretize` for the two operators that dominate its run time
// (src/Helmholtz.jl:405-441: every tetrahedron contributes a 4x4 block to M and to K) with
//   1. one kernel: per tetrahedron the coordinate transformation (src/FEM/FEM.jl:9-20; tet_geometry.h), the local mass matrix
//      |det J|/120 (1 + delta_ab) (FEM.jl:704-710) and the local stiffness matrix -c^2 |det J|/6 grad phi_a . grad phi_b
//      (FEM.jl:1745-1766, Helmholtz.jl:120-124), written as 16 (key = row*np + col, m, k) triplets;
//   2. a stable radix sort of the keys (hipCUB) -- duplicates become adjacent, in element order, so the sums below are
//      deterministic (no atomics);
//   3. reduce-by-key (hipCUB) of both value streams, and the CSR row pointer from the unique keys.
// The result is what Julia's sparse(I, J, V) returns for the same triplets, up to the order of the additions.
#include <cstring>
#include <memory>
#include <vector>

#include "tet_geometry.h"
#include "../../include/waehip.h"

namespace {

// local P1 matrices of one tetrahedron with corner coordinates X: M_ab = |det J|/120 (1+delta_ab), K_ab = -c^2 |det J|/6 grad_a.grad_b
__device__ inline void p1_local(const double X[4][3], double c, double M[16], double K[16]) {
    double G[4][3];
    const double adet = fabs(tet_gradients(X, G));
    const double ks = -(c * c) * adet / 6.0;
    for (int a = 0; a < 4; ++a)
        for (int b = 0; b < 4; ++b) {
            M[a * 4 + b] = adet * (a == b ? 2.0 : 1.0) / 120.0;
            K[a * 4 + b] = ks * (G[a][0] * G[b][0] + G[a][1] * G[b][1] + G[a][2] * G[b][2]);
        }
}

// the same with the speed of sound interpolated linearly between the corner values c[0..3] (generate_field(...; order=:lin) and
// s43nv1nu1cc1 of the reference, Helmholtz.jl:59-74,120-124).  The gradients are constant on the tetrahedron, so c enters through
//     int c^2 = |det J| sum_pq c_p c_q (1 + delta_pq)/120 = |det J| ((sum_p c_p)^2 + sum_p c_p^2)/120 :
// K_ab = (-|det J|/6 grad_a.grad_b) ((sum c)^2 + sum c^2)/20, the first factor being what p1_local returns for c = 1.
__device__ inline void p1_local_cpoint(const double X[4][3], const double c[4], double M[16], double K[16]) {
    p1_local(X, 1.0, M, K);
    const double s = (c[0] + c[1]) + (c[2] + c[3]);
    double q = c[0] * c[0];
    for (int p = 1; p < 4; ++p) q = fma(c[p], c[p], q);
    const double w = fma(s, s, q) / 20.0;
    for (int i = 0; i < 16; ++i) K[i] *= w;
}

// Discrete-adjoint shape sensitivity (src/shape_sensitivity.jl:16-141), interior part: for the pair (surface point p,
// adjacent tetrahedron t) and coordinate x:  out = -v_adj_loc^H [ w^2 (M+ - M-) + (K+ - K-) ] v_loc / (2h), M+-/K+- the local
// matrices with x_p moved by +-h (central difference of two local re-discretisations, as the reference does).
// NODAL: cs holds one speed of sound per mesh point (p1_local_cpoint; the values stay with their points while a point moves), else one per
// tetrahedron (NULL = 1).
template <bool NODAL>
__global__ __launch_bounds__(256) void shape_tet_kernel(const double *__restrict__ pts, const int *__restrict__ tets, const double *__restrict__ cs,
                                                        int64_t npair, const int *__restrict__ pair_pt, const int *__restrict__ pair_tet,
                                                        double wr, double wi, const cplx *__restrict__ v, const cplx *__restrict__ vadj, double h,
                                                        cplx *__restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= npair * 3) return;
    const int64_t pr = e / 3;
    const int crd = (int)(e - pr * 3);
    const int t = pair_tet[pr], p = pair_pt[pr];
    int vtx[4];
    double X[4][3];
    int a0 = -1;
    for (int a = 0; a < 4; ++a) {
        vtx[a] = tets[(size_t)t * 4 + a];
        if (vtx[a] == p) a0 = a;
        for (int k = 0; k < 3; ++k) X[a][k] = pts[(size_t)vtx[a] * 3 + k];
    }
    if (a0 < 0) { out[e] = cplx{0.0, 0.0}; return; }
    double Mp[16], Kp[16], Mm[16], Km[16];
    if (NODAL) {                                           // the moved corner enters through selects on unrolled counters: no run-time index, no scratch
        double c[4], Xp[4][3], Xm[4][3];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            c[a] = cs[vtx[a]];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const bool moved = a == a0 && k == crd;
                Xp[a][k] = moved ? X[a][k] + h : X[a][k];
                Xm[a][k] = moved ? X[a][k] - h : X[a][k];
            }
        }
        p1_local_cpoint(Xp, c, Mp, Kp);
        p1_local_cpoint(Xm, c, Mm, Km);
    } else {
        const double c = cs ? cs[t] : 1.0;
        const double x0 = X[a0][crd];
        X[a0][crd] = x0 + h; p1_local(X, c, Mp, Kp);
        X[a0][crd] = x0 - h; p1_local(X, c, Mm, Km);
    }
    const double w2r = wr * wr - wi * wi, w2i = 2.0 * wr * wi;
    const double s = 1.0 / (2.0 * h);
    cplx acc = {0.0, 0.0};
    for (int a = 0; a < 4; ++a) {
        const cplx ya = vadj[vtx[a]];
        for (int b = 0; b < 4; ++b) {
            const double dm = (Mp[a * 4 + b] - Mm[a * 4 + b]) * s, dk = (Kp[a * 4 + b] - Km[a * 4 + b]) * s;
            const cplx D = {w2r * dm + dk, w2i * dm};
            const cplx xb = v[vtx[b]];
            const cplx Dx = {D.x * xb.x - D.y * xb.y, D.x * xb.y + D.y * xb.x};
            acc.x += ya.x * Dx.x + ya.y * Dx.y;          // conj(ya) * Dx
            acc.y += ya.x * Dx.y - ya.y * Dx.x;
        }
    }
    out[e] = cplx{-acc.x, -acc.y};
}

// boundary (admittance) part: C_ab = -i c |(x0-x2) x (x1-x2)| (1+delta_ab)/24 (FEM.jl:435-441, Helmholtz.jl:151-156,459),
// operator term w*Y*C:  out = -v_adj_loc^H [ w Y (C+ - C-) ] v_loc / (2h).  NODAL: cs holds one speed of sound per mesh point and the weights
// are those of p1_boundary_cpoint_kernel, b_aa = |..| (2 c_a + S)/60, b_ab = |..| (c_a + c_b + S)/120; else one value per triangle.
template <bool NODAL>
__global__ __launch_bounds__(256) void shape_tri_kernel(const double *__restrict__ pts, const int *__restrict__ tris, const double *__restrict__ cs,
                                                        int64_t npair, const int *__restrict__ pair_pt, const int *__restrict__ pair_tri,
                                                        double wyr, double wyi, const cplx *__restrict__ v, const cplx *__restrict__ vadj, double h,
                                                        cplx *__restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= npair * 3) return;
    const int64_t pr = e / 3;
    const int crd = (int)(e - pr * 3);
    const int t = pair_tri[pr], p = pair_pt[pr];
    int vtx[3];
    double X[3][3];
    int a0 = -1;
    for (int a = 0; a < 3; ++a) {
        vtx[a] = tris[(size_t)t * 3 + a];
        if (vtx[a] == p) a0 = a;
        for (int k = 0; k < 3; ++k) X[a][k] = pts[(size_t)vtx[a] * 3 + k];
    }
    if (a0 < 0) { out[e] = cplx{0.0, 0.0}; return; }
    auto area2 = [&]() {
        const double u0 = X[0][0] - X[2][0], u1 = X[0][1] - X[2][1], u2 = X[0][2] - X[2][2];
        const double w0 = X[1][0] - X[2][0], w1 = X[1][1] - X[2][1], w2 = X[1][2] - X[2][2];
        const double n0 = u1 * w2 - u2 * w1, n1 = u2 * w0 - u0 * w2, n2 = u0 * w1 - u1 * w0;
        return sqrt(n0 * n0 + n1 * n1 + n2 * n2);
    };
    const double x0 = X[a0][crd];
    X[a0][crd] = x0 + h; const double dp = area2();
    X[a0][crd] = x0 - h; const double dm = area2();
    double cn[3] = {1.0, 1.0, 1.0};
    if (NODAL)
        for (int a = 0; a < 3; ++a) cn[a] = cs[vtx[a]];
    const double S = cn[0] + cn[1] + cn[2];
    const double dd = NODAL ? (dp - dm) / (2.0 * h) : cs[t] * (dp - dm) / (2.0 * h) / 24.0;          // d/dx of c |..| /24; C = -i * that * (1+delta)
    // w Y C' = (wyr + i wyi) * (-i) * dd * (1+delta) = (wyi - i wyr) dd (1+delta)
    const cplx f = {wyi * dd, -wyr * dd};
    cplx acc = {0.0, 0.0};
    for (int a = 0; a < 3; ++a) {
        const cplx ya = vadj[vtx[a]];
        for (int b = 0; b < 3; ++b) {
            const double m = NODAL ? (a == b ? (2.0 * cn[a] + S) / 60.0 : ((cn[a] + cn[b]) + S) / 120.0) : (a == b) ? 2.0 : 1.0;
            const cplx xb = v[vtx[b]];
            const cplx Dx = {m * (f.x * xb.x - f.y * xb.y), m * (f.x * xb.y + f.y * xb.x)};
            acc.x += ya.x * Dx.x + ya.y * Dx.y;
            acc.y += ya.x * Dx.y - ya.y * Dx.x;
        }
    }
    out[e] = cplx{-acc.x, -acc.y};
}

__global__ __launch_bounds__(256) void p1_local_kernel(const double *__restrict__ pts, const int *__restrict__ tets, const double *__restrict__ c_tet,
                                                       int64_t nt, int64_t np, unsigned long long *__restrict__ keys, double *__restrict__ mv,
                                                       double *__restrict__ kv) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= nt) return;
    int v[4];
    double X[4][3];
    for (int a = 0; a < 4; ++a) {
        v[a] = tets[t * 4 + a];
        for (int k = 0; k < 3; ++k) X[a][k] = pts[(size_t)v[a] * 3 + k];
    }
    double Ml[16], Kl[16];
    p1_local(X, c_tet ? c_tet[t] : 1.0, Ml, Kl);
    for (int a = 0; a < 4; ++a)
        for (int b = 0; b < 4; ++b) {
            const size_t o = (size_t)t * 16 + a * 4 + b;
            keys[o] = (unsigned long long)v[a] * (unsigned long long)np + (unsigned long long)v[b];
            mv[o] = Ml[a * 4 + b];
            kv[o] = Kl[a * 4 + b];
        }
}

// p1_local_kernel with the speed of sound given at the mesh points
__global__ __launch_bounds__(256) void p1_local_cpoint_kernel(const double *__restrict__ pts, const int *__restrict__ tets,
                                                              const double *__restrict__ c_point, int64_t nt, int64_t np,
                                                              unsigned long long *__restrict__ keys, double *__restrict__ mv, double *__restrict__ kv) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= nt) return;
    int v[4];
    double X[4][3], c[4];
    for (int a = 0; a < 4; ++a) {
        v[a] = tets[t * 4 + a];
        for (int k = 0; k < 3; ++k) X[a][k] = pts[(size_t)v[a] * 3 + k];
        c[a] = c_point[v[a]];
    }
    double Ml[16], Kl[16];
    p1_local_cpoint(X, c, Ml, Kl);
    for (int a = 0; a < 4; ++a)
        for (int b = 0; b < 4; ++b) {
            const size_t o = (size_t)t * 16 + a * 4 + b;
            keys[o] = (unsigned long long)v[a] * (unsigned long long)np + (unsigned long long)v[b];
            mv[o] = Ml[a * 4 + b];
            kv[o] = Kl[a * 4 + b];
        }
}

__global__ __launch_bounds__(256) void gather_d_kernel(const double *__restrict__ src, const unsigned int *__restrict__ idx, double *__restrict__ dst, size_t n) {
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) dst[e] = src[idx[e]];
}
__global__ __launch_bounds__(256) void iota_kernel(unsigned int *__restrict__ idx, size_t n) {
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) idx[e] = (unsigned int)e;
}
// col[e] = key % np; rows counted into rowcnt[key / np + 1]
__global__ __launch_bounds__(256) void split_keys_kernel(const unsigned long long *__restrict__ keys, size_t nnz, unsigned long long np,
                                                         int *__restrict__ col, int *__restrict__ rowptr) {
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < nnz; e += (size_t)gridDim.x * 256) {
        const unsigned long long k = keys[e];
        const unsigned long long r = k / np;
        col[e] = (int)(k - r * np);
        // first entry of a row records its position; rows without entries are filled by the host scan
        if (e == 0 || keys[e - 1] / np != r) rowptr[r] = (int)e;
    }
}

}  // namespace

// keyed triplets (key = row * np + col; up to two value streams) -> CSR: stable radix sort (duplicates adjacent, in
// element order: the sums are deterministic, no atomics), reduce-by-key, row pointer from the unique keys  (declared in
// wae_internal.h: assemble_p2.hip feeds it too).  triplets_to_csr_dev leaves the result in HBM (galerkin.hip keeps it there);
// triplets_to_csr copies it out and fills the pointer of the rows without entries.
void triplets_to_csr_dev(int64_t npoints, size_t ne, Dev<unsigned long long> &k0, Dev<double> &mv, Dev<double> *kv, TripletCsr &out) {
    Dev<double> ms(ne), ks(kv ? ne : 1);
    DevBuf<double> &mu = out.m, &ku = out.k;
    DevBuf<int> &dcol = out.col, &drow = out.rowptr;
    mu.alloc(std::max<size_t>(ne, 1)); ku.alloc(kv ? std::max<size_t>(ne, 1) : 1);
    dcol.alloc(std::max<size_t>(ne, 1)); drow.alloc((size_t)npoints + 1);
    Dev<int> dnum(1);
    Dev<unsigned long long> k1(ne), ku0(ne);
    Dev<unsigned int> i0(ne), i1(ne);
    const dim3 g = grid_for(ne, GRID_STRIDE_CAP);
    hipLaunchKernelGGL(iota_kernel, g, dim3(256), 0, 0, i0.p, ne);
    const int bits = key_bits((unsigned long long)npoints * (unsigned long long)npoints);
    auto sort = [&](void *t, size_t &b) { return hipcub::DeviceRadixSort::SortPairs(t, b, k0.p, k1.p, i0.p, i1.p, (int)ne, 0, bits); };
    auto reduce = [&](double *in, double *out) {
        return [&, in, out](void *t, size_t &b) { return hipcub::DeviceReduce::ReduceByKey(t, b, k1.p, ku0.p, in, out, dnum.p, hipcub::Sum(), (int)ne); };
    };
    DevBuf<char> tmp;
    cub_reserve(tmp, sort, reduce(ms.p, mu.p));
    cub_run(sort, tmp);
    hipLaunchKernelGGL(gather_d_kernel, g, dim3(256), 0, 0, mv.p, i1.p, ms.p, ne);
    if (kv) hipLaunchKernelGGL(gather_d_kernel, g, dim3(256), 0, 0, kv->p, i1.p, ks.p, ne);
    cub_run(reduce(ms.p, mu.p), tmp);
    if (kv) cub_run(reduce(ks.p, ku.p), tmp);
    int nnz = 0;
    dnum.to_host(&nnz, 1);
    HIP_CHECK(hipMemset(drow.p, 0xff, ((size_t)npoints + 1) * sizeof(int)));          // -1 = row without entries
    hipLaunchKernelGGL(split_keys_kernel, g, dim3(256), 0, 0, ku0.p, (size_t)nnz, (unsigned long long)npoints, dcol.p, drow.p);
    HIP_CHECK(hipGetLastError());
    out.np = npoints; out.nnz = nnz;
}

P1Handle *triplets_to_csr(int64_t npoints, size_t ne, Dev<unsigned long long> &k0, Dev<double> &mv, Dev<double> *kv) {
    TripletCsr D;
    triplets_to_csr_dev(npoints, ne, k0, mv, kv, D);
    const int nnz = D.nnz;
    std::unique_ptr<P1Handle> H(new P1Handle);
    H->np = npoints; H->nnz = nnz;
    H->rowptr.resize((size_t)npoints + 1); H->col.resize(nnz); H->m.resize(nnz); H->k.assign(nnz, 0.0);
    D.rowptr.to_host(H->rowptr.data(), (size_t)npoints + 1);
    D.col.to_host(H->col.data(), (size_t)nnz);
    D.m.to_host(H->m.data(), (size_t)nnz);
    if (kv) D.k.to_host(H->k.data(), (size_t)nnz);
    H->rowptr[npoints] = nnz;
    for (int64_t r = npoints - 1; r >= 0; --r)
        if (H->rowptr[r] < 0) H->rowptr[r] = H->rowptr[r + 1];
    return H.release();
}

// (declared in mesh_host.h: FlameSetup of tet_geometry.h sums every order's flame with it)
double flame_volume(const Dev<double> &adet, int64_t nflame) {
    const double volume = device_sum(adet.p, (int)nflame) / 6.0;
    if (!(volume > 0.0)) throw WaeError(WAE_ERR_INVALID, "flame domain has no volume");
    return volume;
}

void pairs_to_dense(int64_t n, size_t ne, Dev<unsigned long long> &k0, Dev<double> &v, double *out) {
    std::unique_ptr<P1Handle> H(triplets_to_csr(n, ne, k0, v, nullptr));
    for (int64_t r = 0; r < n; ++r) out[r] = H->rowptr[r + 1] > H->rowptr[r] ? H->m[(size_t)H->rowptr[r]] : 0.0;
}

namespace {

// boundary mass of one triangle: b_ab = c |(x0-x2) x (x1-x2)| (1+delta_ab)/24  (FEM.jl:9-20,435-441; Helmholtz.jl:151-156); C = -i b
__global__ __launch_bounds__(256) void p1_boundary_kernel(const double *__restrict__ pts, const int *__restrict__ tris, const double *__restrict__ c_tri,
                                                          int64_t nt, int64_t np, unsigned long long *__restrict__ keys, double *__restrict__ bv) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= nt) return;
    int v[3];
    double X[3][3];
    for (int a = 0; a < 3; ++a) {
        v[a] = tris[t * 3 + a];
        for (int k = 0; k < 3; ++k) X[a][k] = pts[(size_t)v[a] * 3 + k];
    }
    const double u0 = X[0][0] - X[2][0], u1 = X[0][1] - X[2][1], u2 = X[0][2] - X[2][2];
    const double w0 = X[1][0] - X[2][0], w1 = X[1][1] - X[2][1], w2 = X[1][2] - X[2][2];
    const double n0 = u1 * w2 - u2 * w1, n1 = u2 * w0 - u0 * w2, n2 = u0 * w1 - u1 * w0;
    const double det = sqrt(n0 * n0 + n1 * n1 + n2 * n2);
    const double c = c_tri ? c_tri[t] : 1.0;
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            const size_t o = (size_t)t * 9 + a * 3 + b;
            keys[o] = (unsigned long long)v[a] * (unsigned long long)np + (unsigned long long)v[b];
            bv[o] = c * ((a == b ? 2.0 : 1.0) / 24.0) * det;
        }
}

// the same with c interpolated linearly between the corner values (s33v1u1c1 of the reference, Helmholtz.jl:151-156): with
// int l^alpha = alpha!/(|alpha| + 2)! on the triangle,  b_ab = |..| sum_p c_p int l_a l_b l_p:
//     b_aa = |..| (2 c_a + S)/60,     b_ab = |..| (c_a + c_b + S)/120  (a != b),     S = c_1 + c_2 + c_3
__global__ __launch_bounds__(256) void p1_boundary_cpoint_kernel(const double *__restrict__ pts, const int *__restrict__ tris,
                                                                 const double *__restrict__ c_point, int64_t nt, int64_t np,
                                                                 unsigned long long *__restrict__ keys, double *__restrict__ bv) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= nt) return;
    int v[3];
    double X[3][3], c[3];
    for (int a = 0; a < 3; ++a) {
        v[a] = tris[t * 3 + a];
        for (int k = 0; k < 3; ++k) X[a][k] = pts[(size_t)v[a] * 3 + k];
        c[a] = c_point[v[a]];
    }
    const double u0 = X[0][0] - X[2][0], u1 = X[0][1] - X[2][1], u2 = X[0][2] - X[2][2];
    const double w0 = X[1][0] - X[2][0], w1 = X[1][1] - X[2][1], w2 = X[1][2] - X[2][2];
    const double n0 = u1 * w2 - u2 * w1, n1 = u2 * w0 - u0 * w2, n2 = u0 * w1 - u1 * w0;
    const double det = sqrt(n0 * n0 + n1 * n1 + n2 * n2);
    const double S = c[0] + c[1] + c[2];
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            const size_t o = (size_t)t * 9 + a * 3 + b;
            keys[o] = (unsigned long long)v[a] * (unsigned long long)np + (unsigned long long)v[b];
            bv[o] = (a == b ? (2.0 * c[a] + S) / 60.0 : ((c[a] + c[b]) + S) / 120.0) * det;          // (c_a + c_b) first: b_ab == b_ba
        }
}

// speaker source vector of one triangle (wallsrc of the reference divided by i, Helmholtz.jl:488-505): s_a = |(x0-x2) x (x1-x2)| int c l_a with
// int l^alpha = alpha!/(|alpha| + 2)!:  c per triangle: s_a = c |..|/6;  c per point: s_a = |..| (c_a/12 + (c_b + c_c)/24).  Three (node, value)
// pairs per triangle, key = node * np (column 0 of triplets_to_csr)
__global__ __launch_bounds__(256) void p1_source_kernel(const double *__restrict__ pts, const int *__restrict__ tris, const double *__restrict__ c, int nodal,
                                                        int64_t nt, int64_t np, unsigned long long *__restrict__ keys, double *__restrict__ sv) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= nt) return;
    int v[3];
    double X[3][3];
    for (int a = 0; a < 3; ++a) {
        v[a] = tris[t * 3 + a];
        for (int k = 0; k < 3; ++k) X[a][k] = pts[(size_t)v[a] * 3 + k];
    }
    const double u0 = X[0][0] - X[2][0], u1 = X[0][1] - X[2][1], u2 = X[0][2] - X[2][2];
    const double w0 = X[1][0] - X[2][0], w1 = X[1][1] - X[2][1], w2 = X[1][2] - X[2][2];
    const double n0 = u1 * w2 - u2 * w1, n1 = u2 * w0 - u0 * w2, n2 = u0 * w1 - u1 * w0;
    const double det = sqrt(n0 * n0 + n1 * n1 + n2 * n2);
    double cc[3] = {1.0, 1.0, 1.0};
    if (nodal)
        for (int a = 0; a < 3; ++a) cc[a] = c[v[a]];
    const double ct = (!nodal && c) ? c[t] : 1.0;
    for (int a = 0; a < 3; ++a) {
        const size_t o = (size_t)t * 3 + a;
        keys[o] = (unsigned long long)v[a] * (unsigned long long)np;
        sv[o] = nodal ? det * (cc[a] / 12.0 + (cc[(a + 1) % 3] + cc[(a + 2) % 3]) / 24.0) : ct * det / 6.0;
    }
}

// Q triplets: (node a of flame tetrahedron i, node b of the reference tetrahedron) -> |det J_i|/24 * g_b   (Helmholtz.jl:19-33,483)
__global__ __launch_bounds__(256) void p1_flame_kernel(const int *__restrict__ tets, const int *__restrict__ list, int64_t n, const double *__restrict__ adet,
                                                       int r0, int r1, int r2, int r3, double g0, double g1, double g2, double g3, int64_t np,
                                                       unsigned long long *__restrict__ keys, double *__restrict__ qv) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int t = list[i];
    const double s = adet[i] / 24.0;
    const int rn[4] = {r0, r1, r2, r3};
    const double g[4] = {g0, g1, g2, g3};
    for (int a = 0; a < 4; ++a)
        for (int b = 0; b < 4; ++b) {
            const size_t o = (size_t)i * 16 + a * 4 + b;
            keys[o] = (unsigned long long)tets[(size_t)t * 4 + a] * (unsigned long long)np + (unsigned long long)rn[b];
            qv[o] = s * g[b];
        }
}

}  // namespace

// Flame part of the discrete-adjoint shape sensitivity (shape_sensitivity.jl:62-141 with a :flame domain in dscrp).  The
// reference re-discretises, per surface point, the flame tetrahedra that touch the point: Q = S (x) g with S_a = |det J|/24 on
// their nodes (FEM.jl:2429-2431), nlocal = nglobal_scaled / (volume of THOSE tetrahedra) (Helmholtz.jl:325 on the reduced domain)
// and g_b = -nlocal grad(phi_b).n_ref on the reference tetrahedron (FEM.jl:2442-2448).  Per (point, flame tetrahedron,
// coordinate) this kernel returns |det J| with the point moved by +h and by -h, and per pair the sum of conj(v_adj) over the
// tetrahedron's nodes: the host sums them per point (fixed order) and forms  -v_adj' (Q+ - Q-)/(2h) v.
__global__ __launch_bounds__(256) void shape_flame_kernel(const double *__restrict__ pts, const int *__restrict__ tets, int64_t npair,
                                                          const int *__restrict__ pair_pt, const int *__restrict__ pair_tet,
                                                          const cplx *__restrict__ vadj, double h, double *__restrict__ det_pm,
                                                          cplx *__restrict__ ssum) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= npair * 3) return;
    const int64_t pr = e / 3;
    const int crd = (int)(e - pr * 3);
    const int t = pair_tet[pr], p = pair_pt[pr];
    int vtx[4];
    double X[4][3];
    int a0 = -1;
    cplx sa = {0.0, 0.0};
    for (int a = 0; a < 4; ++a) {
        vtx[a] = tets[(size_t)t * 4 + a];
        if (vtx[a] == p) a0 = a;
        for (int k = 0; k < 3; ++k) X[a][k] = pts[(size_t)vtx[a] * 3 + k];
        const cplx y = vadj[vtx[a]];
        sa.x += y.x; sa.y -= y.y;                              // conj(v_adj)
    }
    if (crd == 0) ssum[pr] = sa;
    auto adet = [&]() {
        double J[3][3], Ji[3][3];
        return fabs(tet_jacobian(X, J, Ji));
    };
    if (a0 < 0) { det_pm[e * 2] = det_pm[e * 2 + 1] = adet(); return; }
    const double x0 = X[a0][crd];
    X[a0][crd] = x0 + h; det_pm[e * 2] = adet();
    X[a0][crd] = x0 - h; det_pm[e * 2 + 1] = adet();
}
// sum_b (grad(phi_b) . n_ref) v_b on the reference tetrahedron with vertex `p` moved by +h / -h along each coordinate (3 x 2
// complex numbers per listed vertex), and undisplaced (g0)
__global__ void shape_ref_kernel(const double *__restrict__ pts, const int *__restrict__ tets, int ref_tet, int64_t npair, const int *__restrict__ pair_pt,
                                 double n0, double n1, double n2, const cplx *__restrict__ v, double h, cplx *__restrict__ g_pm, cplx *__restrict__ g0) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e > npair * 6) return;                                  // e == npair * 6: the undisplaced value
    int vtx[4];
    double X[4][3];
    for (int a = 0; a < 4; ++a) {
        vtx[a] = tets[(size_t)ref_tet * 4 + a];
        for (int k = 0; k < 3; ++k) X[a][k] = pts[(size_t)vtx[a] * 3 + k];
    }
    if (e < npair * 6) {
        const int64_t pr = e / 6;
        const int crd = (int)((e - pr * 6) >> 1), sgn = (int)(e & 1);
        for (int a = 0; a < 4; ++a)
            if (vtx[a] == pair_pt[pr]) X[a][crd] += sgn ? -h : h;
    }
    double G[4][3];
    tet_gradients(X, G);
    cplx acc = {0.0, 0.0};
    for (int b = 0; b < 4; ++b) {
        const double gb = G[b][0] * n0 + G[b][1] * n1 + G[b][2] * n2;
        const cplx xb = v[vtx[b]];
        acc.x += gb * xb.x; acc.y += gb * xb.y;
    }
    if (e < npair * 6) g_pm[e] = acc; else *g0 = acc;
}

namespace {

// One half of wae_p1_shape_sensitivity (tetrahedra with omega, triangles with omega Y): the simplices, their speed of sound (nc values, NULL = 1)
// and the (point, simplex) pairs go up, `kernel` runs over the 3 npair (pair, coordinate) items, out receives their 3 npair complex numbers.
typedef void (*ShapeKernel)(const double *, const int *, const double *, int64_t, const int *, const int *, double, double, const cplx *, const cplx *,
                            double, cplx *);
void shape_half(ShapeKernel kernel, const Dev<double> &dpts, const int32_t *simplices, size_t nints, const double *c, size_t nc, int64_t npair,
                const int32_t *pair_pt, const int32_t *pair_simplex, const double *w, const Dev<cplx> &dv, const Dev<cplx> &dva, double h, double *out) {
    Dev<int> dt(simplices, nints), dpp(pair_pt, (size_t)npair), dps(pair_simplex, (size_t)npair);
    Dev<double> dc(c, c ? nc : 0);
    Dev<cplx> dout((size_t)npair * 3);
    hipLaunchKernelGGL(kernel, grid_for(npair * 3), dim3(256), 0, 0, dpts.p, dt.p, c ? dc.p : nullptr, npair, dpp.p, dps.p, w[0], w[1], dv.p, dva.p, h, dout.p);
    HIP_CHECK(hipGetLastError());
    dout.to_host((cplx *)out, (size_t)npair * 3);
}

}  // namespace

extern "C" {

// c: per triangle (NULL = 1), or per mesh point (nodal; required)
static int p1_assemble_boundary(int32_t device, int64_t npoints, const double *points, int64_t ntris, const int32_t *tris, const double *c, bool nodal,
                                void **out) {
    return wae_guarded([&]() {
        if (!(npoints > 0 && ntris > 0 && points && tris && out)) throw WaeError(WAE_ERR_INVALID, "bad argument");
        if (nodal) check_c_point(npoints, c);
        check_tris(tris, ntris, npoints);
        HIP_CHECK(hipSetDevice(device));
        const size_t ne = (size_t)ntris * 9;
        Dev<double> dpts(points, (size_t)npoints * 3), dc(c, c ? (size_t)(nodal ? npoints : ntris) : 0), bv(ne);
        Dev<int> dt(tris, (size_t)ntris * 3);
        Dev<unsigned long long> k0(ne);
        if (nodal) hipLaunchKernelGGL(p1_boundary_cpoint_kernel, grid_for(ntris), dim3(256), 0, 0, dpts.p, dt.p, dc.p, ntris, npoints, k0.p, bv.p);
        else hipLaunchKernelGGL(p1_boundary_kernel, grid_for(ntris), dim3(256), 0, 0, dpts.p, dt.p, c ? dc.p : nullptr, ntris, npoints, k0.p, bv.p);
        HIP_CHECK(hipGetLastError());
        *out = triplets_to_csr(npoints, ne, k0, bv, nullptr);
        return WAE_OK;
    });
}

int wae_p1_assemble_boundary(int32_t device, int64_t npoints, const double *points, int64_t ntris, const int32_t *tris, const double *c_tri, void **out) {
    return p1_assemble_boundary(device, npoints, points, ntris, tris, c_tri, false, out);
}

int wae_p1_assemble_boundary_cpoint(int32_t device, int64_t npoints, const double *points, int64_t ntris, const int32_t *tris, const double *c_point,
                                    void **out) {
    return p1_assemble_boundary(device, npoints, points, ntris, tris, c_point, true, out);
}

// c: per triangle (NULL = 1), or per mesh point (nodal; required)
static int p1_assemble_source(int32_t device, int64_t npoints, const double *points, int64_t ntris, const int32_t *tris, const double *c, bool nodal,
                              double *out) {
    return wae_guarded([&]() {
        if (!(npoints > 0 && ntris >= 0 && points && (ntris == 0 || tris) && out)) throw WaeError(WAE_ERR_INVALID, "bad argument");
        if (nodal) check_c_point(npoints, c);
        if ((size_t)ntris * 3 >= 0x7fffffffull) throw WaeError(WAE_ERR_INVALID, "too many triangles for a 32-bit pair count");
        check_tris(tris, ntris, npoints);
        if (ntris == 0) {                                                     // an empty speaker domain: the zero vector
            std::fill(out, out + npoints, 0.0);
            return WAE_OK;
        }
        HIP_CHECK(hipSetDevice(device));
        const size_t ne = (size_t)ntris * 3;
        Dev<double> dpts(points, (size_t)npoints * 3), dc(c, c ? (size_t)(nodal ? npoints : ntris) : 0), sv(ne);
        Dev<int> dt(tris, (size_t)ntris * 3);
        Dev<unsigned long long> k0(ne);
        hipLaunchKernelGGL(p1_source_kernel, grid_for(ntris), dim3(256), 0, 0, dpts.p, dt.p, c ? dc.p : nullptr, nodal ? 1 : 0, ntris, npoints, k0.p, sv.p);
        HIP_CHECK(hipGetLastError());
        pairs_to_dense(npoints, ne, k0, sv, out);
        return WAE_OK;
    });
}

int wae_p1_assemble_source(int32_t device, int64_t npoints, const double *points, int64_t ntris, const int32_t *tris, const double *c_tri, double *out) {
    return p1_assemble_source(device, npoints, points, ntris, tris, c_tri, false, out);
}

int wae_p1_assemble_source_cpoint(int32_t device, int64_t npoints, const double *points, int64_t ntris, const int32_t *tris, const double *c_point,
                                  double *out) {
    return p1_assemble_source(device, npoints, points, ntris, tris, c_point, true, out);
}

int wae_p1_assemble_flame(int32_t device, int64_t npoints, const double *points, int64_t ntets, const int32_t *tets, int64_t nflame,
                          const int32_t *flame_tets, int32_t ref_tet, const double *n_ref, double nglobal_scaled, void **out, double *volume_out) {
    return wae_guarded([&]() {
        if (!(npoints > 0 && ntets > 0 && nflame > 0 && points && tets && flame_tets && n_ref && out)) throw WaeError(WAE_ERR_INVALID, "bad argument");
        if (ref_tet < 0 || ref_tet >= ntets) throw WaeError(WAE_ERR_INVALID, "reference tetrahedron out of range");
        check_indices(flame_tets, nflame, ntets, "flame tetrahedron out of range");
        check_tets(tets, ntets, npoints);
        HIP_CHECK(hipSetDevice(device));
        const size_t ne = (size_t)nflame * 16;
        Dev<double> dpts(points, (size_t)npoints * 3), qv(ne);
        Dev<int> dt(tets, (size_t)ntets * 4);
        Dev<unsigned long long> k0(ne);
        FlameSetup<4> f(dpts.p, dt.p, nflame, flame_tets, nglobal_scaled, volume_out, points, tets, ref_tet);
        // g_b = -nlocal grad(phi_b) . n_ref on the reference tetrahedron (FEM.jl:2442-2448, Helmholtz.jl:482): 4 numbers, on the host
        double G[4][3], g[4];
        if (tet_gradients(f.X, G) == 0.0) throw WaeError(WAE_ERR_INVALID, "degenerate reference tetrahedron");
        for (int b = 0; b < 4; ++b) g[b] = -f.nlocal * (G[b][0] * n_ref[0] + G[b][1] * n_ref[1] + G[b][2] * n_ref[2]);
        const int32_t *rn = tets + (size_t)ref_tet * 4;
        hipLaunchKernelGGL(p1_flame_kernel, grid_for(nflame), dim3(256), 0, 0, dt.p, f.list.p, nflame, f.adet.p, rn[0], rn[1], rn[2], rn[3], g[0], g[1], g[2], g[3],
                           npoints, k0.p, qv.p);
        HIP_CHECK(hipGetLastError());
        *out = triplets_to_csr(npoints, ne, k0, qv, nullptr);
        return WAE_OK;
    });
}

static int p1_assemble_interior(int32_t device, int64_t npoints, const double *points, int64_t ntets, const int32_t *tets, const double *c, bool nodal,
                                void **out) {
    return wae_guarded([&]() {
        if (!(npoints > 0 && ntets > 0 && points && tets && out)) throw WaeError(WAE_ERR_INVALID, "bad argument");
        if (nodal) check_c_point(npoints, c);
        if ((size_t)ntets * 16 >= 0xffffffffull) throw WaeError(WAE_ERR_INVALID, "too many tetrahedra for 32-bit triplet indices");
        check_tets(tets, ntets, npoints);
        HIP_CHECK(hipSetDevice(device));
        const size_t ne = (size_t)ntets * 16;
        Dev<double> dpts(points, (size_t)npoints * 3), dc(c, c ? (size_t)(nodal ? npoints : ntets) : 0), mv(ne), kv(ne);
        Dev<int> dt(tets, (size_t)ntets * 4);
        Dev<unsigned long long> k0(ne);
        if (nodal) hipLaunchKernelGGL(p1_local_cpoint_kernel, grid_for(ntets), dim3(256), 0, 0, dpts.p, dt.p, dc.p, ntets, npoints, k0.p, mv.p, kv.p);
        else hipLaunchKernelGGL(p1_local_kernel, grid_for(ntets), dim3(256), 0, 0, dpts.p, dt.p, c ? dc.p : nullptr, ntets, npoints, k0.p, mv.p, kv.p);
        HIP_CHECK(hipGetLastError());
        *out = triplets_to_csr(npoints, ne, k0, mv, &kv);
        return WAE_OK;
    });
}

int wae_p1_assemble(int32_t device, int64_t npoints, const double *points, int64_t ntets, const int32_t *tets, const double *c_tet, void **out) {
    return p1_assemble_interior(device, npoints, points, ntets, tets, c_tet, false, out);
}

int wae_p1_assemble_cpoint(int32_t device, int64_t npoints, const double *points, int64_t ntets, const int32_t *tets, const double *c_point, void **out) {
    return p1_assemble_interior(device, npoints, points, ntets, tets, c_point, true, out);
}

// c_tet / c_tri: per tetrahedron (NULL = 1) / per triangle, or, nodal, both the one array per mesh point (required, finite)
static int p1_shape_sensitivity(int32_t device, int64_t npoints, const double *points, const int32_t *tets, const double *c_tet, int64_t npair_t,
                                const int32_t *pair_pt_t, const int32_t *pair_tet, const int32_t *tris, const double *c_tri, bool nodal, int64_t npair_s,
                                const int32_t *pair_pt_s, const int32_t *pair_tri, int64_t ntets, int64_t ntris, const double *omega,
                                const double *omegaY, const double *v, const double *v_adj, double h, double *out_t, double *out_s) {
    return wae_guarded([&]() {
        if (!(npoints > 0 && points && v && v_adj && omega && h > 0.0)) throw WaeError(WAE_ERR_INVALID, "bad argument");
        if (nodal) {
            if (!std::isfinite(h)) throw WaeError(WAE_ERR_INVALID, "the step h must be finite and positive");
            if (npair_t < 0 || npair_s < 0) throw WaeError(WAE_ERR_INVALID, "bad argument");
            check_c_point(npoints, c_tet);
        }
        if (npair_t > 0 && !(tets && pair_pt_t && pair_tet && out_t && ntets > 0)) throw WaeError(WAE_ERR_INVALID, "bad tetrahedron pair arguments");
        if (npair_s > 0 && !(tris && c_tri && pair_pt_s && pair_tri && out_s && omegaY && ntris > 0)) throw WaeError(WAE_ERR_INVALID, "bad triangle pair arguments");
        check_indices(pair_tet, npair_t, ntets, "pair index out of range");
        check_indices(pair_pt_t, npair_t, npoints, "pair index out of range");
        check_indices(pair_tri, npair_s, ntris, "pair index out of range");
        check_indices(pair_pt_s, npair_s, npoints, "pair index out of range");
        if (npair_t > 0) check_tets(tets, ntets, npoints);
        if (npair_s > 0) check_tris(tris, ntris, npoints);
        HIP_CHECK(hipSetDevice(device));
        Dev<double> dpts(points, (size_t)npoints * 3);
        Dev<cplx> dv((const cplx *)v, (size_t)npoints), dva((const cplx *)v_adj, (size_t)npoints);
        if (npair_t > 0)
            shape_half(nodal ? shape_tet_kernel<true> : shape_tet_kernel<false>, dpts, tets, (size_t)ntets * 4, c_tet, (size_t)(nodal ? npoints : ntets),
                       npair_t, pair_pt_t, pair_tet, omega, dv, dva, h, out_t);
        if (npair_s > 0)
            shape_half(nodal ? shape_tri_kernel<true> : shape_tri_kernel<false>, dpts, tris, (size_t)ntris * 3, c_tri, (size_t)(nodal ? npoints : ntris),
                       npair_s, pair_pt_s, pair_tri, omegaY, dv, dva, h, out_s);
        return WAE_OK;
    });
}

int wae_p1_shape_sensitivity(int32_t device, int64_t npoints, const double *points, const int32_t *tets, const double *c_tet, int64_t npair_t,
                             const int32_t *pair_pt_t, const int32_t *pair_tet, const int32_t *tris, const double *c_tri, int64_t npair_s,
                             const int32_t *pair_pt_s, const int32_t *pair_tri, int64_t ntets, int64_t ntris, const double *omega,
                             const double *omegaY, const double *v, const double *v_adj, double h, double *out_t, double *out_s) {
    return p1_shape_sensitivity(device, npoints, points, tets, c_tet, npair_t, pair_pt_t, pair_tet, tris, c_tri, false, npair_s, pair_pt_s, pair_tri, ntets,
                                ntris, omega, omegaY, v, v_adj, h, out_t, out_s);
}

int wae_p1_shape_sensitivity_cpoint(int32_t device, int64_t npoints, const double *points, const int32_t *tets, const double *c_point, int64_t npair_t,
                                    const int32_t *pair_pt_t, const int32_t *pair_tet, const int32_t *tris, int64_t npair_s, const int32_t *pair_pt_s,
                                    const int32_t *pair_tri, int64_t ntets, int64_t ntris, const double *omega, const double *omegaY, const double *v,
                                    const double *v_adj, double h, double *out_t, double *out_s) {
    return p1_shape_sensitivity(device, npoints, points, tets, c_point, npair_t, pair_pt_t, pair_tet, tris, c_point, true, npair_s, pair_pt_s, pair_tri, ntets,
                                ntris, omega, omegaY, v, v_adj, h, out_t, out_s);
}

int wae_p1_shape_sensitivity_flame(int32_t device, int64_t npoints, const double *points, int64_t ntets, const int32_t *tets, int64_t npair,
                                   const int32_t *pair_pt, const int32_t *pair_tet, int32_t ref_tet, int64_t npair_r, const int32_t *pair_pt_r,
                                   const double *n_ref, const double *v, const double *v_adj, double h, double *det_pm, double *ssum,
                                   double *g_pm, double *g0) {
    return wae_guarded([&]() {
        if (!(npoints > 0 && ntets > 0 && points && tets && n_ref && v && v_adj && h > 0.0 && g0)) throw WaeError(WAE_ERR_INVALID, "bad argument");
        if (npair > 0 && !(pair_pt && pair_tet && det_pm && ssum)) throw WaeError(WAE_ERR_INVALID, "bad flame pair arguments");
        if (npair_r > 0 && !(pair_pt_r && g_pm)) throw WaeError(WAE_ERR_INVALID, "bad reference pair arguments");
        if (ref_tet < 0 || ref_tet >= ntets) throw WaeError(WAE_ERR_INVALID, "reference tetrahedron out of range");
        check_indices(pair_tet, npair, ntets, "pair index out of range");
        check_indices(pair_pt, npair, npoints, "pair index out of range");
        check_indices(pair_pt_r, npair_r, npoints, "pair index out of range");
        check_tets(tets, ntets, npoints);
        HIP_CHECK(hipSetDevice(device));
        Dev<double> dpts(points, (size_t)npoints * 3);
        Dev<cplx> dv((const cplx *)v, (size_t)npoints), dva((const cplx *)v_adj, (size_t)npoints);
        Dev<int> dt(tets, (size_t)ntets * 4);
        if (npair > 0) {
            Dev<int> dpp(pair_pt, (size_t)npair), dpt(pair_tet, (size_t)npair);
            Dev<double> ddet((size_t)npair * 6);
            Dev<cplx> dss((size_t)npair);
            hipLaunchKernelGGL(shape_flame_kernel, grid_for(npair * 3), dim3(256), 0, 0, dpts.p, dt.p, npair, dpp.p, dpt.p, dva.p, h, ddet.p, dss.p);
            HIP_CHECK(hipGetLastError());
            ddet.to_host(det_pm, (size_t)npair * 6);
            dss.to_host((cplx *)ssum, (size_t)npair);
        }
        const size_t nr = (size_t)npair_r;
        Dev<int> dpr(pair_pt_r, nr);
        Dev<cplx> dg(nr * 6 + 1);
        hipLaunchKernelGGL(shape_ref_kernel, dim3((unsigned)((nr * 6 + 1 + 63) / 64)), dim3(64), 0, 0, dpts.p, dt.p, ref_tet, npair_r, dpr.p, n_ref[0], n_ref[1],
                           n_ref[2], dv.p, h, dg.p, dg.p + nr * 6);
        HIP_CHECK(hipGetLastError());
        dg.to_host((cplx *)g_pm, nr * 6);
        dg.to_host((cplx *)g0, 1, nr * 6);
        return WAE_OK;
    });
}

int wae_p1_info(const void *handle, int64_t *npoints, int64_t *nnz) {
    return wae_guarded([&]() {
        if (!handle) throw WaeError(WAE_ERR_INVALID, "null handle");
        const P1Handle *H = (const P1Handle *)handle;
        if (npoints) *npoints = H->np;
        if (nnz) *nnz = H->nnz;
        return WAE_OK;
    });
}

int wae_p1_get(const void *handle, int32_t *rowptr, int32_t *col, double *mass, double *stiff) {
    return wae_guarded([&]() {
        if (!handle) throw WaeError(WAE_ERR_INVALID, "null handle");
        const P1Handle *H = (const P1Handle *)handle;
        if (rowptr) memcpy(rowptr, H->rowptr.data(), H->rowptr.size() * sizeof(int));
        if (col) memcpy(col, H->col.data(), H->col.size() * sizeof(int));
        if (mass) memcpy(mass, H->m.data(), H->m.size() * sizeof(double));
        if (stiff) memcpy(stiff, H->k.data(), H->k.size() * sizeof(double));
        return WAE_OK;
    });
}

int wae_p1_free(void *handle) {
    delete (P1Handle *)handle;
    return WAE_OK;
}

}  // extern "C"
