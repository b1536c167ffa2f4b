// Galerkin products C = P^T A P on the device, for the levels of a hierarchy whose prolongators the caller supplies
// (wae_solver_setup_nested, setup.hip).  A is a square CSR plane in HBM, P a real CSR prolongator with short rows (a nested P1
// hierarchy: one or two entries per row).
//   1. One thread per stored entry (i, j, v) of A finds its row i (binary search in the row pointer) and counts |P_i| * |P_j|.
//   2. An exclusive scan (hipCUB) of the counts gives every entry its place in the triplet list; the total is checked against the
//      count the sort takes before anything of that size is allocated.
//   3. One thread per entry writes its triplets (a * n_c + b, w_a w_b v), a over row i of P, b over row j of P, with 64-bit keys.
//      The entry stream (column, value, row, offset) is read coalesced, the two P rows are gathers of a few words each.
//   4. triplets_to_csr_dev (assemble.hip): stable radix sort, reduce-by-key, row pointer.  Real and imaginary parts are its two value
//      streams; a real plane carries one.
// No atomics: the triplets are written in the order of A's entries and the stable sort keeps that order among equal keys, so every sum
// is formed in a fixed order and two products of the same inputs have the same bits.  Structural zeros are kept (planes of one pattern
// keep one pattern), as the host products keep them.
#include <hipcub/hipcub.hpp>

#include <vector>

#include "wae_internal.h"

namespace {

typedef unsigned long long u64;

inline dim3 gal_grid(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }

// row[e] = the row of entry e (ptr[row] <= e < ptr[row + 1]); cnt[e] = |P_row| * |P_col[e]|
__global__ __launch_bounds__(256) void galerkin_count_kernel(const int *__restrict__ aptr, const int *__restrict__ acol, int64_t n, int64_t nnz,
                                                             const int *__restrict__ pptr, int *__restrict__ row, u64 *__restrict__ cnt) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= nnz) return;
    int64_t lo = 0, hi = n;                                 // the last row with ptr[row] <= e
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)aptr[mid] <= e) lo = mid; else hi = mid;
    }
    const int i = (int)lo, j = acol[e];
    row[e] = i;
    cnt[e] = (u64)(pptr[i + 1] - pptr[i]) * (u64)(pptr[j + 1] - pptr[j]);
}

// the triplets of entry e at off[e] .. off[e] + cnt[e] - 1 (a outer, b inner)
template <bool CPLX>
__global__ __launch_bounds__(256) void galerkin_expand_kernel(const int *__restrict__ row, const int *__restrict__ acol, const double *__restrict__ are,
                                                              const double *__restrict__ aim, int64_t nnz, const int *__restrict__ pptr,
                                                              const int *__restrict__ pcol, const double *__restrict__ pval, u64 nc,
                                                              const u64 *__restrict__ off, u64 total, u64 *__restrict__ keys,
                                                              double *__restrict__ vre, double *__restrict__ vim) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= nnz) return;
    const int i = row[e], j = acol[e];
    const int a0 = pptr[i], a1 = pptr[i + 1], b0 = pptr[j], b1 = pptr[j + 1];
    const double re = are[e], im = CPLX ? aim[e] : 0.0;
    u64 o = off[e];
    for (int a = a0; a < a1; ++a) {
        const u64 ka = (u64)pcol[a] * nc;
        const double wa = pval[a];
        for (int b = b0; b < b1; ++b, ++o) {
            if (o >= total) return;                         // (never: off and total come from the same counts)
            const double w = wa * pval[b];
            keys[o] = ka + (u64)pcol[b];
            vre[o] = w * re;
            if (CPLX) vim[o] = w * im;
        }
    }
}

template <class T> void gal_download(std::vector<T> &dst, const T *src, size_t count) {
    dst.resize(count);
    if (count) HIP_CHECK(hipMemcpy(dst.data(), src, count * sizeof(T), hipMemcpyDeviceToHost));
}

}  // namespace

void upload_plane(const CsrZ &A, DevPlane &D) {
    D.n = A.n; D.nnz = A.nnz();
    D.real = true;
    std::vector<double> re((size_t)D.nnz), im((size_t)D.nnz);
    for (int64_t p = 0; p < D.nnz; ++p) {
        re[(size_t)p] = A.val[(size_t)p].real();
        im[(size_t)p] = A.val[(size_t)p].imag();
        if (im[(size_t)p] != 0.0) D.real = false;
    }
    D.ptr.alloc((size_t)A.n + 1); D.col.alloc((size_t)D.nnz); D.re.alloc((size_t)D.nnz);
    HIP_CHECK(hipMemcpy(D.ptr.p, A.ptr.data(), ((size_t)A.n + 1) * sizeof(int), hipMemcpyHostToDevice));
    if (D.nnz) {
        HIP_CHECK(hipMemcpy(D.col.p, A.col.data(), (size_t)D.nnz * sizeof(int), hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(D.re.p, re.data(), (size_t)D.nnz * sizeof(double), hipMemcpyHostToDevice));
    }
    D.im.release();
    if (!D.real) {
        D.im.alloc((size_t)D.nnz);
        HIP_CHECK(hipMemcpy(D.im.p, im.data(), (size_t)D.nnz * sizeof(double), hipMemcpyHostToDevice));
    }
}

void upload_prolongator(const CsrD &P, DevProlongator &D) {
    D.n = P.n; D.m = P.m; D.nnz = P.nnz();
    D.ptr.alloc((size_t)P.n + 1); D.col.alloc((size_t)D.nnz); D.val.alloc((size_t)D.nnz);
    HIP_CHECK(hipMemcpy(D.ptr.p, P.ptr.data(), ((size_t)P.n + 1) * sizeof(int), hipMemcpyHostToDevice));
    if (D.nnz) {
        HIP_CHECK(hipMemcpy(D.col.p, P.col.data(), (size_t)D.nnz * sizeof(int), hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(D.val.p, P.val.data(), (size_t)D.nnz * sizeof(double), hipMemcpyHostToDevice));
    }
}

int64_t galerkin_device(const DevPlane &A, const DevProlongator &P, DevPlane &C, CsrZ &host) {
    if (A.n != P.n) throw WaeError(WAE_ERR_INVALID, "galerkin_device: the prolongator's rows are not the plane's");
    const int64_t nc = P.m;
    host = CsrZ();
    host.n = host.m = nc;
    host.ptr.assign((size_t)nc + 1, 0);
    C.n = nc; C.nnz = 0; C.real = A.real;
    C.ptr.alloc((size_t)nc + 1);
    C.col.release(); C.re.release(); C.im.release();
    u64 total = 0;
    Dev<int> row((size_t)A.nnz);
    Dev<u64> cnt((size_t)A.nnz), off((size_t)A.nnz);
    if (A.nnz) {
        hipLaunchKernelGGL(galerkin_count_kernel, gal_grid(A.nnz), dim3(256), 0, 0, A.ptr.p, A.col.p, A.n, A.nnz, P.ptr.p, row.p, cnt.p);
        HIP_CHECK(hipGetLastError());
        size_t tb = 0;
        HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, cnt.p, off.p, (int)A.nnz));
        Dev<char> tmp(tb);
        HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(tmp.p, tb, cnt.p, off.p, (int)A.nnz));
        u64 last[2] = {0, 0};
        HIP_CHECK(hipMemcpy(&last[0], off.p + (A.nnz - 1), sizeof(u64), hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(&last[1], cnt.p + (A.nnz - 1), sizeof(u64), hipMemcpyDeviceToHost));
        total = last[0] + last[1];
    }
    if (total > (u64)WAE_GALERKIN_MAX_TRIPLETS)
        throw WaeError(WAE_ERR_INVALID, "a Galerkin product of the supplied prolongators expands to " + std::to_string(total) +
                                            " triplets, more than the 2^31 - 1 the device pipeline takes");
    if (total == 0) {                                        // nothing stored: an empty plane
        HIP_CHECK(hipMemset(C.ptr.p, 0, ((size_t)nc + 1) * sizeof(int)));
        return 0;
    }
    TripletCsr T;
    {
        Dev<u64> keys((size_t)total);
        Dev<double> vre((size_t)total), vim(A.real ? 1 : (size_t)total);
        if (A.real)
            hipLaunchKernelGGL(galerkin_expand_kernel<false>, gal_grid(A.nnz), dim3(256), 0, 0, row.p, A.col.p, A.re.p, (const double *)nullptr, A.nnz,
                               P.ptr.p, P.col.p, P.val.p, (u64)nc, off.p, total, keys.p, vre.p, (double *)nullptr);
        else
            hipLaunchKernelGGL(galerkin_expand_kernel<true>, gal_grid(A.nnz), dim3(256), 0, 0, row.p, A.col.p, A.re.p, A.im.p, A.nnz, P.ptr.p, P.col.p,
                               P.val.p, (u64)nc, off.p, total, keys.p, vre.p, vim.p);
        HIP_CHECK(hipGetLastError());
        triplets_to_csr_dev(nc, (size_t)total, keys, vre, A.real ? nullptr : &vim, T);
    }
    const size_t nnz = (size_t)T.nnz;
    // the host copy (tile plan, operator groups, dense level); the row pointer of the rows without entries is filled here and goes back
    std::vector<int> col;
    std::vector<double> re, im;
    gal_download(host.ptr, T.rowptr.p, (size_t)nc + 1);
    gal_download(col, T.col.p, nnz);
    gal_download(re, T.m.p, nnz);
    if (!A.real) gal_download(im, T.k.p, nnz);
    host.ptr[(size_t)nc] = (int)nnz;
    for (int64_t r = nc - 1; r >= 0; --r)
        if (host.ptr[(size_t)r] < 0) host.ptr[(size_t)r] = host.ptr[(size_t)r + 1];
    host.col = std::move(col);
    host.val.resize(nnz);
    for (size_t p = 0; p < nnz; ++p) host.val[p] = zc(re[p], A.real ? 0.0 : im[p]);
    // the device copy, cut to its size (the pipeline's arrays have the length of the triplet list)
    C.nnz = (int64_t)nnz;
    HIP_CHECK(hipMemcpy(C.ptr.p, host.ptr.data(), ((size_t)nc + 1) * sizeof(int), hipMemcpyHostToDevice));
    C.col.alloc(nnz); C.re.alloc(nnz);
    HIP_CHECK(hipMemcpy(C.col.p, T.col.p, nnz * sizeof(int), hipMemcpyDeviceToDevice));
    HIP_CHECK(hipMemcpy(C.re.p, T.m.p, nnz * sizeof(double), hipMemcpyDeviceToDevice));
    if (!A.real) {
        C.im.alloc(nnz);
        HIP_CHECK(hipMemcpy(C.im.p, T.k.p, nnz * sizeof(double), hipMemcpyDeviceToDevice));
    }
    return (int64_t)total;
}
