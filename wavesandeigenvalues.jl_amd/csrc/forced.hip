// Forced response (wae_forced_response, lib.hip): the two kernels that keep a frequency sweep in HBM.  Both work on the solver's
// interleaved batch layout X[row][b] (leading dimension nb = the chunk's columns, one excitation frequency per column) and in the handle's
// row numbering -- the host maps the caller's row indices through the inverse permutation before it uploads them.  gfx950 only.
//
//   forced_rhs_kernel      B[row][b] = sum_s g[b][s] m[row][s]   on the rows that carry a source entry (the rest of B was cleared)
//   forced_observe_kernel  H[q][j0 + b] = sum_i w_q[i] X[idx_q[i]][b]
//
// Neither uses an atomic, and every sum runs in an order fixed by the launch geometry alone: the same bits on every call.
#include "block_reduce.h"

// One thread per (source row, column).  rows: the nr distinct rows that any source vector touches, ascending; M: [nr][nsrc] the value of
// every source vector on that row (0 where it has none; repeated indices already summed by the host); G: [nb][nsrc] the scalar
// coefficients of the chunk's frequencies.  Each (row, column) is written by exactly one thread; the sum over s runs in index order.
// Consecutive threads write consecutive columns of a row: nb * 16 contiguous bytes.
__global__ __launch_bounds__(256) void forced_rhs_kernel(const int *__restrict__ rows, const cplx *__restrict__ M, int64_t nr, int nsrc,
                                                         const cplx *__restrict__ G, cplx *__restrict__ B, int nb) {
    const size_t total = (size_t)nr * nb;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const size_t r = e / nb;
        const int b = (int)(e - r * nb);
        cplx acc = {0.0, 0.0};
        for (int s = 0; s < nsrc; ++s) cfma(acc, G[(size_t)b * nsrc + s], M[r * nsrc + s]);
        B[(size_t)rows[r] * nb + b] = acc;
    }
}

void launch_forced_rhs(const int *rows, const cplx *M, int64_t nr, int nsrc, const cplx *G, cplx *B, int nb, hipStream_t st) {
    if (!nr || !nb) return;
    hipLaunchKernelGGL(forced_rhs_kernel, dim3(grid_for((size_t)nr * nb)), dim3(256), 0, st, rows, M, nr, nsrc, G, B, nb);
    HIP_CHECK(hipGetLastError());
}

// One workgroup per (observer q, group of up to FORCED_COLS columns).  Thread t owns column c0 + t % w and the entries rl, rl + R, ... of
// the observer (rl = t / w, R = 256 / w; threads beyond R * w idle), so a wavefront reads w consecutive columns of 64 / w rows of X: whole
// 16-byte elements side by side.  A point probe (4 or 10 entries) is done after one step with most threads adding nothing; a surface average
// over thousands of nodes takes entries / R steps.  The thread's own sum runs in entry order, block_colsum (serial arm) adds the R partial
// sums of a column in index order.  Repeated indices inside an observer simply add up.
constexpr int FORCED_COLS = 64;
__global__ __launch_bounds__(256) void forced_observe_kernel(const int64_t *__restrict__ ptr, const int *__restrict__ idx, const cplx *__restrict__ val,
                                                             const cplx *__restrict__ X, int nb, cplx *__restrict__ H, int nobs, int64_t j0) {
    __shared__ cplx sm[256];
    const int q = blockIdx.x, c0 = blockIdx.y * FORCED_COLS;
    const int w = min(FORCED_COLS, nb - c0);
    const int tid = threadIdx.x;
    const int R = 256 / w;
    const int b = tid % w, rl = tid / w;
    cplx acc = {0.0, 0.0};
    if (rl < R)
        for (int64_t i = ptr[q] + rl; i < ptr[q + 1]; i += R) cfma(acc, val[i], X[(size_t)idx[i] * nb + c0 + b]);
    const cplx s = block_colsum<false, 256>(acc, w, sm);
    if (tid < w) H[(size_t)q + (size_t)nobs * (size_t)(j0 + c0 + tid)] = s;
}

void launch_forced_observe(const int64_t *ptr, const int *idx, const cplx *val, int nobs, const cplx *X, int nb, cplx *H, int64_t j0, hipStream_t st) {
    if (!nobs || !nb) return;
    hipLaunchKernelGGL(forced_observe_kernel, dim3((unsigned)nobs, (unsigned)((nb + FORCED_COLS - 1) / FORCED_COLS)), dim3(256), 0, st, ptr, idx, val, X,
                       nb, H, nobs, j0);
    HIP_CHECK(hipGetLastError());
}
