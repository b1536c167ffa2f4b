// Forced response (wae_forced_response, at the end): the two kernels that keep a frequency sweep in HBM.  Both work on the solver's
// interleaved batch layout X[row][b] (leading dimension nb = the chunk's columns, one excitation frequency per column) and in the handle's
// row numbering -- the host maps the caller's row indices through the inverse permutation before it uploads them.  gfx950 only.
//
//   forced_rhs_kernel      B[row][b] = sum_s g[b][s] m[row][s]   on the rows that carry a source entry (the rest of B was cleared)
//   forced_observe_kernel  H[q][j0 + b] = sum_i w_q[i] X[idx_q[i]][b]
//
// Neither uses an atomic, and every sum runs in an order fixed by the launch geometry alone: the same bits on every call.
#include <cmath>

#include "block_reduce.h"
#include "solver.h"

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

// ----------------------------------------------------------------------------------------------------
// the host side: a frequency sweep that stays in HBM (the solves go through solver.h)
// ----------------------------------------------------------------------------------------------------
// a family of sparse complex vectors in compressed form (ptr: n+1 offsets, idx: 0-based rows in the caller's numbering), checked
static void check_sparse_vectors(const char *what, int32_t n, const int64_t *ptr, const int32_t *idx, const double *val, int64_t d) {
    const std::string w(what);
    WAE_REQUIRE(n >= 0, w + ": negative count");
    if (n == 0) return;
    WAE_REQUIRE(ptr, w + ": ptr is required");
    WAE_REQUIRE(ptr[0] == 0, w + ": ptr must start at 0");
    for (int32_t s = 0; s < n; ++s) WAE_REQUIRE(ptr[s + 1] >= ptr[s], w + ": ptr decreases");
    const int64_t nnz = ptr[n];
    WAE_REQUIRE(nnz == 0 || (idx && val), w + ": idx and val are required");
    for (int64_t i = 0; i < nnz; ++i) {
        WAE_REQUIRE(idx[i] >= 0 && idx[i] < d, w + ": index outside 0..d-1");
        WAE_REQUIRE(std::isfinite(val[2 * i]) && std::isfinite(val[2 * i + 1]), w + ": value that is not finite");
    }
}

extern "C" {

int wae_forced_response(wae_family *h, int32_t nfreq, const double *coeff_table, int32_t nsrc, const int64_t *src_ptr, const int32_t *src_idx,
                        const double *src_val, const double *src_coeff, int32_t nobs, const int64_t *obs_ptr, const int32_t *obs_idx,
                        const double *obs_val, double *H_out, int32_t nkeep, const int32_t *keep, double *X_out, double tol, int32_t maxit,
                        wae_solve_info *info) {
    return guarded([&]() {
        WAE_REQUIRE(h && nfreq >= 0, "bad argument");
        if (nfreq == 0) {                                         // an empty sweep: nothing is read, nothing is written
            if (info) std::memset(info, 0, sizeof(*info));
            return WAE_OK;
        }
        const int64_t d = h->d;
        const int T = h->T;
        WAE_REQUIRE(coeff_table, "coeff_table is required");
        for (size_t i = 0; i < (size_t)nfreq * T * 2; ++i) WAE_REQUIRE(std::isfinite(coeff_table[i]), "coeff_table: coefficient that is not finite");
        check_sparse_vectors("source vectors", nsrc, src_ptr, src_idx, src_val, d);
        WAE_REQUIRE(nsrc == 0 || src_coeff, "src_coeff is required");
        for (size_t i = 0; i < (size_t)nfreq * std::max(nsrc, 0) * 2; ++i) WAE_REQUIRE(std::isfinite(src_coeff[i]), "src_coeff: coefficient that is not finite");
        check_sparse_vectors("observers", nobs, obs_ptr, obs_idx, obs_val, d);
        WAE_REQUIRE(nkeep >= 0 && (nkeep == 0 || keep), "bad keep list");
        for (int32_t k = 0; k < nkeep; ++k)
            WAE_REQUIRE(keep[k] >= 0 && keep[k] < nfreq && (k == 0 || keep[k] > keep[k - 1]), "keep must hold strictly ascending frequency indices in 0..nfreq-1");
        WAE_REQUIRE(nobs > 0 || nkeep > 0, "nothing was asked for: no observer and no kept solution");
        WAE_REQUIRE((nobs == 0 || H_out) && (nkeep == 0 || X_out), "an output array is missing");
        require_solver(h);
        HIP_CHECK(hipSetDevice(h->device));
        hipStream_t st = h->stream;
        CallInfo ci;
        // caller's row -> internal row (the inverse of the handle's permutation)
        std::vector<int> inv;
        if (!h->perm_h.empty()) {
            inv.resize((size_t)d);
            for (int64_t i = 0; i < d; ++i) inv[(size_t)h->perm_h[(size_t)i]] = (int)i;
        }
        auto internal = [&](int32_t row) { return inv.empty() ? (int)row : inv[(size_t)row]; };
        // The source vectors merged into one ascending list of distinct rows with an nsrc-wide value table: the fill kernel then writes
        // every (row, column) from exactly one thread.  Indices that repeat inside a vector add up, in the order they were given.
        struct Entry { int row, s; zc v; };
        std::vector<Entry> ent;
        for (int32_t s = 0; s < nsrc; ++s)
            for (int64_t i = src_ptr[s]; i < src_ptr[s + 1]; ++i) ent.push_back(Entry{internal(src_idx[i]), s, zc(src_val[2 * i], src_val[2 * i + 1])});
        std::stable_sort(ent.begin(), ent.end(), [](const Entry &a, const Entry &b) { return a.row < b.row; });
        std::vector<int> rows;
        std::vector<cplx> mtab;
        for (const Entry &e : ent) {
            if (rows.empty() || rows.back() != e.row) { rows.push_back(e.row); mtab.resize(mtab.size() + (size_t)nsrc, cplx{0.0, 0.0}); }
            cplx &m = mtab[mtab.size() - (size_t)nsrc + (size_t)e.s];
            m.x += e.v.real(); m.y += e.v.imag();
        }
        const int64_t nr = (int64_t)rows.size();
        DevBuf<int> drows, dobs_idx;
        DevBuf<int64_t> dobs_ptr;
        DevBuf<cplx> dm, dg, dobs_val, dH, dX;
        if (nr) {
            drows.upload(rows.data(), rows.size(), st);
            dm.upload(mtab.data(), mtab.size(), st);
            dg.upload((const cplx *)src_coeff, (size_t)nfreq * nsrc, st);
        }
        std::vector<int> oidx;
        if (nobs) {
            const int64_t onnz = obs_ptr[nobs];
            oidx.resize((size_t)onnz);
            for (int64_t i = 0; i < onnz; ++i) oidx[(size_t)i] = internal(obs_idx[i]);
            dobs_ptr.upload(obs_ptr, (size_t)nobs + 1, st);
            dobs_idx.upload(oidx.data(), oidx.size(), st);
            dobs_val.upload((const cplx *)obs_val, (size_t)onnz, st);
            dH.alloc((size_t)nobs * nfreq);
        }
        if (nkeep) dX.alloc((size_t)d * nkeep);
        // (experiment) WAE_FORCED_POLISH=1: penalty_polish on every chunk before it is observed.  Off: from a zero guess the Krylov process
        // delivers the speaker rows, whose unknowns are O(A), to the tolerance of the solve (DESIGN.md "Forced response").
        static const int polish = env_int("WAE_FORCED_POLISH", 0);
        int k0 = 0;                                               // first kept frequency not yet written
        for (int c0 = 0; c0 < nfreq; c0 += h->NB) {
            const int nb = std::min(h->NB, nfreq - c0);
            const Batch bt = Batch::per_column(nb, WAE_OP_N);                // one coefficient set per column, as wae_solve with ncoef == r
            std::vector<std::vector<zc>> pcs((size_t)nb);
            for (int b = 0; b < nb; ++b) plane_coeffs(h, coeff_table + (size_t)(c0 + b) * 2 * T, WAE_OP_N, pcs[(size_t)b]);
            launch_fill_zero(h->Bs.p, (size_t)d * nb, st);
            launch_forced_rhs(drows.p, dm.p, nr, nsrc, dg.p + (size_t)c0 * nsrc, h->Bs.p, nb, st);
            solve_chunk(h, bt, pcs, h->Bs.p, h->Xs.p, tol, maxit, &ci.li);
            if (polish) penalty_polish(h, bt, h->Bs.p, h->Xs.p);
            launch_forced_observe(dobs_ptr.p, dobs_idx.p, dobs_val.p, nobs, h->Xs.p, nb, dH.p, c0, st);
            while (k0 < nkeep && keep[k0] < c0 + nb) {                        // kept columns leave in runs of neighbouring frequencies
                int k1 = k0 + 1;
                while (k1 < nkeep && keep[k1] < c0 + nb && keep[k1] == keep[k1 - 1] + 1) ++k1;
                launch_inter_to_colmajor(h->Xs.p + (keep[k0] - c0), nb, d, k1 - k0, dX.p + (size_t)k0 * d, st, h->perm());
                k0 = k1;
            }
        }
        if (nobs) HIP_CHECK(hipMemcpyAsync(H_out, dH.p, (size_t)nobs * nfreq * sizeof(cplx), hipMemcpyDeviceToHost, st));
        if (nkeep) HIP_CHECK(hipMemcpyAsync(X_out, dX.p, (size_t)d * nkeep * sizeof(cplx), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        return ci.finish(info);
    });
}

}   // extern "C"
