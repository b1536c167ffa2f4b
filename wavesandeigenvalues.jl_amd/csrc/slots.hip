// libwaehip.so -- device-resident multivectors ("slots"): wae_slot_write / _read / _axpby / _forms, and the column access that the Arnoldi and
// perturbation units use (solver.h).  Host code only.  The Newton-type solvers iterate on a handful of vectors per start value (right and left
// eigenvector estimates, the Ritz vectors of the step): with the processes' inputs and outputs in host memory a Householder step of 8
// start values at 1M DoF moved 2 GB over PCIe into freshly touched pages and spent as long in host copies as the GPU spent computing
// (45 % idle in the kernel trace).  A slot holds d x ncols in the library's row numbering; the calls below read and write slot columns
// in place of host arrays, so that an iteration touches host memory once at its start and once at its end.
#include "solver.h"

static wae_family::Slot &slot_ref(wae_family *h, int32_t slot) {
    WAE_REQUIRE(slot >= 0 && slot < WAE_NSLOTS, "slot index out of range");
    return h->slots[slot];
}
cplx *slot_col(wae_family *h, int32_t slot, int32_t col) {
    wae_family::Slot &S = slot_ref(h, slot);
    WAE_REQUIRE(S.ncols > 0, "slot is empty");
    WAE_REQUIRE(col >= 0 && col < S.ncols, "slot column out of range");
    return S.buf.p + (size_t)col * h->d;
}
const cplx *slot_cols_ptr(wae_family *h, int32_t slot, const int32_t *cols, int n, DevBuf<cplx> &stage, hipStream_t st) {
    WAE_REQUIRE(cols && n >= 1, "bad argument");
    bool consecutive = true;
    for (int i = 0; i < n; ++i) { (void)slot_col(h, slot, cols[i]); consecutive = consecutive && cols[i] == cols[0] + i; }
    if (consecutive) return slot_col(h, slot, cols[0]);
    stage.reserve((size_t)n * h->d);
    for (int i = 0; i < n; ++i) launch_copy(slot_col(h, slot, cols[i]), stage.p + (size_t)i * h->d, (size_t)h->d, st);
    return stage.p;
}

extern "C" {

int wae_slot_write(wae_family *h, int32_t slot, int32_t ncols_total, int32_t col0, int32_t ncols, const double *X) {
    return guarded([&]() {
        WAE_REQUIRE(h && ncols_total >= 1 && ncols_total <= 256 && col0 >= 0 && ncols >= 0 && col0 + ncols <= ncols_total && (ncols == 0 || X), "bad argument");
        HIP_CHECK(hipSetDevice(h->device));
        hipStream_t st = h->stream;
        wae_family::Slot &S = slot_ref(h, slot);
        const int64_t d = h->d;
        if (S.ncols != ncols_total) {                        // (re)created: zero columns
            S.buf.alloc((size_t)d * ncols_total);
            S.ncols = ncols_total;
            launch_fill_zero(S.buf.p, (size_t)d * ncols_total, st);
        }
        if (ncols) {
            h->io_a.reserve((size_t)d * ncols);
            HIP_CHECK(hipMemcpyAsync(h->io_a.p, X, (size_t)d * ncols * sizeof(cplx), hipMemcpyHostToDevice, st));
            for (int c = 0; c < ncols; ++c) launch_colmajor_to_inter(h->io_a.p + (size_t)c * d, d, 1, S.buf.p + (size_t)(col0 + c) * d, 1, st, h->perm());
        }
        HIP_CHECK(hipStreamSynchronize(st));
        return WAE_OK;
    });
}

int wae_slot_read(wae_family *h, int32_t slot, int32_t col0, int32_t ncols, double *X) {
    return guarded([&]() {
        WAE_REQUIRE(h && col0 >= 0 && ncols >= 0 && (ncols == 0 || X), "bad argument");
        if (!ncols) return WAE_OK;
        HIP_CHECK(hipSetDevice(h->device));
        hipStream_t st = h->stream;
        (void)slot_col(h, slot, col0);
        (void)slot_col(h, slot, col0 + ncols - 1);
        const int64_t d = h->d;
        h->io_b.reserve((size_t)d * ncols);
        for (int c = 0; c < ncols; ++c) launch_inter_to_colmajor(slot_col(h, slot, col0 + c), 1, d, 1, h->io_b.p + (size_t)c * d, st, h->perm());
        HIP_CHECK(hipMemcpyAsync(X, h->io_b.p, (size_t)d * ncols * sizeof(cplx), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        return WAE_OK;
    });
}

int wae_slot_axpby(wae_family *h, int32_t n, int32_t dst_slot, const int32_t *dst_cols, int32_t src_slot, const int32_t *src_cols, const double *alpha,
                   const double *beta, int32_t conj_src) {
    return guarded([&]() {
        WAE_REQUIRE(h && n >= 0 && (n == 0 || (dst_cols && src_cols && alpha && beta)), "bad argument");
        HIP_CHECK(hipSetDevice(h->device));
        hipStream_t st = h->stream;
        for (int i = 0; i < n; ++i) {
            cplx *y = slot_col(h, dst_slot, dst_cols[i]);
            const cplx *x = slot_col(h, src_slot, src_cols[i]);
            launch_axpby1(cplx{alpha[2 * i], alpha[2 * i + 1]}, x, cplx{beta[2 * i], beta[2 * i + 1]}, y, y, (size_t)h->d, st, conj_src ? 1 : 0);
        }
        HIP_CHECK(hipStreamSynchronize(st));
        return WAE_OK;
    });
}

int wae_slot_forms(wae_family *h, int32_t n, const double *coeffs, int32_t op, int32_t a_slot, const int32_t *a_cols, int32_t b_slot, const int32_t *b_cols,
                   double *out) {
    return guarded([&]() {
        WAE_REQUIRE(h && n >= 0 && (n == 0 || (coeffs && a_cols && b_cols && out)), "bad argument");
        WAE_REQUIRE(op == WAE_OP_N || op == WAE_OP_C || op == WAE_OP_T, "bad op");
        if (!n) return WAE_OK;
        WAE_REQUIRE(n <= 256, "more than 256 forms in one call");
        HIP_CHECK(hipSetDevice(h->device));
        hipStream_t st = h->stream;
        const int64_t d = h->d;
        const int T = h->T;
        const size_t vec = (size_t)d * n;
        h->io_b.reserve(3 * vec);
        cplx *Bi = h->io_b.p, *ABi = Bi + vec, *Ai = ABi + vec;
        launch_colmajor_to_inter(slot_cols_ptr(h, b_slot, b_cols, n, h->io_a, st), d, n, Bi, n, st, nullptr);
        launch_colmajor_to_inter(slot_cols_ptr(h, a_slot, a_cols, n, h->io_a, st), d, n, Ai, n, st, nullptr);
        std::vector<cplx> tab((size_t)n * h->nplanes);
        std::vector<zc> pc;
        for (int i = 0; i < n; ++i) {
            plane_coeffs(h, coeffs + (size_t)i * 2 * T, op, pc);
            slot_coeffs(h, h->slot_plane[0], pc, &tab[(size_t)i * h->nplanes]);
        }
        h->pt_pcd.upload(tab.data(), tab.size(), st);
        launch_spmv(h->ops[0].dev(op), h->pt_pcd.p, 1, Bi, ABi, nullptr, 0.0, n, MODE_AX, st);
        h->partial.reserve((size_t)1024 * 32 * std::max(n, 8));      // (launch_dots: DOT_BLOCKS x vectors x columns; the solver set-up allocates more)
        h->pt_Gd.reserve((size_t)n);
        launch_dots(Ai, 0, 1, ABi, d, n, h->partial.p, h->pt_Gd.p, st);
        std::vector<cplx> r(n);
        HIP_CHECK(hipMemcpyAsync(r.data(), h->pt_Gd.p, (size_t)n * sizeof(cplx), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        for (int i = 0; i < n; ++i) { out[2 * i] = r[i].x; out[2 * i + 1] = r[i].y; }
        return WAE_OK;
    });
}

}   // extern "C"
