// libwaehip.so -- error state, handle queries and the operator-product entries (wae_spmv_sum*, wae_eig_residuals) of the C ABI.  The handle
// is built in setup.hip; the solvers are in gmres.hip, beyn.hip, forced.hip, arnoldi.hip, slots.hip and perturb.hip (solver.h).
// gfx950 only.  See include/waehip.h for the contract of every exported function.
#include <cmath>

#include "family.h"

static thread_local std::string g_last_error;
void wae_set_error(const std::string &m) { g_last_error = m; }

int wae_internal_device(const wae_family *h) { return h->device; }
hipStream_t wae_internal_stream(const wae_family *h) { return h->stream; }

extern "C" {

const char *wae_last_error(void) { return g_last_error.c_str(); }
const char *wae_version(void) { return "waehip 0.1 (gfx950; fused multi-term CSR SpMV, SA-multigrid GMRES)"; }

int wae_device_count(int *n) {
    return guarded([&]() {
        HIP_CHECK(hipGetDeviceCount(n));
        return WAE_OK;
    });
}

int wae_family_destroy(wae_family *h) {
    return guarded([&]() {
        if (h) {
            (void)hipSetDevice(h->device);
            delete h;
        }
        return WAE_OK;
    });
}

int wae_family_info(const wae_family *h, int64_t *d, int32_t *T, int64_t *nnz_total) {
    return guarded([&]() {
        WAE_REQUIRE(h, "null handle");
        if (d) *d = h->d;
        if (T) *T = h->T;
        if (nnz_total) { int64_t s = 0; for (auto v : h->term_nnz) s += v; *nnz_total = s; }
        return WAE_OK;
    });
}

int64_t wae_family_spmv_bytes(const wae_family *h, const uint8_t *mask, int32_t r) {
    if (!h) return -1;
    int64_t bytes = 0;
    for (int k = 0; k < h->T; ++k)
        if (!mask || mask[k]) bytes += h->term_nnz[k] * 20 + (h->d + 1) * 4;
    return bytes + 2 * (int64_t)r * h->d * 16;
}

int wae_spmv_sum_cols(wae_family *h, const double *coeffs, int32_t ncoef, const double *X, double *Y, int32_t r, int32_t op) {
    return guarded([&]() {
        WAE_REQUIRE(h && r >= 0 && (r == 0 || (coeffs && X && Y)), "bad argument");
        WAE_REQUIRE(op >= 0 && op <= 2, "bad op");
        if (r == 0) return WAE_OK;                                // L(z) * zeros(d, 0): nothing to do (LinOpFam.jl:482-529 returns d x 0)
        WAE_REQUIRE(ncoef == 1 || ncoef == r, "ncoef must be 1 or r");
        HIP_CHECK(hipSetDevice(h->device));
        hipStream_t st = h->stream;
        const size_t cnt = (size_t)h->d * r;
        h->io_a.reserve(cnt); h->io_b.reserve(cnt);
        constexpr int GW = 256;                                   // widest launch (the side-row / long-row scratch is sized for it)
        const int gw = std::min<int>(r, GW);
        DevBuf<cplx> xi, yi;
        xi.alloc((size_t)h->d * gw); yi.alloc((size_t)h->d * gw);
        std::vector<cplx> tab((size_t)ncoef * h->nplanes);
        std::vector<zc> pc;
        for (int s = 0; s < ncoef; ++s) {
            plane_coeffs(h, coeffs + (size_t)s * 2 * h->T, op, pc);
            slot_coeffs(h, h->slot_plane[0], pc, &tab[(size_t)s * h->nplanes]);
        }
        DevBuf<cplx> pcd;
        pcd.upload(tab.data(), tab.size(), st);
        HIP_CHECK(hipMemcpyAsync(h->io_a.p, X, cnt * sizeof(cplx), hipMemcpyHostToDevice, st));
        for (int c0 = 0; c0 < r; c0 += GW) {                      // column groups of at most GW
            const int w = std::min(GW, r - c0);
            launch_colmajor_to_inter(h->io_a.p + (size_t)c0 * h->d, h->d, w, xi.p, w, st, h->perm());
            launch_spmv(h->ops[0].dev(op), ncoef == 1 ? pcd.p : pcd.p + (size_t)c0 * h->nplanes, ncoef == 1 ? (1 << 30) : 1, xi.p, yi.p, nullptr, 0.0,
                        w, MODE_AX, st);
            launch_inter_to_colmajor(yi.p, w, h->d, w, h->io_b.p + (size_t)c0 * h->d, st, h->perm());
        }
        HIP_CHECK(hipMemcpyAsync(Y, h->io_b.p, cnt * sizeof(cplx), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        return WAE_OK;
    });
}

int wae_eig_residuals(wae_family *h, int32_t n, const double *coeff_table, const double *P, uint64_t P_dev, double *res_out) {
    if (h && n > 256 && coeff_table && (P || P_dev) && res_out) {  // pairs are independent: groups of at most 256 (the widest launch)
        for (int32_t j0 = 0; j0 < n; j0 += 256) {
            const int32_t w = std::min<int32_t>(256, n - j0);
            const int rc = wae_eig_residuals(h, w, coeff_table + (size_t)j0 * 2 * h->T, P ? P + (size_t)j0 * 2 * h->d : nullptr,
                                             P_dev ? P_dev + (uint64_t)j0 * h->d * sizeof(cplx) : 0, res_out + j0);
            if (rc != WAE_OK) return rc;
        }
        return WAE_OK;
    }
    return guarded([&]() {
        WAE_REQUIRE(h && n >= 0 && (n == 0 || (coeff_table && (P || P_dev) && res_out)), "bad argument");
        if (n == 0) return WAE_OK;                                // no pairs: nothing to test
        HIP_CHECK(hipSetDevice(h->device));
        hipStream_t st = h->stream;
        const int T = h->T;
        const size_t cnt = (size_t)h->d * n;
        DevBuf<cplx> xi, yi, pcd, nrm, part;
        xi.alloc(cnt); yi.alloc(cnt); nrm.alloc((size_t)n); part.alloc((size_t)1024 * n);
        const cplx *src = (const cplx *)(uintptr_t)P_dev;
        if (!src) {
            h->io_a.reserve(cnt);
            HIP_CHECK(hipMemcpyAsync(h->io_a.p, P, cnt * sizeof(cplx), hipMemcpyHostToDevice, st));
            src = h->io_a.p;
        }
        launch_colmajor_to_inter(src, h->d, n, xi.p, n, st, h->perm());
        std::vector<cplx> tab((size_t)n * h->nplanes), hn(n);
        std::vector<zc> pc;
        auto pass = [&](int only_term, std::vector<double> &out) {     // norms of (sum_k c_jk A_k v_j), k = all or one term
            std::vector<double> ck((size_t)2 * T);
            for (int j = 0; j < n; ++j) {
                for (int k = 0; k < T; ++k) {
                    const bool on = only_term < 0 || k == only_term;
                    ck[2 * k] = on ? coeff_table[((size_t)j * T + k) * 2] : 0.0;
                    ck[2 * k + 1] = on ? coeff_table[((size_t)j * T + k) * 2 + 1] : 0.0;
                }
                plane_coeffs(h, ck.data(), WAE_OP_N, pc);
                slot_coeffs(h, h->slot_plane[0], pc, &tab[(size_t)j * h->nplanes]);
            }
            pcd.upload(tab.data(), tab.size(), st);
            launch_spmv(h->ops[0].dev(WAE_OP_N), pcd.p, 1, xi.p, yi.p, nullptr, 0.0, n, MODE_AX, st);
            launch_norms(yi.p, h->d, n, part.p, nrm.p, st);
            HIP_CHECK(hipMemcpyAsync(hn.data(), nrm.p, (size_t)n * sizeof(cplx), hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
            out.resize(n);
            for (int j = 0; j < n; ++j) out[j] = hn[j].x;
        };
        std::vector<double> num, one, den(n, 0.0);
        pass(-1, num);
        for (int k = 0; k < T; ++k) {
            bool used = false;
            for (int j = 0; j < n && !used; ++j) used = coeff_table[((size_t)j * T + k) * 2] != 0.0 || coeff_table[((size_t)j * T + k) * 2 + 1] != 0.0;
            if (!used) continue;
            pass(k, one);
            for (int j = 0; j < n; ++j) den[j] += one[j];
        }
        for (int j = 0; j < n; ++j) res_out[j] = num[j] / std::max(den[j], 1e-300);
        return WAE_OK;
    });
}

int wae_spmv_sum(wae_family *h, const double *coeffs, const double *X, double *Y, int32_t r, int32_t op) {
    return wae_spmv_sum_cols(h, coeffs, 1, X, Y, r, op);
}

int wae_spmv_sum_multi(wae_family *h, const double *coeffs, const double *X, double *Y) {
    return guarded([&]() {
        WAE_REQUIRE(h && coeffs && X && Y, "bad argument");
        HIP_CHECK(hipSetDevice(h->device));
        hipStream_t st = h->stream;
        // a term aliased onto a shared plane still multiplies its own input column, so expand per TERM:
        // Y = sum_k c_k A_k X[:,k].  Terms sharing a plane are handled by one pass per distinct input column.
        const int T = h->T;
        const size_t cnt = (size_t)h->d * T;
        h->io_a.reserve(cnt); h->io_b.reserve((size_t)h->d);
        DevBuf<cplx> xi, yi, acc, pcd;
        xi.alloc(cnt); yi.alloc((size_t)h->d); acc.alloc((size_t)h->d);
        HIP_CHECK(hipMemcpyAsync(h->io_a.p, X, cnt * sizeof(cplx), hipMemcpyHostToDevice, st));
        launch_colmajor_to_inter(h->io_a.p, h->d, T, xi.p, T, st, h->perm());
        launch_fill_zero(acc.p, (size_t)h->d, st);
        // passes: in pass t every plane takes the t-th term mapped to it (if any)
        std::vector<std::vector<int>> plane_terms(h->nplanes);
        for (int k = 0; k < T; ++k) plane_terms[h->term_plane[k]].push_back(k);
        size_t npass = 0;
        for (auto &v : plane_terms) npass = std::max(npass, v.size());
        std::vector<cplx> tab(h->nplanes);
        std::vector<int> pcol(h->nplanes);
        for (size_t t = 0; t < npass; ++t) {
            for (int s = 0; s < h->nplanes; ++s) {
                const int q = h->slot_plane[0][s];
                if (t < plane_terms[q].size()) {
                    const int k = plane_terms[q][t];
                    const zc c = h->term_scale[k] * zc(coeffs[2 * k], coeffs[2 * k + 1]);
                    tab[s] = cplx{c.real(), c.imag()};
                    pcol[s] = k;
                } else { tab[s] = cplx{0.0, 0.0}; pcol[s] = 0; }
            }
            pcd.upload(tab.data(), tab.size(), st);
            h->plane_col_dev.upload(pcol.data(), pcol.size(), st);
            launch_spmv_multi(h->ops[0].dev(WAE_OP_N), pcd.p, h->plane_col_dev.p, xi.p, yi.p, T, st);
            launch_add(yi.p, acc.p, (size_t)h->d, st);
            HIP_CHECK(hipStreamSynchronize(st));
        }
        launch_inter_to_colmajor(acc.p, 1, h->d, 1, h->io_b.p, st, h->perm());      // back to the caller's row numbering
        HIP_CHECK(hipMemcpyAsync(Y, h->io_b.p, (size_t)h->d * sizeof(cplx), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        return WAE_OK;
    });
}

}   // extern "C"
