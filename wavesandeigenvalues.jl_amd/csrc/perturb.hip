// libwaehip.so -- adjoint perturbation.  Host code only (kernels: vec.hip, kernels.hip); the solves and the slot columns go through solver.h.
// The one recurrence behind wae_perturb / wae_perturb_slots (nsys = 1) and wae_perturb_batch /
// wae_perturb_batch_slots, for nsys eigenpairs in lock-step.  Every vector of the batch is an interleaved block [row][system] of
// leading dimension nb, the series is N+1 such blocks.
// Per order: the partition weights of every system on the host (they need lambda_1..k-1 of that system), ONE tall-skinny product, ONE
// multi-input SpMV per plane pass, ONE inner product with the left vectors, ONE read-back of the nsys numerators -- the only host
// synchronisation of an order outside the solve --, ONE fused right-hand side, ONE lock-step solve, the projection dots and ONE fused
// projection update.  All device work space is carved out of ONE buffer the entry point hands in: a buffer of its own, released on
// return (the batched calls), or the family's grow-only pt_ws (the single-pair calls: a Newton step of the Householder iteration makes
// one per start value, and a dozen hipMalloc / hipFree pairs per call showed up there).
#include <cmath>

#include "solver.h"

// Kelleher's accelerated ascending-composition generator (same order as perturbation.jl:2-80)
template <class F> static void for_each_partition(int n, F &&f) {
    std::vector<int> a(n + 1, 0);
    int k = 1, y = n - 1;
    while (k != 0) {
        int x = a[k - 1] + 1;
        k -= 1;
        while (2 * x <= y) { a[k] = x; y -= x; k += 1; }
        const int l = k + 1;
        while (x <= y) {
            a[k] = x; a[l] = y;
            f(a.data(), k + 2);
            x += 1; y -= 1;
        }
        a[k] = x + y;
        y = x + y - 1;
        f(a.data(), k + 1);
    }
}

// G[i*T + t] = weight of v_i in the input column of term t at order k (perturbation.jl:394-415 regrouped)
static void perturb_weights(int k, int N, int T, const double *coeff_table, const std::vector<zc> &lam, std::vector<zc> &G) {
    auto F = [&](int m, int n, int t) { const size_t e = ((size_t)(m * (N + 1) + n) * T + t) * 2; return zc(coeff_table[e], coeff_table[e + 1]); };
    G.assign((size_t)k * T, zc(0));
    auto addF = [&](int i, int m, int n, zc coeff) {
        for (int t = 0; t < T; ++t) G[(size_t)i * T + t] += coeff * F(m, n, t);
    };
    for (int n = 1; n <= k; ++n) addF(k - n, 0, n, 1.0);
    std::vector<int> mu;
    for (int mw = 1; mw <= k; ++mw)
        for_each_partition(mw, [&](const int *p, int len) {
            if (len == 1 && p[0] == k) return;
            mu.assign(mw, 0);
            for (int i = 0; i < len; ++i) mu[p[i] - 1]++;
            double mn = std::tgamma((double)len + 1.0);
            zc coeff = 1.0;
            for (int g = 0; g < mw; ++g)
                if (mu[g]) {
                    mn /= std::tgamma((double)mu[g] + 1.0);
                    coeff *= std::pow(lam[g + 1], mu[g]);
                }
            coeff *= mn;
            for (int n = 0; n <= k - mw; ++n) {
                if (k == 1 && len == 1) continue;
                addF(k - n - mw, len, n, coeff);
            }
        });
}

// The batch keeps its own width.  WAE_PERTURB_PAD=1 (A/B measurements): batches of 2..7 systems run as a full 8-column chunk (columns
// of zeros with the coefficients of system 0), which puts every operator product of the solves on the tile kernel -- measured at 500k
// unknowns, 4 systems, order 10: 0.66 s padded against 0.43 s at the batch's own width (four single-pair calls: 0.65 s), so it is off.
static int perturb_batch_width(const wae_family *h, int nsys) {
    static const int pad = env_int("WAE_PERTURB_PAD", 0);
    return (pad && nsys >= 2 && nsys < 8 && h->NB >= 8) ? 8 : nsys;
}

// v0c / v0adjc: d x nsys column-major on the DEVICE; in the caller's row numbering if `permuted` (host vectors), else the library's (slots).
// nvec_out: v_0 .. v_{nvec_out-1} of every system go to v_out (if not null); ws: see above
static int perturb_batch_core(wae_family *h, int32_t nsys, const double *coeff_tables, int32_t N, const cplx *v0c, const cplx *v0adjc, bool permuted,
                              int32_t norm_mode_in, const double *coeffsY, double tol, int32_t maxit, double *lambda_out, double *v_out, int nvec_out,
                              int32_t *status_out, wae_solve_info *info, DevBuf<cplx> &ws) {
    const bool skip_last = (norm_mode_in & 16) != 0;
    const int norm_mode = norm_mode_in & 15;
    WAE_REQUIRE(norm_mode >= 0 && norm_mode <= 2 && (norm_mode != 2 || coeffsY), "bad norm_mode");
    hipStream_t st = h->stream;
    CallInfo ci;
    wae_solve_info &li = ci.li;
    const int64_t d = h->d;
    const int T = h->T, ns = nsys, npl = h->nplanes;
    const int nb = perturb_batch_width(h, ns);
    const size_t vec = (size_t)d * nb;
    const size_t tsz = (size_t)(N + 1) * (N + 1) * T * 2;         // doubles per coefficient table
    const int *perm = permuted ? h->perm() : nullptr;
    const int nser = skip_last ? std::max(N, 1) : N + 1;          // (the eigenvalue series needs v_0..v_{N-1} only)
    WAE_REQUIRE(nvec_out >= 0 && nvec_out <= nser, "bad argument");
    // plane passes of the multi-input SpMV (coefficient term_scale per term: the weights live in G), the same for every order
    std::vector<std::vector<int>> plane_terms(npl);
    for (int t = 0; t < T; ++t) plane_terms[h->term_plane[t]].push_back(t);
    size_t npass = 0;
    for (auto &v : plane_terms) npass = std::max(npass, v.size());
    // the work space: series | T input columns | five vectors | weights | coefficients | dots | plane tables (L(1,0), Y, passes) | pass columns
    const size_t sizes[] = {vec * nser, vec * T, vec * 5, (size_t)std::max(N, 1) * T * nb, (size_t)2 * nb, (size_t)(N + 2) * nb,
                            (size_t)nb * npl, (size_t)nb * npl, npass * npl, (npass * npl * sizeof(int) + sizeof(cplx) - 1) / sizeof(cplx)};
    size_t total = 0;
    for (size_t n : sizes) total += n;
    ws.reserve(total);
    const size_t *next = sizes;
    cplx *carve = ws.p;
    auto take = [&]() { cplx *p = carve; carve += *next++; return p; };
    cplx *PV = take(), *Ub = take(), *rb = take(), *Gd = take(), *coef = take(), *dotsd = take(), *pc1 = take(), *pcY = take(), *pcM = take();
    int *pcolM = (int *)take();
    cplx *rhs = rb + vec, *u10 = rhs + vec, *wl = u10 + vec, *tmp = wl + vec, *V0 = PV;
    auto put = [&](auto *dst, const auto &src) { HIP_CHECK(hipMemcpyAsync(dst, src.data(), src.size() * sizeof(src[0]), hipMemcpyHostToDevice, st)); };
    std::vector<cplx> hc((size_t)2 * nb), hd((size_t)nb), Gc;
    std::vector<unsigned char> dead(ns, 0);
    std::vector<int> status(ns, WAE_OK);

    // level-0 plane table of `n` coefficient rows (row i from coeffs(i)); rows n..nb-1 repeat row 0
    auto plane_table = [&](cplx *dst, int n, auto &&coeffs, int op) {
        std::vector<cplx> tab((size_t)nb * npl);
        std::vector<zc> pc;
        for (int i = 0; i < nb; ++i) {
            if (i < n) plane_coeffs(h, coeffs(i), op, pc);
            if (i < n) slot_coeffs(h, h->slot_plane[0], pc, &tab[(size_t)i * npl]);
            else std::copy(tab.begin(), tab.begin() + npl, tab.begin() + (size_t)i * npl);
        }
        put(dst, tab);
        HIP_CHECK(hipStreamSynchronize(st));                        // (tab is a stack vector)
    };
    auto applyY = [&](int op, const cplx *x, cplx *y) {            // pcY holds the table of that op
        launch_spmv(h->ops[0].dev(op), pcY, 1 << 30, x, y, nullptr, 0.0, nb, MODE_AX, st);
    };
    auto dots_to = [&](const cplx *a, const cplx *b, cplx *out) { launch_dots(a, 0, 1, b, d, nb, h->partial.p, out, st); };   // out[s] = a_s^H b_s
    auto ipY_to = [&](const cplx *a, const cplx *b, cplx *out) {   // a^H Y b (mode 2) or a^H b
        if (norm_mode == 2) { applyY(WAE_OP_N, b, tmp); dots_to(a, tmp, out); }
        else dots_to(a, b, out);
    };
    auto read_dots = [&](const cplx *src) {                        // -> hd[0..nb)
        HIP_CHECK(hipMemcpyAsync(hd.data(), src, (size_t)nb * sizeof(cplx), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
    };
    // out = a_s x (+ c_s y) with host coefficients; systems given up (and the padding) get zeros.  Always called after a read_dots:
    // the previous upload of hc has completed
    auto scale_cols = [&](const std::vector<zc> &a, const cplx *x, const std::vector<zc> *c, const cplx *y, cplx *out) {
        for (int s = 0; s < nb; ++s) {
            const bool on = s < ns && !dead[s];
            hc[s] = on ? cplx{a[s].real(), a[s].imag()} : cplx{0.0, 0.0};
            hc[nb + s] = (on && c) ? cplx{(*c)[s].real(), (*c)[s].imag()} : cplx{0.0, 0.0};
        }
        put(coef, hc);
        launch_pt_axpby_cols(coef, x, y ? y : x, out, d, nb, st);
    };
    auto give_up = [&](int s, int code) { dead[s] = 1; status[s] = code; };
    auto finite = [](zc z) { return std::isfinite(z.real()) && std::isfinite(z.imag()); };

    launch_colmajor_to_inter(v0c, d, ns, V0, nb, st, perm);
    launch_colmajor_to_inter(v0adjc, d, ns, wl, nb, st, perm);
    if (norm_mode == 2) plane_table(pcY, 1, [&](int) { return coeffsY; }, WAE_OP_N);
    std::vector<zc> fac(ns), fac2(ns);
    {                                                               // v0 /= sqrt(ip(v0, v0))
        ipY_to(V0, V0, dotsd);
        read_dots(dotsd);
        for (int s = 0; s < ns; ++s) {
            fac[s] = 1.0 / std::sqrt(zc(hd[s].x, hd[s].y));
            if (!finite(fac[s])) give_up(s, WAE_ERR_NAN);
        }
        scale_cols(fac, V0, nullptr, nullptr, V0);
    }
    std::vector<std::vector<zc>> lam(ns, std::vector<zc>(N + 1, zc(0)));
    std::vector<int> order_iters;
    if (N >= 1) {
        plane_table(pc1, ns, [&](int s) { return coeff_tables + (size_t)s * tsz + (size_t)(1 * (N + 1) + 0) * T * 2; }, WAE_OP_N);
        launch_spmv(h->ops[0].dev(WAE_OP_N), pc1, 1, V0, u10, nullptr, 0.0, nb, MODE_AX, st);          // u10_s = L_s(1,0) v0_s
        if (norm_mode == 2) {                                       // perturbation.jl:493-494
            std::vector<std::vector<zc>> pcs(1);
            plane_coeffs(h, coeffsY, WAE_OP_N, pcs[0]);
            solve_chunk(h, Batch::one_system(nb, WAE_OP_N), pcs, wl, tmp, tol, maxit, &li);      // v0Adj = Y \ v0Adj
            applyY(WAE_OP_N, u10, rhs);
            dots_to(tmp, rhs, dotsd);                             // v0Adj' Y L10 v0
            read_dots(dotsd);
            for (int s = 0; s < ns; ++s) { fac[s] = 1.0 / zc(hd[s].x, hd[s].y); if (!finite(fac[s])) give_up(s, WAE_ERR_NAN); }
            scale_cols(fac, tmp, nullptr, nullptr, rb);             // v0Adj /= s
            plane_table(pcY, 1, [&](int) { return coeffsY; }, WAE_OP_C);
            applyY(WAE_OP_C, rb, wl);                               // wl = Y' v0Adj
            plane_table(pcY, 1, [&](int) { return coeffsY; }, WAE_OP_N);
        } else {
            dots_to(wl, u10, dotsd);                              // v0Adj' L10 v0
            read_dots(dotsd);
            for (int s = 0; s < ns; ++s) { fac[s] = 1.0 / zc(hd[s].x, hd[s].y); if (!finite(fac[s])) give_up(s, WAE_ERR_NAN); }
            scale_cols(fac, wl, nullptr, nullptr, wl);
        }
        dots_to(wl, u10, dotsd);
        read_dots(dotsd);
        std::vector<zc> denom(ns);
        for (int s = 0; s < ns; ++s) denom[s] = zc(hd[s].x, hd[s].y);
        // the solves: one coefficient set L_s(0,0) per column
        const Batch bt = Batch::per_column(nb, WAE_OP_N);
        std::vector<std::vector<zc>> pcs(nb);
        for (int s = 0; s < nb; ++s) plane_coeffs(h, coeff_tables + (size_t)(s < ns ? s : 0) * tsz, WAE_OP_N, pcs[s]);
        bool l00_ready = false;      // set up lazily: order-1 Newton steps (skip_last) never solve with L(0,0), which is exactly
                                     // singular for small dense families (the reference would throw there)
        {
            std::vector<cplx> tab(npass * npl);
            std::vector<int> pcol(npass * npl);
            for (size_t ps = 0; ps < npass; ++ps)
                for (int sidx = 0; sidx < npl; ++sidx) {
                    const int q = h->slot_plane[0][sidx];
                    if (ps < plane_terms[q].size()) {
                        const int t = plane_terms[q][ps];
                        const zc c = h->term_scale[t];
                        tab[ps * npl + sidx] = cplx{c.real(), c.imag()};
                        pcol[ps * npl + sidx] = t;
                    } else { tab[ps * npl + sidx] = cplx{0.0, 0.0}; pcol[ps * npl + sidx] = 0; }
                }
            put(pcM, tab);
            put(pcolM, pcol);
            HIP_CHECK(hipStreamSynchronize(st));
        }
        const OpDev A0 = h->ops[0].dev(WAE_OP_N);
        std::vector<zc> G, minus_one(ns, zc(-1.0)), mlam(ns);
        std::vector<double> rr(nb);
        for (int k = 1; k <= N; ++k) {
            Gc.assign((size_t)k * T * nb, cplx{0.0, 0.0});
            for (int s = 0; s < ns; ++s) {
                if (dead[s]) continue;
                perturb_weights(k, N, T, coeff_tables + (size_t)s * tsz, lam[s], G);
                for (size_t e = 0; e < (size_t)k * T; ++e) Gc[e * nb + s] = cplx{G[e].real(), G[e].imag()};
            }
            put(Gd, Gc);                                            // (complete before this order's read-back returns)
            launch_pt_gemm_batch(PV, vec, k, Gd, Ub, d, T, nb, st);
            for (size_t ps = 0; ps < npass; ++ps)
                launch_pt_spmv_batch(A0, pcM + ps * npl, pcolM + ps * npl, Ub, T, rb, nb, ps > 0, st);
            dots_to(wl, rb, dotsd);
            read_dots(dotsd);                                     // the order's one read-back: lambda_k of every system
            for (int s = 0; s < ns; ++s) {
                if (dead[s]) continue;
                lam[s][k] = -zc(hd[s].x, hd[s].y) / denom[s];
                if (!finite(lam[s][k])) { lam[s][k] = 0; give_up(s, WAE_ERR_NAN); }
                mlam[s] = -lam[s][k];
            }
            if (skip_last && k == N) break;
            scale_cols(minus_one, rb, &mlam, u10, rhs);             // rhs = -(r + lam_k L10 v0)
            cplx *vk = PV + (size_t)k * vec;
            if (!l00_ready) { upload_pc(h, pcs); dense_setup(h, bt); l00_ready = true; }
            order_iters.push_back(gmres(h, bt, rhs, vk, tol, maxit, &li, nullptr, false, rr.data()));
            for (int s = 0; s < ns; ++s)
                if (!dead[s] && !(rr[s] <= tol) && status[s] == WAE_OK) status[s] = WAE_WARN_MAXITER;
            ipY_to(V0, vk, dotsd);                                // v0' [Y] v_k
            int nd = 1;
            if (norm_mode >= 1)
                for (int l = 1; l < k; ++l, ++nd) ipY_to(PV + (size_t)l * vec, PV + (size_t)(k - l) * vec, dotsd + (size_t)nd * nb);
            launch_pt_project(vk, V0, dotsd, nd, d, nb, st);      // v_k -= (v0' [Y] v_k) v0;  v_k += c v0
        }
    }
    if (v_out) {                                                    // nsys blocks of d x (N+1), the caller's row numbering
        for (int k = 0; k < nvec_out; ++k) {
            launch_inter_to_colmajor(PV + (size_t)k * vec, nb, d, ns, Ub, st, h->perm());
            for (int s = 0; s < ns; ++s)
                HIP_CHECK(hipMemcpyAsync(v_out + ((size_t)s * (N + 1) + k) * d * 2, Ub + (size_t)s * d, (size_t)d * sizeof(cplx), hipMemcpyDeviceToHost, st));
        }
    }
    HIP_CHECK(hipStreamSynchronize(st));
    for (int s = 0; s < ns; ++s)
        for (int k = 1; k <= N; ++k) { lambda_out[((size_t)s * (N + 1) + k) * 2] = lam[s][k].real(); lambda_out[((size_t)s * (N + 1) + k) * 2 + 1] = lam[s][k].imag(); }
    if (status_out) for (int s = 0; s < ns; ++s) status_out[s] = status[s];
    if (getenv("WAE_PERTURB_DEBUG")) {
        fprintf(stderr, "[perturb_batch] nsys=%d nb=%d N=%d lock-step iterations per order:", ns, nb, N);
        for (int it : order_iters) fprintf(stderr, " %d", it);
        fprintf(stderr, "\n");
    }
    int rc_ = ci.finish(info);
    for (int s = 0; s < ns; ++s) if (status[s] != WAE_OK && rc_ == WAE_OK) rc_ = WAE_WARN_MAXITER;
    return rc_;
}

static void perturb_batch_check(wae_family *h, int32_t nsys, const double *coeff_tables, int32_t N, const double *lambda_out) {
    WAE_REQUIRE(h && coeff_tables && lambda_out && N >= 0 && N <= 200, "bad argument");
    require_solver(h);
    WAE_REQUIRE(nsys >= 1 && nsys <= h->NB, "nsys must be between 1 and the solver batch width");
    HIP_CHECK(hipSetDevice(h->device));
}

// the single-pair calls: one system, the family's work space, v_0..v_{N-1} also with norm_mode + 16 (no solve at order N); a system
// the recurrence gave up is an error of the call
static int perturb_single(wae_family *h, const double *coeff_table, int32_t N, const cplx *v0c, const cplx *v0adjc, bool permuted, int32_t norm_mode,
                          const double *coeffsY, double tol, int32_t maxit, double *lambda_out, double *v_out, wae_solve_info *info) {
    int32_t status = WAE_OK;
    const int rc = perturb_batch_core(h, 1, coeff_table, N, v0c, v0adjc, permuted, norm_mode, coeffsY, tol, maxit, lambda_out, v_out,
                                      (norm_mode & 16) ? std::max(N, 1) : N + 1, &status, info, h->pt_ws);
    if (status == WAE_ERR_NAN) throw WaeError(WAE_ERR_NAN, "perturbation: a normalisation or an eigenvalue coefficient is not finite");
    return rc;
}

extern "C" {

int wae_perturb(wae_family *h, const double *coeff_table, int32_t N, const double *v0, const double *v0adj, int32_t norm_mode, const double *coeffsY,
                double tol, int32_t maxit, double *lambda_out, double *v_out, wae_solve_info *info) {
    return guarded([&]() {
        WAE_REQUIRE(h && coeff_table && v0 && v0adj && lambda_out && v_out && N >= 0 && N <= 200, "bad argument");
        perturb_batch_check(h, 1, coeff_table, N, lambda_out);
        const size_t d = (size_t)h->d;
        h->io_a.reserve(2 * d);
        HIP_CHECK(hipMemcpyAsync(h->io_a.p, v0, d * sizeof(cplx), hipMemcpyHostToDevice, h->stream));
        HIP_CHECK(hipMemcpyAsync(h->io_a.p + d, v0adj, d * sizeof(cplx), hipMemcpyHostToDevice, h->stream));
        return perturb_single(h, coeff_table, N, h->io_a.p, h->io_a.p + d, true, norm_mode, coeffsY, tol, maxit, lambda_out, v_out, info);
    });
}

int wae_perturb_slots(wae_family *h, const double *coeff_table, int32_t N, int32_t v_slot, int32_t v_col, int32_t vadj_slot, int32_t vadj_col,
                      int32_t norm_mode, const double *coeffsY, double tol, int32_t maxit, double *lambda_out, double *v_out, wae_solve_info *info) {
    return guarded([&]() {
        WAE_REQUIRE(h && coeff_table && lambda_out && N >= 0 && N <= 200, "bad argument");
        perturb_batch_check(h, 1, coeff_table, N, lambda_out);
        return perturb_single(h, coeff_table, N, slot_col(h, v_slot, v_col), slot_col(h, vadj_slot, vadj_col), false, norm_mode, coeffsY, tol, maxit,
                              lambda_out, v_out, info);
    });
}

int wae_perturb_batch(wae_family *h, int32_t nsys, const double *coeff_tables, int32_t N, const double *v0, const double *v0adj, int32_t norm_mode,
                      const double *coeffsY, double tol, int32_t maxit, double *lambda_out, double *v_out, int32_t *status_out, wae_solve_info *info) {
    return guarded([&]() {
        perturb_batch_check(h, nsys, coeff_tables, N, lambda_out);
        WAE_REQUIRE(v0 && v0adj, "bad argument");
        const size_t cnt = (size_t)h->d * nsys;
        DevBuf<cplx> in;
        in.alloc(2 * cnt);
        HIP_CHECK(hipMemcpyAsync(in.p, v0, cnt * sizeof(cplx), hipMemcpyHostToDevice, h->stream));
        HIP_CHECK(hipMemcpyAsync(in.p + cnt, v0adj, cnt * sizeof(cplx), hipMemcpyHostToDevice, h->stream));
        DevBuf<cplx> ws;
        return perturb_batch_core(h, nsys, coeff_tables, N, in.p, in.p + cnt, true, norm_mode, coeffsY, tol, maxit, lambda_out, v_out,
                                  (norm_mode & 16) ? 0 : N + 1, status_out, info, ws);
    });
}

int wae_perturb_batch_slots(wae_family *h, int32_t nsys, const double *coeff_tables, int32_t N, int32_t v_slot, const int32_t *v_cols, int32_t vadj_slot,
                            const int32_t *vadj_cols, int32_t norm_mode, const double *coeffsY, double tol, int32_t maxit, double *lambda_out,
                            double *v_out, int32_t *status_out, wae_solve_info *info) {
    return guarded([&]() {
        perturb_batch_check(h, nsys, coeff_tables, N, lambda_out);
        WAE_REQUIRE(v_cols && vadj_cols, "bad argument");
        DevBuf<cplx> sv, sw;                                        // (non-consecutive columns are gathered into these)
        const cplx *v = slot_cols_ptr(h, v_slot, v_cols, nsys, sv, h->stream);
        const cplx *w = slot_cols_ptr(h, vadj_slot, vadj_cols, nsys, sw, h->stream);
        DevBuf<cplx> ws;
        return perturb_batch_core(h, nsys, coeff_tables, N, v, w, false, norm_mode, coeffsY, tol, maxit, lambda_out, v_out,
                                  (norm_mode & 16) ? 0 : N + 1, status_out, info, ws);
    });
}

}   // extern "C"
