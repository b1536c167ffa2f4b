// libwaehip.so -- wae_debug_vec (include/waehip.h, "test hook"): ONE launch_* call of wae_internal.h on the caller's host arrays, so
// that tests/ can pin every streaming and reduction kernel to a reference of its own.  No family, no solver set-up.
// wae_debug_gmres: a script of launch_gmres_* calls against one GmresDev, for the recurrence kernels of the lock-step GMRES.
#include <algorithm>
#include <vector>

#include "family.h"

namespace {
struct StreamGuard {
    hipStream_t s = nullptr;
    ~StreamGuard() { if (s) (void)hipStreamDestroy(s); }
};
// entries spanned by nv vectors of blk entries each, `stride` apart
int64_t span(int64_t nv, int64_t stride, int64_t blk) { return nv > 0 ? (nv - 1) * stride + blk : 0; }
}   // namespace

extern "C" int wae_debug_vec(int32_t device, int32_t op, const int64_t *sz, int32_t nsz, double *const *bufs, const int64_t *lens, int32_t nbuf,
                             const uint8_t *cmask, const int32_t *perm, int32_t *status_out) {
    return guarded([&]() {
        WAE_REQUIRE(sz && nsz >= 2 && nsz <= 16 && nbuf >= 0 && nbuf <= 16 && (nbuf == 0 || (bufs && lens)), "bad argument");
        int ndev = 0;
        HIP_CHECK(hipGetDeviceCount(&ndev));
        WAE_REQUIRE(device >= 0 && device < ndev, "no such device");
        for (int i = 0; i < nsz; ++i) WAE_REQUIRE(sz[i] >= 0 && sz[i] <= ((int64_t)1 << 31), "a size is negative or too large");
        for (int i = 0; i < nbuf; ++i) WAE_REQUIRE(lens[i] >= 0 && lens[i] <= ((int64_t)1 << 31), "a buffer length is negative or too large");
        auto S = [&](int i) -> int64_t { WAE_REQUIRE(i < nsz, "too few sizes for this operation"); return sz[i]; };
        WAE_REQUIRE(op != WAE_VEC_DENSE || sz[0] <= 2048, "dense coarse level too large (n > 2048)");   // (before anything is uploaded or launched)
        HIP_CHECK(hipSetDevice(device));
        StreamGuard sg;
        HIP_CHECK(hipStreamCreate(&sg.s));
        hipStream_t st = sg.s;
        DevBuf<cplx> d[16], partial;
        DevBuf<unsigned char> cm;
        DevBuf<int> pm, stat;
        for (int i = 0; i < nbuf; ++i)
            if (bufs[i] && lens[i]) d[i].upload((const cplx *)bufs[i], (size_t)lens[i], st);
        // a required buffer of `count` entries (count = 0: may be absent) / an optional one (absent: null)
        auto need = [&](int i, int64_t count) -> cplx * {
            WAE_REQUIRE(count >= 0 && (count == 0 || (i < nbuf && bufs[i] && lens[i] >= count)), "a buffer is missing or too short");
            return i < nbuf ? d[i].p : nullptr;
        };
        auto opt = [&](int i, int64_t count) -> cplx * { return (i < nbuf && bufs[i]) ? need(i, count) : nullptr; };
        const int64_t n = S(0), nb = S(1);
        WAE_REQUIRE(n >= 1 && n < ((int64_t)1 << 31) && nb >= 1 && nb <= 256, "rows >= 1 and 1 <= nb <= 256");
        const int64_t blk = n * nb;
        auto mask = [&]() -> const unsigned char * {
            if (!cmask) return nullptr;
            cm.upload(cmask, (size_t)(nb + 7) / 8, st);
            return cm.p;
        };
        auto count_of = [&](int i) -> int { const int64_t v = S(i); WAE_REQUIRE(v <= 4096, "a count is too large"); return (int)v; };
        auto want_partial = [&]() { partial.alloc((size_t)std::max(1024 * 32, 768 * 35) * (size_t)nb); return partial.p; };
        switch (op) {
        case WAE_VEC_DOTS: {                      // sz: n, nb, nv, stride   bufs: V, W, out[nv][nb], scale[nv][nb] (optional)
            const int nv = count_of(2);
            const int64_t stride = S(3);
            const cplx *V = need(0, span(nv, stride, blk)), *W = need(1, blk), *scale = opt(3, (int64_t)nv * nb);
            cplx *out = need(2, (int64_t)nv * nb);
            if (scale) launch_dots_scaled(V, (size_t)stride, nv, W, n, (int)nb, want_partial(), out, scale, st, mask());
            else launch_dots(V, (size_t)stride, nv, W, n, (int)nb, want_partial(), out, st, mask());
            break;
        }
        case WAE_VEC_NORMS:                       // sz: n, nb   bufs: X, out[nb]
            launch_norms(need(0, blk), n, (int)nb, want_partial(), need(1, nb), st, mask());
            break;
        case WAE_VEC_DOTS_MULTI: {                // sz: n, nb, nv, nw, sv, sw   bufs: V, W, out[nv][nw][nb]
            const int nv = count_of(2), nw = count_of(3);
            WAE_REQUIRE(nw >= 1 && nw <= 4, "nw in 1..4");
            const cplx *V = need(0, span(nv, S(4), blk)), *W = need(1, span(nw, S(5), blk));
            launch_dots_multi(V, (size_t)S(4), nv, W, (size_t)S(5), nw, n, (int)nb, want_partial(), need(2, (int64_t)nv * nw * nb), st);
            break;
        }
        case WAE_VEC_AXPY_NEG: case WAE_VEC_LINCOMB: case WAE_VEC_LINCOMB_ADD: {     // sz: n, nb, nv, stride   bufs: V, c[nv][nb], W
            const int nv = count_of(2);
            const cplx *V = need(0, span(nv, S(3), blk)), *c = need(1, (int64_t)nv * nb);
            cplx *W = need(2, blk);
            if (op == WAE_VEC_AXPY_NEG) launch_axpy_neg(V, (size_t)S(3), nv, c, W, n, (int)nb, st, mask());
            else if (op == WAE_VEC_LINCOMB) launch_lincomb(V, (size_t)S(3), nv, c, W, n, (int)nb, st);
            else launch_lincomb_add(V, (size_t)S(3), nv, c, W, n, (int)nb, st);
            break;
        }
        case WAE_VEC_AXPY_NEG_NORM: {             // sz: n, nb, nv, stride   bufs: V, h, W, norms[nb], base (optional), inv[nb] (optional)
            const int nv = count_of(2);
            const cplx *V = need(0, span(nv, S(3), blk)), *h = need(1, (int64_t)nv * nb), *base = opt(4, blk);
            cplx *W = need(2, blk), *norms = need(3, nb), *inv = opt(5, nb);
            launch_axpy_neg_norm(V, (size_t)S(3), nv, h, W, n, (int)nb, want_partial(), norms, st, mask(), base, inv);
            break;
        }
        case WAE_VEC_AXPY_NEG_MULTI: {            // sz: n, nb, nv, stride, cnt, wstride   bufs: V, h[nv][cnt][nb], W (cnt vectors)
            const int nv = count_of(2), cnt = count_of(4);
            WAE_REQUIRE(nv >= 1 && cnt >= 1 && cnt <= 4, "nv >= 1, cnt in 1..4");
            const cplx *V = need(0, span(nv, S(3), blk)), *h = need(1, (int64_t)nv * cnt * nb);
            launch_axpy_neg_multi(V, (size_t)S(3), nv, h, need(2, span(cnt, S(5), blk)), (size_t)S(5), cnt, n, (int)nb, st);
            break;
        }
        case WAE_VEC_DOTS2: {                     // sz: n, nb, nv, stride   bufs: V, W1, W2, out1, out2 [nv][nb], gram[3][nb], scale[nv][nb]
            const int nv = count_of(2);
            WAE_REQUIRE(nv >= 1, "nv >= 1");
            const cplx *V = need(0, span(nv, S(3), blk)), *W1 = need(1, blk), *W2 = need(2, blk), *scale = need(6, (int64_t)nv * nb);
            cplx *o1 = need(3, (int64_t)nv * nb), *o2 = need(4, (int64_t)nv * nb), *gram = need(5, 3 * nb);
            launch_dots2_scaled(V, (size_t)S(3), nv, W1, W2, n, (int)nb, want_partial(), o1, o2, gram, scale, st, mask());
            break;
        }
        case WAE_VEC_AXPY2: {                     // sz: n, nb, nv, stride   bufs: V, c1, c2m [nv][nb], alpha[nb], W1, W2, norms[2][nb], inv[2][nb]
            const int nv = count_of(2);
            const cplx *V = need(0, span(nv, S(3), blk)), *c1 = need(1, (int64_t)nv * nb), *c2m = need(2, (int64_t)nv * nb), *al = need(3, nb);
            cplx *W1 = need(4, blk), *W2 = need(5, blk), *norms = need(6, 2 * nb), *inv = need(7, 2 * nb);
            launch_axpy2_norm(V, (size_t)S(3), nv, c1, c2m, al, W1, W2, n, (int)nb, want_partial(), norms, inv, st, mask());
            break;
        }
        case WAE_VEC_LINCOMB_REP: {               // sz: n, nb, nv, stride, l   bufs: Q (nv vectors of n x l), y[nv][nb], X
            const int nv = count_of(2);
            const int64_t l = S(4);
            WAE_REQUIRE(l >= 1 && l <= nb, "l in 1..nb");
            launch_lincomb_rep(need(0, span(nv, S(3), n * l)), (size_t)S(3), nv, need(1, (int64_t)nv * nb), need(2, blk), n, (int)nb, (int)l, st);
            break;
        }
        case WAE_VEC_SCALE_INV:                   // sz: n, nb   bufs: X, alpha[nb], Y
            launch_scale_inv(need(0, blk), need(1, nb), need(2, blk), n, (int)nb, st, mask());
            break;
        case WAE_VEC_MASK_COLS:                   // sz: n, nb   bufs: X, keep[nb]
            launch_mask_cols(need(0, blk), need(1, nb), n, (int)nb, st);
            break;
        case WAE_VEC_EXTRACT_COLS: {              // sz: n, nb, off, l   bufs: X, out (n x l)
            const int64_t off = S(2), l = S(3);
            WAE_REQUIRE(l >= 1 && off + l <= nb, "columns off .. off+l-1 must lie inside the batch");
            launch_extract_cols(need(0, blk), (int)nb, (int)off, (int)l, need(1, n * l), n, st);
            break;
        }
        case WAE_VEC_BEYN_ACCUM: {                // sz: d, nb, l, nsys, npow, lA (0 = l), c0   bufs: X, w[nsys], z[nsys], A[npow][lA][d]; perm[d]
            const int64_t l = S(2), nsys = S(3), npow = S(4), lA = S(5) > 0 ? S(5) : l, c0 = S(6);
            WAE_REQUIRE(l >= 1 && nsys >= 1 && nsys * l <= nb && npow >= 1 && npow <= 64 && c0 + l <= lA && lA <= 4096, "bad moment shape");
            if (perm) {
                for (int64_t i = 0; i < n; ++i) WAE_REQUIRE(perm[i] >= 0 && perm[i] < n, "perm entry out of range");
                pm.upload(perm, (size_t)n, st);
            }
            launch_beyn_accum(need(0, blk), (int)nb, n, (int)l, (int)nsys, need(1, nsys), need(2, nsys), (int)npow, need(3, npow * lA * n), st,
                              (int)S(5), (int)c0, perm ? pm.p : nullptr);
            break;
        }
        case WAE_VEC_PT_GEMM_BATCH: {             // sz: d, nb, k, stride, T   bufs: V, G[k][T][nb], U (d x T x nb)
            const int k = count_of(2), T = count_of(4);
            WAE_REQUIRE(k >= 1 && T >= 1, "k >= 1, T >= 1");
            launch_pt_gemm_batch(need(0, span(k, S(3), blk)), (size_t)S(3), k, need(1, (int64_t)k * T * nb), need(2, blk * T), n, T, (int)nb, st);
            break;
        }
        case WAE_VEC_PT_AXPBY_COLS:               // sz: d, nb   bufs: coef[2][nb], x, y, out
            launch_pt_axpby_cols(need(0, 2 * nb), need(1, blk), need(2, blk), need(3, blk), n, (int)nb, st);
            break;
        case WAE_VEC_PT_PROJECT: {                // sz: d, nb, nd   bufs: vk, v0, dots[nd][nb]
            const int nd = count_of(2);
            WAE_REQUIRE(nd >= 1, "nd >= 1");
            launch_pt_project(need(0, blk), need(1, blk), need(2, (int64_t)nd * nb), nd, n, (int)nb, st);
            break;
        }
        case WAE_VEC_DENSE: {                     // sz: n, nb, nsys, nplanes, op, cps   bufs: planes, pc[nsys][nplanes], Ainv (out), X, Y (optional pair)
            const int64_t nsys = S(2), npl = S(3), dop = S(4), cps = S(5);
            WAE_REQUIRE(nsys >= 1 && nsys <= 256 && npl >= 1 && npl <= WAE_MAXP && dop >= 0 && dop <= 2 && cps >= 1 && (nb - 1) / cps < nsys,
                        "bad dense shape");
            const cplx *planes = need(0, npl * n * n), *pc = need(1, nsys * npl), *X = opt(3, blk);
            cplx *Ainv = need(2, nsys * n * n), *Y = X ? need(4, blk) : nullptr;
            stat.alloc(1);
            HIP_CHECK(hipMemsetAsync(stat.p, 0, sizeof(int), st));
            launch_dense_assemble(planes, (int)npl, (int)n, pc, (int)nsys, (int)dop, Ainv, st);
            launch_dense_invert(Ainv, (int)n, (int)nsys, stat.p, st);
            if (X) launch_dense_apply(Ainv, (int)n, (int)std::min<int64_t>(cps, 1 << 30), X, Y, (int)nb, st, mask());
            if (status_out) HIP_CHECK(hipMemcpyAsync(status_out, stat.p, sizeof(int), hipMemcpyDeviceToHost, st));
            break;
        }
        default:
            throw WaeError(WAE_ERR_INVALID, "wae_debug_vec: unknown operation");
        }
        for (int i = 0; i < nbuf; ++i)
            if (bufs[i] && lens[i]) HIP_CHECK(hipMemcpyAsync(bufs[i], d[i].p, (size_t)lens[i] * sizeof(cplx), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        return WAE_OK;
    });
}

extern "C" int wae_debug_gmres(int32_t device, int32_t nb, int32_t m, int32_t histcap, int64_t n, const double *bnorm, const int64_t *ev,
                               const double *evd, int32_t nev, double *pool, int64_t plen, double *cstate, double *dstate, double *snap_relres,
                               int32_t *snap_int, uint8_t *snap_cmask, double *snap_rescale, double *snap_sv, double *snap_vsq) {
    return guarded([&]() {
        WAE_REQUIRE(bnorm && ev && evd && pool && cstate && dstate && snap_relres && snap_int && snap_cmask && snap_rescale && snap_sv && snap_vsq,
                    "bad argument");
        WAE_REQUIRE(nb >= 1 && nb <= 256, "1 <= nb <= 256");
        WAE_REQUIRE(m >= 1 && m <= 256 && histcap >= 1 && histcap <= 65536 && n >= 1 && n <= 65536 && nev >= 1 && nev <= 4096,
                    "m in 1..256, histcap, n in 1..65536, 1..4096 events");
        WAE_REQUIRE(plen >= 1 && plen <= ((int64_t)1 << 28), "the pool is empty or too large");
        int ndev = 0;
        HIP_CHECK(hipGetDeviceCount(&ndev));
        WAE_REQUIRE(device >= 0 && device < ndev, "no such device");
        // every event is checked before anything is uploaded or launched
        const int64_t N = nb, blk = n * N;
        const cplx *hpool = (const cplx *)pool;
        int ninit = 0;
        for (int e = 0; e < nev; ++e) {
            const int64_t kind = ev[4 * e], j = ev[4 * e + 1], off = ev[4 * e + 3];
            int64_t need = 0;
            switch (kind) {
            case WAE_GMRES_INIT: need = 2 * N; ++ninit; break;
            case WAE_GMRES_STEP:
                WAE_REQUIRE(j >= 0 && j < m, "a step outside the cycle (0 <= j < m)");
                need = (j + 2) * N + blk;
                break;
            case WAE_GMRES_PAIR:
                WAE_REQUIRE(j >= 0 && j + 2 <= m, "a pair step outside the cycle (0 <= j, j + 2 <= m)");
                need = (3 * (j + 1) + (j + 2) + 6) * N + 2 * blk;
                break;
            case WAE_GMRES_SOLVE_Y:
                WAE_REQUIRE(j >= 1 && j <= m, "solve_y: 1 <= ju <= m");
                need = (int64_t)m * N;
                break;
            default: throw WaeError(WAE_ERR_INVALID, "wae_debug_gmres: unknown event");
            }
            WAE_REQUIRE(off >= 0 && off <= plen && need <= plen - off, "an event's arrays do not fit the pool");
        }
        // host-side staging: the `done` bytes of every INIT and the 1/norm^2 rows the vector kernels write in the solver
        const int nch = (nb + 7) / 8, nint = 5 * nb + 4;
        std::vector<unsigned char> hdone((size_t)std::max(ninit, 1) * nb);
        std::vector<cplx> hinv((size_t)nev * 2 * nb, cplx{0.0, 0.0});
        auto inv2 = [](double r) { return cplx{r > 0.0 ? 1.0 / (r * r) : 0.0, 0.0}; };
        for (int e = 0, ii = 0; e < nev; ++e) {
            const int64_t kind = ev[4 * e], j = ev[4 * e + 1], off = ev[4 * e + 3];
            if (kind == WAE_GMRES_INIT) {
                for (int b = 0; b < nb; ++b) hdone[(size_t)ii * nb + b] = hpool[off + N + b].x != 0.0 ? 1 : 0;
                ++ii;
            } else if (kind == WAE_GMRES_STEP) {
                for (int b = 0; b < nb; ++b) hinv[(size_t)e * 2 * nb + b] = inv2(hpool[off + (j + 1) * N + b].x);
            } else if (kind == WAE_GMRES_PAIR) {
                const int64_t onorm = off + (2 * (j + 1) + 3) * N;
                for (int b = 0; b < 2 * nb; ++b) hinv[(size_t)e * 2 * nb + b] = inv2(hpool[onorm + b].x);
            }
        }
        HIP_CHECK(hipSetDevice(device));
        StreamGuard sg;
        HIP_CHECK(hipStreamCreate(&sg.s));
        hipStream_t st = sg.s;
        // the state, laid out as lib.hip run_device lays it out (one integer block: conv, steps, iters, histlen, stalled, status)
        const size_t nR = (size_t)m * (m + 1) * nb, nrow = (size_t)m * nb;
        DevBuf<cplx> dpool, R, sn, g, vsq, Hraw, rescale, dinv, s_rescale, s_vsq;
        DevBuf<double> cs, sv, sub, hist, relres, bn, s_relres, s_sv;
        DevBuf<int> ints, s_int;
        DevBuf<unsigned char> cmask, ddone, s_cmask;
        const cplx *hc = (const cplx *)cstate;
        dpool.upload(hpool, (size_t)plen, st);
        R.upload(hc, nR, st); sn.upload(hc + nR, nrow, st); g.upload(hc + nR + nrow, nrow + nb, st);
        vsq.upload(hc + nR + 2 * nrow + nb, nrow + 2 * nb, st); Hraw.upload(hc + nR + 3 * nrow + 3 * nb, nR, st);
        cs.upload(dstate, nrow, st); sv.upload(dstate + nrow, nrow + 2 * nb, st); sub.upload(dstate + 2 * nrow + 2 * nb, nrow, st);
        hist.upload(dstate + 3 * nrow + 2 * nb, (size_t)histcap * nb, st);
        bn.upload(bnorm, (size_t)nb, st);
        ddone.upload(hdone.data(), hdone.size(), st);
        dinv.upload(hinv.data(), hinv.size(), st);
        relres.alloc(nb); rescale.alloc(nb); ints.alloc(nint); cmask.alloc(nch);
        HIP_CHECK(hipMemsetAsync(ints.p, 0, (size_t)nint * sizeof(int), st));
        HIP_CHECK(hipMemsetAsync(relres.p, 0, (size_t)nb * sizeof(double), st));
        HIP_CHECK(hipMemsetAsync(rescale.p, 0, (size_t)nb * sizeof(cplx), st));
        HIP_CHECK(hipMemsetAsync(cmask.p, 0, (size_t)nch, st));
        s_relres.alloc((size_t)nev * nb); s_int.alloc((size_t)nev * nint); s_cmask.alloc((size_t)nev * nch); s_rescale.alloc((size_t)nev * nb);
        s_sv.alloc((size_t)nev * 2 * nb); s_vsq.alloc((size_t)nev * 2 * nb);
        HIP_CHECK(hipMemsetAsync(s_sv.p, 0, (size_t)nev * 2 * nb * sizeof(double), st));
        HIP_CHECK(hipMemsetAsync(s_vsq.p, 0, (size_t)nev * 2 * nb * sizeof(cplx), st));
        GmresDev S;
        S.nb = nb; S.m = m; S.histcap = histcap;
        S.R = R.p; S.cs = cs.p; S.sn = sn.p; S.g = g.p; S.sv = sv.p; S.vsq = vsq.p;
        S.conv = ints.p; S.steps = S.conv + nb; S.iters = S.steps + nb; S.histlen = S.iters + nb; S.stalled = S.histlen + nb; S.status = S.stalled + nb;
        S.relres = relres.p; S.bnorm = bn.p; S.hist = hist.p; S.rescale = rescale.p; S.cmask = cmask.p;
        S.Hraw = Hraw.p; S.sub = sub.p;
        auto d2d = [&](void *dst, const void *src, size_t bytes) { HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st)); };
        for (int e = 0, ii = 0; e < nev; ++e) {
            const int64_t kind = ev[4 * e], j = ev[4 * e + 1], off = ev[4 * e + 3];
            const int use_mask = ev[4 * e + 2] ? 1 : 0;
            const double tol = evd[2 * e], lim = evd[2 * e + 1];
            cplx *a = dpool.p + off;
            int row0 = -1, rows = 0;                    // the sv / vsq rows this event writes
            if (kind == WAE_GMRES_INIT) {               // pool: beta[nb] done[nb]
                launch_gmres_init(S, a, ddone.p + (size_t)ii * nb, use_mask, st);
                ++ii;
                row0 = 0; rows = 1;
            } else if (kind == WAE_GMRES_STEP) {        // pool: hd[j+2][nb] Vnew[n][nb]
                d2d(vsq.p + (size_t)(j + 1) * nb, dinv.p + (size_t)e * 2 * nb, (size_t)nb * sizeof(cplx));       // (axpy_neg_norm in the solver)
                launch_gmres_step(S, a, (int)j, tol, lim, use_mask, a + (j + 2) * N, n, st);
                row0 = (int)j + 1; rows = 1;
            } else if (kind == WAE_GMRES_PAIR) {        // pool: c1 c2 [j+1][nb] gram[3][nb] norms[2][nb] W1 W2 [n][nb] alpha[nb] c2m[j+1][nb] hd2[j+2][nb]
                cplx *c1 = a, *c2 = c1 + (j + 1) * N, *gram = c2 + (j + 1) * N, *norms = gram + 3 * N, *W1 = norms + 2 * N, *W2 = W1 + blk,
                     *alpha = W2 + blk, *c2m = alpha + N, *hd2 = c2m + (j + 1) * N;
                launch_gmres_pair_coef(S, (int)j, c1, c2, gram, alpha, c2m, hd2, st);
                d2d(vsq.p + (size_t)(j + 1) * nb, dinv.p + (size_t)e * 2 * nb, (size_t)2 * nb * sizeof(cplx));   // (axpy2_norm in the solver)
                launch_gmres_step(S, c1, (int)j, tol, 1e300, use_mask, W1, n, st, norms);
                launch_gmres_step(S, hd2, (int)j + 1, tol, lim, use_mask, W2, n, st, norms + N);
                row0 = (int)j + 1; rows = 2;
            } else {                                    // pool: out[m][nb] (rows < max(ju, steps[b]) are written)
                launch_gmres_solve_y(S, (int)j, a, st);
            }
            d2d(s_relres.p + (size_t)e * nb, relres.p, (size_t)nb * sizeof(double));
            d2d(s_int.p + (size_t)e * nint, ints.p, (size_t)nint * sizeof(int));
            d2d(s_cmask.p + (size_t)e * nch, cmask.p, (size_t)nch);
            d2d(s_rescale.p + (size_t)e * nb, rescale.p, (size_t)nb * sizeof(cplx));
            if (rows) {
                d2d(s_sv.p + (size_t)e * 2 * nb, sv.p + (size_t)row0 * nb, (size_t)rows * nb * sizeof(double));
                d2d(s_vsq.p + (size_t)e * 2 * nb, vsq.p + (size_t)row0 * nb, (size_t)rows * nb * sizeof(cplx));
            }
        }
        auto back = [&](void *dst, const void *src, size_t bytes) { HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st)); };
        cplx *oc = (cplx *)cstate;
        back(pool, dpool.p, (size_t)plen * sizeof(cplx));
        back(oc, R.p, nR * sizeof(cplx)); back(oc + nR, sn.p, nrow * sizeof(cplx)); back(oc + nR + nrow, g.p, (nrow + nb) * sizeof(cplx));
        back(oc + nR + 2 * nrow + nb, vsq.p, (nrow + 2 * nb) * sizeof(cplx)); back(oc + nR + 3 * nrow + 3 * nb, Hraw.p, nR * sizeof(cplx));
        back(dstate, cs.p, nrow * sizeof(double)); back(dstate + nrow, sv.p, (nrow + 2 * nb) * sizeof(double));
        back(dstate + 2 * nrow + 2 * nb, sub.p, nrow * sizeof(double)); back(dstate + 3 * nrow + 2 * nb, hist.p, (size_t)histcap * nb * sizeof(double));
        back(snap_relres, s_relres.p, (size_t)nev * nb * sizeof(double)); back(snap_int, s_int.p, (size_t)nev * nint * sizeof(int));
        back(snap_cmask, s_cmask.p, (size_t)nev * nch); back(snap_rescale, s_rescale.p, (size_t)nev * nb * sizeof(cplx));
        back(snap_sv, s_sv.p, (size_t)nev * 2 * nb * sizeof(double)); back(snap_vsq, s_vsq.p, (size_t)nev * 2 * nb * sizeof(cplx));
        HIP_CHECK(hipStreamSynchronize(st));
        return WAE_OK;
    });
}
