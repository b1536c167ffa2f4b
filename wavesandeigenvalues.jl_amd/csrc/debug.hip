// libwaehip.so -- wae_debug_vec (include/waehip.h, "test hook"): ONE launch_* call of wae_internal.h on the caller's host arrays, so
// that tests/ can pin every streaming and reduction kernel to a reference of its own.  No family, no solver set-up.
// wae_debug_gmres: a script of launch_gmres_* calls against one GmresDev, for the recurrence kernels of the lock-step GMRES.
// wae_debug_spmv / _prolong / _vcycle: ONE operator product, prolongation or V-cycle (gmres.hip's own vcycle) of a family that has been set up.
// wae_bench_spmv / _spmv_level / _triad: timed launches.
#include <algorithm>
#include <vector>

#include "solver.h"

namespace {
struct StreamGuard {
    hipStream_t s = nullptr;
    ~StreamGuard() { if (s) (void)hipStreamDestroy(s); }
};
// entries spanned by nv vectors of blk entries each, `stride` apart
int64_t span(int64_t nv, int64_t stride, int64_t blk) { return nv > 0 ? (nv - 1) * stride + blk : 0; }
// the input of the timed launches: xorshift values in [-1, 1), the same on every call
void fill_xorshift(std::vector<cplx> &hx) {
    uint64_t s = 0x9E3779B97F4A7C15ull;
    for (auto &v : hx) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; v.x = (double)(s & 0xFFFFF) / 524288.0 - 1.0; v.y = (double)((s >> 20) & 0xFFFFF) / 524288.0 - 1.0; }
}
// milliseconds per call of one() on the stream: the mean over `reps` calls, after three that are not timed
template <class F> double mean_ms(hipStream_t st, int reps, F &&one) {
    for (int i = 0; i < 3; ++i) one();
    hipEvent_t e0, e1;
    HIP_CHECK(hipEventCreate(&e0));
    HIP_CHECK(hipEventCreate(&e1));
    HIP_CHECK(hipEventRecord(e0, st));
    for (int i = 0; i < reps; ++i) one();
    HIP_CHECK(hipEventRecord(e1, st));
    HIP_CHECK(hipEventSynchronize(e1));
    float ms = 0.f;
    HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return (double)ms / reps;
}
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
        // the state, laid out as gmres.hip run_device lays it out (one integer block: conv, steps, iters, histlen, stalled, status)
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

extern "C" {

int wae_bench_spmv(wae_family *h, const double *coeffs, int32_t r, int32_t reps, double *ms_out) {
    return guarded([&]() {
        WAE_REQUIRE(h && coeffs && r > 0 && reps > 0 && ms_out, "bad argument");
        HIP_CHECK(hipSetDevice(h->device));
        hipStream_t st = h->stream;
        const size_t cnt = (size_t)h->d * r;
        DevBuf<cplx> x, y, pcd;
        x.alloc(cnt); y.alloc(cnt);
        std::vector<cplx> hx(cnt);
        fill_xorshift(hx);
        HIP_CHECK(hipMemcpyAsync(x.p, hx.data(), cnt * sizeof(cplx), hipMemcpyHostToDevice, st));
        std::vector<zc> pc;
        plane_coeffs(h, coeffs, WAE_OP_N, pc);
        std::vector<cplx> tab((size_t)h->nplanes);                 // one system, all columns
        slot_coeffs(h, h->slot_plane[0], pc, tab.data());
        pcd.upload(tab.data(), tab.size(), st);
        const OpDev A = h->ops[0].dev(WAE_OP_N);
        // WAE_BENCH_MODE (diagnostic): the fused form timed -- 0 A X (default), 1 residual, 2 Jacobi sweep, 6 product + first sweep
        const int bmode = getenv("WAE_BENCH_MODE") ? atoi(getenv("WAE_BENCH_MODE")) : MODE_AX;
        DevBuf<cplx> bb;
        if (bmode != MODE_AX) { bb.alloc(cnt); HIP_CHECK(hipMemcpyAsync(bb.p, hx.data(), cnt * sizeof(cplx), hipMemcpyHostToDevice, st)); }
        auto one = [&]() { launch_spmv(A, pcd.p, 1 << 30, x.p, y.p, bmode != MODE_AX ? bb.p : nullptr, 0.8, r, bmode, st); };
        *ms_out = mean_ms(st, reps, one);
        return WAE_OK;
    });
}

int wae_debug_spmv(wae_family *h, int32_t which, int32_t level, int32_t mode, const double *coeffs, int32_t ncoef, const double *X,
                   const double *B, double *Y, double *B2, int32_t r, int32_t op, double jac_w, const uint8_t *cmask, int32_t flags,
                   int64_t *n_in_q, int64_t *n_out_q) {
    return guarded([&]() {
        WAE_REQUIRE(h && which >= 0 && which <= 2 && level >= 0 && op >= 0 && op <= 2, "bad argument");
        WAE_REQUIRE(level == 0 || h->solver_ready, "levels >= 1 need wae_solver_setup");
        // (the last level of a hierarchy is dense: it has no sparse operator to launch)
        WAE_REQUIRE(which == 0 ? (level == 0 || level < (int)h->ops.size() - 1) : level < (int)h->xfer.size(), "no such level");
        const int64_t n_in = which == 0 ? h->ops[level].n : (which == 1 ? h->xfer[level].nf : h->xfer[level].nc);
        const int64_t n_out = which == 0 ? h->ops[level].n : (which == 1 ? h->xfer[level].nc : h->xfer[level].nf);
        if (n_in_q) *n_in_q = n_in;
        if (n_out_q) *n_out_q = n_out;
        if (!X && !Y) return WAE_OK;                               // size query
        WAE_REQUIRE(X && Y && r > 0 && r <= 256, "bad argument (1 <= r <= 256)");
        WAE_REQUIRE(which != 0 || (coeffs && (ncoef == 1 || ncoef == r)), "ncoef must be 1 or r");
        WAE_REQUIRE(mode >= MODE_AX && mode <= MODE_AX_J0 && (which == 0 || mode == (which == 1 ? MODE_AX : MODE_ADD)), "bad mode");
        WAE_REQUIRE(B || mode == MODE_AX || mode == MODE_AX_DS || mode == MODE_AX_J0, "this mode reads B");
        WAE_REQUIRE(mode != MODE_AX_J0 || B2, "mode 6 writes B2");
        HIP_CHECK(hipSetDevice(h->device));
        hipStream_t st = h->stream;
        const int *perm = level == 0 && which != 1 ? h->perm() : nullptr;                 // (numbering of the OUTPUT rows: level 0 is the caller's)
        const int *perm_in = level == 0 && which != 2 ? h->perm() : nullptr;
        DevBuf<cplx> xc, yc, xi, yi, bi, pcd;
        DevBuf<unsigned char> cm;
        const size_t cin = (size_t)n_in * r, cout = (size_t)n_out * r;
        xc.alloc(std::max(cin, cout)); yc.alloc(cout); xi.alloc(cin); yi.alloc(cout); bi.alloc(cout);
        HIP_CHECK(hipMemcpyAsync(xc.p, X, cin * sizeof(cplx), hipMemcpyHostToDevice, st));
        launch_colmajor_to_inter(xc.p, n_in, r, xi.p, r, st, perm_in);
        auto stage = [&](const double *src, cplx *dst) {           // host column-major n_out x r -> interleaved on the device
            HIP_CHECK(hipMemcpyAsync(yc.p, src, cout * sizeof(cplx), hipMemcpyHostToDevice, st));
            launch_colmajor_to_inter(yc.p, n_out, r, dst, r, st, perm);
        };
        stage(Y, yi.p);                                             // a masked chunk keeps what Y held on entry
        if (mode == MODE_AX_J0) stage(B2, bi.p);
        else if (B) stage(B, bi.p);
        if (cmask) cm.upload(cmask, (size_t)(r + 7) / 8, st);
        OpDev A;
        int cps = 1 << 30;
        if (which == 0) {
            std::vector<cplx> tab((size_t)ncoef * h->nplanes);
            std::vector<zc> pc;
            for (int s = 0; s < ncoef; ++s) {
                plane_coeffs(h, coeffs + (size_t)s * 2 * h->T, op, pc);
                slot_coeffs(h, h->slot_plane[level], pc, &tab[(size_t)s * h->nplanes]);
            }
            pcd.upload(tab.data(), tab.size(), st);
            A = h->ops[level].dev(op);
            cps = ncoef == 1 ? (1 << 30) : 1;
        } else {
            A = h->xfer[level].devR();
        }
        if (flags & 1) A.tiles = nullptr;
        const Transfer *xf = which == 0 ? nullptr : &h->xfer[level];
        const bool by_tile = xf && xf->ft.ready && !(flags & 1) && r >= 8;
        if (which == 2) {                                           // Y = B + P X; B and Y the same array: in place.  A masked chunk keeps what Y held
            const cplx *src = (const void *)B == (const void *)Y ? yi.p : bi.p;
            if (by_tile) launch_prolong_tiles(xf->ft.dev, xi.p, src, yi.p, r, st, cmask ? cm.p : nullptr);
            else launch_prolong_add(xf->p_ptr.p, xf->p_col.p, xf->p_val.p, xf->nf, xi.p, src, yi.p, r, st, cmask ? cm.p : nullptr);
        } else
        launch_spmv(A, which == 0 ? pcd.p : h->one_dev.p, cps, xi.p, yi.p, (mode == MODE_AX || mode == MODE_AX_DS) ? nullptr : bi.p, jac_w, r, mode, st,
                    cmask ? cm.p : nullptr);
        launch_inter_to_colmajor(yi.p, r, n_out, r, yc.p, st, perm);
        HIP_CHECK(hipMemcpyAsync(Y, yc.p, cout * sizeof(cplx), hipMemcpyDeviceToHost, st));
        if (mode == MODE_AX_J0) {
            HIP_CHECK(hipStreamSynchronize(st));
            launch_inter_to_colmajor(bi.p, r, n_out, r, yc.p, st, perm);
            HIP_CHECK(hipMemcpyAsync(B2, yc.p, cout * sizeof(cplx), hipMemcpyDeviceToHost, st));
        }
        HIP_CHECK(hipStreamSynchronize(st));
        return WAE_OK;
    });
}

// ONE launch of a prolongation kernel with its norm output (include/waehip.h)
int wae_debug_prolong(wae_family *h, int32_t level, const double *X, const double *B, double *Y, double *norms, int32_t r, const uint8_t *cmask,
                      int32_t flags) {
    return guarded([&]() {
        WAE_REQUIRE(h && X && B && Y && norms, "bad argument");
        require_solver(h);
        WAE_REQUIRE(level >= 0 && level < (int)h->xfer.size(), "no such level");
        WAE_REQUIRE(r >= 1 && r <= 256, "bad argument (1 <= r <= 256)");
        WAE_REQUIRE(flags >= 0 && flags < 4, "unknown flag");
        const Transfer *xf = &h->xfer[level];
        const int64_t nc = xf->nc, nf = xf->nf;
        HIP_CHECK(hipSetDevice(h->device));
        hipStream_t st = h->stream;
        const int *perm = level == 0 ? h->perm() : nullptr;       // level 0 is in the caller's row numbering
        const size_t cin = (size_t)nc * r, cout = (size_t)nf * r;
        const bool by_tile = xf->ft.ready && !(flags & 1) && r >= 8;
        DevBuf<cplx> xc, yc, xi, yi, bi, part, nrm;
        DevBuf<unsigned char> cm;
        xc.alloc(cin); yc.alloc(cout); xi.alloc(cin); yi.alloc(cout); bi.alloc(cout); nrm.alloc((size_t)r);
        part.alloc((size_t)(by_tile ? xf->ft.dev.ntiles : PROLONG_NORM_BLOCKS) * r);
        HIP_CHECK(hipMemcpyAsync(xc.p, X, cin * sizeof(cplx), hipMemcpyHostToDevice, st));
        launch_colmajor_to_inter(xc.p, nc, r, xi.p, r, st, nullptr);
        HIP_CHECK(hipMemcpyAsync(yc.p, Y, cout * sizeof(cplx), hipMemcpyHostToDevice, st));
        launch_colmajor_to_inter(yc.p, nf, r, yi.p, r, st, perm);
        HIP_CHECK(hipStreamSynchronize(st));                       // (yc is staged twice)
        HIP_CHECK(hipMemcpyAsync(yc.p, B, cout * sizeof(cplx), hipMemcpyHostToDevice, st));
        launch_colmajor_to_inter(yc.p, nf, r, bi.p, r, st, perm);
        if (cmask) cm.upload(cmask, (size_t)(r + 7) / 8, st);
        cplx *const dst = (flags & 2) ? nullptr : yi.p;
        if (by_tile) launch_prolong_tiles(xf->ft.dev, xi.p, bi.p, dst, r, st, cmask ? cm.p : nullptr, part.p, nrm.p);
        else launch_prolong_add(xf->p_ptr.p, xf->p_col.p, xf->p_val.p, nf, xi.p, bi.p, dst, r, st, cmask ? cm.p : nullptr, part.p, nrm.p);
        launch_inter_to_colmajor(yi.p, r, nf, r, yc.p, st, perm);
        HIP_CHECK(hipMemcpyAsync(Y, yc.p, cout * sizeof(cplx), hipMemcpyDeviceToHost, st));
        std::vector<cplx> hn((size_t)r);
        HIP_CHECK(hipMemcpyAsync(hn.data(), nrm.p, (size_t)r * sizeof(cplx), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        for (int b = 0; b < r; ++b) norms[b] = hn[(size_t)b].x;
        return WAE_OK;
    });
}

// ONE application of vcycle() -- the solver's own, not a copy -- from `level` down, on the handle's workspaces (include/waehip.h)
int wae_debug_vcycle(wae_family *h, int32_t level, const double *coeffs, int32_t ncoef, const double *B, double *Y, int32_t r, int32_t op,
                     int32_t flags, const uint8_t *cmask) {
    return guarded([&]() {
        WAE_REQUIRE(h && coeffs && B && Y, "bad argument");
        require_solver(h);
        const int L = (int)h->ops.size() - 1;
        WAE_REQUIRE(level >= 0 && level <= L, "no such level");
        WAE_REQUIRE(r >= 1 && r <= h->NB, "r must be in 1..NB (opts[6] of wae_solver_setup)");
        WAE_REQUIRE(ncoef == 1 || ncoef == r, "ncoef must be 1 or r");
        WAE_REQUIRE(op >= 0 && op <= 2, "bad op");
        WAE_REQUIRE(flags >= 0 && flags < 8, "unknown flag");
        WAE_REQUIRE(!(flags & 4) || level == 0, "flags bit 2 (Y = M^-1 A V) needs level 0");
        HIP_CHECK(hipSetDevice(h->device));
        hipStream_t st = h->stream;
        struct LightRestore { bool &on; bool was; ~LightRestore() { on = was; } } light_restore{h->vc_light, h->vc_light};
        h->vc_light = (flags & 1) != 0;
        const Batch bt = ncoef == 1 ? Batch::one_system(r, op) : Batch::per_column(r, op);   // the batch and the plane tables as wae_solve_guess builds them
        std::vector<std::vector<zc>> pcs((size_t)bt.nsys);
        for (int s = 0; s < bt.nsys; ++s) plane_coeffs(h, coeffs + (size_t)s * 2 * h->T, op, pcs[(size_t)s]);
        upload_pc(h, pcs);
        dense_setup(h, bt);
        const int64_t n = h->ops[level].n;
        const size_t cnt = (size_t)n * r;
        const int *perm = level == 0 ? h->perm() : nullptr;       // level 0 is in the caller's row numbering
        DevBuf<cplx> col, vin, fout;
        DevBuf<unsigned char> cm;
        col.alloc(cnt);
        if (cmask) cm.upload(cmask, (size_t)(r + 7) / 8, st);
        const unsigned char *mk = (cmask && r >= 8) ? cm.p : nullptr;   // (narrower batches run unmasked in the solver)
        // what a masked chunk holds on return is what every buffer the cycle may return held before it: the caller's Y
        cplx *x = h->lx[level].p;
        HIP_CHECK(hipMemcpyAsync(col.p, Y, cnt * sizeof(cplx), hipMemcpyHostToDevice, st));
        launch_colmajor_to_inter(col.p, n, r, x, r, st, perm);
        launch_copy(x, h->lt[level].p, cnt, st);
        if (flags & 2) { fout.alloc(cnt); launch_copy(x, fout.p, cnt, st); }
        cplx *b = level == 0 ? h->W.p : h->lb[level].p;            // the right-hand side where the solver keeps it
        HIP_CHECK(hipMemcpyAsync(col.p, B, cnt * sizeof(cplx), hipMemcpyHostToDevice, st));
        bool have_x0 = false;
        if (flags & 4) {                                            // one Krylov step's product and cycle: B is V, b = A V
            vin.alloc(cnt);
            launch_colmajor_to_inter(col.p, n, r, vin.p, r, st, perm);
            have_x0 = L > 0;
            launch_spmv(h->ops[0].dev(op), pc_level(h, 0), bt.cps, vin.p, b, have_x0 ? x : nullptr, have_x0 ? pre_weight(h) : 0.0, r,
                        have_x0 ? MODE_AX_J0 : MODE_AX, st, mk);
        } else {
            launch_colmajor_to_inter(col.p, n, r, b, r, st, perm);
        }
        const cplx *res = vcycle(h, bt, level, b, mk, have_x0, (flags & 2) ? fout.p : nullptr);
        launch_inter_to_colmajor(res, r, n, r, col.p, st, perm);
        HIP_CHECK(hipMemcpyAsync(Y, col.p, cnt * sizeof(cplx), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        return WAE_OK;
    });
}

int wae_bench_spmv_level(wae_family *h, const double *coeffs, int32_t which, int32_t level, int32_t r, int32_t reps, double *ms_out,
                         int64_t *bytes_out) {
    return guarded([&]() {
        WAE_REQUIRE(h && coeffs && which >= 0 && which <= 2 && level >= 0 && r > 0 && r <= 256 && reps > 0 && ms_out, "bad argument");
        require_solver(h);
        WAE_REQUIRE(which == 0 ? (level == 0 || level < (int)h->ops.size() - 1) : level < (int)h->xfer.size(), "no such level");
        HIP_CHECK(hipSetDevice(h->device));
        hipStream_t st = h->stream;
        const int64_t n_in = which == 0 ? h->ops[level].n : (which == 1 ? h->xfer[level].nf : h->xfer[level].nc);
        const int64_t n_out = which == 0 ? h->ops[level].n : (which == 1 ? h->xfer[level].nc : h->xfer[level].nf);
        DevBuf<cplx> x, y, pcd;
        x.alloc((size_t)n_in * r); y.alloc((size_t)n_out * r);
        std::vector<cplx> hx((size_t)n_in * r);
        fill_xorshift(hx);
        HIP_CHECK(hipMemcpyAsync(x.p, hx.data(), hx.size() * sizeof(cplx), hipMemcpyHostToDevice, st));
        OpDev A;
        const cplx *pcp = h->one_dev.p;
        int64_t bytes = 2;
        if (which == 0) {
            std::vector<zc> pc;
            plane_coeffs(h, coeffs, WAE_OP_N, pc);
            std::vector<cplx> tab(h->nplanes);
            slot_coeffs(h, h->slot_plane[level], pc, tab.data());
            pcd.upload(tab.data(), tab.size(), st);
            pcp = pcd.p;
            A = h->ops[level].dev(WAE_OP_N);
            bytes = 0;
            for (size_t g = 0; g < h->ops[level].groups.size(); ++g) {
                const GroupHost &G = h->ops[level].groups[g];
                for (int q = 0; q < G.nplanes; ++q)
                    if (tab[G.plane0 + q].x != 0.0 || tab[G.plane0 + q].y != 0.0) bytes += G.nnz * 20 + (n_out + 1) * 4;
            }
        } else {
            A = h->xfer[level].devR();
            bytes = (int64_t)h->xfer[level].r_col.n * 12 + (n_out + 1) * 4;       // real values: 8 + 4 bytes per entry
        }
        bytes += (int64_t)r * (n_in + n_out) * 16;
        if (which == 2) bytes += (int64_t)r * n_out * 16;          // (the prolongation updates the fine vector in place: read + write)
        if (bytes_out) *bytes_out = bytes;
        const Transfer *xf = which == 0 ? nullptr : &h->xfer[level];
        const bool by_tile = xf && xf->ft.ready && r >= 8 && xfer_tiles_on();
        auto one = [&]() {
            if (which == 2) {
                if (by_tile) launch_prolong_tiles(xf->ft.dev, x.p, y.p, y.p, r, st);
                else launch_prolong_add(xf->p_ptr.p, xf->p_col.p, xf->p_val.p, xf->nf, x.p, y.p, y.p, r, st, nullptr);
            } else launch_spmv(A, pcp, 1 << 30, x.p, y.p, nullptr, 0.0, r, MODE_AX, st);
        };
        if (which == 2) HIP_CHECK(hipMemsetAsync(y.p, 0, (size_t)n_out * r * sizeof(cplx), st));
        *ms_out = mean_ms(st, reps, one);
        return WAE_OK;
    });
}

int wae_bench_triad(int32_t device, int64_t n, int32_t reps, double *gbs_out) {
    return guarded([&]() {
        WAE_REQUIRE(n > 0 && reps > 0 && gbs_out, "bad argument");
        HIP_CHECK(hipSetDevice(device));
        DevBuf<double> a, b, c;
        a.alloc(n); b.alloc(n); c.alloc(n);
        HIP_CHECK(hipMemset(b.p, 0, n * sizeof(double)));
        HIP_CHECK(hipMemset(c.p, 0, n * sizeof(double)));
        hipStream_t st;
        HIP_CHECK(hipStreamCreate(&st));
        // The rate depends on the shape of the launch (measured, round 4: 4.6 ... 5.7 TB/s between 256 and 65 536 workgroups on one
        // box; the 8 192 this probe used until then sits at the low end): the best of five grid sizes is what the device attains.
        hipEvent_t e0, e1;
        HIP_CHECK(hipEventCreate(&e0));
        HIP_CHECK(hipEventCreate(&e1));
        double best = 0.0;
        for (unsigned cap : {512u, 1024u, 4096u, 8192u, 65536u}) {
            for (int i = 0; i < 2; ++i) launch_triad(a.p, b.p, c.p, 1.5, n, st, cap);
            HIP_CHECK(hipEventRecord(e0, st));
            for (int i = 0; i < reps; ++i) launch_triad(a.p, b.p, c.p, 1.5, n, st, cap);
            HIP_CHECK(hipEventRecord(e1, st));
            HIP_CHECK(hipEventSynchronize(e1));
            float ms = 0.f;
            HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
            best = std::max(best, 3.0 * n * sizeof(double) * reps / (ms * 1e-3) / 1e9);
        }
        *gbs_out = best;
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
        (void)hipStreamDestroy(st);
        return WAE_OK;
    });
}

}   // extern "C"
