// libwaehip.so -- the contour pass: the snapshot basis for projected initial guesses (rb_*), the one Beyn pass behind wae_beyn_moments and
// every mode of wae_beyn_moments_rb, wae_rb_export / wae_rb_import.  Host code only (kernels: vec.hip); the solves go through solver.h.
#include <cmath>

#include "solver.h"

// ----------------------------------------------------------------------------------------------------
// snapshot basis for projected initial guesses (wae_beyn_moments_rb)
// ----------------------------------------------------------------------------------------------------
// Gaussian elimination with partial pivoting on a small dense complex system (column-major n x n), in place.
// Unknowns whose pivot vanishes are set to zero (a deficient direction of the snapshot basis).
static void small_solve(std::vector<zc> &A, std::vector<zc> &b, int n) {
    std::vector<char> dead(n, 0);
    double amax = 0.0;
    for (const zc &a : A) amax = std::max(amax, std::abs(a));
    for (int k = 0; k < n; ++k) {
        int p = k;
        double best = 0.0;
        for (int i = k; i < n; ++i) { const double v = std::abs(A[(size_t)k * n + i]); if (v > best) { best = v; p = i; } }
        if (!(best > 1e-14 * amax)) { dead[k] = 1; continue; }
        if (p != k) {
            for (int j = 0; j < n; ++j) std::swap(A[(size_t)j * n + k], A[(size_t)j * n + p]);
            std::swap(b[k], b[p]);
        }
        const zc inv = 1.0 / A[(size_t)k * n + k];
        for (int i = k + 1; i < n; ++i) {
            const zc f = A[(size_t)k * n + i] * inv;
            if (f == zc(0)) continue;
            for (int j = k + 1; j < n; ++j) A[(size_t)j * n + i] -= f * A[(size_t)j * n + k];
            b[i] -= f * b[k];
        }
    }
    for (int k = n - 1; k >= 0; --k) {
        if (dead[k]) { b[k] = 0; continue; }
        zc sres = b[k];
        for (int j = k + 1; j < n; ++j) sres -= A[(size_t)j * n + k] * b[j];
        b[k] = sres / A[(size_t)k * n + k];
    }
}

static void rb_d2h(wae_family *h, const cplx *src, cplx *dst, size_t cnt) {
    HIP_CHECK(hipMemcpyAsync(dst, src, cnt * sizeof(cplx), hipMemcpyDeviceToHost, h->stream));
    HIP_CHECK(hipStreamSynchronize(h->stream));
}

// start an empty basis on the store Q (cap snapshots of d x l); kact = terms with a non-zero coefficient in `table`
static void rb_reset(wae_family *h, cplx *Q, int cap, int l, const double *table, int npts, const cplx *Vinter) {
    RbState &R = h->rb;
    const int T = h->T;
    R.Q = Q; R.cap = cap; R.l = l; R.S = 0;
    R.kact.clear();
    for (int k = 0; k < T; ++k) {
        bool used = false;
        for (int p = 0; p < npts && !used; ++p) used = table[((size_t)p * T + k) * 2] != 0.0 || table[((size_t)p * T + k) * 2 + 1] != 0.0;
        if (used) R.kact.push_back(k);
    }
    const size_t vecl = (size_t)h->d * l;
    R.wait_w();
    if (R.W.n < R.kact.size() * (size_t)cap * vecl) {
        const size_t need = R.kact.size() * (size_t)cap * vecl;
        const int dev = h->device;
        RbState *Rp = &R;
        R.w_job = std::async(std::launch::async, [Rp, need, dev]() {
            HIP_CHECK(hipSetDevice(dev));
            Rp->W.alloc(need);
        });
    }
    R.Hk.assign(R.kact.size() * (size_t)cap * cap * l, zc(0));
    R.g.assign((size_t)cap * l, zc(0));
    R.Vi.reserve(vecl);
    HIP_CHECK(hipMemcpyAsync(R.Vi.p, Vinter, vecl * sizeof(cplx), hipMemcpyDeviceToDevice, h->stream));
    R.vi_valid = true;
    R.hb.reserve((size_t)4 * (cap + 4) * l); R.alpha.reserve(l); R.alpha2.reserve((size_t)cap * l);
}

// the store slots S .. S+count-1 hold new raw vectors: orthonormalise them per column against the basis (classical
// Gram-Schmidt, two passes), then extend  g = Q^H V  and every projected term  H_k = Q^H A_k Q  by the new rows/columns.
// W_k = A_k Q stays resident (HBM is plentiful: C2 6.5 GB, C3 16 GB), so a new row costs dot products only.  The new
// vectors are handled four at a time (dots_multi reads the basis once per block): the build is a tall-skinny Gram product.
static void rb_append_block(wae_family *h, int cnt, const std::vector<std::vector<std::vector<zc>>> &pck) {
    RbState &R = h->rb;
    hipStream_t st = h->stream;
    const int64_t d = h->d;
    const int l = R.l, cap = R.cap, S = R.S;
    const size_t vecl = (size_t)d * l;
    std::vector<cplx> hh((size_t)(S + cnt) * cnt * l), n0((size_t)cnt * l), n1(l);
    const OpDev A0 = h->ops[0].dev(WAE_OP_N);
    cplx *qn = R.Q + (size_t)S * vecl;                       // the block of new vectors
    for (int j = 0; j < cnt; ++j) launch_norms(qn + (size_t)j * vecl, d, l, h->partial.p, R.hb.p + (size_t)j * l, st);
    rb_d2h(h, R.hb.p, n0.data(), (size_t)cnt * l);
    // (1) against the existing basis: block classical Gram-Schmidt, two passes
    // (the update of all new vectors in one reading of the basis, with the coefficients where dots_multi left them: no round trip
    // through the host; the basis used to be read once per new vector and pass -- 96 ms of a 1M-DoF pass)
    static const bool multi_axpy = !(getenv("WAE_RB_MULTI_AXPY") && atoi(getenv("WAE_RB_MULTI_AXPY")) == 0);
    const bool fits = (size_t)S * cnt * l * sizeof(cplx) <= 60 * 1024;
    for (int pass = 0; pass < 2 && S > 0; ++pass) {
        launch_dots_multi(R.Q, vecl, S, qn, vecl, cnt, d, l, h->partial.p, R.hb.p, st);       // hb[(i*cnt + j)*l + c]
        if (multi_axpy && fits) {
            launch_axpy_neg_multi(R.Q, vecl, S, R.hb.p, qn, vecl, cnt, d, l, st);
            continue;
        }
        rb_d2h(h, R.hb.p, hh.data(), (size_t)S * cnt * l);
        std::vector<cplx> cj((size_t)S * l);
        for (int j = 0; j < cnt; ++j) {
            for (int i = 0; i < S; ++i)
                for (int c = 0; c < l; ++c) cj[(size_t)i * l + c] = hh[((size_t)i * cnt + j) * l + c];
            R.alpha2.upload(cj.data(), cj.size(), st);
            launch_axpy_neg(R.Q, vecl, S, R.alpha2.p, qn + (size_t)j * vecl, d, l, st);
            HIP_CHECK(hipStreamSynchronize(st));             // cj is re-filled for the next vector
        }
    }
    // (2) inside the block, vector by vector; normalise (a vector that adds nothing to a column's span is zeroed there)
    for (int j = 0; j < cnt; ++j) {
        cplx *q = qn + (size_t)j * vecl;
        for (int pass = 0; pass < 2 && j > 0; ++pass) {
            launch_dots(qn, vecl, j, q, d, l, h->partial.p, R.hb.p, st);
            launch_axpy_neg(qn, vecl, j, R.hb.p, q, d, l, st);
        }
        launch_norms(q, d, l, h->partial.p, R.hb.p, st);
        rb_d2h(h, R.hb.p, n1.data(), l);
        for (int c = 0; c < l; ++c) {
            const double nrm0 = n0[(size_t)j * l + c].x;
            n1[c] = (n1[c].x > 1e-9 * nrm0 && nrm0 > 0.0) ? cplx{n1[c].x, 0.0} : cplx{0.0, 0.0};
        }
        R.alpha.upload(n1.data(), l, st);
        launch_scale_inv(q, R.alpha.p, q, d, l, st);
        HIP_CHECK(hipStreamSynchronize(st));
    }
    // (3) g = Q^H V for the new vectors
    launch_dots_multi(qn, vecl, cnt, R.Vi.p, vecl, 1, d, l, h->partial.p, R.hb.p, st);
    rb_d2h(h, R.hb.p, hh.data(), (size_t)cnt * l);
    for (int j = 0; j < cnt; ++j)
        for (int c = 0; c < l; ++c) R.g[(size_t)(S + j) * l + c] = zc(hh[(size_t)j * l + c].x, hh[(size_t)j * l + c].y);
    // (4) projected terms: new columns (all rows) and new rows (old columns)
    for (size_t ki = 0; ki < R.kact.size(); ++ki) {
        R.wait_w();
        cplx *Wk = R.W.p + ki * (size_t)cap * vecl;
        cplx *wn = Wk + (size_t)S * vecl;
        upload_pc(h, pck[ki]);
        for (int j = 0; j < cnt; ++j)
            launch_spmv(A0, pc_level(h, 0), l, qn + (size_t)j * vecl, wn + (size_t)j * vecl, nullptr, 0.0, l, MODE_AX, st);
        zc *H = &R.Hk[ki * (size_t)cap * cap * l];
        launch_dots_multi(R.Q, vecl, S + cnt, wn, vecl, cnt, d, l, h->partial.p, R.hb.p, st);  // q_i^H A_k q_{S+j}, i < S+cnt
        rb_d2h(h, R.hb.p, hh.data(), (size_t)(S + cnt) * cnt * l);
        for (int i = 0; i < S + cnt; ++i)
            for (int j = 0; j < cnt; ++j)
                for (int c = 0; c < l; ++c) {
                    const cplx v = hh[((size_t)i * cnt + j) * l + c];
                    H[((size_t)(S + j) * cap + i) * l + c] = zc(v.x, v.y);
                }
        // new rows (old columns).  A term A_k = s B with B real and symmetric (K, M of a Helmholtz family) projects to s x (a Hermitian
        // matrix): the new rows follow from the new columns, H[S+j, i] = (s / conj s) conj(H[i, S+j]), without reading A_k Q again.
        zc herm_factor(0);
        bool herm = false;
        {
            static const bool herm_on = !(getenv("WAE_RB_HERMITIAN") && atoi(getenv("WAE_RB_HERMITIAN")) == 0);
            const int kterm = R.kact[ki], pl = h->term_plane[kterm];
            const LevelOp &L0 = h->ops[0];
            for (size_t g = 0; g < L0.groups.size() && herm_on && !herm; ++g)
                for (int q = 0; q < L0.groups[g].nplanes; ++q)
                    if (h->slot_plane[0][(size_t)L0.groups[g].plane0 + q] == pl && L0.groups[g].symmetric && L0.groups[g].is_real) {
                        const zc sc = h->term_scale[kterm];
                        if (sc != zc(0)) { herm = true; herm_factor = sc / std::conj(sc); }
                    }
        }
        if (S > 0 && herm) {
            for (int i = 0; i < S; ++i)
                for (int j = 0; j < cnt; ++j)
                    for (int c = 0; c < l; ++c)
                        H[((size_t)i * cap + S + j) * l + c] = herm_factor * std::conj(H[((size_t)(S + j) * cap + i) * l + c]);
        } else if (S > 0) {
            launch_dots_multi(Wk, vecl, S, qn, vecl, cnt, d, l, h->partial.p, R.hb.p, st);     // (A_k q_i)^H q_{S+j} = conj(row S+j), i < S
            rb_d2h(h, R.hb.p, hh.data(), (size_t)S * cnt * l);
            for (int i = 0; i < S; ++i)
                for (int j = 0; j < cnt; ++j)
                    for (int c = 0; c < l; ++c) {
                        const cplx v = hh[((size_t)i * cnt + j) * l + c];
                        H[((size_t)i * cap + S + j) * l + c] = zc(v.x, -v.y);
                    }
        }
    }
    R.S += cnt;
}

static void rb_append(wae_family *h, int count) {
    RbState &R = h->rb;
    WAE_REQUIRE(R.S + count <= R.cap, "snapshot store is full");
    std::vector<std::vector<std::vector<zc>>> pck(R.kact.size());
    for (size_t ki = 0; ki < R.kact.size(); ++ki) {
        std::vector<double> ek((size_t)2 * h->T, 0.0);
        ek[(size_t)2 * R.kact[ki]] = 1.0;
        pck[ki].resize(1);
        plane_coeffs(h, ek.data(), WAE_OP_N, pck[ki][0]);
    }
    for (int done = 0; done < count; done += 4) rb_append_block(h, std::min(4, count - done), pck);
}

// Galerkin guesses of one chunk, Xs[row][sy*l + c] = Q_c (sum_k c_k(z_sy) Q_c^H A_k Q_c)^{-1} Q_c^H v_c, in two steps: the
// S x S solves (host only, reads the projected terms -- safe to run on a helper thread while the device works on the
// previous chunk), and the application of the coefficients on the device.
static std::vector<cplx> rb_guess_coeffs(const wae_family *h, const double *ct_chunk, int ns) {
    const RbState &R = h->rb;
    const int S = R.S, l = R.l, cap = R.cap, T = h->T, nb = ns * l;
    std::vector<cplx> Y((size_t)S * nb);
    std::vector<zc> Hs((size_t)S * S), rhs(S);
    for (int sy = 0; sy < ns; ++sy) {
        const double *ct = ct_chunk + (size_t)sy * 2 * T;
        for (int k = 0; k < T; ++k)
            if ((ct[2 * k] != 0.0 || ct[2 * k + 1] != 0.0) && std::find(R.kact.begin(), R.kact.end(), k) == R.kact.end())
                throw WaeError(WAE_ERR_INVALID, "a term outside the projected set has a non-zero coefficient: rebuild the basis (mode 1)");
        for (int c = 0; c < l; ++c) {
            std::fill(Hs.begin(), Hs.end(), zc(0));
            for (size_t ki = 0; ki < R.kact.size(); ++ki) {
                const zc ck(ct[2 * R.kact[ki]], ct[2 * R.kact[ki] + 1]);
                if (ck == zc(0)) continue;
                const zc *H = &R.Hk[ki * (size_t)cap * cap * l];
                for (int sc = 0; sc < S; ++sc)
                    for (int i = 0; i < S; ++i) Hs[(size_t)sc * S + i] += ck * H[((size_t)sc * cap + i) * l + c];
            }
            for (int i = 0; i < S; ++i) rhs[i] = R.g[(size_t)i * l + c];
            small_solve(Hs, rhs, S);
            for (int i = 0; i < S; ++i) {
                const zc yv = std::isfinite(rhs[i].real()) && std::isfinite(rhs[i].imag()) ? rhs[i] : zc(0);
                Y[(size_t)i * nb + (size_t)sy * l + c] = cplx{yv.real(), yv.imag()};
            }
        }
    }
    return Y;
}
static void rb_apply_guess(wae_family *h, const std::vector<cplx> &Y, int ns, cplx *X) {
    RbState &R = h->rb;
    const int S = (int)(Y.size() / ((size_t)ns * R.l));
    R.ycoef.upload(Y.data(), Y.size(), h->stream);
    launch_lincomb_rep(R.Q, (size_t)h->d * R.l, S, R.ycoef.p, X, h->d, ns * R.l, R.l, h->stream);
    HIP_CHECK(hipStreamSynchronize(h->stream));
}

// What one call of the contour pass does, and on what.  wae_beyn_moments and every mode of wae_beyn_moments_rb are values of
// this struct (beyn_pass_for_mode); beyn_pass_core tests its fields, never a mode number.
struct BeynPass {
    enum Keep { nothing, into_basis, raw_to_store };
    bool new_basis = false;          // start an empty basis on the store (else a pass with guesses continues the handle's basis)
    int absorb = 0;                  // raw snapshots that already lie in the store and are orthonormalised into the new basis
    bool solve = true;               // false: return once the basis stands -- no system is solved, the moments are not touched
    bool guess = false;              // a chunk starts from the Galerkin projection on the basis, as soon as that holds a snapshot
    Keep keep = nothing;             // a chunk's solutions: dropped | appended to the basis | written raw into the slots slot0 + point
    int enrich_its = 1 << 30;        // keep == nothing: a chunk that took more iterations than this joins the basis all the same
    bool light_cycle = false;        // solves that start from a guess run the light form of vcycle()
    bool progressive = false;        // a chunk takes no more points than the basis holds snapshots (at first: 16 columns' worth)
    bool prefetch_coeffs = false;    // the basis is fixed: a helper thread computes the next chunk's guess coefficients
    // operands
    int npts = 0;
    const double *z = nullptr, *w = nullptr, *coeff_table = nullptr;
    const double *V = nullptr;       // d x l column-major on the host; nullptr: the probe matrix the handle's basis was started with
    int l = 0, l_total = 0, col0 = 0;   // V holds the columns col0 .. col0+l-1 of a moment tensor with l_total columns
    int K = 1, maxit = 0;
    double tol = 0.0;
    cplx *Q = nullptr;               // snapshot store of nbasis slots (nullptr: the store the handle owns); this call's slots start at slot0
    int nbasis = 0, slot0 = 0;
    double *A_out = nullptr;
    cplx *out_dev = nullptr;
    bool accumulate = false;         // add to the moments in out_dev instead of zeroing them first
};

// the public mode of wae_beyn_moments_rb (include/waehip.h) as a pass, with the argument checks that belong to the mode
static BeynPass beyn_pass_for_mode(int mode, bool have_V, int npts, int nbasis, int slot0) {
    WAE_REQUIRE(have_V || mode == 2, "bad argument");
    WAE_REQUIRE(mode >= 0 && mode <= 4, "mode must be 0 (take snapshots), 1 (rebuild the basis from the store, use it), 2 (use it), "
                                        "3 (solve from zero, store raw) or 4 (build the basis from the store, solve nothing)");
    WAE_REQUIRE(nbasis >= 0 && slot0 >= 0 && (mode == 2 || slot0 + ((mode == 0 || mode == 3) ? npts : 0) <= nbasis), "snapshot slots out of range");
    // adaptive enrichment is off by default: on the C2 contour the orthogonalisation and projection of the extra
    // vectors cost more than the iterations they saved (measured with thresholds 3, 6, 9); WAE_RB_ENRICH=<its> enables
    static const int enrich_its = getenv("WAE_RB_ENRICH") ? atoi(getenv("WAE_RB_ENRICH")) : (1 << 30);
    BeynPass p;
    switch (mode) {
    case 0:                          // progressive: later snapshot chunks start from the earlier ones
        p.new_basis = slot0 == 0; p.guess = true; p.keep = BeynPass::into_basis; p.progressive = true;
        break;
    case 1:                          // the store holds slot0 raw snapshots (e.g. gathered from other ranks)
        p.new_basis = true; p.absorb = slot0;
        [[fallthrough]];
    case 2:                          // the projected phase; enrichment would add to the basis where the guesses were poor (a
                                     // region of the contour close to poles outside it) while the store has room
        p.guess = true; p.light_cycle = true; p.enrich_its = enrich_its; p.prefetch_coeffs = enrich_its >= (1 << 30);
        break;
    case 3:                          // raw solutions into the caller's slots; no basis work (another rank builds it)
        p.keep = BeynPass::raw_to_store;
        break;
    case 4:                          // (the coefficient table only says which terms take part)
        p.new_basis = true; p.absorb = slot0; p.solve = false;
        break;
    }
    return p;
}

// One chunk made ready: the plane coefficients of its ns points (returned), their weights and points on the device
// (zw_dev = [w | z]) and, when the chunk width changed, the lg probe columns from column cg on replicated into Bs.
static std::vector<std::vector<zc>> beyn_chunk_prepare(wae_family *h, const BeynPass &p, int p0, int ns, int cg, int lg, int &rep_nb) {
    hipStream_t st = h->stream;
    std::vector<std::vector<zc>> pcs(ns);
    std::vector<cplx> zw(2 * ns);
    for (int s = 0; s < ns; ++s) {
        plane_coeffs(h, p.coeff_table + (size_t)(p0 + s) * 2 * h->T, WAE_OP_N, pcs[s]);
        zw[s] = cplx{p.w[2 * (p0 + s)], p.w[2 * (p0 + s) + 1]};
        zw[ns + s] = cplx{p.z[2 * (p0 + s)], p.z[2 * (p0 + s) + 1]};
    }
    h->zw_dev.upload(zw.data(), zw.size(), st);
    HIP_CHECK(hipStreamSynchronize(st));
    if (ns * lg != rep_nb) {         // same right-hand sides for every chunk
        launch_replicate(h->io_a.p + (size_t)cg * h->d, h->d, lg, h->Bs.p, ns * lg, st, h->perm());
        rep_nb = ns * lg;
    }
    return pcs;
}

static int beyn_pass_core(wae_family *h, const BeynPass &p, wae_solve_info *info) {
    require_solver(h);
    // a pass without a store takes any l (as the reference does, beyn.jl:39-57); a basis is one per call and spans one batch
    const bool store = p.new_basis || p.guess || p.keep != BeynPass::nothing;
    WAE_REQUIRE(!store || p.l <= h->NB, "l exceeds the solver batch width");
    HIP_CHECK(hipSetDevice(h->device));
    hipStream_t st = h->stream;
    CallInfo ci;
    const int64_t d = h->d;
    const int l = p.l, T = h->T, npts = p.npts, npow = 2 * p.K;
    const size_t acnt = (size_t)d * p.l_total * npow;        // the moment tensor has l_total columns; this call fills l of them
    const size_t vecl = (size_t)d * l;
    RbState &R = h->rb;                                      // (touched only where a field of the pass asks for the store or the basis)
    DevBuf<cplx> Aown;
    cplx *Ad = p.out_dev;
    if (!Ad) { Aown.alloc(acnt); Ad = Aown.p; }
    if (!p.accumulate) launch_fill_zero(Ad, acnt, st);
    cplx *Q = p.Q;
    if (store && !Q) {                           // library-owned snapshot store (single-process use)
        if (p.new_basis && p.keep == BeynPass::into_basis) h->rbQ.reserve(vecl * (size_t)p.nbasis);
        WAE_REQUIRE(h->rbQ.n >= vecl * (size_t)p.nbasis, "no snapshots stored in the handle: run mode 0 first");
        Q = h->rbQ.p;
    }
    h->io_a.reserve(vecl);
    if (p.V) {
        HIP_CHECK(hipMemcpyAsync(h->io_a.p, p.V, vecl * sizeof(cplx), hipMemcpyHostToDevice, st));
    } else {                                     // the probe matrix of the basis this handle started is still in HBM
        WAE_REQUIRE(R.vi_valid && R.l == l && R.Vi.n >= vecl, "V may be NULL only in mode 2 after a mode 0/1 call with the same l on this handle");
        launch_inter_to_colmajor(R.Vi.p, l, d, l, h->io_a.p, st, h->perm());      // (io_a holds the caller's numbering, like an uploaded V)
    }
    if (p.guess) R.ycoef.reserve((size_t)std::max(p.nbasis, 1) * h->NB);
    if (p.new_basis) {
        launch_colmajor_to_inter(h->io_a.p, d, l, h->W.p, l, st, h->perm());
        rb_reset(h, Q, p.nbasis, l, p.coeff_table, npts, h->W.p);
        if (p.absorb > 0) rb_append(h, p.absorb);
    } else if (p.guess) {
        WAE_REQUIRE(R.Q == Q && R.l == l && R.cap == p.nbasis, "the basis in the handle belongs to another store / shape");
        WAE_REQUIRE(p.keep != BeynPass::into_basis || p.slot0 == R.S, "mode 0 appends: slot0 must equal the number of snapshots taken so far");
        WAE_REQUIRE(p.keep == BeynPass::into_basis || R.S > 0, "mode 2 needs a basis: run mode 0 (or 1) first");
    }
    if (!p.solve) {
        HIP_CHECK(hipStreamSynchronize(st));
        ci.li.levels = (int)h->ops.size();
        return ci.finish(info);
    }

    static const bool rbdbg = getenv("WAE_GMRES_DEBUG") && atoi(getenv("WAE_GMRES_DEBUG"));
    double t_guess = 0.0, t_solve = 0.0, t_append = 0.0;
    // A progressive pass should start with small chunks: a chunk never takes more points than the basis already
    // holds, starting with 16 columns' worth (1, 1, 2, 4, 4, ... points for l = 16; 16, 16, 32 for l = 1).  Measured on
    // the snapshot phase: C2 0.695 -> 0.668 s, C3 2.71 -> 2.56 s; one rank's share of C3 when the probe columns are split
    // over 8 / 4 / 2 GPUs (1 / 2 / 4 columns x 64 points): 0.97 -> 0.63, 1.19 -> 0.97, 1.79 -> 1.69 s (dev/c3_rank_share.py).
    // (Starting widths of 4, 8 and 32 columns measured: slower.)
    struct LightOff { bool &on; ~LightOff() { on = false; } } light_off{h->vc_light};      // set before every solve; off again however the loop ends
    for (int cg = 0; cg < l; cg += h->NB) {      // probe columns in groups of <= NB (one group whenever there is a store)
        const int lg = std::min(h->NB, l - cg);
        const int spc = std::max(1, h->NB / lg);   // systems per chunk
        const int c0 = std::max(1, 16 / lg);       // points of a progressive pass's first chunk
        h->zw_dev.reserve((size_t)2 * spc);
        std::future<std::vector<cplx>> next_Y;
        auto launch_coeffs = [&](int q0) {
            const int nq = std::min(spc, npts - q0);
            const double *ct = p.coeff_table + (size_t)q0 * 2 * T;
            return std::async(std::launch::async, [h, ct, nq]() { return rb_guess_coeffs(h, ct, nq); });
        };
        if (p.prefetch_coeffs && npts > 0 && R.S > 0) next_Y = launch_coeffs(0);
        int rep_nb = -1;
        for (int p0 = 0, ns; p0 < npts; p0 += ns) {
            ns = std::min(spc, npts - p0);
            if (p.progressive) ns = std::min(ns, std::max(c0, R.S));
            const Batch bt{ns * lg, lg, ns, WAE_OP_N};
            const auto pcs = beyn_chunk_prepare(h, p, p0, ns, cg, lg, rep_nb);
            const bool guess = p.guess && R.S > 0;
            const double ta = now_s();
            if (guess) {
                std::vector<cplx> Y;
                if (next_Y.valid()) {
                    Y = next_Y.get();
                    if (p0 + spc < npts) next_Y = launch_coeffs(p0 + spc);
                } else {
                    Y = rb_guess_coeffs(h, p.coeff_table + (size_t)p0 * 2 * T, ns);
                }
                rb_apply_guess(h, Y, ns, h->Xs.p);
            }
            const double tb = now_s();
            h->vc_light = guess && p.light_cycle;
            const int its = solve_chunk(h, bt, pcs, h->Bs.p, h->Xs.p, p.tol, p.maxit, &ci.li, nullptr, guess);
            launch_beyn_accum(h->Xs.p, bt.nb, d, lg, ns, h->zw_dev.p, h->zw_dev.p + ns, npow, Ad, st, p.l_total, p.col0 + cg, h->perm());
            if (rbdbg) HIP_CHECK(hipStreamSynchronize(st));
            const double tc = now_s();
            if (p.keep == BeynPass::raw_to_store) {
                for (int s = 0; s < ns; ++s)
                    launch_extract_cols(h->Xs.p, bt.nb, s * l, l, Q + (size_t)(p.slot0 + p0 + s) * vecl, d, st);
            } else if (p.keep == BeynPass::into_basis || (its > p.enrich_its && R.S + ns <= R.cap)) {
                for (int s = 0; s < ns; ++s)
                    launch_extract_cols(h->Xs.p, bt.nb, s * l, l, Q + (size_t)(R.S + s) * vecl, d, st);
                rb_append(h, ns);
            }
            if (rbdbg) {
                HIP_CHECK(hipStreamSynchronize(st));
                t_guess += tb - ta; t_solve += tc - tb; t_append += now_s() - tc;
            }
        }
    }
    if (rbdbg && store) fprintf(stderr, "[rb] keep=%d S=%d guess %.3f s  solve %.3f s  append %.3f s\n", (int)p.keep, R.S, t_guess, t_solve, t_append);
    if (p.A_out) HIP_CHECK(hipMemcpyAsync(p.A_out, Ad, acnt * sizeof(cplx), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    return ci.finish(info);
}

extern "C" {

int wae_beyn_moments(wae_family *h, int32_t npts, const double *z, const double *w, const double *coeff_table, const double *V, int32_t l, int32_t K,
                     double tol, int32_t maxit, double *A_out, uint64_t out_dev, wae_solve_info *info) {
    return guarded([&]() {
        WAE_REQUIRE(h && npts >= 0 && (npts == 0 || (z && w && coeff_table)) && V && l > 0 && K > 0, "bad argument");
        WAE_REQUIRE(A_out || out_dev, "no output buffer");
        BeynPass p;                  // every system from zero and nothing kept: no store, and the handle's basis is left alone
        p.npts = npts; p.z = z; p.w = w; p.coeff_table = coeff_table; p.V = V; p.l = p.l_total = l; p.K = K; p.tol = tol; p.maxit = maxit;
        p.A_out = A_out; p.out_dev = (cplx *)(uintptr_t)out_dev;
        return beyn_pass_core(h, p, info);
    });
}

int wae_beyn_moments_rb(wae_family *h, int32_t npts, const double *z, const double *w, const double *coeff_table, const double *V, int32_t l, int32_t K,
                        double tol, int32_t maxit, int32_t mode, int32_t nbasis, int32_t slot0, uint64_t Q_dev, double *A_out, uint64_t out_dev,
                        int32_t accumulate, int32_t l_total, int32_t col0, wae_solve_info *info) {
    return guarded([&]() {
        WAE_REQUIRE(h && npts >= 0 && (npts == 0 || (z && w && coeff_table)) && l > 0 && K > 0, "bad argument");
        WAE_REQUIRE(A_out || out_dev, "no output buffer");
        BeynPass p = beyn_pass_for_mode(mode, V != nullptr, npts, nbasis, slot0);
        WAE_REQUIRE(!accumulate || out_dev, "accumulate needs a device-resident moment buffer");
        if (l_total <= 0) { l_total = l; col0 = 0; }
        WAE_REQUIRE(col0 >= 0 && col0 + l <= l_total, "column slice out of range");
        p.npts = npts; p.z = z; p.w = w; p.coeff_table = coeff_table; p.V = V; p.l = l; p.l_total = l_total; p.col0 = col0; p.K = K; p.tol = tol;
        p.maxit = maxit; p.Q = (cplx *)(uintptr_t)Q_dev; p.nbasis = nbasis; p.slot0 = slot0;
        p.A_out = A_out; p.out_dev = (cplx *)(uintptr_t)out_dev; p.accumulate = accumulate != 0;
        return beyn_pass_core(h, p, info);
    });
}

int wae_rb_export(wae_family *h, int32_t *S_out, int32_t *l_out, int32_t *nk_out, int32_t *kact_out, double *Hk_out, double *g_out) {
    return guarded([&]() {
        WAE_REQUIRE(h && S_out && l_out && nk_out, "bad argument");
        const RbState &R = h->rb;
        *S_out = R.S; *l_out = R.l; *nk_out = (int32_t)R.kact.size();
        if (kact_out) for (size_t i = 0; i < R.kact.size(); ++i) kact_out[i] = R.kact[i];
        const int S = R.S, l = R.l, cap = R.cap;
        if (Hk_out)                                              // dense [ki][s][i][c], c fastest
            for (size_t ki = 0; ki < R.kact.size(); ++ki)
                for (int s = 0; s < S; ++s)
                    for (int i = 0; i < S; ++i)
                        for (int c = 0; c < l; ++c) {
                            const zc v = R.Hk[ki * (size_t)cap * cap * l + ((size_t)s * cap + i) * l + c];
                            const size_t o = (((ki * S + s) * (size_t)S + i) * l + c) * 2;
                            Hk_out[o] = v.real(); Hk_out[o + 1] = v.imag();
                        }
        if (g_out)
            for (int i = 0; i < S; ++i)
                for (int c = 0; c < l; ++c) { g_out[((size_t)i * l + c) * 2] = R.g[(size_t)i * l + c].real(); g_out[((size_t)i * l + c) * 2 + 1] = R.g[(size_t)i * l + c].imag(); }
        return WAE_OK;
    });
}

int wae_rb_import(wae_family *h, int32_t S, int32_t l, uint64_t Q_dev, int32_t nk, const int32_t *kact, const double *Hk, const double *g) {
    return guarded([&]() {
        WAE_REQUIRE(h && S > 0 && l > 0 && Q_dev && nk >= 0 && (nk == 0 || kact) && Hk && g, "bad argument");
        RbState &R = h->rb;
        R.Q = (cplx *)(uintptr_t)Q_dev; R.cap = S; R.l = l; R.S = S;
        R.vi_valid = false;
        R.kact.assign(kact, kact + nk);
        R.Hk.resize((size_t)nk * S * S * l);
        for (size_t i = 0; i < R.Hk.size(); ++i) R.Hk[i] = zc(Hk[2 * i], Hk[2 * i + 1]);     // cap == S: same dense layout
        R.g.resize((size_t)S * l);
        for (size_t i = 0; i < R.g.size(); ++i) R.g[i] = zc(g[2 * i], g[2 * i + 1]);
        return WAE_OK;
    });
}

}   // extern "C"
