// libwaehip.so -- family handle, multigrid-preconditioned batched GMRES, Beyn moment loop, C ABI.
// gfx950 only.  See include/waehip.h for the contract of every exported function.
#include <cmath>

#include "family.h"

static thread_local std::string g_last_error;
void wae_set_error(const std::string &m) { g_last_error = m; }

int wae_internal_device(const wae_family *h) { return h->device; }
hipStream_t wae_internal_stream(const wae_family *h) { return h->stream; }

// ----------------------------------------------------------------------------------------------------
// coefficient tables
// ----------------------------------------------------------------------------------------------------
// upload [level][sys][slot] tables (plane_coeffs: family.h)
static void upload_pc(wae_family *h, const std::vector<std::vector<zc>> &pcs) {
    const int nsys = (int)pcs.size();
    const int nl = (int)h->ops.size();
    const size_t per_level = (size_t)nsys * h->nplanes;
    std::vector<cplx> tab(per_level * (nl + 2));
    for (int l = 0; l <= nl + 1; ++l) {                  // blocks nl, nl+1: the penalty block and the penalty rows (own slot orders)
        if (l >= nl && h->n_penalty == 0) break;
        const std::vector<int> &sp = l < nl ? h->slot_plane[l] : (l == nl ? h->pen_slot : h->pen_row_slot);
        for (int s = 0; s < nsys; ++s)
            for (int q = 0; q < h->nplanes; ++q) {
                const zc c = pcs[s][sp[q]];
                tab[l * per_level + (size_t)s * h->nplanes + q] = cplx{c.real(), c.imag()};
            }
    }
    h->pc_stride_level = per_level;
    h->pcdev.upload(tab.data(), tab.size(), h->stream);
    HIP_CHECK(hipStreamSynchronize(h->stream));
}
static inline const cplx *pc_level(const wae_family *h, int l) { return h->pcdev.p + (size_t)l * h->pc_stride_level; }

// ----------------------------------------------------------------------------------------------------
// multigrid V-cycle (all columns in lock-step)
// ----------------------------------------------------------------------------------------------------
static void dense_setup(wae_family *h, const Batch &bt) {
    const int L = (int)h->ops.size() - 1;
    if (h->nc <= 0) return;
    HIP_CHECK(hipMemsetAsync(h->dstatus.p, 0, sizeof(int), h->stream));
    launch_dense_assemble(h->dense_planes.p, h->nplanes, (int)h->nc, pc_level(h, L), bt.nsys, bt.op, h->Ainv.p, h->stream);
    launch_dense_invert(h->Ainv.p, (int)h->nc, bt.nsys, h->dstatus.p, h->stream);
    int st = 0;
    HIP_CHECK(hipMemcpyAsync(&st, h->dstatus.p, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIP_CHECK(hipStreamSynchronize(h->stream));
    if (st) throw WaeError(WAE_ERR_BREAKDOWN, "coarse operator is singular");
}

// weight of the PRE-smoothing sweeps: the set-up's (opts[2]) -- or, in the light cycle of the projected phase, WAE_JAC_LIGHT (experiments)
static double pre_weight(const wae_family *h) {
    static const double w_light = getenv("WAE_JAC_LIGHT") ? atof(getenv("WAE_JAC_LIGHT")) : 0.0;
    return h->vc_light ? (w_light > 0.0 ? w_light : h->jac_w_light) : h->jac_w;
}
// x = Minv b on level l;  returns pointer to the result (either lx[l] or lt[l])
// have_x0: the first sweep of level l (x = w/diag b) is already in lx[l] (written by the SpMV that produced b, MODE_AX_J0)
// final_out (level 0 only): the last post-smoothing sweep -- or, in a cycle without one, the prolongation -- writes its result there (a
// Krylov basis slot) instead of into lx/lt; masked chunks of final_out are left as they were
// cn (level 0 only): the caller wants the column norms of the result in cn->out.  A cycle that ends in its prolongation (the light
// cycle) takes them from that kernel and sets cn->done -- with cn->only it then writes no result at all; any other cycle leaves
// cn->done false and the caller runs its own pass over the result.
struct CycleNorms { cplx *out; bool only; bool done = false; };
static cplx *vcycle(wae_family *h, const Batch &bt, int l, const cplx *b, const unsigned char *cm = nullptr, bool have_x0 = false,
                    cplx *final_out = nullptr, CycleNorms *cn = nullptr) {
    const int L = (int)h->ops.size() - 1;
    hipStream_t st = h->stream;
    if (l == L) {
        launch_dense_apply(h->Ainv.p, (int)h->nc, bt.cps, b, h->lx[l].p, bt.nb, st, cm);
        return h->lx[l].p;
    }
    const OpDev A = h->ops[l].dev(bt.op);
    const cplx *pc = pc_level(h, l);
    cplx *x = h->lx[l].p, *t = h->lt[l].p;
    if (!have_x0) launch_jacobi0(A, pc, bt.cps, b, x, pre_weight(h), bt.nb, st, cm);
    for (int s = 1; s < h->nsweeps; ++s) {
        launch_spmv(A, pc, bt.cps, x, t, b, pre_weight(h), bt.nb, MODE_JAC, st, cm);
        std::swap(x, t);
    }
    // (experiment) WAE_VC_LIGHT_ADD=1: the light cycle additive -- the coarse correction is computed from b itself, not from the residual
    // after the first sweep: no second fine-level product per cycle
    static const int light_add = getenv("WAE_VC_LIGHT_ADD") ? atoi(getenv("WAE_VC_LIGHT_ADD")) : 0;
    // residual -> t, restrict -> lb[l+1]
    const bool additive = h->vc_light && light_add && l == 0 && h->nsweeps == 1;
    if (!additive) launch_spmv(A, pc, bt.cps, x, t, b, 0.0, bt.nb, MODE_RES, st, cm);
    // for op = T/C the transfer operators are unchanged (real): (R A P)^H = R A^H P
    const bool by_tile = h->xfer[l].ft.ready && bt.nb >= 8 && xfer_tiles_on();      // (wae_internal.h XferTiles: level 0, wide batches)
    launch_spmv(h->xfer[l].devR(), h->one_dev.p, 1 << 30, additive ? b : t, h->lb[l + 1].p, nullptr, 0.0, bt.nb, MODE_AX, st, cm);
    const cplx *xc = vcycle(h, bt, l + 1, h->lb[l + 1].p, cm);
    // Post-smoothing on the coarse levels (WAE_VC_POST_COARSE): 1 always, 0 never, 2 (default) everywhere but in the projected phase of
    // a contour integral.  A solve that starts from a projected guess (216 of the 256 points of the benchmark contour) takes 1-5 steps:
    // there a cheaper cycle beats a better one (measured at 1M unknowns: projected phase 1.17 -> 0.99 s without the coarse
    // post-smoothing, while the from-zero solves of the snapshot phase lose 1.26 -> 1.63 s).
    static const int post_coarse = getenv("WAE_VC_POST_COARSE") ? atoi(getenv("WAE_VC_POST_COARSE")) : 2;
    // ... and the fine level's too (WAE_VC_LIGHT_POST0=1 keeps it): the light cycle is V(1,0) on every level -- projected phase 1.02 -> 0.89 s,
    // same eigenpairs (residuals 5.6e-9 -> 6.4e-9, rank gap 1.2e9), 9 325 -> 9 139 column-iterations per pass.
    static const int light_post0 = getenv("WAE_VC_LIGHT_POST0") ? atoi(getenv("WAE_VC_LIGHT_POST0")) : 0;
    const bool no_post = l >= 1 ? (post_coarse == 0 || (post_coarse == 2 && h->vc_light)) : (h->vc_light && !light_post0);
    const int npost = no_post ? 0 : h->nsweeps;
    // x + P xc: in place, or -- when no sweep follows -- straight into final_out, with the norms of the result if they are asked for
    const size_t npart = (size_t)(by_tile ? h->xfer[l].ft.dev.ntiles : PROLONG_NORM_BLOCKS) * bt.nb;
    // (not fused -- the caller then runs its own norms pass, cn->done stays false -- when the partial sums do not fit the reduction
    // scratch, when the level is empty (the launchers return at once), or when a caller wants no result AND a result in final_out)
    const bool norms = cn && l == 0 && npost == 0 && npart <= h->partial.n && h->ops[l].n > 0 && !(cn->only && final_out);
    cplx *const px = (norms && cn->only) ? nullptr : (final_out && npost == 0) ? final_out : x;
    cplx *const part = norms ? h->partial.p : nullptr, *const nout = norms ? cn->out : nullptr;
    if (by_tile) launch_prolong_tiles(h->xfer[l].ft.dev, xc, x, px, bt.nb, st, cm, part, nout);
    else launch_prolong_add(h->xfer[l].p_ptr.p, h->xfer[l].p_col.p, h->xfer[l].p_val.p, h->xfer[l].nf, xc, x, px, bt.nb, st, cm, part, nout);
    if (norms) cn->done = true;
    if (px) x = px;
    // (WAE_JAC_POST: a post-smoothing weight of its own -- two sweeps with different weights form a degree-2 polynomial smoother)
    static const double w_post_env = getenv("WAE_JAC_POST") ? atof(getenv("WAE_JAC_POST")) : 0.0;
    const double w_post = w_post_env > 0.0 ? w_post_env : h->jac_w_post;
    for (int s = 0; s < npost; ++s) {
        cplx *dst = (final_out && s == npost - 1) ? final_out : t;
        launch_spmv(A, pc, bt.cps, x, dst, b, w_post, bt.nb, MODE_JAC, st, cm);
        if (dst == t) std::swap(x, t); else x = dst;
    }
    // (for a cycle in which neither the last sweep nor the prolongation has written final_out; none is left today)
    if (final_out && x != final_out) { launch_copy(x, final_out, (size_t)h->ops[l].n * bt.nb, st); x = final_out; }
    return x;
}

// ----------------------------------------------------------------------------------------------------
// batched left-preconditioned GMRES(m)
// ----------------------------------------------------------------------------------------------------
struct ColState {
    std::vector<zc> H;      // (m+1) x m column-major upper part after rotations
    std::vector<zc> Hraw;   // the same columns before the rotations (pair steps of the narrow batches; empty otherwise)
    std::vector<zc> g;
    std::vector<double> cs;
    std::vector<zc> sn;
    std::vector<zc> cdef;   // deflation: c_j = u^H M^-1 A v_j, the component removed from every new Krylov vector
    int ld = 0;             // leading dimension of H and Hraw: m + 1
    int steps = 0;          // Arnoldi steps to use for the update
    bool conv = false;

    ColState(int m, bool keep_raw, double beta, bool done)
        : H((size_t)(m + 1) * m), Hraw(keep_raw ? (size_t)(m + 1) * m : 0), g(m + 1), cs(m), sn(m), cdef(m), ld(m + 1), conv(done) { g[0] = beta; }
    // the Givens rotations of a new column raw[0..jc+1]; false on a zero or NaN pivot (`nan` set), which ends the column
    bool rotate_in(int jc, const zc *raw, zc cdef_j, bool &nan) {
        zc *Hc = &H[(size_t)jc * ld];
        for (int i = 0; i <= jc + 1; ++i) Hc[i] = raw[i];
        if (!Hraw.empty()) std::copy(raw, raw + jc + 2, &Hraw[(size_t)jc * ld]);
        cdef[jc] = cdef_j;
        for (int i = 0; i < jc; ++i) {
            const zc a = Hc[i], bb = Hc[i + 1];
            Hc[i] = cs[i] * a + sn[i] * bb;
            Hc[i + 1] = -std::conj(sn[i]) * a + cs[i] * bb;
        }
        const zc a = Hc[jc];
        const double bb = Hc[jc + 1].real();
        const double aa = std::abs(a);
        const double t = std::sqrt(aa * aa + bb * bb);
        if (!(t > 0.0) || std::isnan(t)) { conv = true; if (std::isnan(t)) nan = true; return false; }
        if (aa == 0.0) { cs[jc] = 0.0; sn[jc] = 1.0; }
        else { cs[jc] = aa / t; sn[jc] = (a / aa) * (bb / t); }
        Hc[jc] = cs[jc] * a + sn[jc] * bb;
        Hc[jc + 1] = 0;
        g[jc + 1] = -std::conj(sn[jc]) * g[jc];
        g[jc] = cs[jc] * g[jc];
        steps = jc + 1;
        return true;
    }
    std::vector<zc> back_substitute() const {       // y = R^-1 g
        std::vector<zc> y(steps);
        for (int i = steps - 1; i >= 0; --i) {
            zc s = g[i];
            for (int q = i + 1; q < steps; ++q) s -= H[(size_t)q * ld + i] * y[q];
            const zc dgi = H[(size_t)i * ld + i];
            y[i] = (dgi != zc(0)) ? s / dgi : zc(0);
        }
        return y;
    }
};

// A solution that starts from a guess assembled out of other solutions (wae_beyn_moments_rb) is accurate in the norm of
// the stopping test but not componentwise on the penalty rows: their unknowns are ~1e-11 of the rest and are multiplied by
// 1e15 in the operator, so eigenvectors built from such solutions show a large residual exactly there.  (From a zero guess
// the ~30 V-cycle applications of the Krylov process resolve them as a by-product.)  This solves the penalty rows' own
// equations  A_bb d = (b - A x)_b  for the given interior values: the block is an admittance-scaled boundary mass matrix,
// for which point relaxation with weight 0.8 contracts by 0.6 per sweep (spectrum of D^-1 M_P1,2D in [1/2, 2]); the sweeps
// run on the compact n_b x n_b operator and cost microseconds.  Best effort: a block of another kind on which the
// relaxation does not contract is left as it was.
static void penalty_polish(wae_family *h, const Batch &bt, const cplx *B, cplx *X) {
    if (h->n_penalty <= 0) return;
    // Sweeps: 22 damped point relaxations whose weights are the reciprocals of the Chebyshev nodes of [0.4, 2.2] -- the interval that
    // holds the spectrum of D^-1 A_bb for a P1 boundary mass matrix ([1/2, 2]) with a margin -- taken in an order that keeps the partial
    // products bounded (round 4: the same 1e-9 as 40 sweeps with the fixed weight 0.8, whose contraction is 0.6 per sweep; 1.3 -> 0.7 ms
    // per chunk of the projected phase).  WAE_PEN_SWEEPS=<n> restores n fixed-weight sweeps (0: no polish).
    static const int sweeps_fixed = getenv("WAE_PEN_SWEEPS") ? atoi(getenv("WAE_PEN_SWEEPS")) : -1;
    if (sweeps_fixed == 0) return;
    static const std::vector<double> cheb = []() {
        const int n = 22;
        const double lo = 0.4, hi = 2.2, th = 0.5 * (hi + lo), de = 0.5 * (hi - lo);
        std::vector<double> w(n);
        for (int k = 0; k < n; ++k) w[k] = 1.0 / (th - de * std::cos((2 * k + 1) * M_PI / (2 * n)));
        std::vector<double> o;                                    // nodes from both ends inwards: large and small weights alternate
        for (int a = 0, b = n - 1; a <= b; ++a, --b) { o.push_back(w[a]); if (a != b) o.push_back(w[b]); }
        return o;
    }();
    const int sweeps = sweeps_fixed > 0 ? sweeps_fixed : (int)cheb.size();
    auto weight = [&](int s_) { return sweeps_fixed > 0 ? 0.8 : cheb[(size_t)s_]; };
    hipStream_t st = h->stream;
    const int nb = bt.nb;
    const int64_t nbk = h->n_penalty;
    const OpDev A = h->ops[0].dev(bt.op);
    const OpDev Ab = h->pen_op.dev(bt.op);
    const cplx *pcb = pc_level(h, (int)h->ops.size());
    if (bt.op == WAE_OP_N && h->pen_row_op.n == nbk) {
        // residual on the penalty rows only: their rows of the operator as a small (n_b x d) operator of its own -- the full
        // fine-level SpMV this replaces cost as much as a Krylov step's operator product per chunk
        launch_gather_rows(B, h->pen_rows.p, nbk, nb, h->pen_t.p, st);
        launch_spmv(h->pen_row_op.dev(WAE_OP_N), pc_level(h, (int)h->ops.size() + 1), bt.cps, X, h->pen_b.p, h->pen_t.p, 0.0, nb, MODE_RES, st);
    } else {
        launch_spmv(A, pc_level(h, 0), bt.cps, X, h->W.p, B, 0.0, nb, MODE_RES, st);
        launch_gather_rows(h->W.p, h->pen_rows.p, nbk, nb, h->pen_b.p, st);
    }
    launch_norms(h->pen_b.p, nbk, nb, h->partial.p, h->hdev.p, st);
    cplx *x = h->pen_x.p, *t = h->pen_t.p;
    launch_jacobi0(Ab, pcb, bt.cps, h->pen_b.p, x, weight(0), nb, st);
    for (int s = 1; s < sweeps; ++s) {
        launch_spmv(Ab, pcb, bt.cps, x, t, h->pen_b.p, weight(s), nb, MODE_JAC, st);
        std::swap(x, t);
    }
    launch_spmv(Ab, pcb, bt.cps, x, t, h->pen_b.p, 0.0, nb, MODE_RES, st);
    launch_norms(t, nbk, nb, h->partial.p, h->hdev.p + nb, st);
    cplx *hp = h->h_pinned;
    HIP_CHECK(hipMemcpyAsync(hp, h->hdev.p, (size_t)2 * nb * sizeof(cplx), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    for (int b = 0; b < nb; ++b)
        if (!(hp[nb + b].x <= 1e-3 * hp[b].x)) return;          // not contracting (or NaN): leave X alone
    launch_scatter_add_rows(x, h->pen_rows.p, nbk, nb, X, st);
}

// The solver's environment switches, read once per process
struct GmresEnv {
    bool lazy = env_int("WAE_LAZY", 1) != 0;                  // 0: the normalisation pass instead of the unnormalised basis
    double lazy_limit = getenv("WAE_LAZY_LIMIT") ? atof(getenv("WAE_LAZY_LIMIT")) : 1e100;   // range guard of the unnormalised basis
    bool device = env_int("WAE_GMRES_DEVICE", 1) != 0;        // 0: the wide batches run the host recurrence too
    int sync = std::max(1, env_int("WAE_GMRES_SYNC", 4));     // iterations between two looks at the device recurrence's status words
    int pair_min = env_int("WAE_GMRES_PAIR", 2);              // device pair steps from this step of a cycle on (< 0: off; 4 until round 4: 2.02 -> 1.99 s per pass)
    int narrow_pair = env_int("WAE_NARROW_PAIR", -1);         // narrow pair steps at every size (1), never (0), from 4 MB per basis vector (-1)
    int debug = env_int("WAE_GMRES_DEBUG", 0);                // 1: one line per solve, 2: also per cycle start, 3: also the wide batches' step counts
    bool mask0 = env_int("WAE_GMRES_MASK0", 1) != 0;          // 0: the device recurrence masks converged chunks only in solves that start from a guess
};
static const GmresEnv &gmres_env() { static const GmresEnv e; return e; }

// LEFT-preconditioned GMRES(m) on  M^-1 A x = M^-1 b  (M^-1 = one multigrid V-cycle), all columns in lock-step.
// Every norm is therefore a norm of the preconditioned residual M^-1 r ~ the error itself.  This matters here:
// the admittance rows carry 1e15-sized entries (Helmholtz.jl:151-156), so the plain residual norm is dominated
// by a handful of boundary rows and says nothing about the interior (a right-preconditioned version accepted
// x = x0/z as "converged" to 1e-17 in inveriter's first step).
// Deflation of a known near-null direction g (guess_dir; the Newton-type solvers pass their current eigenvector
// estimate): with u = M^-1 A g, u^ = u/||u||, the Krylov process runs on P M^-1 A, P = I - u^ u^H (u^ sits in front of
// the basis and takes part in the Gram-Schmidt step; the coefficient c_j = u^H M^-1 A v_j it removes is kept), and
// the solution is x = V y + alpha g with alpha = (u^H r0 - sum_j y_j c_j)/||u||, which cancels the u^ component of
// the residual exactly.  Close to an eigenvalue of the NLEVP the operator is nearly singular along g: the undeflated
// solves needed 50-100 iterations of a long recurrence there, the deflated operator behaves like a regular shift.
struct Gmres {
    wae_family *h;
    const Batch &bt;
    const cplx *B;
    cplx *X;
    const cplx *guess_dir;
    double tol;
    int maxit;
    // X already holds an initial guess (the Galerkin projection on earlier solutions, beyn_moments_rb); the stopping test
    // stays relative to ||M^-1 b||, so the answer is the same as from a zero guess, only cheaper
    bool have_x0;
    double *relres_out = nullptr;                     // (optional) the final relative residual of every column (0: a zero right-hand side)
    hipStream_t st = h->stream;
    int nb = bt.nb;
    int64_t n = h->d;
    size_t vec = (size_t)n * nb;
    OpDev A = h->ops[0].dev(bt.op);
    const cplx *pc = pc_level(h, 0);
    cplx *hp = h->h_pinned;
    // narrow batches get a longer recurrence from the same workspace (near-singular systems in the Newton-type
    // solvers stall under short restarts); they also afford a second Gram-Schmidt pass
    bool reorth = nb <= 8;
    // (a single-level hierarchy is the exact dense inverse: nothing to deflate, and the inverse of a numerically singular
    // small matrix is not something to build a projector from)
    bool deflate = guess_dir != nullptr && h->ops.size() > 1;
    int off = deflate ? 1 : 0;                        // basis slot of v_0: u^ in front of it
    // recurrence length 150 (round 4, narrow solves of the C3 refinement: 24 / 32 / 40 / 60 / 150 steps, 2.26 / 2.16 / 1.00 / 0.85 / 0.85 s)
    int m = (int)std::min<size_t>(150, h->V.n / vec - 1) - off;
    // wide batches, single Gram-Schmidt pass: unnormalised basis (single_step; 4096: coefficients of one axpy launch)
    bool lazy = gmres_env().lazy && !reorth && ((size_t)m + off + 2) * nb <= 4096 && ((size_t)m + off + 2) * nb <= h->vsq.n;
    // Pair steps in the two-pass recurrence (vec.hip "Two Arnoldi steps per pass over the basis"): w1 = Op v_j, w2 = Op w1, both
    // orthogonalised against V_0..j by two passes of classical Gram-Schmidt that read the basis ONCE each for the two vectors -- four
    // readings of the basis per two steps instead of eight; same Krylov space, Hessenberg columns recovered on the host (pair_step).
    // For batches whose basis vectors are large enough for the readings to be what an iteration costs (>= 4 MB per vector).
    // With the deflation vector u^: w1 is projected, w1 <- (I - u^ u^H) w1, before the operator is applied to it -- one inner
    // product and one update with a single vector -- so that w2 = Op (P Op v_j) continues the recurrence of P Op; u^ then takes part in
    // the two passes like a basis vector.  WAE_NARROW_PAIR=0: off, =1: at every size.
    bool pair_cfg = reorth && h->ops.size() > 1 &&
                    (gmres_env().narrow_pair > 0 || (gmres_env().narrow_pair < 0 && vec * sizeof(cplx) >= ((size_t)4 << 20)));
    size_t PK = (size_t)(m + off + 3) * nb;           // one coefficient block of the pair steps
    std::vector<double> bnorm = std::vector<double>(nb), relres = std::vector<double>(nb, 0.0);
    std::vector<int> iters = std::vector<int>(nb, 0);
    std::vector<unsigned char> done = std::vector<unsigned char>(nb, 0), stalled = std::vector<unsigned char>(nb, 0);
    int total_it = 0;
    bool nan_seen = false, x0_unchecked = have_x0;
    double t0 = now_s();
    // host recurrence only
    std::vector<ColState> cs;
    std::vector<std::vector<double>> sv;               // lazy: the scale s_i of every basis slot
    std::vector<std::vector<double>> hist = std::vector<std::vector<double>>(nb);   // per column: the residual estimate of every step
    std::vector<double> unorm = std::vector<double>(nb, 0.0);   // deflation: ||M^-1 A g|| (0: no deflation for that column)
    std::vector<zc> beta0 = std::vector<zc>(nb, zc(0));        // deflation: u^H r0 of the cycle's residual
    const unsigned char *mk = nullptr;
    cplx *pr_dev = nullptr, *pr_host = nullptr;

    // X = 0 unless have_x0; returns M^-1 b, whose norm scales the stopping test; from a zero guess it is also the first
    // preconditioned residual (nothing touches the V-cycle's buffers until then).  From a guess nobody reads M^-1 b itself: a cycle
    // that can deliver the norms from its last kernel does not write it.
    cplx *start() {
        if (!have_x0) launch_fill_zero(X, vec, st);
        CycleNorms cn{h->hdev.p, have_x0};
        cplx *const zb = vcycle(h, bt, 0, B, nullptr, false, nullptr, &cn);
        if (!cn.done) launch_norms(zb, n, nb, h->partial.p, h->hdev.p, st);
        HIP_CHECK(hipMemcpyAsync(hp, h->hdev.p, nb * sizeof(cplx), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        for (int b = 0; b < nb; ++b) { bnorm[b] = hp[b].x; if (!(bnorm[b] > 0.0)) done[b] = 1; }
        return zb;
    }
    cplx *residual(CycleNorms *cn = nullptr) {        // M^-1 (b - A x)
        launch_spmv(A, pc, bt.cps, X, h->W.p, B, 0.0, nb, MODE_RES, st);
        return vcycle(h, bt, 0, h->W.p, nullptr, false, nullptr, cn);
    }
    // a guess that is worse than no guess (an ill-conditioned projected system) is dropped, column by column (true: start over)
    bool drop_bad_guess() {
        if (!x0_unchecked) return false;
        x0_unchecked = false;
        std::vector<cplx> keep(nb, cplx{1.0, 0.0});
        bool any_bad = false;
        for (int b = 0; b < nb; ++b)
            if (bnorm[b] > 0.0 && !(hp[b].x / bnorm[b] <= 1.0)) { keep[b] = cplx{0.0, 0.0}; any_bad = true; }
        if (!any_bad) return false;
        h->ydev.upload(keep.data(), nb, st);
        launch_mask_cols(X, h->ydev.p, n, nb, st);
        HIP_CHECK(hipStreamSynchronize(st));
        return true;
    }
    // relative residuals (norms in hp), done flags and NaN at a cycle start, more(b) after each column; true when all are done
    template <class F> bool cycle_start(F &&more) {
        bool all_done = true;
        for (int b = 0; b < nb; ++b) {
            if (bnorm[b] > 0.0) {
                relres[b] = hp[b].x / bnorm[b];
                if (std::isnan(relres[b])) nan_seen = true;
                done[b] = relres[b] <= tol || stalled[b];
                more(b);
            }
            if (!done[b]) all_done = false;
        }
        return all_done;
    }
    // A short recurrence that ended with every column converged by its Arnoldi estimate needs no confirmation by a
    // true residual (another SpMV + V-cycle): over <= 12 steps the estimate equals the preconditioned residual to
    // rounding.  Long recurrences (Gram-Schmidt drift) and stalled columns are always re-checked at the loop top.
    bool converged_by_estimate(int j) const {
        if (j > 12) return false;
        for (int b = 0; b < nb; ++b) if (stalled[b] || (bnorm[b] > 0.0 && !(relres[b] <= tol))) return false;
        return true;
    }
    // polish of a projected guess, the debug line, the statistics, the NaN error; returns the number of lock-step iterations
    template <class F> int finish(wae_solve_info *info, F &&debug_line) {
        if (have_x0 && !nan_seen) penalty_polish(h, bt, B, X);
        if (relres_out) for (int b = 0; b < nb; ++b) relres_out[b] = bnorm[b] > 0.0 ? relres[b] : 0.0;
        if (gmres_env().debug) {
            HIP_CHECK(hipStreamSynchronize(st));
            debug_line();
        }
        if (info) {
            int imax = 0, itot = 0, nun = 0;
            double rmax = 0.0;
            for (int b = 0; b < nb; ++b) {
                imax = std::max(imax, iters[b]);
                itot += iters[b];
                if (bnorm[b] > 0.0) {
                    if (!(relres[b] <= tol)) ++nun;
                    rmax = std::max(rmax, relres[b]);
                }
                if (stalled[b] && !(relres[b] <= tol)) info->levels |= 1 << 16;   // stagnation marker (masked off below)
            }
            info->iters_max = std::max(info->iters_max, imax);
            info->iters_total += itot;
            info->n_unconverged += nun;
            info->relres_max = std::max(info->relres_max, rmax);
            info->levels = (info->levels & (1 << 16)) | (int)h->ops.size();
        }
        if (nan_seen) throw WaeError(WAE_ERR_NAN, "NaN in GMRES");
        return total_it;
    }

    // The device recurrence: the same left-preconditioned, lock-step, unnormalised-basis GMRES(m) as the host's lazy form, with the
    // per-column Hessenberg / Givens / convergence bookkeeping in kernels (vec.hip gmres_*_kernel): an iteration is a chain of
    // launches with no device-to-host copy; the host looks at three status words every WAE_GMRES_SYNC iterations (default 4) and at
    // the per-column figures once per restart cycle.  In batches of at least 8 columns an 8-column chunk whose columns have all
    // converged is masked on the device at once and skipped by every kernel of the recurrence, from a guess and from zero alike, so
    // finished systems cost launches, not traffic, while the slowest one ends.  A masked chunk of a basis slot keeps stale bits; the
    // update x += V y never reads them, because their coefficients are exact zeros (vec.hip axpy_neg_kernel).  WAE_GMRES_MASK0=0 masks
    // only in solves that start from a guess, as it was while that update still read every entry.
    int run_device(wae_solve_info *info) {
        const GmresEnv &env = gmres_env();
        const double lim = env.lazy_limit;
        const bool use_mask = have_x0 || (env.mask0 && nb >= 8);
        const int nch = (nb + 7) / 8;
        const int histcap = maxit + m + 8;
        // device state
        auto ens = [](auto &buf, size_t cnt) { if (buf.n < cnt) buf.alloc(cnt); };
        ens(h->gs_R, (size_t)m * (m + 1) * nb); ens(h->gs_sn, (size_t)m * nb); ens(h->gs_g, (size_t)(m + 1) * nb); ens(h->gs_rescale, (size_t)nb);
        ens(h->gs_cs, (size_t)m * nb); ens(h->gs_sv, (size_t)(m + 2) * nb); ens(h->gs_relres, (size_t)nb); ens(h->gs_bnorm, (size_t)nb);
        ens(h->gs_hist, (size_t)histcap * nb); ens(h->gs_int, (size_t)5 * nb + 4); ens(h->gs_done, (size_t)nb);
        if (h->cmask.n < (size_t)nch) h->cmask.alloc(nch);
        if (h->vsq.n < (size_t)(m + 2) * nb) h->vsq.alloc((size_t)(m + 2) * nb);
        GmresDev S;
        S.nb = nb; S.m = m; S.histcap = histcap;
        S.R = h->gs_R.p; S.cs = h->gs_cs.p; S.sn = h->gs_sn.p; S.g = h->gs_g.p; S.sv = h->gs_sv.p; S.vsq = h->vsq.p;
        S.conv = h->gs_int.p; S.steps = S.conv + nb; S.iters = S.steps + nb; S.histlen = S.iters + nb; S.stalled = S.histlen + nb; S.status = S.stalled + nb;
        S.relres = h->gs_relres.p; S.bnorm = h->gs_bnorm.p; S.hist = h->gs_hist.p; S.rescale = h->gs_rescale.p; S.cmask = h->cmask.p;
        // Pair steps (vec.hip "Two Arnoldi steps per pass over the basis"): from iteration pair_min of a cycle on, while most columns
        // are still active, the operator is applied twice before the Gram-Schmidt pass.  Same Krylov space, same per-column stopping test
        // after each of the two steps; what it costs is one operator application when the batch ends on the first step of a pair.
        const int pair_min = env.pair_min;
        const bool pair_on = pair_min >= 0 && lim >= 1e50 && nb >= 8 && h->ops.size() > 1;
        ens(h->gs_Hraw, (size_t)m * (m + 1) * nb); ens(h->gs_pair, ((size_t)4 * (m + 3) + 8) * nb);
        if (h->gs_sub.n < (size_t)m * nb) h->gs_sub.alloc((size_t)m * nb);
        S.Hraw = h->gs_Hraw.p; S.sub = h->gs_sub.p;
        cplx *const pr_c1 = h->gs_pair.p, *const pr_c2 = pr_c1 + (size_t)(m + 3) * nb, *const pr_c2m = pr_c2 + (size_t)(m + 3) * nb,
                   *const pr_hd2 = pr_c2m + (size_t)(m + 3) * nb, *const pr_gram = pr_hd2 + (size_t)(m + 3) * nb, *const pr_alpha = pr_gram + (size_t)3 * nb,
                   *const pr_norm = pr_alpha + nb;
        HIP_CHECK(hipMemsetAsync(h->gs_int.p, 0, ((size_t)5 * nb + 4) * sizeof(int), st));
        cplx *const zb = start();
        std::vector<double> bn(bnorm);
        for (double &v : bn) if (!(v > 0.0)) v = 1.0;
        HIP_CHECK(hipMemcpyAsync(h->gs_bnorm.p, bn.data(), nb * sizeof(double), hipMemcpyHostToDevice, st));
        HIP_CHECK(hipStreamSynchronize(st));
        std::vector<int> hostint((size_t)5 * nb + 4);
        bool first = !have_x0;
        while (true) {
            CycleNorms cn{h->hdev.p, false};
            cplx *const z0 = first ? zb : residual(&cn);
            first = false;
            if (!cn.done) launch_norms(z0, n, nb, h->partial.p, h->hdev.p, st);
            HIP_CHECK(hipMemcpyAsync(hp, h->hdev.p, (size_t)nb * sizeof(cplx), hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
            if (drop_bad_guess()) continue;
            if (cycle_start([](int) {}) || total_it >= maxit || nan_seen) break;
            launch_scale_inv(z0, h->hdev.p, h->V.p, n, nb, st);                       // V0 = M^-1 r / beta
            HIP_CHECK(hipMemcpyAsync(h->gs_done.p, done.data(), nb, hipMemcpyHostToDevice, st));
            launch_gmres_init(S, h->hdev.p, h->gs_done.p, use_mask ? 1 : 0, st);
            HIP_CHECK(hipStreamSynchronize(st));                                       // (`done` is reused by the host below)
            const unsigned char *mk = (use_mask && nb >= 8) ? h->cmask.p : nullptr;
            int j = 0;
            int status[4] = {0, 0, 0, 0};
            for (int b = 0; b < nb; ++b) status[0] += done[b] ? 0 : 1;              // columns still to converge at the start of this cycle
            int since_sync = 0;
            for (; j < m && total_it < maxit;) {
                const cplx *vj = h->V.p + (size_t)j * vec;
                const int nvj = j + 1;
                const bool fuse0 = h->ops.size() > 1;
                if (pair_on && j >= pair_min && j + 2 <= m && total_it + 2 <= maxit && status[0] > nb / 4) {
                    cplx *w1 = h->V.p + (size_t)nvj * vec, *w2 = w1 + vec;         // computed in their basis slots, orthogonalised in place
                    launch_spmv(A, pc, bt.cps, vj, h->W.p, h->lx[0].p, pre_weight(h), nb, MODE_AX_J0, st, mk);
                    vcycle(h, bt, 0, h->W.p, mk, true, w1);
                    launch_spmv(A, pc, bt.cps, w1, h->W.p, h->lx[0].p, pre_weight(h), nb, MODE_AX_J0, st, mk);
                    vcycle(h, bt, 0, h->W.p, mk, true, w2);
                    launch_dots2_scaled(h->V.p, vec, nvj, w1, w2, n, nb, h->partial.p, pr_c1, pr_c2, pr_gram, h->vsq.p, st, mk);
                    launch_gmres_pair_coef(S, j, pr_c1, pr_c2, pr_gram, pr_alpha, pr_c2m, pr_hd2, st);
                    launch_axpy2_norm(h->V.p, vec, nvj, pr_c1, pr_c2m, pr_alpha, w1, w2, n, nb, h->partial.p, pr_norm, h->vsq.p + (size_t)nvj * nb, st, mk);
                    // (the middle vector is not renormalised in place -- the relation of the vector after it was formed with it as it is;
                    // its norm is within one operator application of a vector the range guard has seen)
                    launch_gmres_step(S, pr_c1, j, tol, 1e300, use_mask ? 1 : 0, w1, n, st, pr_norm);
                    launch_gmres_step(S, pr_hd2, j + 1, tol, lim, use_mask ? 1 : 0, w2, n, st, pr_norm + nb);
                    j += 2;
                    total_it += 2;
                    since_sync += 2;
                } else {
                    launch_spmv(A, pc, bt.cps, vj, h->W.p, fuse0 ? h->lx[0].p : nullptr, fuse0 ? pre_weight(h) : 0.0, nb, fuse0 ? MODE_AX_J0 : MODE_AX, st, mk);
                    cplx *w = vcycle(h, bt, 0, h->W.p, mk, fuse0);
                    launch_dots_scaled(h->V.p, vec, nvj, w, n, nb, h->partial.p, h->hdev.p, h->vsq.p, st, mk);
                    launch_axpy_neg_norm(h->V.p, vec, nvj, h->hdev.p, h->V.p + (size_t)nvj * vec, n, nb, h->partial.p, h->hdev.p + (size_t)nvj * nb, st, mk,
                                         w, h->vsq.p + (size_t)nvj * nb);
                    launch_gmres_step(S, h->hdev.p, j, tol, lim, use_mask ? 1 : 0, h->V.p + (size_t)nvj * vec, n, st);
                    ++j;
                    ++total_it;
                    ++since_sync;
                }
                // look at the status words every ksync iterations -- every iteration once few columns are left (the end of the
                // cycle is near: an overshoot iteration is ~25 launches of fully masked kernels)
                // (from a projected guess most columns need one or two steps: the first four steps of such a cycle are looked at one by one --
                // a look costs a 12-byte copy and a stream wait, a step run in vain 25 launches of partly masked kernels)
                if (since_sync >= ((have_x0 && j <= 4) ? 1 : env.sync) || j == m || total_it >= maxit || status[0] <= nb / 4) {
                    since_sync = 0;
                    HIP_CHECK(hipMemcpyAsync(status, S.status, 3 * sizeof(int), hipMemcpyDeviceToHost, st));
                    HIP_CHECK(hipStreamSynchronize(st));
                    if (status[1]) nan_seen = true;
                    if (status[0] == 0 || nan_seen) break;
                }
            }
            // x += V y on the device, then the per-column figures of this cycle
            if (j > 0) {
                launch_gmres_solve_y(S, j, h->ydev.p, st);
                launch_lincomb_add(h->V.p, vec, j, h->ydev.p, X, n, nb, st);
            }
            HIP_CHECK(hipMemcpyAsync(hostint.data(), h->gs_int.p, ((size_t)5 * nb + 4) * sizeof(int), hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipMemcpyAsync(hp, h->gs_relres.p, nb * sizeof(double), hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
            const double *rr = (const double *)hp;
            for (int b = 0; b < nb; ++b) {
                iters[b] = hostint[(size_t)2 * nb + b];
                stalled[b] = (unsigned char)hostint[(size_t)4 * nb + b];
                if (hostint[(size_t)nb + b] > 0 && bnorm[b] > 0.0) relres[b] = rr[b];      // columns that took steps in this cycle
            }
            if (hostint[(size_t)5 * nb + 1]) nan_seen = true;
            if (nan_seen || converged_by_estimate(j)) break;
        }
        return finish(info, [&]() {
            int itot = 0;
            for (int b = 0; b < nb; ++b) itot += iters[b];
            fprintf(stderr, "[gmres] nb=%d x0=%d lockstep_its=%d column_its=%d %.1f ms (device recurrence)\n", nb, (int)have_x0, total_it, itot,
                    (now_s() - t0) * 1e3);
            if (env.debug > 2) {                                  // per-column step counts, one system per line
                for (int b0 = 0; b0 < nb; b0 += bt.cps) {
                    fprintf(stderr, "[gmres]   steps");
                    for (int b = b0; b < std::min(nb, b0 + bt.cps); ++b) fprintf(stderr, " %d", iters[b]);
                    fprintf(stderr, "\n");
                }
            }
        });
    }

    // one new column (raw[0..jc+1]) of the Hessenberg matrix of batch column b: rotations, residual estimate, stopping tests
    void absorb(int b, int jc, const zc *raw, zc cdef_j) {
        ColState &c = cs[b];
        if (c.conv || !c.rotate_in(jc, raw, cdef_j, nan_seen)) return;
        iters[b]++;
        relres[b] = std::abs(c.g[jc + 1]) / bnorm[b];
        hist[b].push_back(relres[b]);
        const size_t hs = hist[b].size();
        if (relres[b] <= 0.7 * tol) c.conv = true;
        else if (hs > 60 && relres[b] > 0.9 * hist[b][hs - 31]) { c.conv = true; stalled[b] = 1; }   // attainable accuracy reached
    }

    // two steps per reading of the basis (see the comment at pair_cfg): columns j and j+1 of every Hessenberg matrix
    void pair_step(int j) {
        const cplx *vj = h->V.p + (size_t)(off + j) * vec;
        const int nv = off + j + 1;                          // orthogonalisation set: u^ (when deflating), v_0..v_j
        cplx *w1 = h->V.p + (size_t)nv * vec, *w2 = w1 + vec;
        cplx *c1a = pr_dev, *c2a = c1a + PK, *c1b = c2a + PK, *c2b = c1b + PK, *c2m = c2b + PK, *zero_al = c2m + PK,
             *gram = zero_al + nb, *alpha = gram + 3 * (size_t)nb, *nrm = alpha + nb, *inv = nrm + 2 * (size_t)nb,
             *tdef = inv + 2 * (size_t)nb;
        launch_spmv(A, pc, bt.cps, vj, h->W.p, h->lx[0].p, pre_weight(h), nb, MODE_AX_J0, st, mk);
        vcycle(h, bt, 0, h->W.p, mk, true, w1);
        if (deflate) {                                       // w1 <- P w1, t = u^H w1 kept for the deflation coefficient
            launch_dots(h->V.p, vec, 1, w1, n, nb, h->partial.p, tdef, st, mk);
            launch_axpy_neg(h->V.p, vec, 1, tdef, w1, n, nb, st, mk);
        }
        launch_spmv(A, pc, bt.cps, w1, h->W.p, h->lx[0].p, pre_weight(h), nb, MODE_AX_J0, st, mk);
        vcycle(h, bt, 0, h->W.p, mk, true, w2);
        // first pass
        launch_dots2_scaled(h->V.p, vec, nv, w1, w2, n, nb, h->partial.p, c1a, c2a, gram, h->vsq.p, st, mk);
        launch_fill_zero(zero_al, nb, st);
        launch_axpy2_norm(h->V.p, vec, nv, c1a, c2a, zero_al, w1, w2, n, nb, h->partial.p, nrm, inv, st, mk);
        // second pass: coefficients, and the Gram entries of the once-orthogonalised pair
        launch_dots2_scaled(h->V.p, vec, nv, w1, w2, n, nb, h->partial.p, c1b, c2b, gram, h->vsq.p, st, mk);
        HIP_CHECK(hipMemcpyAsync(pr_host, pr_dev, (4 * PK) * sizeof(cplx), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(pr_host + 5 * PK + nb, gram, (size_t)3 * nb * sizeof(cplx), hipMemcpyDeviceToHost, st));
        cplx *htdef = pr_host + 5 * PK + 7 * (size_t)nb;
        if (deflate) HIP_CHECK(hipMemcpyAsync(htdef, tdef, (size_t)nb * sizeof(cplx), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        const cplx *hc1a = pr_host, *hc2a = hc1a + PK, *hc1b = hc2a + PK, *hc2b = hc1b + PK, *hgram = pr_host + 5 * PK + nb;
        cplx *hc2m = pr_host + 4 * PK, *halpha = pr_host + 5 * PK + 4 * (size_t)nb;
        auto Z = [](const cplx &v) { return zc(v.x, v.y); };
        std::vector<zc> rawcol((size_t)m + 3);
        std::vector<zc> beta(nb, zc(0));
        for (int b = 0; b < nb; ++b) {
            // after the second update: w1'' = w1' - V c1b, w2'' = w2' - V c2b; the second vector is made orthogonal to the
            // first in the same kernel: beta = (w1''^H w2'') / ||w1''||^2, both from the Gram entries of (w1', w2')
            double g11 = hgram[b].x;
            zc g12 = Z(hgram[(size_t)nb + b]);
            for (int i = 0; i < nv; ++i) {
                const zc p1 = Z(hc1b[(size_t)i * nb + b]), p2 = Z(hc2b[(size_t)i * nb + b]);
                g11 -= std::norm(p1);
                g12 -= std::conj(p1) * p2;
            }
            beta[b] = g11 > 0.0 ? g12 / g11 : zc(0);
            if (!std::isfinite(beta[b].real()) || !std::isfinite(beta[b].imag())) beta[b] = zc(0);
            halpha[b] = cplx{beta[b].real(), beta[b].imag()};
            for (int i = 0; i < nv; ++i) {
                const zc q = Z(hc2b[(size_t)i * nb + b]) - beta[b] * Z(hc1b[(size_t)i * nb + b]);
                hc2m[(size_t)i * nb + b] = cplx{q.real(), q.imag()};
            }
        }
        HIP_CHECK(hipMemcpyAsync(c2m, hc2m, (size_t)nv * nb * sizeof(cplx), hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemcpyAsync(alpha, halpha, (size_t)nb * sizeof(cplx), hipMemcpyHostToDevice, st));
        launch_axpy2_norm(h->V.p, vec, nv, c1b, c2m, alpha, w1, w2, n, nb, h->partial.p, nrm, inv, st, mk);
        launch_scale_inv(w1, nrm, w1, n, nb, st, mk);                    // a zero norm leaves the vector as it is (breakdown: below)
        launch_scale_inv(w2, nrm + nb, w2, n, nb, st, mk);
        cplx *hnrm = pr_host + 5 * PK + 5 * (size_t)nb;
        HIP_CHECK(hipMemcpyAsync(hnrm, nrm, (size_t)2 * nb * sizeof(cplx), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        total_it += 2;
        for (int b = 0; b < nb; ++b) {
            ColState &c = cs[b];
            if (c.conv) continue;
            const double a1 = hnrm[b].x, a2 = hnrm[(size_t)nb + b].x;
            // column j:  Op v_j = u^ (t + e1) + V cc1 + a1 v_{j+1}   (cc: the sums of the two passes; e: their u^ entries)
            const int nk = j + 1;
            std::vector<zc> cc1(nk), cc2(nk);
            for (int i = 0; i < nk; ++i) {
                cc1[i] = Z(hc1a[(size_t)(off + i) * nb + b]) + Z(hc1b[(size_t)(off + i) * nb + b]);
                cc2[i] = Z(hc2a[(size_t)(off + i) * nb + b]) + Z(hc2b[(size_t)(off + i) * nb + b]);
            }
            const zc e1 = deflate ? Z(hc1a[b]) + Z(hc1b[b]) : zc(0), e2 = deflate ? Z(hc2a[b]) + Z(hc2b[b]) : zc(0);
            const zc cdef_j = deflate ? Z(htdef[b]) + e1 : zc(0);
            for (int i = 0; i < nk; ++i) rawcol[i] = cc1[i];
            rawcol[nk] = a1;
            absorb(b, j, rawcol.data(), cdef_j);
            if (c.conv) continue;
            if (!(a1 > 0.0)) { c.conv = true; continue; }            // invariant subspace: the first step ended the recurrence
            // column j+1:  Op v_{j+1} = (w2 - Op V cc1) / a1,  Op V cc1 = V_{0..j+1} (H_{0..j-1} cc1[0..j-1]) + cc1[j] w1  (Arnoldi
            // relation of the earlier columns),  w1 = V cc1 + a1 v_{j+1},  w2 = V cc2 + beta a1 v_{j+1} + a2 v_{j+2}
            for (int r = 0; r <= j; ++r) {
                zc d = 0;
                for (int i = std::max(0, r - 1); i < j; ++i) d += c.Hraw[(size_t)i * c.ld + r] * cc1[i];
                rawcol[r] = (cc2[r] - d - cc1[j] * cc1[r]) / a1;
            }
            rawcol[j + 1] = beta[b] - cc1[j];
            rawcol[j + 2] = a2 / a1;
            zc cdef_n = 0;
            if (deflate) {                                   // u^ part of Op v_{j+1}: (e2 - sum_{i<=j} cc1_i cdef_i) / a1
                cdef_n = e2 - cc1[j] * cdef_j;
                for (int i = 0; i < j; ++i) cdef_n -= cc1[i] * c.cdef[i];
                cdef_n /= a1;
            }
            absorb(b, j + 1, rawcol.data(), cdef_n);
        }
    }

    // one Arnoldi step: CGS2 (reorth), one pass with the normalisation, or one pass on the unnormalised basis (lazy)
    void single_step(int j) {
        const cplx *vj = h->V.p + (size_t)(off + j) * vec;
        const int nvj = off + j + 1;                         // vectors in the orthogonalisation set (u^ first when deflating)
        const bool fuse0 = h->ops.size() > 1;                // A v_j and the V-cycle's first sweep on it in one kernel
        launch_spmv(A, pc, bt.cps, vj, h->W.p, fuse0 ? h->lx[0].p : nullptr, fuse0 ? pre_weight(h) : 0.0, nb, fuse0 ? MODE_AX_J0 : MODE_AX, st, mk);
        cplx *w = vcycle(h, bt, 0, h->W.p, mk, fuse0);       // w = M^-1 A v_j  (lives in a V-cycle buffer)
        if (lazy) {
            // The basis is kept UNNORMALISED (v_i = s_i V^_i, s_i = 1/||V^_i||): M^-1 A is linear, so w^ = M^-1 A V^_j = w/s_j,
            // the update coefficients of w^ against V^_i are s_i^2 (V^_i^H w^) -- s_j cancels -- and the new vector goes
            // straight into its slot; the host rescales what it reads (h_ij = s_j c_i / s_i, h_{j+1,j} = s_j ||w^'||).
            // Saves the normalisation pass (read + write of one multivector) of every iteration.
            launch_dots_scaled(h->V.p, vec, nvj, w, n, nb, h->partial.p, h->hdev.p, h->vsq.p, st, mk);
            launch_axpy_neg_norm(h->V.p, vec, nvj, h->hdev.p, h->V.p + (size_t)nvj * vec, n, nb, h->partial.p, h->hdev.p + (size_t)nvj * nb, st, mk,
                                 w, h->vsq.p + (size_t)nvj * nb);
        } else {
            launch_dots(h->V.p, vec, nvj, w, n, nb, h->partial.p, h->hdev.p, st, mk);
            if (reorth) {   // CGS2: h += V^H w', w' -= V (V^H w')
                launch_axpy_neg(h->V.p, vec, nvj, h->hdev.p, w, n, nb, st, mk);
                cplx *h2 = h->hdev.p + (size_t)(off + m + 2) * nb;
                launch_dots(h->V.p, vec, nvj, w, n, nb, h->partial.p, h2, st, mk);
                launch_axpy_neg_norm(h->V.p, vec, nvj, h2, w, n, nb, h->partial.p, h->hdev.p + (size_t)nvj * nb, st, mk);
                launch_add(h2, h->hdev.p, (size_t)nvj * nb, st);
            } else {        // the update and the norm of its result in one pass
                launch_axpy_neg_norm(h->V.p, vec, nvj, h->hdev.p, w, n, nb, h->partial.p, h->hdev.p + (size_t)nvj * nb, st, mk);
            }
            launch_scale_inv(w, h->hdev.p + (size_t)nvj * nb, h->V.p + (size_t)nvj * vec, n, nb, st, mk);
        }
        HIP_CHECK(hipMemcpyAsync(hp, h->hdev.p, (size_t)(nvj + 1) * nb * sizeof(cplx), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        if (lazy) {                                  // back to the coefficients of the normalised recurrence
            for (int b = 0; b < nb; ++b) {
                const double sj = sv[nvj - 1][b];
                for (int i = 0; i < nvj; ++i) {
                    const double f = sv[i][b] > 0.0 ? sj / sv[i][b] : 0.0;
                    hp[(size_t)i * nb + b].x *= f;
                    hp[(size_t)i * nb + b].y *= f;
                }
                const double r = hp[(size_t)nvj * nb + b].x;
                sv[nvj][b] = r > 0.0 ? 1.0 / r : 0.0;
                hp[(size_t)nvj * nb + b].x = sj * r;
            }
            // the stored norms are the running products of the sub-diagonal entries: long recurrences could carry them
            // out of range (their squares are used) -- normalise this one vector in place and start over from 1
            const double lim = gmres_env().lazy_limit;
            bool rescale = false;
            for (int b = 0; b < nb; ++b) rescale = rescale || sv[nvj][b] > lim || (sv[nvj][b] > 0.0 && sv[nvj][b] < 1.0 / lim);
            if (rescale) {
                launch_scale_inv(h->V.p + (size_t)nvj * vec, h->hdev.p + (size_t)nvj * nb, h->V.p + (size_t)nvj * vec, n, nb, st, mk);
                std::vector<cplx> ones(nb, cplx{1.0, 0.0});
                for (int b = 0; b < nb; ++b) if (sv[nvj][b] > 0.0) sv[nvj][b] = 1.0; else ones[b] = cplx{0.0, 0.0};
                HIP_CHECK(hipMemcpyAsync(h->vsq.p + (size_t)nvj * nb, ones.data(), (size_t)nb * sizeof(cplx), hipMemcpyHostToDevice, st));
                HIP_CHECK(hipStreamSynchronize(st));
            }
        }
        ++total_it;
        std::vector<zc> rawcol((size_t)m + 3);
        for (int b = 0; b < nb; ++b) {
            if (cs[b].conv) continue;
            for (int i = 0; i <= j + 1; ++i) rawcol[i] = zc(hp[(size_t)(off + i) * nb + b].x, hp[(size_t)(off + i) * nb + b].y);
            absorb(b, j, rawcol.data(), deflate ? zc(hp[b].x, hp[b].y) : zc(0));
        }
    }

    // The multiple alpha g that cancels the u^ component of the residual is NOT added between cycles: close to an eigenvalue it
    // is ~1/mu times the rest of x, and a residual recomputed from x + alpha g carries the rounding of that cancellation
    // (1e-3..1e-4 of ||M^-1 b|| at 1M DoF, where the recurrence's estimate stood at 1e-12: every solve spent a second and third
    // cycle on it and ended "stalled").  x holds the Krylov part only; the loop top projects the u^ component out of its residual
    // and the exits add alpha g once (there from beta0 of that residual, after a short recurrence from the recurrence's y).
    void add_alpha_g(const std::vector<zc> &num) {
        std::vector<cplx> al(nb, cplx{0.0, 0.0});
        for (int b = 0; b < nb; ++b) {
            if (!(unorm[b] > 0.0)) continue;
            const zc a = num[b] / unorm[b];
            if (std::isfinite(a.real()) && std::isfinite(a.imag())) al[b] = cplx{a.real(), a.imag()};
        }
        h->ydev.upload(al.data(), nb, st);
        launch_lincomb(guess_dir, 0, 1, h->ydev.p, h->U.p, n, nb, st);
        launch_add(h->U.p, X, vec, st);
        HIP_CHECK(hipStreamSynchronize(st));
    }

    int run_host(wae_solve_info *info) {
        sv.assign(lazy ? (size_t)m + off + 2 : 0, std::vector<double>(nb, 1.0));   // basis slots incl. the deflation vector and the newest vector
        const int pair_min = 4;
        if (pair_cfg) {
            const size_t need = 6 * PK + 16 * (size_t)nb;
            if (h->gs_pair.n < need) h->gs_pair.alloc(need);
            if (h->h_pin_pair_n < need) {
                if (h->h_pin_pair) { (void)hipHostFree(h->h_pin_pair); h->h_pin_pair = nullptr; h->h_pin_pair_n = 0; }
                HIP_CHECK(hipHostMalloc((void **)&h->h_pin_pair, need * sizeof(cplx)));
                h->h_pin_pair_n = need;
            }
            pr_dev = h->gs_pair.p; pr_host = h->h_pin_pair;
            if (h->vsq.n < PK) h->vsq.alloc(PK);
            std::vector<cplx> ones(PK, cplx{1.0, 0.0});          // the basis is normalised: unit scales for the scaled inner products
            h->vsq.upload(ones.data(), ones.size(), st);
            HIP_CHECK(hipStreamSynchronize(st));
        }
        cplx *const zb0 = start();        // (with a guess direction, whose set-up runs further V-cycles, not the first residual)
        // Attainable accuracy of the residual itself.  Close to an eigenvalue of the NLEVP the solution is ~1/mu times the right-hand side and
        // M^-1 amplifies along the same direction, so a recomputed M^-1 (b - A x) carries rounding of the order eps |A| |x| ||M^-1|| while
        // the recurrence's estimate has reached the tolerance (with an accurate deflation direction the large part of x stays out of the
        // residual, see add_alpha_g; with a poor one -- the first left solve of a Newton step -- it does not: 1e-2..1e-3 of ||M^-1 b||
        // at 1M DoF).  What is left is a multiple of the near-null direction, which a further cycle cannot remove and an inverse-iteration
        // step does not care about.  A column whose recomputed residual is > 50 x the estimate its cycle ended with (estimate <= tol)
        // switches the batch to cycles of 5 steps (enough to show whether a fresh recurrence still gains: the clean rate is ~0.55 per step),
        // and from then on EVERY column has to halve its recomputed residual per cycle or ends as stalled -- whichever column raised the
        // flag: the columns of a batch sit at their floors one after the other, and with the test tied to the flagged column only the
        // right solves of a Newton step at 1M DoF spent 30 of their 78 steps on a residual that stayed at 2.6e-10.
        std::vector<double> drift_ref(nb, 0.0);         // the recomputed residual at the previous cycle start
        bool drift_mode = false;
        bool first = !have_x0;
        // converged-chunk mask: columns are skipped in groups of 8 (one 128-B segment of every interleaved row) as soon as
        // all 8 have converged -- the columns of one shifted system converge together, so this removes most of the work the
        // lock-step batch would otherwise spend on finished systems.
        // From a zero guess all systems of a batch converge within a few iterations of each other and the predicates cost
        // ~2 %: off.  With projected initial guesses the columns start 0..8 digits from the answer and finish at very
        // different times: on (measured -15 % on the C2 Beyn pass).
        const int nch = (nb + 7) / 8;
        const bool use_mask = have_x0;
        std::vector<unsigned char> cm(nch, 1), cm_prev(nch, 2);
        if (h->cmask.n < (size_t)nch) h->cmask.alloc(nch);
        auto set_mask = [&](auto &&active) {        // the chunks that hold an active column; copied when they have changed
            for (int k = 0; k < nch; ++k) cm[k] = 0;
            for (int b = 0; b < nb; ++b) if (active(b)) cm[b >> 3] = 1;
            if (cm != cm_prev) {
                HIP_CHECK(hipMemcpyAsync(h->cmask.p, cm.data(), nch, hipMemcpyHostToDevice, st));
                HIP_CHECK(hipStreamSynchronize(st));
                cm_prev = cm;
            }
        };
        if (deflate) {
            launch_spmv(A, pc, bt.cps, guess_dir, h->W.p, nullptr, 0.0, nb, MODE_AX, st);
            launch_copy(vcycle(h, bt, 0, h->W.p), h->V.p, vec, st);
            launch_norms(h->V.p, n, nb, h->partial.p, h->hdev.p, st);
            launch_norms(guess_dir, n, nb, h->partial.p, h->hdev.p + nb, st);
            HIP_CHECK(hipMemcpyAsync(hp, h->hdev.p, (size_t)2 * nb * sizeof(cplx), hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
            // ||M^-1 A g|| <= 1e-12 ||g||: g is a null vector to rounding, u^ would be noise -- no deflation for that column
            std::vector<cplx> un(nb);
            for (int b = 0; b < nb; ++b) {
                unorm[b] = (hp[b].x > 1e-12 * hp[nb + b].x && hp[nb + b].x > 0.0) ? hp[b].x : 0.0;
                un[b] = cplx{unorm[b], 0.0};
            }
            h->ydev.upload(un.data(), nb, st);
            launch_scale_inv(h->V.p, h->ydev.p, h->V.p, n, nb, st);          // a column without deflation gets u^ = 0
            HIP_CHECK(hipStreamSynchronize(st));
        }
        if (guess_dir && !deflate) {
            // initial guess x0 = alpha * g, alpha = (M^-1 A g)^H (M^-1 b) / ||M^-1 A g||^2 per column: when the solution is
            // dominated by a known direction (inverse iteration close to an eigenvalue) the Krylov solve only has to
            // produce the small rest
            launch_spmv(A, pc, bt.cps, guess_dir, h->W.p, nullptr, 0.0, nb, MODE_AX, st);
            launch_copy(vcycle(h, bt, 0, h->W.p), h->U.p, vec, st);
            const cplx *zb = vcycle(h, bt, 0, B);
            launch_dots(h->U.p, 0, 1, zb, n, nb, h->partial.p, h->hdev.p, st);
            launch_dots(h->U.p, 0, 1, h->U.p, n, nb, h->partial.p, h->hdev.p + nb, st);
            HIP_CHECK(hipMemcpyAsync(hp, h->hdev.p, (size_t)2 * nb * sizeof(cplx), hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
            std::vector<cplx> al(nb);
            for (int b = 0; b < nb; ++b) {
                const double den = hp[nb + b].x;
                al[b] = den > 0.0 ? cplx{hp[b].x / den, hp[b].y / den} : cplx{0.0, 0.0};
            }
            h->ydev.upload(al.data(), nb, st);
            launch_lincomb(guess_dir, 0, 1, h->ydev.p, X, n, nb, st);
            HIP_CHECK(hipStreamSynchronize(st));
            first = false;
        }
        while (true) {
            // (with a guess direction the buffers of M^-1 b have been used again)
            cplx *const z0 = !first ? residual() : guess_dir ? vcycle(h, bt, 0, B) : zb0;
            first = false;
            if (deflate) {                                   // r0 <- P r0, beta0 = u^H r0
                launch_dots(h->V.p, 0, 1, z0, n, nb, h->partial.p, h->hdev.p + nb, st);
                launch_axpy_neg(h->V.p, 0, 1, h->hdev.p + nb, z0, n, nb, st);
            }
            launch_norms(z0, n, nb, h->partial.p, h->hdev.p, st);
            HIP_CHECK(hipMemcpyAsync(hp, h->hdev.p, (size_t)2 * nb * sizeof(cplx), hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
            if (deflate) for (int b = 0; b < nb; ++b) beta0[b] = zc(hp[nb + b].x, hp[nb + b].y);
            if (drop_bad_guess()) continue;
            const bool all_done = cycle_start([&](int b) {
                if (!done[b]) {
                    const double est = hist[b].empty() ? -1.0 : hist[b].back();
                    if (drift_mode && drift_ref[b] > 0.0 && relres[b] > 0.5 * drift_ref[b]) { stalled[b] = 1; done[b] = 1; }   // a 5-step cycle lies behind this column
                    else if (est >= 0.0 && est <= tol && relres[b] > 50.0 * est) drift_mode = true;
                }
                drift_ref[b] = relres[b];
            });
            if (gmres_env().debug > 1) {
                double rmax = 0.0, emax = 0.0;
                for (int b = 0; b < nb; ++b) { rmax = std::max(rmax, relres[b]); if (!hist[b].empty()) emax = std::max(emax, hist[b].back()); }
                fprintf(stderr, "[gmres]   cycle start at %d steps: true relres max %.2e (last estimate %.2e)\n", total_it, rmax, emax);
            }
            if (all_done || total_it >= maxit || nan_seen) {
                // the projected residual is small, but its u^ component (beta0) has not been cancelled yet for THIS residual:
                // x += (beta0/||u||) g.  (When the right-hand side lies along M^-1 A g -- an Arnoldi step started from an
                // eigenvector -- that is the whole solution.)
                if (deflate && !nan_seen) add_alpha_g(beta0);
                break;
            }
            launch_scale_inv(z0, h->hdev.p, h->V.p + (size_t)off * vec, n, nb, st);     // V0 = M^-1 r / beta
            if (lazy) {                                      // slots 0..off hold unit vectors
                for (int i = 0; i <= off; ++i) std::fill(sv[i].begin(), sv[i].end(), 1.0);
                std::vector<cplx> ones((size_t)(off + 1) * nb, cplx{1.0, 0.0});
                h->vsq.upload(ones.data(), ones.size(), st);
                HIP_CHECK(hipStreamSynchronize(st));
            }
            if (use_mask && nb >= 8) {
                set_mask([&](int b) { return !done[b]; });
                mk = h->cmask.p;
            }
            cs.clear();
            for (int b = 0; b < nb; ++b) cs.emplace_back(m, pair_cfg, hp[b].x, done[b]);
            int j = 0;
            const int m_cycle = drift_mode ? std::min(m, 5) : m;
            while (j < m_cycle && total_it < maxit) {
                if (pair_cfg && j >= pair_min && j + 2 <= m_cycle && total_it + 2 <= maxit) {
                    pair_step(j);
                    j += 2;
                } else {
                    single_step(j);
                    ++j;
                }
                bool all_conv = true;
                for (int b = 0; b < nb; ++b) all_conv = all_conv && cs[b].conv;
                if (all_conv || nan_seen) break;
                if (mk) set_mask([&](int b) { return !cs[b].conv; });
            }
            mk = nullptr;
            // y = R^{-1} g per column, zero-padded to j steps;  x += V y
            const int ju = std::min(j, m);
            std::vector<cplx> y((size_t)std::max(ju, 1) * nb, cplx{0.0, 0.0});
            for (int b = 0; b < nb; ++b) {
                const std::vector<zc> yy = cs[b].back_substitute();
                for (int i = 0; i < cs[b].steps; ++i) {
                    const double f = lazy ? sv[off + i][b] : 1.0;                // x += sum_i y_i s_i V^_i
                    y[(size_t)i * nb + b] = cplx{f * yy[i].real(), f * yy[i].imag()};
                }
            }
            if (ju > 0) {
                h->ydev.upload(y.data(), (size_t)ju * nb, st);
                launch_lincomb_add(h->V.p + (size_t)off * vec, vec, ju, h->ydev.p, X, n, nb, st);      // x += V y in one pass over x
                HIP_CHECK(hipStreamSynchronize(st));       // y is a stack vector
            }
            if (nan_seen) break;
            if (converged_by_estimate(j)) {
                if (deflate) {
                    std::vector<zc> num(beta0);
                    for (int b = 0; b < nb; ++b)
                        for (int i = 0; i < cs[b].steps; ++i) num[b] -= zc(y[(size_t)i * nb + b].x, y[(size_t)i * nb + b].y) * cs[b].cdef[i];
                    add_alpha_g(num);
                }
                break;
            }
        }
        return finish(info, [&]() {
            double r0max = 0.0;
            for (int b = 0; b < nb; ++b) if (!hist[b].empty()) r0max = std::max(r0max, hist[b][0]);
            fprintf(stderr, "[gmres] nb=%d x0=%d lockstep_its=%d first-step relres max=%.2e tol=%.1e %s%.1f ms\n", nb, (int)have_x0, total_it, r0max,
                    tol, pair_cfg ? "pair " : (deflate ? "deflated " : ""), (now_s() - t0) * 1e3);
        });
    }
};

// returns the number of lock-step iterations
static int gmres(wae_family *h, const Batch &bt, const cplx *B, cplx *X, double tol, int maxit, wae_solve_info *info,
                 const cplx *guess_dir = nullptr, bool have_x0 = false, double *relres_out = nullptr) {
    Gmres s{h, bt, B, X, guess_dir, tol, maxit, have_x0, relres_out};
    // wide batches without a guess direction on the unnormalised basis: the recurrence with its bookkeeping on the device
    const bool device = gmres_env().device && s.lazy && !guess_dir && s.nb > 8 && s.nb <= 256;
    return device ? s.run_device(info) : s.run_host(info);
}

// ----------------------------------------------------------------------------------------------------
// helpers
// ----------------------------------------------------------------------------------------------------
static int info_code(wae_solve_info &i) {   // also clears the internal stagnation marker bit

    const bool stag = (i.levels & (1 << 16)) != 0;
    i.levels &= 0xFFFF;
    if (i.n_unconverged > 0) return stag ? WAE_WARN_STAGNATION : WAE_WARN_MAXITER;
    return WAE_OK;
}
// the wae_solve_info of one public call: zeroed, timed from here, handed to the caller with the call's return code
struct CallInfo {
    wae_solve_info li{};
    double t0 = now_s();
    int finish(wae_solve_info *out) {
        li.seconds = now_s() - t0;
        const int rc = info_code(li);
        if (out) *out = li;
        return rc;
    }
};

// ----------------------------------------------------------------------------------------------------
// C ABI
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
    if (R.Vi.n < vecl) R.Vi.alloc(vecl);
    HIP_CHECK(hipMemcpyAsync(R.Vi.p, Vinter, vecl * sizeof(cplx), hipMemcpyDeviceToDevice, h->stream));
    R.vi_valid = true;
    if (R.hb.n < (size_t)4 * (cap + 4) * l) R.hb.alloc((size_t)4 * (cap + 4) * l);
    if (R.alpha.n < (size_t)l) R.alpha.alloc(l);
    if (R.alpha2.n < (size_t)cap * l) R.alpha2.alloc((size_t)cap * l);
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

// ----------------------------------------------------------------------------------------------------
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

static void ensure(DevBuf<cplx> &b, size_t n) { if (b.n < n) b.alloc(n); }

int wae_spmv_sum_cols(wae_family *h, const double *coeffs, int32_t ncoef, const double *X, double *Y, int32_t r, int32_t op) {
    return guarded([&]() {
        WAE_REQUIRE(h && r >= 0 && (r == 0 || (coeffs && X && Y)), "bad argument");
        WAE_REQUIRE(op >= 0 && op <= 2, "bad op");
        if (r == 0) return WAE_OK;                                // L(z) * zeros(d, 0): nothing to do (LinOpFam.jl:482-529 returns d x 0)
        WAE_REQUIRE(ncoef == 1 || ncoef == r, "ncoef must be 1 or r");
        HIP_CHECK(hipSetDevice(h->device));
        hipStream_t st = h->stream;
        const size_t cnt = (size_t)h->d * r;
        ensure(h->io_a, cnt); ensure(h->io_b, cnt);
        constexpr int GW = 256;                                   // widest launch (the side-row / long-row scratch is sized for it)
        const int gw = std::min<int>(r, GW);
        DevBuf<cplx> xi, yi;
        xi.alloc((size_t)h->d * gw); yi.alloc((size_t)h->d * gw);
        std::vector<cplx> tab((size_t)ncoef * h->nplanes);
        std::vector<zc> pc;
        for (int s = 0; s < ncoef; ++s) {
            plane_coeffs(h, coeffs + (size_t)s * 2 * h->T, op, pc);
            for (int q = 0; q < h->nplanes; ++q) { const zc c = pc[h->slot_plane[0][q]]; tab[(size_t)s * h->nplanes + q] = cplx{c.real(), c.imag()}; }
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
        xi.release(); yi.release(); pcd.release();
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
            ensure(h->io_a, cnt);
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
                for (int q = 0; q < h->nplanes; ++q) { const zc c = pc[h->slot_plane[0][q]]; tab[(size_t)j * h->nplanes + q] = cplx{c.real(), c.imag()}; }
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
        xi.release(); yi.release(); pcd.release(); nrm.release(); part.release();
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
        ensure(h->io_a, cnt); ensure(h->io_b, (size_t)h->d);
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
        xi.release(); yi.release(); acc.release(); pcd.release();
        return WAE_OK;
    });
}

// solve a chunk of nb columns already on device in interleaved layout
static int solve_chunk(wae_family *h, const Batch &bt, const std::vector<std::vector<zc>> &pcs, const cplx *B, cplx *X, double tol, int maxit,
                       wae_solve_info *info, const cplx *guess_dir = nullptr, bool have_x0 = false) {
    upload_pc(h, pcs);
    dense_setup(h, bt);
    return gmres(h, bt, B, X, tol, maxit, info, guess_dir, have_x0);
}

int wae_solve_guess(wae_family *h, const double *coeffs, int32_t ncoef, const double *B, const double *Gd, double *X, int32_t r, int32_t op,
                    double tol, int32_t maxit, wae_solve_info *info) {
    return guarded([&]() {
        WAE_REQUIRE(h && r >= 0 && (r == 0 || (coeffs && B && X)), "bad argument");
        WAE_REQUIRE(op >= 0 && op <= 2, "bad op");
        if (r == 0) {                                             // L(z) \ zeros(d, 0)
            if (info) std::memset(info, 0, sizeof(*info));
            return WAE_OK;
        }
        WAE_REQUIRE(ncoef == 1 || ncoef == r, "ncoef must be 1 or r");
        require_solver(h);
        HIP_CHECK(hipSetDevice(h->device));
        hipStream_t st = h->stream;
        CallInfo ci;
        const int64_t d = h->d;
        const size_t cnt = (size_t)d * r;
        ensure(h->io_a, cnt); ensure(h->io_b, cnt);
        HIP_CHECK(hipMemcpyAsync(h->io_a.p, B, cnt * sizeof(cplx), hipMemcpyHostToDevice, st));
        DevBuf<cplx> gcol, gint;
        if (Gd) {
            gcol.alloc(cnt);
            gint.alloc((size_t)d * h->NB);
            HIP_CHECK(hipMemcpyAsync(gcol.p, Gd, cnt * sizeof(cplx), hipMemcpyHostToDevice, st));
        }
        for (int c0 = 0; c0 < r; c0 += h->NB) {
            const int nb = std::min(h->NB, r - c0);
            Batch bt;
            bt.nb = nb; bt.op = op;
            std::vector<std::vector<zc>> pcs;
            if (ncoef == 1) {
                bt.cps = nb; bt.nsys = 1;
                pcs.resize(1);
                plane_coeffs(h, coeffs, op, pcs[0]);
            } else {
                bt.cps = 1; bt.nsys = nb;
                pcs.resize(nb);
                for (int b = 0; b < nb; ++b) plane_coeffs(h, coeffs + (size_t)(c0 + b) * 2 * h->T, op, pcs[b]);
            }
            launch_colmajor_to_inter(h->io_a.p + (size_t)c0 * d, d, nb, h->Bs.p, nb, st, h->perm());
            if (Gd) launch_colmajor_to_inter(gcol.p + (size_t)c0 * d, d, nb, gint.p, nb, st, h->perm());
            solve_chunk(h, bt, pcs, h->Bs.p, h->Xs.p, tol, maxit, &ci.li, Gd ? gint.p : nullptr);
            launch_inter_to_colmajor(h->Xs.p, nb, d, nb, h->io_b.p + (size_t)c0 * d, st, h->perm());
        }
        HIP_CHECK(hipMemcpyAsync(X, h->io_b.p, cnt * sizeof(cplx), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        return ci.finish(info);
    });
}

int wae_solve(wae_family *h, const double *coeffs, int32_t ncoef, const double *B, double *X, int32_t r, int32_t op, double tol, int32_t maxit,
              wae_solve_info *info) {
    return wae_solve_guess(h, coeffs, ncoef, B, nullptr, X, r, op, tol, maxit, info);
}

// ----------------------------------------------------------------------------------------------------
// forced response: a frequency sweep that stays in HBM (kernels: forced.hip)
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
            Batch bt;
            bt.nb = nb; bt.cps = 1; bt.nsys = nb; bt.op = WAE_OP_N;          // one coefficient set per column, as wae_solve with ncoef == r
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
        if (p.new_basis && p.keep == BeynPass::into_basis && h->rbQ.n < vecl * (size_t)p.nbasis) h->rbQ.alloc(vecl * (size_t)p.nbasis);
        WAE_REQUIRE(h->rbQ.n >= vecl * (size_t)p.nbasis, "no snapshots stored in the handle: run mode 0 first");
        Q = h->rbQ.p;
    }
    ensure(h->io_a, vecl);
    if (p.V) {
        HIP_CHECK(hipMemcpyAsync(h->io_a.p, p.V, vecl * sizeof(cplx), hipMemcpyHostToDevice, st));
    } else {                                     // the probe matrix of the basis this handle started is still in HBM
        WAE_REQUIRE(R.vi_valid && R.l == l && R.Vi.n >= vecl, "V may be NULL only in mode 2 after a mode 0/1 call with the same l on this handle");
        launch_inter_to_colmajor(R.Vi.p, l, d, l, h->io_a.p, st, h->perm());      // (io_a holds the caller's numbering, like an uploaded V)
    }
    if (p.guess && R.ycoef.n < (size_t)std::max(p.nbasis, 1) * h->NB) R.ycoef.alloc((size_t)std::max(p.nbasis, 1) * h->NB);
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
    // WAE_RB_DOUBLING=0 restores full chunks, WAE_RB_C0COLS sets the starting width (4, 8, 32 measured: slower).
    static const int doubling = getenv("WAE_RB_DOUBLING") ? atoi(getenv("WAE_RB_DOUBLING")) : 1;
    static const int c0cols = getenv("WAE_RB_C0COLS") ? std::max(1, atoi(getenv("WAE_RB_C0COLS"))) : 16;
    struct LightOff { bool &on; ~LightOff() { on = false; } } light_off{h->vc_light};      // set before every solve; off again however the loop ends
    for (int cg = 0; cg < l; cg += h->NB) {      // probe columns in groups of <= NB (one group whenever there is a store)
        const int lg = std::min(h->NB, l - cg);
        const int spc = std::max(1, h->NB / lg);   // systems per chunk
        const int c0 = doubling ? std::max(1, c0cols / lg) : spc;
        ensure(h->zw_dev, (size_t)2 * spc);
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

// relative Ritz residual |h_{k+1,k}| |y_k| / |theta| of the dominant Ritz pair of the leading k x k block of H (column-major,
// leading dimension ld), by power iteration on the small matrix; +inf when the dominant eigenvalue is not well separated
static double dominant_ritz_residual(const std::vector<zc> &H, int ld, int k) {
    std::vector<zc> y(k, zc(0)), w(k);
    y[0] = 1.0;
    zc theta = 0, prev = 0;
    for (int it = 0; it < 400; ++it) {
        for (int i = 0; i < k; ++i) {
            zc acc = 0;
            for (int j = std::max(0, i - 1); j < k; ++j) acc += H[(size_t)j * ld + i] * y[j];      // Hessenberg: H[i][j] = 0 for i > j+1
            w[i] = acc;
        }
        double nrm = 0.0;
        for (const zc &v : w) nrm += std::norm(v);
        nrm = std::sqrt(nrm);
        if (!(nrm > 0.0)) return INFINITY;
        theta = 0;
        for (int i = 0; i < k; ++i) theta += std::conj(y[i]) * w[i];
        for (int i = 0; i < k; ++i) y[i] = w[i] / nrm;
        if (it > 2 && std::abs(theta - prev) <= 1e-14 * std::abs(theta)) {
            return std::abs(H[(size_t)(k - 1) * ld + k]) * std::abs(y[k - 1]) / std::abs(theta);
        }
        prev = theta;
    }
    return INFINITY;
}

static const cplx *slot_cols_ptr(wae_family *h, int32_t slot, const int32_t *cols, int n, DevBuf<cplx> &stage, hipStream_t st);   // (slots: below)

// The Arnoldi processes behind wae_arnoldi_shiftinvert_batch (start vectors and basis through host memory) and
// wae_arnoldi_shiftinvert_slots (start vectors from a device-resident multivector, basis kept on the device for wae_arnoldi_ritz_to_slot).
// v0_host: d x nsys column-major in the caller's row numbering, or null: then v0_slot / v0_cols name the columns.  V_out null: the
// basis stays in h->arn_EV (h->arn_nsys systems, h->arn_cols vectors each).
static int arnoldi_core(wae_family *h, int32_t nsys, const double *coeffsA, const double *coeffsM, int32_t m, const double *v0_host, int32_t v0_slot,
                        const int32_t *v0_cols, int32_t op, double tol, int32_t maxit, double ritz_tol, double *H_out, double *V_out,
                        wae_solve_info *info) {
    {
        HIP_CHECK(hipSetDevice(h->device));
        hipStream_t st = h->stream;
        CallInfo ci;
        wae_solve_info &li = ci.li;
        const int64_t d = h->d;
        const int T = h->T;
        const size_t vec = (size_t)d * nsys;
        // (work space of the family, grown on demand and kept: a hipMalloc / hipFree pair of 0.9 GB per call at 1M DoF and 8 systems otherwise)
        DevBuf<cplx> &EV = h->arn_EV, &t = h->arn_t, &pcM = h->arn_pcM, &hcol = h->arn_hcol, &stage = h->arn_stage, &gdir = h->arn_gdir;
        h->arn_nsys = 0; h->arn_cols = 0;
        ensure(EV, vec * (m + 1));
        ensure(t, vec);
        if (m > 1) ensure(gdir, vec);
        ensure(stage, vec);
        ensure(hcol, (size_t)2 * (m + 2) * nsys);
        // per-system plane coefficients of M (level-0 slot order) and of A (all levels)
        std::vector<cplx> tab((size_t)nsys * h->nplanes);
        std::vector<zc> pcm;
        std::vector<std::vector<zc>> pcs(nsys);
        for (int sy = 0; sy < nsys; ++sy) {
            plane_coeffs(h, coeffsM + (size_t)sy * 2 * T, op, pcm);
            for (int q = 0; q < h->nplanes; ++q) { const zc c = pcm[h->slot_plane[0][q]]; tab[(size_t)sy * h->nplanes + q] = cplx{c.real(), c.imag()}; }
            plane_coeffs(h, coeffsA + (size_t)sy * 2 * T, op, pcs[sy]);
        }
        pcM.upload(tab.data(), tab.size(), st);
        Batch bt;
        bt.nb = nsys; bt.cps = 1; bt.nsys = nsys; bt.op = op;
        upload_pc(h, pcs);
        dense_setup(h, bt);
        std::vector<std::vector<zc>> H(nsys, std::vector<zc>((size_t)(m + 1) * m, zc(0)));
        std::vector<char> dead(nsys, 0);
        // v_0 = v0 / ||v0||, column by column
        if (v0_host) {
            HIP_CHECK(hipMemcpyAsync(stage.p, v0_host, vec * sizeof(cplx), hipMemcpyHostToDevice, st));
            launch_colmajor_to_inter(stage.p, d, nsys, t.p, nsys, st, h->perm());
        } else {                                             // (slot columns are in the library's row numbering already)
            const cplx *S = slot_cols_ptr(h, v0_slot, v0_cols, nsys, stage, st);
            launch_colmajor_to_inter(S, d, nsys, t.p, nsys, st, nullptr);
        }
        launch_norms(t.p, d, nsys, h->partial.p, hcol.p, st);
        launch_scale_inv(t.p, hcol.p, EV.p, d, nsys, st);
        const OpDev Mop = h->ops[0].dev(op);
        std::vector<cplx> hh((size_t)(m + 2) * nsys), al(nsys);
        int done = 0;
        // Relaxed inner tolerance (inexact Arnoldi: Bouras & Fraysse 2005, Simoncini 2005): the solve of step k may be as
        // inexact as tol / (relative Ritz residual after step k-1) without the true residual of the Ritz pair leaving the
        // computed one by more than ~m tol -- the k-th column of H enters the wanted Ritz vector with a weight of that size.
        // Close to an eigenvalue of the NLEVP (residuals 1e-5, 1e-10 after one and two steps) the second and third solves
        // stop at 1e-8 and 1e-3 instead of 1e-12.  Only with the Ritz test on (ritz_tol > 0, where the residuals are
        // evaluated anyway); a tenth of the bound, never looser than 1e-3, never tighter than tol.  WAE_ARNOLDI_RELAX=0: off.
        static const bool relax_on = !(getenv("WAE_ARNOLDI_RELAX") && atoi(getenv("WAE_ARNOLDI_RELAX")) == 0);
        double tol_j = tol;
        // A poor start costs a whole process step at full accuracy: the left process of a Newton step on a non-symmetric family starts from
        // a vector that is not close to the left eigenvector (relative Ritz residual 0.99 after its first step at 1M DoF), that step's
        // solve ran 86 iterations to an estimate of 1e-12 whose recomputed residual stood at 2.5e-3 -- the deflation direction, the start
        // itself, was useless -- and all it gave was a better direction.  The quality of a start is known beforehand:
        // q = ||M^-1 A v0|| / ||v0|| (one product, one V-cycle; M^-1 A is close to the identity away from the operator's near-null space,
        // so q ~ 1e-6 for an eigenvector estimate of that accuracy and ~ 1 for an arbitrary vector).  Columns with q > 0.1 are replaced by
        // one step of inverse iteration from them, solved to 1e-3 only: the process then starts from a vector whose own step is worth its
        // accuracy.  Only with the Ritz test on (the Newton-type solvers); WAE_ARNOLDI_PRESTEP=0: off.
        static const bool prestep_on = !(getenv("WAE_ARNOLDI_PRESTEP") && atoi(getenv("WAE_ARNOLDI_PRESTEP")) == 0);
        if (prestep_on && ritz_tol > 0.0 && m > 1 && h->ops.size() > 1 && tol < 1e-3) {
            launch_spmv(h->ops[0].dev(op), pc_level(h, 0), bt.cps, EV.p, h->W.p, nullptr, 0.0, nsys, MODE_AX, st);
            launch_norms(vcycle(h, bt, 0, h->W.p), d, nsys, h->partial.p, hcol.p, st);
            HIP_CHECK(hipMemcpyAsync(hh.data(), hcol.p, (size_t)nsys * sizeof(cplx), hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
            std::vector<cplx> keep(nsys), take(nsys);
            int npoor = 0;
            for (int sy = 0; sy < nsys; ++sy) {
                const bool poor = hh[sy].x > 0.1;
                npoor += poor;
                keep[sy] = cplx{poor ? 0.0 : 1.0, 0.0};
                take[sy] = cplx{poor ? 1.0 : 0.0, 0.0};
            }
            if (getenv("WAE_GMRES_DEBUG")) {
                double qmax = 0.0;
                for (int sy = 0; sy < nsys; ++sy) qmax = std::max(qmax, hh[sy].x);
                fprintf(stderr, "[arnoldi] start quality max %.2e: %d of %d columns take a step of inverse iteration first\n", qmax, npoor, nsys);
                if (atoi(getenv("WAE_GMRES_DEBUG")) > 2) { fprintf(stderr, "[arnoldi]   q ="); for (int sy = 0; sy < nsys; ++sy) fprintf(stderr, " %.2e", hh[sy].x); fprintf(stderr, "\n"); }
            }
            if (npoor) {
                wae_solve_info lpre;
                memset(&lpre, 0, sizeof(lpre));
                launch_spmv(Mop, pcM.p, 1, EV.p, t.p, nullptr, 0.0, nsys, MODE_AX, st);
                // (no deflation direction: the start is the only candidate and deflating a vector that is NOT near the null space costs
                // iterations -- 93 against 50 at 1M DoF; the restarted wide recurrence stalls on these systems: 161 steps)
                gmres(h, bt, t.p, h->Xs.p, 1e-3, maxit, &lpre, nullptr);
                li.iters_max = std::max(li.iters_max, lpre.iters_max);
                li.iters_total += lpre.iters_total;
                launch_norms(h->Xs.p, d, nsys, h->partial.p, hcol.p, st);
                launch_scale_inv(h->Xs.p, hcol.p, t.p, d, nsys, st);                 // t = the normalised iterates
                h->ydev.upload(keep.data(), nsys, st);
                launch_mask_cols(EV.p, h->ydev.p, d, nsys, st);
                HIP_CHECK(hipStreamSynchronize(st));                                 // (ydev is read by the kernel: before the next upload)
                h->ydev.upload(take.data(), nsys, st);
                launch_mask_cols(t.p, h->ydev.p, d, nsys, st);
                launch_add(t.p, EV.p, vec, st);
                HIP_CHECK(hipStreamSynchronize(st));
            }
        }
        for (int j = 0; j < m; ++j) {
            launch_spmv(Mop, pcM.p, 1, EV.p + (size_t)j * vec, t.p, nullptr, 0.0, nsys, MODE_AX, st);
            // the start vector is the caller's estimate of the wanted eigenvector: deflated out of the first solve of the process; the
            // later solves deflate the (normalised) solution of the first one -- one step of inverse iteration closer to that
            // eigenvector, which matters when the start is poor (the left process of a Newton step starts from conj(v): for a spinning
            // mode of an annulus that is the OTHER mode of the pair)
            gmres(h, bt, t.p, h->Xs.p, tol_j, maxit, &li, j == 0 ? EV.p : gdir.p);
            cplx *w = h->Xs.p;
            if (j == 0 && m > 1) {
                launch_norms(w, d, nsys, h->partial.p, hcol.p, st);
                launch_scale_inv(w, hcol.p, gdir.p, d, nsys, st);
            }
            std::vector<std::vector<zc>> hc(nsys, std::vector<zc>(j + 2, zc(0)));
            for (int pass = 0; pass < 2; ++pass) {               // classical Gram-Schmidt, two passes, per column
                launch_dots(EV.p, vec, j + 1, w, d, nsys, h->partial.p, hcol.p, st);
                launch_axpy_neg(EV.p, vec, j + 1, hcol.p, w, d, nsys, st);
                HIP_CHECK(hipMemcpyAsync(hh.data(), hcol.p, (size_t)(j + 1) * nsys * sizeof(cplx), hipMemcpyDeviceToHost, st));
                HIP_CHECK(hipStreamSynchronize(st));
                for (int sy = 0; sy < nsys; ++sy)
                    for (int i = 0; i <= j; ++i) hc[sy][i] += zc(hh[(size_t)i * nsys + sy].x, hh[(size_t)i * nsys + sy].y);
            }
            launch_norms(w, d, nsys, h->partial.p, hcol.p, st);
            HIP_CHECK(hipMemcpyAsync(hh.data(), hcol.p, (size_t)nsys * sizeof(cplx), hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
            done = j + 1;
            bool any_alive = false;
            for (int sy = 0; sy < nsys; ++sy) {
                double scale = 0.0;
                for (int i = 0; i <= j; ++i) scale = std::max(scale, std::abs(hc[sy][i]));
                const bool brk = dead[sy] || !(hh[sy].x > 1e-14 * scale);    // invariant subspace: this column stops here
                hc[sy][j + 1] = brk ? zc(0) : zc(hh[sy].x);
                if (!dead[sy]) for (int i = 0; i <= j + 1; ++i) H[sy][(size_t)j * (m + 1) + i] = hc[sy][i];
                if (brk) dead[sy] = 1;
                al[sy] = brk ? cplx{0.0, 0.0} : cplx{hh[sy].x, 0.0};
                any_alive = any_alive || !brk;
            }
            if (!any_alive) {                                    // (column j + 1 is returned, and counted in arn_cols: not what an earlier call left there)
                launch_fill_zero(EV.p + (size_t)(j + 1) * vec, vec, st);
                break;
            }
            h->ydev.upload(al.data(), nsys, st);
            launch_scale_inv(w, h->ydev.p, EV.p + (size_t)(j + 1) * vec, d, nsys, st);
            HIP_CHECK(hipStreamSynchronize(st));
            // early exit: the dominant Ritz pair of every live process has converged (close to an eigenvalue of the NLEVP
            // two or three steps do; a fixed m = 6 spent twice the solves)
            if (ritz_tol > 0.0 && j + 1 < m) {
                double worst = 0.0;
                for (int sy = 0; sy < nsys; ++sy)
                    if (!dead[sy]) worst = std::max(worst, dominant_ritz_residual(H[sy], m + 1, j + 1));
                if (getenv("WAE_GMRES_DEBUG")) fprintf(stderr, "[arnoldi] step %d worst relative Ritz residual %.2e\n", j + 1, worst);
                if (worst <= ritz_tol) break;
                if (relax_on) tol_j = std::max(tol, std::min(1e-3, 0.1 * tol / worst));          // (worst = inf: tol)
            }
        }
        // V_out[sys] = d x (m+1) column-major; only the columns the processes produced are written (steps taken + 1): the rest
        // of the caller's buffer is left as it was (the H columns beyond them are zero) -- at 1M DoF and 8 systems every column is
        // 128 MB of host memory to touch
        if (V_out) {
            for (int j = 0; j <= std::min(done, m); ++j) {
                launch_inter_to_colmajor(EV.p + (size_t)j * vec, nsys, d, nsys, stage.p, st, h->perm());
                for (int sy = 0; sy < nsys; ++sy)
                    HIP_CHECK(hipMemcpyAsync(V_out + ((size_t)sy * (m + 1) + j) * d * 2, stage.p + (size_t)sy * d, (size_t)d * sizeof(cplx),
                                             hipMemcpyDeviceToHost, st));
                HIP_CHECK(hipStreamSynchronize(st));
            }
            if (done < m && !(ritz_tol > 0.0))               // every process ended in an invariant subspace: the documented zeros
                for (int sy = 0; sy < nsys; ++sy)
                    memset(V_out + ((size_t)sy * (m + 1) + done + 1) * d * 2, 0, (size_t)(m - done) * d * sizeof(cplx));
        } else {
            h->arn_nsys = nsys;
            h->arn_cols = std::min(done, m) + 1;
        }
        for (int sy = 0; sy < nsys; ++sy) memcpy(H_out + (size_t)sy * (m + 1) * m * 2, H[sy].data(), H[sy].size() * sizeof(zc));
        return ci.finish(info);
    }
}

int wae_arnoldi_shiftinvert_batch(wae_family *h, int32_t nsys, const double *coeffsA, const double *coeffsM, int32_t m, const double *v0, int32_t op,
                                  double tol, int32_t maxit, double ritz_tol, double *H_out, double *V_out, wae_solve_info *info) {
    return guarded([&]() {
        WAE_REQUIRE(h && nsys >= 1 && coeffsA && coeffsM && v0 && H_out && V_out && m >= 1 && m <= 256, "bad argument");
        WAE_REQUIRE(op == WAE_OP_N || op == WAE_OP_C || op == WAE_OP_T, "bad op");
        require_solver(h);
        WAE_REQUIRE(nsys <= h->NB, "more systems than the solver batch width");
        return arnoldi_core(h, nsys, coeffsA, coeffsM, m, v0, -1, nullptr, op, tol, maxit, ritz_tol, H_out, V_out, info);
    });
}

int wae_arnoldi_shiftinvert(wae_family *h, const double *coeffsA, const double *coeffsM, int32_t m, const double *v0, int32_t op, double tol,
                            int32_t maxit, double *H_out, double *V_out, wae_solve_info *info) {
    return wae_arnoldi_shiftinvert_batch(h, 1, coeffsA, coeffsM, m, v0, op, tol, maxit, 0.0, H_out, V_out, info);
}

// ----------------------------------------------------------------------------------------------------
// Device-resident multivectors ("slots").  The Newton-type solvers iterate on a handful of vectors per start value (right and left
// eigenvector estimates, the Ritz vectors of the step): with the processes' inputs and outputs in host memory a Householder step of 8
// start values at 1M DoF moved 2 GB over PCIe into freshly touched pages and spent as long in host copies as the GPU spent computing
// (45 % idle in the kernel trace).  A slot holds d x ncols in the library's row numbering; the calls below read and write slot columns
// in place of host arrays, so that an iteration touches host memory once at its start and once at its end.
// ----------------------------------------------------------------------------------------------------
static wae_family::Slot &slot_ref(wae_family *h, int32_t slot) {
    WAE_REQUIRE(slot >= 0 && slot < WAE_NSLOTS, "slot index out of range");
    return h->slots[slot];
}
static cplx *slot_col(wae_family *h, int32_t slot, int32_t col) {
    wae_family::Slot &S = slot_ref(h, slot);
    WAE_REQUIRE(S.ncols > 0, "slot is empty");
    WAE_REQUIRE(col >= 0 && col < S.ncols, "slot column out of range");
    return S.buf.p + (size_t)col * h->d;
}
// n columns of a slot as one contiguous column-major block: the slot's own memory if they are consecutive, a copy in `stage` otherwise
static const cplx *slot_cols_ptr(wae_family *h, int32_t slot, const int32_t *cols, int n, DevBuf<cplx> &stage, hipStream_t st) {
    WAE_REQUIRE(cols && n >= 1, "bad argument");
    bool consecutive = true;
    for (int i = 0; i < n; ++i) { (void)slot_col(h, slot, cols[i]); consecutive = consecutive && cols[i] == cols[0] + i; }
    if (consecutive) return slot_col(h, slot, cols[0]);
    ensure(stage, (size_t)n * h->d);
    for (int i = 0; i < n; ++i) launch_copy(slot_col(h, slot, cols[i]), stage.p + (size_t)i * h->d, (size_t)h->d, st);
    return stage.p;
}

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
            ensure(h->io_a, (size_t)d * ncols);
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
        ensure(h->io_b, (size_t)d * ncols);
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
        ensure(h->io_b, 3 * vec);
        cplx *Bi = h->io_b.p, *ABi = Bi + vec, *Ai = ABi + vec;
        launch_colmajor_to_inter(slot_cols_ptr(h, b_slot, b_cols, n, h->io_a, st), d, n, Bi, n, st, nullptr);
        launch_colmajor_to_inter(slot_cols_ptr(h, a_slot, a_cols, n, h->io_a, st), d, n, Ai, n, st, nullptr);
        std::vector<cplx> tab((size_t)n * h->nplanes);
        std::vector<zc> pc;
        for (int i = 0; i < n; ++i) {
            plane_coeffs(h, coeffs + (size_t)i * 2 * T, op, pc);
            for (int q = 0; q < h->nplanes; ++q) { const zc c = pc[h->slot_plane[0][q]]; tab[(size_t)i * h->nplanes + q] = cplx{c.real(), c.imag()}; }
        }
        h->pt_pcd.upload(tab.data(), tab.size(), st);
        launch_spmv(h->ops[0].dev(op), h->pt_pcd.p, 1, Bi, ABi, nullptr, 0.0, n, MODE_AX, st);
        ensure(h->partial, (size_t)1024 * 32 * std::max(n, 8));      // (launch_dots: DOT_BLOCKS x vectors x columns; the solver set-up allocates more)
        ensure(h->pt_Gd, (size_t)n);
        launch_dots(Ai, 0, 1, ABi, d, n, h->partial.p, h->pt_Gd.p, st);
        std::vector<cplx> r(n);
        HIP_CHECK(hipMemcpyAsync(r.data(), h->pt_Gd.p, (size_t)n * sizeof(cplx), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        for (int i = 0; i < n; ++i) { out[2 * i] = r[i].x; out[2 * i + 1] = r[i].y; }
        return WAE_OK;
    });
}

int wae_arnoldi_shiftinvert_slots(wae_family *h, int32_t nsys, const double *coeffsA, const double *coeffsM, int32_t m, int32_t v0_slot,
                                  const int32_t *v0_cols, int32_t op, double tol, int32_t maxit, double ritz_tol, double *H_out, wae_solve_info *info) {
    return guarded([&]() {
        WAE_REQUIRE(h && nsys >= 1 && coeffsA && coeffsM && v0_cols && H_out && m >= 1 && m <= 256, "bad argument");
        WAE_REQUIRE(op == WAE_OP_N || op == WAE_OP_C || op == WAE_OP_T, "bad op");
        require_solver(h);
        WAE_REQUIRE(nsys <= h->NB, "more systems than the solver batch width");
        for (int i = 0; i < nsys; ++i) (void)slot_col(h, v0_slot, v0_cols[i]);
        return arnoldi_core(h, nsys, coeffsA, coeffsM, m, nullptr, v0_slot, v0_cols, op, tol, maxit, ritz_tol, H_out, nullptr, info);
    });
}

int wae_arnoldi_ritz_to_slot(wae_family *h, int32_t nsys, int32_t ny, const double *y, int32_t dst_slot, const int32_t *dst_cols, int32_t normalise) {
    return guarded([&]() {
        WAE_REQUIRE(h && nsys >= 1 && ny >= 1 && y && dst_cols, "bad argument");
        WAE_REQUIRE(h->arn_nsys == nsys && ny <= h->arn_cols, "no Arnoldi basis of that shape on the device (wae_arnoldi_shiftinvert_slots first)");
        HIP_CHECK(hipSetDevice(h->device));
        hipStream_t st = h->stream;
        const int64_t d = h->d;
        const size_t vec = (size_t)d * nsys;
        for (int i = 0; i < nsys; ++i) (void)slot_col(h, dst_slot, dst_cols[i]);
        std::vector<cplx> yc((size_t)ny * nsys);
        for (int sy = 0; sy < nsys; ++sy)
            for (int j = 0; j < ny; ++j) yc[(size_t)j * nsys + sy] = cplx{y[((size_t)sy * ny + j) * 2], y[((size_t)sy * ny + j) * 2 + 1]};
        ensure(h->arn_hcol, yc.size() + (size_t)nsys);
        HIP_CHECK(hipMemcpyAsync(h->arn_hcol.p, yc.data(), yc.size() * sizeof(cplx), hipMemcpyHostToDevice, st));
        launch_lincomb(h->arn_EV.p, vec, ny, h->arn_hcol.p, h->arn_t.p, d, nsys, st);
        if (normalise) {
            launch_norms(h->arn_t.p, d, nsys, h->partial.p, h->arn_hcol.p + yc.size(), st);
            launch_scale_inv(h->arn_t.p, h->arn_hcol.p + yc.size(), h->arn_t.p, d, nsys, st);
        }
        launch_inter_to_colmajor(h->arn_t.p, nsys, d, nsys, h->arn_stage.p, st, nullptr);
        for (int i = 0; i < nsys; ++i) launch_copy(h->arn_stage.p + (size_t)i * d, slot_col(h, dst_slot, dst_cols[i]), (size_t)d, st);
        HIP_CHECK(hipStreamSynchronize(st));                 // (yc is a stack vector)
        return WAE_OK;
    });
}

// ----------------------------------------------------------------------------------------------------
// Adjoint perturbation: the one recurrence behind wae_perturb / wae_perturb_slots (nsys = 1) and wae_perturb_batch /
// wae_perturb_batch_slots, for nsys eigenpairs in lock-step.  Every vector of the batch is an interleaved block [row][system] of
// leading dimension nb, the series is N+1 such blocks.
// Per order: the partition weights of every system on the host (they need lambda_1..k-1 of that system), ONE tall-skinny product, ONE
// multi-input SpMV per plane pass, ONE inner product with the left vectors, ONE read-back of the nsys numerators -- the only host
// synchronisation of an order outside the solve --, ONE fused right-hand side, ONE lock-step solve, the projection dots and ONE fused
// projection update.  All device work space is carved out of ONE buffer the entry point hands in: a buffer of its own, released on
// return (the batched calls), or the family's grow-only pt_ws (the single-pair calls: a Newton step of the Householder iteration makes
// one per start value, and a dozen hipMalloc / hipFree pairs per call showed up there).
// ----------------------------------------------------------------------------------------------------
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
    ensure(ws, total);
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
            for (int q = 0; q < npl; ++q) {
                if (i < n) { const zc c = pc[h->slot_plane[0][q]]; tab[(size_t)i * npl + q] = cplx{c.real(), c.imag()}; }
                else tab[(size_t)i * npl + q] = tab[q];
            }
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
        Batch bt;
        bt.nb = nb; bt.op = WAE_OP_N;
        if (norm_mode == 2) {                                       // perturbation.jl:493-494
            bt.cps = nb; bt.nsys = 1;
            std::vector<std::vector<zc>> pcs(1);
            plane_coeffs(h, coeffsY, WAE_OP_N, pcs[0]);
            solve_chunk(h, bt, pcs, wl, tmp, tol, maxit, &li);      // v0Adj = Y \ v0Adj
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
        bt.cps = 1; bt.nsys = nb;
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

int wae_perturb(wae_family *h, const double *coeff_table, int32_t N, const double *v0, const double *v0adj, int32_t norm_mode, const double *coeffsY,
                double tol, int32_t maxit, double *lambda_out, double *v_out, wae_solve_info *info) {
    return guarded([&]() {
        WAE_REQUIRE(h && coeff_table && v0 && v0adj && lambda_out && v_out && N >= 0 && N <= 200, "bad argument");
        perturb_batch_check(h, 1, coeff_table, N, lambda_out);
        const size_t d = (size_t)h->d;
        ensure(h->io_a, 2 * d);
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

int wae_bench_spmv(wae_family *h, const double *coeffs, int32_t r, int32_t reps, double *ms_out) {
    return guarded([&]() {
        WAE_REQUIRE(h && coeffs && r > 0 && reps > 0 && ms_out, "bad argument");
        HIP_CHECK(hipSetDevice(h->device));
        hipStream_t st = h->stream;
        const size_t cnt = (size_t)h->d * r;
        DevBuf<cplx> x, y, pcd;
        x.alloc(cnt); y.alloc(cnt);
        std::vector<cplx> hx(cnt);
        uint64_t s = 0x9E3779B97F4A7C15ull;
        for (size_t i = 0; i < cnt; ++i) {
            s ^= s << 13; s ^= s >> 7; s ^= s << 17;
            hx[i].x = (double)(s & 0xFFFFF) / 524288.0 - 1.0;
            hx[i].y = (double)((s >> 20) & 0xFFFFF) / 524288.0 - 1.0;
        }
        HIP_CHECK(hipMemcpyAsync(x.p, hx.data(), cnt * sizeof(cplx), hipMemcpyHostToDevice, st));
        std::vector<zc> pc;
        plane_coeffs(h, coeffs, WAE_OP_N, pc);
        // WAE_BENCH_CPS = columns per system (diagnostic: 1, 2 or 4 is what a rank of a multi-GPU pass sees: its share of the
        // probe columns of every system); default: one system, all columns
        const int cps = getenv("WAE_BENCH_CPS") ? std::max(1, atoi(getenv("WAE_BENCH_CPS"))) : (1 << 30);
        const int nsys = cps >= r ? 1 : (r + cps - 1) / cps;
        std::vector<cplx> tab((size_t)h->nplanes * nsys);
        for (int sidx = 0; sidx < nsys; ++sidx)
            for (int q = 0; q < h->nplanes; ++q) { const zc c = pc[h->slot_plane[0][q]]; tab[(size_t)sidx * h->nplanes + q] = cplx{c.real(), c.imag()}; }
        pcd.upload(tab.data(), tab.size(), st);
        const OpDev A = h->ops[0].dev(WAE_OP_N);
        // WAE_BENCH_MODE (diagnostic): the fused form timed -- 0 A X (default), 1 residual, 2 Jacobi sweep, 6 product + first sweep
        const int bmode = getenv("WAE_BENCH_MODE") ? atoi(getenv("WAE_BENCH_MODE")) : MODE_AX;
        DevBuf<cplx> bb;
        if (bmode != MODE_AX) { bb.alloc(cnt); HIP_CHECK(hipMemcpyAsync(bb.p, hx.data(), cnt * sizeof(cplx), hipMemcpyHostToDevice, st)); }
        auto one = [&]() { launch_spmv(A, pcd.p, cps, x.p, y.p, bmode != MODE_AX ? bb.p : nullptr, 0.8, r, bmode, st); };
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
        *ms_out = (double)ms / reps;
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
        x.release(); y.release(); pcd.release();
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
        if (cmask) {
            cm.alloc((size_t)(r + 7) / 8);
            HIP_CHECK(hipMemcpyAsync(cm.p, cmask, (size_t)(r + 7) / 8, hipMemcpyHostToDevice, st));
        }
        OpDev A;
        int cps = 1 << 30;
        if (which == 0) {
            std::vector<cplx> tab((size_t)ncoef * h->nplanes);
            std::vector<zc> pc;
            for (int s = 0; s < ncoef; ++s) {
                plane_coeffs(h, coeffs + (size_t)s * 2 * h->T, op, pc);
                for (int q = 0; q < h->nplanes; ++q) { const zc c = pc[h->slot_plane[level][q]]; tab[(size_t)s * h->nplanes + q] = cplx{c.real(), c.imag()}; }
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
        if (cmask) {
            cm.alloc((size_t)(r + 7) / 8);
            HIP_CHECK(hipMemcpyAsync(cm.p, cmask, (size_t)(r + 7) / 8, hipMemcpyHostToDevice, st));
        }
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
        Batch bt;                                                   // the batch and the plane tables as wae_solve_guess builds them
        bt.nb = r; bt.op = op;
        bt.cps = ncoef == 1 ? r : 1;
        bt.nsys = ncoef == 1 ? 1 : r;
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
        if (cmask) {
            cm.alloc((size_t)(r + 7) / 8);
            HIP_CHECK(hipMemcpyAsync(cm.p, cmask, (size_t)(r + 7) / 8, hipMemcpyHostToDevice, st));
        }
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
        uint64_t sd = 0x9E3779B97F4A7C15ull;
        for (auto &v : hx) { sd ^= sd << 13; sd ^= sd >> 7; sd ^= sd << 17; v.x = (double)(sd & 0xFFFFF) / 524288.0 - 1.0; v.y = (double)((sd >> 20) & 0xFFFFF) / 524288.0 - 1.0; }
        HIP_CHECK(hipMemcpyAsync(x.p, hx.data(), hx.size() * sizeof(cplx), hipMemcpyHostToDevice, st));
        OpDev A;
        const cplx *pcp = h->one_dev.p;
        int64_t bytes = 2;
        if (which == 0) {
            std::vector<zc> pc;
            plane_coeffs(h, coeffs, WAE_OP_N, pc);
            std::vector<cplx> tab(h->nplanes);
            bytes = 0;
            for (int q = 0; q < h->nplanes; ++q) {
                const zc c = pc[h->slot_plane[level][q]];
                tab[q] = cplx{c.real(), c.imag()};
            }
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
        *ms_out = (double)ms / reps;
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
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
        a.release(); b.release(); c.release();
        return WAE_OK;
    });
}

}   // extern "C"
