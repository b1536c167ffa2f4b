// libwaehip.so -- the solver proper: coefficient tables, the multigrid V-cycle, the penalty polish, the lock-step batched GMRES they
// precondition, and wae_solve / wae_solve_guess.  Host code only (kernels: kernels.hip, vec.hip); what the other solver units use of
// this one is declared in solver.h.
#include <cmath>

#include "solver.h"

// ----------------------------------------------------------------------------------------------------
// coefficient tables
// ----------------------------------------------------------------------------------------------------
void upload_pc(wae_family *h, const std::vector<std::vector<zc>> &pcs) {
    const int nsys = (int)pcs.size();
    const int nl = (int)h->ops.size();
    const size_t per_level = (size_t)nsys * h->nplanes;
    std::vector<cplx> tab(per_level * (nl + 2));
    for (int l = 0; l <= nl + 1; ++l) {                  // blocks nl, nl+1: the penalty block and the penalty rows (own slot orders)
        if (l >= nl && h->n_penalty == 0) break;
        const std::vector<int> &sp = l < nl ? h->slot_plane[l] : (l == nl ? h->pen_slot : h->pen_row_slot);
        for (int s = 0; s < nsys; ++s) slot_coeffs(h, sp, pcs[s], &tab[l * per_level + (size_t)s * h->nplanes]);
    }
    h->pc_stride_level = per_level;
    h->pcdev.upload(tab.data(), tab.size(), h->stream);
    HIP_CHECK(hipStreamSynchronize(h->stream));
}
const cplx *pc_level(const wae_family *h, int l) { return h->pcdev.p + (size_t)l * h->pc_stride_level; }

// ----------------------------------------------------------------------------------------------------
// multigrid V-cycle (all columns in lock-step)
// ----------------------------------------------------------------------------------------------------
void dense_setup(wae_family *h, const Batch &bt) {
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

double pre_weight(const wae_family *h, int l) { return (h->vc_light ? h->jac_w_light : h->jac_w) * h->lvl_scale[(size_t)l]; }

// (have_x0, final_out, cn: solver.h)
cplx *vcycle(wae_family *h, const Batch &bt, int l, const cplx *b, const unsigned char *cm, bool have_x0, cplx *final_out, CycleNorms *cn) {
    const int L = (int)h->ops.size() - 1;
    hipStream_t st = h->stream;
    if (l == L) {
        launch_dense_apply(h->Ainv.p, (int)h->nc, bt.cps, b, h->lx[l].p, bt.nb, st, cm);
        return h->lx[l].p;
    }
    const OpDev A = h->ops[l].dev(bt.op);
    const cplx *pc = pc_level(h, l);
    cplx *x = h->lx[l].p, *t = h->lt[l].p;
    if (!have_x0) launch_jacobi0(A, pc, bt.cps, b, x, pre_weight(h, l), bt.nb, st, cm);
    for (int s = 1; s < h->nsweeps; ++s) {
        launch_spmv(A, pc, bt.cps, x, t, b, pre_weight(h, l), bt.nb, MODE_JAC, st, cm);
        std::swap(x, t);
    }
    // residual -> t, restrict -> lb[l+1]
    launch_spmv(A, pc, bt.cps, x, t, b, 0.0, bt.nb, MODE_RES, st, cm);
    // for op = T/C the transfer operators are unchanged (real): (R A P)^H = R A^H P
    const bool by_tile = h->xfer[l].ft.ready && bt.nb >= 8 && xfer_tiles_on();      // (wae_internal.h XferTiles: level 0, wide batches)
    launch_spmv(h->xfer[l].devR(), h->one_dev.p, 1 << 30, t, h->lb[l + 1].p, nullptr, 0.0, bt.nb, MODE_AX, st, cm);
    const cplx *xc = vcycle(h, bt, l + 1, h->lb[l + 1].p, cm);
    // Post-smoothing on the coarse levels: everywhere but in the projected phase of a contour integral.  A solve that starts from a
    // projected guess (216 of the 256 points of the benchmark contour) takes 1-5 steps: there a cheaper cycle beats a better one
    // (measured at 1M unknowns: projected phase 1.17 -> 0.99 s without the coarse post-smoothing, while the from-zero solves of the
    // snapshot phase lose 1.26 -> 1.63 s).
    // ... and the fine level's too: the light cycle is V(1,0) on every level -- projected phase 1.02 -> 0.89 s, same eigenpairs
    // (residuals 5.6e-9 -> 6.4e-9, rank gap 1.2e9), 9 325 -> 9 139 column-iterations per pass.
    const int npost = h->vc_light ? 0 : h->nsweeps;
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
    // (post-smoothing has a weight of its own, opts[10]: two sweeps with different weights form a degree-2 polynomial smoother)
    for (int s = 0; s < npost; ++s) {
        cplx *dst = (final_out && s == npost - 1) ? final_out : t;
        launch_spmv(A, pc, bt.cps, x, dst, b, h->jac_w_post * h->lvl_scale[(size_t)l], bt.nb, MODE_JAC, st, cm);
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
void penalty_polish(wae_family *h, const Batch &bt, const cplx *B, cplx *X) {
    if (h->n_penalty <= 0) return;
    // Sweeps: 22 damped point relaxations whose weights are the reciprocals of the Chebyshev nodes of [0.4, 2.2] -- the interval that
    // holds the spectrum of D^-1 A_bb for a P1 boundary mass matrix ([1/2, 2]) with a margin -- taken in an order that keeps the partial
    // products bounded (round 4: the same 1e-9 as 40 sweeps with the fixed weight 0.8, whose contraction is 0.6 per sweep; 1.3 -> 0.7 ms
    // per chunk of the projected phase).
    static const std::vector<double> cheb = []() {
        const int n = 22;
        const double lo = 0.4, hi = 2.2, th = 0.5 * (hi + lo), de = 0.5 * (hi - lo);
        std::vector<double> w(n);
        for (int k = 0; k < n; ++k) w[k] = 1.0 / (th - de * std::cos((2 * k + 1) * M_PI / (2 * n)));
        std::vector<double> o;                                    // nodes from both ends inwards: large and small weights alternate
        for (int a = 0, b = n - 1; a <= b; ++a, --b) { o.push_back(w[a]); if (a != b) o.push_back(w[b]); }
        return o;
    }();
    const int sweeps = (int)cheb.size();
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
    launch_jacobi0(Ab, pcb, bt.cps, h->pen_b.p, x, cheb[0], nb, st);
    for (int s = 1; s < sweeps; ++s) {
        launch_spmv(Ab, pcb, bt.cps, x, t, h->pen_b.p, cheb[(size_t)s], nb, MODE_JAC, st);
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
        h->gs_R.reserve((size_t)m * (m + 1) * nb); h->gs_sn.reserve((size_t)m * nb); h->gs_g.reserve((size_t)(m + 1) * nb); h->gs_rescale.reserve((size_t)nb);
        h->gs_cs.reserve((size_t)m * nb); h->gs_sv.reserve((size_t)(m + 2) * nb); h->gs_relres.reserve((size_t)nb); h->gs_bnorm.reserve((size_t)nb);
        h->gs_hist.reserve((size_t)histcap * nb); h->gs_int.reserve((size_t)5 * nb + 4); h->gs_done.reserve((size_t)nb);
        h->cmask.reserve(nch); h->vsq.reserve((size_t)(m + 2) * nb);
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
        h->gs_Hraw.reserve((size_t)m * (m + 1) * nb); h->gs_pair.reserve(((size_t)4 * (m + 3) + 8) * nb); h->gs_sub.reserve((size_t)m * nb);
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
            h->gs_pair.reserve(need);
            if (h->h_pin_pair_n < need) {
                if (h->h_pin_pair) { (void)hipHostFree(h->h_pin_pair); h->h_pin_pair = nullptr; h->h_pin_pair_n = 0; }
                HIP_CHECK(hipHostMalloc((void **)&h->h_pin_pair, need * sizeof(cplx)));
                h->h_pin_pair_n = need;
            }
            pr_dev = h->gs_pair.p; pr_host = h->h_pin_pair;
            h->vsq.reserve(PK);
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
        h->cmask.reserve(nch);
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
int gmres(wae_family *h, const Batch &bt, const cplx *B, cplx *X, double tol, int maxit, wae_solve_info *info, const cplx *guess_dir, bool have_x0,
          double *relres_out) {
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
int CallInfo::finish(wae_solve_info *out) {
    li.seconds = now_s() - t0;
    const int rc = info_code(li);
    if (out) *out = li;
    return rc;
}

// solve a chunk of nb columns already on device in interleaved layout
int solve_chunk(wae_family *h, const Batch &bt, const std::vector<std::vector<zc>> &pcs, const cplx *B, cplx *X, double tol, int maxit,
                wae_solve_info *info, const cplx *guess_dir, bool have_x0) {
    upload_pc(h, pcs);
    dense_setup(h, bt);
    return gmres(h, bt, B, X, tol, maxit, info, guess_dir, have_x0);
}

extern "C" {

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
        h->io_a.reserve(cnt); h->io_b.reserve(cnt);
        HIP_CHECK(hipMemcpyAsync(h->io_a.p, B, cnt * sizeof(cplx), hipMemcpyHostToDevice, st));
        DevBuf<cplx> gcol, gint;
        if (Gd) {
            gcol.alloc(cnt); gint.alloc((size_t)d * h->NB);
            HIP_CHECK(hipMemcpyAsync(gcol.p, Gd, cnt * sizeof(cplx), hipMemcpyHostToDevice, st));
        }
        for (int c0 = 0; c0 < r; c0 += h->NB) {
            const int nb = std::min(h->NB, r - c0);
            const Batch bt = ncoef == 1 ? Batch::one_system(nb, op) : Batch::per_column(nb, op);
            std::vector<std::vector<zc>> pcs((size_t)bt.nsys);
            for (int b = 0; b < bt.nsys; ++b) plane_coeffs(h, coeffs + (size_t)(ncoef == 1 ? 0 : c0 + b) * 2 * h->T, op, pcs[(size_t)b]);
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

}   // extern "C"
