// The family handle and the few helpers that setup.hip (construction of the handle and of the multigrid hierarchy), lib.hip (operator
// products, C ABI) and the solver units (solver.h) share.  Private to those files: mgpu.hip goes through the C ABI and
// wae_internal_device / _stream.
#pragma once
#include <algorithm>
#include <chrono>
#include <future>

#include "amg.h"
#include "tiles.h"

struct RbState {                     // snapshot basis of wae_beyn_moments_rb (one per handle)
    cplx *Q = nullptr;               // store: cap snapshots of d x l (interleaved [row][column]); slots < S are orthonormal per column
    int cap = 0, l = 0, S = 0;
    std::vector<int> kact;           // terms that take part in the projection
    std::vector<zc> Hk;              // Hk[ki][(s*cap + i)*l + c] = q_i^H A_k q_s   (column c's basis)
    std::vector<zc> g;               // g[i*l + c] = q_i^H v_c
    DevBuf<cplx> W, Vi, hb, alpha, alpha2, ycoef;   // W_k = A_k Q (resident), probe columns interleaved, small scratch
    std::future<void> w_job;         // W (20 GB at 1M unknowns: ~0.4 s of hipMalloc) is mapped on a helper thread while the first
    void wait_w() { if (w_job.valid()) w_job.get(); }       // snapshot systems are solved; whoever touches W waits for it here
    bool vi_valid = false;           // Vi holds the probe matrix the basis was started with (false after an import)
    ~RbState() { if (w_job.valid()) w_job.wait(); }
};

struct wae_family {
    bool vc_light = false;               // the current solve belongs to the projected phase of a contour integral (1-5 steps from a good guess): vcycle() runs its light form
    int device = 0;
    hipStream_t stream = nullptr;
    int64_t d = 0;
    int T = 0;
    std::vector<int> term_plane;     // term k -> plane index (in the order planes were discovered)
    std::vector<zc> term_scale;      // term k = scale * plane
    std::vector<int64_t> term_nnz;
    int nplanes = 0;
    std::vector<CsrZ> planes0;       // host copies of the fine planes (set-up input), in the library's row numbering
    // Row renumbering (tiles.h): internal row i is the caller's row perm[i].  Applied to the term matrices at create, to
    // every vector at the ABI boundary (layout kernels), never visible outside.
    std::vector<int> perm_h;
    DevBuf<int> perm_dev;
    std::vector<int> tile_row_ptr;   // tiles of the fine level (empty: no tiling)
    const int *perm() const { return perm_dev.p; }
    std::vector<LevelOp> ops;        // ops[0] = fine level
    std::vector<std::vector<int>> slot_plane;   // per level: slot -> plane
    std::vector<Transfer> xfer;
    // dense coarsest level
    int64_t nc = 0;
    DevBuf<cplx> dense_planes, Ainv;
    DevBuf<int> dstatus;
    bool solver_ready = false;
    double jac_w = 0.8;                  // weight of the pre-smoothing sweeps of the full V-cycle (opts[2])
    double jac_w_post = 0.9;             // ... of its post-smoothing sweeps (opts[10])
    double jac_w_light = 0.5;            // ... of the single sweep of the light cycle (opts[11]; projected phase of a contour integral)
    int nsweeps = 1, restart = 30, NB = 64;
    std::vector<double> lvl_lambda, lvl_scale;   // per level (ops.size() entries): the spectral estimate and the factor on the three weights (opts[12]; 0 and exactly 1.0 without)
    // workspaces
    std::vector<DevBuf<cplx>> lx, lb, lt;
    DevBuf<cplx> V, W, Z, Xs, Bs, U, partial, hdev, ydev, pcdev, one_dev, io_a, io_b, zw_dev;
    DevBuf<cplx> vsq;                // 1/||v_i||^2 per basis slot and column: the wide-batch GMRES keeps its basis unnormalised
    DevBuf<cplx> rbQ;                // library-owned snapshot store of wae_beyn_moments_rb
    RbState rb;                      // the snapshot basis and its projected terms
    DevBuf<int> plane_col_dev;
    DevBuf<unsigned char> cmask;     // one byte per 8-column chunk of the current batch (0 = converged)
    // device-resident recurrence of the wide-batch GMRES (Gmres::run_device)
    DevBuf<cplx> gs_R, gs_sn, gs_g, gs_rescale, gs_Hraw, gs_pair;
    DevBuf<double> gs_sub;
    DevBuf<double> gs_cs, gs_sv, gs_relres, gs_bnorm, gs_hist;
    DevBuf<int> gs_int;              // conv | steps | iters | histlen | stalled | status(4)
    DevBuf<unsigned char> gs_done;
    // penalty (Dirichlet-like) rows found at set-up: their sub-block as a small operator of its own (see penalty_polish)
    int64_t n_penalty = 0;
    LevelOp pen_op;
    std::vector<int> pen_slot;
    LevelOp pen_row_op;              // the penalty ROWS of the operator (n_penalty x d): their residual without a full SpMV
    std::vector<int> pen_row_slot;
    DevBuf<int> pen_rows;
    DevBuf<cplx> pen_b, pen_x, pen_t;
    // device-resident multivectors of the caller ("slots", wae_slot_*): d x ncols, column-major, in the library's row numbering
    struct Slot { DevBuf<cplx> buf; int ncols = 0; };
    Slot slots[WAE_NSLOTS];
    // work space of the Arnoldi processes (kept between calls); after wae_arnoldi_shiftinvert_slots the basis of that call stays in
    // arn_EV: arn_cols vectors of arn_nsys systems each, interleaved [row][system], for wae_arnoldi_ritz_to_slot
    DevBuf<cplx> arn_EV, arn_t, arn_pcM, arn_hcol, arn_stage, arn_gdir;
    int arn_nsys = 0, arn_cols = 0;
    DevBuf<cplx> pt_ws;              // work space of wae_perturb / wae_perturb_slots (grow-only, kept between calls)
    DevBuf<cplx> pt_Gd, pt_pcd;      // results and plane tables of wae_slot_forms
    cplx *h_pinned = nullptr;        // (restart+2)*NB
    cplx *h_pin_pair = nullptr;      // staging of the pair steps of the narrow batches (gmres)
    size_t h_pin_pair_n = 0;
    size_t pc_stride_level = 0;      // elements per level in pcdev
    ~wae_family() {                  // every DevBuf member frees itself
        if (stream) (void)hipStreamSynchronize(stream);
        if (h_pinned) (void)hipHostFree(h_pinned);
        if (h_pin_pair) (void)hipHostFree(h_pin_pair);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

struct Batch {
    int nb;     // columns (leading dimension of every multivector)
    int cps;    // columns per system
    int nsys;
    int op;
    static Batch one_system(int nb, int op) { return Batch{nb, nb, 1, op}; }       // one coefficient set for all columns
    static Batch per_column(int nb, int op) { return Batch{nb, 1, nb, op}; }       // one system (coefficient set) per column
};

// ----------------------------------------------------------------------------------------------------
// helpers
// ----------------------------------------------------------------------------------------------------
static int env_int(const char *name, int dflt) { const char *v = getenv(name); return v ? atoi(v) : dflt; }
// WAE_XFER_TILES=0: the older prolongation kernel (A/B measurements, tests)
static bool xfer_tiles_on() { return env_int("WAE_XFER_TILES", 1) != 0; }
static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static void require_solver(const wae_family *h) {
    if (!h->solver_ready) throw WaeError(WAE_ERR_INVALID, "wae_solver_setup has not been called");
}
// plane coefficients for one system from term coefficients (aliased terms folded in), conj for op = C
static void plane_coeffs(const wae_family *h, const double *coeffs, int op, std::vector<zc> &pc) {
    pc.assign(h->nplanes, zc(0));
    for (int k = 0; k < h->T; ++k) pc[h->term_plane[k]] += h->term_scale[k] * zc(coeffs[2 * k], coeffs[2 * k + 1]);
    if (op == WAE_OP_C)
        for (auto &c : pc) c = std::conj(c);
}
// dst[q] = pc[slot_plane[q]]: the nplanes coefficients of one system in the slot order of a level (h->slot_plane[level]) or of a penalty block
static void slot_coeffs(const wae_family *h, const std::vector<int> &slot_plane, const std::vector<zc> &pc, cplx *dst) {
    for (int q = 0; q < h->nplanes; ++q) dst[q] = cplx{pc[slot_plane[q]].real(), pc[slot_plane[q]].imag()};
}

template <class F> static int guarded(F &&f) { return wae_guarded(f); }       // the one definition: wae_internal.h
