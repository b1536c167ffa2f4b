// What crosses the solver units (gmres.hip, beyn.hip, forced.hip, arnoldi.hip, slots.hip, perturb.hip, debug.hip): every function and
// struct here is used by more than one of them, everything else is static in its unit.  Private to the library.
#pragma once
#include "family.h"

// ---- gmres.hip ----
// upload [level][sys][slot] tables (plane_coeffs: family.h)
void upload_pc(wae_family *h, const std::vector<std::vector<zc>> &pcs);
const cplx *pc_level(const wae_family *h, int l);
// the dense coarsest level of the systems of the last upload_pc, assembled and inverted
void dense_setup(wae_family *h, const Batch &bt);
// weight of the PRE-smoothing sweeps of level l: the set-up's (opts[2]) -- or, in the light cycle of the projected phase, its own
// (opts[11]) -- times the level's scale (opts[12]; exactly 1.0 without it).  The callers outside vcycle() fuse the first sweep of level 0.
double pre_weight(const wae_family *h, int l = 0);
// x = Minv b on level l;  returns pointer to the result (either lx[l] or lt[l])
// have_x0: the first sweep of level l (x = w/diag b) is already in lx[l] (written by the SpMV that produced b, MODE_AX_J0)
// final_out (level 0 only): the last post-smoothing sweep -- or, in a cycle without one, the prolongation -- writes its result there (a
// Krylov basis slot) instead of into lx/lt; masked chunks of final_out are left as they were
// cn (level 0 only): the caller wants the column norms of the result in cn->out.  A cycle that ends in its prolongation (the light
// cycle) takes them from that kernel and sets cn->done -- with cn->only it then writes no result at all; any other cycle leaves
// cn->done false and the caller runs its own pass over the result.
struct CycleNorms { cplx *out; bool only; bool done = false; };
cplx *vcycle(wae_family *h, const Batch &bt, int l, const cplx *b, const unsigned char *cm = nullptr, bool have_x0 = false,
             cplx *final_out = nullptr, CycleNorms *cn = nullptr);
// the penalty rows' own equations  A_bb d = (b - A x)_b  solved for the given interior values, X += d (best effort; see gmres.hip)
void penalty_polish(wae_family *h, const Batch &bt, const cplx *B, cplx *X);
// left-preconditioned lock-step GMRES(m) on the systems of the last upload_pc / dense_setup; returns the number of lock-step iterations
int gmres(wae_family *h, const Batch &bt, const cplx *B, cplx *X, double tol, int maxit, wae_solve_info *info, const cplx *guess_dir = nullptr,
          bool have_x0 = false, double *relres_out = nullptr);
// solve a chunk of nb columns already on device in interleaved layout
int solve_chunk(wae_family *h, const Batch &bt, const std::vector<std::vector<zc>> &pcs, const cplx *B, cplx *X, double tol, int maxit,
                wae_solve_info *info, const cplx *guess_dir = nullptr, bool have_x0 = false);
// the wae_solve_info of one public call: zeroed, timed from here, handed to the caller with the call's return code
struct CallInfo {
    wae_solve_info li{};
    double t0 = now_s();
    int finish(wae_solve_info *out);
};

// ---- slots.hip ----
// column `col` of a slot (d entries, the library's row numbering); throws on an empty slot or a column outside it
cplx *slot_col(wae_family *h, int32_t slot, int32_t col);
// n columns of a slot as one contiguous column-major block: the slot's own memory if they are consecutive, a copy in `stage` otherwise
const cplx *slot_cols_ptr(wae_family *h, int32_t slot, const int32_t *cols, int n, DevBuf<cplx> &stage, hipStream_t st);
