/* waehip.h -- C ABI of libwaehip.so: the MI355X (gfx950) NLEVP hot path for WavesAndEigenvalues.jl.
 *
 * The reference (Julia, serial, CPU) has no FFI of its own; the drop-in boundary is the method surface its
 * solvers use on a LinearOperatorFamily.  Each entry below names the reference call sites
 * it replaces (paths relative to the reference repository root).  Conventions:
 *   - every function returns int: 0 ok, >0 warning (e.g. WAE_WARN_MAXITER), <0 error; no C++ exception
 *     crosses the boundary; wae_last_error() returns a thread-local message for the last failure.
 *   - complex numbers are interleaved (re,im) doubles == Julia ComplexF64 == C99 double _Complex.
 *   - dense arrays are column-major (Julia Array) with leading dimension d unless stated.
 *   - the caller owns all host buffers and must keep them alive for the duration of the call only
 *     (Julia: GC.@preserve); the library copies inputs at wae_family_create.
 *   - calls on one handle must be serialised by the caller (the reference is single-threaded).
 *   - no torch / HIP types appear in signatures; "dev" pointers are raw device addresses (uint64-castable).
 */
#ifndef WAEHIP_H
#define WAEHIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct wae_family wae_family;      /* opaque: all terms A_k resident in HBM + solver workspaces */

/* return codes: mapped by the host wrappers onto the reference's itsol_* flags
 * (src/NLEVP/iterative_solvers.jl:4-14), like the reference maps exceptions (:192-210). */
#define WAE_OK                 0
#define WAE_WARN_MAXITER       1   /* inner Krylov solve hit maxit on >=1 column  -> itsol_maxiter            */
#define WAE_WARN_STAGNATION    2   /*                                             -> itsol_slow_convergence   */
#define WAE_ERR_INVALID       -1   /* bad argument                                -> itsol_impossible         */
#define WAE_ERR_BREAKDOWN     -2   /* singular coarse operator / Krylov breakdown -> itsol_singular_exception */
#define WAE_ERR_EIGS          -3   /* shift-invert Arnoldi did not converge       -> itsol_arpack_exception   */
#define WAE_ERR_NAN           -4   /*                                             -> itsol_isnan              */
#define WAE_ERR_HIP           -5   /* HIP runtime failure                         -> itsol_unknown            */

/* operator applied: N = L, T = L^T, C = L^H (Julia `A'`: Householder.jl:101, iterative_solvers.jl:398,572) */
#define WAE_OP_N 0
#define WAE_OP_T 1
#define WAE_OP_C 2

/* storage orientation of the term matrices handed to wae_family_create */
#define WAE_CSC 0   /* Julia SparseMatrixCSC (colptr,rowval,nzval) */
#define WAE_CSR 1

const char *wae_last_error(void);
int wae_device_count(int *n);
/* version / build info string (static) */
const char *wae_version(void);

/* -- family ------------------------------------------------------------------------------------------
 * Upload the T term matrices of a LinearOperatorFamily once (replaces nothing in the reference by itself:
 * it is what makes `L(z)` (src/NLEVP/LinOpFam.jl:482-529) a device-resident operator instead of a new
 * SparseMatrixCSC per call).  Re-create only if a term's matrix changes, not if L.params change.
 *   d            dimension (size(L), LinOpFam.jl:385-393)
 *   T            number of terms (length(L.terms)), including the "__aux__" term if present
 *   index_bytes  4 (UInt32/Int32, Helmholtz.jl:407-408,515) or 8 (Int64)
 *   base         0 or 1 (Julia)
 *   orientation  WAE_CSC / WAE_CSR
 *   ptr[k], idx[k], val[k]  per-term arrays: ptr has d+1 entries, idx/val have nnz_k entries
 *   device       HIP device ordinal
 */
int wae_family_create(wae_family **out, int64_t d, int32_t T, int32_t index_bytes, int32_t base,
                      int32_t orientation, const void *const *ptr, const void *const *idx,
                      const double *const *val, int32_t device);
/* wae_family_create with options (opts may be NULL / nopts 0 = wae_family_create):
 *   opts[0]  symmetry tolerance of the TRANSPOSED products, default 0.  A term matrix whose transpose equals itself is stored
 *            once and applied as it is for op = T / C (`A'*y`, `A'\\b`: Householder.jl:101, iterative_solvers.jl:398,572); with 0
 *            that requires mirror entries that are equal bit for bit, so `A'` is exactly `A'`.  A finite-element matrix
 *            (`discretize`: M, K, C of src/Helmholtz.jl:405-463) is symmetric by construction but, assembled in floating point,
 *            only up to the order of its element sums; opts[0] = t > 0 accepts  |a_ij - a_ji| <= t * min(s_i, s_j),
 *            s_i = largest off-diagonal magnitude of row i (a penalty or Dirichlet diagonal entry does not widen the test),
 *            and the adjoint products of such a family then run on the same fast path as the forward ones -- differing from the
 *            exact transposed product by that assembly rounding (<= t per entry, relative to the row scale).  The Helmholtz
 *            wrappers pass 1e-14; must lie in [0, 1e-8]. */
int wae_family_create_opts(wae_family **out, int64_t d, int32_t T, int32_t index_bytes, int32_t base,
                           int32_t orientation, const void *const *ptr, const void *const *idx,
                           const double *const *val, int32_t device, const double *opts, int32_t nopts);
int wae_family_destroy(wae_family *h);
/* d, T, total nnz, and the algorithmic byte count of one spmv_sum with r right-hand sides over the terms
 * whose coefficient is non-zero in `mask` (NULL = all):  sum_k[nnz_k*(16+4)+(d+1)*4] + 2*r*d*16 */
int wae_family_info(const wae_family *h, int64_t *d, int32_t *T, int64_t *nnz_total);
int64_t wae_family_spmv_bytes(const wae_family *h, const uint8_t *mask, int32_t r);

/* -- Y = sum_k c_k op(A_k) X -------------------------------------------------------------------------
 * Replaces `L(z)*x`, `L(z,1)*x`, `L(m,n)*w`, `M*v`, `A'*y`: LinOpFam.jl:482-529 followed by a sparse
 * mat-vec (iterative_solvers.jl:307,399,571-572,581; perturbation.jl:339,352,413; Householder.jl:189-190).
 *   coeffs  T complex scalars c_k = prod_j f_kj(params; derivs) evaluated on the host (LinOpFam.jl:466-477);
 *           a term skipped by the functor (LinOpFam.jl:502-516) is passed as 0.
 *   X, Y    d x r column-major complex, host memory.  r = 0 is a no-op (`L(z)*zeros(d,0)`), and so are wae_solve /
 *           wae_solve_guess with r = 0 and wae_eig_residuals with n = 0: WAE_OK, nothing is read or written.
 */
int wae_spmv_sum(wae_family *h, const double *coeffs, const double *X, double *Y, int32_t r, int32_t op);
/* one coefficient set per column (ncoef = r): Y[:,j] = sum_k c_jk op(A_k) X[:,j] -- e.g. the residuals L(w_j) v_j of
 * all Beyn eigenpairs in one launch; ncoef = 1 is wae_spmv_sum. */
int wae_spmv_sum_cols(wae_family *h, const double *coeffs, int32_t ncoef, const double *X, double *Y, int32_t r,
                      int32_t op);
/* per-term inputs: Y = sum_k c_k A_k X_k, X = d x T column-major (regrouped perturbation recurrence,
 * SURVEY appendix C; replaces the sum over (m,n) of `L(m,n)*w` at perturbation.jl:394-415). */
int wae_spmv_sum_multi(wae_family *h, const double *coeffs, const double *X, double *Y);

/* -- solver set-up ----------------------------------------------------------------------------------
 * Build the multigrid hierarchy used to precondition every `L(z)\b` (smoothed aggregation on
 * Re(sum_k c_ref_k A_k); every term is Galerkin-projected so that coarse operators are again families).
 * Replaces the symbolic analysis UMFPACK repeats at every `\`/`lu` call (beyn.jl:65,257; perturbation.jl:329).
 * Must be called once before wae_solve / wae_beyn_moments / wae_arnoldi_shiftinvert / wae_perturb.
 * opts (may be NULL -> defaults): [0] strength threshold (0.02), [1] max coarse size (128; the coarsest
 *   level is inverted dense by one workgroup per system and may have at most 2048 unknowns: WAE_ERR_INVALID beyond),
 *   [2] Jacobi weight (0.8), [3] pre/post sweeps (1), [4] GMRES restart (30), [5] penalty-row ratio (1e8),
 *   [6] batch width (columns solved in lock-step, 64).
 *       Recurrence length: the Krylov basis holds opts[4] + 1 vectors of opts[6] columns, and a request of r columns runs in chunks of
 *       opts[6], opts[6], ..., remainder.  A chunk of nb columns restarts after m = min(150, floor((opts[4] + 1) * opts[6] / nb) - 1)
 *       steps: opts[4] for a full chunk, MORE for a chunk narrower than the batch width (16 columns, restart 6: m = 8 for 12 columns, 13
 *       for 8, 36 for 3).  A deflated guess direction (wae_solve_guess) takes one slot: m - 1.
 *   [7] bit mask (as a double) of terms kept OUT of the shape matrix that the strength graph, the aggregates and the
 *       prolongator smoothing are built from (0).  Bloch families (src/Helmholtz.jl:508-513) pass the seam parts here:
 *       the solution jumps by exp(i b 2pi/N) across the seam, so no aggregate may span it.
 *   [10] weight of the POST-smoothing sweeps (0.9), [11] weight of the one sweep of the light cycle (0.5) -- the V(1,0) cycle the
 *       solves of wae_beyn_moments_rb's projected phase run, which start next to the answer and take 1-5 steps.
 *   [8], [9] workspace hints (0 = none): probe columns l and snapshot capacity of the contour integrals that will follow
 *       (wae_beyn_moments_rb): the snapshot store and the resident term products are then mapped during the set-up, behind
 *       its host work, instead of during the first integral.
 *   [12] per-level weight scaling: 0 (default) none, 1 spectral; anything else WAE_ERR_INVALID.  With 1, every level l above the dense one
 *       gets s_l = min(1, 5 / (3 * 1.1 * lambda_l)) and the V-cycle multiplies its three weights ([2], [10], [11]) by s_l on that level.
 *       lambda_l estimates lambda_max(D^-1 Re A_ref) of the level, D = diag(Re A_ref): WAE_WEIGHT_POWER_STEPS steps of a power iteration
 *       on |D|^-1/2 Re A_ref |D|^-1/2 with the level's own operator product, from a fixed start vector -- a lower bound (the quotient of
 *       two norms of a symmetric matrix's iterates), reached to within 10 % on the hierarchies it was chosen on, hence the factor 1.1;
 *       a sweep with weight 5 / (3 lambda) damps every eigenvalue in [lambda / 5, lambda] by 2/3 or better.  Two set-ups give the same
 *       bits.  With 0 every s_l is exactly 1.0 and every launch receives the arguments it received before the option existed.
 */
#define WAE_WEIGHT_POWER_STEPS 40
int wae_solver_setup(wae_family *h, const double *coeffs_ref, const double *opts, int32_t nopts);
/* The same set-up from prolongators the caller supplies -- the nested hierarchy of a refined mesh (wae_octosplit_prolongator), or any
 * other nested hierarchy -- instead of aggregating the fine matrix.  coeffs_ref, opts, nopts as in wae_solver_setup.
 *   nlev >= 1 real CSR prolongators, finest first, 0-based, 32-bit indices, columns ascending without duplicates in every row:
 *   prolongator k has rows[k] rows and cols[k] columns; rows[0] = d, rows[k + 1] = cols[k]; all in the caller's numbering.  R = P^T.
 *  - Penalty rows are found at the fine level by the rule of wae_solver_setup (|a_ii| > opts[5] x the median at coeffs_ref); their rows of
 *    prolongator 0 are emptied.  A column left without entries is dropped from its level and from the rows of the next prolongator.
 *    Coarser levels have no penalty rows.
 *  - The coarse planes P^T A P of the supplied levels are formed on the device, plane by plane: one thread per stored entry writes its
 *    keyed triplets, a stable sort and a reduce-by-key sum them in a fixed order (the pipeline of the device assembly).  Two set-ups give
 *    the same bits.  A product that expands to more than 2^31 - 1 triplets is refused (WAE_ERR_INVALID).
 *  - If the coarsest supplied level is larger than opts[1], smoothed aggregation continues from that level's planes and its levels are
 *    appended; opts[7] applies to those levels only.  The dense limit of wae_solver_setup holds for the last level.
 *  - The fine level's renumbering, the tile storage of level 1, the penalty operators, the dense level and the work spaces are those of
 *    wae_solver_setup.
 * WAE_ERR_INVALID with a message, before the hierarchy the handle has is touched (it keeps working): nlev < 1, a null array, dimensions
 * that do not chain, prolongator 0 with other than d rows, a row pointer that is not monotone from 0, a column out of range, unsorted or
 * duplicate columns in a row, a value that is not finite.  wae_solver_setup after this call replaces the hierarchy again. */
int wae_solver_setup_nested(wae_family *h, const double *coeffs_ref, const double *opts, int32_t nopts, int32_t nlev, const int64_t *rows,
                            const int64_t *cols, const int32_t *const *ptr, const int32_t *const *col, const double *const *val);
/* The levels above the dense one of the current hierarchy: *nlev their number; lambda[l], scale[l] for l < min(cap, *nlev) the estimate
 * and the factor s_l of opts[12] (0.0 and 1.0 with the option off).  Any pointer may be NULL.  Needs a set-up. */
int wae_solver_level_weights(const wae_family *h, int32_t cap, double *lambda, double *scale, int32_t *nlev);

typedef struct {
    int32_t iters_max;      /* most iterations any column needed            */
    int32_t iters_total;    /* sum over columns (of the steps each column took itself, not of the lock-step iterations) */
    int32_t n_unconverged;  /* columns that stopped at maxit                 */
    int32_t levels;         /* multigrid levels used                         */
    double  relres_max;     /* max_b ||M^-1(B_b - A X_b)|| / ||M^-1 B_b||: preconditioned (error-like) residual.  Recomputed from X,
                               except after a cycle of at most 12 steps that was accepted on its estimate (below): then the estimate */
    double  seconds;        /* wall time of the device work                  */
} wae_solve_info;
/* Stopping rule of every solve (tests/test_gpu_solve_driver.py).  Within a cycle a column stops at the first step whose residual ESTIMATE
 * (the least-squares residual of the recurrence, relative to ||M^-1 B_b||) is <= 0.7 * tol.  A cycle that ends with every column stopped
 * after at most 12 steps is accepted on the estimate.  Otherwise the preconditioned residual is recomputed from X at the start of the
 * next cycle, and a column is done when it is <= tol (so a column can end between 0.7 * tol and tol at a cycle start).  A column whose
 * estimate gained less than 10 % over 30 steps, with more than 60 steps behind it, ends as stalled (WAE_WARN_STAGNATION if above tol).
 * A step -- or a pair of steps, where the recurrence takes two per pass over the basis -- is only started if it ends at or before maxit:
 * no column takes more than maxit steps.  A column with a zero right-hand side takes no step and is returned as zeros. */

/* -- X = op(sum_k c_k A_k)^{-1} B -------------------------------------------------------------------
 * Replaces sparse `\` / `lu` + solve (UMFPACK): beyn.jl:65,257; iterative_solvers.jl:307,397-398,570-572;
 * perturbation.jl:359,423,539.  ncoef = 1: one coefficient set for all r columns;
 * ncoef = r: column j uses coeffs[j*T .. j*T+T) (independent systems solved in lock-step).
 */
int wae_solve(wae_family *h, const double *coeffs, int32_t ncoef, const double *B, double *X, int32_t r,
              int32_t op, double tol, int32_t maxit, wae_solve_info *info);

/* wae_solve with a known near-null direction per column, G[:,b].  The Newton-type solvers know the dominant direction of
 * the solution close to an eigenvalue (the current eigenvector iterate: `u = L(z)\(L(z,1)*x0)`,
 * iterative_solvers.jl:307,571-572), where the reference relies on UMFPACK factorising a nearly singular L(z).  Here the
 * direction is deflated: with u^ = M^-1 A g / ||.|| the Krylov process runs on (I - u^ u^H) M^-1 A and the solution is
 * x = x_K + alpha g, alpha cancelling the u^ component of the residual (single-level hierarchies, whose preconditioner is
 * the exact inverse, fall back to the initial guess x0 = alpha g).  G may be NULL (= wae_solve). */
int wae_solve_guess(wae_family *h, const double *coeffs, int32_t ncoef, const double *B, const double *G, double *X,
                    int32_t r, int32_t op, double tol, int32_t maxit, wae_solve_info *info);

/* -- forced response: x_j = L(w_j)^{-1} b_j over a list of excitation frequencies, in HBM ------------------------------
 * The forced problem of the reference (`L(w) \ Array(rhs(w))` with the `rhs` family of `discretize(...; source=true)`, read with
 * get_p / get_n_grad_p, src/FEM/helmholtz_getters.jl) as a sweep: neither the d x nfreq right-hand sides nor the d x nfreq solutions exist
 * anywhere; what crosses the bus is the sparse input and what was asked for.  All row indices are 0-based, in the caller's numbering:
 *     b_j    = sum_s src_coeff[j,s] m_s          nsrc sparse vectors (src_ptr: nsrc+1 offsets, src_idx, src_val complex)
 *     x_j    = (sum_k coeff_table[j,k] A_k)^{-1} b_j
 *     H[q,j] = sum_i obs_val_q[i] x_j[obs_idx_q[i]]   nobs sparse functionals, no conjugation; H_out[q + nobs*j], complex
 *     X_out[:,k] = x_{keep[k]}                    d x nkeep column-major, keep: strictly ascending frequency indices
 * Indices that repeat inside one sparse vector add up.  The frequencies run in chunks of the handle's batch width (opts[6] of
 * wae_solver_setup), each chunk one lock-step solve from a zero guess with one coefficient set per column (wae_solve with ncoef == r); the
 * right-hand sides are filled and the functionals applied on the device, without atomics and in a fixed order: the same bits on every
 * call.  coeff_table: nfreq x T complex, row j = the coefficients of L(w_j); src_coeff: nfreq x nsrc complex, row j.
 * WAE_ERR_INVALID, with nothing launched: nfreq < 0; a ptr array that does not start at 0 or decreases; an index outside 0..d-1; a value
 * or coefficient that is not finite; keep out of range or not strictly ascending; nobs == 0 and nkeep == 0 (nothing was asked for); no
 * wae_solver_setup.  nfreq == 0 returns WAE_OK and touches nothing.  info as in wae_solve, maxima and sums over all chunks. */
int wae_forced_response(wae_family *h, int32_t nfreq, const double *coeff_table, int32_t nsrc, const int64_t *src_ptr, const int32_t *src_idx,
                        const double *src_val, const double *src_coeff, int32_t nobs, const int64_t *obs_ptr, const int32_t *obs_idx,
                        const double *obs_val, double *H_out, int32_t nkeep, const int32_t *keep, double *X_out, double tol, int32_t maxit,
                        wae_solve_info *info);

/* -- Beyn moments -------------------------------------------------------------------------------------
 * The whole quadrature loop of `beyn` / `compute_moment_matrices` (beyn.jl:62-74,112-138,251-268):
 *   A[:,:,p] = sum_j w_j z_j^p (sum_k c_jk A_k)^{-1} V ,  p = 0..2K-1
 * npts points z[j] with effective weights w[j] (= GL weight * (b-a)/2), coefficient table npts x T
 * (row j = coefficients of L(z_j)), V d x l column-major.  Output d x l x 2K column-major (host), or, with
 * out_dev != 0, written to that device address instead (layout identical) so that the caller can reduce
 * partial moments across GPUs with RCCL before copying to the host.
 */
int wae_beyn_moments(wae_family *h, int32_t npts, const double *z, const double *w, const double *coeff_table,
                     const double *V, int32_t l, int32_t K, double tol, int32_t maxit, double *A_out,
                     uint64_t out_dev, wae_solve_info *info);

/* -- Beyn moments on several GPUs of one node, from ONE host process (SURVEY.md 8b `beyn_moments(..., ngpu)`, 8e) ------------
 * The quadrature loop of `beyn` / `compute_moment_matrices` (beyn.jl:62-74,112-138,251-268) with its points shared out over
 * ngpu devices.  handles[g]: a replica of the family on device g (wae_family_create(..., device = g) + wae_solver_setup with
 * the same arguments on each; distinct devices); the library runs one host thread and one stream per device.  nsnap > 0 (and
 * npts >= 2 nsnap): the snapshot-projection scheme of wae_beyn_moments_rb -- nsnap snapshot points solved first, split over
 * the devices by probe column when ngpu divides l (every device finishes the basis of its columns; the bases are exchanged
 * with one RCCL all-gather over xGMI), otherwise by point (raw snapshots all-gathered, every device rebuilds the basis); the
 * other points start from the projection, round-robin over the devices.  nsnap = 0: every point from a zero guess.  The
 * partial moment tensors are summed on device 0 with one RCCL reduce and copied to A_out (host, d x l x 2K column-major).
 * RCCL is loaded at first use (dlopen of librccl.so.1); ngpu = 1 runs the same code with one rank.  info: maxima / sums over
 * all devices.  Everything else as wae_beyn_moments. */
int wae_beyn_moments_mgpu(wae_family *const *handles, int32_t ngpu, int32_t npts, const double *z, const double *w,
                          const double *coeff_table, const double *V, int32_t l, int32_t K, double tol, int32_t maxit,
                          int32_t nsnap, double *A_out, wae_solve_info *info);

/* -- residual check of eigenpairs (the last step of `beyn`'s callers: which Ritz pairs are eigenpairs) --------------
 * res_out[j] = || sum_k c_jk A_k v_j || / sum_k |c_jk| || A_k v_j ||   for the n pairs (coeff_table: n x T complex, row j =
 * the coefficients of L(omega_j); v_j = column j of the column-major d x n matrix P on the host, or P_dev on the device).
 * This componentwise-scaled backward error is meaningful in the presence of penalty rows (1e15-sized admittance entries,
 * src/Helmholtz.jl:151-156), where ||L(omega) v|| / ||v|| is not. */
int wae_eig_residuals(wae_family *h, int32_t n, const double *coeff_table, const double *P, uint64_t P_dev, double *res_out);

/* -- Beyn moments with snapshot-projection initial guesses -----------------------------------------------------
 * The solutions X(z) = L(z)^{-1} V along a contour form a low-dimensional manifold (a handful of poles near the
 * contour plus a smooth part) -- the observation behind the reference's `generate_subspace`/`project`
 * (src/NLEVP/beyn.jl:429-560).  Here it accelerates the integrand evaluation of `beyn`/`compute_moment_matrices`
 * (src/NLEVP/beyn.jl:62-71,253-259) itself, without changing its result: a few quadrature points are solved from a
 * zero guess and kept as snapshots (mode 0); for all other points (mode 1) every system starts from the Galerkin
 * projection of its solution on the per-column span of the snapshots and multigrid-GMRES only has to supply the rest,
 * to the same tolerance relative to the same right-hand side.
 *   nbasis: capacity of the snapshot store in snapshots (each d x l complex, interleaved [row][column]).
 *   mode 0: solve the npts points, accumulate their moment contributions and append their solutions to the store
 *           (slot0 = number of snapshots already there; 0 starts a new basis).  Progressive: a chunk of points starts
 *           from the projection on the snapshots taken before it, so pass the points in a spread-out order.
 *   mode 1: the store holds slot0 raw snapshots (e.g. all-gathered from several GPUs): orthonormalise them per
 *           column (in place), project every term, then process the npts points with projected initial guesses.
 *   mode 2: as mode 1 with the basis as mode 0 calls left it (no rebuild).
 *   mode 3: solve the npts points from ZERO guesses, accumulate their moment contributions and write their solutions RAW into the
 *           store slots slot0 .. slot0+npts-1; the handle's basis is not touched.  (A multi-GPU rank's share of the snapshot
 *           points as full-width batches; another rank -- or mode 4 -- builds the basis.)
 *   mode 4: the store holds slot0 raw snapshots of THIS call's l columns: orthonormalise them per column (in place) and project
 *           every term that has a non-zero coefficient in the table (npts rows) -- then return: no system is solved, the
 *           moments are not touched.  With mode 3 and the exchanges of wae_rb_export / wae_rb_import this is the "hybrid" split
 *           of the snapshot phase over G GPUs: points for the solves, probe columns for the basis.
 *   (Environment WAE_RB_ENRICH=<n>: in modes 1/2 append a chunk of points that still needed more than n iterations to
 *   the basis while the store has room.  Off by default: it did not pay on the benchmark contour.)
 *   Q_dev : device pointer of the snapshot store, or 0 for a store owned by the handle; a caller-owned store is
 *           what a multi-GPU driver all-gathers between modes 0 and 1.
 *   accumulate != 0: add to the moments already in out_dev instead of zeroing them first (requires out_dev).
 *   V     : in mode 2 V may be NULL: the probe matrix of the mode 0/1 call that started the basis (kept on the device) is
 *           used again, which saves the second host-to-device copy of a pass.  Not after wae_rb_import.
 * Everything else as wae_beyn_moments.
 *   l_total, col0: the moment tensor has l_total columns and V holds columns col0 .. col0+l-1 of the probe matrix
 *           (l_total <= 0: l_total = l, col0 = 0).  A multi-GPU driver lets every rank take ALL snapshot points for its
 *           own slice of the probe columns (mode 0 stays progressive and leaves a finished basis for that slice), then
 *           exchanges the bases: wae_rb_export / all-gather / wae_rb_import, and runs mode 2 on its share of the points. */
int wae_beyn_moments_rb(wae_family *h, int32_t npts, const double *z, const double *w, const double *coeff_table, const double *V,
                        int32_t l, int32_t K, double tol, int32_t maxit, int32_t mode, int32_t nbasis, int32_t slot0, uint64_t Q_dev,
                        double *A_out, uint64_t out_dev, int32_t accumulate, int32_t l_total, int32_t col0, wae_solve_info *info);
/* The snapshot basis of the handle, host side: S vectors per column, l columns, nk projected terms kact[0..nk-1];
 * Hk dense [ki][s][i][c] (= q_i^H A_k q_s of column c's basis, c fastest), g [i][c] (= q_i^H v_c); complex interleaved.
 * export: pass NULL arrays to query the sizes first.  import: installs a basis whose vectors lie in Q_dev
 * (S x d x l, interleaved [row][column], orthonormal per column) for mode 2. */
int wae_rb_export(wae_family *h, int32_t *S_out, int32_t *l_out, int32_t *nk_out, int32_t *kact_out, double *Hk_out, double *g_out);
int wae_rb_import(wae_family *h, int32_t S, int32_t l, uint64_t Q_dev, int32_t nk, const int32_t *kact, const double *Hk, const double *g);

/* -- shift-invert Arnoldi factorisation for (A, M), A = sum cA_k A_k, M = sum cM_k A_k -----------------
 * The device half of `Arpack.eigs(A,M,nev=nev,sigma=0,v0=v0)` and of the adjoint call on (A',M')
 * (Householder.jl:100-101, iterative_solvers.jl:132-133):  m steps of Arnoldi on  op(A)^{-1} op(M)
 * started from v0, every step one multigrid-GMRES solve on the device:
 *      op(A)^{-1} op(M) V[:,0:m] = V[:,0:m+1] H ,   V^H V = I.
 * The small (m x m) Hessenberg eigenproblem, Ritz extraction and restarts stay on the host side
 * (Julia LinearAlgebra / numpy), as ARPACK's do.  op = WAE_OP_N (right) or WAE_OP_C (left: A^H, M^H).
 *   H_out  (m+1) x m column-major complex;  V_out  d x (m+1) column-major complex.
 *   If an invariant subspace ends the recurrence after j < m steps, the remaining columns of H_out / V_out
 *   are zero (H[j+1,j] = 0 marks the end) and the call still returns WAE_OK.
 */
int wae_arnoldi_shiftinvert(wae_family *h, const double *coeffsA, const double *coeffsM, int32_t m,
                            const double *v0, int32_t op, double tol, int32_t maxit, double *H_out,
                            double *V_out, wae_solve_info *info);
/* The same for nsys operator pairs at once, all Arnoldi processes advancing in lock-step (one batched solve per step):
 * refining all the estimates a Beyn solve returned costs about as much as refining one, because a single-column solve
 * is latency-bound.  coeffsA, coeffsM: nsys x T; v0: d x nsys column-major; H_out: nsys blocks of (m+1) x m;
 * V_out: nsys blocks of d x (m+1), column-major.  A column whose Krylov space becomes invariant stops (its later H
 * entries and basis vectors are zero).  ritz_tol > 0: stop as soon as the dominant Ritz pair of every process has a
 * relative residual |h_{k+1,k}| |y_k| / |theta| <= ritz_tol (the H columns of the steps not taken are zero, their basis
 * vectors in V_out are NOT written -- 128 MB of host memory each at 1M DoF and 8 systems; pass zeroed or scratch storage);
 * the inner solves of the later steps are then relaxed as the Ritz residual falls (inexact Arnoldi: step k is solved to
 * tol / (10 x relative Ritz residual after step k-1), at most 1e-3).  0: always m steps, every solve to tol. */
int wae_arnoldi_shiftinvert_batch(wae_family *h, int32_t nsys, const double *coeffsA, const double *coeffsM, int32_t m, const double *v0,
                                  int32_t op, double tol, int32_t maxit, double ritz_tol, double *H_out, double *V_out,
                                  wae_solve_info *info);

/* -- adjoint perturbation recurrence -----------------------------------------------------------------
 * Replaces `perturb` / `perturb_disk` / `perturb_norm` (perturbation.jl:319-367,374-444,487-560) for a
 * two-parameter expansion L(m,n) = d^m/dλ^m d^n/dε^n L /(m! n!):
 *   coeff_table[(m*(N+1)+n)*T + k]  = coefficient of term k in L(m,n), m,n = 0..N  (0 where m+n>N)
 *   v0, v0adj   base eigenvectors (un-normalised as the reference receives them)
 *   norm_mode   0: perturb (no `c` normalisation)  1: perturb_disk  2: perturb_norm with Y = sum cY_k A_k;
 *               +16: eigenvalue series only (skip the solve at order N; what householder/mslp need, Householder.jl:115-116)
 * Outputs lambda_out[N+1] (entry 0 untouched, the wrappers overwrite it: LinOpFam.jl:555), v_out d x (N+1).
 * wae_perturb and wae_perturb_slots are the nsys = 1 form of wae_perturb_batch (below): one recurrence in the library serves all four.
 * What the single-pair calls keep of their own: with norm_mode + 16 they still return v_0 .. v_{N-1} in v_out (column N is not written:
 * it keeps what the caller passed; at N = 0, v_0 is written), and their work space stays in the family between calls.  If the
 * normalisation of the pair or an eigenvalue coefficient is not finite the call returns WAE_ERR_NAN (lambda_out holds the coefficients
 * found before that, zeros after); otherwise WAE_OK, or WAE_WARN_MAXITER / WAE_WARN_STAGNATION if an inner solve ended above tol.
 */
int wae_perturb(wae_family *h, const double *coeff_table, int32_t N, const double *v0, const double *v0adj,
                int32_t norm_mode, const double *coeffsY, double tol, int32_t maxit, double *lambda_out,
                double *v_out, wae_solve_info *info);

/* -- device-resident multivectors ("slots") for the Newton-type solvers ------------------------------------------
 * `householder` (Householder.jl:70-192) iterates, per start value, on a right and a left eigenvector estimate: every Newton step
 * runs two shift-invert Arnoldi processes from them (Householder.jl:100-101), forms the Ritz vectors, and feeds both to the
 * perturbation step (Householder.jl:115-116, perturbation.jl:319-367).  Through wae_arnoldi_shiftinvert_batch / wae_perturb those
 * vectors cross the host boundary five times per step; with slots they stay in HBM from the first step to the last.
 * A family owns WAE_NSLOTS slots; a slot holds d x ncols complex numbers (column-major for the caller, stored in the library's row
 * numbering).  All arrays of column indices are 0-based.
 *   wae_slot_write   (re)creates the slot with ncols_total columns if it has a different column count (new columns are zero) and
 *                    copies X (d x ncols, column-major, host) into columns col0 .. col0+ncols-1.  ncols = 0: create / resize only.
 *   wae_slot_read    copies columns col0 .. col0+ncols-1 to X (host).
 *   wae_slot_axpby   dst[:, dst_cols[i]] = alpha[i] * src[:, src_cols[i]] + beta[i] * dst[:, dst_cols[i]],  i < n, one after the other
 *                    (alpha, beta: n complex numbers; src and dst may be the same slot and column: a scaling; conj_src != 0: the
 *                    conjugate of the source column is used).  The relaxed update of Householder.jl:173-176; with conj_src the left
 *                    start vectors conj(v0) of Householder.jl:84-86 from the right ones.  beta[i] == 0 overwrites: the destination
 *                    column is not read (BLAS convention), so what it held -- a NaN included -- does not matter.
 *   wae_slot_forms   out[i] = a_i^H op(sum_k coeffs[i][k] A_k) b_i  for n pairs of columns a_i = slot a[:, a_cols[i]], b_i likewise
 *                    (coeffs: n x T): the normalisations v^H M v and v_adj^H L'(z) v of Householder.jl:189-190 without moving a vector.
 *   wae_arnoldi_shiftinvert_slots   wae_arnoldi_shiftinvert_batch with the start vectors taken from slot columns v0_cols[0..nsys-1] and
 *                    the basis KEPT on the device (only H_out comes back): the caller solves the small Hessenberg eigenproblems and
 *   wae_arnoldi_ritz_to_slot   writes  sum_j y[s][j] v_j^(s)  (y: nsys x ny complex, ny <= steps taken + 1; normalise != 0: scaled to
 *                    unit 2-norm) of the basis of the LAST wae_arnoldi_shiftinvert_slots call (same nsys) into dst[:, dst_cols[s]].
 *   wae_perturb_slots   wae_perturb with v0 = slot v[:, v_col], v0adj = slot vadj[:, vadj_col]; v_out may be NULL (eigenvalue series
 *                    only: what householder / mslp need).
 * Both Arnoldi entries: with ritz_tol > 0 a start column that is not close to an eigenvector (||M^-1 op(A) v0|| > 0.1 ||v0||, M^-1 the
 * multigrid cycle: known before the first solve) is first replaced by one step of inverse iteration from it, solved to 1e-3 -- the
 * process then starts from that vector (V[:,0] is the replaced start). */
#define WAE_NSLOTS 8
int wae_slot_write(wae_family *h, int32_t slot, int32_t ncols_total, int32_t col0, int32_t ncols, const double *X);
int wae_slot_read(wae_family *h, int32_t slot, int32_t col0, int32_t ncols, double *X);
int wae_slot_axpby(wae_family *h, int32_t n, int32_t dst_slot, const int32_t *dst_cols, int32_t src_slot, const int32_t *src_cols,
                   const double *alpha, const double *beta, int32_t conj_src);
int wae_slot_forms(wae_family *h, int32_t n, const double *coeffs, int32_t op, int32_t a_slot, const int32_t *a_cols, int32_t b_slot,
                   const int32_t *b_cols, double *out);
int wae_arnoldi_shiftinvert_slots(wae_family *h, int32_t nsys, const double *coeffsA, const double *coeffsM, int32_t m, int32_t v0_slot,
                                  const int32_t *v0_cols, int32_t op, double tol, int32_t maxit, double ritz_tol, double *H_out,
                                  wae_solve_info *info);
int wae_arnoldi_ritz_to_slot(wae_family *h, int32_t nsys, int32_t ny, const double *y, int32_t dst_slot, const int32_t *dst_cols,
                             int32_t normalise);
int wae_perturb_slots(wae_family *h, const double *coeff_table, int32_t N, int32_t v_slot, int32_t v_col, int32_t vadj_slot, int32_t vadj_col,
                      int32_t norm_mode, const double *coeffsY, double tol, int32_t maxit, double *lambda_out, double *v_out,
                      wae_solve_info *info);

/* -- batched adjoint perturbation -----------------------------------------------------------------------------------
 * The recurrence behind wae_perturb (perturbation.jl:319-367,374-444,487-560; the wrappers LinOpFam.jl:546-618) for nsys eigenpairs in
 * lock-step: what a user does with the handful of modes a Beyn solve returned (expand each of them in tau, n, ...).  Every system has
 * its own base eigenvalue and parameter point -- its own coefficient table --, its own right and left vector; per order the library
 * runs ONE tall-skinny product, ONE multi-input operator product and ONE lock-step solve with nsys coefficient sets for the whole
 * batch, where nsys calls of wae_perturb run nsys one-column solves one after another.
 *   nsys          1 .. the solver batch width (opts[6] of wae_solver_setup); anything else: WAE_ERR_INVALID.  nsys = 1 is what
 *                 wae_perturb runs.
 *   coeff_tables  nsys tables, each laid out as wae_perturb's coeff_table, one after the other
 *   v0, v0adj     d x nsys column-major, host   (wae_perturb_batch)
 *   v_slot, v_cols, vadj_slot, vadj_cols   the same vectors as nsys slot columns each   (wae_perturb_batch_slots)
 *   norm_mode     as in wae_perturb (0, 1, 2; +16: eigenvalue series only); coeffsY: one row of T coefficients shared by all systems
 *   lambda_out    nsys x (N+1) complex, system-major (entry 0 of every row untouched)
 *   v_out         nsys blocks of d x (N+1), column-major; may be NULL; NOT written with norm_mode + 16
 *   status_out    (may be NULL) one code per system: WAE_OK, WAE_WARN_MAXITER (an inner solve of that system ended above tol), or
 *                 WAE_ERR_NAN (its normalisation or an eigenvalue coefficient was not finite: the system is given up, its remaining
 *                 coefficients and vectors are zero).  The columns of a lock-step solve are independent: a system that fails neither
 *                 stops the others nor changes their results.
 *   info          maxima and sums over all systems and orders, as in wae_beyn_moments_mgpu
 * Returns WAE_OK, or WAE_WARN_MAXITER / WAE_WARN_STAGNATION if any status is not WAE_OK.  All work space -- d*(N+1)*nsys for the
 * series, d*T*nsys input columns and five vectors of d*nsys -- is allocated by the call and released when it returns. */
int wae_perturb_batch(wae_family *h, int32_t nsys, const double *coeff_tables, int32_t N, const double *v0, const double *v0adj,
                      int32_t norm_mode, const double *coeffsY, double tol, int32_t maxit, double *lambda_out, double *v_out,
                      int32_t *status_out, wae_solve_info *info);
int wae_perturb_batch_slots(wae_family *h, int32_t nsys, const double *coeff_tables, int32_t N, int32_t v_slot, const int32_t *v_cols,
                            int32_t vadj_slot, const int32_t *vadj_cols, int32_t norm_mode, const double *coeffsY, double tol,
                            int32_t maxit, double *lambda_out, double *v_out, int32_t *status_out, wae_solve_info *info);

/* -- P1 assembly on the device (input production) ------------------------------------------------
 * Mass and stiffness matrices of the P1 tetrahedral discretisation, as `discretize` assembles them for the "interior"
 * domain (src/Helmholtz.jl:405-441 with the element kernels src/FEM/FEM.jl:704-710,1745-1766):
 *     M_ab += |det J|/120 (1 + delta_ab),      K_ab += -c_tet^2 |det J|/6 grad(phi_a).grad(phi_b)
 * points: 3 doubles per point (x,y,z); tets: 4 point indices (0-based) per tetrahedron; c_tet: speed of sound per
 * tetrahedron (NULL = 1).  Triplets are sorted and summed on the device (hipCUB), deterministic, no atomics.  The two
 * matrices share one CSR pattern (rowptr npoints+1, col nnz; real values).  wae_p1_assemble returns a handle, wae_p1_info
 * the sizes, wae_p1_get copies the arrays out (any pointer may be NULL), wae_p1_free releases it. */
int wae_p1_assemble(int32_t device, int64_t npoints, const double *points, int64_t ntets, const int32_t *tets, const double *c_tet, void **out);
/* The other two operators of `discretize` for a P1 Helmholtz problem, same pipeline and same handle type (wae_p1_info /
 * wae_p1_get / wae_p1_free; the values come back in the `mass` array of wae_p1_get, `stiff` is zero):
 *  - admittance boundary (src/Helmholtz.jl:443-463 with src/FEM/FEM.jl:9-20,435-441): per boundary triangle
 *        b_ab = c_tri |(x0-x2) x (x1-x2)| (1 + delta_ab) / 24 ;   the operator term is  C = -i b  (Helmholtz.jl:459).
 *    tris: 3 point indices (0-based) per triangle, c_tri: speed of sound of the tetrahedron behind each (NULL = 1).
 *  - flame (src/Helmholtz.jl:292-344,464-487 with FEM.jl:2429-2431,2442-2448): Q = sum over the flame tetrahedra of S (x) g,
 *        S_a = |det J|/24 on the four nodes of a flame tetrahedron,   g_b = -nlocal grad(phi_b).n_ref on the reference
 *        tetrahedron,   nlocal = nglobal_scaled / V_flame  (the caller passes (gamma-1)/rho * Q02U0, Helmholtz.jl:325; the
 *        flame volume is summed on the device and returned in volume_out if not NULL).
 *    flame_tets: indices into tets of the nflame flame tetrahedra; ref_tet: index of the tetrahedron that contains the
 *    reference point (Meshutils.jl:800-816 finds it; that search stays on the host); n_ref: 3 doubles. */
int wae_p1_assemble_boundary(int32_t device, int64_t npoints, const double *points, int64_t ntris, const int32_t *tris, const double *c_tri, void **out);
int wae_p1_assemble_flame(int32_t device, int64_t npoints, const double *points, int64_t ntets, const int32_t *tets, int64_t nflame,
                          const int32_t *flame_tets, int32_t ref_tet, const double *n_ref, double nglobal_scaled, void **out, double *volume_out);
int wae_p1_info(const void *handle, int64_t *npoints, int64_t *nnz);
int wae_p1_get(const void *handle, int32_t *rowptr, int32_t *col, double *mass, double *stiff);
int wae_p1_free(void *handle);
/* -- P2 (second-order) assembly on the device: `discretize(...; order=:quad)` ----------------------------------------
 * Edge numbering (replaces aggregate_elements, src/FEM/FEM.jl:84-116, with collect_lines!, Meshutils.jl:831-840): one DoF per
 * unique mesh edge, DoF of edge e = npoints + e, the edges sorted by (smaller point, larger point) -- the reference's order for
 * meshes whose simplices list their points in ascending order.  Edge keys, radix sort, unique pass and the binary searches run on
 * the device.  Local node order, as in the reference: tetrahedron = its 4 points, then the edges (1,2), (1,3), (1,4), (2,3), (2,4),
 * (3,4); triangle = its 3 points, then the edges (1,2), (1,3), (2,3).  tets: 4 point indices (0-based) per tetrahedron, tris: 3 per
 * boundary triangle (ntris may be 0, tris NULL).  wae_p2_connectivity returns a handle, wae_p2_connectivity_info the sizes,
 * wae_p2_connectivity_get copies out edges[2*nedges], tets10[10*ntets], tris6[6*ntris] (0-based; any pointer may be NULL),
 * wae_p2_connectivity_free releases it.  WAE_ERR_INVALID: an index outside 0..npoints-1, a triangle edge that is no tetrahedron's
 * edge, or a mesh with 100*ntets or 36*ntris beyond a 32-bit count (the limit of the assembly below; nothing is truncated). */
int wae_p2_connectivity(int32_t device, int64_t npoints, int64_t ntets, const int32_t *tets, int64_t ntris, const int32_t *tris, void **out);
int wae_p2_connectivity_info(const void *handle, int64_t *nedges, int64_t *ntets, int64_t *ntris);
int wae_p2_connectivity_get(const void *handle, int32_t *edges, int32_t *tets10, int32_t *tris6);
int wae_p2_connectivity_free(void *handle);
/* The embedding of the P1 space of the mesh into its P2 space (a P1 function at the P2 nodes; the coarse space of p-coarsening, a
 * prolongator wae_solver_setup_nested takes) as a CSR matrix, built by a kernel from the handle's edge list: npoints + nedges rows,
 * npoints columns, npoints + 2 nedges entries (ptr: rows + 1; 0-based); the row of point a holds (a, 1.0), the row of edge (a, b), a < b,
 * holds (a, 0.5) (b, 0.5).  WAE_ERR_INVALID, nothing written: a NULL pointer, or npoints other than the handle's. */
int wae_p2_embedding(const void *handle, int64_t npoints, int32_t *ptr, int32_t *col, double *val);
/* The three operators on the P2 space, basis phi_i = l_i (2 l_i - 1) on the points and phi_ij = 4 l_i l_j on the edges (l:
 * barycentric coordinates), node order and numbering as above.  Each entry takes the plain mesh, numbers the edges itself and
 * returns the handle type of the P1 entries (wae_p1_info / wae_p1_get / wae_p1_free) with npoints + nedges rows; same pipeline:
 * triplets sorted and summed on the device, deterministic, no atomics.
 *  - interior (src/Helmholtz.jl:120-149,405-441 with the element matrices s43v2u2 / s43nv2nu2, FEM.jl:726-738,1768-):
 *        M_ab += |det J| int phi_a phi_b,      K_ab += -c_tet^2 |det J| int grad(phi_a).grad(phi_b)     (c_tet NULL = 1)
 *  - admittance boundary (Helmholtz.jl:151-170,443-463 with s33v2u2, FEM.jl:442-450): b_ab = c_tri |(x0-x2) x (x1-x2)| int phi_a phi_b
 *    on the 6-node triangle; the operator term is C = -i b.  The tetrahedra are needed for the edge numbers.
 *  - flame (Helmholtz.jl:292-344,464-487 with s43v2 / s43nv2rx, FEM.jl:2433-2435,2450-2484): Q = sum over the flame tetrahedra of
 *    S (x) g,  S_a = |det J| int phi_a (-|det J|/120 on points, |det J|/30 on edges),  g_b = -nlocal grad(phi_b)(x_ref).n_ref on the 10
 *    nodes of the reference tetrahedron, nlocal = nglobal_scaled / V_flame.  Unlike P1 the gradients depend on where x_ref (3
 *    doubles) lies inside ref_tet.  The flame volume is returned in volume_out if not NULL. */
int wae_p2_assemble(int32_t device, int64_t npoints, const double *points, int64_t ntets, const int32_t *tets, const double *c_tet, void **out);
int wae_p2_assemble_boundary(int32_t device, int64_t npoints, const double *points, int64_t ntets, const int32_t *tets, int64_t ntris,
                             const int32_t *tris, const double *c_tri, void **out);
int wae_p2_assemble_flame(int32_t device, int64_t npoints, const double *points, int64_t ntets, const int32_t *tets, int64_t nflame,
                          const int32_t *flame_tets, int32_t ref_tet, const double *x_ref, const double *n_ref, double nglobal_scaled, void **out,
                          double *volume_out);
/* -- Hermite (cubic) assembly on the device: `discretize(...; order=:herm)` ------------------------------------------
 * The element (aggregate_elements, src/FEM/FEM.jl:117-160; recombine_hermite, FEM.jl:171-336): P3 on the tetrahedron p0..p3, 20 DoF, the
 * basis dual to  u(p_k) (local 0..3, global p_k),  du/dx, du/dy, du/dz at p_k (local 4..7, 8..11, 12..15, global N + p_k, 2N + p_k,
 * 3N + p_k; N = npoints; physical gradients, not reference ones),  u at the centroid of the face opposite p_k (local 16..19, global
 * 4N + face number).  Boundary triangle: the trace, 13 DoF -- 3 values, the x, y, z derivatives at the 3 points, the face value.
 * Face numbering (collect_triangles, FEM.jl:49-68): the boundary triangle at position t of `tris` is face t; every tetrahedron face that
 * is not in `tris` (interior, or a boundary face the caller did not list) follows as ntris + rank, the rank ascending by (largest point,
 * middle point, smallest point); ndof = 4N + ntris + ninner.  With `tris` in the reference's sorted order this is its numbering.  Face
 * keys, radix sort, unique pass, scan and the binary searches run on the device, without atomics: the same bits on every call.
 * wae_herm_connectivity returns a handle, wae_herm_connectivity_info the sizes, wae_herm_connectivity_get copies out faces[3*ninner]
 * (each as smallest, middle, largest point), tets20[20*ntets], tris13[13*ntris] (0-based; any pointer may be NULL),
 * wae_herm_connectivity_free releases it.  WAE_ERR_INVALID, nothing written: an index outside 0..npoints-1, a boundary triangle that is
 * no tetrahedron's face, a triangle listed twice, a face shared by more than two tetrahedra, 400*ntets or 169*ntris beyond a 32-bit
 * count, or npoints > 2^21 = 2097152: the 64-bit face key holds three point numbers, larger meshes are refused, never truncated. */
int wae_herm_connectivity(int32_t device, int64_t npoints, int64_t ntets, const int32_t *tets, int64_t ntris, const int32_t *tris, void **out);
int wae_herm_connectivity_info(const void *handle, int64_t *ninner, int64_t *ntets, int64_t *ntris, int64_t *ndof);
int wae_herm_connectivity_get(const void *handle, int32_t *faces, int32_t *tets20, int32_t *tris13);
int wae_herm_connectivity_free(void *handle);
/* The three operators on the Hermite space.  Each entry takes the plain mesh and numbers the faces itself -- `tris` is always part of
 * that numbering (ntris may be 0 for the interior and the flame) -- and returns the handle type of the P1 entries (wae_p1_info /
 * wae_p1_get / wae_p1_free) with ndof rows; triplets sorted and summed on the device, deterministic, no atomics.  With x = p3 + J xi,
 * J[:, j] = p_j - p_3 (CooTrafo, FEM.jl:9-21), the function of d/dx_i at p_k is sum_j J[i][j] (reference function of d/dxi_j at p_k);
 * the entries of J keep their sign, the measure is |det J|: a tetrahedron listed with det J < 0 is legal.  The reference-element
 * tensors come from a table generated in exact rational arithmetic from this definition (dev/gen_herm_tables.py).
 *  - interior (src/Helmholtz.jl:120-149,405-441):
 *        M_ab += |det J| int phi_a phi_b,      K_ab += -c_tet^2 |det J| int grad(phi_a).grad(phi_b)     (c_tet NULL = 1)
 *  - admittance boundary (Helmholtz.jl:151-170,443-463): b_ab = c_tri |(x0-x2) x (x1-x2)| int phi_a phi_b on the 13-DoF triangle, only
 *    the tangential part of a vertex gradient acting; the operator term is C = -i b; the full 13 x 13 coupling stays in the pattern.
 *  - flame (Helmholtz.jl:292-344,464-487): Q = sum over the flame tetrahedra of S (x) g,  S_a = |det J| int phi_a (|det J|/240 on the
 *    values, 0 on the gradients, 3|det J|/80 on the faces),  g_b = -nlocal grad(phi_b)(x_ref).n_ref on the 20 DoF of ref_tet,
 *    nlocal = nglobal_scaled / V_flame; arguments as wae_p2_assemble_flame.
 * Out of scope for Hermite elements: a nodal speed of sound, source vectors, shape sensitivity, Bloch numbering, prolongation across
 * octosplit levels, the tile path.  The solver path of a Hermite family: wae_hermite_prolongators below; sampling a Hermite vector at
 * located points, and carrying it onto another mesh: wae_hermite_locator_set and order 3 of the locator entries below. */
int wae_herm_assemble(int32_t device, int64_t npoints, const double *points, int64_t ntets, const int32_t *tets, int64_t ntris, const int32_t *tris,
                      const double *c_tet, void **out);
int wae_herm_assemble_boundary(int32_t device, int64_t npoints, const double *points, int64_t ntets, const int32_t *tets, int64_t ntris,
                               const int32_t *tris, const double *c_tri, void **out);
int wae_herm_assemble_flame(int32_t device, int64_t npoints, const double *points, int64_t ntets, const int32_t *tets, int64_t ntris,
                            const int32_t *tris, int64_t nflame, const int32_t *flame_tets, int32_t ref_tet, const double *x_ref, const double *n_ref,
                            double nglobal_scaled, void **out, double *volume_out);
/* The p-hierarchy of a Hermite family: two real prolongators that carry it down to P1, for wae_solver_setup_nested (with opts[12] = 1: the
 * set-up's Jacobi weights diverge on a cubic level, lambda_max(D^-1 A) is 5.8 there).  Both CSR, 0-based, columns ascending without
 * duplicates; the faces numbered as in wae_herm_connectivity, by the same device pass.  No atomics: the same bits on every call.
 *   which = 0, P_face, ndof x 4N: row r < 4N is (r, 1); the row of face f with the points a, b, c and the centroid
 *       x_f = ((x_a + x_b) + x_c) / 3 has the 12 entries (p, 1/3) and ((1+i) N + p, (x_f - x_p)_i / 6), p in {a, b, c}, i = 0..2: the
 *       centroid value of the cubic that the nine vertex data fix when quadratics are to be reproduced.  One thread per face.
 *   which = 1, P_lin, 4N x N: row p is (p, 1); row (1+i) N + p is the volume-weighted mean over the tetrahedra t that hold p of the P1
 *       gradient, sum_t |det J_t| d_i lambda_k^t / sum_t |det J_t| at column tets[t][k].  Triplets and weight sums go through the
 *       stable sort and reduce-by-key of the assembly; entries that cancel to zero stay in the pattern; det J < 0 is legal.
 * wae_hermite_prolongators returns a handle, wae_hermite_prolongators_info the sizes of one matrix, wae_hermite_prolongators_get copies it out
 * (ptr[rows + 1], col[nnz], val[nnz]; any pointer may be NULL), wae_hermite_prolongators_free releases it.  Refused with WAE_ERR_INVALID,
 * nothing written: everything wae_herm_connectivity refuses, points == NULL, which outside 0..1, a point that belongs to no
 * tetrahedron (it has no gradient to average), and a point whose tetrahedra all have det J = 0 (its weight sum is 0).
 * (The prefix is wae_hermite_, not wae_herm_: the set of wae_herm_ entries is the assembly's and is pinned as such by its tests.) */
int wae_hermite_prolongators(int32_t device, int64_t npoints, const double *points, int64_t ntets, const int32_t *tets, int64_t ntris,
                          const int32_t *tris, void **out);
int wae_hermite_prolongators_info(const void *handle, int32_t which, int64_t *rows, int64_t *cols, int64_t *nnz);
int wae_hermite_prolongators_get(const void *handle, int32_t which, int32_t *ptr, int32_t *col, double *val);
int wae_hermite_prolongators_free(void *handle);
/* -- uniform mesh refinement on the device: `octosplit(mesh)` with the nested P1 and P2 prolongations ------------------
 * Every tetrahedron is split into 8 and every boundary triangle into 4 (src/Meshutils.jl:589-747); the handle keeps `levels`
 * successive refinements in HBM, level 0 being the input.  points: 3 doubles per point, tets: 4 point indices (0-based) per
 * tetrahedron, tris: 3 per boundary triangle (ntris may be 0, tris NULL).  One level, index for index what the reference returns:
 *  - points (Meshutils.jl:596-601): the old points keep their numbers, the midpoint of edge e is point npoints + e = (x_a + x_b) * 0.5;
 *    the unique tetrahedron edges are ordered as mesh.lines (collect_lines!, Meshutils.jl:831-840, with src/Mesh/sorter.jl:9-31):
 *    ascending by (larger point, smaller point) -- NOT the (smaller, larger) order of wae_p2_connectivity.
 *  - children of a tetrahedron (A,B,C,D) (Meshutils.jl:604-641): the corners [A,AB,AC,AD] [B,AB,BC,BD] [C,AC,BC,CD] [D,AD,BD,CD], then the
 *    inner octahedron cut along the shortest of its diagonals AB-CD, AC-BD, AD-BC, the <= tie-breaks tested in that order:
 *        AB-CD: [AB,CD,AC,AD] [AB,CD,AD,BD] [AB,CD,BD,BC] [AB,CD,BC,AC]
 *        AC-BD: [AC,BD,AB,AD] [AC,BD,AD,CD] [AC,BD,CD,BC] [AC,BD,BC,AB]
 *        AD-BC: [AD,BC,AC,CD] [AD,BC,CD,BD] [AD,BC,BD,AB] [AD,BC,AB,AC]
 *    The vertex order of a child is kept as listed, so the orientation is mixed as in the reference (every assembly here takes |det J|).
 *    The diagonals are compared by d2 = (dx*dx + dy*dy) + dz*dz of the stored midpoints in double, every operation rounded on its own,
 *    so that a host restatement gets the same children.  The reference compares LinearAlgebra.norm, whose rounding is not specified: on
 *    tetrahedra whose two shortest diagonals are equal or within a rounding (85 of the 3380 of the tutorial Rijke tube) the package may cut
 *    along another diagonal.
 *  - children of a triangle (A,B,C) (Meshutils.jl:645-654): [A,AB,AC] [B,AB,BC] [C,AC,BC] [AB,AC,BC].
 *  - list order (insert_smplx!, sorter.jl:141-150): ascending by "vertices sorted descending, compared lexicographically", which
 *    find_smplx (a binary search) and the choice of a flame's reference tetrahedron rely on.  tet_labels[8 t + k] / tri_labels[4 s + k] is the
 *    position of child k (in the order above) of parent t / s in the new list (Meshutils.jl:670-722, 0-based here).
 * Edge keys, radix sorts, unique pass and binary searches run on the device (hipCUB), deterministic, no atomics; between two levels only
 * the edge count and the error flags cross the bus.
 * wae_octosplit returns a handle (levels >= 1), wae_octosplit_info the sizes of a level, wae_octosplit_get copies a level out:
 * points[3*npoints], tets[4*ntets], tris[3*ntris], parents[2 per NEW point of this level: (larger, smaller) end of its edge, in the
 * numbers of level - 1], tet_labels[8 per tetrahedron of level - 1], tri_labels[4 per triangle of level - 1]; any pointer may be NULL,
 * and the last three must be NULL for level 0.  wae_octosplit_free releases the handle.
 * wae_octosplit_prolong: the nested P1 embedding from_level < to_level applied level by level to ncols complex columns (X:
 * npoints(from) x ncols column-major, interleaved re/im; Y: npoints(to) x ncols): the rows of old points are copied, the row of a new
 * point is (x[a] + x[b]) * 0.5; one kernel per level, the intermediate levels stay in HBM.
 * wae_octosplit_prolongator: the step from_level -> from_level + 1 of that embedding as a CSR matrix, built by a kernel from the parents
 * table in HBM: npoints(from_level + 1) rows in the order of the finer level's points, 2 npoints(from_level + 1) - npoints(from_level)
 * entries (ptr: rows + 1, col and val: entries; 0-based); row a < npoints(from_level) holds (a, 1.0), the row of a new point holds
 * (parent, 0.5) twice, columns ascending.  These are the prolongators wae_solver_setup_nested takes.
 * WAE_ERR_INVALID, nothing returned and nothing truncated: an index outside 0..npoints-1, a triangle edge that is no tetrahedron's
 * edge, two equal children after the sort (a simplex listed twice or repeating a point), levels < 1, or a level whose point,
 * tetrahedron or triangle count passes a 32-bit index.
 * P2 prolongation.  The P2 unknowns of a level are those of wae_p2_assemble on its mesh: the points, then the edges ascending by (smaller
 * point, larger point).  The step level -> level + 1 evaluates the coarse basis (l_i (2 l_i - 1), 4 l_i l_j) at the fine unknowns: a real
 * CSR matrix with ndof(level + 1) rows and ndof(level) columns, five kinds of row with exact weights, every row summing to 1:
 *      old point a                                 (a, 1)
 *      new point, midpoint of the coarse edge AB   (edge AB, 1)
 *      fine edge (A, AB)                           (A, 3/8) (B, -1/8) (edge AB, 3/4)
 *      fine edge (AB, AC)                          (B, -1/8) (C, -1/8) (edge AB, 1/2) (edge AC, 1/2) (edge BC, 1/4)
 *      fine edge (AB, CD), an inner diagonal       the four points -1/8, the six edges among them 1/4
 * columns ascending.  The first of the three P2 entries called on a handle numbers the edges of every level on the device (keys, sort and
 * unique pass of wae_p2_connectivity) and builds every step in HBM (row lengths by kind, an exclusive scan, one thread per row; binary
 * searches in the coarse edge list, no atomics); a handle that never sees one pays nothing.
 * wae_octosplit_p2_info: nedges and ndof = npoints + nedges of a level, prolongator_nnz of the step level -> level + 1 (0 for the last
 * level); any pointer may be NULL.  wae_octosplit_prolongator_p2 copies the step from_level -> from_level + 1 out (ptr: ndof(from_level +
 * 1) + 1, col and val: prolongator_nnz; 0-based), in the form wae_solver_setup_nested takes.  wae_octosplit_prolong_p2 applies the same
 * arrays, level by level, to ncols complex columns (X: ndof(from_level) x ncols column-major, interleaved re/im; Y: ndof(to_level) x
 * ncols); one kernel per level, the intermediate levels stay in HBM.  WAE_ERR_INVALID, nothing written: a level out of range, from_level
 * >= to_level, ncols < 1, a NULL pointer, or a level whose unknowns or whose step's entries pass a 32-bit index.
 * Out of scope: meshes with a degree of symmetry (the point classes of a Bloch unit cell do not survive appended points; the reference
 * drops `dos` too), interior-triangle lists (a TODO in the reference, Meshutils.jl:656-668), and Hermite prolongation. */
int wae_octosplit(int32_t device, int64_t npoints, const double *points, int64_t ntets, const int32_t *tets, int64_t ntris, const int32_t *tris,
                  int32_t levels, void **out);
int wae_octosplit_info(const void *handle, int32_t level, int64_t *npoints, int64_t *ntets, int64_t *ntris);
int wae_octosplit_get(const void *handle, int32_t level, double *points, int32_t *tets, int32_t *tris, int32_t *parents, int32_t *tet_labels,
                      int32_t *tri_labels);
int wae_octosplit_prolong(const void *handle, int32_t from_level, int32_t to_level, int32_t ncols, const double *X, double *Y);
int wae_octosplit_prolongator(const void *handle, int32_t from_level, int32_t *ptr, int32_t *col, double *val);
int wae_octosplit_p2_info(void *handle, int32_t level, int64_t *nedges, int64_t *ndof, int64_t *prolongator_nnz);
int wae_octosplit_prolongator_p2(void *handle, int32_t from_level, int32_t *ptr, int32_t *col, double *val);
int wae_octosplit_prolong_p2(void *handle, int32_t from_level, int32_t to_level, int32_t ncols, const double *X, double *Y);
int wae_octosplit_free(void *handle);
/* -- point location in a tetrahedral mesh and sampling of P1 / P2 / Hermite vectors there, on the device --------------------------
 * find_tetrahedron_containing_point (src/Meshutils.jl:800-815) and get_p / get_n_grad_p (src/FEM/helmholtz_getters.jl:7-45) for many
 * points at once.  wae_locator_create keeps the mesh (points: 3 doubles per point, tets: 4 point indices per tetrahedron, 0-based) and a
 * uniform cell grid over it in HBM; every pointer of these entries is a host pointer.
 *  - containment: the barycentric coordinates of x by Cramer's rule on J = [p1-p4, p2-p4, p3-p4], the fourth 1 - sum, every operation
 *    rounded on its own in double (a float64 host restatement gets the same bits), independent of the sign of det J.  A tetrahedron
 *    contains x if all four are >= -tol, 0 <= tol <= 1e-6 (tol = 0: the reference's all(0 .<= xi .<= 1)); wae_locator_find returns the
 *    LOWEST such index in list order in tet[q], -1 if there is none, and in lambda (4 per point, may be NULL) the coordinates that
 *    decided, NaN for -1.
 *  - cells: the bounding box of the points (block reduction), a grid of about ntets / cell_target cells over it (cell_target = 0: 8), as
 *    cubical as the box allows, at most 1024 per axis and 8 ntets in all (every dim is halved until that holds).  Every tetrahedron is listed in the cells that its bounding box, grown per axis by
 *    (4e-6 + 2^-30) times the extent of the mesh, overlaps; a point's cell and a box corner's cell come from the same expression
 *    clamp(floor((x - lo) * (dim / (hi - lo))), 0, dim - 1), which is monotone in x under rounding, so the list of a point's cell holds
 *    every tetrahedron the rule can accept.  Count, exclusive scan, stable radix sort by cell (hipCUB): the tetrahedra ascend within a
 *    cell, a query stops at its first hit.  More than 32 ntets pairs: every dim is halved and the pairs recounted, down to one cell.  No
 *    atomics; the same input gives the same indices and bits on every call.  A point outside the box grown by the same amount (no
 *    tetrahedron can accept it) is -1 without a look at the cells; a point in the rim between the two boxes or on an upper face of
 *    the box belongs to the first or last cell of the axis.
 * wae_locator_info: the sizes, dims[3], nrefs = the (cell, tet) pairs, max_per_cell = the longest list; any pointer may be NULL.
 * wae_locator_set_p2: the P2 unknowns of every tetrahedron (tets10: 10 per tetrahedron as wae_p2_connectivity_get gives them: the 4
 * points, then the edges (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)), ndof = npoints + nedges; needed before any call with order 2.
 * wae_hermite_locator_set: the Hermite unknowns of every tetrahedron (tets20: 20 per tetrahedron as wae_herm_connectivity_get gives
 * them for the boundary triangles the family was assembled with: b * npoints + point k at 4 b + k, b = 0 the value, b = 1..3 the x, y, z
 * derivative, then 4 npoints + the number of the face opposite point k), ndof = 4 npoints + nfaces; needed before any call with order 3 (until
 * then order 3 is refused like any unknown order, "order must be 1 or 2").  A
 * second call replaces the table; a refused one keeps nothing and leaves the table of an earlier call untouched.
 * wae_locator_weights: the rows of the point functionals, idx / val with 4 (order 1), 10 (order 2) or 20 (order 3) entries per point:
 * kind 0, p(x) = sum val v[idx]: l_i on the points (order 1), l_i (2 l_i - 1) on the points and 4 l_i l_j on the edges (order 2), the
 * functions of the assembled Hermite space in the order of tets20 (order 3: with xi = (l_1, l_2, l_3) the reference functions psi_a(xi), the
 * twelve of the vertex gradients recombined with J = [p1-p4, p2-p4, p3-p4] as w[4 (1 + i) + k] = sum_j J[i][j] psi[4 (1 + j) + k], since the
 * unknowns are physical gradients); kind 1, n . grad p(x):
 * the derivative of those weights along n (3 per point).  tet: the tetrahedron of every point (from wae_locator_find); a row with tet ==
 * -1 has idx 0 and val 0.
 * wae_locator_sample: out[q, c] = sum_i val[q, i] V[idx[q, i], c] in one gather kernel, i ascending, without the weights leaving the
 * device.  V: d x ncols complex column-major (interleaved re/im), d = npoints (order 1) or the ndof of the table (orders 2 and 3); out: nq x ncols complex
 * column-major; a row with tet == -1 is NaN.
 * WAE_ERR_INVALID, nothing launched: a negative count, a tetrahedron index outside 0..npoints-1, a point or query coordinate that is
 * not finite, tol outside [0, 1e-6], a tet outside -1..ntets-1, order 2 before wae_locator_set_p2, order 3 before
 * wae_hermite_locator_set, d different from npoints / ndof, an entry of tets10 outside 0..ndof-1, tets20 == NULL, its ndof below 4 npoints
 * or beyond a 32-bit index, an entry 4 b + k of tets20 that is not b npoints + point k of the tetrahedron, an entry 16..19 outside 4 npoints
 * .. ndof-1, kind 1 with n == NULL, npoints or 32 ntets beyond a 32-bit index.  nq == 0 returns WAE_OK and
 * touches nothing.  Out of scope: Hermite source vectors, nearest-tetrahedron answers outside the mesh, curved geometry, Bloch-expanded fields. */
int wae_locator_create(int32_t device, int64_t npoints, const double *points, int64_t ntets, const int32_t *tets, int64_t cell_target,
                       void **out);
int wae_locator_info(const void *handle, int64_t *npoints, int64_t *ntets, int64_t *dims, int64_t *nrefs, int64_t *max_per_cell);
int wae_locator_find(const void *handle, int64_t nq, const double *x, double tol, int32_t *tet, double *lambda);
int wae_locator_set_p2(void *handle, int64_t ndof, const int32_t *tets10);
int wae_hermite_locator_set(void *locator, int64_t ndof, const int32_t *tets20);
int wae_locator_weights(const void *handle, int32_t order, int32_t kind, int64_t nq, const double *x, const int32_t *tet, const double *n,
                        int32_t *idx, double *val);
int wae_locator_sample(const void *handle, int32_t order, int32_t kind, int64_t nq, const double *x, const int32_t *tet, const double *n,
                       int64_t d, int32_t ncols, const double *V, double *out);
int wae_locator_free(void *handle);
/* -- Bloch unit cells with P1 or P2 elements: cell numbering and operator fold on the device ------------------------
 * `discretize(mesh, dscrp, C; order, b=:b)` on a mesh with a degree of symmetry: blochify (src/Bloch.jl:4-112), the dimension of
 * Helmholtz.jl:107-113.  The mesh is the EXTENDED unit cell: points < naxis lie on the symmetry axis, points >= nsector are image
 * points (the rotated copy of the reference boundary), the twin of image point p is p - (nsector - naxis).  Edge DoFs are those of
 * wae_p2_connectivity (sorted by (smaller point, larger point), DoF of edge e = npoints + e).  The reference computes the twin of a line
 * by a constant shift, relying on the line order of its mesh generator (annular_meshes.jl:459-489); here the twin is FOUND:
 *  - image edge: every endpoint is an image or an axis point and at least one is an image point; its twin is the edge with the image
 *    endpoints shifted by -(nsector - naxis), located by binary search in the sorted edge keys, one thread per edge;
 *  - axis edge: both endpoints are axis points;
 *  - cell numbering: points 0..nsector-1 keep their index, an edge that is no image edge gets nsector + (number of non-image edges
 *    before it) (exclusive scan, hipCUB), image points and image edges get the cell DoF of their twin;
 *    dim = nsector + nedges - nimage_edges.  Image edges need not be the tail of the list: (axis point, image point) sorts early.
 * order: 1 (lin: no edges, the point rule alone) or 2 (quad).  wae_bloch_numbering returns a handle, wae_bloch_numbering_info the
 * sizes (ndof = npoints + nedges), wae_bloch_numbering_get copies out cell_dof[ndof], flags[ndof] (WAE_BLOCH_IMAGE | WAE_BLOCH_AXIS; the
 * axis bit marks axis points and axis edges) and edges[2*nedges] (any pointer may be NULL), wae_bloch_numbering_free releases it.
 * WAE_ERR_INVALID, nothing returned: naxis > nsector, nsector > npoints, more image points than nsector - naxis, a point index out of
 * range, an image edge whose twin is no edge of the mesh (the cell is not periodic; the message counts them), a twin that is an image
 * edge itself, or a mesh beyond the 32-bit limits of wae_p2_connectivity.
 *
 * wae_bloch_fold: a square CSR matrix on the extended numbering (n = ndof rows; rowptr, col, real values v0 and, sharing the
 * pattern, v1 or NULL -- M and K, or the real and imaginary part of a complex operator) -> its nparts parts of dimension dim.  Entry
 * (i, j) goes to (cell_dof[i], cell_dof[j]) of the part  base (image bits of i and j equal), plus (only j an image DoF) or minus
 * (only i); with nparts = 6 the entries with an axis bit on i or j go to the axis / axis-plus / axis-minus parts instead
 * (Bloch.jl:54-104).  nparts = 3: parts 0..2, the axis bits are ignored.  Duplicates created by the fold are summed by the assembly
 * pipeline: key (part, row, column), stable radix sort, reduce-by-key in input order -- no atomics, the same bits on every call.
 * out: nparts handles of the assembly type (wae_p1_info / wae_p1_get / wae_p1_free; v0 comes back as `mass`, v1 as `stiff`); a part
 * without entries is a valid handle with nnz = 0.  WAE_ERR_INVALID, nothing launched: a malformed CSR, an index outside its range in
 * col or cell_dof, an unknown flag bit, nparts not 3 or 6, dim outside 1..n, or nparts * dim beyond a 32-bit index. */
#define WAE_BLOCH_IMAGE 1
#define WAE_BLOCH_AXIS  2
int wae_bloch_numbering(int32_t device, int64_t npoints, int64_t ntets, const int32_t *tets, int64_t nsector, int64_t naxis, int32_t order, void **out);
int wae_bloch_numbering_info(const void *handle, int64_t *ndof, int64_t *dim, int64_t *nedges, int64_t *nimage_edges, int64_t *naxis_edges);
int wae_bloch_numbering_get(const void *handle, int32_t *cell_dof, int32_t *flags, int32_t *edges);
int wae_bloch_numbering_free(void *handle);
int wae_bloch_fold(int32_t device, int64_t n, const int32_t *rowptr, const int32_t *col, const double *v0, const double *v1, const int32_t *cell_dof,
                   const int32_t *flags, int64_t dim, int32_t nparts, void **out);
/* -- nodal speed of sound: K and C of the P1 and P2 spaces from one value per mesh point -----------------------------
 * The second form of `C` in `discretize(mesh, dscrp, C; order)` (src/Helmholtz.jl:43,59-74): length(C) == size(mesh.points, 2), the
 * speed of sound interpolated linearly between the vertices, generate_field(mesh, f; order=:lin).  On every simplex
 *     c(x) = sum_p c_p l_p        (l: barycentric coordinates, c_p = c_point[corner p]; P2 uses the 4 resp. 3 corner points only)
 * and the element matrices are those of `stiff` / `bound` (Helmholtz.jl:120-171: s43nv1nu1cc1, s43nv2nu2cc1, s33v1u1c1, s33v2u2c1),
 * here from the monomial formula  int l^alpha = |det J| alpha! / (|alpha| + n - 1)!  -- exact polynomials, no quadrature:
 *  - interior:  K_ab += -|det J| int c(x)^2 grad(phi_a).grad(phi_b);  M does not depend on c and is that of wae_p1_assemble / wae_p2_assemble.
 *        P1: K_ab = -|det J| (grad l_a . grad l_b) ((sum_p c_p)^2 + sum_p c_p^2) / 120
 *        P2: grad phi_a = sum_k l_k w_a[k]:  K_ab = -|det J| sum_km (w_a[k].w_b[m]) W_km,  W_km = sum_pq c_p c_q int l_k l_m l_p l_q  (/7!)
 *  - admittance boundary:  b_ab = |(x0-x2) x (x1-x2)| int c(x) phi_a phi_b on the triangle, the operator term is C = -i b.
 *        P1: b_aa = |..| (2 c_a + S)/60,  b_ab = |..| (c_a + c_b + S)/120,  S = c_1 + c_2 + c_3  (b_11 = |..| (c_1/20 + c_2/60 + c_3/60))
 *        P2: degree-5 monomials on the 6-node triangle  (/7!)
 * The local K_ab and K_ba, b_ab and b_ba get the same bits.  Arguments, index checks, pipeline (sorted triplets, no atomics, the same bits
 * on every call) and handle type (wae_p1_info / wae_p1_get / wae_p1_free) are those of the per-simplex entry of the same name.
 * c_point: npoints doubles, required: NULL or a value that is not finite returns WAE_ERR_INVALID and nothing is launched.
 * The shape sensitivity with a nodal c: wae_p1_shape_sensitivity_cpoint, wae_p2_shape_sensitivity_cpoint below.  Not covered: Hermite elements. */
int wae_p1_assemble_cpoint(int32_t device, int64_t npoints, const double *points, int64_t ntets, const int32_t *tets, const double *c_point, void **out);
int wae_p1_assemble_boundary_cpoint(int32_t device, int64_t npoints, const double *points, int64_t ntris, const int32_t *tris, const double *c_point,
                                    void **out);
int wae_p2_assemble_cpoint(int32_t device, int64_t npoints, const double *points, int64_t ntets, const int32_t *tets, const double *c_point, void **out);
int wae_p2_assemble_boundary_cpoint(int32_t device, int64_t npoints, const double *points, int64_t ntets, const int32_t *tets, int64_t ntris,
                                    const int32_t *tris, const double *c_point, void **out);
/* -- speaker source vector: `discretize(mesh, dscrp, C; source=true)` with a :speaker domain -------------------------------
 * The second family `rhs` of the reference (src/Helmholtz.jl:251-258,488-505,519-522) holds one sparse vector m = -i s,
 *     s_a = |(x0-x2) x (x1-x2)| int c(x) phi_a   over the triangles of the speaker domain   (wallsrc, divided by i),
 * with the scalar functions of the admittance term and the excitation symbol: rhs(w) = w Y A m, while L gets the w Y C of an admittance
 * boundary.  These entries return the real vector s in dense form (out: npoints doubles; P2: nout = npoints + nedges doubles, and a
 * wrong nout is WAE_ERR_INVALID).  Element vectors from the monomial formula  int l^alpha = |..| alpha! / (|alpha| + 2)! :
 *     P1, c per triangle:  s_a = c |..| / 6                     P1, c per point:  s_a = |..| (c_a/12 + c_b/24 + c_c/24)
 *     P2, c per triangle:  0 on the points, c |..| / 6 on the edges
 *     P2, c per point:     |..| (c_a/60 - c_b/120 - c_c/120) on point a,  |..| (c_i/15 + c_j/15 + c_k/30) on edge (i,j), k the third point
 * (node order and edge numbers: wae_p2_connectivity).  Pipeline and guarantees are those of the boundary-matrix entries of the same space:
 * (node, value) pairs per triangle, sorted and summed on the device, no atomics, the same bits on every call; the same index and argument
 * checks, WAE_ERR_INVALID before the element kernel is launched.  c_tri == NULL means 1; c_point is required and must be finite.
 * ntris == 0 is allowed and gives the zero vector.  Hermite elements are not covered. */
int wae_p1_assemble_source(int32_t device, int64_t npoints, const double *points, int64_t ntris, const int32_t *tris, const double *c_tri,
                           double *out);
int wae_p1_assemble_source_cpoint(int32_t device, int64_t npoints, const double *points, int64_t ntris, const int32_t *tris, const double *c_point,
                                  double *out);
int wae_p2_assemble_source(int32_t device, int64_t npoints, const double *points, int64_t ntets, const int32_t *tets, int64_t ntris,
                           const int32_t *tris, const double *c_tri, double *out, int64_t nout);
int wae_p2_assemble_source_cpoint(int32_t device, int64_t npoints, const double *points, int64_t ntets, const int32_t *tets, int64_t ntris,
                                  const int32_t *tris, const double *c_point, double *out, int64_t nout);
/* Discrete-adjoint shape sensitivity (src/shape_sensitivity.jl:16-141) of an eigenvalue w.r.t. the coordinates of surface
 * points, for the interior (M, K) and the admittance-boundary (w*Y*C) parts of the P1 Helmholtz operator.  As in the
 * reference the operator derivative is a central difference (step h) of two local re-discretisations of the simplices
 * that touch the point; here one device thread does that for one (point, simplex, coordinate).
 *   pair_pt_t[i], pair_tet[i]: surface point and one tetrahedron containing it (npair_t pairs); pair_pt_s, pair_tri:
 *   the same for boundary triangles (tris: 3 point indices each, c_tri: speed of sound of the adjacent tetrahedron).
 *   omega: eigenvalue (re, im); omegaY: omega*Y (re, im); v, v_adj: eigenvectors, normalised v'v = 1, v_adj' L'(omega) v = 1.
 *   out_t[3*npair_t], out_s[3*npair_s] (complex): -v_adj' (dL/dx) v contribution of every pair and coordinate; the
 *   caller sums them per point (deterministic order). */
int wae_p1_shape_sensitivity(int32_t device, int64_t npoints, const double *points, const int32_t *tets, const double *c_tet, int64_t npair_t,
                             const int32_t *pair_pt_t, const int32_t *pair_tet, const int32_t *tris, const double *c_tri, int64_t npair_s,
                             const int32_t *pair_pt_s, const int32_t *pair_tri, int64_t ntets, int64_t ntris, const double *omega,
                             const double *omegaY, const double *v, const double *v_adj, double h, double *out_t, double *out_s);

/* Flame part of the same sensitivity (a :flame entry in dscrp; shape_sensitivity.jl:62-141 with Helmholtz.jl:292-344,464-487):
 * per (surface point, flame tetrahedron touching it) pair and coordinate, |det J| of the tetrahedron with the point moved by +h
 * and -h (det_pm[pair][3][2]) and, per pair, the sum of conj(v_adj) over the tetrahedron's nodes (ssum, complex); per listed
 * vertex of the reference tetrahedron (pair_pt_r) and coordinate, sum_b (grad(phi_b).n_ref) v_b on the reference tetrahedron with
 * that vertex moved by +h / -h (g_pm[pair][3][2], complex) and the undisplaced value g0.  The caller (helmholtz/assemble.py,
 * julia) sums the pairs of a point in order and forms  -v_adj' (Q+ - Q-)/(2h) v  with Q = S (x) g,  S_a = |det J|/24,
 * g_b = -(nglobal_scaled / volume of the point's flame tetrahedra) grad(phi_b).n_ref  -- the reference re-discretises the flame
 * domain REDUCED to the simplices at the point, volume included. */
int wae_p1_shape_sensitivity_flame(int32_t device, int64_t npoints, const double *points, int64_t ntets, const int32_t *tets, int64_t npair,
                                   const int32_t *pair_pt, const int32_t *pair_tet, int32_t ref_tet, int64_t npair_r, const int32_t *pair_pt_r,
                                   const double *n_ref, const double *v, const double *v_adj, double h, double *det_pm, double *ssum,
                                   double *g_pm, double *g0);

/* The same sensitivity for P2 elements and for a nodal speed of sound.  Semantics, conventions and outputs are those of the two entries
 * above: per (point, simplex) pair and coordinate the central difference (step h) of two local re-discretisations with the point moved by
 * +h and -h, contracted with the local entries of v_adj and v; 0-based int32 indices, interleaved complex, out_t[3*npair_t] and
 * out_s[3*npair_s] summed per point by the caller in pair order.  A pair whose point is no corner of its simplex contributes zero.
 * npair_t == 0 and npair_s == 0 are allowed; nothing is launched for an empty list, and with both empty nothing at all (the P2 entries then
 * check nv against an edge count made on the host).  No atomics: the same bits on every call.
 *  - wae_p2_shape_sensitivity: P2 elements, c per simplex (c_tet, c_tri: NULL = 1).  tets / tris are the plain 4-point / 3-point lists;
 *    the entry numbers the edges itself (the wae_p2_connectivity pipeline of wae_p2_assemble*: ntets > 0 always, the triangles only if
 *    npair_s > 0).  Straight-sided elements depend on their corner points only, so only corner points move.  v, v_adj: nv = npoints + nedges
 *    entries; a wrong nv returns WAE_ERR_INVALID.  The kernel contracts the geometry-free element tensors with the local vector entries
 *    once per pair and differences only |det J| and |det J| grad l_i . grad l_j  (resp. |(x0-x2) x (x1-x2)|)  at +-h.
 *  - wae_p1_shape_sensitivity_cpoint, wae_p2_shape_sensitivity_cpoint: c_point (npoints doubles, required, finite) in the place of c_tet
 *    and c_tri, element matrices of wae_p1_assemble_cpoint / wae_p2_assemble_cpoint and their boundary forms; the nodal values stay with
 *    their points while a point moves.
 * WAE_ERR_INVALID with a message in wae_last_error, before any launch: a point, tetrahedron or triangle index out of range in the meshes or
 * the pair lists, h not finite or <= 0, a c_point value that is not finite, a wrong nv. */
int wae_p2_shape_sensitivity(int32_t device, int64_t npoints, const double *points, const int32_t *tets, const double *c_tet, int64_t npair_t,
                             const int32_t *pair_pt_t, const int32_t *pair_tet, const int32_t *tris, const double *c_tri, int64_t npair_s,
                             const int32_t *pair_pt_s, const int32_t *pair_tri, int64_t ntets, int64_t ntris, const double *omega,
                             const double *omegaY, int64_t nv, const double *v, const double *v_adj, double h, double *out_t, double *out_s);
int wae_p1_shape_sensitivity_cpoint(int32_t device, int64_t npoints, const double *points, const int32_t *tets, const double *c_point, int64_t npair_t,
                                    const int32_t *pair_pt_t, const int32_t *pair_tet, const int32_t *tris, int64_t npair_s, const int32_t *pair_pt_s,
                                    const int32_t *pair_tri, int64_t ntets, int64_t ntris, const double *omega, const double *omegaY, const double *v,
                                    const double *v_adj, double h, double *out_t, double *out_s);
int wae_p2_shape_sensitivity_cpoint(int32_t device, int64_t npoints, const double *points, const int32_t *tets, const double *c_point, int64_t npair_t,
                                    const int32_t *pair_pt_t, const int32_t *pair_tet, const int32_t *tris, int64_t npair_s, const int32_t *pair_pt_s,
                                    const int32_t *pair_tri, int64_t ntets, int64_t ntris, const double *omega, const double *omegaY, int64_t nv,
                                    const double *v, const double *v_adj, double h, double *out_t, double *out_s);
/* P2 form of wae_p1_shape_sensitivity_flame: the same outputs and the same combination by the caller, with
 *   ssum = sum_a s_a conj(v_adj_a) over the 10 nodes of the flame tetrahedron, s_a = int phi_a / |det J| (-1/120 on points, 1/30 on edges), so
 *          that v_adj' S+- = sum over the point's pairs of det_pm * ssum  (P1: det_pm / 24 * ssum);
 *   g_pm / g0 = sum_b (grad(phi_b)(x_ref) . n_ref) v_b over the 10 nodes of the reference tetrahedron.  x_ref (3 doubles) is fixed in space,
 *          so its barycentric coordinates are taken in the displaced reference tetrahedron, as wae_p2_assemble_flame takes them in the mesh's.
 * v, v_adj: nv = npoints + nedges entries (a wrong nv: WAE_ERR_INVALID, as are ref_tet or a flame tetrahedron out of range, an index out of
 * range, h not finite or <= 0).  The flame does not depend on c. */
int wae_p2_shape_sensitivity_flame(int32_t device, int64_t npoints, const double *points, int64_t ntets, const int32_t *tets, int64_t npair,
                                   const int32_t *pair_pt, const int32_t *pair_tet, int32_t ref_tet, int64_t npair_r, const int32_t *pair_pt_r,
                                   const double *x_ref, const double *n_ref, int64_t nv, const double *v, const double *v_adj, double h, double *det_pm,
                                   double *ssum, double *g_pm, double *g0);

/* -- tall matrices: Beyn's eigenpair extraction on the device ------------------------------------------------------
 * The step that turns the moments into eigenpairs (beyn.jl:76-107; `moments2eigs`, beyn.jl:289-323): block Hankel matrices
 * B0, B1 of size (d K) x (l K), the thin SVD  B0 = U S W^H,  the small matrix  U^H B1 W S^-1,  its eigenpairs (Omega, Y), and
 * P = U[1:d, :] Y.  Everything tall stays in HBM and runs in the library; the (l K) x (l K) problems stay with the host's
 * LAPACK (Julia LinearAlgebra / numpy), the split the Arnoldi entries use.  The host wrappers build the SVD from Gram matrices
 * by deflation in stages (julia/WAEHip.jl `moments2eigs_device`, nlevp/beyn.py `moments2eigs_native`).
 * A wae_tall is a column-major rows x ncols ComplexF64 matrix in HBM with leading dimension = rows, in the caller's row
 * numbering, owned by the library and independent of any family; host arrays are column-major, interleaved (re,im).
 * The dev_ptr of wae_tall_info is what the caller passes as out_dev of wae_beyn_moments / wae_beyn_moments_rb (moments of
 * d x l x 2K = a d x (l 2K) tall matrix: they never visit the host) and as P_dev of wae_eig_residuals (d x n).
 * Calls that name one handle -- in any argument, `const` ones included: wae_tall_gram keeps its reduction scratch in `a` -- must be
 * serialised by the caller, like calls on a family; calls on different handles may run from different threads.
 * Every entry returns when its result is complete.  WAE_ERR_INVALID (nothing launched): null pointers, ranges outside a
 * matrix, widths above WAE_TALL_MAXCOLS or below 0, matrices that differ in rows or device, shapes that do not fit
 * wae_tall_hankel.  A call with a zero width (na, nb, ns, nc, nrows or ncols = 0) is a no-op: WAE_OK.
 *   create   zero-filled.  write / read: the block rows row0 .. row0+nrows-1, columns col0 .. col0+ncols-1 from / to
 *            X (nrows x ncols, host).
 *   gram     G (na x nb, host) = A[:, a_col0 .. +na)^H B[:, b_col0 .. +nb);  A and B on one device, same rows; a == b allowed.
 *            Summed in two stages in a fixed order (no atomics): two identical calls return identical bits.
 *   mul      dst[r, dst_col0+j] = beta dst[r, dst_col0+j] + alpha sum_i src[src_row0+r, src_col0+i] C[i,j]  for r < rows of
 *            dst, j < nc;  C: ns x nc on the host; alpha, beta: one complex number each; needs src_row0 + rows of dst <= rows of
 *            src.  dst and src may be one matrix if the two column ranges do not overlap (WAE_ERR_INVALID if they do).
 *            beta = 0: dst is not read (NaNs there do not propagate).
 *   hankel   from a moment tensor kept as a d x (l 2K) tall matrix (the layout wae_beyn_moments writes), dst (d K) x (l K):
 *            dst[i d + r, j l + c] = moments[r, (i+j+shift) l + c],  shift = 0 (B0) or 1 (B1)   (beyn.jl:76-90) */
typedef struct wae_tall wae_tall;
#define WAE_TALL_MAXCOLS 64     /* widest block one gram / mul call takes; the wrappers loop over blocks */
int wae_tall_create (wae_tall **out, int32_t device, int64_t rows, int32_t ncols);
int wae_tall_destroy(wae_tall *m);
int wae_tall_info   (const wae_tall *m, int64_t *rows, int32_t *ncols, uint64_t *dev_ptr);
int wae_tall_write  (wae_tall *m, int64_t row0, int64_t nrows, int32_t col0, int32_t ncols, const double *X);
int wae_tall_read   (const wae_tall *m, int64_t row0, int64_t nrows, int32_t col0, int32_t ncols, double *X);
int wae_tall_gram(const wae_tall *a, int32_t a_col0, int32_t na, const wae_tall *b, int32_t b_col0, int32_t nb, double *G_out);
int wae_tall_mul(wae_tall *dst, int32_t dst_col0, const wae_tall *src, int64_t src_row0, int32_t src_col0, int32_t ns,
                 const double *C, int32_t nc, const double *alpha, const double *beta);
int wae_tall_hankel(wae_tall *dst, const wae_tall *moments, int32_t l, int32_t K, int32_t shift);

/* -- measurement helpers (bench.py) --------------------------------------------------------------------
 * Time `reps` launches of the fused multi-term SpMV on device-resident data with HIP events on the
 * library's own stream; r right-hand sides.  ms_out = average milliseconds per launch. */
int wae_bench_spmv(wae_family *h, const double *coeffs, int32_t r, int32_t reps, double *ms_out);
/* the same for an operator of the multigrid hierarchy (which = 0: level operator `level`, 1: restriction from `level`, 2: prolongation
 * to `level`, an in-place update of the fine vector), with its
 * algorithmic bytes per launch (SURVEY 8d layout: 16 + 4 bytes per nonzero and plane with a non-zero coefficient -- 8 + 4 for the
 * real restriction -- row pointers, input and output vectors touched once): the roofline line of the level-1 kernels. */
int wae_bench_spmv_level(wae_family *h, const double *coeffs, int32_t which, int32_t level, int32_t r, int32_t reps, double *ms_out,
                         int64_t *bytes_out);
/* device triad a = b + s*c over n doubles: measured streaming bandwidth in GB/s (the best of five grid sizes: the rate depends on the
 * shape of the launch by up to 20 %) */
int wae_bench_triad(int32_t device, int64_t n, int32_t reps, double *gbs_out);

/* -- test hook (tests/ only) ----------------------------------------------------------------------------
 * The solver applies the operator `L(z)*X` (LinOpFam.jl:482-529) in fused forms that no public entry exposes -- residual,
 * damped-Jacobi sweep, product + first sweep, converged-chunk masks -- and on the coarse levels of its hierarchy.  This entry
 * runs ONE such launch so that the parity tests can compare every form with the CPU oracle:
 *   which = 0: the operator of multigrid level `level` (0 = the family itself; >= 1 needs wae_solver_setup);
 *   which = 1: the restriction from `level` to `level + 1` (coefficients ignored; mode 0);
 *   which = 2: the prolongation from `level + 1` to `level`, Y = B + P X (coefficients ignored; mode 3): the out-of-place
 *              form of the prolongation kernels, or, when B and Y are the same array, their in-place form.
 *   mode: 0 Y = A X | 1 Y = B - A X | 2 Y = X + w/diag (B - A X) | 3 Y = B + A X | 4 Y = (A X)/diag | 5 Y = (B - A X)/diag
 *         | 6 Y = A X and B2 = w/diag (A X)  (diag = the diagonal of sum_k c_k A_k, w = jac_w)
 *   coeffs: ncoef x T (ncoef = 1: one system; ncoef = r: one coefficient row per column);
 *   X, B, Y, B2: column-major n_in x r / n_out x r complex (B may be NULL for modes 0, 4; B2 only for mode 6).  Level 0 is in
 *   the caller's row numbering; coarser levels in the hierarchy's own (their size: n_in/n_out = 0 on entry returns it in *n_out_q).
 *   cmask: NULL or one byte per 8-column chunk; 0 = the chunk is skipped and keeps the values Y (and B2) hold on entry.
 *   flags bit 0: bypass the tile-local storage (the plain CSR kernels), for A/B comparisons of the two storage forms. */
int wae_debug_spmv(wae_family *h, int32_t which, int32_t level, int32_t mode, const double *coeffs, int32_t ncoef, const double *X,
                   const double *B, double *Y, double *B2, int32_t r, int32_t op, double jac_w, const uint8_t *cmask, int32_t flags,
                   int64_t *n_in_q, int64_t *n_out_q);

/* ONE launch of the prolongation from `level + 1` to `level` in the form that also delivers the column norms of its result (the light
 * cycle of the solvers ends in it): Y = B + P X and norms[b] = ||Y[:, b]||, summed per workgroup and then in workgroup order, so that two
 * calls give the same bits.  Needs wae_solver_setup.
 *   X       column-major n_coarse x r complex; B, Y: column-major n_fine x r complex (sizes: wae_debug_spmv, which = 2); norms: r doubles.
 *           Level 0 is in the caller's row numbering, coarser levels in the hierarchy's own.
 *   cmask   NULL or one byte per 8-column chunk; the columns of a chunk with byte 0 keep what Y held on entry and get the norm 0.
 *   flags   bit 0: the CSR kernel where the level has the tile form too; bit 1: the norms alone -- Y is returned as it was passed.
 * No set-up, a level without a prolongation, r outside 1..256 or an unknown flag: WAE_ERR_INVALID, nothing is launched. */
int wae_debug_prolong(wae_family *h, int32_t level, const double *X, const double *B, double *Y, double *norms, int32_t r, const uint8_t *cmask,
                      int32_t flags);

/* ONE application of the multigrid preconditioner -- the V-cycle the solvers run, on the handle's own workspaces -- started at
 * multigrid level `level`, so that tests/ can compare the composition (which weight goes to which sweep, the light cycle, the fused
 * first sweep, the redirected last sweep, the coefficient table of every level, op = T/C on the coarse levels, the masks passed
 * down the recursion) with a reference of their own.  Needs wae_solver_setup.
 *   level   0 ... number of levels - 1; the last level is the dense one: the call is then the dense apply alone (wae_debug_spmv
 *           has no form for that level).
 *   coeffs  ncoef x T (ncoef = 1: one system; ncoef = r: one coefficient row per column).  The batch and the per-level plane tables are
 *           built as wae_solve builds them (conjugated for op = C), uploaded, and the dense level is assembled and inverted first.
 *   B, Y    column-major n_level x r complex, 1 <= r <= the batch width of the set-up (opts[6]): Y = M_level^-1 B.  Level 0 is in the
 *           caller's row numbering, coarser levels in the hierarchy's own (sizes: wae_debug_spmv; the dense level has as many rows as
 *           the last restriction).
 *   flags   bit 0: the light cycle of the projected phase of a contour integral (pre-smoothing weight opts[11], no post-smoothing),
 *                  for this call only;
 *           bit 1: the result is delivered through a separate output buffer, as the Krylov steps that let the last post-smoothing
 *                  sweep write into a basis slot (without a post-smoothing sweep: a copy);
 *           bit 2 (level 0 only): B is a vector V and Y = M^-1 A V as one Krylov step forms it -- the product that also writes
 *                  the first sweep, then the cycle without its first sweep.
 *   cmask   NULL or one byte per 8-column chunk, handed down as the solver hands it down (batches narrower than 8 columns run
 *           unmasked); the columns of a chunk with byte 0 return what Y held on entry.
 * No set-up, a level that does not exist, r outside 1..opts[6], ncoef other than 1 or r, an op outside 0..2, an unknown flag, or
 * flags bit 2 on a level >= 1: WAE_ERR_INVALID with a message, nothing is launched and the handle stays usable. */
int wae_debug_vcycle(wae_family *h, int32_t level, const double *coeffs, int32_t ncoef, const double *B, double *Y, int32_t r, int32_t op,
                     int32_t flags, const uint8_t *cmask);

/* The streaming and reduction kernels under the lock-step GMRES, the snapshot basis, the Beyn accumulation, the batched
 * perturbation and the dense coarse level, ONE library launch per call (the dense level: assemble, invert, apply), so that tests/
 * can compare each with a reference of its own.  Needs no family and no solver set-up: the entry uploads the caller's arrays to
 * `device`, allocates the scratch of the reductions as the solver set-up sizes it, runs the launch on a stream of its own, copies
 * every array back and synchronises.
 *   op     one of WAE_VEC_* below; sz[0..nsz) its sizes, bufs[0..nbuf) its arrays in the order listed (complex128, lens[i] entries
 *          each; NULL = an optional argument left out).  Multivectors are in the library's interleaved layout: vector i of an
 *          [nv][n][nb] array starts `stride` entries after vector i-1, entry (row, b) of a vector at row*nb + b.
 *   cmask  NULL or one byte per 8-column chunk (only the operations marked `m`); perm: NULL or d row indices (BEYN_ACCUM only);
 *          status_out: NULL or the status word of the dense inversion (DENSE only; 0 = every pivot non-zero).
 *   A size outside the ranges a launcher accepts, or an array shorter than the sizes need: WAE_ERR_INVALID, nothing is launched
 *   past the point of the refusal.
 * Contract of a masked chunk (cmask byte 0), as the consumers rely on it (vec.hip gmres_step_kernel, gmres_pair_coef_kernel read
 * the reductions of every column, retired ones included, and take 0 for "column retired": 1/norm = 0 keeps it out of every later
 * coefficient): vector outputs of its columns keep what they held; every reduction output of its columns (dots, norms, 1/norm^2,
 * Gram entries) is WRITTEN as exact 0.  Columns never mix: a NaN in one column changes no output of another.
 *                          sz                                   bufs
 *   DOTS            m   n nb nv stride          V W out[nv][nb] scale[nv][nb]?      (scale given: launch_dots_scaled)
 *   NORMS           m   n nb                    X out[nb]
 *   DOTS_MULTI          n nb nv nw sv sw        V W out[nv][nw][nb]
 *   AXPY_NEG        m   n nb nv stride          V h[nv][nb] W                       W -= sum_i h_i V_i  (nv = 0 allowed)
 *   LINCOMB / _ADD      n nb nv stride          V y[nv][nb] Y                       Y (+)= sum_i y_i V_i
 *   AXPY_NEG_NORM   m   n nb nv stride          V h W norms[nb] base? inv[nb]?      W = (base or W) - V h, its norms, 1/norm^2
 *   AXPY_NEG_MULTI      n nb nv stride cnt ws   V h[nv][cnt][nb] W (cnt vectors, ws apart)
 *   DOTS2           m   n nb nv stride          V W1 W2 out1 out2 gram[3][nb] scale[nv][nb]
 *   AXPY2           m   n nb nv stride          V c1 c2m alpha[nb] W1 W2 norms[2][nb] inv[2][nb]
 *   LINCOMB_REP         n nb nv stride l        Q (vectors of n x l) y[nv][nb] X
 *   SCALE_INV       m   n nb                    X alpha[nb] Y
 *   MASK_COLS           n nb                    X keep[nb]
 *   EXTRACT_COLS        n nb off l              X out (n x l)
 *   BEYN_ACCUM          d nb l nsys npow lA c0  X w[nsys] z[nsys] A[npow][lA][d]    (lA = 0: l)
 *   PT_GEMM_BATCH       d nb k stride T         V G[k][T][nb] U (d x T x nb)
 *   PT_AXPBY_COLS       d nb                    coef[2][nb] x y out
 *   PT_PROJECT          d nb nd                 vk v0 dots[nd][nb]
 *   DENSE           m   n nb nsys nplanes op cps   planes[nplanes][n][n] pc[nsys][nplanes] Ainv[nsys][n][n] X? Y?   (n <= 2048; the mask
 *                                               is the apply's; pc conjugated by the caller for op = C, as the solver passes it) */
enum {
    WAE_VEC_DOTS = 0, WAE_VEC_NORMS, WAE_VEC_DOTS_MULTI, WAE_VEC_AXPY_NEG, WAE_VEC_LINCOMB, WAE_VEC_LINCOMB_ADD, WAE_VEC_AXPY_NEG_NORM,
    WAE_VEC_AXPY_NEG_MULTI, WAE_VEC_DOTS2, WAE_VEC_AXPY2, WAE_VEC_LINCOMB_REP, WAE_VEC_SCALE_INV, WAE_VEC_MASK_COLS, WAE_VEC_EXTRACT_COLS,
    WAE_VEC_BEYN_ACCUM, WAE_VEC_PT_GEMM_BATCH, WAE_VEC_PT_AXPBY_COLS, WAE_VEC_PT_PROJECT, WAE_VEC_DENSE
};
int wae_debug_vec(int32_t device, int32_t op, const int64_t *sz, int32_t nsz, double *const *bufs, const int64_t *lens, int32_t nbuf,
                  const uint8_t *cmask, const int32_t *perm, int32_t *status_out);

/* The small-matrix half of the lock-step GMRES (vec.hip gmres_init / step / rescale / clear_rescale / pair_coef / solve_y kernels):
 * a SCRIPT of events against one recurrence state, each event the launcher calls the solver issues for it, so that tests/ can
 * compare the Hessenberg columns, rotations, residual estimates, masks and pair coefficients with references of their own.  Needs no
 * family and no solver set-up: the state is allocated for (nb, m, histcap) as the solver lays it out (integer block zeroed, bnorm[nb]
 * from the caller, Hraw and sub present), the caller's arrays are uploaded to `device`, the events run on a stream of their own,
 * everything is copied back and the stream synchronised.
 *   ev[4 e ..]   kind (WAE_GMRES_* below), j (SOLVE_Y: ju), use_mask, offset of the event's arrays in `pool`;  evd[2 e ..]  tol, lim
 *   pool         plen complex128 entries, in and out; an event's arrays lie back to back from its offset ([rows][nb], entry (i, b) at
 *                i*nb + b; vectors [n][nb] alike):
 *     INIT     beta[nb] done[nb] (real part non-zero = done)                        launch_gmres_init
 *     STEP     hd[j+2][nb] Vnew[n][nb]                                              launch_gmres_step (step, rescale, clear_rescale);
 *              row j+1 of vsq is set to 1/hd[j+1]^2 first, as the fused update writes it in the solver
 *     PAIR     c1[j+1][nb] c2[j+1][nb] gram[3][nb] norms[2][nb] W1[n][nb] W2[n][nb] alpha[nb] c2m[j+1][nb] hd2[j+2][nb]
 *              launch_gmres_pair_coef (writes alpha, c2m, hd2), rows j+1, j+2 of vsq set to 1/norms^2, then the two steps of the
 *              solver's pair branch: (c1, j, lim 1e300, norm norms[0]) on W1 and (hd2, j+1, lim, norm norms[1]) on W2
 *     SOLVE_Y  out[m][nb]: launch_gmres_solve_y(ju) writes rows below max(ju, steps[b]) of column b
 *   cstate       complex128, in and out: R[m][m+1][nb] sn[m][nb] g[m+1][nb] vsq[m+2][nb] Hraw[m][m+1][nb] back to back
 *   dstate       double, in and out: cs[m][nb] sv[m+2][nb] sub[m][nb] hist[histcap][nb]  (what the kernels do not write keeps the
 *                caller's values)
 *   after EVERY event e:  snap_relres[e][nb];  snap_int[e][5 nb + 4] = conv steps iters histlen stalled [nb each], status[0..2] (active
 *                columns, NaN seen, renormalisation pending) and one unused word;  snap_cmask[e][(nb+7)/8];  snap_rescale[e][nb]
 *                (complex128);  snap_sv[e][2][nb] and snap_vsq[e][2][nb] (complex128): the rows the event wrote (INIT: row 0; STEP: row
 *                j+1; PAIR: rows j+1, j+2; unused rows 0).
 *   nb outside 1..256, m < 1, a j outside the cycle (STEP: 0 <= j < m; PAIR: j + 2 <= m; SOLVE_Y: 1 <= ju <= m), an unknown event or
 *   arrays that do not fit the pool: WAE_ERR_INVALID before anything is uploaded or launched. */
enum { WAE_GMRES_INIT = 0, WAE_GMRES_STEP, WAE_GMRES_PAIR, WAE_GMRES_SOLVE_Y };
int wae_debug_gmres(int32_t device, int32_t nb, int32_t m, int32_t histcap, int64_t n, const double *bnorm, const int64_t *ev,
                    const double *evd, int32_t nev, double *pool, int64_t plen, double *cstate, double *dstate, double *snap_relres,
                    int32_t *snap_int, uint8_t *snap_cmask, double *snap_rescale, double *snap_sv, double *snap_vsq);

#ifdef __cplusplus
}
#endif
#endif
