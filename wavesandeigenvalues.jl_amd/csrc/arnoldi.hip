// libwaehip.so -- shift-invert Arnoldi: the one process behind the three wae_arnoldi_shiftinvert* entries, wae_arnoldi_ritz_to_slot.
// Host code only; the solves and the slot columns go through solver.h.
#include <cmath>

#include "solver.h"

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

// The Arnoldi processes behind wae_arnoldi_shiftinvert_batch (start vectors and basis through host memory) and
// wae_arnoldi_shiftinvert_slots (start vectors from a device-resident multivector, basis kept on the device for wae_arnoldi_ritz_to_slot).
// v0_host: d x nsys column-major in the caller's row numbering, or null: then v0_slot / v0_cols name the columns.  V_out null: the
// basis stays in h->arn_EV (h->arn_nsys systems, h->arn_cols vectors each).
static int arnoldi_core(wae_family *h, int32_t nsys, const double *coeffsA, const double *coeffsM, int32_t m, const double *v0_host, int32_t v0_slot,
                        const int32_t *v0_cols, int32_t op, double tol, int32_t maxit, double ritz_tol, double *H_out, double *V_out,
                        wae_solve_info *info) {
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
    EV.reserve(vec * (m + 1)); t.reserve(vec); stage.reserve(vec); hcol.reserve((size_t)2 * (m + 2) * nsys);
    if (m > 1) gdir.reserve(vec);
    // per-system plane coefficients of M (level-0 slot order) and of A (all levels)
    std::vector<cplx> tab((size_t)nsys * h->nplanes);
    std::vector<zc> pcm;
    std::vector<std::vector<zc>> pcs(nsys);
    for (int sy = 0; sy < nsys; ++sy) {
        plane_coeffs(h, coeffsM + (size_t)sy * 2 * T, op, pcm);
        slot_coeffs(h, h->slot_plane[0], pcm, &tab[(size_t)sy * h->nplanes]);
        plane_coeffs(h, coeffsA + (size_t)sy * 2 * T, op, pcs[sy]);
    }
    pcM.upload(tab.data(), tab.size(), st);
    const Batch bt = Batch::per_column(nsys, op);
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

extern "C" {

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
        h->arn_hcol.reserve(yc.size() + (size_t)nsys);
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

}   // extern "C"
