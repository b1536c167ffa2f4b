"""ctypes binding of libwaehip.so (include/waehip.h).  No CPU fallback: importing works without a GPU
(so that the ABI can be inspected), but every compute entry point needs the HIP library and a device."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("WAE_LIB_PATH") or os.path.join(_HERE, "csrc", "libwaehip.so")     # (WAE_LIB_PATH: an A/B build of the library)

WAE_OK, WAE_WARN_MAXITER, WAE_WARN_STAGNATION = 0, 1, 2
WAE_ERR_INVALID, WAE_ERR_BREAKDOWN, WAE_ERR_EIGS, WAE_ERR_NAN, WAE_ERR_HIP = -1, -2, -3, -4, -5
OP_N, OP_T, OP_C = 0, 1, 2
CSC, CSR = 0, 1


class SolveInfo(C.Structure):
    _fields_ = [("iters_max", C.c_int32), ("iters_total", C.c_int32), ("n_unconverged", C.c_int32),
                ("levels", C.c_int32), ("relres_max", C.c_double), ("seconds", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class WaeError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libwaehip error {code}: {msg}")
        self.code = code


_lib = None

# every symbol include/waehip.h declares (checked by tests/test_abi.py)
EXPORTS = [
    "wae_last_error", "wae_device_count", "wae_version", "wae_family_create", "wae_family_create_opts", "wae_family_destroy",
    "wae_family_info", "wae_family_spmv_bytes", "wae_spmv_sum", "wae_spmv_sum_cols", "wae_spmv_sum_multi", "wae_solver_setup",
    "wae_solve", "wae_solve_guess", "wae_beyn_moments", "wae_beyn_moments_mgpu", "wae_beyn_moments_rb", "wae_rb_export", "wae_rb_import", "wae_eig_residuals", "wae_arnoldi_shiftinvert", "wae_arnoldi_shiftinvert_batch", "wae_perturb", "wae_slot_write", "wae_slot_read", "wae_slot_axpby", "wae_slot_forms", "wae_arnoldi_shiftinvert_slots", "wae_arnoldi_ritz_to_slot", "wae_perturb_slots", "wae_perturb_batch", "wae_perturb_batch_slots", "wae_p1_assemble", "wae_p1_assemble_boundary", "wae_p1_assemble_flame", "wae_p1_info", "wae_p1_get", "wae_p1_free", "wae_p1_shape_sensitivity", "wae_p1_shape_sensitivity_flame", "wae_bench_spmv", "wae_bench_spmv_level", "wae_bench_triad", "wae_debug_spmv", "wae_debug_prolong", "wae_debug_vcycle", "wae_debug_vec", "wae_debug_gmres",
    "wae_tall_create", "wae_tall_destroy", "wae_tall_info", "wae_tall_write", "wae_tall_read", "wae_tall_gram", "wae_tall_mul", "wae_tall_hankel",
    "wae_p2_connectivity", "wae_p2_connectivity_info", "wae_p2_connectivity_get", "wae_p2_connectivity_free", "wae_p2_assemble",
    "wae_p2_assemble_boundary", "wae_p2_assemble_flame",
    "wae_p1_assemble_cpoint", "wae_p1_assemble_boundary_cpoint", "wae_p2_assemble_cpoint", "wae_p2_assemble_boundary_cpoint",
    "wae_p1_assemble_source", "wae_p1_assemble_source_cpoint", "wae_p2_assemble_source", "wae_p2_assemble_source_cpoint", "wae_forced_response",
    "wae_p2_shape_sensitivity", "wae_p1_shape_sensitivity_cpoint", "wae_p2_shape_sensitivity_cpoint", "wae_p2_shape_sensitivity_flame",
    "wae_bloch_numbering", "wae_bloch_numbering_info", "wae_bloch_numbering_get", "wae_bloch_numbering_free", "wae_bloch_fold",
    "wae_octosplit", "wae_octosplit_info", "wae_octosplit_get", "wae_octosplit_prolong", "wae_octosplit_free",
    "wae_octosplit_prolongator", "wae_solver_setup_nested",
    "wae_octosplit_p2_info", "wae_octosplit_prolongator_p2", "wae_octosplit_prolong_p2", "wae_p2_embedding",
    "wae_locator_create", "wae_locator_info", "wae_locator_find", "wae_locator_set_p2", "wae_locator_weights", "wae_locator_sample",
    "wae_locator_free",
    "wae_herm_connectivity", "wae_herm_connectivity_info", "wae_herm_connectivity_get", "wae_herm_connectivity_free", "wae_herm_assemble",
    "wae_herm_assemble_boundary", "wae_herm_assemble_flame",
    "wae_hermite_prolongators", "wae_hermite_prolongators_info", "wae_hermite_prolongators_get", "wae_hermite_prolongators_free",
    "wae_solver_level_weights", "wae_hermite_locator_set",
]
BLOCH_IMAGE, BLOCH_AXIS = 1, 2      # WAE_BLOCH_* flag bits
TALL_MAXCOLS = 64           # WAE_TALL_MAXCOLS

# operation codes of wae_debug_vec (include/waehip.h WAE_VEC_*)
(VEC_DOTS, VEC_NORMS, VEC_DOTS_MULTI, VEC_AXPY_NEG, VEC_LINCOMB, VEC_LINCOMB_ADD, VEC_AXPY_NEG_NORM, VEC_AXPY_NEG_MULTI, VEC_DOTS2, VEC_AXPY2,
 VEC_LINCOMB_REP, VEC_SCALE_INV, VEC_MASK_COLS, VEC_EXTRACT_COLS, VEC_BEYN_ACCUM, VEC_PT_GEMM_BATCH, VEC_PT_AXPBY_COLS,
 VEC_PT_PROJECT, VEC_DENSE) = range(19)
# event kinds of wae_debug_gmres (include/waehip.h WAE_GMRES_*)
GMRES_INIT, GMRES_STEP, GMRES_PAIR, GMRES_SOLVE_Y = range(4)


def lib():
    """Load libwaehip.so (built by __graft_entry__.build() / csrc/Makefile); raise loudly if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950). There is no CPU fallback for the product path.")
    L = C.CDLL(LIB_PATH)
    dp = C.POINTER(C.c_double)
    vpp = C.POINTER(C.c_void_p)
    i32p = C.POINTER(C.c_int32)
    i64p = C.POINTER(C.c_int64)
    L.wae_last_error.restype = C.c_char_p
    L.wae_version.restype = C.c_char_p
    L.wae_device_count.argtypes = [C.POINTER(C.c_int)]
    L.wae_family_create.argtypes = [C.POINTER(C.c_void_p), C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                    vpp, vpp, vpp, C.c_int32]
    L.wae_family_create_opts.argtypes = [C.POINTER(C.c_void_p), C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                         vpp, vpp, vpp, C.c_int32, dp, C.c_int32]
    L.wae_family_destroy.argtypes = [C.c_void_p]
    L.wae_family_info.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
    L.wae_family_spmv_bytes.argtypes = [C.c_void_p, C.POINTER(C.c_uint8), C.c_int32]
    L.wae_family_spmv_bytes.restype = C.c_int64
    L.wae_spmv_sum.argtypes = [C.c_void_p, dp, dp, dp, C.c_int32, C.c_int32]
    L.wae_spmv_sum_cols.argtypes = [C.c_void_p, dp, C.c_int32, dp, dp, C.c_int32, C.c_int32]
    L.wae_spmv_sum_multi.argtypes = [C.c_void_p, dp, dp, dp]
    L.wae_solver_setup.argtypes = [C.c_void_p, dp, dp, C.c_int32]
    L.wae_solve.argtypes = [C.c_void_p, dp, C.c_int32, dp, dp, C.c_int32, C.c_int32, C.c_double, C.c_int32,
                            C.POINTER(SolveInfo)]
    L.wae_solve_guess.argtypes = [C.c_void_p, dp, C.c_int32, dp, dp, dp, C.c_int32, C.c_int32, C.c_double, C.c_int32,
                                  C.POINTER(SolveInfo)]
    L.wae_beyn_moments.argtypes = [C.c_void_p, C.c_int32, dp, dp, dp, dp, C.c_int32, C.c_int32, C.c_double, C.c_int32,
                                   dp, C.c_uint64, C.POINTER(SolveInfo)]
    L.wae_beyn_moments_rb.argtypes = [C.c_void_p, C.c_int32, dp, dp, dp, dp, C.c_int32, C.c_int32, C.c_double, C.c_int32,
                                      C.c_int32, C.c_int32, C.c_int32, C.c_uint64, dp, C.c_uint64, C.c_int32, C.c_int32, C.c_int32,
                                      C.POINTER(SolveInfo)]
    L.wae_beyn_moments_mgpu.argtypes = [vpp, C.c_int32, C.c_int32, dp, dp, dp, dp, C.c_int32, C.c_int32, C.c_double, C.c_int32, C.c_int32, dp,
                                        C.POINTER(SolveInfo)]
    L.wae_rb_export.argtypes = [C.c_void_p, i32p, i32p, i32p, i32p, dp, dp]
    L.wae_rb_import.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_uint64, C.c_int32, i32p, dp, dp]
    L.wae_eig_residuals.argtypes = [C.c_void_p, C.c_int32, dp, dp, C.c_uint64, dp]
    L.wae_arnoldi_shiftinvert.argtypes = [C.c_void_p, dp, dp, C.c_int32, dp, C.c_int32, C.c_double, C.c_int32, dp, dp,
                                          C.POINTER(SolveInfo)]
    L.wae_arnoldi_shiftinvert_batch.argtypes = [C.c_void_p, C.c_int32, dp, dp, C.c_int32, dp, C.c_int32, C.c_double, C.c_int32, C.c_double,
                                                dp, dp, C.POINTER(SolveInfo)]
    L.wae_perturb.argtypes = [C.c_void_p, dp, C.c_int32, dp, dp, C.c_int32, dp, C.c_double, C.c_int32, dp, dp,
                              C.POINTER(SolveInfo)]
    L.wae_slot_write.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, dp]
    L.wae_slot_read.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, dp]
    L.wae_slot_axpby.argtypes = [C.c_void_p, C.c_int32, C.c_int32, i32p, C.c_int32, i32p, dp, dp, C.c_int32]
    L.wae_slot_forms.argtypes = [C.c_void_p, C.c_int32, dp, C.c_int32, C.c_int32, i32p, C.c_int32, i32p, dp]
    L.wae_arnoldi_shiftinvert_slots.argtypes = [C.c_void_p, C.c_int32, dp, dp, C.c_int32, C.c_int32, i32p, C.c_int32, C.c_double, C.c_int32, C.c_double,
                                                dp, C.POINTER(SolveInfo)]
    L.wae_arnoldi_ritz_to_slot.argtypes = [C.c_void_p, C.c_int32, C.c_int32, dp, C.c_int32, i32p, C.c_int32]
    L.wae_perturb_slots.argtypes = [C.c_void_p, dp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, dp, C.c_double, C.c_int32, dp, dp,
                                    C.POINTER(SolveInfo)]
    L.wae_perturb_batch.argtypes = [C.c_void_p, C.c_int32, dp, C.c_int32, dp, dp, C.c_int32, dp, C.c_double, C.c_int32, dp, dp, i32p,
                                    C.POINTER(SolveInfo)]
    L.wae_perturb_batch_slots.argtypes = [C.c_void_p, C.c_int32, dp, C.c_int32, C.c_int32, i32p, C.c_int32, i32p, C.c_int32, dp, C.c_double, C.c_int32,
                                          dp, dp, i32p, C.POINTER(SolveInfo)]
    L.wae_p1_assemble.argtypes = [C.c_int32, C.c_int64, dp, C.c_int64, C.POINTER(C.c_int32), dp, C.POINTER(C.c_void_p)]
    L.wae_p1_assemble_boundary.argtypes = [C.c_int32, C.c_int64, dp, C.c_int64, C.POINTER(C.c_int32), dp, C.POINTER(C.c_void_p)]
    L.wae_p1_assemble_flame.argtypes = [C.c_int32, C.c_int64, dp, C.c_int64, C.POINTER(C.c_int32), C.c_int64, C.POINTER(C.c_int32), C.c_int32, dp,
                                        C.c_double, C.POINTER(C.c_void_p), dp]
    L.wae_p1_info.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.wae_p1_get.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), dp, dp]
    L.wae_p1_free.argtypes = [C.c_void_p]
    L.wae_p2_connectivity.argtypes = [C.c_int32, C.c_int64, C.c_int64, i32p, C.c_int64, i32p, C.POINTER(C.c_void_p)]
    L.wae_p2_connectivity_info.argtypes = [C.c_void_p, i64p, i64p, i64p]
    L.wae_p2_connectivity_get.argtypes = [C.c_void_p, i32p, i32p, i32p]
    L.wae_p2_connectivity_free.argtypes = [C.c_void_p]
    L.wae_p2_assemble.argtypes = [C.c_int32, C.c_int64, dp, C.c_int64, i32p, dp, C.POINTER(C.c_void_p)]
    L.wae_p2_assemble_boundary.argtypes = [C.c_int32, C.c_int64, dp, C.c_int64, i32p, C.c_int64, i32p, dp, C.POINTER(C.c_void_p)]
    L.wae_p2_assemble_flame.argtypes = [C.c_int32, C.c_int64, dp, C.c_int64, i32p, C.c_int64, i32p, C.c_int32, dp, dp, C.c_double,
                                        C.POINTER(C.c_void_p), dp]
    for name in ("wae_p1_assemble", "wae_p1_assemble_boundary", "wae_p2_assemble", "wae_p2_assemble_boundary"):       # c_point in the place of c_tet / c_tri
        getattr(L, name + "_cpoint").argtypes = getattr(L, name).argtypes
    for name in ("wae_p1_assemble_source", "wae_p1_assemble_source_cpoint"):
        getattr(L, name).argtypes = [C.c_int32, C.c_int64, dp, C.c_int64, i32p, dp, dp]
    for name in ("wae_p2_assemble_source", "wae_p2_assemble_source_cpoint"):
        getattr(L, name).argtypes = [C.c_int32, C.c_int64, dp, C.c_int64, i32p, C.c_int64, i32p, dp, dp, C.c_int64]
    L.wae_forced_response.argtypes = [C.c_void_p, C.c_int32, dp, C.c_int32, i64p, i32p, dp, dp, C.c_int32, i64p, i32p, dp, dp, C.c_int32, i32p, dp,
                                      C.c_double, C.c_int32, C.POINTER(SolveInfo)]
    L.wae_p1_shape_sensitivity.argtypes = [C.c_int32, C.c_int64, dp, i32p, dp, C.c_int64, i32p, i32p, i32p, dp, C.c_int64, i32p, i32p,
                                           C.c_int64, C.c_int64, dp, dp, dp, dp, C.c_double, dp, dp]
    L.wae_p1_shape_sensitivity_flame.argtypes = [C.c_int32, C.c_int64, dp, C.c_int64, i32p, C.c_int64, i32p, i32p, C.c_int32, C.c_int64, i32p, dp, dp, dp,
                                                 C.c_double, dp, dp, dp, dp]
    L.wae_p2_shape_sensitivity.argtypes = [C.c_int32, C.c_int64, dp, i32p, dp, C.c_int64, i32p, i32p, i32p, dp, C.c_int64, i32p, i32p,
                                           C.c_int64, C.c_int64, dp, dp, C.c_int64, dp, dp, C.c_double, dp, dp]
    L.wae_p1_shape_sensitivity_cpoint.argtypes = [C.c_int32, C.c_int64, dp, i32p, dp, C.c_int64, i32p, i32p, i32p, C.c_int64, i32p, i32p,
                                                  C.c_int64, C.c_int64, dp, dp, dp, dp, C.c_double, dp, dp]
    L.wae_p2_shape_sensitivity_cpoint.argtypes = [C.c_int32, C.c_int64, dp, i32p, dp, C.c_int64, i32p, i32p, i32p, C.c_int64, i32p, i32p,
                                                  C.c_int64, C.c_int64, dp, dp, C.c_int64, dp, dp, C.c_double, dp, dp]
    L.wae_p2_shape_sensitivity_flame.argtypes = [C.c_int32, C.c_int64, dp, C.c_int64, i32p, C.c_int64, i32p, i32p, C.c_int32, C.c_int64, i32p, dp, dp,
                                                 C.c_int64, dp, dp, C.c_double, dp, dp, dp, dp]
    L.wae_bloch_numbering.argtypes = [C.c_int32, C.c_int64, C.c_int64, i32p, C.c_int64, C.c_int64, C.c_int32, C.POINTER(C.c_void_p)]
    L.wae_bloch_numbering_info.argtypes = [C.c_void_p, i64p, i64p, i64p, i64p, i64p]
    L.wae_bloch_numbering_get.argtypes = [C.c_void_p, i32p, i32p, i32p]
    L.wae_bloch_numbering_free.argtypes = [C.c_void_p]
    L.wae_bloch_fold.argtypes = [C.c_int32, C.c_int64, i32p, i32p, dp, dp, i32p, i32p, C.c_int64, C.c_int32, C.POINTER(C.c_void_p)]
    L.wae_octosplit.argtypes = [C.c_int32, C.c_int64, dp, C.c_int64, i32p, C.c_int64, i32p, C.c_int32, C.POINTER(C.c_void_p)]
    L.wae_octosplit_info.argtypes = [C.c_void_p, C.c_int32, i64p, i64p, i64p]
    L.wae_octosplit_get.argtypes = [C.c_void_p, C.c_int32, dp, i32p, i32p, i32p, i32p, i32p]
    L.wae_octosplit_prolong.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, dp, dp]
    L.wae_octosplit_free.argtypes = [C.c_void_p]
    L.wae_octosplit_prolongator.argtypes = [C.c_void_p, C.c_int32, i32p, i32p, dp]
    L.wae_octosplit_p2_info.argtypes = [C.c_void_p, C.c_int32, i64p, i64p, i64p]
    L.wae_octosplit_prolongator_p2.argtypes = [C.c_void_p, C.c_int32, i32p, i32p, dp]
    L.wae_octosplit_prolong_p2.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, dp, dp]
    L.wae_p2_embedding.argtypes = [C.c_void_p, C.c_int64, i32p, i32p, dp]
    L.wae_locator_create.argtypes = [C.c_int32, C.c_int64, dp, C.c_int64, i32p, C.c_int64, C.POINTER(C.c_void_p)]
    L.wae_locator_info.argtypes = [C.c_void_p, i64p, i64p, i64p, i64p, i64p]
    L.wae_locator_find.argtypes = [C.c_void_p, C.c_int64, dp, C.c_double, i32p, dp]
    L.wae_locator_set_p2.argtypes = [C.c_void_p, C.c_int64, i32p]
    L.wae_locator_weights.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int64, dp, i32p, dp, i32p, dp]
    L.wae_locator_sample.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int64, dp, i32p, dp, C.c_int64, C.c_int32, dp, dp]
    L.wae_locator_free.argtypes = [C.c_void_p]
    L.wae_hermite_locator_set.argtypes = [C.c_void_p, C.c_int64, i32p]
    L.wae_herm_connectivity.argtypes = [C.c_int32, C.c_int64, C.c_int64, i32p, C.c_int64, i32p, C.POINTER(C.c_void_p)]
    L.wae_herm_connectivity_info.argtypes = [C.c_void_p, i64p, i64p, i64p, i64p]
    L.wae_herm_connectivity_get.argtypes = [C.c_void_p, i32p, i32p, i32p]
    L.wae_herm_connectivity_free.argtypes = [C.c_void_p]
    L.wae_herm_assemble.argtypes = [C.c_int32, C.c_int64, dp, C.c_int64, i32p, C.c_int64, i32p, dp, C.POINTER(C.c_void_p)]
    L.wae_herm_assemble_boundary.argtypes = [C.c_int32, C.c_int64, dp, C.c_int64, i32p, C.c_int64, i32p, dp, C.POINTER(C.c_void_p)]
    L.wae_herm_assemble_flame.argtypes = [C.c_int32, C.c_int64, dp, C.c_int64, i32p, C.c_int64, i32p, C.c_int64, i32p, C.c_int32, dp, dp, C.c_double,
                                          C.POINTER(C.c_void_p), dp]
    L.wae_hermite_prolongators.argtypes = [C.c_int32, C.c_int64, dp, C.c_int64, i32p, C.c_int64, i32p, C.POINTER(C.c_void_p)]
    L.wae_hermite_prolongators_info.argtypes = [C.c_void_p, C.c_int32, i64p, i64p, i64p]
    L.wae_hermite_prolongators_get.argtypes = [C.c_void_p, C.c_int32, i32p, i32p, dp]
    L.wae_hermite_prolongators_free.argtypes = [C.c_void_p]
    L.wae_solver_level_weights.argtypes = [C.c_void_p, C.c_int32, dp, dp, i32p]
    L.wae_solver_setup_nested.argtypes = [C.c_void_p, dp, dp, C.c_int32, C.c_int32, i64p, i64p, vpp, vpp, vpp]
    L.wae_bench_spmv.argtypes = [C.c_void_p, dp, C.c_int32, C.c_int32, dp]
    L.wae_bench_triad.argtypes = [C.c_int32, C.c_int64, C.c_int32, dp]
    L.wae_bench_spmv_level.argtypes = [C.c_void_p, dp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, dp, C.POINTER(C.c_int64)]
    L.wae_debug_spmv.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, dp, C.c_int32, dp, dp, dp, dp, C.c_int32, C.c_int32, C.c_double,
                                 C.POINTER(C.c_uint8), C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.wae_debug_prolong.argtypes = [C.c_void_p, C.c_int32, dp, dp, dp, dp, C.c_int32, C.POINTER(C.c_uint8), C.c_int32]
    L.wae_debug_vcycle.argtypes = [C.c_void_p, C.c_int32, dp, C.c_int32, dp, dp, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_uint8)]
    L.wae_debug_vec.argtypes = [C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.c_int32, C.POINTER(dp), C.POINTER(C.c_int64), C.c_int32,
                                C.POINTER(C.c_uint8), i32p, i32p]
    L.wae_debug_gmres.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, dp, C.POINTER(C.c_int64), dp, C.c_int32, dp, C.c_int64,
                                  dp, dp, dp, i32p, C.POINTER(C.c_uint8), dp, dp, dp]
    L.wae_tall_create.argtypes = [C.POINTER(C.c_void_p), C.c_int32, C.c_int64, C.c_int32]
    L.wae_tall_destroy.argtypes = [C.c_void_p]
    L.wae_tall_info.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_uint64)]
    L.wae_tall_write.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, dp]
    L.wae_tall_read.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, dp]
    L.wae_tall_gram.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, dp]
    L.wae_tall_mul.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, dp, C.c_int32, dp, dp]
    L.wae_tall_hankel.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32]
    _lib = L
    return L


def check(code, warn_ok=True):
    if code < 0 or (code > 0 and not warn_ok):
        raise WaeError(code, lib().wae_last_error().decode(errors="replace"))
    return code


def zptr(a):
    """pointer to the interleaved (re,im) doubles of a complex128 array (must be contiguous)."""
    assert a.dtype == np.complex128
    return a.ctypes.data_as(C.POINTER(C.c_double))


def device_count():
    n = C.c_int(0)
    check(lib().wae_device_count(C.byref(n)))
    return n.value


def debug_vec(op, sizes, bufs, cmask=None, perm=None, device=0, raise_on_error=True):
    """wae_debug_vec (test hook, the family-free companion of DeviceFamily.debug_spmv): ONE launch of a streaming / reduction kernel
    on host arrays.  ``bufs``: C-contiguous complex128 arrays in the order include/waehip.h lists (None = an optional argument left
    out); every array is updated in place with what the device holds after the launch.  Returns (code, status word of the dense
    inversion); with raise_on_error=False a negative code is returned instead of raised."""
    for a in bufs:
        assert a is None or (a.dtype == np.complex128 and a.flags.c_contiguous and a.flags.writeable)
    sz = (C.c_int64 * len(sizes))(*[int(s) for s in sizes])
    dp = C.POINTER(C.c_double)
    ptrs = (dp * len(bufs))(*[None if a is None else zptr(a) for a in bufs])
    lens = (C.c_int64 * len(bufs))(*[0 if a is None else a.size for a in bufs])
    nb = int(sizes[1])
    cm = None if cmask is None else (C.c_uint8 * ((nb + 7) // 8))(*[1 if x else 0 for x in cmask])
    pm = None if perm is None else np.ascontiguousarray(perm, dtype=np.int32)
    status = C.c_int32(0)
    code = lib().wae_debug_vec(device, op, sz, len(sizes), ptrs, lens, len(bufs), cm,
                               None if pm is None else pm.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(status))
    if raise_on_error:
        check(code)
    return code, status.value


class GmresScript:
    """wae_debug_gmres (test hook): a script of INIT / STEP / PAIR / SOLVE_Y events for the recurrence kernels of the lock-step GMRES,
    run against one device state.  Build it with the four methods below (each returns the event's index), then run()."""

    def __init__(self, nb, m, n, histcap=None):
        self.nb, self.m, self.n = int(nb), int(m), int(n)
        self.histcap = int(histcap) if histcap is not None else self.m + 8
        self.ev, self.evd, self.parts, self.layout, self.plen = [], [], [], [], 0

    def _event(self, kind, j, use_mask, tol, lim, arrays):
        views, off = {}, self.plen
        for name, a in arrays:
            a = np.ascontiguousarray(a, dtype=np.complex128)
            views[name] = (self.plen, a.shape)
            self.parts.append(a.ravel())
            self.plen += a.size
        self.ev.append([kind, int(j), int(bool(use_mask)), off])
        self.evd.append([float(tol), float(lim)])
        self.layout.append(views)
        return len(self.ev) - 1

    def init(self, beta, done, use_mask):
        return self._event(GMRES_INIT, 0, use_mask, 0.0, 0.0, [("beta", beta), ("done", np.asarray(done, dtype=np.float64))])

    def step(self, j, hd, tol, lim, Vnew, use_mask):
        return self._event(GMRES_STEP, j, use_mask, tol, lim, [("hd", hd), ("Vnew", Vnew)])

    def pair(self, j, c1, c2, gram, norms, tol, lim, W1, W2, use_mask, sentinel=3 + 7j):
        nb = self.nb
        out = [("alpha", np.full(nb, sentinel)), ("c2m", np.full((j + 1, nb), sentinel)), ("hd2", np.full((j + 2, nb), sentinel))]
        return self._event(GMRES_PAIR, j, use_mask, tol, lim,
                           [("c1", c1), ("c2", c2), ("gram", gram), ("norms", norms), ("W1", W1), ("W2", W2)] + out)

    def solve_y(self, ju, sentinel=3 + 7j):
        return self._event(GMRES_SOLVE_Y, ju, 0, 0.0, 0.0, [("out", np.full((self.m, self.nb), sentinel))])

    def run(self, bnorm, device=0, raise_on_error=True, sentinel=3 + 7j, short=0):
        """Returns (code, result): result.events[e] holds the event's arrays as the device left them and its snapshot (relres, conv,
        steps, iters, histlen, stalled, status, cmask, rescale, sv, vsq); result.R, cs, sn, g, sv, vsq, Hraw, sub, hist the final state
        (entries no kernel wrote hold `sentinel`, its real part in the double arrays).  short: entries by which the pool's length is understated."""
        nb, m, n, hc = self.nb, self.m, self.n, self.histcap
        nev, nch, nint = len(self.ev), (nb + 7) // 8, 5 * nb + 4
        mm, mp = max(m, 0), max(m, 0) + 1
        pool = np.concatenate(self.parts) if self.parts else np.zeros(1, dtype=np.complex128)
        ev = np.ascontiguousarray(self.ev, dtype=np.int64).reshape(-1)
        evd = np.ascontiguousarray(self.evd, dtype=np.float64).reshape(-1)
        bn = np.ascontiguousarray(bnorm, dtype=np.float64)
        nR, nrow = mm * mp * max(nb, 0), mm * max(nb, 0)
        cstate = np.full(2 * nR + 3 * nrow + 3 * max(nb, 0), sentinel, dtype=np.complex128)
        dstate = np.full(3 * nrow + 2 * max(nb, 0) + max(hc, 0) * max(nb, 0), np.real(sentinel), dtype=np.float64)
        s_rel = np.zeros((nev, max(nb, 0)))
        s_int = np.zeros((nev, max(nint, 4)), dtype=np.int32)
        s_cm = np.zeros((nev, max(nch, 1)), dtype=np.uint8)
        s_resc = np.zeros((nev, max(nb, 0)), dtype=np.complex128)
        s_sv = np.zeros((nev, 2, max(nb, 0)))
        s_vsq = np.zeros((nev, 2, max(nb, 0)), dtype=np.complex128)
        dp = C.POINTER(C.c_double)
        code = lib().wae_debug_gmres(device, nb, m, hc, n, bn.ctypes.data_as(dp), ev.ctypes.data_as(C.POINTER(C.c_int64)), evd.ctypes.data_as(dp),
                                     nev, zptr(pool), pool.size - short, zptr(cstate), dstate.ctypes.data_as(dp), s_rel.ctypes.data_as(dp),
                                     s_int.ctypes.data_as(C.POINTER(C.c_int32)), s_cm.ctypes.data_as(C.POINTER(C.c_uint8)), zptr(s_resc),
                                     s_sv.ctypes.data_as(dp), zptr(s_vsq))
        if raise_on_error:
            check(code)
        if code < 0:
            return code, None

        class Result:
            pass
        res = Result()
        o = 0
        for name, cnt, shape in (("R", nR, (m, m + 1, nb)), ("sn", nrow, (m, nb)), ("g", nrow + nb, (m + 1, nb)), ("vsq", nrow + 2 * nb, (m + 2, nb)),
                                 ("Hraw", nR, (m, m + 1, nb))):
            setattr(res, name, cstate[o:o + cnt].reshape(shape))
            o += cnt
        o = 0
        for name, cnt, shape in (("cs", nrow, (m, nb)), ("sv", nrow + 2 * nb, (m + 2, nb)), ("sub", nrow, (m, nb)), ("hist", hc * nb, (hc, nb))):
            setattr(res, name, dstate[o:o + cnt].reshape(shape))
            o += cnt
        res.events = []
        for e, views in enumerate(self.layout):
            d = {k: pool[off:off + int(np.prod(shape))].reshape(shape) for k, (off, shape) in views.items()}
            ints = s_int[e, :5 * nb].reshape(5, nb)
            d.update(relres=s_rel[e], conv=ints[0], steps=ints[1], iters=ints[2], histlen=ints[3], stalled=ints[4],
                     status=s_int[e, 5 * nb:5 * nb + 3], cmask=s_cm[e, :nch], rescale=s_resc[e], sv=s_sv[e], vsq=s_vsq[e])
            res.events.append(d)
        return code, res
