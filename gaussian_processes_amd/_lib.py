"""ctypes binding of libgpfit_mi355x.so (the C ABI declared in include/gpfit_mi355x.h).

The product path has NO fallback: if the HIP library is missing or a call fails, an
exception is raised."""
from __future__ import annotations

import ctypes
import os

from .build import lib_path

vp, i32, i64, f64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double
pd = ctypes.POINTER(ctypes.c_double)



class DevGemmArgs(ctypes.Structure):
    """gpfit_dev_gemm_args (test hooks of include/gpfit_mi355x.h)."""
    _fields_ = ([(n, vp) for n in ("A", "B", "C")] + [(n, i64) for n in ("lda", "ldb", "ldc", "sA", "sB", "sC")] +
                [("alpha", f64), ("beta", f64)] +
                [(n, vp) for n in ("sk_ws", "aux", "sumsq", "Ap", "Bp", "Cp", "auxp", "sumsqp")] +
                [(n, ctypes.c_int32) for n in ("M", "N", "K", "a_kmajor", "b_kmajor", "out_lower", "a_tri", "b_tri", "batch",
                                               "split_k", "tile", "walk", "epi", "nptr", "k_slabs", "b_split")])


class DevGemmRoute(ctypes.Structure):
    """gpfit_dev_gemm_route_t."""
    _fields_ = [(n, ctypes.c_int32) for n in ("rc", "tile", "sk_first", "xcd", "stages", "half_occ", "edge", "epi",
                                              "sumsq_entries", "blocks", "pair", "slabs")]


class DevEwArgs(ctypes.Structure):
    """gpfit_dev_ew_args (test hooks of include/gpfit_mi355x.h): the slots of gpfit_dev_elementwise."""
    _fields_ = [("p", vp * 16), ("ld", i64 * 4), ("n", ctypes.c_int32 * 4), ("s", f64 * 2), ("theta", f64 * 8),
                ("n_units", ctypes.c_int32), ("up", ctypes.POINTER(vp) * 8), ("uld", ctypes.POINTER(i64) * 4),
                ("un", ctypes.POINTER(ctypes.c_int32) * 4), ("us", pd * 2)]


# the op numbers of gpfit_dev_elementwise, in the order of the header's enum; a group form is op + EW_GROUP
EW_OPS = ("trmv_lower", "trmv_lower_t", "symv_lower", "gemv_sub", "gemv_t_sub", "dot", "logdet", "logdet_pair", "frob_lower",
          "frob_tiles", "reduce_slices", "reduce_slabs", "reduce_slices_sym", "pack_lower", "pack_tri", "unpack_sym",
          "unpack_tri", "symmetrize", "symmetrize_avg", "pad_copy", "gather", "estep_build", "add_diag", "axpby_block",
          "demote_block", "qvec", "moments", "adjoint", "adjoint_reduce", "adjoint_rect", "metric_contract", "dk_sigma0", "dq",
          "dk_metric", "estep_prep", "rowscale_add")
EW_OP = {name: k for k, name in enumerate(EW_OPS)}
EW_GROUP = 256


class DevSkinnyArgs(ctypes.Structure):
    """gpfit_dev_skinny_args: the fields of SkinnyArgs and SkinnySumArgs and the arguments of the finish launcher."""
    _fields_ = [("A", vp), ("sam", i64), ("sar", i64), ("B", vp), ("sbr", i64), ("sbc", i64), ("O", vp), ("soz", i64),
                ("som", i64), ("soc", i64), ("alpha", f64), ("M", ctypes.c_int32), ("K", ctypes.c_int32),
                ("kc", ctypes.c_int32), ("tri", ctypes.c_int32), ("P", vp), ("pz", i64), ("nslab", ctypes.c_int32),
                ("mode", ctypes.c_int32), ("dst", vp), ("L", vp), ("ldl", i64), ("Li", vp), ("ldi", i64), ("Kc", vp),
                ("ldk", i64), ("n", ctypes.c_int32), ("Lt", vp), ("Lit", vp), ("logdet", vp)]


class DevProjArgs(ctypes.Structure):
    """gpfit_dev_proj_args: the slots of gpfit_dev_projected."""
    _fields_ = [(n, ctypes.c_int32) for n in ("n_units", "n", "np", "nb", "nrows", "npc")] + [
        ("ld", i64), ("lda", i64), ("A", f64), ("up", ctypes.POINTER(vp) * 13), ("uA", pd), ("ulambda0", pd),
        ("un", ctypes.POINTER(ctypes.c_int32)), ("p", vp * 6)]


# the op numbers of gpfit_dev_skinny and gpfit_dev_projected, in the order of the header's enums
SKINNY_OP = {name: k for k, name in enumerate(("slabs", "sum", "finish"))}
PROJ_OP = {name: k for k, name in enumerate(("moments", "ga", "gkb", "gktb", "trace", "estep_rows", "estep_scale",
                                             "estep_moments"))}


_SIGS = {
    "gpfit_version": (i32, []),
    "gpfit_last_error": (ctypes.c_char_p, []),
    "gpfit_dgemm": (i32, [vp, i32, i32, i32, i32, i32, f64, vp, i64, vp, i64, f64, vp, i64, i32, i32, i32]),
    "gpfit_dgemm_ex": (i32, [vp, i32, i32, i32, i32, i32, f64, vp, i64, vp, i64, f64, vp, i64, i32, i32, i32, i32, i32]),
    "gpfit_ctx_create": (i32, [i32, i64, i64, i64, ctypes.POINTER(vp)]),
    "gpfit_ctx_destroy": (None, [vp]),
    "gpfit_check_limits": (i32, [pd, pd, pd]),
    "gpfit_localker_mask": (i32, [pd, i32, i32, vp, ctypes.POINTER(i64)]),
    "gpfit_localker": (i32, [vp, vp, pd, i32, i32, vp, i64, vp, vp]),
    "gpfit_acosker": (i32, [vp, vp, f64, vp, i64, i64, vp, i64, i64, i64, vp, i64, vp, vp, i64, vp]),
    "gpfit_acosker_pullback": (i32, [vp, vp, f64, vp, i64, i64, vp, i64, i64, i64, vp, i64, vp, i64, vp, vp, i64, pd]),
    "gpfit_acosker_diag": (i32, [vp, vp, f64, vp, i64, i64, i64, vp, i64, vp, vp, vp]),
    "gpfit_fit_eval": (i32, [vp, vp, pd, pd, pd, i32, i32, vp, i64, i64, vp, vp, vp, i64, f64, f64, i32, pd,
                             vp, vp, vp]),
    "gpfit_potrf": (i32, [vp, vp, vp, i64, i64, vp, i64, vp, i64, pd, ctypes.POINTER(i32)]),
    "gpfit_potrf_append": (i32, [vp, vp, vp, i64, vp, i64, i64, vp, pd, ctypes.POINTER(i32)]),
    "gpfit_potrf_append_block": (i32, [vp, vp, vp, i64, vp, i64, i64, i64, vp, i64, pd, ctypes.POINTER(i32)]),
    "gpfit_estep": (i32, [vp, vp, vp, i64, i64, vp, vp, vp, f64, vp, vp, i64]),
    "gpfit_estep_projected": (i32, [vp, vp, vp, i64, vp, i64, vp, i64, i64, i64, vp, vp, vp, f64, vp, vp, i64, vp, vp,
                                    vp]),
    "gpfit_estep_projected_damped": (i32, [vp, vp, vp, i64, vp, i64, vp, i64, vp, i64, vp, i64, i64, i64, vp, vp, vp, f64, f64,
                                           vp, vp, i64, ctypes.POINTER(i32)]),
    "gpfit_fparam_eval": (i32, [vp, vp, vp, vp, vp, i64, f64, i32, f64, vp, pd]),
    "gpfit_fparam_lbfgs": (i32, [vp, vp, vp, vp, vp, i64, f64, i32, f64, i32, i32, f64, f64, f64, vp, pd]),
    "gpfit_estep_chain": (i32, [vp, vp, vp, i64, vp, i64, vp, i64, i64, i64, vp, vp, vp, vp, vp, i64, vp, vp, f64, i32, f64,
                                i32, i32, i32, f64, f64, f64, pd]),
    "gpfit_estep_chain_full": (i32, [vp, vp, vp, i64, i64, vp, vp, vp, vp, vp, i64, vp, vp, f64, i32, f64, i32, i32, i32, f64,
                                     f64, f64, pd]),
    "gpfit_estep_chain_batch": (i32, [vp, i32, vp, vp, vp, vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, pd, i32, pd,
                                      i32, i32, i32, f64, f64, f64, pd]),
    "gpfit_estep_chain_full_batch": (i32, [vp, i32, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, pd, i32, pd, i32, i32, i32,
                                           f64, f64, f64, pd]),
    "gpfit_estep_chain_damped": (i32, [vp, vp, vp, i64, vp, i64, vp, i64, vp, i64, i64, i64, vp, vp, vp, vp, vp, i64, vp, vp,
                                       f64, f64, i32, f64, i32, i32, i32, f64, f64, f64, pd]),
    "gpfit_estep_chain_damped_batch": (i32, [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp,
                                             vp, pd, f64, i32, pd, i32, i32, i32, f64, f64, f64, pd]),
    "gpfit_elbo": (i32, [vp, vp, vp, vp, i64, vp, i64, vp, i64, i64, i32, f64, vp, vp, vp, i64, f64, f64, pd,
                         ctypes.POINTER(i32)]),
    "gpfit_elbo_batch": (i32, [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, ctypes.POINTER(i32), pd, vp, vp, vp, i64, pd, pd, pd,
                               ctypes.POINTER(i32)]),
    "gpfit_subspace_sweeps": (i32, [vp, vp, vp, i64, i64, i64, vp, vp, vp, vp, i32, pd, i32, ctypes.POINTER(i32)]),
    "gpfit_subspace_sweeps_batch": (i32, [vp, i32, vp, vp, i64, i64, i64, vp, vp, vp, vp, ctypes.POINTER(i32), vp, i32,
                                          ctypes.POINTER(i32)]),
    "gpfit_sign_steps": (i32, [vp, vp, vp, i64, f64, vp, vp, vp, i32, pd, i32, i32, ctypes.POINTER(i32)]),
    "gpfit_sign_steps_batch": (i32, [vp, i32, vp, vp, i64, pd, vp, vp, vp, i32, pd, i32, i32, ctypes.POINTER(i32)]),
    "gpfit_fparam_lbfgs_host": (i32, [vp, vp, vp, i64, f64, i32, f64, i32, i32, f64, f64, f64, vp, pd]),
    "gpfit_set_profile": (i32, [vp, i32]),
    "gpfit_get_profile": (i32, [vp, pd]),
    "gpfit_get_phases": (i32, [vp, pd]),
    "gpfit_last_enqueue_ms": (f64, [vp]),
    "gpfit_fit_eval_f32": (i32, [vp, vp, pd, pd, pd, i32, i32, vp, i64, i64, vp, vp, vp, i64, f64, f64, i32, pd,
                                 vp, vp, vp]),
    "gpfit_fit_eval_finish": (i32, [vp, pd]),
    "gpfit_fit_eval_batch": (i32, [vp, i32, vp, pd, pd, pd, i32, i32, vp, i64, i64, vp, vp, vp, i64, pd, pd, i32, pd,
                                   ctypes.POINTER(i32)]),
    "gpfit_fit_eval_batch_f32": (i32, [vp, i32, vp, pd, pd, pd, i32, i32, vp, i64, i64, vp, vp, vp, i64, pd, pd, i32, pd,
                                       ctypes.POINTER(i32)]),
    "gpfit_fit_eval_projected": (i32, [vp, vp, pd, pd, pd, i32, i32, vp, i64, i64, vp, vp, i64, i64, vp, vp, i64, f64, f64, pd]),
    "gpfit_fit_eval_projected_batch": (i32, [vp, i32, vp, pd, pd, pd, i32, i32, vp, i64, i64, vp, vp, vp, vp, vp, vp, vp, pd, pd,
                                             pd, ctypes.POINTER(i32)]),
    "gpfit_fit_eval_sparse": (i32, [vp, vp, pd, pd, pd, i32, i32, vp, i64, i64, vp, i64, i64, vp, vp, i64, i64, vp, vp, i64,
                                    f64, f64, pd]),
    "gpfit_fit_eval_sparse_batch": (i32, [vp, i32, vp, pd, pd, pd, i32, i32, vp, i64, i64, vp, i64, i64, vp, vp, vp, vp, vp,
                                          vp, vp, pd, pd, pd, ctypes.POINTER(i32)]),
    "gpfit_grad_pullback": (i32, [vp, vp, pd, i32, i32, vp, i64, i64, vp, i64, vp, pd]),
    "gpfit_nd_utility": (i32, [vp, vp, vp, i64, vp, i32, vp]),
    "gpfit_score_pool": (i32, [vp, vp, f64, vp, i64, i64, vp, i64, vp, i64, i64, i64, vp, i64, vp, i64, i64, vp, i64, vp,
                               f64, f64, vp, i32, i64, vp, vp, vp, vp]),
    "gpfit_score_pool_batch": (i32, [vp, i32, vp, pd, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, pd, pd,
                                     vp, i32, i64, vp, vp, vp, vp]),
    "gpfit_utility_sum": (i32, [vp, vp, i64, i32, vp, i64, vp]),
    "gpfit_pool_covariance": (i32, [vp, vp, f64, vp, i64, i64, vp, i64, vp, i64, i64, i64, vp, i64, vp, i64, i64, vp, i64, vp,
                                    i64]),
    "gpfit_select_batch": (i32, [vp, i32, vp, vp, i64, vp, pd, pd, pd, vp, i32, i32, vp, vp, vp, vp]),
    "gpfit_probe_mfma_f64": (i32, [vp, vp, i32, i32]),
    "gpfit_probe_stream_copy": (i32, [vp, vp, vp, i64]),
    # test hooks
    "gpfit_dev_gemm_route": (i32, [i32, ctypes.POINTER(DevGemmArgs), ctypes.POINTER(DevGemmArgs), ctypes.POINTER(DevGemmRoute)]),
    "gpfit_dev_gemm_plan": (i64, [i32, ctypes.POINTER(DevGemmArgs), i32, ctypes.POINTER(ctypes.c_int32), i64]),
    "gpfit_dev_gemm": (i32, [vp, i32, ctypes.POINTER(DevGemmArgs), ctypes.POINTER(DevGemmArgs)]),
    "gpfit_dev_ctx_copy": (i32, [vp, ctypes.c_char_p, i64, vp, i64, i32]),
    "gpfit_dev_ctx_fill": (i32, [vp, ctypes.c_char_p, i32]),
    "gpfit_dev_ctx_buffer_name": (i32, [i32, ctypes.c_char_p, i32]),
    "gpfit_dev_potrf": (i32, [vp, vp, i32, i32, vp, vp, vp, vp, vp, i64, i32, ctypes.c_uint32, ctypes.c_uint32, i32]),
    "gpfit_dev_elementwise": (i32, [vp, vp, i32, i32, ctypes.POINTER(DevEwArgs)]),
    "gpfit_dev_skinny": (i32, [vp, vp, i32, ctypes.POINTER(DevSkinnyArgs)]),
    "gpfit_dev_projected": (i32, [vp, vp, i32, ctypes.POINTER(DevProjArgs)]),
}

_lib = None


class GpfitError(RuntimeError):
    pass


def exported_symbols():
    return sorted(_SIGS)


def load():
    """Load the shared library (once).  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise GpfitError(
            f"{path} not found: build it with `python -m gaussian_processes_amd.build` "
            "(there is no CPU fallback for the GP fit path)")
    lib = ctypes.CDLL(path)
    for name, (res, args) in _SIGS.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def last_error() -> str:
    return load().gpfit_last_error().decode(errors="replace")


def check(rc: int, what: str):
    if rc < 0 and rc != -2:
        raise GpfitError(f"{what} failed (rc={rc}): {last_error()}")
    return rc


def darr(values):
    return (ctypes.c_double * len(values))(*[float(v) for v in values])
