"""ctypes binding of libmfcd_hip.so (C-ABI declared in include/mfcd.h).

There is no fallback: if the HIP library is not built, or a call is made without a GPU tensor,
this module raises.  PyTorch is used only to own device memory and streams.
"""
import ctypes
import os

import torch

_PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("MFCD_LIB") or os.path.join(_PKG_DIR, "libmfcd_hip.so")  # MFCD_LIB: diagnostic builds (tools/)

_vp, _i32, _i64, _dbl, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double, ctypes.c_size_t

# name -> (restype, argtypes); mirrors include/mfcd.h one to one
SIGNATURES = {
    "mfcd_abi_version": (_i32, []),
    "mfcd_error_string": (ctypes.c_char_p, [_i32]),
    "mfcd_check_samples": (_i32, [_vp, _i64, _i32, _i32, _vp, _vp]),
    "mfcd_eval_batches": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "mfcd_train_workspace_bytes": (_sz, [_i64, _i32, _i32, _i32, _i32]),
    "mfcd_train_workspace_init": (_i32, [_vp, _sz, _i64, _i32, _i32, _i32, _i32, _vp]),
    "mfcd_train_workspace_release": (_i32, [_vp]),
    "mfcd_set_train_path": (_i32, [_i32]),
    "mfcd_set_resident_math": (_i32, [_i32]),
    "mfcd_set_tuning": (_i32, [_i32, _i64]),
    "mfcd_train_plan_query": (_i32, [_i64, _i32, _i32, _i32, _i32, _i32, _vp]),
    "mfcd_train_steps": (_i32, [_vp] * 7 + [_i64, _i32, _i64, _i32, _i32, _i32] + [_dbl] * 5 + [_vp, _vp, _sz, _vp]),
    "mfcd_train_steps_bf16": (_i32, [_vp] * 7 + [_i64, _i32, _i64, _i32, _i32, _i32] + [_dbl] * 5 + [_vp, _vp, _sz, _vp]),
    "mfcd_eval_batches_bf16": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "mfcd_train_steps_timed": (_i32, [_vp] * 7 + [_i64, _i32, _i64, _i32, _i32, _i32] + [_dbl] * 5 +
                               [_vp, _vp, _sz, _vp, _vp]),
    "mfcd_train_call_prepare": (_i32, [_vp] * 6 + [_i32] * 5 + [_dbl] * 5 + [_vp, _sz, ctypes.POINTER(ctypes.c_void_p)]),
    "mfcd_train_call_run": (_i32, [_vp, _vp, _i64, _i64, _vp, _vp]),
    "mfcd_train_call_stage": (_i32, [_vp, _vp, _i64, _i64, _vp, _vp]),
    "mfcd_train_call_release": (_i32, [_vp]),
    "mfcd_local_model_bytes": (_sz, []),
    "mfcd_eval_model_bytes": (_sz, []),
    "mfcd_train_local_multi_workspace_bytes": (_sz, [_vp, _i32, ctypes.POINTER(_sz)]),
    "mfcd_eval_multi_workspace_bytes": (_sz, [_i32, ctypes.POINTER(_sz)]),
    "mfcd_multi_workspace_init": (_i32, [_vp, _sz, _sz]),
    "mfcd_train_steps_local_multi": (_i32, [_vp, _i32, _vp, _sz, _vp]),
    "mfcd_eval_batches_multi": (_i32, [_vp, _i32, _vp, _sz, _vp]),
    "mfcd_batch_coefficients": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "mfcd_apply_step": (_i32, [_vp] * 8 + [_i32, _i64, _i32, _i32, _i32] + [_dbl] * 5 + [_vp, _sz, _vp]),
    "mfcd_dense_grad": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "mfcd_dense_grad_from_coefficients": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp]),
    "mfcd_adam_dense": (_i32, [_vp] * 8 + [_i64, _i32, _i32, _i32] + [_dbl] * 5 + [_vp]),
    "mfcd_dp_unique_id": (_i32, [_vp, _sz]),
    "mfcd_dp_comm_create": (_i32, [_vp, _sz, _i32, _i32, ctypes.POINTER(ctypes.c_void_p)]),
    "mfcd_dp_comm_destroy": (_i32, [_vp]),
    "mfcd_dp_workspace_bytes": (_sz, [_i64, _i32, _i32, _i32, _i32, _i32]),
    "mfcd_dp_train_steps": (_i32, [_vp] * 7 + [_i64, _i32, _i32, _i32, _i64, _i32, _i32, _i32] + [_dbl] * 5 +
                            [_vp, _vp, _sz, _vp, _vp]),
    "mfcd_dp_train_steps_bf16": (_i32, [_vp] * 7 + [_i64, _i32, _i32, _i32, _i64, _i32, _i32, _i32] + [_dbl] * 5 +
                            [_vp, _vp, _sz, _vp, _vp]),
    "mfcd_shard_rows": (_i32, [_i32, _i32, _i32, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    "mfcd_shard_workspace_bytes": (_sz, [_i64, _i32, _i32]),
    "mfcd_shard_pack": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp]),
    "mfcd_shard_collisions": (_i32, [_vp, _i64, _i32, _vp, _vp]),
    "mfcd_shard_pack_ahead": (_i32, [_vp] * 7 + [_i32, _i32, _i64, _i32, _i32, _i32, _i32, _i32] + [_dbl] * 5 + [_vp, _vp]),
    "mfcd_shard_apply": (_i32, [_vp] * 7 + [_i32, _i32, _vp, _i64, _i32, _i32, _i32, _i32, _i32] + [_dbl] * 5 + [_vp, _vp]),
    "mfcd_shard_train_steps": (_i32, [_vp] * 7 + [_i64, _i32, _i32, _i32, _i64, _i32, _i32, _i32] + [_dbl] * 5 +
                               [_vp, _vp, _sz, _vp, _vp]),
    "mfcd_shard_train_steps_bf16": (_i32, [_vp] * 7 + [_i64, _i32, _i32, _i32, _i64, _i32, _i32, _i32] + [_dbl] * 5 +
                               [_vp, _vp, _sz, _vp, _vp]),
    "mfcd_uvt_workspace_bytes": (_sz, [_i32, _i32, _i32]),
    "mfcd_uvt_stats": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _dbl, _vp, _vp, _vp, _sz, _vp]),
    "mfcd_uvt_stats_select": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _dbl, _i32, _vp, _vp, _vp, _sz, _vp]),
    "mfcd_uvt_slab_workspace_bytes": (_sz, [_i32, _i32, _i32, _i32]),
    "mfcd_uvt_stats_slab": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _dbl, _i32, _i32, _i32, _vp, _vp, _vp, _sz, _vp]),
    "mfcd_uvt_rows": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp]),
    "mfcd_generate_labels": (_i32, [_vp, _i64, _vp, _i32, _i32, _vp, _vp, _i32, _dbl, _i32, _i32, ctypes.c_uint64, _vp,
                                     _vp]),
    "mfcd_train_big_workspace_bytes": (_sz, [_i64, _i32]),
    "mfcd_train_steps_big": (_i32, [_vp] * 7 + [_i64, _i32, _i64, _i32, _i32, _i32] + [_dbl] * 5 + [_vp, _vp, _sz, _vp]),
    "mfcd_train_big_status": (_i32, [_vp, ctypes.POINTER(ctypes.c_int), _vp]),
    "mfcd_train_big_slots": (_i32, []),
    "mfcd_train_big_check": (_i32, [_vp, _i64, _i32, _i32, _i32, _vp, _vp]),
    "mfcd_sample_workspace_bytes": (_sz, [_i64, _i64]),
    "mfcd_sample_triplets": (_i32, [_vp, _vp, _i64, _i64, _i64, ctypes.c_uint64, _i64, _vp, _vp, _vp, _vp, _sz, _vp]),
    "mfcd_spearman_max_columns": (_i32, []),
    "mfcd_spearman_rows": (_i32, [_vp, _i64, _vp, _i64, _i32, _i32, _vp, _vp]),
    "mfcd_spearman_long_workspace_bytes": (_sz, [_i32, _i32]),
    "mfcd_spearman_rows_long": (_i32, [_vp, _i64, _vp, _i64, _i32, _i32, _vp, _vp, _sz, _vp]),
    "mfcd_topk_max_k": (_i32, []),
    "mfcd_topk_rows_workspace_bytes": (_sz, [_i32] * 5),
    "mfcd_topk_rows": (_i32, [_vp, _i64, _vp, _vp, _i32, _vp] + [_i32] * 5 + [_vp] * 7 + [_sz, _vp]),
    "mfcd_kmeans_max_k": (_i32, []),
    "mfcd_kmeans_workspace_bytes": (_sz, [_i64, _i64, _i32]),
    "mfcd_kmeans_assign": (_i32, [_vp, _i64, _i64, _vp, _i32, _vp, _vp, _vp, _vp, _sz, _vp]),
    "mfcd_kmeans_update": (_i32, [_vp, _i64, _i64, _vp, _i32, _vp, _vp, _vp, _sz, _vp]),
    "mfcd_pair_stats_workspace_bytes": (_sz, [_i32, _i32]),
    "mfcd_pair_stats_rows": (_i32, [_vp, _i64, _vp, _i64, _i32, _i32, _dbl, _i32, _vp, _vp, _vp, _sz, _vp]),
    "mfcd_pair_grad_rows": (_i32, [_vp, _i64, _vp, _i64, _i32, _i32, _dbl, _vp, _i64, _vp]),
    "mfcd_pair_law_stats_workspace_bytes": (_sz, [_i32, _i32]),
    "mfcd_pair_law_stats_rows": (_i32, [_vp, _i64, _vp, _i64, _i32, _i32, _dbl, _vp, _vp, _vp, _vp, _sz, _vp]),
    "mfcd_pair_law_grad_rows": (_i32, [_vp, _i64, _vp, _i64, _i32, _i32, _dbl, _vp, _vp, _i64, _vp]),
    "mfcd_pair_hvp_rows": (_i32, [_vp, _i64, _vp, _i64, _i32, _i32, _vp, _i64, _vp, _i64, _vp]),
    "mfcd_pair_law_hvp_rows": (_i32, [_vp, _i64, _vp, _i64, _vp, _i64, _i32, _i32, _vp, _vp, _i64, _vp, _i64, _vp]),
    "mfcd_pair_hvp_multi_workspace_bytes": (_sz, [_i32, _i32, _i32]),
    "mfcd_pair_hvp_multi_rows": (_i32, [_vp, _i64, _vp, _i64, _vp, _i64, _i32, _i32, _vp, _i64, _i32, _i32, _vp, _vp, _i64, _vp,
                                        _i64, _vp, _sz, _vp]),
    "mfcd_pair_best_workspace_bytes": (_sz, [_i32, _i32, _i32]),
    "mfcd_pair_best_rows": (_i32, [_vp, _i64, _vp, _i64, _vp, _i64, _i64, _i32, _i32, _i32, _vp, _vp, _i64, _vp, _i64, _vp, _sz,
                                   _vp]),
    "mfcd_fold_in_max_d": (_i32, []),
    "mfcd_fold_in_chunk": (_i32, []),
    "mfcd_fold_in_workspace_bytes": (_sz, [_i32, _i32]),
    "mfcd_fold_in_users": (_i32, [_vp, _i32, _i32, _vp, _vp, _i32, _dbl, _vp, _i32, _dbl, _vp, _vp, _vp, _vp, _sz, _vp]),
    "mfcd_item_step_workspace_bytes": (_sz, [_i32, _i32, _i64]),
    "mfcd_item_step": (_i32, [_vp, _i32, _vp, _i32, _i32, _vp, _vp, _vp, _i32, _dbl, _dbl, _i32, _dbl, _vp, _vp, _vp, _vp,
                              _sz, _vp]),
    "mfcd_fold_in_cg_max_d": (_i32, []),
    "mfcd_fold_in_cg_chunk": (_i32, [_i32]),
    "mfcd_fold_in_cg_resident": (_i32, [_i32]),
    "mfcd_fold_in_cg_workspace_bytes": (_sz, [_i32, _i32, _i64]),
    "mfcd_fold_in_users_cg": (_i32, [_vp, _i32, _i32, _vp, _vp, _i32, _dbl, _vp, _i32, _dbl, _vp, _vp, _vp, _vp, _vp, _sz,
                                     _vp]),
    "mfcd_item_step_cg_workspace_bytes": (_sz, [_i32, _i32, _i64]),
    "mfcd_item_step_cg": (_i32, [_vp, _i32, _vp, _i32, _i32, _vp, _vp, _vp, _i32, _dbl, _dbl, _i32, _dbl, _vp, _vp, _vp, _vp,
                                 _vp, _sz, _vp]),
    "mfcd_triplet_rows_segment": (_i32, []),
    "mfcd_triplet_rows_workspace_bytes": (_sz, [_i32, _i32, _i64]),
    "mfcd_triplet_rows": (_i32, [_i32, _i32, _i32, _vp, _i32, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _i64, _dbl,
                                 _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "mfcd_pair_ragged_tile": (_i32, []),
    "mfcd_pair_ragged_workspace_bytes": (_sz, [_i32, _i64]),
    "mfcd_pair_ragged_stats": (_i32, [_vp, _vp, _i64, _vp, _i32, _vp, _i64, _dbl, _i32, _i32, _vp, _vp, _vp, _vp, _sz, _vp]),
    "mfcd_pair_ragged_grad": (_i32, [_vp, _vp, _i64, _vp, _i32, _vp, _i64, _dbl, _i32, _vp, _vp, _vp]),
    "mfcd_pair_ragged_hvp": (_i32, [_vp, _vp, _vp, _i64, _vp, _i32, _vp, _i64, _i32, _vp, _vp, _vp, _vp]),
    "mfcd_ragged_dot": (_i32, [_vp, _i32, _vp, _i32, _i32, _i64, _vp, _i32, _vp, _vp, _vp, _vp]),
    "mfcd_ragged_segment": (_i32, []),
    "mfcd_ragged_gather_sum_workspace_bytes": (_sz, [_i32, _i32, _i64]),
    "mfcd_ragged_gather_sum": (_i32, [_vp, _i32, _i32, _i64, _vp, _i32, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _sz, _vp]),
    "mfcd_ratings_fold_in_max_d": (_i32, []),
    "mfcd_ratings_fold_in_max_len": (_i32, []),
    "mfcd_ratings_fold_in_workspace_bytes": (_sz, [_i32, _i32, _i64]),
    "mfcd_ratings_fold_in_users": (_i32, [_vp, _i32, _i32, _vp, _vp, _i64, _vp, _i32, _dbl, _i32, _dbl, _dbl, _vp, _i32, _dbl,
                                          _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "mfcd_rank_entries_workspace_bytes": (_sz, [_i32, _i32, _i32, _i64]),
    "mfcd_rank_entries": (_i32, [_vp, _i64, _vp, _vp, _i32, _vp, _i32, _i32, _i32, _vp, _vp, _i64, _vp, _vp, _i64] +
                          [_vp] * 6 + [_sz, _vp]),
    "mfcd_implicit_chunk": (_i32, []),
    "mfcd_implicit_tile": (_i32, []),
    "mfcd_implicit_rows_workspace_bytes": (_sz, [_i32, _i32, _i32]),
    "mfcd_implicit_rows": (_i32, [_vp, _i64, _vp, _vp, _i32, _vp, _i32, _i32, _i32, _vp, _vp, _i64, _vp, _vp, _i64] +
                           [_vp] * 4 + [_i64, _vp, _vp, _sz, _vp]),
    "mfcd_implicit_hvp_rows_workspace_bytes": (_sz, [_i32, _i32, _i32]),
    "mfcd_implicit_hvp_rows": (_i32, [_vp, _i64, _vp, _i64] + [_vp] * 4 + [_i32, _vp, _i32, _i32, _i32, _vp, _vp, _i64, _vp,
                                      _vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _sz, _vp]),
    "mfcd_implicit_fold_in_max_d": (_i32, []),
    "mfcd_implicit_fold_in_max_pos": (_i32, []),
    "mfcd_implicit_fold_in_max_pairs": (_i64, []),
    "mfcd_implicit_fold_in_chunk": (_i32, []),
    "mfcd_implicit_fold_in_workspace_bytes": (_sz, [_i32, _i32, _i32]),
    "mfcd_implicit_fold_in_users": (_i32, [_vp, _i32, _i32, _vp, _vp, _i64, _vp, _vp, _i64, _i32, _vp, _dbl, _vp, _i32, _dbl,
                                           _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "mfcd_list_pl_tile": (_i32, []),
    "mfcd_list_pl_workspace_bytes": (_sz, [_i32, _i64]),
    "mfcd_list_pl": (_i32, [_vp, _i64, _vp, _vp, _i32, _vp, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "mfcd_list_pl_hvp_workspace_bytes": (_sz, [_i32, _i64]),
    "mfcd_list_pl_hvp": (_i32, [_vp, _vp, _i64, _vp, _vp, _i32, _vp, _i64, _vp, _vp, _vp, _vp, _sz, _vp]),
}

TUNE_KEYS = {"resident_lookahead": 3, "resident_spin_limit": 5, "uvt_target_wgs": 9, "uvt_min_stages": 10,
             "uvt_split": 11, "shard_pipeline": 13}


class TrainPlan(ctypes.Structure):
    """mfcd_train_plan of include/mfcd.h."""
    _fields_ = [(k, ctypes.c_int32) for k in ("form", "resident_q", "resident_waves", "resident_blocks",
                                               "resident_lookahead", "fast_math", "streaming_vec",
                                               "streaming_chunks", "streaming_blocks", "device_cus")] + \
               [("reserved", ctypes.c_int32 * 6)]


class LocalModel(ctypes.Structure):
    """mfcd_local_model of include/mfcd.h (one model of mfcd_train_steps_local_multi)."""
    _fields_ = [(k, _vp) for k in ("U", "V", "mU", "vU", "mV", "vV", "samples")] + \
               [("N", ctypes.c_int64), ("step0", ctypes.c_int64)] + [(k, ctypes.c_int32) for k in ("B", "n", "m", "d")] + \
               [(k, _dbl) for k in ("lr", "beta1", "beta2", "eps", "weight_decay")] + [("loss_per_step", _vp)]


class EvalModel(ctypes.Structure):
    """mfcd_eval_model of include/mfcd.h (one model of mfcd_eval_batches_multi)."""
    _fields_ = [(k, _vp) for k in ("U", "V", "samples")] + [("N", ctypes.c_int64)] + \
               [(k, ctypes.c_int32) for k in ("B", "n", "m", "d")] + [("loss_per_batch", _vp), ("correct_per_batch", _vp)]


class Sampler(ctypes.Structure):
    """mfcd_sampler of include/mfcd.h."""
    _fields_ = [("law", ctypes.c_int32), ("n", ctypes.c_int32), ("m", ctypes.c_int32), ("pair_rule", ctypes.c_int32),
                ("cdf", _vp), ("list_i", _vp), ("list_j", _vp), ("k", ctypes.c_int32),
                ("list_row_stride", ctypes.c_int32), ("users", _vp), ("n_users", ctypes.c_int32),
                ("use_margin", ctypes.c_int32), ("margin", _dbl), ("X", _vp), ("A", _vp), ("B", _vp),
                ("dx", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class PairLawC(ctypes.Structure):
    """mfcd_pair_law of include/mfcd.h."""
    _fields_ = [("alpha", _vp), ("beta", _vp), ("labels", _vp), ("label_stride", ctypes.c_int64),
                ("use_margin", ctypes.c_int32), ("reserved", ctypes.c_int32), ("margin", _dbl)]


_lib = None


class MfcdError(RuntimeError):
    pass


def load():
    """Load the shared library and bind every declared symbol (no GPU needed for this)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise MfcdError(
                f"{LIB_PATH} is missing: the HIP hot path has not been built "
                "(run `python -c 'import __graft_entry__ as g; g.build()'` or make -C csrc). "
                "There is no CPU fallback.")
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError if the library does not export it
            fn.restype, fn.argtypes = res, args
        if lib.mfcd_abi_version() != 4:
            raise MfcdError("libmfcd_hip.so ABI version mismatch")
        _lib = lib
    return _lib


def check(code):
    if code != 0:
        raise MfcdError(load().mfcd_error_string(code).decode())


def ptr(t):
    """Raw device pointer of a CUDA(HIP) tensor; None -> NULL."""
    if t is None:
        return None
    if not t.is_cuda:
        raise MfcdError("the HIP hot path needs tensors on a GPU device (got a CPU tensor)")
    if not t.is_contiguous():
        raise MfcdError("the HIP hot path needs contiguous tensors")
    return t.data_ptr()


def is_factored(X):
    """X is kept as its factors, X = A @ B.T (a generation_data.FactoredMatrix, told by its shape: this package does
    not import that module)."""
    return not torch.is_tensor(X) and hasattr(X, "A") and hasattr(X, "B")


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)   # the handle without building a Stream object


def stream_ptr(device=None):
    if _raw_stream is not None and isinstance(device, torch.device) and device.index is not None:
        return _raw_stream(device.index)
    return torch.cuda.current_stream(device).cuda_stream


_workspaces = {}    # (device index, stream handle) -> the scratch buffer of the row kernels


def workspace(nbytes, device):
    """Scratch for one kernel call: a uint8 buffer of at least `nbytes` (256 at the least), grow-only, one per (device,
    current stream): work on two streams of a device is not ordered, so it may not share scratch.  No kernel expects
    anything of its contents.  Fetch it per call: a later request on the same stream may replace it by a larger one.
    An entry is never dropped: a process keeps the high-water mark of every stream it ran a row kernel on."""
    index = torch.device(device).index             # "cuda" and "cuda:0" are one device
    key = (torch.cuda.current_device() if index is None else index, stream_ptr(device))
    buf = _workspaces.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = _workspaces[key] = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
    return buf


def row_pair(A, X, who):
    """Two [rows, m] matrices of a row kernel, checked → (A, X, rows, m, lda, ldx): float32, on a GPU, of one shape, unit
    column stride (copies otherwise), leading dimensions in elements (m for a single row: its stride says nothing)."""
    if not torch.is_tensor(A) or not torch.is_tensor(X) or A.dim() != 2 or X.shape != A.shape \
            or A.dtype != torch.float32 or X.dtype != torch.float32 or not A.is_cuda or not X.is_cuda:
        raise MfcdError(f"{who} needs two float32 GPU matrices of the same shape (no CPU fallback)")
    rows, m = A.shape
    if A.stride(1) != 1 or X.stride(1) != 1:
        A, X = A.contiguous(), X.contiguous()
    return A, X, rows, m, (A.stride(0) if rows > 1 else m), (X.stride(0) if rows > 1 else m)
