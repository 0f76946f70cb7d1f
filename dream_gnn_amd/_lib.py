"""ctypes binding of ``libdgmi.so`` (the C ABI declared in ``include/dgmi.h``).

The library is built in-tree by ``__graft_entry__.build()`` / ``csrc/Makefile``.  A missing
library is an error at import time: the product path has no fallback.
"""
from __future__ import annotations

import ctypes
import os

import torch  # noqa: F401  -- must come first: libdgmi.so binds to the HIP runtime torch already loaded

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libdgmi.so")
TORCH_LIB_PATH = os.path.join(_HERE, "libdgmi_torch.so")  # the dreamgnn_mi::* dispatcher ops over the C ABI

ABI_VERSION = 20

# name -> (restype, argtypes); mirrors include/dgmi.h one to one.
_vp = ctypes.c_void_p
_i64 = ctypes.c_int64
_EPI = [ctypes.c_int32, ctypes.c_float, _vp, _i64, ctypes.c_float]  # act, act_slope, out_mask, ld_mask, out_mask_scale


SIGNATURES = {
    "dgmi_abi_version": (ctypes.c_int, []),
    "dgmi_status_string": (ctypes.c_char_p, [ctypes.c_int]),
    "dgmi_device_ok": (ctypes.c_int, []),
    "dgmi_csr_from_coo_i32": (ctypes.c_int, [_vp, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp,
                                             ctypes.POINTER(ctypes.c_size_t), _vp]),
    "dgmi_spmm_csr_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, ctypes.c_int32, _vp, _i64, _vp, _vp, _vp, _i64, _i64,
                                         _i64, _i64] + _EPI + [_vp]),
    "dgmi_gather_f32": (ctypes.c_int, [_vp, _vp, _i64, _vp, _vp]),
    "dgmi_gather_concat_f32": (ctypes.c_int, [_vp, _vp, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _vp]),
    "dgmi_csr_sliced_from_coo_i32": (ctypes.c_int, [_vp, _vp, _i64, _i64, _i64, ctypes.c_int32, _vp, _vp, _vp, _vp,
                                                    ctypes.POINTER(ctypes.c_size_t), _vp]),
    "dgmi_csr_sliced_from_csr_i32": (ctypes.c_int, [_vp, _vp, _vp, _i64, _i64, _i64, ctypes.c_int32, _vp, _vp, _vp, _vp,
                                                    ctypes.POINTER(ctypes.c_size_t), _vp]),
    "dgmi_spmm_sliced_planes_bytes": (ctypes.c_size_t, [_i64, ctypes.c_int32, _i64]),
    "dgmi_spmm_sliced_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, ctypes.c_int32, _vp, _i64, _vp, _vp, _vp, _i64, _i64,
                                            _i64, _i64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _vp, ctypes.c_size_t] + _EPI
                             + [_vp]),
    "dgmi_knn_cosine_supported": (ctypes.c_int, [_i64, _i64, _i64]),
    "dgmi_knn_cosine_workspace_bytes": (ctypes.c_size_t, [_i64, _i64, ctypes.c_int32]),
    "dgmi_knn_cosine_topk_f32": (ctypes.c_int, [_vp, _i64, _i64, _i64, ctypes.c_int32, _vp, _vp, ctypes.c_size_t, _vp]),
    "dgmi_probe_row_gather_f32": (ctypes.c_int, [_vp, _i64, _i64, _i64, _i64, _i64, ctypes.c_int32, _vp, _vp]),
    "dgmi_epilogue_backward_f32": (ctypes.c_int, [_vp, _vp, _vp, _i64, ctypes.c_int32, ctypes.c_float, ctypes.c_float, _vp, _vp]),
    "dgmi_gather_add_f32": (ctypes.c_int, [_vp, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, ctypes.c_int32, _vp]),
    "dgmi_random_subset_workspace_bytes": (ctypes.c_size_t, []),
    "dgmi_random_subset_mask_f32": (ctypes.c_int, [_i64, _i64, ctypes.c_uint64, _vp, _vp, ctypes.c_size_t, _vp]),
    "dgmi_spmm_default_chunk": (ctypes.c_int32, [_i64, _i64]),
    "dgmi_spmm_plan_bytes": (ctypes.c_size_t, [_i64, _i64, ctypes.c_int32]),
    "dgmi_spmm_partials_bytes": (ctypes.c_size_t, [_i64, ctypes.c_int32, _i64]),
    "dgmi_spmm_plan_build": (ctypes.c_int, [_vp, _i64, _i64, ctypes.c_int32, _vp, ctypes.c_size_t, _vp,
                                            ctypes.POINTER(ctypes.c_size_t), _vp]),
    "dgmi_spmm_csr_planned_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, ctypes.c_int32, _vp, _i64, _vp, _vp, _vp, _i64,
                                                 _i64, _i64, _i64, _i64, ctypes.c_int32, _vp, _vp, ctypes.c_size_t] + _EPI
                                  + [_vp]),
    "dgmi_random_subset_select": (ctypes.c_int, [_i64, _i64, ctypes.c_uint64, ctypes.c_uint32, _vp, _vp, ctypes.c_size_t,
                                                 _vp]),
    "dgmi_random_subset_select_batch": (ctypes.c_int, [ctypes.c_int32, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_size_t, _vp]),
    "dgmi_random_subset_select_batch_dseed": (ctypes.c_int, [ctypes.c_int32, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_size_t, _vp]),
    "dgmi_keep_mask_f32": (ctypes.c_int, [_vp, ctypes.c_int32, _i64, _vp, _vp]),
    "dgmi_scale_rows_f32": (ctypes.c_int, [_vp, _i64, _vp, _i64, _i64, _vp, _i64, _vp]),
    "dgmi_weighted_colsum_f32": (ctypes.c_int, [_vp, _i64, _vp, _i64, _i64, _i64, ctypes.c_int32, _vp, _i64, _vp]),
    "dgmi_rank_add_f32": (ctypes.c_int, [_vp, _i64, _vp, _i64, _vp, _i64, _i64, _i64, ctypes.c_int32, _vp]),
    "dgmi_compact_layout_workspace_bytes": (ctypes.c_size_t, [_i64]),
    "dgmi_compact_layout_i32": (ctypes.c_int, [_vp, _i64, _vp, _vp, _vp, _i64, _vp, ctypes.c_int32, _vp, _vp, _vp, _vp,
                                               ctypes.c_size_t, _vp]),
    "dgmi_set_tuning": (ctypes.c_int, [ctypes.c_char_p, _i64]),
    "dgmi_row_multiplicity_f32": (ctypes.c_int, [_vp, _vp, _i64, _i64, ctypes.c_float, _vp, _vp, _vp, _vp]),
}


# name -> (restype, argtypes); mirrors include/dgmi_pairs.h (kept apart from SIGNATURES, which is dgmi.h one to one).
PAIR_SIGNATURES = {
    "dgmi_pair_topk_workspace_bytes": (ctypes.c_size_t, [_i64, _i64, ctypes.c_int32]),
    "dgmi_pair_mlp_topk_f32": (ctypes.c_int, [_vp, _i64, _i64, _vp, _i64, _i64, ctypes.c_int32, ctypes.c_int32, _vp, _vp, _vp,
                                              _vp, _vp, _vp, _i64, ctypes.c_int32, _vp, _vp, _vp, _vp, _vp, ctypes.c_size_t,
                                              _vp]),
}
PAIR_TOPK_MAX_K = 1024  # DGMI_PAIR_TOPK_MAX_K

# name -> (restype, argtypes); mirrors include/dgmi_rank.h (a third table: the two above are pinned one to one).
RANK_SIGNATURES = {
    "dgmi_row_topk_workspace_bytes": (ctypes.c_size_t, [_i64, _i64, ctypes.c_int32]),
    "dgmi_pair_mlp_row_topk_f32": (ctypes.c_int, [_vp, _i64, _i64, _vp, _i64, _i64, ctypes.c_int32, ctypes.c_int32, _vp, _vp,
                                                  _vp, _vp, _vp, _vp, _i64, ctypes.c_int32, _vp, _vp, _vp, _vp, _vp,
                                                  ctypes.c_size_t, _vp]),
}
ROW_TOPK_MAX_K = 128  # DGMI_ROW_TOPK_MAX_K

# name -> (restype, argtypes); mirrors include/dgmi_above.h (a fourth table, for the same reason).
ABOVE_SIGNATURES = {
    "dgmi_pair_emit_workspace_bytes": (ctypes.c_size_t, [_i64, _i64]),
    "dgmi_pair_mlp_emit_f32": (ctypes.c_int, [_vp, _i64, _i64, _vp, _i64, _i64, ctypes.c_int32, ctypes.c_int32, _vp, _vp, _vp,
                                              _vp, _vp, _vp, _i64, ctypes.c_float, _i64, _vp, _vp, _vp, _vp, _vp, _vp,
                                              ctypes.c_size_t, _vp]),
    "dgmi_pair_records_sort_workspace_bytes": (ctypes.c_size_t, [_i64]),
    "dgmi_pair_records_sort_f32": (ctypes.c_int, [_vp, _vp, _vp, _i64, _vp, ctypes.c_size_t, _vp]),
}
PAIR_EMIT_MAX_RECORDS = 1 << 24  # DGMI_PAIR_EMIT_MAX_RECORDS

# name -> (restype, argtypes); mirrors include/dgmi_bf16.h (a fifth table, for the same reason).
BF16_SIGNATURES = {
    "dgmi_rows_to_bf16": (ctypes.c_int, [_vp, _i64, _vp, _i64, _i64, _vp, _i64, _vp]),
    "dgmi_spmm_sliced_bf16": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, ctypes.c_int32, _vp, _i64, _vp, _vp, _i64, _i64, _i64, _i64,
                                             ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _vp, ctypes.c_size_t] + _EPI + [_vp]),
}


# name -> (restype, argtypes); mirrors include/dgmi_given.h (a sixth table, for the same reason).
GIVEN_SIGNATURES = {
    "dgmi_pair_rank_workspace_bytes": (ctypes.c_size_t, [_i64, _i64, _i64]),
    "dgmi_pair_mlp_score_list_f32": (ctypes.c_int, [_vp, _i64, _i64, _vp, _i64, _i64, ctypes.c_int32, ctypes.c_int32, _vp, _vp,
                                                    _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp]),
    "dgmi_pair_mlp_rank_list_f32": (ctypes.c_int, [_vp, _i64, _i64, _vp, _i64, _i64, ctypes.c_int32, ctypes.c_int32, _vp, _vp,
                                                   _vp, _vp, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp,
                                                   ctypes.c_size_t, _vp]),
}

# name -> (restype, argtypes); mirrors include/dgmi_curve.h (its own table, for the same reason).
CURVE_SIGNATURES = {
    "dgmi_curve_areas_workspace_bytes": (ctypes.c_size_t, [_i64, _i64]),
    "dgmi_curve_areas_f32": (ctypes.c_int, [_vp, _vp, _vp, _i64, _i64, ctypes.c_float, _vp, _vp, _vp, _vp, ctypes.c_size_t,
                                            _vp]),
}
CURVE_MAX_SEGMENTS = 1 << 24  # DGMI_CURVE_MAX_SEGMENTS

# name -> (restype, argtypes); mirrors include/dgmi_layout.h (a seventh table, for the same reason).
LAYOUT_SIGNATURES = {
    "dgmi_sliced_layout_slices": (ctypes.c_int32, [_i64, _i64, _i64, ctypes.c_int32]),
}

# name -> (restype, argtypes); mirrors include/dgmi_train.h (its own table, for the same reason).
_TRAIN_OPERANDS = [_vp, _i64, _i64, _vp, _i64, _i64, ctypes.c_int32, ctypes.c_int32, _vp, _vp, _vp, _vp, _vp, _vp, _i64,
                   ctypes.c_float, _vp]
TRAIN_SIGNATURES = {
    "dgmi_pair_mlp_train_workspace_bytes": (ctypes.c_size_t, [_i64]),
    "dgmi_pair_mlp_train_forward_f32": (ctypes.c_int, _TRAIN_OPERANDS + [_vp, _vp, _vp]),
    "dgmi_pair_mlp_train_backward_f32": (ctypes.c_int, _TRAIN_OPERANDS + [_vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp,
                                                                          ctypes.c_size_t, _vp]),
}

# name -> (restype, argtypes); mirrors include/dgmi_attn.h (its own table, for the same reason).
_ATTN_OPERANDS = [_vp, _i64, _vp, _i64, _i64, ctypes.c_int32, ctypes.c_int32, _vp, _vp, _vp, _vp]
ATTN_SIGNATURES = {
    "dgmi_attn_fuse_workspace_bytes": (ctypes.c_size_t, [_i64, ctypes.c_int32]),
    "dgmi_attn_fuse_forward_f32": (ctypes.c_int, _ATTN_OPERANDS + [_vp, _i64, _vp, _vp]),
    "dgmi_attn_fuse_backward_f32": (ctypes.c_int, _ATTN_OPERANDS + [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp,
                                                                     ctypes.c_size_t, _vp]),
}

# name -> (restype, argtypes); mirrors include/dgmi_scale.h (its own table, for the same reason).
SCALE_SIGNATURES = {
    "dgmi_spmm_owned_scaled_takes": (ctypes.c_int32, [_i64, _i64, _i64, _i64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]),
    "dgmi_spmm_owned_scaled_f32": (ctypes.c_int, [_vp, _vp, _vp, _i64, _vp, ctypes.c_int32, _vp, _vp, _i64, _i64, _i64, _i64,
                                                  ctypes.c_int32, ctypes.c_int32] + _EPI + [ctypes.POINTER(ctypes.c_int32), _vp]),
}
SCALE_CODE_SHIFT, SCALE_CODE_BITS = 17, 11  # DGMI_SCALE_CODE_SHIFT, DGMI_SCALE_CODE_BITS


class DgmiError(RuntimeError):
    """A non-zero dgmi_status came back from the C ABI."""


def _load() -> ctypes.CDLL:
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "dream_gnn_amd: %s is missing. Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C dream_gnn_amd/csrc` (hipcc --offload-arch=gfx950). There is no CPU fallback." % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in (list(SIGNATURES.items()) + list(PAIR_SIGNATURES.items()) + list(RANK_SIGNATURES.items())
                              + list(ABOVE_SIGNATURES.items()) + list(BF16_SIGNATURES.items())
                              + list(GIVEN_SIGNATURES.items()) + list(CURVE_SIGNATURES.items())
                              + list(LAYOUT_SIGNATURES.items()) + list(TRAIN_SIGNATURES.items())
                              + list(ATTN_SIGNATURES.items()) + list(SCALE_SIGNATURES.items())):
        fn = getattr(lib, name)  # AttributeError if the .so does not export what the eleven headers declare
        fn.restype = res
        fn.argtypes = args
    got = lib.dgmi_abi_version()
    if got != ABI_VERSION:
        raise ImportError("libdgmi.so ABI version %d != expected %d; rebuild" % (got, ABI_VERSION))
    return lib


lib = _load()


def _load_torch_ops():
    """Register the ``dreamgnn_mi`` operator library (csrc/dgmi_torch.cpp).  The product path calls the
    kernels through these ops; a missing library is an error, as for libdgmi.so."""
    if not os.path.exists(TORCH_LIB_PATH):
        raise ImportError(
            "dream_gnn_amd: %s is missing. Build it with `python -c 'import __graft_entry__ as g; g.build()'` or "
            "`make -C dream_gnn_amd/csrc`. There is no CPU fallback." % TORCH_LIB_PATH)
    torch.ops.load_library(TORCH_LIB_PATH)
    return torch.ops.dreamgnn_mi


torch_ops = _load_torch_ops()


def set_tuning(name: str, value: int) -> None:
    """Override one launch parameter of the library (``dgmi_set_tuning``; measurement tools and one test)."""
    check(lib.dgmi_set_tuning(name.encode(), int(value)), "dgmi_set_tuning(%s)" % name)


def sliced_layout_slices(n_dst: int, n_src: int, F: int, id_mult: bool = False) -> int:
    """Source slices of the layout a plain fp32 XCD-local product of this shape should be given
    (``dgmi_sliced_layout_slices``: 8 but for the measured class; host arithmetic, no launch)."""
    return int(lib.dgmi_sliced_layout_slices(int(n_dst), int(n_src), int(F), 1 if id_mult else 0))


def owned_scaled_takes(n_dst: int, n_src: int, F: int, ldx: int, n_slices: int, id_mult: bool, n_codes: int) -> bool:
    """Whether ``dgmi_spmm_owned_scaled_f32`` would run this product (host arithmetic, no launch)."""
    return bool(lib.dgmi_spmm_owned_scaled_takes(int(n_dst), int(n_src), int(F), int(ldx), int(n_slices), 1 if id_mult else 0,
                                                 int(n_codes)))


def spmm_owned_scaled(segptr, words, X, table, dst_scale, out, n_src: int, n_slices: int, id_mult: bool, epi) -> bool:
    """``out = diag(dst_scale) A diag(table[code]) X`` on the owned form's scaled kernel (include/dgmi_scale.h) with the
    coded id words ``words``, on the current stream of ``X``'s device.  The operands are what the caller has already
    checked: float32, 16-byte aligned rows, one device.  False: declined, nothing was launched."""
    act, slope, mask, mask_scale = epi
    taken = ctypes.c_int32(0)
    with torch.cuda.device(X.device):
        check(lib.dgmi_spmm_owned_scaled_f32(
            segptr.data_ptr(), words.data_ptr(), X.data_ptr(), X.stride(0), table.data_ptr(), table.numel(),
            None if dst_scale is None else dst_scale.data_ptr(), out.data_ptr(), out.stride(0), out.shape[0], int(n_src),
            X.shape[1], int(n_slices), 1 if id_mult else 0, int(act), float(slope), None if mask is None else mask.data_ptr(),
            0 if mask is None else mask.stride(0), float(mask_scale), ctypes.byref(taken),
            torch.cuda.current_stream(X.device).cuda_stream), "dgmi_spmm_owned_scaled_f32")
    return taken.value == 1


def check(status: int, what: str) -> None:
    if status != 0:
        raise DgmiError("%s failed: %s (status %d)" % (what, lib.dgmi_status_string(status).decode(), status))
