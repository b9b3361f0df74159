"""ctypes binding of ``libtvr.so`` (the C ABI declared in include/tvr.h).

The reference is Python, so its binding to a native engine is a ctypes stub
(INTEGRATION.md).  The compute entry points (clean forward, patch sweep, head
projection, logits) are called as torch.library operators ``torch.ops.tvr.*``
registered by ``_tvr_ops.so`` (csrc/torch_ops.cpp, over the same C ABI:
load_ops); handle lifetime, GEMM mode, traces and profiling stay on ctypes.
Loading fails loudly: there is no CPU fallback anywhere in the product path.
"""
from __future__ import annotations

import ctypes
import os
from pathlib import Path

LIB_NAME = "libtvr.so"
OPS_NAME = "_tvr_ops.so"
# TVR_LIB: another in-tree build of the engine (same-box A/B of two builds)
LIB_PATH = Path(os.environ["TVR_LIB"]).resolve() if os.environ.get("TVR_LIB") else Path(__file__).resolve().parent / LIB_NAME

# enum tvr_status
TVR_OK = 0
TVR_ERR_INVALID = -1
TVR_ERR_HIP = -2
TVR_ERR_NOMEM = -3
TVR_ERR_UNSUPPORTED = -4
TVR_ERR_RANGE = -5
TVR_ERR_INTERNAL = -6

# enum tvr_trace_hook
TRACE_RESID_PRE = 0
TRACE_Z = 1
TRACE_Q = 2  # blocks.{l}.attn.hook_q / hook_k / hook_v, before rotary
TRACE_K = 3
TRACE_V = 4

# enum tvr_site_kind
SITE_NONE = 0
SITE_REPLACE_HEAD_ALLPOS = 1
SITE_ADD_ATTN_OUT_LASTPOS = 2
SITE_SET_RESID_PRE_POS = 3
SITE_REPLACE_HEADSET_ALLPOS = 4  # tvr_patch_sweep_sets only
SITE_REPLACE_HEADSET_LASTPOS = 5
SITE_SET_RESID_PRE_VEC = 6  # hook_resid_pre[layer][0, pos] = vectors[vec] (either sweep)
SITE_ATTN_KNOCKOUT_LASTPOS = 7  # hook_attn_scores[0, head, -1, keys] = -inf (tvr_patch_sweep_knockout only)

c_f32p = ctypes.c_void_p
c_i32p = ctypes.c_void_p


class CLayerWeights(ctypes.Structure):
    _fields_ = [("w1", ctypes.c_void_p), ("b1", ctypes.c_void_p),
                ("w2", ctypes.c_void_p), ("b2", ctypes.c_void_p)]


class CExact16Layer(ctypes.Structure):
    _fields_ = [("w1", ctypes.c_void_p), ("w2", ctypes.c_void_p), ("g1", ctypes.c_void_p), ("g2", ctypes.c_void_p)]


class CSite(ctypes.Structure):
    _fields_ = [("seq", ctypes.c_int32), ("kind", ctypes.c_int32), ("layer", ctypes.c_int32),
                ("head", ctypes.c_int32), ("pos", ctypes.c_int32), ("src_seq", ctypes.c_int32),
                ("src_pos", ctypes.c_int32), ("vec", ctypes.c_int32), ("target", ctypes.c_int32)]


SITE_FIELDS = [f for f, _ in CSite._fields_]


class CHeadPatch(ctypes.Structure):
    _fields_ = [("layer", ctypes.c_int32), ("head", ctypes.c_int32), ("vec", ctypes.c_int32)]


class CHeadsetItem(ctypes.Structure):
    """Mirror of ``tvr_headset_item`` (include/tvr.h; tvr_headset_apply, the head-set test primitive)."""
    _fields_ = [("row0", ctypes.c_int32), ("n_rows", ctypes.c_int32), ("first_patch", ctypes.c_int32),
                ("n_patches", ctypes.c_int32)]


class CHeadsetPatch(ctypes.Structure):
    _fields_ = [("head", ctypes.c_int32), ("vec", ctypes.c_int32)]


ENTRY_FORCE_VALU = 1  # include/tvr.h TVR_ENTRY_FORCE_VALU (tvr_site_entry, the site-entry test primitive)


class CAttnSeq(ctypes.Structure):
    """Mirror of ``tvr_attn_seq`` (include/tvr.h; the kernels' SeqDesc)."""
    _fields_ = [("row0", ctypes.c_int32), ("n", ctypes.c_int32), ("p0", ctypes.c_int32),
                ("cache_row", ctypes.c_int32), ("q0", ctypes.c_int32), ("prefix_live", ctypes.c_int32)]


class CKnockoutItem(ctypes.Structure):
    """Mirror of ``tvr_knockout_item`` (include/tvr.h; tvr_attention_knockout, the knockout test primitive)."""
    _fields_ = [("seq", ctypes.c_int32), ("heads", ctypes.c_uint64), ("first_key", ctypes.c_int32),
                ("n_keys", ctypes.c_int32)]


ACT_X2F16_IL = 0x12  # include/tvr.h TVR_ACT_X2F16_IL


class CGemmArgs(ctypes.Structure):
    """Mirror of ``tvr_gemm_args`` (include/tvr.h; tvr_gemm_launch, the GEMM test primitive)."""
    _fields_ = ([(n, ctypes.c_int32) for n in (
        "fmt", "exact16", "epi", "form", "form_n", "form_tile", "slicing", "skinny",
        "M", "N", "K", "lda", "ldw", "ld0", "n_split", "ld1h",
        "ps1h", "raw_rows", "ld_raw", "mirror_rows", "ldr", "a2_col", "a_buf_rows", "out_buf_rows")] +
                [("w_scale", ctypes.c_float), ("reserved", ctypes.c_int32), ("wps", ctypes.c_uint64)] +
                [(n, ctypes.c_void_p) for n in (
                    "A", "a2", "W", "bias", "out0", "out0m", "out1h", "raw", "resid", "range_flag",
                    "a_rows", "out_rows")])


class CLnpreArgs(ctypes.Structure):
    """Mirror of ``tvr_lnpre_args`` (include/tvr.h; tvr_lnpre_rows, the LayerNormPre test primitive)."""
    _fields_ = ([(n, ctypes.c_int32) for n in ("fmt", "rows", "d", "ldx", "ldy", "x_rows", "copy_rows")] +
                [("eps", ctypes.c_float)] +
                [(n, ctypes.c_void_p) for n in ("x", "row_idx", "y", "stats", "copy", "g1", "g2", "y2")])


# include/tvr.h enum tvr_gemm_epi / tvr_gemm_form / tvr_gemm_slicing
EPI_BIAS, EPI_GELU, EPI_RESID = 0, 1, 2
FORM_PLAN, FORM_PLAIN, FORM_SPLITK, FORM_TAIL, FORM_STREAMK = 0, 1, 2, 3, 4
SLICE_MODEL, SLICE_ON, SLICE_OFF = 0, 1, 2
# include/tvr.h tvr_model_weight_layout: the exact-fp16 GEMMs read engine-owned row-pair-interleaved copies
W_IL_LAYERS, W_IL_UNEMBED, W_IL_NOMEM = 1, 2, 4


class CKernelStats(ctypes.Structure):
    _fields_ = [("gemm_launches", ctypes.c_int64 * 3), ("gemm_flops", ctypes.c_double * 3),
                ("gemm_ms", ctypes.c_double * 3), ("gemm_bytes", ctypes.c_double * 3)]


GEMM_VARIANTS = ("unembed", "qkv_mlpin", "o_mlpout")


class CHbmStats(ctypes.Structure):
    _fields_ = [("launches", ctypes.c_int64 * 6), ("ms", ctypes.c_double * 6), ("bytes", ctypes.c_double * 6)]


# include/tvr.h enum tvr_hbm_kind
HBM_KINDS = ("entry", "capture", "lnpre", "attention", "row_stats", "lin_entry")

# name -> (restype, argtypes); every symbol include/tvr.h declares.
ABI_VERSION = 11  # include/tvr.h TVR_ABI_VERSION

# include/tvr.h enum tvr_gemm_mode
GEMM_MODES = {"f32": 0, "x3bf16": 1, "x2f16": 2, "bf16": 3}
GEMM_NAMES = {v: k for k, v in GEMM_MODES.items()}

SIGNATURES = {
    "tvr_version": (ctypes.c_char_p, []),
    "tvr_abi_version": (ctypes.c_int32, []),
    "tvr_last_error": (ctypes.c_char_p, []),
    "tvr_model_create": (ctypes.c_int, [ctypes.c_void_p, c_f32p, ctypes.POINTER(CLayerWeights),
                                        c_f32p, c_f32p, ctypes.POINTER(ctypes.c_void_p)]),
    "tvr_model_destroy": (ctypes.c_int, [ctypes.c_void_p]),
    "tvr_trace_create": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32,
                                        ctypes.POINTER(ctypes.c_void_p)]),
    "tvr_trace_destroy": (ctypes.c_int, [ctypes.c_void_p]),
    "tvr_trace_flush": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "tvr_trace_read": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, c_f32p,
                                      ctypes.c_void_p]),
    "tvr_trace_num_tokens": (ctypes.c_int32, [ctypes.c_void_p]),
    "tvr_trace_capture_resid": (ctypes.c_int, [ctypes.c_void_p, c_i32p, c_i32p, ctypes.c_int32, c_f32p,
                                               ctypes.c_void_p]),
    "tvr_forward_clean": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, c_i32p, c_i32p, ctypes.c_int32,
                                         c_i32p, c_f32p, c_i32p, ctypes.c_int32, c_f32p, c_f32p,
                                         ctypes.c_void_p]),
    "tvr_forward_clean_deferred": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, c_i32p, c_i32p, ctypes.c_int32,
                                                  c_i32p, c_f32p, c_i32p, ctypes.c_int32, ctypes.c_void_p]),
    "tvr_forward_logits": (ctypes.c_int, [ctypes.c_void_p, c_i32p, c_f32p, ctypes.c_int32, c_i32p, ctypes.c_int32,
                                          c_f32p, ctypes.c_void_p]),
    "tvr_patch_sweep": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32,
                                       c_f32p, ctypes.c_int32, c_f32p, c_i32p, ctypes.c_int32, c_f32p,
                                       ctypes.c_void_p]),
    "tvr_patch_sweep_sets": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32,
                                            c_i32p, ctypes.c_void_p, c_f32p, ctypes.c_int32, c_f32p, c_i32p,
                                            ctypes.c_int32, c_f32p, ctypes.c_void_p]),
    "tvr_patch_sweep_knockout": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32,
                                                c_i32p, ctypes.c_void_p, c_i32p, c_i32p, c_f32p, ctypes.c_int32,
                                                c_f32p, c_i32p, ctypes.c_int32, c_f32p, ctypes.c_void_p]),
    "tvr_attention_knockout": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, c_f32p, c_f32p, ctypes.c_void_p,
                                              ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p,
                                              ctypes.c_int32, c_i32p, ctypes.c_int32, ctypes.c_void_p, c_f32p, c_f32p,
                                              ctypes.c_void_p]),
    "tvr_project_heads": (ctypes.c_int, [ctypes.c_void_p, c_f32p, c_f32p, ctypes.c_void_p]),
    "tvr_gemm_f32": (ctypes.c_int, [c_f32p, ctypes.c_int32, c_f32p, ctypes.c_int32, c_f32p, c_f32p,
                                    ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                    ctypes.c_void_p]),
    "tvr_lnpre_f32": (ctypes.c_int, [c_f32p, ctypes.c_int32, c_f32p, ctypes.c_int32, ctypes.c_int32,
                                     ctypes.c_int32, ctypes.c_float, ctypes.c_void_p]),
    "tvr_lnpre_rows": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(CLnpreArgs), ctypes.c_void_p]),
    "tvr_center_rows": (ctypes.c_int, [c_f32p, c_f32p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p]),
    "tvr_workspace_bytes":(ctypes.c_size_t, [ctypes.c_void_p]),
    "tvr_model_set_gemm": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]),
    "tvr_model_set_exact16": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "tvr_model_set_exact16_unembed": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "tvr_model_get_gemm": (ctypes.c_int32, [ctypes.c_void_p]),
    "tvr_model_weight_layout": (ctypes.c_int32, [ctypes.c_void_p]),
    "tvr_weight_rows_il": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32,
                                          ctypes.c_void_p]),
    "tvr_split_planes": (ctypes.c_int, [c_f32p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "tvr_gemm_x3bf16": (ctypes.c_int, [c_f32p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32,
                                       ctypes.c_size_t, c_f32p, c_f32p, ctypes.c_int32, ctypes.c_int32,
                                       ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p]),
    "tvr_model_range_status": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "tvr_weight_planes": (ctypes.c_int, [ctypes.c_int32, c_f32p, ctypes.c_float, ctypes.c_void_p, ctypes.c_size_t,
                                         ctypes.c_void_p]),
    "tvr_gemm_x2f16": (ctypes.c_int, [c_f32p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32,
                                      ctypes.c_size_t, ctypes.c_float, c_f32p, c_f32p, ctypes.c_int32,
                                      ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p,
                                      ctypes.c_void_p]),
    "tvr_act_rows": (ctypes.c_int, [ctypes.c_int32, c_f32p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32,
                                    ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]),
    "tvr_gemm_planar": (ctypes.c_int, [ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p,
                                       ctypes.c_int32, ctypes.c_size_t, ctypes.c_float, c_f32p, c_f32p,
                                       ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                       ctypes.c_void_p]),
    "tvr_profile_enable": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32]),
    "tvr_profile_read": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(CKernelStats)]),
    "tvr_profile_read_hbm": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(CHbmStats)]),
    "tvr_gemm_plan": (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                     ctypes.c_void_p]),
    "tvr_attention": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, c_f32p, c_f32p, ctypes.c_void_p, ctypes.c_int32,
                                     ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, c_f32p,
                                     ctypes.c_int32, ctypes.c_int32, c_f32p, c_f32p, ctypes.c_void_p]),
    "tvr_attention_pattern": (ctypes.c_int, [ctypes.c_void_p, c_f32p, ctypes.c_int32, c_i32p, c_i32p, ctypes.c_int32,
                                             c_i32p, ctypes.c_int32, c_f32p, ctypes.c_int32, c_f32p, c_f32p, c_f32p,
                                             ctypes.c_void_p]),
    "tvr_trace_capture_pattern": (ctypes.c_int, [ctypes.c_void_p, c_i32p, c_i32p, ctypes.c_int32, c_f32p,
                                                 ctypes.c_int32, c_f32p, ctypes.c_void_p]),
    "tvr_gemm_launch": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(CGemmArgs), ctypes.c_void_p]),
    "tvr_head_attribution": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, c_f32p, c_f32p, ctypes.c_int32, c_f32p,
                                            ctypes.c_void_p]),
    "tvr_trace_logit_attribution": (ctypes.c_int, [ctypes.c_void_p, c_i32p, c_i32p, c_i32p, c_f32p, c_f32p,
                                                   ctypes.c_void_p]),
    "tvr_decode_rows": (ctypes.c_int, [ctypes.c_void_p, c_f32p, ctypes.c_int32, c_i32p, c_f32p, c_i32p,
                                       ctypes.c_int32, ctypes.c_void_p]),
    "tvr_trace_logit_lens": (ctypes.c_int, [ctypes.c_void_p, c_i32p, c_i32p, c_f32p, c_i32p, ctypes.c_int32,
                                            ctypes.c_void_p]),
    "tvr_head_directions": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, c_f32p, ctypes.c_int32, c_f32p,
                                           ctypes.c_void_p]),
    "tvr_attention_source": (ctypes.c_int, [ctypes.c_void_p, c_f32p, ctypes.c_int32, c_i32p, c_i32p, ctypes.c_int32,
                                            c_f32p, c_i32p, ctypes.c_int32, c_f32p, ctypes.c_int32, c_f32p, c_f32p,
                                            c_f32p, ctypes.c_void_p]),
    "tvr_trace_source_attribution": (ctypes.c_int, [ctypes.c_void_p, c_i32p, c_i32p, c_i32p, c_i32p, ctypes.c_int32,
                                                    c_f32p, ctypes.c_int32, c_f32p, ctypes.c_void_p]),
    "tvr_site_entry": (ctypes.c_int, [ctypes.c_void_p, c_i32p, ctypes.c_int32, c_i32p, ctypes.c_int32, c_f32p, c_f32p,
                                      ctypes.c_void_p, ctypes.c_int32, c_i32p, ctypes.c_void_p, c_f32p,
                                      ctypes.c_int32, ctypes.c_int32, c_f32p, ctypes.c_int32, c_i32p, c_i32p, c_i32p,
                                      ctypes.c_void_p]),
    "tvr_headset_apply": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32,
                                         ctypes.c_void_p, ctypes.c_int32, c_f32p, ctypes.c_int32, ctypes.c_void_p,
                                         c_f32p, ctypes.c_int32, ctypes.c_void_p]),
}

OPS_PATH = LIB_PATH.parent / OPS_NAME
# the torch.library operators _tvr_ops.so registers (csrc/torch_ops.cpp)
OPS = ("forward_clean", "patch_sweep", "project_heads", "forward_logits")
# the joint head-set sweep (tvr_patch_sweep_sets), registered by the same extension
SET_OPS = ("patch_sweep_sets",)
# the attention-knockout sweep and its kernel alone (tvr_patch_sweep_knockout, tvr_attention_knockout)
KNOCKOUT_OPS = ("patch_sweep_knockout", "attention_knockout")
# the grouped residual capture (tvr_trace_capture_resid), registered by the same extension
RESID_OPS = ("capture_resid",)
# one query's attention pattern / per-class attention mass per traced sequence (tvr_trace_capture_pattern)
PATTERN_OPS = ("capture_pattern",)
# tvr_trace_capture_pattern's upper limit on n_classes (include/tvr.h)
PATTERN_MAX_CLASSES = 64
# direct logit attribution and the logit lens / vocabulary decoding (tvr_head_attribution,
# tvr_trace_logit_attribution, tvr_trace_logit_lens, tvr_decode_rows)
ATTRIBUTION_OPS = ("head_attribution", "logit_attribution", "logit_lens", "decode_rows")
# per-source-token logit attribution (tvr_head_directions, tvr_attention_source, tvr_trace_source_attribution)
SOURCE_OPS = ("head_directions", "attention_source", "source_attribution")
# the largest top-k of the row statistics (csrc/kernels.hpp STATS_MAX_K)
STATS_MAX_K = 16

_LIB = None
_OPS_LOADED = False


class EngineError(RuntimeError):
    pass


class RangeError(EngineError):
    """TVR_ERR_RANGE: an x2f16 GEMM input left the fp16 split's range (the
    results since the last check are not fp32-accurate).  The experiment
    functions retry on a path without that limit (``Model.range_fallback``)."""


def load(path: os.PathLike | str | None = None) -> ctypes.CDLL:
    """Load libtvr.so (cached).  Raises if it is missing: build it with
    ``python __graft_entry__.py`` or ``make -C task-vector-replication_amd/csrc``."""
    global _LIB
    if _LIB is not None and path is None:
        return _LIB
    p = Path(path) if path else LIB_PATH
    if not p.exists():
        raise EngineError(f"{p} not found: the HIP engine is not built (no CPU fallback exists); "
                          "run `make -C task-vector-replication_amd/csrc`")
    lib = ctypes.CDLL(str(p))
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.tvr_abi_version() != ABI_VERSION:
        raise EngineError("libtvr ABI mismatch")
    if path is None:
        _LIB = lib
    return lib


def load_ops():
    """Register the ``torch.ops.tvr`` operators (once; after libtvr.so, which
    they link from their own directory).  Raises if the extension is missing."""
    global _OPS_LOADED
    import torch
    load()
    if not _OPS_LOADED:
        if not OPS_PATH.exists():
            raise EngineError(f"{OPS_PATH} not found: the torch operator extension is not built (no CPU fallback "
                              "exists); run `make -C task-vector-replication_amd/csrc`")
        torch.ops.load_library(str(OPS_PATH))
        _OPS_LOADED = True
    return torch.ops.tvr


def check(rc: int, what: str) -> None:
    """Status code → exception, with the reference's error types: invalid
    shapes raise ValueError (scratch2.py:172-175), the rest RuntimeError."""
    if rc == TVR_OK:
        return
    msg = (load().tvr_last_error() or b"").decode(errors="replace")
    if rc == TVR_ERR_INVALID:
        raise ValueError(f"{what}: {msg}")
    if rc == TVR_ERR_RANGE:
        raise RangeError(f"{what} failed ({rc}): {msg}")
    raise EngineError(f"{what} failed ({rc}): {msg}")


def ptr(t) -> int:
    """Device pointer of a torch tensor (None → NULL)."""
    return 0 if t is None else t.data_ptr()
