"""ctypes binding of ``liballophant_amx.so`` (C ABI declared in ``include/allophant_amx.h``).

There is deliberately no fallback: if the HIP library has not been built (``python -c 'import __graft_entry__ as g;
g.build()'`` or ``make -C allophant_amd/csrc``) every compute entry point raises ``RuntimeError``.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

# AMX_ABI_OVERRIDE: developer switch for same-box A/B runs against a library built from an OLDER revision (tools/ab_build.sh):
# ABI 5 and 6 added flags and entry points to ABI 4 without changing a struct, and ABI 7 split the last 32-bit member of amx_config
# into use_attention_mask and adapter_attn_dim, 16 bits each (an older build reads the pair as the mask while the dimension is 0:
# models without attention adapters only), so an older build runs under this binding
AMX_ABI_VERSION = int(os.environ.get("AMX_ABI_OVERRIDE") or 7)
AMX_MAX_CONV = 8
AMX_MAX_DEPS = 64
AMX_NAME_LEN = 48

AMX_OK, AMX_EINVAL, AMX_EHIP, AMX_ESTATE, AMX_ENOMEM, AMX_ERANGE = 0, -1, -2, -3, -4, -5
PRECISIONS = {"bf16": 0, "f16": 1, "bf16x3": 2, "f16x3": 3}
FLAG_HOST_IO, FLAG_RAW_LOGITS, FLAG_KEEP_HIDDEN, FLAG_TIMING, FLAG_PADDED, FLAG_NO_PACK, FLAG_CONTINUE = 1, 2, 4, 8, 16, 32, 64
FLAG_NO_GRAPH, FLAG_NO_RANGE_CHECK = 128, 256
NORM_LAYER, NORM_GROUP = 0, 1
PASS_INFO = ["ln_fold", "packed", "graph", "rows", "id", "attention", "conv0"]  # AMX_PASS_INFO_*
CONV0_STATS = ["none", "table", "covariance", "recompute8", "recompute"]  # AMX_PASS_INFO_CONV0's statistics digit
KERNEL_CLASSES = ["gemm_pp", "gemm_tile", "attention", "rownorm", "conv0", "other", "gemm_ln", "conv_tail"]
DEP_OUTPUT = -1

LIB_NAME = "liballophant_amx.so"
# AMX_LIB_PATH: developer switch (A/B builds of the library side by side); the default is the in-tree build
LIB_PATH = os.environ.get("AMX_LIB_PATH") or os.path.join(os.path.dirname(os.path.abspath(__file__)), LIB_NAME)

# every symbol include/allophant_amx.h declares
EXPORTS = [
    "amx_create", "amx_destroy", "amx_last_error", "amx_set_inventory", "amx_output_layout", "amx_forward",
    "amx_synchronize", "amx_greedy_ctc", "amx_debug_fetch", "amx_device_bytes", "amx_timing_fetch",
    "amx_max_utterances", "amx_greedy_ctc_emissions", "amx_check_finite", "amx_gather_outputs", "amx_dist_last_error",
    "amx_graph_info", "amx_pass_info", "amx_debug_scribble",
]
# the allophone-layer entry points (include/allophant_amx_allophones.h; added to ABI 6, detected by name)
ALLOPHONE_EXPORTS = ["amx_set_allophones", "amx_map_allophones"]
# the CTC beam-search entry points (include/allophant_amx_beam.h; added to ABI 6, detected by name)
BEAM_EXPORTS = ["amx_beam_ctc_workspace", "amx_beam_ctc", "amx_beam_ctc_emissions"]
BEAM_EXP_EMISSIONS = 1  # AMX_BEAM_EXP_EMISSIONS
BEAM_MAX_WIDTH = 64
# the same search with a phonotactic language model (include/allophant_amx_beam_lm.h; added to ABI 7, detected by name)
BEAM_LM_EXPORTS = ["amx_beam_ctc_lm_workspace", "amx_beam_ctc_lm_emissions"]
BEAM_LM_MAX_CLASSES = 4095  # AMX_BEAM_LM_MAX_CLASSES
# the sinc-resampling entry points (include/allophant_amx_resample.h; added to ABI 6, detected by name)
RESAMPLE_EXPORTS = ["amx_resample_bank", "amx_resample"]
RESAMPLE_MAX_PHASES = 4096  # AMX_RESAMPLE_MAX_PHASES
RESAMPLE_MAX_WINDOW = 16384  # AMX_RESAMPLE_MAX_WINDOW
# the edit-statistics entry points (include/allophant_amx_edit.h; added to ABI 6, detected by name)
EDIT_EXPORTS = ["amx_edit_workspace", "amx_edit_statistics", "amx_edit_operations_workspace", "amx_edit_operations"]
EDIT_WEIGHTED_EXPORTS = ["amx_edit_cost_table_bytes", "amx_edit_cost_table", "amx_edit_weighted_statistics",
                         "amx_edit_weighted_operations", "amx_edit_matrix"]
EDIT_CONFUSION_EXPORTS = ["amx_edit_confusion_table_bytes", "amx_edit_confusions", "amx_edit_weighted_confusions",
                          "amx_edit_confusion_merge"]  # (added to ABI 7, detected by name)
EDIT_CONFUSION_GROUP_BITS, EDIT_CONFUSION_SYMBOL_BITS = 22, 21  # AMX_EDIT_CONFUSION_GROUP_BITS / _SYMBOL_BITS
EDIT_MAX_LENGTH = 65535  # AMX_EDIT_MAX_LENGTH
EDIT_MAX_SYMBOLS = 8192  # AMX_EDIT_MAX_SYMBOLS
EDIT_MAX_FEATURES = 255  # AMX_EDIT_MAX_FEATURES
EDIT_MAX_CANDIDATES = 64  # AMX_EDIT_MAX_CANDIDATES
# the CTC forced-alignment entry points (include/allophant_amx_align.h; added to ABI 6, detected by name)
ALIGN_EXPORTS = ["amx_ctc_align_workspace", "amx_ctc_align_emissions", "amx_ctc_align"]
ALIGN_MAX_TARGET = 4095  # AMX_ALIGN_MAX_TARGET
# the same contract for whole transcripts (the same header; added to ABI 6, detected by name)
ALIGN_LONG_EXPORTS = ["amx_ctc_align_long_workspace", "amx_ctc_align_long_emissions", "amx_ctc_align_long"]
ALIGN_LONG_MAX_TARGET = 262143  # AMX_ALIGN_LONG_MAX_TARGET
ALIGN_LONG_FRAME_BLOCK = 64  # AMX_ALIGN_LONG_FRAME_BLOCK
ALIGN_LONG_TILE_STATES = 832  # AMX_ALIGN_LONG_TILE_STATES
# the alignment over pronunciation graphs (include/allophant_amx_align_graph.h; added to ABI 7, detected by name)
ALIGN_GRAPH_EXPORTS = ["amx_ctc_align_graph_workspace", "amx_ctc_align_graph_emissions", "amx_ctc_align_graph"]
ALIGN_GRAPH_MAX_NODES = 4095  # AMX_ALIGN_GRAPH_MAX_NODES
ALIGN_GRAPH_MAX_IN = 6  # AMX_ALIGN_GRAPH_MAX_IN
# the CTC forward-backward scoring entry points (include/allophant_amx_score.h; added to ABI 6, detected by name)
SCORE_EXPORTS = ["amx_ctc_score_workspace", "amx_ctc_score_emissions", "amx_ctc_score"]
SCORE_MAX_TARGET = 4095  # AMX_SCORE_MAX_TARGET
# the CTC one-edit-variant entry points (include/allophant_amx_variants.h; added to ABI 7, detected by name)
VARIANTS_EXPORTS = ["amx_ctc_variants_workspace", "amx_ctc_variants_emissions"]
VARIANTS_MAX_TARGET = 4095  # AMX_VARIANTS_MAX_TARGET
VARIANTS_MAX_CLASSES = 65535  # AMX_VARIANTS_MAX_CLASSES
# the CTC search entry points (include/allophant_amx_search.h; added to ABI 6, detected by name)
SEARCH_EXPORTS = ["amx_ctc_search_workspace", "amx_ctc_search_emissions"]
SEARCH_MAX_QUERY = 256  # AMX_SEARCH_MAX_QUERY
# the inventory-restriction entry point (include/allophant_amx_restrict.h; added to ABI 6, detected by name)
RESTRICT_EXPORTS = ["amx_restrict_outputs"]
RESTRICT_NORMALIZE = 1  # AMX_RESTRICT_NORMALIZE
RESTRICT_MAX_CLASSES = 65535  # AMX_RESTRICT_MAX_CLASSES
# the long-recording entry points (include/allophant_amx_long.h; added to ABI 6, detected by name)
LONG_EXPORTS = ["amx_long_plan", "amx_long_gather", "amx_long_stitch"]
LONG_MAX_BLOCKS = 64  # AMX_LONG_MAX_BLOCKS
# amx_long_window: six int32 fields, held by the binding as an int32 [W, 6] array in this order
LONG_WINDOW_FIELDS = ("recording", "index", "start", "keep_lo", "keep_hi", "samples")


def dep_output_layer(i: int) -> int:
    return -2 - i


class AmxConfig(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32), ("n_conv", C.c_int32), ("conv_dim", C.c_int32),
        ("conv_kernel", C.c_int32 * AMX_MAX_CONV), ("conv_stride", C.c_int32 * AMX_MAX_CONV),
        ("hidden", C.c_int32), ("layers", C.c_int32), ("heads", C.c_int32), ("ffn", C.c_int32),
        ("pos_kernel", C.c_int32), ("pos_groups", C.c_int32), ("eps", C.c_float), ("do_normalize", C.c_int32),
        ("dependency_blanks", C.c_int32), ("embedding_size", C.c_int32), ("allophone_layer", C.c_int32),
        ("precision", C.c_int32), ("feat_extract_norm", C.c_int32), ("conv_bias", C.c_int32),
        ("stable_layer_norm", C.c_int32), ("use_attention_mask", C.c_int16), ("adapter_attn_dim", C.c_int16),
    ]


class AmxClassDesc(C.Structure):
    _fields_ = [
        ("name", C.c_char * AMX_NAME_LEN), ("size", C.c_int32), ("out_features", C.c_int32), ("n_deps", C.c_int32),
        ("deps", C.c_int32 * AMX_MAX_DEPS), ("time_heads", C.c_int32), ("time_positional", C.c_int32),
    ]


class AmxTensor(C.Structure):
    _fields_ = [("name", C.c_char_p), ("data", C.POINTER(C.c_float)), ("numel", C.c_int64)]


class AmxOutputDesc(C.Structure):
    _fields_ = [("name", C.c_char * AMX_NAME_LEN), ("classes", C.c_int32), ("offset", C.c_int64)]


class AmxLongBlock(C.Structure):
    _fields_ = [("src_offset", C.c_int64), ("dst_offset", C.c_int64), ("classes", C.c_int32)]


class AmxResampleGeometry(C.Structure):
    _fields_ = [(f, C.c_int64) for f in ("o", "m", "width", "taps", "bank_size", "window")]


# amx_resample_row: six int64 fields, built by the binding as an int64 [N, 6] tensor in this order
RESAMPLE_ROW_FIELDS = ("o", "m", "width", "taps", "bank_offset", "phase_offset")


_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """Loads the shared library and declares the prototypes; raises if it is missing (no CPU fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: build the HIP extension first (make -C allophant_amd/csrc, or "
            "__graft_entry__.build()). allophant_amd has no CPU fallback."
        )
    lib = C.CDLL(LIB_PATH)
    vp, i32, i64 = C.c_void_p, C.c_int, C.c_int64
    lib.amx_create.argtypes = [C.POINTER(vp), i32, C.POINTER(AmxConfig), C.POINTER(AmxClassDesc), i32,
                               C.POINTER(AmxTensor), i32]
    lib.amx_create.restype = i32
    lib.amx_destroy.argtypes = [vp]
    lib.amx_destroy.restype = i32
    lib.amx_last_error.argtypes = [vp]
    lib.amx_last_error.restype = C.c_char_p
    lib.amx_set_inventory.argtypes = [vp, C.POINTER(i64), i32, i32, C.POINTER(i64), vp]
    lib.amx_set_inventory.restype = i32
    lib.amx_output_layout.argtypes = [vp, i32, i64, C.POINTER(AmxOutputDesc), C.POINTER(i32), C.POINTER(i64),
                                      C.POINTER(i64)]
    lib.amx_output_layout.restype = i32
    lib.amx_forward.argtypes = [vp, vp, C.POINTER(i64), i32, i64, vp, C.POINTER(i64), C.c_uint32, vp]
    lib.amx_forward.restype = i32
    lib.amx_synchronize.argtypes = [vp, vp]
    lib.amx_synchronize.restype = i32
    if hasattr(lib, "amx_graph_info") or AMX_ABI_VERSION >= 5:  # (absent from an ABI-4 build under AMX_ABI_OVERRIDE)
        lib.amx_graph_info.argtypes = [vp, C.POINTER(i64), C.POINTER(i64)]
        lib.amx_graph_info.restype = i32
    if hasattr(lib, "amx_pass_info") or AMX_ABI_VERSION >= 6:  # (absent from older builds under AMX_ABI_OVERRIDE)
        lib.amx_pass_info.argtypes = [vp, C.POINTER(C.c_int32), i32]
        lib.amx_pass_info.restype = i32
    if hasattr(lib, "amx_debug_scribble"):  # (added to ABI 7 by name: absent from older builds)
        lib.amx_debug_scribble.argtypes = [vp, C.c_uint32, vp]
        lib.amx_debug_scribble.restype = i32
    if hasattr(lib, "amx_map_allophones"):  # (absent from older builds under AMX_ABI_OVERRIDE)
        lib.amx_set_allophones.argtypes = [vp, i32, i32, i32, C.POINTER(C.c_float), C.POINTER(C.c_uint8)]
        lib.amx_set_allophones.restype = i32
        lib.amx_map_allophones.argtypes = [vp, vp, i64, i64, vp, i32, i64, vp, vp]
        lib.amx_map_allophones.restype = i32
    if hasattr(lib, "amx_beam_ctc"):  # (absent from older builds under AMX_ABI_OVERRIDE)
        lib.amx_beam_ctc_workspace.argtypes = [i32, i64, i64, C.POINTER(C.c_size_t)]
        lib.amx_beam_ctc_workspace.restype = i32
        lib.amx_beam_ctc.argtypes = [vp, vp, C.POINTER(i64), i32, i64, i32, i32, C.c_uint32, vp, C.c_size_t, vp, vp, vp, vp, vp, vp]
        lib.amx_beam_ctc.restype = i32
        lib.amx_beam_ctc_emissions.argtypes = [i32, vp, i64, i64, vp, i32, i64, i32, i32, i32, i32, C.c_uint32, vp, C.c_size_t,
                                               vp, vp, vp, vp, vp, vp]
        lib.amx_beam_ctc_emissions.restype = i32
    if hasattr(lib, "amx_beam_ctc_lm_emissions"):  # (added to ABI 7 by name: absent from older builds)
        lib.amx_beam_ctc_lm_workspace.argtypes = [i32, i64, i64, C.POINTER(C.c_size_t)]
        lib.amx_beam_ctc_lm_workspace.restype = i32
        lib.amx_beam_ctc_lm_emissions.argtypes = [i32, vp, i64, i64, vp, i32, i64, i32, i32, i32, i32, C.c_uint32, vp, i32, vp,
                                                  C.c_double, C.c_double, vp, C.c_size_t, vp, vp, vp, vp, vp, vp]
        lib.amx_beam_ctc_lm_emissions.restype = i32
    if hasattr(lib, "amx_resample"):  # (absent from older builds under AMX_ABI_OVERRIDE)
        lib.amx_resample_bank.argtypes = [i64, i64, C.c_int32, C.c_double, C.POINTER(AmxResampleGeometry), vp, vp]
        lib.amx_resample_bank.restype = i32
        lib.amx_resample.argtypes = [i32, vp, i64, i64, vp, vp, vp, vp, i64, i32, i64, vp, vp]
        lib.amx_resample.restype = i32
    # device to workspace_bytes: what the statistics and confusion entries begin with, uniform and weighted
    edit_head = [i32, vp, i64, i64, i64, i32, i32, i32, i64, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, i32, i64, i64, vp, C.c_size_t]
    if hasattr(lib, "amx_edit_statistics"):  # (absent from older builds under AMX_ABI_OVERRIDE)
        lib.amx_edit_workspace.argtypes = [i64, i64, i64, C.POINTER(C.c_size_t)]
        lib.amx_edit_workspace.restype = i32
        lib.amx_edit_statistics.argtypes = edit_head + [vp, vp, vp, vp]
        lib.amx_edit_statistics.restype = i32
    if hasattr(lib, "amx_edit_operations"):
        lib.amx_edit_operations_workspace.argtypes = [i64, i64, i64, C.POINTER(C.c_size_t)]
        lib.amx_edit_operations_workspace.restype = i32
        lib.amx_edit_operations.argtypes = [i32, vp, i64, i64, i32, i32, i64, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, i32, i64,
                                            i64, vp, C.c_size_t, i64, vp, vp, vp]
        lib.amx_edit_operations.restype = i32
    if hasattr(lib, "amx_edit_weighted_statistics"):
        f32 = C.c_float
        lib.amx_edit_cost_table_bytes.argtypes = [i64, C.POINTER(C.c_size_t)]
        lib.amx_edit_cost_table_bytes.restype = i32
        lib.amx_edit_cost_table.argtypes = [i32, vp, i64, i64, vp, vp]
        lib.amx_edit_cost_table.restype = i32
        lib.amx_edit_weighted_statistics.argtypes = edit_head + [f32, f32, vp, vp, vp, vp, vp, vp, vp]
        lib.amx_edit_weighted_statistics.restype = i32
        lib.amx_edit_weighted_operations.argtypes = [i32, vp, i64, i64, i32, i32, i64, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp,
                                                     i32, i64, i64, vp, C.c_size_t, f32, f32, vp, vp, i64, vp, vp, vp, vp]
        lib.amx_edit_weighted_operations.restype = i32
        lib.amx_edit_matrix.argtypes = [i32, vp, vp, vp, vp, i64, i64, i64, f32, f32, vp, i64, vp, C.c_size_t, vp, vp, vp]
        lib.amx_edit_matrix.restype = i32
    if hasattr(lib, "amx_edit_confusions"):  # (added to ABI 7 by name: absent from older builds)
        tail = [vp, vp, i64, vp, vp, vp]  # best, table, capacity, row_events, counters, stream
        lib.amx_edit_confusion_table_bytes.argtypes = [i64, C.POINTER(C.c_size_t)]
        lib.amx_edit_confusion_table_bytes.restype = i32
        lib.amx_edit_confusions.argtypes = edit_head + tail
        lib.amx_edit_confusions.restype = i32
        lib.amx_edit_weighted_confusions.argtypes = edit_head + [C.c_float, C.c_float, vp, vp] + tail
        lib.amx_edit_weighted_confusions.restype = i32
        lib.amx_edit_confusion_merge.argtypes = [i32, vp, i64, vp, i64, vp, vp]
        lib.amx_edit_confusion_merge.restype = i32
    if hasattr(lib, "amx_ctc_align"):  # (absent from older builds under AMX_ABI_OVERRIDE)
        lib.amx_ctc_align_workspace.argtypes = [i64, i64, i64, C.POINTER(C.c_size_t)]
        lib.amx_ctc_align_workspace.restype = i32
        lib.amx_ctc_align_emissions.argtypes = [i32, vp, i64, i64, vp, i32, i64, i32, i32, vp, vp, i64, vp, C.c_size_t, vp, vp, vp,
                                                vp, vp, vp, vp]
        lib.amx_ctc_align_emissions.restype = i32
        lib.amx_ctc_align.argtypes = [vp, vp, C.POINTER(i64), i32, i64, vp, vp, i64, vp, C.c_size_t, vp, vp, vp, vp, vp, vp, vp]
        lib.amx_ctc_align.restype = i32
    if hasattr(lib, "amx_ctc_align_long"):  # (absent from older builds under AMX_ABI_OVERRIDE)
        lib.amx_ctc_align_long_workspace.argtypes = lib.amx_ctc_align_workspace.argtypes
        lib.amx_ctc_align_long_workspace.restype = i32
        lib.amx_ctc_align_long_emissions.argtypes = lib.amx_ctc_align_emissions.argtypes
        lib.amx_ctc_align_long_emissions.restype = i32
        lib.amx_ctc_align_long.argtypes = lib.amx_ctc_align.argtypes
        lib.amx_ctc_align_long.restype = i32
    if hasattr(lib, "amx_ctc_align_graph"):  # (added to ABI 7 by name: absent from older builds)
        lib.amx_ctc_align_graph_workspace.argtypes = [i64, i64, i64, C.POINTER(C.c_size_t)]
        lib.amx_ctc_align_graph_workspace.restype = i32
        lib.amx_ctc_align_graph_emissions.argtypes = [i32, vp, i64, i64, vp, i32, i64, i32, i32, vp, vp, vp, vp, vp, i64, vp,
                                                      C.c_size_t, vp, vp, vp, vp, vp, vp, vp]
        lib.amx_ctc_align_graph_emissions.restype = i32
        lib.amx_ctc_align_graph.argtypes = [vp, vp, C.POINTER(i64), i32, i64, vp, vp, vp, vp, vp, i64, vp, C.c_size_t, vp, vp, vp,
                                            vp, vp, vp, vp]
        lib.amx_ctc_align_graph.restype = i32
    if hasattr(lib, "amx_ctc_score"):  # (absent from older builds under AMX_ABI_OVERRIDE)
        lib.amx_ctc_score_workspace.argtypes = [i64, i64, i64, C.POINTER(C.c_size_t)]
        lib.amx_ctc_score_workspace.restype = i32
        lib.amx_ctc_score_emissions.argtypes = [i32, vp, i64, i64, vp, i32, i64, i32, i32, i32, vp, vp, i64, vp, C.c_size_t, vp, vp,
                                                vp, vp, vp, vp, vp]
        lib.amx_ctc_score_emissions.restype = i32
        lib.amx_ctc_score.argtypes = [vp, vp, C.POINTER(i64), i32, i64, i32, vp, vp, i64, vp, C.c_size_t, vp, vp, vp, vp, vp, vp, vp]
        lib.amx_ctc_score.restype = i32
    if hasattr(lib, "amx_ctc_variants_emissions"):  # (added to ABI 7 by name: absent from older builds)
        lib.amx_ctc_variants_workspace.argtypes = [i64, i64, i64, C.POINTER(C.c_size_t)]
        lib.amx_ctc_variants_workspace.restype = i32
        lib.amx_ctc_variants_emissions.argtypes = [i32, vp, i64, i64, vp, i32, i64, i32, i32, vp, vp, i64, vp, C.c_size_t, vp, vp, vp,
                                                   vp, vp]
        lib.amx_ctc_variants_emissions.restype = i32
    if hasattr(lib, "amx_ctc_search_emissions"):  # (absent from older builds under AMX_ABI_OVERRIDE)
        lib.amx_ctc_search_workspace.argtypes = [i64, i64, i64, i64, C.POINTER(C.c_size_t)]
        lib.amx_ctc_search_workspace.restype = i32
        lib.amx_ctc_search_emissions.argtypes = [i32, vp, i64, i64, vp, i32, i64, i32, i32, vp, vp, i32, i64, vp, C.c_size_t, vp, vp, vp,
                                                 vp, vp, vp]
        lib.amx_ctc_search_emissions.restype = i32
    if hasattr(lib, "amx_restrict_outputs"):  # (absent from older builds under AMX_ABI_OVERRIDE)
        lib.amx_restrict_outputs.argtypes = [i32, vp, i64, i64, i32, vp, vp, vp, i32, i32, i64, C.c_uint32, vp, i64, i64, vp, vp]
        lib.amx_restrict_outputs.restype = i32
    if hasattr(lib, "amx_long_plan"):  # (absent from older builds under AMX_ABI_OVERRIDE)
        lib.amx_long_plan.argtypes = [C.POINTER(i64), i32, i64, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), i32, vp, i64,
                                      C.POINTER(i64), C.POINTER(i64)]
        lib.amx_long_plan.restype = i32
        lib.amx_long_gather.argtypes = [i32, vp, i64, vp, i32, vp, i32, i64, i64, vp, vp, vp]
        lib.amx_long_gather.restype = i32
        lib.amx_long_stitch.argtypes = [i32, vp, i64, i32, vp, C.POINTER(AmxLongBlock), i32, vp, i32, i64, vp, vp]
        lib.amx_long_stitch.restype = i32
    lib.amx_check_finite.argtypes = [vp, vp, C.POINTER(i64)]
    lib.amx_check_finite.restype = i32
    lib.amx_greedy_ctc.argtypes = [vp, vp, C.POINTER(i64), i32, i64, vp, vp, vp, vp, vp]
    lib.amx_greedy_ctc.restype = i32
    lib.amx_debug_fetch.argtypes = [vp, i32, i32, vp, i64, C.POINTER(i64)]
    lib.amx_debug_fetch.restype = i32
    lib.amx_timing_fetch.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_int32), i32]
    lib.amx_timing_fetch.restype = i32
    lib.amx_device_bytes.argtypes = [vp]
    lib.amx_device_bytes.restype = i64
    lib.amx_max_utterances.argtypes = [vp, i64]
    lib.amx_max_utterances.restype = i64
    lib.amx_greedy_ctc_emissions.argtypes = [i32, vp, i64, i64, vp, i32, i64, i32, i32, vp, vp, vp, vp, vp]
    lib.amx_greedy_ctc_emissions.restype = i32
    lib.amx_gather_outputs.argtypes = [vp, i32, i32, i32, vp, i64, vp, vp, i32, vp, vp]
    lib.amx_gather_outputs.restype = i32
    lib.amx_dist_last_error.argtypes = []
    lib.amx_dist_last_error.restype = C.c_char_p
    _lib = lib
    return lib


def check(lib: C.CDLL, handle, code: int) -> None:
    """Maps C status codes onto the exception types the reference raises (ValueError for configuration / argument
    problems, RuntimeError otherwise)."""
    if code == AMX_OK:
        return
    message = lib.amx_last_error(handle)
    message = message.decode() if message else f"liballophant_amx error {code}"
    if code == AMX_EINVAL:
        raise ValueError(message)
    if code == AMX_ENOMEM:
        raise MemoryError(message)
    if code == AMX_ERANGE:
        raise FloatingPointError(message)
    raise RuntimeError(message)
