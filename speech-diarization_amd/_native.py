"""ctypes binding of libsd_hip.so (C ABI: include/sd_hip.h).

The HIP library is the product path.  There is no CPU fallback: if the shared
object is missing, or exports fewer symbols than the header declares, loading
raises instead of degrading silently.
"""
from __future__ import annotations

import ctypes as C
import threading
from pathlib import Path

PKG_DIR = Path(__file__).resolve().parent
LIB_PATH = PKG_DIR / "libsd_hip.so"

SD_OK = 0
SD_PAD_ZERO, SD_PAD_REFLECT = 0, 1
SD_LOG_LN_EPS, SD_LOG_DB_TOPDB = 0, 1
SD_ACT_NONE, SD_ACT_RELU, SD_ACT_TANH, SD_ACT_SIGMOID = 0, 1, 2, 3
SD_DT_F32, SD_DT_F16, SD_DT_SPLIT16 = 0, 1, 2
SD_TUNE_SKINNY_TILES = 1
SD_TUNE_WIDE_TILES = 2
SD_TUNE_F16_NARROW_TILES = 3
SD_TUNE_S64_TILES = 4
SD_TUNE_HALF_TILES = 5
SD_TUNE_TILE_ROWS = 6
SD_TUNE_T256_LOCKSTEP_TILES = 7
SD_MAX_RES2 = 15
SD_MAX_BLOCKS = 8
SD_ABI_VERSION = 11
SD_PROF_CONV_GEMM, SD_PROF_FBANK, SD_PROF_CONV_WIDE, SD_PROF_SEG_SPLITK = 0, 1, 2, 3


def profile_enable(on: bool) -> None:
    check(load().sd_profile_enable(int(on)), "sd_profile_enable")


def profile_read(kind: int):
    """(total_ms, launches, work) of one kernel family since profile_enable(True)."""
    ms, n, w = C.c_double(), C.c_longlong(), C.c_double()
    check(load().sd_profile_read(kind, C.byref(ms), C.byref(n), C.byref(w)), "sd_profile_read")
    return ms.value, n.value, w.value


class SdError(RuntimeError):
    """A libsd_hip.so entry point returned a non-zero status."""


class sd_conv_args(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("lda", C.c_int), ("a_col0", C.c_int),
        ("w", C.c_void_p), ("w_dtype", C.c_int),
        ("y", C.c_void_p), ("ldo", C.c_int), ("o_col0", C.c_int),
        ("M", C.c_int), ("T", C.c_int),
        ("cin", C.c_int), ("cin_pad", C.c_int), ("cout", C.c_int), ("taps", C.c_int), ("dil", C.c_int),
        ("bias", C.c_void_p), ("bias_per_seg", C.c_int),
        ("act", C.c_int),
        ("scale", C.c_void_p), ("shift", C.c_void_p),
        ("act2", C.c_int),
        ("tee", C.c_void_p), ("ldt", C.c_int), ("tee_lo", C.c_int), ("tee_hi", C.c_int),
        ("tee_add", C.c_void_p), ("ld_ta", C.c_int), ("ta_col0", C.c_int),
        ("x_dtype", C.c_int), ("y_dtype", C.c_int),
        ("colstat", C.c_void_p),
        ("w_scale_inv", C.c_float),
    ]


class sd_layer(C.Structure):
    _fields_ = [
        ("w", C.c_void_p), ("bias", C.c_void_p), ("scale", C.c_void_p), ("shift", C.c_void_p),
        ("cin", C.c_int), ("cin_pad", C.c_int), ("cout", C.c_int), ("taps", C.c_int), ("dil", C.c_int),
        ("w_dtype", C.c_int),
        ("w_split", C.c_void_p), ("bias_split", C.c_void_p), ("scale_split", C.c_void_p), ("split_scale_inv", C.c_float),
    ]


class sd_se_res2_block(C.Structure):
    _fields_ = [
        ("tdnn1", sd_layer),
        ("res2", sd_layer * SD_MAX_RES2),
        ("tdnn2", sd_layer),
        ("se1", sd_layer), ("se2", sd_layer),
    ]


class sd_ecapa_weights(C.Structure):
    _fields_ = [
        ("w_dtype", C.c_int), ("n_mels", C.c_int), ("channels", C.c_int), ("n_blocks", C.c_int),
        ("res2_scale", C.c_int), ("mfa_channels", C.c_int), ("att_channels", C.c_int), ("emb_dim", C.c_int),
        ("asp_eps", C.c_float),
        ("split16", C.c_int),
        ("block0", sd_layer),
        ("blocks", sd_se_res2_block * SD_MAX_BLOCKS),
        ("mfa", sd_layer), ("asp_tdnn_h", sd_layer), ("asp_tdnn_g", sd_layer), ("asp_conv", sd_layer), ("fc", sd_layer),
    ]


_P = C.c_void_p
_I = C.c_int
_F = C.c_float
_Z = C.c_size_t

# symbol -> (restype, argtypes); must list every function sd_hip.h declares
PROTOTYPES = {
    "sd_abi_version": (_I, []),
    "sd_sizeof": (_Z, [_I]),
    "sd_last_error": (C.c_char_p, []),
    "sd_device_count": (_I, []),
    "sd_profile_enable": (_I, [_I]),
    "sd_profile_read": (_I, [_I, C.POINTER(C.c_double), C.POINTER(C.c_longlong), C.POINTER(C.c_double)]),
    "sd_fbank_plan_create": (_P, [_P, _I, _I, _P, _I, _I, _I, _F, _F]),
    "sd_fbank_plan_destroy": (None, [_P]),
    "sd_fbank_num_frames": (_I, [_P, _I]),
    "sd_fbank_workspace_bytes": (_Z, [_P, _I, _I]),
    "sd_fbank_f32": (_I, [_P, _P, _I, _I, _I, _P, _I, _P, _Z, _P]),
    "sd_fbank_windows_f32": (_I, [_P, _P, C.c_longlong, _P, _I, _I, _I, _P, _I, _P, _Z, _P]),
    "sd_conv1d_cl_f32": (_I, [C.POINTER(sd_conv_args), _P]),
    "sd_seg_gemm_f32": (_I, [C.POINTER(sd_conv_args), _P, _Z, _P]),
    "sd_seg_gemm_scratch_bytes": (_Z, [_I, _I, _I]),
    "sd_conv1d_cl_f16": (_I, [C.POINTER(sd_conv_args), _P]),
    "sd_conv1d_cl_split16": (_I, [C.POINTER(sd_conv_args), _P]),
    "sd_split16_pack_f32": (_I, [_P, _I, _I, _I, _I, _F, _P, _I, _P]),
    "sd_set_tuning": (_I, [_I, C.c_long]),
    "sd_colstat_floats": (_Z, [_I, _I]),
    "sd_colstat_finish_dt": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _F, _P, _P]),
    "sd_seg_mean_std_dt": (_I, [_P, _I, _I, _I, _I, _I, _I, _I, _F, _P, _P]),
    "sd_se_scale_residual_dt": (_I, [_P, _I, _P, _P, _I, _I, _P, _I, _I, _I, _I, _I, _I, _P]),
    "sd_asp_pool_dt": (_I, [_P, _I, _P, _I, _I, _I, _I, _I, _F, _P, _P]),
    "sd_asp_attend_pool_supported": (_I, [_I, _I, _I, _I]),
    "sd_asp_attend_pool_dt": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _F, _P, _P]),
    "sd_res2net_chain_supported": (_I, [_I, _I, _I, _I, _I]),
    "sd_res2net_chain_workspace_bytes": (C.c_size_t, [_I]),
    "sd_res2net_chain_f16": (_I, [_P, _I, _I, _I, C.POINTER(sd_layer), _I, _P, C.c_size_t, _P]),
    "sd_ecapa_forward_f16": (_I, [C.POINTER(sd_ecapa_weights), _P, _I, _I, _P, _P, _Z, _P]),
    "sd_seg_mean_f32": (_I, [_P, _I, _I, _I, _I, _I, _P, _P]),
    "sd_seg_mean_std_f32": (_I, [_P, _I, _I, _I, _I, _I, _F, _P, _P]),
    "sd_se_scale_residual_f32": (_I, [_P, _I, _P, _P, _I, _I, _P, _I, _I, _I, _I, _I, _P]),
    "sd_asp_pool_f32": (_I, [_P, _I, _P, _I, _I, _I, _I, _F, _P, _P]),
    "sd_ecapa_workspace_bytes": (_Z, [C.POINTER(sd_ecapa_weights), _I, _I]),
    "sd_ecapa_forward_f32": (_I, [C.POINTER(sd_ecapa_weights), _P, _I, _I, _P, _P, _Z, _P]),
    "sd_l2norm_rows_f32": (_I, [_P, _I, _I, _I, _F, _I, _P, _I, _P]),
    "sd_cosine_workspace_bytes": (_Z, [_I, _I]),
    "sd_cosine_affinity_f32": (_I, [_P, _I, _I, _P, _I, _P, _Z, _P]),
    "sd_cosine_affinity_rows_f32": (_I, [_P, _I, _I, _I, _I, _P, _I, _P, _Z, _P]),
    "sd_cosine_split16_workspace_bytes": (_Z, [_I, _I]),
    "sd_cosine_affinity_rows_split16": (_I, [_P, _I, _I, _I, _I, _P, _I, _P, _Z, _P]),
    "sd_adjacent_cosine_f32": (_I, [_P, _I, _I, _I, _F, _P, _P]),
    "sd_sim_argmax_f32": (_I, [_P, _I, _I, _I, _P, _I, _I, _P, _P, _P]),
    "sd_topk_mean_std_f32": (_I, [_P, _I, _I, _I, _I, _P, _P]),
    "sd_asnorm_combine_f32": (_I, [_P, _I, _I, _I, _P, _P, _P, _I, _P]),
    "sd_viterbi_workspace_bytes": (_Z, [_I, _I]),
    "sd_viterbi_f32": (_I, [_P, _I, _I, _I, _F, _F, _P, _Z, _P, _P]),
    # relative lengths (speechbrain wav_lens)
    "sd_wav_lens_frames": (_I, [_P, _I, _I, _P, _P, _P]),
    "sd_fbank_lens_f32": (_I, [_P, _P, _I, _I, _P, _P, _I, _P, _Z, _P]),
    "sd_seg_mean_std_lens_dt": (_I, [_P, _I, _I, _I, _I, _I, _P, _I, _I, _F, _P, _P]),
    "sd_asp_pool_lens_dt": (_I, [_P, _I, _P, _I, _I, _I, _I, _P, _I, _F, _P, _P]),
    "sd_asp_attend_pool_lens_dt": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _I, _I, _F, _P, _P]),
    "sd_ecapa_forward_lens_f32": (_I, [C.POINTER(sd_ecapa_weights), _P, _I, _I, _P, _P, _P, _Z, _P]),
    "sd_ecapa_forward_lens_f16": (_I, [C.POINTER(sd_ecapa_weights), _P, _I, _I, _P, _P, _P, _Z, _P]),
    # packed spans (segments of different lengths in one launch, each embedded as if alone)
    "sd_fbank_packed_workspace_bytes": (_Z, [_P, _I, _I, _I]),
    "sd_fbank_packed_f32": (_I, [_P, _P, C.c_longlong, _P, _P, _P, _I, _I, _I, _P, _I, _P, _Z, _P]),
    "sd_conv1d_cl_packed_f32": (_I, [C.POINTER(sd_conv_args), _P, _I, _P]),
    "sd_seg_mean_std_packed_dt": (_I, [_P, _I, _I, _I, _P, _I, _I, _I, _I, _F, _P, _P]),
    "sd_se_scale_residual_packed_dt": (_I, [_P, _I, _P, _P, _I, _I, _P, _I, _I, _P, _I, _I, _I, _I, _P]),
    "sd_asp_pool_packed_dt": (_I, [_P, _I, _P, _I, _I, _P, _I, _I, _I, _F, _P, _P]),
    "sd_ecapa_packed_workspace_bytes": (_Z, [C.POINTER(sd_ecapa_weights), _I, _I]),
    "sd_ecapa_forward_packed_f32": (_I, [C.POINTER(sd_ecapa_weights), _P, _P, _I, _I, _P, _P, _Z, _P]),
}

# include/sd_hip_spectral.h: the spectral-clustering entries, same shared object, a table and a version of their own
SD_SPECTRAL_ABI_VERSION = 1
SPECTRAL_PROTOTYPES = {
    "sd_spectral_abi_version": (_I, []),
    "sd_affinity_degree_f32": (_I, [_P, _I, C.c_long, _I, _P, _P]),
    "sd_affinity_apply_workspace_bytes": (_Z, [_I, _I]),
    "sd_affinity_apply_f32": (_I, [_P, _I, C.c_long, _I, _P, _P, _I, _I, _P, _I, _P, _Z, _P]),
}

# include/sd_hip_ahc.h: the agglomerative-clustering entries, same shared object, a table and a version of their own
SD_AHC_ABI_VERSION = 1
AHC_PROTOTYPES = {
    "sd_ahc_abi_version": (_I, []),
    "sd_ahc_nearest_workspace_bytes": (_Z, [_I, _I]),
    "sd_ahc_nearest_f32": (_I, [_P, C.c_long, _I, _I, _P, _P, _P, _P, _Z, _P]),
    "sd_ahc_merge_f32": (_I, [_P, C.c_long, _I, _I, _P, _P, _P, _P, _F, _P, _P, _P]),
    "sd_ahc_nearest_grouped_workspace_bytes": (_Z, [_I, _I, _I]),
    "sd_ahc_nearest_grouped_f32": (_I, [_P, C.c_long, _I, _I, _P, _P, _I, _P, _P, _P, _P, _Z, _P]),
}

# include/sd_hip_hdbscan.h: the density-clustering entries, same shared object, a table and a version of their own
SD_HDBSCAN_ABI_VERSION = 1
HDBSCAN_PROTOTYPES = {
    "sd_hdbscan_abi_version": (_I, []),
    "sd_hdb_core_workspace_bytes": (_Z, [_I, _I, _I]),
    "sd_hdb_core_f32": (_I, [_P, C.c_long, _I, _I, _I, _P, _P, _Z, _P]),
    "sd_hdb_outgoing_workspace_bytes": (_Z, [_I, _I]),
    "sd_hdb_outgoing_f32": (_I, [_P, C.c_long, _I, _I, _P, _P, _P, _P, _P, _Z, _P]),
    "sd_hdb_core_grouped_workspace_bytes": (_Z, [_I, _I, _I, _I]),
    "sd_hdb_core_grouped_f32": (_I, [_P, C.c_long, _I, _I, _I, _P, _I, _P, _P, _P, _Z, _P]),
    "sd_hdb_outgoing_grouped_workspace_bytes": (_Z, [_I, _I, _I]),
    "sd_hdb_outgoing_grouped_f32": (_I, [_P, C.c_long, _I, _I, _P, _P, _P, _I, _P, _P, _P, _P, _Z, _P]),
}

# include/sd_hip_tree.h: from a spanning tree's edges to HDBSCAN's labels, same shared object, a table and a version of their own.
# The table is named TREE_ENTRIES, not *_PROTOTYPES: the six tables of that name are a closed set (ops._ENTRIES is their union, and
# tests/test_binding_rules.py counts them); `ops.launch` looks a name up in this table beside them
SD_TREE_ABI_VERSION = 1
TREE_ENTRIES = {
    "sd_tree_abi_version": (_I, []),
    "sd_tree_labels_workspace_bytes": (_Z, [_I, _I, _I]),
    "sd_tree_labels_grouped": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _Z, _P]),
}

# include/sd_hip_cut.h: from the AHC merge log to the labels at a bounded cluster count, same shared object, a table and a version of
# their own.  CUT_ENTRIES for the reason TREE_ENTRIES has its name: the *_PROTOTYPES tables are a closed set
SD_CUT_ABI_VERSION = 1
CUT_ENTRIES = {
    "sd_cut_abi_version": (_I, []),
    "sd_ahc_cut_workspace_bytes": (_Z, [_I, _I]),
    "sd_ahc_cut_grouped": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _F, _P, _P, _P, _P, _P, _P, _Z, _P]),
}

# include/sd_hip_kmeans.h: scikit-learn's k-means labels for many recordings in one launch, same shared object, a table and a version of
# their own.  KMEANS_ENTRIES for the reason TREE_ENTRIES has its name: the *_PROTOTYPES tables are a closed set
SD_KMEANS_ABI_VERSION = 1
SD_KMEANS_U_STRIDE = 155
KMEANS_ENTRIES = {
    "sd_kmeans_abi_version": (_I, []),
    "sd_kmeans_grouped_workspace_bytes": (_Z, [_I, _I, _I]),
    "sd_kmeans_grouped_f64": (_I, [_P, C.c_long, _I, _I, _P, _I, _P, _I, _I, C.c_double, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _Z, _P]),
}

# include/sd_hip_vad.h: frame scores of the stand-in scorer and frame probabilities to speech runs for many recordings, same shared
# object, a table and a version of their own.  VAD_ENTRIES for the reason TREE_ENTRIES has its name: the *_PROTOTYPES tables are a closed set
SD_VAD_ABI_VERSION = 1
SD_VAD_LDS_FRAMES = 16383
VAD_ENTRIES = {
    "sd_vad_abi_version": (_I, []),
    "sd_vad_energy_grouped_f32": (_I, [_P, C.c_longlong, _P, _P, _I, _I, _I, _F, _F, _P, _I, _P, _P, _P]),
    "sd_vad_segments_workspace_bytes": (_Z, [_I, _I]),
    "sd_vad_segments_grouped": (_I, [_P, _P, _I, _I, _F, _F, _I, _I, _I, _I, _P, _I, _P, _P, _P, _P, _P, _P, _Z, _P]),
}

# include/sd_hip_scd.h: window embeddings to split pieces for the segments of many recordings in one launch, same shared object, a table
# and a version of their own.  SCD_ENTRIES for the reason TREE_ENTRIES has its name: the *_PROTOTYPES tables are a closed set
SD_SCD_ABI_VERSION = 1
SD_SCD_LDS_ROWS = 2048
SCD_ENTRIES = {
    "sd_scd_abi_version": (_I, []),
    "sd_scd_split_workspace_bytes": (_Z, [_I, _I]),
    "sd_scd_split_grouped_f32": (_I, [_P, _I, _I, _I, _P, _I, _P, _P, C.c_double, C.c_double, C.c_double, _F, _P, _I, _P, _P, _P, _P, _P, _P, _P,
                                      _P, _Z, _P]),
}

# include/sd_hip_turns.h: window labels to relabelled labels and speaker-turn runs for many recordings in one launch, same shared object, a
# table and a version of their own.  TURNS_ENTRIES for the reason TREE_ENTRIES has its name: the *_PROTOTYPES tables are a closed set
SD_TURNS_ABI_VERSION = 1
SD_TURNS_LDS_WINDOWS = 4096
TURNS_ENTRIES = {
    "sd_turns_abi_version": (_I, []),
    "sd_turns_workspace_bytes": (_Z, [_I, _I]),
    "sd_turns_grouped": (_I, [_P, _P, _I, _P, _I, _P, _I, _P, _P, C.c_double, _P, _P, _P, _P, _P, _P, _P, _P, _P, _Z, _P]),
}

# include/sd_hip_diag.h: f64 whitening statistics / transform and cluster centres, same shared object, a table and a version of their own
SD_DIAG_ABI_VERSION = 1
_D = C.c_double
DIAG_PROTOTYPES = {
    "sd_diag_abi_version": (_I, []),
    "sd_whiten_stats_workspace_bytes": (_Z, [_I, _I]),
    "sd_whiten_stats_f64": (_I, [_P, C.c_long, _I, _I, _P, _P, C.c_long, _P, _Z, _P]),
    "sd_whiten_apply_f64": (_I, [_P, C.c_long, _I, _I, _P, _P, C.c_long, _D, _P, C.c_long, _P]),
    "sd_label_centroids_f32": (_I, [_P, C.c_long, _I, _I, _P, _I, _D, _P, C.c_long, _P, _P]),
}

# include/sd_hip_trace.h: the launch log and the ECAPA plan, same shared object, a table and a version of its own
SD_TRACE_ABI_VERSION = 3
TRACE_PROTOTYPES = {
    "sd_trace_abi_version": (_I, []),
    "sd_launch_log_enable": (_I, [_I]),
    "sd_launch_log_read": (_Z, [C.c_char_p, _Z]),
    "sd_ecapa_plan_read": (_Z, [_P, _I, _I, _I, _I, C.c_char_p, _Z]),
    "sd_conv_choice_read": (_Z, [C.POINTER(sd_conv_args), _I, _I, _Z, C.c_char_p, _Z]),
}

_lib = None
_lock = threading.Lock()


def load() -> C.CDLL:
    """Load libsd_hip.so once per process; raises if it is absent or incomplete."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        import os
        lib_path = LIB_PATH
        if os.environ.get("SD_HIP_LIB") and os.environ.get("SD_EXPERIMENT") == "1":   # A/B builds (build_native.py --variant); never in product runs
            lib_path = Path(os.environ["SD_HIP_LIB"])
            if not lib_path.exists():
                raise RuntimeError(f"SD_HIP_LIB={lib_path} does not exist")
        if not lib_path.exists():
            raise RuntimeError(
                f"{LIB_PATH} is missing: the HIP hot path is not built. Run "
                "`python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc). "
                "There is deliberately no CPU fallback."
            )
        lib = C.CDLL(str(lib_path))
        for header, table, version, expected, label in (
                ("sd_hip.h", PROTOTYPES, "sd_abi_version", SD_ABI_VERSION, ""),
                ("sd_hip_spectral.h", SPECTRAL_PROTOTYPES, "sd_spectral_abi_version", SD_SPECTRAL_ABI_VERSION, "spectral "),
                ("sd_hip_ahc.h", AHC_PROTOTYPES, "sd_ahc_abi_version", SD_AHC_ABI_VERSION, "AHC "),
                ("sd_hip_hdbscan.h", HDBSCAN_PROTOTYPES, "sd_hdbscan_abi_version", SD_HDBSCAN_ABI_VERSION, "HDBSCAN "),
                ("sd_hip_tree.h", TREE_ENTRIES, "sd_tree_abi_version", SD_TREE_ABI_VERSION, "tree "),
                ("sd_hip_cut.h", CUT_ENTRIES, "sd_cut_abi_version", SD_CUT_ABI_VERSION, "cut "),
                ("sd_hip_kmeans.h", KMEANS_ENTRIES, "sd_kmeans_abi_version", SD_KMEANS_ABI_VERSION, "k-means "),
                ("sd_hip_vad.h", VAD_ENTRIES, "sd_vad_abi_version", SD_VAD_ABI_VERSION, "VAD "),
                ("sd_hip_scd.h", SCD_ENTRIES, "sd_scd_abi_version", SD_SCD_ABI_VERSION, "SCD "),
                ("sd_hip_turns.h", TURNS_ENTRIES, "sd_turns_abi_version", SD_TURNS_ABI_VERSION, "turns "),
                ("sd_hip_diag.h", DIAG_PROTOTYPES, "sd_diag_abi_version", SD_DIAG_ABI_VERSION, "diag "),
                ("sd_hip_trace.h", TRACE_PROTOTYPES, "sd_trace_abi_version", SD_TRACE_ABI_VERSION, "trace ")):
            missing = [name for name in table if not hasattr(lib, name)]
            if missing:
                raise RuntimeError(f"{lib_path} lacks symbols declared in include/{header}: {missing}")
            for name, (res, args) in table.items():
                fn = getattr(lib, name)
                fn.restype = res
                fn.argtypes = args
            got = getattr(lib, version)()
            if got != expected:
                raise RuntimeError(f"libsd_hip.so {label}ABI {got} != binding ABI {expected}; rebuild")
        for which, st in enumerate((sd_conv_args, sd_layer, sd_se_res2_block, sd_ecapa_weights)):
            if lib.sd_sizeof(which) != C.sizeof(st):
                raise RuntimeError(f"{st.__name__}: binding layout is {C.sizeof(st)} bytes, the library's {lib.sd_sizeof(which)}; rebuild")
        _lib = lib
    return _lib


def launch_log_enable(on: bool) -> bool:
    """Start (clearing the counts) or stop the launch log of include/sd_hip_trace.h; -> whether it was on."""
    return bool(load().sd_launch_log_enable(int(on)))


def launch_log_read() -> dict:
    """{label: launches} since the last launch_log_enable(True)."""
    lib = load()
    need = lib.sd_launch_log_read(None, 0)
    while True:
        buf = C.create_string_buffer(need)
        got = lib.sd_launch_log_read(buf, need)
        if got <= need:
            break
        need = got
    out = {}
    for line in buf.value.decode().splitlines():
        label, _, count = line.rpartition("\t")
        out[label] = int(count)
    return out


PLAN_MAPS = {"uniform": 0, "lengths": 1, "packed": 2}


def ecapa_plan_read(weights, B: int, T: int = 0, M: int = 0, map_kind: str = "uniform") -> list:
    """The plan of one ECAPA forward (include/sd_hip_trace.h; no device): [(step, route, [reads], [writes])], the "carve" line first.
    `weights`: an sd_ecapa_weights.  Tensors are "buffer[col0:col1]:form"."""
    lib = load()
    need = 1 << 14
    while True:
        buf = C.create_string_buffer(need)
        got = lib.sd_ecapa_plan_read(C.byref(weights), B, T, M, PLAN_MAPS[map_kind], buf, need)
        if got == 0:
            raise SdError(f"sd_ecapa_plan_read refused: {last_error()}")
        if got <= need:
            break
        need = got
    return [(s, r, rd.split(), wr.split()) for s, r, rd, wr in (line.split("\t") for line in buf.value.decode().splitlines())]


CONV_OPS = {"f32": 0, "f32_symmetric": 1, "f32_stat_rows": 2, "f16": 3, "split16": 4, "packed": 5, "seg_gemm": 6}


def conv_choice_read(args, op: str, n_cu: int = 256, scratch_bytes: int = 0) -> list:
    """What entry `op` (CONV_OPS) would launch for the sd_conv_args `args` on a device of n_cu compute units (include/sd_hip_trace.h; no
    device, no pointer is read): [(label, grid, block, lds_bytes, stat_rows)], one per launch.  SdError where the entry refuses."""
    buf = C.create_string_buffer(512)
    if load().sd_conv_choice_read(C.byref(args), CONV_OPS[op], n_cu, scratch_bytes, buf, 512) == 0:
        raise SdError(f"sd_conv_choice_read refused: {last_error()}")
    return [(f[0], *(int(v) for v in f[1:])) for f in (line.split("\t") for line in buf.value.decode().splitlines())]


def last_error() -> str:
    msg = load().sd_last_error()
    return msg.decode("utf-8", "replace") if msg else ""


def check(status: int, what: str) -> None:
    if status != SD_OK:
        raise SdError(f"{what} failed (status {status}): {last_error()}")
