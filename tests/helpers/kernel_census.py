"""The census of launch labels (include/sd_hip_trace.h): every label the sources of libsd_hip.so can count, and the GPU test that
asserts the label ran (tests/helpers/launch_log.py) while it checks the kernel's numbers against a reference.

tests/test_launch_log_rules.py reads the labels out of csrc/*.hip and csrc/sd_conv_choice.h and fails when this table and the sources differ, when a named test
does not exist, or when a label is exempt without the guard its exemption claims.  A retuned threshold that orphans a kernel then
fails the named test on the MI355X instead of going unnoticed."""

_EXACT = "test_gpu_exact"
_F32 = (_EXACT, "test_conv1d_cl_f32_every_selection_gives_the_integers")
_F16 = (_EXACT, "test_conv1d_cl_f16_gives_the_integers")
_SPLIT = (_EXACT, "test_conv1d_cl_split16_gives_the_integers")
_REDUCE = (_EXACT, "test_seg_mean_std_and_se_scale_residual_uniform")
_REDUCE_PACKED = (_EXACT, "test_seg_mean_std_and_se_scale_residual_packed")
_POOL = (_EXACT, "test_asp_pool_one_hot_logits_return_one_frame")
_FUSED = (_EXACT, "test_fused_attention_pooling_one_hot")
_CHAIN = (_EXACT, "test_res2net_chain_f16_gives_the_integer_chain")
_AFFINITY = (_EXACT, "test_cosine_affinity_is_k_over_16")
_AHC = (_EXACT, "test_ahc_nearest_breaks_every_tie_towards_the_lowest_index")
_SPECTRAL = (_EXACT, "test_affinity_apply_and_degree_are_exact")
_SWITCH = ("test_gpu_fbank_ecapa", "test_fbank_both_kernels_at_their_length_switch")
_GENERIC = ("test_gpu_fbank_ecapa", "test_fbank_batch_at_other_sample_rates")
_PACKED_FBANK = ("test_gpu_packed", "test_fbank_packed_is_bitwise_the_span_alone")
_HDB_CORE = ("test_gpu_hdbscan", "test_core_equals_the_numpy_kth_largest_on_integer_rows")
_HDB_OUT = ("test_gpu_hdbscan", "test_outgoing_equals_the_numpy_statement_on_integer_rows")

# label -> (test module, test function)
KERNEL_TESTS = {
    # ---- sd_conv1d_cl_f32, sd_seg_gemm_f32, sd_conv1d_cl_packed_f32
    "conv_gemm_f32_s64_kernel<32>": _F32, "conv_gemm_f32_s64_kernel<64>": _F32, "skinny_gemm_f32_kernel": _F32,
    "conv_gemm_f32_t256_kernel": _F32, "conv_gemm_f32_vh_kernel<5>": _F32, "conv_gemm_f32_vh_kernel<6>": _F32,
    "conv_gemm_f32_vh_kernel<7>": _F32, "conv_gemm_f32_n64_kernel": _F32, "conv_gemm_f32_kernel<dma>": _F32,
    "conv_gemm_f32_kernel<dma>/symmetric": _AFFINITY,
    "seg_gemm_partial_f32_kernel": _F32, "seg_gemm_reduce_f32_kernel": _F32,
    "conv_gemm_f32_packed_kernel": (_EXACT, "test_conv1d_cl_packed_f32_gives_the_integers"),
    # ---- sd_conv1d_cl_f16
    **{f"conv_gemm_f16_kernel<{x},{y}>": _F16 for x in ("f16", "f32") for y in ("f16", "f32")},
    **{f"conv_gemm_f16_t256_kernel<{y},{e}>/{w}": _F16 for y in ("f16", "f32") for e, w in (("direct", "grid"), ("direct", "lockstep"), ("staged", "grid"))},
    # ---- sd_conv1d_cl_split16
    **{f"conv_gemm_f16_t256_kernel<split,{e}>/{w}": _SPLIT for e, w in (("direct", "grid"), ("direct", "lockstep"), ("staged", "grid"))},
    "conv_gemm_split16_n128_kernel": _SPLIT, "split16_pack_kernel": _SPLIT,
    # ---- the Res2Net chain
    **{f"res2net_chain_f16_kernel<{n}>": _CHAIN for n in range(1, 8)}, "chain_pack_kernel": _CHAIN,
    # ---- sd_pool.hip, sd_asp_fused.hip
    **{f"seg_mean_std_kernel<{t},uniform,{f}>": _REDUCE for t in ("f32", "f16") for f in ("16x16", "64x4")},
    **{f"seg_mean_std_kernel<{t},packed,64x4>": _REDUCE_PACKED for t in ("f32", "f16")},
    **{f"se_scale_residual_kernel<{t},uniform>": _REDUCE for t in ("f32", "f16")},
    **{f"se_scale_residual_kernel<{t},packed>": _REDUCE_PACKED for t in ("f32", "f16")},
    **{f"asp_pool_lds_kernel<{t}>": _POOL for t in ("f32", "f16")}, **{f"asp_pool_kernel<{t},uniform>": _POOL for t in ("f32", "f16")},
    **{f"asp_pool_kernel<{t},packed>": (_EXACT, "test_asp_pool_packed_one_hot") for t in ("f32", "f16")},
    **{f"asp_attend_pool_f32_kernel<{n}{s}>": _FUSED for n in (4, 8, 13, 16) for s in ("", ",split")},
    **{f"asp_attend_pool_f16_kernel<{n}>": _FUSED for n in (1, 2, 3, 4)},
    "colstat_finish_kernel<f32>": (_EXACT, "test_colstat_f32_gives_the_integer_sums"),
    "colstat_finish_kernel<f16>": (_EXACT, "test_colstat_f16_gives_the_integer_sums"),
    "cast_f32_f16_kernel": ("test_gpu_f16", "test_ecapa_f16_full_geometry"),
    "wav_lens_frames_kernel": ("test_gpu_wav_lens", "test_device_rule_equals_host_rule"),
    # ---- products outside the network
    "affinity_sym_kernel<exact f32>": _AFFINITY, "affinity_sym_kernel<split16x3>": _AFFINITY, "fill_f32_kernel": _AFFINITY,
    "l2norm_rows_kernel": (_EXACT, "test_adjacent_cosine_and_l2norm_rows_are_exact"),
    "adjacent_cosine_kernel": (_EXACT, "test_adjacent_cosine_and_l2norm_rows_are_exact"),
    "sim_argmax_kernel": (_EXACT, "test_sim_argmax_returns_the_first_maximum"),
    "ahc_nearest_kernel": _AHC, "ahc_nearest_finish_kernel": _AHC, "ahc_merge_kernel": _AHC,
    **{f"affinity_apply_kernel<{nj},{ld}>": _SPECTRAL for nj in (1, 2) for ld in ("vec", "scalar")}, "apply_finish_kernel": _SPECTRAL, "affinity_degree_kernel": _SPECTRAL,
    "topk_mean_std_kernel": (_EXACT, "test_topk_mean_std_on_tied_integer_rows"),
    "asnorm_combine_kernel": ("test_gpu_ops", "test_asnorm_scores_gpu_matches_reference_goldens_and_host"),
    "viterbi_kernel": (_EXACT, "test_viterbi_ties_go_to_the_first_state"),
    **{f"{kern}<{k}>": _HDB_CORE for kern in ("hdb_core_kernel", "hdb_core_finish_kernel") for k in (1, 2, 4, 8, 16)},
    "hdb_outgoing_kernel": _HDB_OUT, "hdb_outgoing_finish_kernel": _HDB_OUT,
    # ---- fbank
    "fbank_utt16_kernel<uniform>": _SWITCH, "fbank_logmel_kernel<uniform>": _SWITCH, "fbank_finalize_kernel<uniform>": _SWITCH, "fill_i32_kernel": _SWITCH,
    "fbank_utt16_kernel<packed>": _PACKED_FBANK, "fbank_logmel_kernel<packed>": _PACKED_FBANK, "fbank_finalize_kernel<packed>": _PACKED_FBANK,
    "fbank_packed_tiles_kernel": _PACKED_FBANK,
    "fbg_pad_kernel": _GENERIC, "fbg_dft_f64_kernel": _GENERIC, "fbg_finalize_kernel": _GENERIC,
}

# label -> (reason, the guard in front of its launch site: an experiment variable read through sd_experiment_env, or a build flag the
# shipped build does not set).  A label that is merely hard to reach does not belong here.
EXEMPT = {}
ALLOWED_GUARDS = ("sd_experiment_env(", "#ifdef SD_STAMP")
