"""No-GPU checks of packed spans (segments of different lengths in one launch, each embedded as if alone): the new C-ABI entries are
declared, bound and exported under ABI 11, they refuse what the host can check without touching a device, and the host side of
`embed_spans` (frame offsets, the micro-batch planner, span validation) behaves as documented."""
import ctypes as C

import numpy as np
import pytest
import torch

from speech_diarization_amd import _native
from speech_diarization_amd.engine import check_spans, plan_span_batches, span_frame_offsets

PACKED = ("sd_fbank_packed_workspace_bytes", "sd_fbank_packed_f32", "sd_conv1d_cl_packed_f32", "sd_seg_mean_std_packed_dt",
          "sd_se_scale_residual_packed_dt", "sd_asp_pool_packed_dt", "sd_ecapa_packed_workspace_bytes", "sd_ecapa_forward_packed_f32")


def test_packed_entries_are_declared_bound_and_exported_under_abi_11():
    lib = _native.load()
    assert _native.SD_ABI_VERSION == 11 and lib.sd_abi_version() == 11
    header = open(_native.LIB_PATH.parent.parent / "include" / "sd_hip.h").read()
    for name in PACKED:
        assert hasattr(lib, name) and name in _native.PROTOTYPES and f"{name}(" in header, name


def test_host_side_refusals_launch_nothing():
    lib = _native.load()
    x = (C.c_float * 64)()
    p = C.addressof(x)
    # fbank: null plan, B < 0, M <= 0 with B > 0; B == 0 is an empty call
    assert lib.sd_fbank_packed_f32(None, p, 64, p, p, p, 1, 5, 640, p, 80, p, 256, None) == -1 and "null plan" in _native.last_error()
    assert lib.sd_fbank_packed_f32(None, p, 64, p, p, p, -1, 5, 640, p, 80, p, 256, None) == -1
    # (a plan needs device tables; the workspace size does not depend on it)
    assert lib.sd_fbank_packed_workspace_bytes(None, 0, 0, 0) == 0
    assert lib.sd_fbank_packed_workspace_bytes(None, 3, 30, 640) >= 3 * 4 + 4 * 4
    # conv: null args / table, B < 1
    a = _native.sd_conv_args()
    assert lib.sd_conv1d_cl_packed_f32(None, p, 1, None) == -1
    assert lib.sd_conv1d_cl_packed_f32(C.byref(a), None, 1, None) == -1
    assert lib.sd_conv1d_cl_packed_f32(C.byref(a), p, 0, None) == -1
    a.x, a.w, a.y, a.M, a.cin, a.cin_pad, a.cout, a.taps, a.dil, a.lda, a.ldo = p, p, p, 0, 4, 32, 8, 3, 1, 4, 8
    assert lib.sd_conv1d_cl_packed_f32(C.byref(a), p, 1, None) == -1 and "M=0" in _native.last_error()
    # reductions: B < 0 refused, B == 0 nothing to do, M <= 0 with B > 0 refused, null table refused
    for B, M, fs, want in ((-1, 10, p, -1), (0, 0, None, 0), (2, 0, p, -1), (2, 10, None, -1)):
        assert lib.sd_seg_mean_std_packed_dt(p, 0, 4, 0, fs, B, M, 4, 1, 1e-12, p, None) == want, (B, M)
        assert lib.sd_asp_pool_packed_dt(p, 4, p, 0, 4, fs, B, M, 4, 1e-12, p, None) == want, (B, M)
        assert lib.sd_se_scale_residual_packed_dt(p, 4, p, p, 4, 0, p, 4, 0, fs, B, M, 4, 0, None) == want, (B, M)
    assert lib.sd_seg_mean_std_packed_dt(None, 0, 4, 0, p, 1, 10, 4, 1, 1e-12, p, None) == -1        # null input


def test_forward_refuses_weights_that_are_not_exact_f32():
    lib = _native.load()
    x = (C.c_float * 64)()
    p = C.addressof(x)
    assert lib.sd_ecapa_forward_packed_f32(None, p, p, 1, 5, p, p, 64, None) == -1
    for dtype, split in ((_native.SD_DT_F16, 0), (_native.SD_DT_F32, 1), (_native.SD_DT_F32, 2)):
        w = _native.sd_ecapa_weights()
        w.w_dtype, w.split16 = dtype, split
        assert lib.sd_ecapa_forward_packed_f32(C.byref(w), p, p, 1, 5, p, p, 64, None) == -2, (dtype, split)
        assert "exact-f32" in _native.last_error()
    w = _native.sd_ecapa_weights()
    assert lib.sd_ecapa_forward_packed_f32(C.byref(w), p, p, -1, 5, p, p, 64, None) == -1
    assert lib.sd_ecapa_forward_packed_f32(C.byref(w), p, p, 0, 0, p, p, 64, None) == 0
    assert lib.sd_ecapa_forward_packed_f32(C.byref(w), p, None, 2, 10, p, p, 64, None) == -1
    assert lib.sd_ecapa_forward_packed_f32(C.byref(w), p, p, 2, 0, p, p, 64, None) == -1
    assert lib.sd_ecapa_packed_workspace_bytes(None, 2, 10) == 0


def test_frame_offsets_are_prefix_sums_of_one_plus_n_over_160():
    n = [640, 799, 800, 9600, 32000, 32100, 32160, 100000, 480000]
    fs = span_frame_offsets(n)
    assert fs.dtype == np.int32 and fs.shape == (len(n) + 1,)
    T = [1 + k // 160 for k in n]
    assert T[:3] == [5, 5, 6] and T[4:7] == [201, 201, 202] and T[-1] == 3001
    assert fs.tolist() == [0] + np.cumsum(T).tolist()
    assert span_frame_offsets([]).tolist() == [0]
    with pytest.raises(ValueError):
        span_frame_offsets([2 ** 31 - 1] * 200)


def _check_plan(frames, budget):
    plan = plan_span_batches(frames, budget)
    flat = [i for lo, hi in plan for i in range(lo, hi)]
    assert flat == list(range(len(frames)))                         # order kept, nothing split, nothing lost
    for lo, hi in plan:
        assert hi > lo
        total = sum(frames[lo:hi])
        assert total <= budget or hi - lo == 1                      # over budget only alone
    for (lo, hi), (lo2, _) in zip(plan, plan[1:]):
        assert sum(frames[lo:hi]) + frames[lo2] > budget            # greedy: the next span would not have fitted
    return plan


def test_micro_batch_planner():
    assert plan_span_batches([], 100) == []
    assert _check_plan([10, 20, 30, 40], 1000) == [(0, 4)]
    assert _check_plan([10, 20, 30, 40], 50) == [(0, 2), (2, 3), (3, 4)]
    assert _check_plan([5, 300, 5, 5], 100) == [(0, 1), (1, 2), (2, 4)]     # an over-budget span alone
    assert _check_plan([300], 100) == [(0, 1)]
    g = np.random.default_rng(3)
    for _ in range(50):
        frames = g.integers(5, 3002, int(g.integers(1, 60))).tolist()
        _check_plan(frames, int(g.integers(5, 20000)))


def test_span_validation_raises_before_any_launch():
    n_total = 50000
    st, ln = check_spans(np.array([0, 100], np.int32), torch.tensor([640, 49900]), n_total, 640, 5)
    assert st.dtype == np.int64 and ln.dtype == np.int64 and st.tolist() == [0, 100] and ln.tolist() == [640, 49900]
    st, ln = check_spans([], [], n_total, 640, 5)
    assert st.size == 0 and ln.size == 0
    with pytest.raises(ValueError, match=r"too short.*5 frames \(640 samples\)"):
        check_spans([0, 10], [640, 639], n_total, 640, 5)
    with pytest.raises(ValueError, match="past the end"):
        check_spans([0, n_total - 700], [640, 701], n_total, 640, 5)
    with pytest.raises(ValueError, match=">= 0"):
        check_spans([-1], [640], n_total, 640, 5)
    with pytest.raises(ValueError, match="differ"):
        check_spans([0, 1], [640], n_total, 640, 5)
    with pytest.raises(ValueError, match="integers"):
        check_spans([0.0], [640.0], n_total, 640, 5)
    with pytest.raises(ValueError, match="integers"):
        check_spans([True], [640], n_total, 640, 5)
    with pytest.raises(ValueError, match="1-d"):
        check_spans([[0]], [[640]], n_total, 640, 5)
