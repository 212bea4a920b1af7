"""No-GPU checks behind tests/test_gpu_buffer_edges.py: the sizing functions of the C ABI (host code: they load without a device and
read only the geometry fields of a hand-filled `sd_ecapa_weights`), the guard-band helper's self-test, and the rule that every exported
entry taking a device pointer has a guarded case.

The caller owns every byte (include/sd_hip.h: the library "never allocates"): it asks a sizing function, hands over exactly that
much, and `EmbeddingEngine` sizes ONE workspace for its largest micro-batch and runs the shorter last one in it.  That is sound only
if the sizes never shrink as B or T grow."""
import ctypes as C
import importlib.util
import os
import re
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import guarded as G  # noqa: E402

from speech_diarization_amd import _native as N  # noqa: E402
from speech_diarization_amd.synth import EcapaConfig  # noqa: E402

GEOMETRIES = {
    "default": EcapaConfig(),
    "c512": EcapaConfig(channels=(512, 512, 512, 512, 1536), attention_channels=128, se_channels=128),
    "small64": EcapaConfig.small(64),
    "small128": EcapaConfig.small(128),
}
PRECISIONS = {"f32": (N.SD_DT_F32, 0), "f32s": (N.SD_DT_F32, 1), "f32ns": (N.SD_DT_F32, 2), "f16": (N.SD_DT_F16, 0)}


def _pad(v, m):
    return (v + m - 1) // m * m


def per_segment_layers(cfg):
    """(cin, cout) of the five per-segment layers (one row per segment: f32 weights, K step 32) from the geometry alone: the SE squeeze
    FC of every block, the global-context bias of the attention TDNN (acts on [mean | std] of the MFA output) and the final FC."""
    C_, Cm = cfg.channels[0], cfg.channels[-1]
    return [(C_, cfg.se_channels)] * cfg.n_blocks + [(2 * Cm, cfg.attention_channels), (2 * Cm, cfg.lin_neurons)]


def geometry_struct(cfg, precision, eligible=True):
    """The fields the sizing functions read, filled by hand (no device, no weights).  eligible=False: cin_pad = 0 on se1, asp_tdnn_g
    and fc, which takes those layers off the split-K route and leaves every other buffer as it is."""
    W = N.sd_ecapa_weights()
    W.w_dtype, W.split16 = PRECISIONS[precision]
    W.n_mels, W.channels, W.n_blocks, W.res2_scale = cfg.input_size, cfg.channels[0], cfg.n_blocks, cfg.res2net_scale
    W.mfa_channels, W.att_channels, W.emb_dim = cfg.channels[-1], cfg.attention_channels, cfg.lin_neurons
    layers = per_segment_layers(cfg)
    for i in range(cfg.n_blocks):
        W.blocks[i].se1.cin, W.blocks[i].se1.cin_pad, W.blocks[i].se1.cout = layers[i][0], _pad(layers[i][0], 32) if eligible else 0, layers[i][1]
    for L, (cin, cout) in ((W.asp_tdnn_g, layers[-2]), (W.fc, layers[-1])):
        L.cin, L.cin_pad, L.cout = cin, _pad(cin, 32) if eligible else 0, cout
    return W


def need(W, B, T):
    return int(N.load().sd_ecapa_workspace_bytes(C.byref(W), B, T))


ALL = [(g, p) for g in GEOMETRIES for p in PRECISIONS]
T_GRID = (5, 63, 64, 127, 128, 201, 212, 213, 256, 257, 3001)


@pytest.mark.parametrize("geom,prec", ALL)
def test_ecapa_workspace_never_shrinks_as_the_batch_grows(geom, prec):
    """Non-decreasing in B at fixed T, B = 1 .. 600.  It used to DROP from B = 256 to 257 for every geometry with 6 C >= 512 at every
    precision: the split-K scratch of the per-segment layers (up to 4.7 MB, final FC) was reserved only up to 256 rows.  Default
    geometry, f32, T = 5: 68 157 440 bytes at 256 rows, 63 686 656 at 257, below the 256-row need up to 275 rows, so an engine with
    max_batch in 257 .. 286 refused its own <= 256-row last micro-batch with SD_ERR_WORKSPACE.  Fixed in carve() (sd_ecapa.hip): the
    256-row share stays reserved above 256 rows."""
    W = geometry_struct(GEOMETRIES[geom], prec)
    for T in T_GRID:
        sizes = [need(W, B, T) for B in range(1, 601)]
        assert sizes[0] > 0
        drops = [(B + 1, sizes[B - 1], sizes[B]) for B in range(1, 600) if sizes[B] < sizes[B - 1]]
        assert not drops, f"{geom} {prec} T={T}: sd_ecapa_workspace_bytes shrinks at (B, bytes before, bytes at B) {drops[:3]}"


@pytest.mark.parametrize("geom,prec", ALL)
def test_ecapa_workspace_never_shrinks_as_segments_grow(geom, prec):
    W = geometry_struct(GEOMETRIES[geom], prec)
    for B in (1, 31, 224, 225, 255, 256, 257, 600):
        sizes = [need(W, B, T) for T in list(range(1, 420)) + [1000, 3000, 3001]]
        assert all(b >= a for a, b in zip(sizes, sizes[1:])), (geom, prec, B)


@pytest.mark.parametrize("geom,prec", ALL)
def test_last_micro_batch_fits_the_workspace_sized_for_the_first(geom, prec):
    """The engine-level form: `embed` / `embed_windows` size for mb = min(max_batch, B) rows and run the remainder of
    B % max_batch rows in the same workspace."""
    W = geometry_struct(GEOMETRIES[geom], prec)
    for T in (5, 201):
        size = {B: need(W, B, T) for B in range(1, 301)}
        for max_batch in range(200, 301):
            for r in (1, 255, 256):
                B = max_batch + r
                last = B % max_batch or max_batch
                assert size[last] <= size[min(max_batch, B)], \
                    f"{geom} {prec} T={T}: max_batch={max_batch}, {B} segments: the last micro-batch of {last} rows needs {size[last]} bytes, the workspace has {size[min(max_batch, B)]}"


@pytest.mark.parametrize("geom", list(GEOMETRIES))
def test_packed_workspace_is_the_uniform_one_and_never_shrinks(geom):
    """One carve serves both schedules: for f32 weights sd_ecapa_packed_workspace_bytes(w, B, M) == sd_ecapa_workspace_bytes(w, B, T)
    whenever M == B * T; non-decreasing in M and in B."""
    lib = N.load()
    W = geometry_struct(GEOMETRIES[geom], "f32")

    def packed(B, M):
        return int(lib.sd_ecapa_packed_workspace_bytes(C.byref(W), B, M))
    for B in (1, 7, 31, 255, 256, 257, 300):
        for T in (5, 64, 201, 3001):
            assert packed(B, B * T) == need(W, B, T), (geom, B, T)
    for B in (1, 31, 256, 257):
        sizes = [packed(B, M) for M in range(5 * B, 5 * B + 3000, 7)]
        assert all(b >= a for a, b in zip(sizes, sizes[1:])), (geom, B)
    M = 600 * 5
    sizes = [packed(B, M) for B in range(1, 601)]
    assert all(b >= a for a, b in zip(sizes, sizes[1:])), (geom, [i + 2 for i, (a, b) in enumerate(zip(sizes, sizes[1:])) if b < a][:3])


def test_seg_gemm_scratch_is_positive_exactly_where_k_is_split():
    lib = N.load()
    for M in (1, 7, 32, 33, 225, 255, 256, 257, 300):
        for cin_pad in (32, 256, 480, 512, 544, 1024, 2048, 2080, 6144):
            for cout in (36, 64, 128, 192):
                got = int(lib.sd_seg_gemm_scratch_bytes(M, cin_pad, cout))
                assert (got > 0) == (M <= 256 and cin_pad >= 512), (M, cin_pad, cout, got)
                assert got % 16 == 0


@pytest.mark.parametrize("geom,prec", ALL)
def test_forward_reserves_the_split_k_scratch_of_its_per_segment_layers(geom, prec):
    """For every B in 1 .. 256 the workspace holds, beyond its other buffers, at least the largest sd_seg_gemm_scratch_bytes over the five
    per-segment layers -- their shapes from EcapaConfig, not from the C code.  (The check that would have caught the forward's scratch
    being 0.7 MB short for the final FC at 225 .. 256 segments, tests/test_gpu_configs.py.)"""
    lib = N.load()
    cfg = GEOMETRIES[geom]
    W, W0 = geometry_struct(cfg, prec), geometry_struct(cfg, prec, eligible=False)
    for T in (5, 201):
        for B in range(1, 257):
            share = need(W, B, T) - need(W0, B, T)
            want = max(int(lib.sd_seg_gemm_scratch_bytes(B, _pad(cin, 32), cout)) for cin, cout in per_segment_layers(cfg))
            assert share >= want, (geom, prec, B, T, share, want)
            assert (want > 0) == (6 * cfg.channels[0] >= 512)


def test_colstat_floats_cover_every_tile_height():
    """sd_conv_args.colstat is documented as [ceil(M / 128)][6][cout], and the exported operators write units of 128 rows whenever they are
    given a colstat: sd_conv1d_cl_f32 takes its 80 / 96 / 112-row tiles only without one (the forward, which can reach them through an
    internal entry that reports the height, parks its statistics in buffers it sizes for 80-row units itself, sd_ecapa.hip)."""
    lib = N.load()
    for M in (1, 79, 80, 127, 128, 129, 1005, 51456):
        for cout in (256, 1024, 3072):
            assert int(lib.sd_colstat_floats(M, cout)) == -(-M // 128) * 6 * cout
    assert int(lib.sd_colstat_floats(0, 256)) == 0 and int(lib.sd_colstat_floats(128, 0)) == 0


def test_small_workspace_formulas():
    lib = N.load()
    for n in (1, 129, 1500, 3001):
        for d in (7, 50, 192):
            f32 = int(lib.sd_cosine_workspace_bytes(n, d))
            assert f32 == _pad(n * _pad(d, 32) * 4, 256)                    # "N * D_pad floats"
            s16 = int(lib.sd_cosine_split16_workspace_bytes(n, d))
            assert s16 >= f32 + n * _pad(d, 32) * 4 + n * 4                 # + the rows as two f16 halves + one scale per row
    assert int(lib.sd_cosine_workspace_bytes(0, 192)) == 0 and int(lib.sd_cosine_split16_workspace_bytes(5, 0)) == 0
    for T, K in ((1, 1), (2, 2), (129, 8), (257, 64), (36000, 8)):
        assert int(lib.sd_viterbi_workspace_bytes(T, K)) == _pad(T * K, 256)  # one back pointer (K <= 64: a byte) per frame and state
    assert int(lib.sd_viterbi_workspace_bytes(0, 8)) == 0
    for n in range(1, 8):                                                     # n convs of 128 -> 128, k = 3, as f16
        assert int(lib.sd_res2net_chain_workspace_bytes(n)) >= n * 128 * 3 * 128 * 2
    assert int(lib.sd_res2net_chain_workspace_bytes(0)) == 0 and int(lib.sd_res2net_chain_workspace_bytes(8)) == 0


# ------------------------------------------------------------------ every entry with a device pointer has a guarded case

EXEMPT = (
    ("sd_abi_version", "version query"), ("sd_sizeof", "layout query"), ("sd_last_error", "host string"), ("sd_device_count", "device query"),
    ("sd_profile_enable", "profiling"), ("sd_profile_read", "profiling: host pointers"),
    ("sd_fbank_plan_create", "plan creation: host tables, allocates its own device tables"), ("sd_fbank_plan_destroy", "plan destruction"),
    ("sd_fbank_num_frames", "size query"), ("sd_fbank_workspace_bytes", "size query"), ("sd_fbank_packed_workspace_bytes", "size query"),
    ("sd_seg_gemm_scratch_bytes", "size query"), ("sd_colstat_floats", "size query"), ("sd_set_tuning", "tuning"),
    ("sd_asp_attend_pool_supported", "geometry query"), ("sd_res2net_chain_supported", "geometry query"),
    ("sd_res2net_chain_workspace_bytes", "size query"), ("sd_ecapa_workspace_bytes", "size query"),
    ("sd_ecapa_packed_workspace_bytes", "size query"), ("sd_cosine_workspace_bytes", "size query"),
    ("sd_cosine_split16_workspace_bytes", "size query"), ("sd_viterbi_workspace_bytes", "size query"),
)


def _gpu_module():
    spec = importlib.util.spec_from_file_location("sd_test_gpu_buffer_edges", os.path.join(HERE, "test_gpu_buffer_edges.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_every_entry_that_takes_a_device_pointer_has_a_guarded_case():
    header = open(N.LIB_PATH.parent.parent / "include" / "sd_hip.h").read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    names = set(re.findall(r"\b(sd_[a-z0-9_]+)\s*\(", header))
    assert names == set(N.PROTOTYPES), names ^ set(N.PROTOTYPES)
    cases = _gpu_module().CASES
    exempt = dict(EXEMPT)
    assert all(reason for reason in exempt.values())
    assert not set(cases) & set(exempt), set(cases) & set(exempt)
    assert not set(cases) - names, set(cases) - names
    missing = sorted(names - set(cases) - set(exempt))
    assert not missing, f"no guarded case in tests/test_gpu_buffer_edges.py for {missing}"
    assert all(len(v) > 0 for v in cases.values())


# ------------------------------------------------------------------ the helper can fail

def test_guard_helper_layout():
    for nbytes in (1, 4, 255, 256, 1000):
        g = G.guarded(nbytes, 0x7B, "cpu")
        assert g.ptr % 256 == 0 and g.payload.numel() == nbytes and g.payload.data_ptr() == g.ptr
        assert g.off >= G.GUARD_BYTES and g.raw.numel() - g.off - nbytes >= G.GUARD_BYTES
        assert bool((g.payload == 0x7B).all()) and bool((g.raw[:g.off] == 0xFF).all()) and bool((g.raw[g.off + nbytes:] == 0xFF).all())
        g.assert_guards_intact()
    t = torch.arange(12, dtype=torch.float32)
    g = G.guarded_from(t, "cpu")
    assert torch.equal(g.view(torch.float32, 3, 4), t.view(3, 4))
    with pytest.raises(ValueError):
        G.guarded(44, 0, "cpu").put(t)


def test_guard_helper_sees_a_stray_write_and_a_stray_read():
    g = G.guarded(64, 0x00, "cpu", name="buf")
    g.raw[g.off - 3] = 1                                   # one byte in front of the payload
    with pytest.raises(G.GuardError, match=r"buf \(64 bytes\): front guard written, first changed byte at offset -3 "):
        g.assert_guards_intact()
    g = G.guarded(64, 0x00, "cpu", name="buf")
    g.raw[g.off + 64 + 5] = 0                              # one byte behind it
    with pytest.raises(G.GuardError, match=r"back guard written, first changed byte at offset 69 "):
        g.assert_guards_intact()
    with pytest.raises(G.GuardError):
        G.assert_guards_intact(G.guarded(8, 0, "cpu"), g)
    # a neighbour column of an output slice
    m = G.guarded(6 * 10 * 4, 0x7B, "cpu").view(torch.float32, 6, 10)
    m[:, 3:7] = 1.0
    G.assert_columns_keep(m, 3, 7, 0x7B)
    m[4, 7] = 1.0
    with pytest.raises(G.GuardError, match=r"neighbour of output columns \[3, 7\) written at row 4, column 7"):
        G.assert_columns_keep(m, 3, 7, 0x7B, "out")
    h = G.guarded(6 * 10 * 2, 0xFF, "cpu").view(torch.float16, 6, 10)
    h[:, 8:] = 2.0
    h[2, 1] = 0.5
    with pytest.raises(G.GuardError, match=r"row 2, column 1"):
        G.assert_columns_keep(h, 8, 10, 0xFF)
    # a read that includes one guard element gives NaN, as f32 and as f16
    for dt, es in ((torch.float32, 4), (torch.float16, 2)):
        g = G.guarded(8 * es, 0x00, "cpu")
        over = g.raw[g.off:g.off + 9 * es].view(dt)       # the payload and the first element behind it
        assert not bool(torch.isnan(g.view(dt).float().sum())) and bool(torch.isnan(over.float().sum()))
        under = g.raw[g.off - es:g.off + 8 * es].view(dt)
        assert bool(torch.isnan(under.float().sum()))
    assert torch.tensor([0x7B] * 4, dtype=torch.uint8).view(torch.float32).item() > 1e36
    assert torch.tensor([0x7B] * 2, dtype=torch.uint8).view(torch.float16).item() == 61280.0
    assert torch.tensor([0xFF] * 4, dtype=torch.uint8).view(torch.int32).item() == -1
