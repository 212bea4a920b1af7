"""The plan of an ECAPA forward (`sd_ecapa_plan_read`, include/sd_hip_trace.h) for the tests and for
tools/forward_census.py: geometries, CPU-built weights, the parsed plan, its rules, and the launch counts it must agree with.

Imported as a helper (tests/helpers on sys.path), like launch_log.py.  Nothing here needs a device."""
import collections
import functools
import re

from launch_log import F32_CONV, kernel_of

PRECISIONS = ("f32", "f16", "f32s", "f32ns")
TILES = ("auto", "wide256")              # the two settings of the f16_tiles fixture (kernel_selection.py): SD_TUNE_F16_NARROW_TILES -1 / 0
GEOMETRIES = ("full", "w64", "w128", "w256", "w256a128", "w512")


def config(geom):
    from speech_diarization_amd.synth import EcapaConfig
    if geom == "full":
        return EcapaConfig()
    if geom == "w512":                                   # no split packing on the wide layers (256 < cout < 1024)
        return EcapaConfig(channels=(512, 512, 512, 512, 1536), attention_channels=128, se_channels=128)
    if geom == "w256a128":
        return EcapaConfig(channels=(256, 256, 256, 256, 768), attention_channels=128, lin_neurons=192, res2net_scale=8, se_channels=32)
    return EcapaConfig.small(int(geom[1:]))              # att 32: the narrow packing on wide-role layers


@functools.lru_cache(maxsize=None)
def state_dict(geom):
    from speech_diarization_amd import synth
    return synth.make_ecapa_state_dict(1234, config(geom))


@functools.lru_cache(maxsize=None)
def cpu_weights(geom, precision):
    """EcapaWeights on the CPU: the struct a forward would be handed, with host pointers nobody dereferences."""
    import torch
    from speech_diarization_amd.engine import EcapaWeights
    return EcapaWeights(state_dict(geom), torch.device("cpu"), precision)


def set_tiles(tiles):
    from speech_diarization_amd import _native as N
    N.check(N.load().sd_set_tuning(N.SD_TUNE_F16_NARROW_TILES, {"auto": -1, "wide256": 0}[tiles]), "sd_set_tuning")


Ref = collections.namedtuple("Ref", "buf lo hi form")
Step = collections.namedtuple("Step", "name route reads writes")
REF = re.compile(r"^([a-z0-9]+)\[(\d+):(\d+)\]:([a-z0-9]+)$")


def read_plan(struct, B, T=0, M=0, map_kind="uniform"):
    """-> (the buffers the carve holds, [Step])"""
    from speech_diarization_amd import _native as N

    def refs(words):
        out = []
        for word in words:
            m = REF.match(word)
            assert m, word
            out.append(Ref(m.group(1), int(m.group(2)), int(m.group(3)), m.group(4)))
        return out
    lines = N.ecapa_plan_read(struct, B, T, M, map_kind)
    assert lines[0][:3] == ("carve", "-", []), lines[0]
    return set(lines[0][3]), [Step(s, r, refs(rd), refs(wr)) for s, r, rd, wr in lines[1:]]


# ------------------------------------------------------------------ the plan against a launch log
ROUTE_KERNELS = {           # route(s) -> the kernels whose launches they are, one launch per step
    ("pack",): {"split16_pack_kernel"},
    ("split128", "split128_folded"): {"conv_gemm_split16_n128_kernel"},
    # (a forward is either f16 or split: "f16" steps are the f16 operator's three kernels, 256x256 split steps two of them)
    ("split256_pack", "split256_twin", "f16"): {"conv_gemm_f16_t256_kernel", "conv_gemm_f16_w4_kernel", "conv_gemm_f16_kernel"},
    ("packed",): {"conv_gemm_f32_packed_kernel"},
    ("chain",): {"res2net_chain_f16_kernel"},
    ("asp_fused",): {"asp_attend_pool_f32_kernel", "asp_attend_pool_f16_kernel"},
    ("asp_pool",): {"asp_pool_kernel", "asp_pool_lds_kernel"},
    ("se_scale",): {"se_scale_residual_kernel"},
    ("colstat_finish",): {"colstat_finish_kernel"},
    ("seg_mean_std",): {"seg_mean_std_kernel"},
    ("cast",): {"cast_f32_f16_kernel"},
}


def launches_of(log, kernels):
    return sum(n for label, n in log.items() if kernel_of(label) in kernels)


def count_mismatches(steps, log):
    """The per-route step counts of a plan against a launch log {label: count} of that forward -> the list of disagreements.
    The exact-f32 and per-segment steps are one launch each of the F32_CONV family, except that a per-segment GEMM that splits K over
    the grid is two (partial + reduce): F32_CONV total == f32 + seg_gemm + packed steps + seg_gemm_reduce launches."""
    routes = collections.Counter(s.route for s in steps)
    bad = []
    for names, kernels in ROUTE_KERNELS.items():
        want, got = sum(routes[r] for r in names), launches_of(log, kernels)
        if want != got:
            bad.append(f"{'/'.join(names)}: {want} steps, {got} launches of {sorted(kernels)}")
    want = routes["f32"] + routes["seg_gemm"] + routes["packed"] + launches_of(log, {"seg_gemm_reduce_f32_kernel"})
    if want != launches_of(log, F32_CONV):
        bad.append(f"f32 + seg_gemm + packed + reduce: {want}, F32_CONV launches {launches_of(log, F32_CONV)}")
    known = {r for names in ROUTE_KERNELS for r in names} | {"f32", "seg_gemm"}
    bad += [f"route {r} is not in the vocabulary" for r in routes if r not in known]
    return bad


# ------------------------------------------------------------------ the forwards of the census and of the GPU test
Case = collections.namedtuple("Case", "id geom precision tiles kind B n rel spans")


def _case(geom, precision, tiles, kind, B=0, n=0, rel=None, spans=None):
    shape = "-".join(str(s) for s in spans) if spans else f"B{B}-n{n}"
    return Case(f"{geom}-{precision}-{tiles}-{kind}-{shape}", geom, precision, tiles, kind, B, n, rel, spans)


def gpu_cases():
    """The smallest forwards at which a route can still go wrong ("the plan is what ran")."""
    out = []
    for tiles in TILES:
        for p in PRECISIONS:
            # T = 201; T = 61, below both colstat floors; T = 129, just above the split colstat floor; past the small-launch routing
            out += [_case("full", p, tiles, "uniform", B, n) for B, n in ((2, 32000), (3, 9600), (2, 20480), (41, 32000))]
        out += [_case("full", p, tiles, "lengths", 3, 32000, rel=(1.0, 0.5, 0.37)) for p in ("f32", "f16")]
        out.append(_case("full", "f32", tiles, "packed", spans=(640, 9600, 32000)))
        out += [_case(g, p, tiles, "uniform", 3, 32000) for g in ("w256a128", "w512") for p in ("f32s", "f32ns")]
    # f16 on either side of sd_res2net_chain_supported (T <= 212): T = 201 is above; T = 216
    out.append(_case("full", "f16", "auto", "uniform", 2, 34400))
    return out


def census_cases():
    """gpu_cases plus both sides of the two small-launch edges at T = 201 (8192 rows: B = 40 / 41; 56 tiles: B = 35 / 36)."""
    edges = [_case("full", p, tiles, "uniform", B, 32000) for tiles in TILES for p in ("f32s", "f32ns") for B in (35, 36, 40)]
    return gpu_cases() + edges


def frames(n):
    return 1 + n // 160


def case_plan(case, struct):
    if case.kind == "packed":
        return read_plan(struct, len(case.spans), M=sum(frames(n) for n in case.spans), map_kind="packed")
    return read_plan(struct, case.B, frames(case.n), map_kind=case.kind)


def run_case(case, engine):
    """One forward of `case` on the GPU -> the embeddings (device tensor).  Seeded by the case alone."""
    import numpy as np
    import torch
    from speech_diarization_amd import synth
    if case.kind == "packed":
        starts = np.concatenate([[0], np.cumsum(case.spans)[:-1]])
        signal = torch.from_numpy(synth.synthetic_segments(7, 1, int(sum(case.spans)))[0]).to(engine.device)
        return engine.embed_spans(signal, starts, np.asarray(case.spans))
    wav = torch.from_numpy(synth.synthetic_segments(7, case.B, case.n)).to(engine.device)
    rel = None if case.rel is None else torch.tensor(case.rel, dtype=torch.float32, device=engine.device)
    return engine.embed(wav, rel)
