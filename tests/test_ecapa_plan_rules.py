"""No-GPU checks of the ECAPA forward's plan (csrc/sd_ecapa.hip), read through `sd_ecapa_plan_read`
(include/sd_hip_trace.h) over a sweep of precisions, tunings, segment maps, batch sizes, lengths and geometries.

The forward decides every layer's route and every tensor's form once, in make_plan(); a tensor written only as SD_DT_SPLIT16 halves,
with no f32 copy, is read correctly only if its readers' routes and its writer agree.  These tests hold the plan to that as a data-flow
property of its text, and to the parent's launches and workspace sizes recorded in profiles/ecapa_plan_parity.json
(tools/forward_census.py: the parent commit's library on the MI355X)."""
import collections
import ctypes as C
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import ecapa_plan as P  # noqa: E402

from speech_diarization_amd import _native as N  # noqa: E402

pytestmark = pytest.mark.skipif(not N.LIB_PATH.exists(), reason="libsd_hip.so is not built")

# Edges, from the code: at C = 1024 and T = 201 the C-wide layers leave the 128x128 kernels above 8192 rows (B = 40: 8040, B = 41:
# 8241); the narrow layers leave the exact operator above 56 tiles of 128x128 (B = 35: 7035 rows, B = 36: 7236); column statistics
# start at T = 64, or 128 when the wide layers are split; the split-K scratch share is 256 / 257 rows.
SWEEP_B = (1, 2, 35, 36, 40, 41, 44, 256, 257)
SWEEP_T = (7, 61, 63, 64, 127, 128, 129, 201)
PARITY = os.path.join(os.path.dirname(HERE), "profiles", "ecapa_plan_parity.json")

# Two names for the same bytes: the attention TDNN's output lies over x0 (dead once block 1 has consumed it), the attention logits over
# xcat (dead after the MFA conv).  A buffer also changes ROLE with its form: s0 and r hold a conv epilogue's column sums ("stat") once
# their activations are dead.  A role may be read only while it is the last one written to its bytes.
ALIAS = {"a1": "x0", "e": "xcat"}


def overlaps(a, b):
    return a.buf == b.buf and a.form == b.form and a.lo < b.hi and b.lo < a.hi


def covered(ref, writes):
    """Is every column of `ref` inside the union of `writes` (same buffer and form)?"""
    at = ref.lo
    for w in sorted((w for w in writes if w.buf == ref.buf and w.form == ref.form), key=lambda w: w.lo):
        if w.lo > at:
            break
        at = max(at, w.hi)
    return at >= ref.hi


def minus(pieces, ref):
    """[(step, Ref)] with the columns of `ref` taken out of every piece of its buffer and form"""
    out = []
    for n, w in pieces:
        if not overlaps(w, ref):
            out.append((n, w))
            continue
        out += [(n, w._replace(hi=ref.lo))] if w.lo < ref.lo else []
        out += [(n, w._replace(lo=ref.hi))] if ref.hi < w.hi else []
    return out


def plan_faults(present, steps):
    """Every way `steps` breaks the four data-flow rules -> a list of texts (empty: the plan is sound)."""
    bad = []
    written = []                                    # every Ref written so far
    role = {}                                       # bytes (canonical buffer) -> (buffer name, form) last written there
    unread = []                                     # (step, columns) written and not read since: for "one writer"
    for k, s in enumerate(steps):
        for r in s.reads:
            # closure: what a step reads, an earlier step wrote in that form (the features come from the caller).  With it, an f32
            # form that is skipped has no reader: a step that read it as f32 would fail here.
            if r.buf != "feats" and not covered(r, written):
                bad.append(f"{s.name} reads {r}, which no earlier step wrote")
            if r.buf != "feats" and role.get(ALIAS.get(r.buf, r.buf)) not in (None, (r.buf, r.form)):
                bad.append(f"{s.name} reads {r} after its bytes were reused as {role[ALIAS.get(r.buf, r.buf)]}")
            unread = minus(unread, r)
        for w in s.writes:
            # one writer between two reads: columns that were written and not read since are not written again
            bad += [f"{s.name} overwrites {old} of {n}, which nothing read" for n, old in unread if overlaps(old, w)]
            unread = minus(unread, w)
            if w.form != "scratch":
                unread.append((s.name, w))
            written.append(w)
            role[ALIAS.get(w.buf, w.buf)] = (w.buf, w.form)
        # The stated exception, the Res2Net tee: tdnn1 writes all of r AND a copy of chunk 1 into s0 (its second write).  Chunk 1 is
        # consumed from that copy, never from r, where the first Res2Net step (or the next block's tdnn1) overwrites it unread.  The
        # other chunks are read from r (pack, tee_add, tdnn2, the fused chain) before the ping-pong through s0 / s1 overwrites them.
        if s.name.endswith(".tdnn1") and len(s.writes) == 2 and s.writes[1].buf == "s0":
            chunk = s.writes[1].hi - s.writes[1].lo
            unread = minus(unread, s.writes[0]._replace(lo=chunk, hi=2 * chunk))
        # buffers present: the carve of this geometry and mode holds every buffer a step names
        for r in s.reads + s.writes:
            if r.buf not in ("feats", "emb") and r.buf not in present:
                bad.append(f"{s.name} names {r.buf}, which the carve does not hold")
    # no dead forms: every SD_DT_SPLIT16 tensor (every pack output is one) has a later reader
    for k, s in enumerate(steps):
        for w in s.writes:
            if w.form == "split" and not any(overlaps(w, r) for t in steps[k + 1:] for r in t.reads):
                bad.append(f"{s.name} writes {w}, which no later step reads")
    if not steps or [w.buf for w in steps[-1].writes] != ["emb"]:
        bad.append("the last step does not write the embedding")
    return bad


def shapes(precision):
    for kind in ("uniform", "lengths") + (("packed",) if precision == "f32" else ()):
        for B in SWEEP_B:
            for T in SWEEP_T:
                yield kind, B, T


def read(struct, kind, B, T):
    return P.read_plan(struct, B, M=B * T, map_kind="packed") if kind == "packed" else P.read_plan(struct, B, T, map_kind=kind)


@pytest.fixture(params=P.TILES)
def tiles(request):
    P.set_tiles(request.param)
    yield request.param
    P.set_tiles("auto")


@pytest.mark.parametrize("geom", P.GEOMETRIES)
def test_every_plan_of_the_sweep_is_closed_alive_single_writer_and_inside_its_carve(geom, tiles):
    seen = collections.Counter()
    for precision in P.PRECISIONS:
        struct = P.cpu_weights(geom, precision).struct
        for kind, B, T in shapes(precision):
            present, steps = read(struct, kind, B, T)
            faults = plan_faults(present, steps)
            assert not faults, (geom, precision, tiles, kind, B, T, faults[:4])
            seen.update(s.route for s in steps)
    # the sweep is worth its name: it reaches every route this geometry can take
    # (the fused chain is for chunks of 128 channels and the folded / 256x256 routes for cout >= 1024: the full geometry alone)
    want = {"f32", "f16", "packed", "seg_gemm", "cast", "se_scale", "seg_mean_std", "split128"} | ({"asp_fused"} if geom in ("w256a128", "w512") else {"asp_pool"})
    if geom == "full":
        want = {"f32", "split128", "split128_folded", "split256_pack", "split256_twin", "f16", "packed", "seg_gemm", "chain", "cast", "pack",
                "asp_fused", "asp_pool", "se_scale", "colstat_finish", "seg_mean_std"} - ({"split128_folded"} if tiles == "wide256" else set())
    assert want <= set(seen), sorted(want - set(seen))


def test_the_rules_bite():
    """A plan with a reader of an unwritten form, a dead split tensor, a double write, a reused buffer and a missing buffer is faulted."""
    R, S = P.Ref, P.Step
    good = [S("stem", "f32", [R("feats", 0, 80, "f32")], [R("x0", 0, 64, "f32")]), S("fc", "seg_gemm", [R("x0", 0, 64, "f32")], [R("emb", 0, 8, "f32")])]
    assert plan_faults({"x0"}, good) == []
    assert any("carve" in f for f in plan_faults(set(), good))
    assert any("no earlier step wrote" in f for f in plan_faults({"x0"}, [good[0]._replace(writes=[R("x0", 0, 32, "f32")]), good[1]]))
    assert any("no earlier step wrote" in f for f in plan_faults({"x0", "x0s"}, [good[0]._replace(writes=[R("x0s", 0, 64, "split")]), good[1]]))
    dead = [good[0]._replace(writes=[R("x0", 0, 64, "f32"), R("x0s", 0, 64, "split")]), good[1]]
    assert any("no later step reads" in f for f in plan_faults({"x0", "x0s"}, dead))
    twice = [good[0], S("again", "f32", [R("feats", 0, 80, "f32")], [R("x0", 32, 64, "f32")]), good[1]]
    assert any("nothing read" in f for f in plan_faults({"x0"}, twice))
    reused = [good[0], S("asp_h", "f32", [R("feats", 0, 80, "f32")], [R("a1", 0, 8, "f32")]), good[1]]
    assert any("reused" in f for f in plan_faults({"x0", "a1"}, reused))


def test_a_changed_tuning_value_does_not_split_a_plan():
    """Each read takes one snapshot of SD_TUNE_F16_NARROW_TILES: the plan before and the plan after a change are each sound, and they
    differ (B = 2 is a small launch only under the shipped value)."""
    struct = P.cpu_weights("full", "f32s").struct
    texts = []
    try:
        for tiles in ("auto", "wide256", "auto"):
            P.set_tiles(tiles)
            present, steps = P.read_plan(struct, 2, 201)
            assert not plan_faults(present, steps), tiles
            texts.append([(s.name, s.route) for s in steps])
    finally:
        P.set_tiles("auto")
    assert texts[0] == texts[2] != texts[1]
    assert {r for _, r in texts[0]} >= {"split128_folded"} and not {r for _, r in texts[1]} & {"split128_folded"}


def test_refusals_set_the_error_and_return_nothing():
    lib = N.load()
    struct = P.cpu_weights("w64", "f32s").struct
    assert lib.sd_ecapa_plan_read(None, 2, 201, 0, 0, None, 0) == 0 and "null weights" in N.last_error()
    assert lib.sd_ecapa_plan_read(C.byref(struct), 2, 201, 402, 2, None, 0) == 0 and "exact-f32 schedule only" in N.last_error()
    assert lib.sd_ecapa_plan_read(C.byref(struct), 0, 201, 0, 0, None, 0) == 0 and "sd_ecapa_plan_read" in N.last_error()
    assert lib.sd_ecapa_plan_read(C.byref(struct), 2, 201, 0, 3, None, 0) == 0
    need = int(lib.sd_ecapa_plan_read(C.byref(struct), 2, 201, 0, 0, None, 0))
    small = C.create_string_buffer(b"x" * 16, 16)
    assert need > 16 and int(lib.sd_ecapa_plan_read(C.byref(struct), 2, 201, 0, 0, small, 16)) == need and small.raw[15] == 0 and small.raw[:5] == b"carve"


# ------------------------------------------------------------------ against the parent commit's record

def parity():
    return json.load(open(PARITY))


def test_the_parity_record_shows_no_difference():
    rec = parity()
    assert rec["summary"]["differing"] == [] and rec["summary"]["forwards"] == len(P.census_cases()) == len(rec["forwards"])
    assert set(rec["forwards"]) == {c.id for c in P.census_cases()}
    assert rec["summary"]["workspace_sizes"] == len(rec["workspace"]) == len(P.GEOMETRIES) * len(P.PRECISIONS) * len(SWEEP_B) * len(SWEEP_T)


def test_workspace_sizes_never_shrink_with_B_and_equal_the_parents():
    lib, want = N.load(), parity()["workspace"]
    for geom in P.GEOMETRIES:
        for precision in P.PRECISIONS:
            W = C.byref(P.cpu_weights(geom, precision).struct)
            for T in SWEEP_T:
                last = (0, 0)
                for B in SWEEP_B:
                    got = (int(lib.sd_ecapa_workspace_bytes(W, B, T)), int(lib.sd_ecapa_packed_workspace_bytes(W, B, B * T)))
                    assert list(got) == want[f"{geom}-{precision}-B{B}-T{T}"], (geom, precision, B, T)
                    assert got[0] >= last[0] > -1 and got[1] >= last[1], (geom, precision, B, T)
                    last = got


def test_every_plan_counts_what_the_parent_launched():
    """The launch logs are the parent library's (one forward each on the MI355X), not the new code's: route by route the plan of the
    same forward has as many steps as the parent launched kernels of that route."""
    logs = parity()["forwards"]
    try:
        for case in P.census_cases():
            P.set_tiles(case.tiles)
            present, steps = P.case_plan(case, P.cpu_weights(case.geom, case.precision).struct)
            assert not plan_faults(present, steps), case.id
            assert not P.count_mismatches(steps, logs[case.id]["launches"]), (case.id, P.count_mismatches(steps, logs[case.id]["launches"]))
    finally:
        P.set_tiles("auto")


def test_the_small_launch_edge_of_the_wide_layers_is_where_the_parent_had_it():
    """f32s, full geometry, shipped tuning, T = 201.  B = 41 (8241 rows): four pack passes -- the stem's input and chunk 0 of r in each
    block -- and the stem's output exists as SD_DT_SPLIT16 only.  B = 40 (8040 rows): no pack pass, and no 256x256 route on a layer of
    1024 output channels (the MFA conv, 3072 wide, always takes it).  The counts are the parent's launch log."""
    logs, struct = parity()["forwards"], P.cpu_weights("full", "f32s").struct
    packs = {B: P.launches_of(logs[f"full-f32s-auto-uniform-B{B}-n32000"]["launches"], {"split16_pack_kernel"}) for B in (40, 41)}
    assert packs == {40: 0, 41: 4}
    _, steps = P.read_plan(struct, 41, 201)
    assert [(s.name, s.reads[0].buf, s.writes[0].buf) for s in steps if s.route == "pack"] == \
        [("stem.pack", "feats", "xs"), ("b0.tdnn2.pack", "r", "rs"), ("b1.tdnn2.pack", "r", "rs"), ("b2.tdnn2.pack", "r", "rs")]
    stem = next(s for s in steps if s.name == "stem")
    assert [(w.buf, w.form) for w in stem.writes] == [("x0s", "split")] and not any(r.buf == "x0" for s in steps for r in s.reads)
    _, steps = P.read_plan(struct, 40, 201)
    assert not [s for s in steps if s.route == "pack"]
    assert [s.name for s in steps if s.route.startswith("split256")] == ["mfa"]
    t256 = {"conv_gemm_f16_t256_kernel", "conv_gemm_f16_w4_kernel"}
    assert P.launches_of(logs["full-f32s-auto-uniform-B40-n32000"]["launches"], t256) == 1
