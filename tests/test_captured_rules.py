"""No-GPU checks behind tests/test_gpu_captured.py: every entry of every header under include/ that takes an `sd_stream_t` has a
captured case, and the capture-and-replay helper (tests/helpers/captured.py) does what it says, shown with a stub launch and a stub
graph on CPU buffers."""
import importlib.util
import os
import re
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import captured as CAP  # noqa: E402
import guarded as G  # noqa: E402

INCLUDE = os.path.join(HERE, "..", "include")

# entry -> why it has no captured case.  Entries without a stream (size queries, sd_profile_read, plan creation) never enter the rule.
EXEMPT = {}


def launching_entries():
    """{entry: header} for every function, in any header, whose parameter list names sd_stream_t (comments stripped)."""
    found = {}
    for name in sorted(os.listdir(INCLUDE)):
        if not name.endswith(".h"):
            continue
        text = open(os.path.join(INCLUDE, name)).read()
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        text = re.sub(r"//[^\n]*", "", text)
        for m in re.finditer(r"\b(sd_[a-z0-9_]+)\s*\(([^;{}()]*)\)\s*;", text):
            if re.search(r"\bsd_stream_t\b", m.group(2)):
                found[m.group(1)] = name
    return found


def _gpu_module():
    spec = importlib.util.spec_from_file_location("sd_test_gpu_captured", os.path.join(HERE, "test_gpu_captured.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_every_launching_entry_of_every_header_has_a_captured_case():
    entries = launching_entries()
    headers = {h for h in os.listdir(INCLUDE) if h.endswith(".h")}
    assert set(entries.values()) == headers - {"sd_hip_trace.h"}, sorted(set(entries.values()))        # the launch log launches nothing
    assert len(entries) >= 60 and "sd_ecapa_forward_packed_f32" in entries and "sd_turns_grouped" in entries
    assert not {"sd_fbank_plan_create", "sd_profile_read", "sd_ecapa_workspace_bytes"} & set(entries)
    cases = _gpu_module().CAPTURED
    assert all(reason.strip() for reason in EXEMPT.values()) and not set(EXEMPT) & set(cases) and not set(EXEMPT) - set(entries)
    assert not set(cases) - set(entries), f"CAPTURED names what no header declares: {sorted(set(cases) - set(entries))}"
    missing = sorted(set(entries) - set(cases) - set(EXEMPT))
    assert not missing, f"no captured case in tests/test_gpu_captured.py for {missing}"
    assert all(len(v) > 0 for v in cases.values())
    for entry, lst in cases.items():
        assert len({cid for cid, _ in lst}) == len(lst), entry
    print(f"{len(entries)} launching entries in {len(set(entries.values()))} headers, {sum(len(v) for v in cases.values())} captured cases, "
          f"{len(EXEMPT)} exempt")


def test_the_four_memset_entries_have_a_case_that_leaves_the_word_non_zero():
    cases = _gpu_module().CAPTURED
    assert "n129-bad-set" in dict(cases["sd_ahc_nearest_grouped_f32"])
    assert "n129-d190-ld192" in dict(cases["sd_ahc_merge_f32"])                       # merges at the median score: several pairs
    for entry in ("sd_hdb_core_grouped_f32", "sd_hdb_outgoing_grouped_f32"):         # the body runs its broken promises when n > 1
        assert any(cid.startswith("n129-") for cid, _ in cases[entry])


# ------------------------------------------------------------------ the helper, with a stub launch and a stub graph

class StubGraph:
    def __init__(self, nodes):
        self.nodes, self.replays = nodes, 0

    def replay(self):
        self.replays += 1
        for node in self.nodes:
            node()


class StubBackend:
    """Capture runs the thunk with `self.recording` set: a well-behaved stub launch appends its work to the graph instead of doing it;
    a stray one does it at once, as a kernel issued on stream 0 would."""

    def __init__(self):
        self.recording, self.graphs, self.syncs = None, [], 0

    def synchronize(self):
        self.syncs += 1

    def capture(self, thunk):
        self.recording = []
        try:
            status = thunk()
        finally:
            nodes, self.recording = self.recording, None
        self.graphs.append(StubGraph(nodes))
        return self.graphs[-1], status


def _add_one(be, src, dst, stray=None, seen=None):
    """A stub entry: dst = src + 1 as a graph node (eagerly outside a capture); `stray`: a buffer it also writes at once, captured or not."""
    def work():
        if seen is not None:
            seen.append((bytes(src.payload.tolist()), bytes(dst.payload.tolist())))
        dst.payload.copy_(src.payload + 1)
    if stray is not None:
        stray.payload.fill_(0x11)
    if be.recording is not None:
        be.recording.append(work)
    else:
        work()
    return 0


def test_the_snapshot_is_restored_before_each_replay():
    be, seen = StubBackend(), []
    with CAP.replaying("sd_stub", backend=be) as mode:
        src = G.guarded(8, 0x00, "cpu", "src").put(torch.arange(8, dtype=torch.uint8))
        dst, other = G.guarded(8, 0x7B, "cpu", "dst"), G.guarded(8, 0x7B, "cpu", "other")
        assert CAP.route("sd_stub", lambda: _add_one(be, src, dst, stray=other, seen=seen)) == 0
    assert mode.launches == 1 and be.graphs[0].replays == 2 and be.syncs >= 4
    # every replay saw the inputs valid and the output poisoned again, and the stray write of the capture is gone
    assert seen == [(bytes(range(8)), bytes([0x7B] * 8))] * 2
    assert dst.payload.tolist() == list(range(1, 9)) and other.payload.tolist() == [0x7B] * 8
    assert list(mode.records[0]) == [(1, "src"), (2, "dst"), (3, "other")]
    # the same launch eagerly leaves the same record but for the buffer the stray write reached: the comparison can fail
    with CAP.observing("sd_stub", backend=be) as eager:
        src = G.guarded(8, 0x00, "cpu", "src").put(torch.arange(8, dtype=torch.uint8))
        dst, other = G.guarded(8, 0x7B, "cpu", "dst"), G.guarded(8, 0x7B, "cpu", "other")
        CAP.route("sd_stub", lambda: _add_one(be, src, dst, stray=other))
    with pytest.raises(AssertionError, match=r"replayed bytes differ from the eager ones in \[\(3, 'other'\)\]"):
        CAP.same_records(eager.records, mode.records, "sd_stub")
    eager.records[0].pop((3, "other")), mode.records[0].pop((3, "other"))
    CAP.same_records(eager.records, mode.records, "sd_stub")


def test_a_word_left_behind_by_the_first_replay_fails_the_second():
    """A counter the entry adds to without resetting it, kept OUTSIDE the guarded buffers (device state of the library): replay 2 differs."""
    be, state = StubBackend(), [0]
    with CAP.replaying("sd_stub", backend=be):
        out = G.guarded(1, 0x7B, "cpu", "count")

        def entry():
            def work():
                state[0] += 1
                out.payload.fill_(state[0])
            be.recording.append(work)
            return 0
        with pytest.raises(AssertionError, match="the second replay differs from the first in count"):
            CAP.route("sd_stub", entry)


def test_a_launch_of_a_different_entry_passes_through_and_a_refusal_is_returned_unchanged():
    be = StubBackend()
    with CAP.replaying("sd_stub", backend=be) as mode:
        src = G.guarded(8, 0x00, "cpu", "src").put(torch.arange(8, dtype=torch.uint8))
        dst = G.guarded(8, 0x7B, "cpu", "dst")
        assert CAP.route("sd_other", lambda: _add_one(be, src, dst)) == 0
        assert not be.graphs and dst.payload.tolist() == list(range(1, 9))            # ran eagerly, at once
        assert CAP.route("sd_stub", lambda: -3) == -3                                  # refused: captured, never replayed
    assert (mode.launches, mode.refused, mode.passed_through) == (0, 1, 1) and be.graphs[0].replays == 0 and not mode.records
    assert CAP._ACTIVE is None
    assert CAP.route("sd_stub", lambda: 7) == 7                                        # no scope: the thunk, nothing else


def test_a_failed_capture_raises_once_with_the_status_and_the_error_text():
    class Refusing(StubBackend):
        def capture(self, thunk):
            thunk()
            raise RuntimeError("operation not permitted when stream is capturing")
    be = Refusing()
    with CAP.replaying("sd_stub", backend=be):
        with pytest.raises(CAP.CaptureError, match=r"sd_stub: capture failed: status None, sd_last_error .*operation not permitted"):
            CAP.route("sd_stub", lambda: 0)
    assert be.syncs >= 2
    with CAP.replaying("sd_stub", backend=StubBackend()):
        with pytest.raises(CAP.CaptureError, match="HIP refused an operation under capture: status -4"):
            CAP.route("sd_stub", lambda: CAP.SD_ERR_HIP)
    assert CAP._ACTIVE is None
