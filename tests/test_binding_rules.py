"""No-GPU checks of the Python binding's three shared pieces: the one checked launch (`ops.launch`), the grow-only
`ops.Workspace`, and the source rules that keep the wrappers on them.  The launch is run against a stand-in library object, so nothing
here needs a device."""
import re
import types

import pytest
import torch

from speech_diarization_amd import _native as N
from speech_diarization_amd import engine, ops


class StandInLib:
    """Records every entry call and returns `status`; `sd_last_error` is what `N.check` reads for its message."""

    def __init__(self, status=0):
        self.status, self.calls = status, []

    def sd_last_error(self):
        return b"stand-in refusal"

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return self.status
        return entry


@pytest.fixture
def stand_in(monkeypatch):
    """-> make(status): `ops.launch` then calls a StandInLib; the stream lookup, the one replaceable function, answers 0x5EED.  `on` is an
    object whose device index is -1: `torch.cuda.device` documents a negative index as a no-op, so no GPU is asked for."""
    def make(status=0):
        lib = StandInLib(status)
        monkeypatch.setattr(N, "load", lambda: lib)
        monkeypatch.setattr(ops, "_current_stream", lambda index: 0x5EED)
        return lib
    return make


ON = types.SimpleNamespace(device=types.SimpleNamespace(index=-1))


def test_launch_appends_the_stream_as_the_last_argument(stand_in):
    lib = stand_in(0)
    assert ops.launch("sd_seg_mean_f32", ON, 1, 2.5, None) is None
    (name, args), = lib.calls
    assert name == "sd_seg_mean_f32" and args[:-1] == (1, 2.5, None)
    assert args[-1].value == 0x5EED                                     # a c_void_p, as every prototype's last argument


def test_launch_names_the_entry_it_called_in_the_error(stand_in):
    stand_in(-2)
    for name in ("sd_hdb_core_f32", "sd_ecapa_forward_f32", "sd_fbank_lens_f32"):
        with pytest.raises(N.SdError, match=rf"^{name} failed \(status -2\): stand-in refusal$"):
            ops.launch(name, ON, 7)


def test_launch_refuses_a_name_that_is_in_no_table(stand_in):
    lib = stand_in(0)
    tables = [getattr(N, k) for k in dir(N) if k.endswith("PROTOTYPES")]
    assert len(tables) == 6 and ops._ENTRIES == {name for t in tables for name in t}
    for name in ("sd_ecapa_forward_f32s", "sd_no_such_entry", "check"):
        with pytest.raises(ValueError, match="none of the prototype tables"):
            ops.launch(name, ON)
    assert lib.calls == []


def test_an_f32s_engine_reports_the_entry_it_calls():
    """"f32s" and "f32ns" are packings of the weights on the f32 schedule: their forward is sd_ecapa_forward_f32, and that is the name an
    error carries (an engine cannot be constructed without a GPU, so: the function the constructor takes the names from, and the source)."""
    for precision in ("f32", "f32s", "f32ns"):
        assert engine.forward_entries(precision) == ("sd_ecapa_forward_f32", "sd_ecapa_forward_lens_f32")
    assert engine.forward_entries("f16") == ("sd_ecapa_forward_f16", "sd_ecapa_forward_lens_f16")
    assert all(name in N.PROTOTYPES for p in ("f32", "f16", "f32s", "f32ns") for name in engine.forward_entries(p))
    src = open(engine.__file__).read()
    assert "self._forward, self._forward_lens = forward_entries(precision)" in src
    assert "ops.launch(self._forward," in src and "ops.launch(self._forward_lens," in src
    assert not re.search(r"sd_ecapa_forward_\w*\{", src)                # no name is put together from the precision string


def test_workspace_grows_only_and_keeps_its_storage():
    ws = ops.Workspace("cpu")
    assert ws.take(0).numel() == 16 and ws.take(0).dtype == torch.uint8
    first = ws.take(16)
    assert first.data_ptr() == ws.take(1).data_ptr() == ws.take(16).data_ptr()
    big = ws.take(1000)
    assert big.numel() >= 1000 and big.data_ptr() != first.data_ptr()
    for need in (1000, 999, 17, 0):                                     # the need falls: nothing moves, nothing shrinks
        again = ws.take(need)
        assert again.data_ptr() == big.data_ptr() and again.numel() == big.numel()
    assert ws.take(1001).numel() >= 1001


def test_workspace_argument_forms():
    """`ws=`: a Workspace is taken from, a tensor that is large enough is used as it is, one that is too small or None gives a fresh one."""
    keep = ops.Workspace("cpu")
    assert ops._workspace(keep, 100, "cpu") is keep.buf and keep.buf.numel() == 100
    t = torch.empty(64, dtype=torch.float32)                             # 256 bytes
    assert ops._workspace(t, 256, "cpu") is t
    fresh = ops._workspace(t, 257, "cpu")
    assert fresh is not t and fresh.numel() == 257 and fresh.dtype == torch.uint8
    assert ops._workspace(None, 0, "cpu").numel() == 16


def _code_lines(path):
    return [(i, line) for i, line in enumerate(open(path).read().splitlines(), 1) if not line.lstrip().startswith("#")]


def test_no_call_site_types_an_entry_name_twice():
    """Outside `ops.launch`: no line of ops.py or engine.py calls an sd_ entry directly and also passes an entry's name as a string, and
    `N.check(` is left to the launch helper alone."""
    for mod in (ops, engine):
        lines = _code_lines(mod.__file__)
        both = [(i, line) for i, line in lines if re.search(r"\.sd_\w+\(", line) and re.search(r"[\"']sd_\w+[\"']", line)]
        assert not both, (mod.__name__, both)
        checks = [i for i, line in lines if "N.check(" in line]
        assert len(checks) == (1 if mod is ops else 0), (mod.__name__, checks)
    src = open(ops.__file__).read()
    body = src[src.index("def launch("):src.index("class Workspace")]
    assert "N.check(getattr(N.load(), name)(*args, _stream(on)), name)" in body
    assert src.count("torch.cuda.current_stream(") == 1                # the replaceable lookup, `ops._current_stream`
    assert open(engine.__file__).read().count("current_stream") == 0


def test_no_operator_class_asks_for_a_workspace_size():
    from speech_diarization_amd import ahc_gpu, cluster_gpu, device_rows, diag_gpu, hdbscan_gpu
    for mod, cls in ((cluster_gpu, "DeviceOperator"), (ahc_gpu, "DeviceSums"), (hdbscan_gpu, "DeviceRows"), (diag_gpu, "DeviceDiag")):
        src = open(mod.__file__).read()
        assert "_workspace_bytes" not in src and "torch.uint8" not in src, mod.__name__
        assert issubclass(getattr(mod, cls), device_rows.DeviceRoute)
    assert "_workspace_bytes" not in open(device_rows.__file__).read()
