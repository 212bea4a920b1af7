"""Capture and replay for raw-ABI launches: what an entry does as nodes of a hipGraph must be what it does as an eager call.

Every header under include/ promises, for every entry that takes an `sd_stream_t`, that the call is asynchronous on `stream`, never
allocates and never synchronises, so that it can be captured.  On the default stream none of that can fail a test.  Here a test runs
its own guarded helper (tests/helpers/guarded.py) a second time inside `with replaying(entry) as mode:`.  Every launch of `entry` --
through `speech_diarization_amd.ops.launch` or through `call` below, which tests/test_gpu_buffer_edges.py and the module tests use
for the raw ABI -- is then captured with `torch.cuda.graph` and replayed instead of running eagerly; launches of any other entry
pass through.  Per launch:

 1. synchronise; snapshot the payload bytes of every live guarded buffer (inputs hold their valid values, outputs and workspace
    their poison);
 2. capture the one call.  A non-zero status is returned unchanged, nothing is replayed (a refusal stays a refusal);
 3. restore the snapshot in place -- whatever executed eagerly during capture (a kernel issued on stream 0 instead of `stream`) is
    erased -- replay, synchronise;
 4. restore again, replay again, synchronise.  The caller reads the results of the SECOND replay, and every guarded buffer that is
    not a workspace must hold after it the bytes it held after the first, bit for bit: a counter, flag or key that a replay leaves
    behind and the next one relies on shows here.

Inputs are valid at every moment.  A capture that fails (HIP refuses an operation under capture, the entry reports SD_ERR_HIP, torch
raises at capture end) raises `CaptureError` with the entry's status, `sd_last_error` and the error text, after the capture context
is left and the device synchronised; nothing is tried again.

`observing(entry)` is the eager twin: launches run as they always do, and after each one the same record is taken, so that a test can
hold the replayed bytes against the eager ones (`mode.records`).  A record is {(serial since the scope began, buffer name): digest}
over the guarded buffers made inside the scope that are not workspaces (names "ws", "workspace", "scratch", "... ws": a workspace's
bytes after a call are not part of any entry's contract).

The graph machinery is a `backend` object so that the protocol can be tested on the CPU with a stub (tests/test_captured_rules.py)."""
import contextlib
import ctypes as C
import gc
import hashlib

import torch

import guarded as G

SD_ERR_HIP = -4


class CaptureError(AssertionError):
    pass


class TorchBackend:
    """`torch.cuda.graph` on the current device: capture on torch's capture stream (the binding's `_current_stream` and `call` below ask
    torch for the current stream inside it), error mode "global" so that an allocating or synchronising call inside the entry fails."""

    def synchronize(self):
        torch.cuda.synchronize()

    def capture(self, thunk):
        graph = torch.cuda.CUDAGraph()
        status = None
        with torch.cuda.graph(graph):
            status = thunk()
        return graph, status


class Mode:
    def __init__(self, entry, replay, backend):
        self.entry, self.replay, self.backend = entry, replay, backend
        self.first_serial = next(G._SERIAL)
        self.launches = 0          # launches of `entry` that returned 0 (replay mode: captured and replayed twice)
        self.refused = 0           # launches of `entry` that returned non-zero (returned unchanged)
        self.passed_through = 0    # launches of other entries
        self.records = []


_ACTIVE = None


def _is_workspace(name):
    n = (name or "").lower()
    return n in ("ws", "workspace", "scratch") or n.endswith(" ws")


def _record(mode):
    rec = {}
    for g in G.live():
        if g.serial > mode.first_serial and not _is_workspace(g.name):
            rec[(g.serial - mode.first_serial, g.name)] = hashlib.blake2b(g.payload.cpu().numpy().tobytes(), digest_size=16).hexdigest()
    return rec


def _last_error():
    from speech_diarization_amd import _native as N
    return N.last_error()


def _replayed(mode, thunk):
    be = mode.backend
    gc.collect()
    be.synchronize()
    bufs = G.live()
    snap = [g.payload.clone() for g in bufs]

    def restore():
        for g, s in zip(bufs, snap):
            g.payload.copy_(s)
        be.synchronize()
    status, graph = None, None
    try:
        graph, status = be.capture(thunk)
    except Exception as e:                                   # torch raising inside or at the end of the capture
        be.synchronize()
        raise CaptureError(f"{mode.entry}: capture failed: status {status}, sd_last_error {_last_error()!r}: {type(e).__name__}: {e}") from e
    if status == SD_ERR_HIP:
        be.synchronize()
        raise CaptureError(f"{mode.entry}: HIP refused an operation under capture: status {status}, sd_last_error {_last_error()!r}")
    if status != 0:
        restore()
        mode.refused += 1
        return status
    restore()
    graph.replay()
    be.synchronize()
    outs = [g for g in bufs if not _is_workspace(g.name)]
    first = [g.payload.clone() for g in outs]
    restore()
    graph.replay()
    be.synchronize()
    for g, f in zip(outs, first):
        same = g.payload == f
        if not bool(same.all()):
            at = int(torch.nonzero(~same.reshape(-1))[0, 0])
            raise AssertionError(f"{mode.entry}: the second replay differs from the first in {g.name or 'buffer'} ({g.nbytes} bytes), first at byte {at}: "
                                 f"0x{int(f.reshape(-1)[at]):02X} after replay 1, 0x{int(g.payload.reshape(-1)[at]):02X} after replay 2")
    mode.launches += 1
    mode.records.append(_record(mode))
    return status


def route(name, thunk):
    """`thunk()` launches entry `name` on the current torch stream and returns its status: run it the way the active mode asks."""
    mode = _ACTIVE
    if mode is None:
        return thunk()
    if name != mode.entry:
        mode.passed_through += 1
        return thunk()
    if mode.replay:
        return _replayed(mode, thunk)
    status = thunk()
    if status != 0:
        mode.refused += 1
        return status
    gc.collect()                                             # the buffers alive at a record are those alive in the replayed run
    mode.backend.synchronize()
    mode.launches += 1
    mode.records.append(_record(mode))
    return status


def _arg(a):
    if isinstance(a, G.Guarded):
        return a.ptr
    if isinstance(a, torch.Tensor):
        return a.data_ptr()
    return a


def call(name, *args):
    """The raw entry `name` with `args` (guarded buffers and tensors as their pointers) and, last, the current torch stream -> status."""
    from speech_diarization_amd import _native as N

    def thunk():
        return getattr(N.load(), name)(*[_arg(a) for a in args], C.c_void_p(torch.cuda.current_stream().cuda_stream))
    return route(name, thunk)


@contextlib.contextmanager
def _mode(entry, replay, backend):
    global _ACTIVE
    from speech_diarization_amd import _native as N
    from speech_diarization_amd import ops
    assert _ACTIVE is None, "capture scopes do not nest"
    gc.collect()                                             # the same buffers are alive in the eager and in the replayed run
    gc.freeze()                                              # ... and the collections per launch walk only what the scope made
    mode = Mode(entry, replay, backend or TorchBackend())
    plain = ops.launch

    def launch(name, on, *args):
        def thunk():
            with torch.cuda.device(on.device.index):
                return getattr(N.load(), name)(*args, ops._stream(on))
        if name == entry:
            N.check(route(name, thunk), name)
        else:
            mode.passed_through += 1
            plain(name, on, *args)
    ops.launch = launch
    _ACTIVE = mode
    try:
        yield mode
    finally:
        _ACTIVE = None
        ops.launch = plain
        gc.unfreeze()


def replaying(entry, backend=None):
    return _mode(entry, True, backend)


def observing(entry, backend=None):
    return _mode(entry, False, backend)


def same_records(eager, replayed, entry):
    """Record for record and buffer for buffer, the replayed bytes are the eager ones."""
    assert len(eager) == len(replayed) > 0, f"{entry}: {len(eager)} eager launches, {len(replayed)} replayed"
    for i, (a, b) in enumerate(zip(eager, replayed)):
        assert sorted(a) == sorted(b), f"{entry}, launch {i}: buffers {sorted(a)} eager, {sorted(b)} replayed"
        differ = [k for k in a if a[k] != b[k]]
        assert not differ, f"{entry}, launch {i}: replayed bytes differ from the eager ones in {differ}"
    assert any(eager), f"{entry}: no launch had a guarded buffer to compare"     # (a launch on plain tensors, a reference, has none)
