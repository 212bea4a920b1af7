"""Guard bands around the buffers a test hands to libsd_hip.so.

`guarded(nbytes, fill, device)` is ONE uint8 allocation laid out as

    [ front guard | payload: exactly nbytes, 256-byte aligned | back guard ]

Both guards hold the byte 0xFF.  0xFFFFFFFF is a NaN as f32, 0xFFFF a NaN as f16 and -1 as an index, so a guard byte that a
kernel READS into arithmetic shows up as NaN in a result, and a guard byte that a kernel WRITES shows up in
`assert_guards_intact()` (an exact byte compare that names the first changed offset relative to the payload: negative in
front of it, >= nbytes behind it).  A guard is 4 MiB: more than one 256-row tile of the widest activation (256 x 3072 x 4 B
= 3 MiB), so that an overshoot stays inside memory the test owns.  The payload is pre-filled with a poison byte the test
chooses; POISONS are neutral for different kinds of bug: 0xFF (NaN in every float type), 0x7B (f32 1.3e36, f16 61280:
finite and large, survives fmaxf, ReLU and NaN-dropping clamps) and 0x00.

Imported by the tests (not a fixture file); works on the CPU too, where the self-test of tests/test_buffer_rules.py runs.
"""
import itertools
import weakref

import torch

GUARD_BYTES = 4 << 20
GUARD_BYTE = 0xFF
POISONS = (0xFF, 0x7B, 0x00)


class GuardError(AssertionError):
    pass


def _first_changed(region: torch.Tensor, byte: int):
    bad = region != byte
    if not bool(bad.any()):
        return None
    return int(torch.nonzero(bad.reshape(-1))[0, 0])


_LIVE = weakref.WeakSet()          # every Guarded that still exists: tests/helpers/captured.py snapshots and restores their payloads
_SERIAL = itertools.count()


def live() -> list:
    """The guarded buffers that exist now, in the order they were made."""
    return sorted(_LIVE, key=lambda g: g.serial)


class Guarded:
    def __init__(self, nbytes: int, fill: int, device, guard: int = GUARD_BYTES, name: str = ""):
        self.nbytes, self.name, self.guard = int(nbytes), name, int(guard)
        self.serial = next(_SERIAL)
        _LIVE.add(self)
        self.raw = torch.full((2 * guard + 256 + self.nbytes,), GUARD_BYTE, dtype=torch.uint8, device=device)
        self.off = guard + (-(self.raw.data_ptr() + guard)) % 256
        self.payload = self.raw[self.off:self.off + self.nbytes]
        self.payload.fill_(fill)

    @property
    def ptr(self) -> int:
        return self.raw.data_ptr() + self.off

    def view(self, dtype, *shape) -> torch.Tensor:
        """The whole payload as `dtype` (its element count must fit exactly), optionally reshaped."""
        t = self.payload.view(dtype)
        return t.view(*shape) if shape else t

    def put(self, t: torch.Tensor) -> "Guarded":
        """Copy the bytes of `t` (exactly nbytes of them) into the payload."""
        src = t.detach().contiguous().reshape(-1).view(torch.uint8)
        if src.numel() != self.nbytes:
            raise ValueError(f"{self.name}: tensor has {src.numel()} bytes, payload {self.nbytes}")
        self.payload.copy_(src.to(self.raw.device))
        return self

    def first_guard_change(self):
        """Offset, relative to the payload, of the first guard byte that is no longer 0xFF (None: both guards intact)."""
        i = _first_changed(self.raw[:self.off], GUARD_BYTE)
        if i is not None:
            return i - self.off
        i = _first_changed(self.raw[self.off + self.nbytes:], GUARD_BYTE)
        return None if i is None else self.nbytes + i

    def assert_guards_intact(self) -> None:
        at = self.first_guard_change()
        if at is not None:
            where = "front guard" if at < 0 else "back guard"
            raise GuardError(f"{self.name or 'buffer'} ({self.nbytes} bytes): {where} written, first changed byte at offset {at} "
                             f"relative to the payload")


def guarded(nbytes: int, fill: int, device, name: str = "") -> Guarded:
    return Guarded(nbytes, fill, device, name=name)


def guarded_from(t: torch.Tensor, device, name: str = "") -> Guarded:
    """A guarded buffer holding exactly the bytes of `t`: its last element is the payload's last."""
    return Guarded(t.numel() * t.element_size(), 0, device, name=name).put(t)


def assert_guards_intact(*bufs: Guarded) -> None:
    for b in bufs:
        b.assert_guards_intact()


def assert_columns_keep(mat: torch.Tensor, lo: int, hi: int, byte: int, name: str = "") -> None:
    """`mat` [rows, ld] is a matrix whose columns [lo, hi) an operator may write: every byte of every other column must still be
    `byte`.  Reports the first changed (row, column)."""
    rows, ld = mat.shape
    es = mat.element_size()
    b = mat.contiguous().view(torch.uint8).view(rows, ld * es)
    for c0, c1 in ((0, lo), (hi, ld)):
        if c1 <= c0:
            continue
        i = _first_changed(b[:, c0 * es:c1 * es], byte)
        if i is not None:
            w = (c1 - c0) * es
            raise GuardError(f"{name or 'matrix'}: neighbour of output columns [{lo}, {hi}) written at row {i // w}, column {c0 + (i % w) // es}")
