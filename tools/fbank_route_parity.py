#!/usr/bin/env python3
"""Two builds of libsd_hip.so give the same fbank: for a fixed list of calls of the four fbank entries, the status code, the refusal
text (without the entry name in front), the launch log and the SHA-256 of the whole output buffer (pre-filled, so untouched words count).

    python tools/fbank_route_parity.py --record FILE                 one library, one process (an A/B build: SD_EXPERIMENT=1 SD_HIP_LIB=...)
    python tools/fbank_route_parity.py --compare A B [--out FILE]    no GPU: the two records entry by entry; exit status 1 if they differ

The calls: both 16 kHz front ends, B in {1, 3}, n on both sides of every route rule (1, 3, 4, 201, 202, 640, 801, 4 959, 5 120, 32 100,
32 102, 35 003, 100 000), mean_norm 0 / 1, ld_out above n_mels, windows past both ends of the signal, relative lengths including 0 and
1; packed spans on both routes, on one, and over a signal of four samples; the generic plan at 8 and 44.1 kHz; and the refusals (null
pointers, B -1 / 0 on the uniform and the packed entry, a short or misaligned workspace, a short ld_out, packed spans on a reflect or
generic plan).  No call of the list passes a pointer the entry would follow after accepting it wrongly: every refused call is refused
before anything is launched."""
import argparse
import ctypes as C
import hashlib
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LENGTHS = (1, 3, 4, 201, 202, 640, 801, 4959, 5120, 32100, 32102, 35003, 100000)


def record(path):
    import numpy as np
    import torch

    from speech_diarization_amd import _native as N
    from speech_diarization_amd.features import FbankPlan
    lib = N.load()
    dev = torch.device("cuda", 0)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    rng = np.random.RandomState(0)
    signal = (rng.randn(300000) * 0.1).astype(np.float32)
    signal[1000:3000] *= 1e-3
    sig = torch.from_numpy(signal).to(dev)
    entries = []

    def ptr(t, null=False):
        return None if null or t is None else t.data_ptr()

    def run(name, fn, out):
        """fn() -> status, under the launch log; the record of the call"""
        N.launch_log_enable(True)
        try:
            status = int(fn())
            torch.cuda.synchronize()
            log = N.launch_log_read()
        finally:
            N.launch_log_enable(False)
        msg = re.sub(r"^sd_fbank_[a-z0-9_]+: ", "", N.last_error()) if status else ""
        digest = hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest() if out is not None else None
        entries.append({"call": name, "status": status, "refusal": msg, "launches": log, "sha256": digest})

    def buffers(plan, B, n, ld_out):
        T = max(int(lib.sd_fbank_num_frames(plan.handle, n)), 1)
        out = torch.full((max(B, 1), T, ld_out), 7.0, dtype=torch.float32, device=dev)
        need = int(lib.sd_fbank_workspace_bytes(plan.handle, max(B, 1), n))
        ws = torch.zeros((max(need, 256) + 64,), dtype=torch.uint8, device=dev)
        return out, ws, need

    def uniform(plan, tag, B, n, mean_norm, ld_out=None, **bad):
        ld_out = plan.n_mels if ld_out is None else ld_out
        out, ws, need = buffers(plan, B, n, max(ld_out, plan.n_mels))
        wav = sig[: max(B, 1) * n].contiguous() if n else sig[:4]
        run(f"f32 {tag} B={B} n={n} mean_norm={mean_norm} ld_out={ld_out} {sorted(bad)}",
            lambda: lib.sd_fbank_f32(None if "no_plan" in bad else plan.handle, ptr(wav, "no_wav" in bad), B, n, mean_norm, ptr(out, "no_out" in bad), ld_out,
                                     None if "no_ws" in bad else ws.data_ptr() + (4 if "misaligned" in bad else 0), need - 1 if "short" in bad else need + 8, stream), out)

    plans = {"speechbrain": FbankPlan("speechbrain"), "torchaudio": FbankPlan("torchaudio")}
    for tag, plan in plans.items():
        for B in (1, 3):
            for n in LENGTHS:
                for mean_norm in (0, 1):
                    uniform(plan, tag, B, n, mean_norm)
        uniform(plan, tag, 3, 640, 1, ld_out=96)
        uniform(plan, tag, 3, 32102, 1, ld_out=96)
        # windows whose starts reach past both ends of the signal; relative lengths including 0 and 1
        for n in (640, 32102):
            n_total, B = 50000, 5
            starts = torch.tensor([-n // 2, 0, 777, n_total - n // 3, n_total - 1], dtype=torch.int64, device=dev)
            out, ws, need = buffers(plan, B, n, plan.n_mels)
            run(f"windows {tag} n={n}", lambda: lib.sd_fbank_windows_f32(plan.handle, sig.data_ptr(), n_total, starts.data_ptr(), B, n, 1, out.data_ptr(), plan.n_mels,
                                                                          ws.data_ptr(), need, stream), out)
            rel = torch.tensor([0.0, 1.0, 0.5, 0.013, 0.999], dtype=torch.float32, device=dev)
            out, ws, need = buffers(plan, B, n, plan.n_mels)
            run(f"lens {tag} n={n}", lambda: lib.sd_fbank_lens_f32(plan.handle, sig.data_ptr(), B, n, rel.data_ptr(), out.data_ptr(), plan.n_mels, ws.data_ptr(), need,
                                                                    stream), out)
        out, ws, need = buffers(plan, 2, 640, plan.n_mels)
        two = torch.tensor([0, -100], dtype=torch.int64, device=dev)
        run(f"windows {tag} n_total=3", lambda: lib.sd_fbank_windows_f32(plan.handle, sig.data_ptr(), 3, two.data_ptr(), 2, 640, 1, out.data_ptr(), plan.n_mels,
                                                                          ws.data_ptr(), need, stream), out)

    def packed(plan, tag, n_total, spans, n_max=None, **bad):
        B = len(spans)
        starts = torch.tensor([s for s, _ in spans], dtype=torch.int64, device=dev)
        lens = torch.tensor([ln for _, ln in spans], dtype=torch.int32, device=dev)
        frames = [1 + ln // 160 for _, ln in spans]
        frame_start = torch.tensor([sum(frames[:i]) for i in range(B)], dtype=torch.int32, device=dev)
        M = sum(frames)
        n_max = max(ln for _, ln in spans) if n_max is None else n_max
        out = torch.full((M, 80), 7.0, dtype=torch.float32, device=dev)
        need = int(lib.sd_fbank_packed_workspace_bytes(plan.handle, B, M, n_max))
        ws = torch.zeros((need + 64,), dtype=torch.uint8, device=dev)
        run(f"packed {tag} n_total={n_total} spans={spans} {sorted(bad)}",
            lambda: lib.sd_fbank_packed_f32(plan.handle, sig.data_ptr(), n_total, ptr(starts, "starts" in bad), ptr(lens, "lens" in bad), ptr(frame_start, "frame_start" in bad),
                                            -1 if "negative" in bad else 0 if "empty" in bad else B, M, n_max, ptr(out, "out" in bad), 79 if "ld_out" in bad else 80,
                                            None if "ws" in bad else ws.data_ptr() + (4 if "misaligned" in bad else 0), need - 1 if "short" in bad else need + 8, stream), out)

    sb = plans["speechbrain"]
    mixed = [(0, 640), (100, 32100), (117, 32102), (4000, 9600), (90000 - 48000, 48000), (90000 - 801, 801)]
    short = [(0, 640), (4000, 9600), (90000 - 801, 801)]
    packed(sb, "mixed", 90000, mixed)
    packed(sb, "one route", 90000, short)
    packed(sb, "folded only", 90000, [(5, 32102), (40000, 48000)])
    packed(sb, "four samples", 4, [(0, 4)])
    for bad in ("starts", "lens", "frame_start", "out", "ws", "misaligned", "short", "ld_out", "negative"):
        packed(sb, "refused", 90000, short, **{bad: True})
    packed(sb, "refused n_total", 3, [(0, 3)])
    packed(sb, "no spans", 90000, short, empty=True)
    packed(plans["torchaudio"], "reflect plan", 90000, short)

    # the generic plan at 8 kHz and 44.1 kHz
    for sr in (8000, 44100):
        plan = FbankPlan("torchaudio", sr=sr)
        tag = f"generic {sr}"
        for B, n in ((1, sr // 2), (3, sr + 7)):
            for mean_norm in (0, 1):
                uniform(plan, tag, B, n, mean_norm)
        uniform(plan, tag, 1, plan.n_fft // 2, 1)            # reflect padding needs one sample more
        uniform(plan, tag, 2, sr // 2, 1, short=True)
        uniform(plan, tag, 2, sr // 2, 1, misaligned=True)
        uniform(plan, tag, 2, sr // 2, 1, ld_out=79)
        packed(plan, tag, 90000, short)

    # the refusal grid of the uniform entries
    for tag, plan in plans.items():
        for bad in ("no_plan", "no_wav", "no_out", "no_ws", "short"):
            uniform(plan, tag, 2, 640, 1, **{bad: True})
        uniform(plan, tag, 2, 640, 1, ld_out=79)
        uniform(plan, tag, -1, 640, 1)
        uniform(plan, tag, 0, 640, 1)
        uniform(plan, tag, 2, 0, 1)
        out, ws, need = buffers(plan, 2, 640, plan.n_mels)
        run(f"windows {tag} null starts", lambda: lib.sd_fbank_windows_f32(plan.handle, sig.data_ptr(), 5000, None, 2, 640, 1, out.data_ptr(), plan.n_mels, ws.data_ptr(),
                                                                            need, stream), out)
        run(f"windows {tag} n_total=0", lambda: lib.sd_fbank_windows_f32(plan.handle, sig.data_ptr(), 0, None, 2, 640, 1, out.data_ptr(), plan.n_mels, ws.data_ptr(),
                                                                          need, stream), out)
        run(f"lens {tag} short ws", lambda: lib.sd_fbank_lens_f32(plan.handle, sig.data_ptr(), 2, 640, None, out.data_ptr(), plan.n_mels, ws.data_ptr(), need - 1, stream), out)

    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        json.dump({"library": os.path.basename(os.environ.get("SD_HIP_LIB") or str(N.LIB_PATH)), "device": torch.cuda.get_device_name(0), "entries": entries}, fh, indent=1)
    refused = sum(1 for e in entries if e["status"])
    print(f"{len(entries)} calls, {refused} refused -> {path}")


def compare(path_a, path_b, out):
    a, b = json.load(open(path_a)), json.load(open(path_b))
    differ = [(x, y) for x, y in zip(a["entries"], b["entries"]) if x != y]
    same_length = len(a["entries"]) == len(b["entries"])
    labels = sorted({lb for e in a["entries"] for lb in e["launches"]})
    result = {"a": os.path.basename(a["library"]), "b": os.path.basename(b["library"]), "device": a["device"], "calls": len(a["entries"]), "refused": sum(1 for e in a["entries"] if e["status"]),
              "labels_seen": labels, "equal": same_length and not differ, "differ": differ, "entries": a["entries"]}
    if out:
        with open(out, "w") as fh:
            json.dump(result, fh, indent=1)
    print(json.dumps({k: result[k] for k in ("a", "b", "calls", "refused", "equal")}), f"{len(differ)} differ")
    for x, y in differ[:10]:
        print("  ", x, "\n  ", y)
    return 0 if result["equal"] else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--record")
    ap.add_argument("--compare", nargs=2)
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.record:
        record(args.record)
    if args.compare:
        sys.exit(compare(args.compare[0], args.compare[1], args.out))
