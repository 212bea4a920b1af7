"""No-GPU checks of the fbank entries' check and route (csrc/sd_fbank_route.h): what an entry refuses and which
kernels it launches, with what geometry, is a pure function of the plan's facts and of a description of the call, so it is checked here
at every length and not only where a GPU test happens to launch.

tests/helpers/fbank_route_pure.cpp is the header alone in a plain C++ program with its own main, built here with the address and
undefined-behaviour sanitizers (nothing preloaded); it prints the route of the calls it is given.  The expected values are derived by
hand from the kernels' geometry (32-frame tiles, four per workgroup; 512-thread one-launch workgroups; a finalize pass of R = 320 / n_mels
row groups), not read off the code under test."""
import os
import re
import shutil
import subprocess

import pytest

from speech_diarization_amd import _native as N

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = N.PKG_DIR / "csrc"
GENERIC, ONE_LAUNCH, FOLDED = 1, 2, 4


@pytest.fixture(scope="module")
def pure(tmp_path_factory):
    cxx = shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    assert os.path.exists(cxx), "no clang++ on this machine"
    exe = tmp_path_factory.mktemp("fbank_route") / "fbank_route_pure"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", f"-I{CSRC}",
           f"-I{N.PKG_DIR.parent / 'include'}", os.path.join(HERE, "helpers", "fbank_route_pure.cpp"), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr

    def run(*calls):
        ran = subprocess.run([str(exe), *calls], capture_output=True, text=True)
        assert ran.returncode == 0 and not ran.stderr, (ran.returncode, ran.stderr[-2000:])
        return ran.stdout.splitlines()
    return run


def call(form="u", plan="sb", n_mels=80, on=1, B=1, n=1, n_total=-1, M=0, ld_out=None, ws=-1, nulls=""):
    spec = f"{form}:{plan}:{n_mels}:{on}:{B}:{n}:{n_total}:{M}:{n_mels if ld_out is None else ld_out}:{ws}"
    return spec + (":" + nulls if nulls else "")


def parse(line):
    if " why=" in line:
        status, why = line.split(" why=", 1)
        return {"status": int(status.split("=")[1]), "why": why}
    out = {}
    for item in line.split():
        k, v = item.split("=")
        out[k] = tuple(int(x) for x in v.split("/")) if "/" in v else int(v)
    return out


def route(pure, **kw):
    (line,) = pure(call(**kw))
    r = parse(line)
    assert r["status"] == 0, r
    return r


NOT_LAUNCHED = (0, 0, 0)
FOLD = (512, 152576)             # threads and LDS bytes of a folded-DFT workgroup


# ------------------------------------------------------------------ the hand-derived table

def test_uniform_routes_equal_the_hand_derived_values(pure):
    r = route(pure, B=1, n=3)                                    # three samples behind `wav`: no 16-byte load, so the folded kernel's tile walk
    assert (r["kinds"], r["T"], r["flat"], r["tiles"], r["logmel"]) == (FOLDED, 1, 0, 1, (1, *FOLD))
    assert (r["R"], r["finalize"], r["fill"], r["utt16"], r["tile_table"]) == (1, (1, 128, 320), (1, 256, 0), NOT_LAUNCHED, NOT_LAUNCHED)
    r = route(pure, B=2, n=2)
    assert (r["kinds"], r["T"], r["utt16"]) == (ONE_LAUNCH, 1, (2, 512, 34644))
    assert r["fill"] == r["logmel"] == r["finalize"] == NOT_LAUNCHED
    r = route(pure, B=1, n=32100)
    assert (r["kinds"], r["T"], r["utt16"]) == (ONE_LAUNCH, 201, (1, 512, 163840))
    r = route(pure, B=1, n=32101)
    assert (r["kinds"], r["T"], r["flat"], r["tiles"], r["logmel"]) == (FOLDED, 201, 1, 7, (2, *FOLD))
    assert (r["R"], r["finalize"]) == (4, (1, 320, 1280))
    r = route(pure, B=3, n=100000)
    assert (r["kinds"], r["T"], r["flat"], r["tiles"], r["logmel"], r["fill"]) == (FOLDED, 626, 1, 59, (15, *FOLD), (1, 256, 0))
    r = route(pure, B=1, n=32101, n_mels=40)
    assert (r["kinds"], r["T"], r["R"], r["finalize"]) == (FOLDED, 201, 8, (1, 320, 1280))
    r = route(pure, B=1, n=32101, n_mels=23)
    assert (r["kinds"], r["T"], r["R"], r["finalize"]) == (FOLDED, 201, 13, (1, 320, 13 * 23 * 4))
    assert route(pure, form="w", B=5, n=640, n_total=3)["kinds"] == FOLDED          # windows over a signal of three samples
    assert route(pure, form="w", B=5, n=640, n_total=4)["kinds"] == ONE_LAUNCH
    # the reciprocals (ceil(2^32 / x)) and use_floor: 80 mels = 20 float4 per row; a dB plan with top_db >= 0 floors
    r = route(pure, B=1, n=32101)
    assert (r["inv_mels"], r["use_floor"]) == (-(-2**32 // 80), 1)
    r = route(pure, B=1, n=640)
    assert (r["inv_row"], r["use_floor"]) == (-(-2**32 // 20), 1)
    r = route(pure, plan="ta", n_mels=23, B=1, n=640)
    assert (r["inv_row"], r["use_floor"]) == (-(-2**32 // 23), 0)


SHAPES = [dict(B=1, n=3), dict(B=2, n=2), dict(B=1, n=32100), dict(B=1, n=32101), dict(B=3, n=100000), dict(B=1, n=32101, n_mels=40),
          dict(B=1, n=32101, n_mels=23), dict(form="w", B=5, n=640, n_total=3)]


def test_a_generic_plan_is_generic_and_the_switch_sends_everything_to_the_folded_kernel(pure):
    for shape in SHAPES:
        shape = dict(shape, n=max(shape["n"], 101))            # (reflect padding of 100 needs 101 samples)
        r = route(pure, **dict(shape, plan="g8"))
        assert r["kinds"] == GENERIC and r["utt16"] == r["logmel"] == r["fill"] == r["finalize"] == NOT_LAUNCHED
        assert r["T"] == 1 + shape["n"] // 80 and r["ws_need"] == r["uniform_ws"] >= 256
    for shape in SHAPES:
        r = route(pure, **dict(shape, on=0))
        assert r["kinds"] == FOLDED and r["utt16"] == NOT_LAUNCHED and r["logmel"][0] >= 1


# ------------------------------------------------------------------ packed spans

def test_packed_routes(pure):
    B, M = 6, 1000
    ws = (256, 256, 512)                     # max keys of 6 spans, offset of the 7-int tile table, both
    r = route(pure, form="p", B=B, n=9600, n_total=90000, M=M)
    assert (r["kinds"], r["n_cap"], r["utt16"][:2], r["logmel"], r["fill"], r["finalize"]) == (ONE_LAUNCH, 9600, (B, 512), NOT_LAUNCHED, NOT_LAUNCHED, NOT_LAUNCHED)
    assert r["utt16"][2] == 33024 + 4 * max(10000 + 10000 // 160 + 1, 61 * 81)
    r = route(pure, form="p", B=B, n=48000, n_total=90000, M=M)
    assert (r["kinds"], r["n_cap"], r["n_lo"], r["flat"], r["T"]) == (ONE_LAUNCH | FOLDED, 32100, 32100, 0, 301)
    assert r["utt16"] == (B, 512, 163840) and r["tile_table"] == (1, 1024, 0) and r["fill"] == (1, 256, 0)
    assert r["logmel"] == (-(-(M // 32 + B) // 4), *FOLD)
    assert (r["R"], r["finalize"]) == (4, (B, 320, 1280))       # not clamped to T: a span's workgroup clamps to its own
    assert (r["maxkey"], r["tile_off"], r["ws_need"]) == ws and r["packed_ws"] == ws[2]
    r = route(pure, form="p", B=B, n=48000, n_total=90000, M=M, on=0)
    assert (r["kinds"], r["n_cap"], r["n_lo"], r["utt16"]) == (FOLDED, 0, 0, NOT_LAUNCHED) and r["logmel"][0] == 10
    r = route(pure, form="p", B=B, n=9600, n_total=90000, M=M, on=0)
    assert (r["kinds"], r["n_lo"]) == (FOLDED, 0)
    # the workspace bytes are those of the two ABI functions
    assert N.LIB_PATH.exists(), "libsd_hip.so is not built"
    lib = N.load()
    for b in (1, 63, 64, 65, 1000):
        r = route(pure, form="p", B=b, n=48000, n_total=90000, M=M)
        want = (-(-4 * b // 256) + -(-4 * (b + 1) // 256)) * 256
        assert r["ws_need"] == r["packed_ws"] == want and r["uniform_ws"] == r["maxkey"] == -(-4 * b // 256) * 256
        assert int(lib.sd_fbank_packed_workspace_bytes(None, b, M, 48000)) == want and int(lib.sd_fbank_workspace_bytes(None, b, 640)) == r["maxkey"]


# ------------------------------------------------------------------ the dense sweep

def rule(B, n):
    """The uniform route of the speechbrain plan, restated: (kinds, T, flat, tiles, one-launch grid, folded grid, R, finalize threads,
    one-launch LDS bytes)."""
    T = 1 + n // 160
    if B * n >= 4 and n <= 32100:
        return (ONE_LAUNCH, T, 0, 0, B, 0, 0, 0, 16384 + 16384 + 256 + 4 * max(n + 400 + (n + 400) // 160 + 1, 81 * T))
    flat = int(T >= 32)
    tiles = -(-B * T // 32) if flat else B * -(-T // 32)
    R = min(320 // 80, T)
    return (FOLDED, T, flat, tiles, 0, -(-tiles // 4), R, -(-R * 80 // 64) * 64, 0)


def test_the_route_equals_the_python_statement_over_the_dense_sweep(pure):
    seen = set()
    for B in (1, 2, 3, 5):
        lines = pure(f"sweep:{B}")
        assert len(lines) == 40000
        for n, line in enumerate(lines, 1):
            got = tuple(int(x) for x in line.split())
            assert got == (B, n, *rule(B, n)), (B, n, got)
            seen.add((got[2], got[4]))
    assert seen == {(ONE_LAUNCH, 0), (FOLDED, 0), (FOLDED, 1)}


# ------------------------------------------------------------------ refusals: the entry's own name, the order of the entries

def test_refusals_name_the_entry_and_keep_their_order(pure):
    ARG, UNSUPPORTED = -1, -2                # SD_ERR_ARG, SD_ERR_UNSUPPORTED (include/sd_hip.h)
    cases = [
        (call(B=1, n=640, nulls="p"), ARG, "sd_fbank_f32: null plan"),
        (call(form="l", B=-1, n=640), ARG, "sd_fbank_lens_f32: B=-1 n=640"),
        (call(form="w", B=1, n=640, n_total=0, nulls="ps"), ARG, "sd_fbank_windows_f32: n_total=0"),        # before the null plan
        (call(form="w", B=1, n=640, n_total=9, nulls="ps"), ARG, "sd_fbank_windows_f32: null starts"),
        (call(form="w", B=1, n=640, n_total=9, nulls="p"), ARG, "sd_fbank_windows_f32: null plan"),
        (call(form="l", B=1, n=640, nulls="o"), ARG, "sd_fbank_lens_f32: null wav/out"),
        (call(B=1, n=640, ld_out=79), ARG, "sd_fbank_f32: ld_out=79 < n_mels=80"),
        (call(B=1, n=0), ARG, "sd_fbank_f32: empty waveform"),
        (call(plan="ta", B=1, n=200), ARG, "sd_fbank_f32: reflect padding of 200 needs more than 200 samples (got 200)"),
        (call(form="w", plan="ta", B=1, n=200, n_total=900), ARG, "sd_fbank_windows_f32: reflect padding of 200 needs more than 200 samples (got 200)"),
        (call(B=65, n=640, ws=256), ARG, "sd_fbank_f32: workspace too small (256 < 512)"),
        (call(B=1, n=640, nulls="k"), ARG, "sd_fbank_f32: workspace too small (256 < 256)"),
        (call(form="l", plan="g8", B=1, n=640, ws=0), ARG, "sd_fbank_lens_f32: workspace too small or misaligned"),
        (call(plan="g8", B=1, n=640, nulls="m"), ARG, "sd_fbank_f32: workspace too small or misaligned"),
        (call(plan="g8", B=1, n=100), ARG, "sd_fbank_f32: reflect padding of 100 needs more than 100 samples (got 100)"),
        (call(form="p", B=-1, n=640, n_total=900, M=5), ARG, "sd_fbank_packed_f32: B=-1"),
        (call(form="p", B=1, n=640, n_total=900, M=0), ARG, "sd_fbank_packed_f32: M=0 n_max=640"),
        (call(form="p", B=1, n=640, n_total=900, M=5, nulls="f"), ARG, "sd_fbank_packed_f32: null pointer"),
        (call(form="p", B=1, n=640, n_total=3, M=5), ARG, "sd_fbank_packed_f32: n_total=3 (at least 4 samples)"),
        (call(form="p", B=1, n=640, n_total=900, M=5, ld_out=8), ARG, "sd_fbank_packed_f32: ld_out=8 < n_mels=80"),
        (call(form="p", plan="ta", B=1, n=640, n_total=900, M=5), UNSUPPORTED, "sd_fbank_packed_f32: packed spans take the 25 ms / 10 ms plan with zero padding (speechbrain)"),
        (call(form="p", plan="g8", B=1, n=640, n_total=900, M=5), UNSUPPORTED, "sd_fbank_packed_f32: packed spans take the 25 ms / 10 ms plan with zero padding (speechbrain)"),
        (call(form="p", B=1, n=640, n_total=900, M=5, ws=511), ARG, "sd_fbank_packed_f32: workspace 511 < 512 bytes, or unaligned"),
        (call(form="p", B=1, n=640, n_total=900, M=5, nulls="m"), ARG, "sd_fbank_packed_f32: workspace 512 < 512 bytes, or unaligned"),
        (call(form="p", B=2**31 - 2, n=640, n_total=900, M=2**31 - 1, ws=2**40), ARG, "sd_fbank_packed_f32: grid too large"),
    ]
    got = [parse(line) for line in pure(*(c[0] for c in cases))]
    for (spec, status, why), g in zip(cases, got):
        assert g == {"status": status, "why": why}, (spec, g)
    # B = 0 is no work and no refusal, whatever else is null
    for spec in (call(B=0, n=640, nulls="wok"), call(form="p", B=0, n=640, n_total=0, M=0, nulls="wosf"), call(form="w", B=0, n=640, n_total=5, nulls="s")):
        (line,) = pure(spec)
        assert parse(line)["status"] == 0 and parse(line)["kinds"] == 0


# ------------------------------------------------------------------ one statement of each rule

def _code(text):
    return re.sub(r"//[^\n]*", "", text)


def test_each_fbank_rule_is_stated_once():
    files = {f.name: f.read_text() for f in sorted(CSRC.glob("sd_fbank*"))}
    assert set(files) == {"sd_fbank.hip", "sd_fbank_utt16.hip", "sd_fbank_generic.hip", "sd_fbank_internal.h", "sd_fbank_route.h"}
    code = {name: _code(text) for name, text in files.items()}
    where = lambda pattern: [name for name, text in code.items() for _ in re.finditer(pattern, text)]  # noqa: E731
    once = ["sd_fbank_route.h"]
    assert where(r"top_db >= 0") == once                                  # use_floor
    assert where(r"1 << 32") == once                                      # ceil(2^32 / x)
    assert where(r"B > 0 \? B : 0") == once and where(r"\+ 255\) & ~") == once      # the max-key bytes, rounded to 256
    assert where(r"SCRATCH_FLOATS \* 4 \+") == once and set(where(r"\bimg_words\(")) == set(once)     # the one-launch LDS formula
    assert where(r"<= \(size_t\)LDS_LIMIT") == once and where(r"U16_MAX_N = 32100\b") == once
    assert where(r"\b320 /") == once and where(r"\+ 63\) / 64|, 64\) \* 64") == once                # the finalize geometry
    for constant in ("NFFT", "HOP", "NFREQ", "MELP"):                      # the framing both kernel files used to repeat
        assert where(rf"constexpr int [^;]*\b{constant} = ") == once, constant
    assert where(r"unsigned short sd_bf16_bits\(") == ["sd_fbank_internal.h"] and where(r"0x7FFFu") == ["sd_fbank_internal.h"]
    assert where(r"\(v - \(double\)\(float\)") == ["sd_fbank_internal.h"]               # the hi / lo f16 split of a table value
    assert where(r"\bhipFree\(") == ["sd_fbank_internal.h"]                               # one function releases a plan's tables
    assert where(r'sd_experiment_env\("SD_FBANK_UTT"\)') == ["sd_fbank.hip"]
    # the route header is host-only C++: no HIP header, no environment, no launch, no label
    raw = files["sd_fbank_route.h"]
    assert re.findall(r'#include [<"]([^>"]+)[>"]', raw) == ["stddef.h", "stdio.h", "sd_hip.h"]
    assert not re.search(r"getenv|std::atomic|hipLaunch|hipGet|hipDevice|hipMalloc|<<<|_kernel", code["sd_fbank_route.h"])
    # the entries name themselves: no refusal text of another entry is left in the launch files
    assert not where(r'"sd_fbank_[a-z0-9_]*f32: ')
