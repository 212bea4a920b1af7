"""The kernel selections of the exact-f32 conv operator (`sd_set_tuning`), as one fixture shared by the GPU test modules, and the two
tile choices of the f16 / split16 operators (`f16_tiles`).

Imported, not a conftest: `from kernel_selection import conv_kernel` (with tests/helpers on sys.path) makes the fixture visible
to the importing module only."""
import pytest

CONV_KERNELS = ["auto", "split32", "tiles128", "tiles64", "rows80", "rows96", "rows112", "wide256"]

# the kernel a selection asks for, as the launch log names it (launch_log.py).  A pin is a request: a launch whose shape fails a side
# condition of the pinned kernel falls through to another one, which `f32_conv_label` states launch by launch.
PINNED_LABEL = {"split32": "skinny_gemm_f32_kernel", "tiles128": "conv_gemm_f32_kernel<dma>", "tiles64": "conv_gemm_f32_n64_kernel",
                "rows80": "conv_gemm_f32_vh_kernel<5>", "rows96": "conv_gemm_f32_vh_kernel<6>", "rows112": "conv_gemm_f32_vh_kernel<7>",
                "wide256": "conv_gemm_f32_t256_kernel"}


def f32_conv_label(sel, M, T, cout, colstat=False, tee_add=False, stat_rows=False):
    """The launch label of one sd_conv1d_cl_f32 call under selection `sel` on the MI355X: sd_choose_conv_f32 (csrc/sd_conv_choice.h)
    restated rule by rule, in its order, with the tuning values `select_conv_kernel` sets (shipped: S64 128, SKINNY 128, WIDE 1024
    tiles of 256x256, half tiles and tile rows by the cost rule).  `stat_rows`: the caller takes column statistics in units other
    than 128 rows (the ECAPA schedule; the public entry does not)."""
    s64 = 128 if sel == "auto" else 0
    skinny = 128 if sel in ("auto", "split32") else 0
    wide_from = 0 if sel == "wide256" else 1024
    half = {"auto": -1, "split32": -1, "tiles64": 1}.get(sel, 0)
    rows = int(sel[4:]) if sel.startswith("rows") else (-1 if sel in ("auto", "split32") else 0)
    cd = lambda a, b: -(-a // b)  # noqa: E731
    tm, tn = cd(M, 128), cd(cout, 128)
    t128 = tm * tn
    if not colstat and T > 1 and M >= 64 and t128 < s64:                 # small time-axis launches: the 64x64 ring kernel
        return "conv_gemm_f32_s64_kernel<32>" if cd(M, 64) * cd(cout, 64) < 128 else "conv_gemm_f32_s64_kernel<64>"
    if not colstat and t128 < skinny:
        return "skinny_gemm_f32_kernel"
    if cout >= 1024 and cd(M, 256) * cd(cout, 256) >= wide_from and not tee_add and not (colstat and T < 128):
        return "conv_gemm_f32_t256_kernel"
    t64 = tm * cd(cout, 64)
    cost128, cost64 = float(cd(t128, 256)), 0.52 * cd(t64, 256)
    can = not colstat or (T >= 128 and cout % 64 == 0)
    best, best_cost = 0, 0.97 * (cost64 if half != 0 and can and cost64 < cost128 else cost128)
    if T > 1 and (not colstat or stat_rows) and rows != 0:
        for j in (5, 6, 7):
            if colstat and T < (80 if j == 5 else 8 * j):
                continue
            cj = cd(cd(M, 16 * j) * tn, 256) * j / 8.0 * 1.02
            if rows == 16 * j or (rows < 0 and cj < best_cost):
                best, best_cost = j, cj
    if best:
        return f"conv_gemm_f32_vh_kernel<{best}>"
    if can and half != 0 and (half == 1 or cost64 < 0.97 * cost128):
        return "conv_gemm_f32_n64_kernel"
    return "conv_gemm_f32_kernel<dma>"


def select_conv_kernel(name: str) -> None:
    """Pin one of CONV_KERNELS process-wide ("auto" = the shipped rules)."""
    from speech_diarization_amd import _native as N
    lib = N.load()
    # "auto": small launches take the 64x64 ring kernel (time-axis convs) or the 32x32 split-K kernel (per-segment layers);
    # "split32": the 32x32 split-K kernel for both
    N.check(lib.sd_set_tuning(N.SD_TUNE_S64_TILES, 0 if name != "auto" else -1), "sd_set_tuning")
    N.check(lib.sd_set_tuning(N.SD_TUNE_SKINNY_TILES, 0 if name not in ("auto", "split32") else -1), "sd_set_tuning")
    N.check(lib.sd_set_tuning(N.SD_TUNE_WIDE_TILES, 0 if name == "wide256" else -1), "sd_set_tuning")   # cout >= 1024 layers: the 256x256 ring kernel
    # 128x64 tiles: by the rule ("auto"), always ("tiles64"), never (the pinned kernels)
    N.check(lib.sd_set_tuning(N.SD_TUNE_HALF_TILES, {"auto": -1, "split32": -1, "tiles64": 1}.get(name, 0)), "sd_set_tuning")
    # tiles of 80 / 96 / 112 rows: by the rule ("auto"), that height wherever the layer allows ("rowsNN"), never (the pinned kernels)
    N.check(lib.sd_set_tuning(N.SD_TUNE_TILE_ROWS, int(name[4:]) if name.startswith("rows") else (-1 if name in ("auto", "split32") else 0)), "sd_set_tuning")


def restore_conv_kernel() -> None:
    from speech_diarization_amd import _native as N
    lib = N.load()
    for key in (N.SD_TUNE_HALF_TILES, N.SD_TUNE_TILE_ROWS, N.SD_TUNE_S64_TILES, N.SD_TUNE_SKINNY_TILES, N.SD_TUNE_WIDE_TILES):
        N.check(lib.sd_set_tuning(key, -1), "sd_set_tuning")


@pytest.fixture(params=CONV_KERNELS)
def conv_kernel(request):
    """Small launches pick the 64x64 ring / 32x32 split-K kernel by themselves ("auto"); the other selections pin "split32", the
    128x128 kernel, 128x64 tiles, tiles of 80 / 96 / 112 rows and the 256x256 ring kernel for every cout >= 1024 layer, so that every
    implementation of the operator sees every case; tuning restored afterwards."""
    select_conv_kernel(request.param)
    yield request.param
    restore_conv_kernel()


@pytest.fixture(params=["wide256", "auto"])
def f16_tiles(request):
    """"wide256" pins the 256x256 kernel for every cout >= 1024 layer; "auto" is the shipped choice."""
    from speech_diarization_amd import _native as N
    lib = N.load()
    N.check(lib.sd_set_tuning(N.SD_TUNE_F16_NARROW_TILES, 0 if request.param == "wide256" else -1), "sd_set_tuning")
    yield request.param
    N.check(lib.sd_set_tuning(N.SD_TUNE_F16_NARROW_TILES, -1), "sd_set_tuning")
