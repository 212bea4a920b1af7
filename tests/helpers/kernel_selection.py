"""The kernel selections of the exact-f32 conv operator (`sd_set_tuning`), as one fixture shared by the GPU test modules, and the two
tile choices of the f16 / split16 operators (`f16_tiles`).

Imported, not a conftest: `from kernel_selection import conv_kernel` (with tests/helpers on sys.path) makes the fixture visible
to the importing module only."""
import pytest

CONV_KERNELS = ["auto", "split32", "tiles128", "tiles64", "rows80", "rows96", "rows112", "wide256"]


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
