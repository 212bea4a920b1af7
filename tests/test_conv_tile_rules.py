"""No-GPU checks that the rules the matrix-core kernels share are stated once, in csrc/sd_conv_tile.h: a copy
that comes back into a kernel file is found here, and a kernel that keeps its own text says which helper it restates."""
import re

from speech_diarization_amd import _native as N

CSRC = N.PKG_DIR / "csrc"
HEADER = "sd_conv_tile.h"
DMA = "__builtin_amdgcn_global_load_lds"
REFLECT = re.compile(r"\?\s*2 \* \([\w.]+ - 1\) - \w+\s*:")                       # t >= T ? 2 * (T - 1) - t : t
REMAP = re.compile(r"xcd \* \(q \+ 1\) : r \* \(q \+ 1\) \+ \(xcd - r\) \* q")
SCATTER = re.compile(r"\((\w) & 3\) \+ 8 \* \(\1 >> 2\)|8 \* \((\w) >> 2\) \+ 4 \* \w+ \+ \(\2 & 3\)")
# the kernels that keep their own text (tools/isa_diff.py: through the helper their device code changes) and the helper each names
OWN_TEXT = {
    "reflect": {"sd_fbank_utt16.hip": (1, "sd_reflect")},
    "remap": {"sd_conv_gemm.hip": (1, "sd_xcd_tile")},
    "scatter": {"sd_conv_gemm.hip": (2, "SD_ACC32_TO_TILE")},
}
# (sd_fbank.hip's DFT writes accumulators of the same MFMA into its own power-spectrum layout: not an epilogue C tile)
SCATTER_FILES = ("sd_conv_gemm.hip", "sd_conv_gemm_f16.hip", "sd_conv_tile_reg16_body.h")


def _sources():
    return {f.name: f.read_text() for f in sorted(CSRC.glob("*.hip")) + sorted(CSRC.glob("*.h"))}


def _sites(pattern, text):
    lines = text.splitlines()
    return [i for i, ln in enumerate(lines) if pattern.search(ln)], lines


def test_the_header_holds_helpers_and_no_kernel():
    header = (CSRC / HEADER).read_text()
    assert not re.search(r"^\s*__global__", header, re.M)
    for name in ("SD_GLDS16", "sd_reflect", "sd_xcd_first", "sd_xcd_count", "sd_xcd_tile", "sd_swap16", "sd_swap32", "SD_ACC32_TO_TILE",
                 "sd_conv_flops", "sd_launch_conv"):
        assert re.search(rf"\b{name}\b", header), name
    assert not re.search(r"^\s*__global__", (CSRC / "sd_conv_tile_reg16_body.h").read_text(), re.M)


def test_the_lds_dma_builtin_and_the_permlane_swaps_stand_in_the_header_only():
    for name, text in _sources().items():
        if name != HEADER:
            assert DMA not in text, name
            assert "permlane32_swap(" not in text, name
    assert DMA in (CSRC / HEADER).read_text()
    # (v_permlane16_swap also joins the f16 pairs of the 256x256 kernel's register epilogue: a different use, in sd_conv_gemm_f16.hip)


def test_every_copy_left_in_a_kernel_names_the_shared_statement():
    src = _sources()
    for rule, pattern in (("reflect", REFLECT), ("remap", REMAP), ("scatter", SCATTER)):
        files = SCATTER_FILES if rule == "scatter" else [n for n in src if n != HEADER]
        found = {}
        for name in files:
            sites, lines = _sites(pattern, src[name])
            if sites:
                found[name] = len(sites)
                helper = OWN_TEXT[rule].get(name, (0, "?"))[1]
                for i in sites:
                    assert any(helper in ln and "//" in ln for ln in lines[max(0, i - 10):i + 1]), (rule, name, i + 1)
        assert found == {n: c for n, (c, _) in OWN_TEXT[rule].items()}, (rule, found)
        assert len(_sites(pattern, src[HEADER])[0]) == 1, rule          # the search finds the statement where it is
