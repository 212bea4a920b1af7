"""What the no-GPU rule tests of the side headers (spectral, AHC, HDBSCAN, diag) check alike: a header and its binding table name the same
exported entries, the ABI versions, and `refused`, the statement that an entry returned its own status code with a message before it
launched anything."""
import re
import subprocess

from speech_diarization_amd import _native as N

ARG, UNSUP, WS = -1, -2, -3          # SD_ERR_ARG, SD_ERR_UNSUPPORTED, SD_ERR_WORKSPACE


def refused(status, code, needle):
    assert status == code, (status, N.last_error())
    assert needle in N.last_error(), N.last_error()


def header_names(header: str) -> set:
    """The sd_* functions include/<header> declares (comments removed)."""
    text = (N.PKG_DIR.parent / "include" / header).read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(sd_[a-z0-9_]+)\s*\(", text))


def check_header_and_table(header: str, table: dict, others) -> set:
    """include/<header> and `table` name the same entries, none of them in one of the `others` tables; the loaded library carries the
    table's prototypes and exports every name -> the names."""
    names = header_names(header)
    assert names == set(table), names ^ set(table)
    for other in others:
        assert not names & set(other), names & set(other)
    lib = N.load()
    for name, (res, args) in table.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    out = subprocess.run(["nm", "-D", "--defined-only", str(N.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (sd_[a-z0-9_]+)$", out, flags=re.M))
    assert names <= exported, names - exported
    return names


def check_versions(**want):
    """Every `sd_*_abi_version` entry named returns the value given."""
    lib = N.load()
    for entry, value in want.items():
        assert getattr(lib, entry)() == value, entry
