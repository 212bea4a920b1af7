"""No-GPU checks of the argument rules every conv entry shares (sd_check_conv): a negative a_col0, which would make the kernel read before
the row, is refused by each of them with nothing launched."""
import ctypes as C

import pytest

from speech_diarization_amd import _native as N

F32, F16, S16 = N.SD_DT_F32, N.SD_DT_F16, N.SD_DT_SPLIT16
# (entry, x / w / y dtypes, value granularity of lda / a_col0, cin_pad)
ENTRIES = [("sd_conv1d_cl_f32", (F32, F32, F32), 4, 32), ("sd_conv1d_cl_packed_f32", (F32, F32, F32), 4, 32),
           ("sd_conv1d_cl_f16", (F16, F16, F16), 8, 64), ("sd_conv1d_cl_split16", (F32, S16, F32), 4, 32),
           ("sd_conv1d_cl_split16", (S16, S16, F32), 32, 32)]


def _call(lib, name, a, p):
    if name == "sd_conv1d_cl_packed_f32":
        return lib.sd_conv1d_cl_packed_f32(C.byref(a), p, 1, None)
    return getattr(lib, name)(C.byref(a), None)


@pytest.mark.parametrize("name,dtypes,gran,cin_pad", ENTRIES, ids=[f"{e[0]}-x{e[1][0]}" for e in ENTRIES])
def test_negative_a_col0_is_refused_by_every_conv_entry(name, dtypes, gran, cin_pad):
    lib = N.load()
    buf = (C.c_float * 4096)()
    p = C.addressof(buf)
    for col0 in sorted({-4, -gran}):
        a = N.sd_conv_args()
        a.x, a.w, a.y = p, p, p
        a.x_dtype, a.w_dtype, a.y_dtype = dtypes
        a.M, a.T = 64, 16
        a.cin, a.cin_pad, a.cout, a.taps, a.dil = 32, cin_pad, 32, 3, 1
        a.lda, a.a_col0, a.ldo = 128, col0, 32
        assert _call(lib, name, a, p) == -1, (name, col0)
        assert "a_col0" in N.last_error(), N.last_error()
