"""Typed volumes (include/vrhip.h vr_dtype), the value contract on the CPU: vr_dtype_size over every
code and flag combination, and vr_convert_host -- the very conversion the upload's pad pass applies
on the device (one definition, csrc/vr_convert.h) -- against numpy: astype(float32), and for UNORM
astype(float32) / float32(255 resp. 65535), bit for bit."""
import ctypes

import numpy as np
import pytest

vr = pytest.importorskip("volume_renderer_amd")
from volume_renderer_amd import _lib, mex  # noqa: E402

F32, U8, U16, I16, F16, UNORM = _lib.VR_F32, _lib.VR_U8, _lib.VR_U16, _lib.VR_I16, _lib.VR_F16, _lib.VR_DTYPE_UNORM


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_dtype_size_all_codes_and_flags():
    valid = {F32: 4, U8: 1, U16: 2, I16: 2, F16: 2, U8 | UNORM: 1, U16 | UNORM: 2}
    for code in list(range(-3, 12)) + [0x7FFFFFFF, -0x80000000, 255, 0x200, 0x101 + 0x100]:
        for flag in (0, UNORM, 0x200, UNORM | 0x200, 0x80, -0x80000000):
            c = ctypes.c_int32(code | flag).value
            assert mex.dtype_size(c) == valid.get(c, 0), hex(c & 0xFFFFFFFF)
    assert mex.dtype_size(F32 | UNORM) == 0 and mex.dtype_size(I16 | UNORM) == 0 and mex.dtype_size(F16 | UNORM) == 0


def test_struct_layout_unchanged():
    """vr_volume.reserved became dtype: same size, same offsets, zero = VR_F32."""
    assert ctypes.sizeof(_lib.VrVolume) == 48
    assert _lib.VrVolume.dtype.offset == 44 and _lib.VrVolume.location.offset == 40
    assert _lib.VrVolume().dtype == F32 == 0


def test_convert_uint8_every_value():
    x = np.arange(256, dtype=np.uint8)
    assert np.array_equal(_bits(mex.convert_host(x)), _bits(x.astype(np.float32)))
    assert np.array_equal(_bits(mex.convert_host(x, unorm=True)), _bits(x.astype(np.float32) / np.float32(255)))


def test_convert_uint16_extremes_and_random():
    rng = np.random.default_rng(7)
    x = np.concatenate([np.array([0, 1, 2, 255, 256, 32767, 32768, 65534, 65535], np.uint16),
                        rng.integers(0, 65536, 20000, dtype=np.uint16)])
    assert np.array_equal(_bits(mex.convert_host(x)), _bits(x.astype(np.float32)))
    assert np.array_equal(_bits(mex.convert_host(x, unorm=True)), _bits(x.astype(np.float32) / np.float32(65535)))
    every = np.arange(65536, dtype=np.uint16)  # (cheap: all of them too)
    assert np.array_equal(_bits(mex.convert_host(every, unorm=True)),
                          _bits(every.astype(np.float32) / np.float32(65535)))


def test_convert_int16_extremes_and_random():
    rng = np.random.default_rng(8)
    x = np.concatenate([np.array([0, 1, -1, 127, -128, 32767, -32768, -32767], np.int16),
                        rng.integers(-32768, 32768, 20000, dtype=np.int16)])
    assert np.array_equal(_bits(mex.convert_host(x)), _bits(x.astype(np.float32)))


def test_convert_half_every_bit_pattern():
    h = np.arange(65536, dtype=np.uint16).view(np.float16)
    got = mex.convert_host(h)
    ref = h.astype(np.float32)
    nan = np.isnan(ref)
    assert nan.sum() == 2 * 1023 and np.array_equal(np.isnan(got), nan)  # the NaN positions
    assert np.array_equal(_bits(got)[~nan], _bits(ref)[~nan])            # everything else by bit pattern
    # subnormals, signed zeros and infinities are among them
    assert _bits(got)[0x8000] == 0x80000000 and _bits(got)[0x0001] == np.float32(2.0 ** -24).view(np.uint32)
    assert np.isposinf(got[0x7C00]) and np.isneginf(got[0xFC00])


def test_convert_float32_is_a_copy_and_shape_is_kept():
    rng = np.random.default_rng(9)
    x = np.asfortranarray(rng.standard_normal((5, 4, 3)).astype(np.float32))
    x[1, 2, 0] = np.nan
    assert np.array_equal(_bits(mex.convert_host(x)), _bits(x))
    y = np.asfortranarray(rng.integers(0, 256, (5, 4, 3), dtype=np.uint8))
    out = mex.convert_host(y)
    assert out.shape == y.shape and np.array_equal(out, y.astype(np.float32))


def test_convert_errors():
    L = vr.lib()
    src = np.zeros(8, np.uint16)
    dst = np.zeros(8, np.float32)
    p, q = src.ctypes.data, dst.ctypes.data
    for code in (7, -1, F32 | UNORM, I16 | UNORM, F16 | UNORM, UNORM):
        assert L.vr_convert_host(p, code, 4, q) == 1  # VR_ERR_ARGUMENT
    assert L.vr_convert_host(p + 1, U16, 2, q) == 1   # not aligned to its element size
    assert L.vr_convert_host(p + 1, U8, 2, q) == 0
    assert L.vr_convert_host(None, U8, 2, q) == 1
    assert L.vr_convert_host(None, U8, 0, None) == 0


def test_python_volume_marshalling_carries_the_dtype(counter_clock):
    """_vr_volume: column-major uint8 / uint16 / int16 / float16 arrays map to their codes, a
    RawVolume's RawData (and Unorm) is taken instead of Data, anything else still raises."""
    for dt, code in ((np.uint8, U8), (np.uint16, U16), (np.int16, I16), (np.float16, F16)):
        rv = vr.RawVolume(np.zeros((3, 2, 2), dt))
        v = mex._vr_volume(rv)
        assert v.dtype == code and v.data == rv.RawData.ctypes.data and list(v.dims) == [3, 2, 2]
    rv = vr.RawVolume(np.zeros((3, 2), np.uint16), True)
    assert mex._vr_volume(rv).dtype == U16 | UNORM and list(mex._vr_volume(rv).dims) == [3, 2, 1]
    t0 = int(rv.TimeLastUpdate)
    rv.RawData = np.ones((3, 2), np.uint16)
    assert int(rv.TimeLastUpdate) > t0  # setting RawData stamps TimeLastUpdate
    t1 = int(rv.TimeLastUpdate)
    rv.Unorm = False
    assert int(rv.TimeLastUpdate) > t1 and mex._vr_volume(rv).dtype == U16
    assert mex._vr_volume(vr.Volume(np.zeros((2, 2, 2)))).dtype == F32
    with pytest.raises(TypeError):
        vr.RawVolume(np.zeros((2, 2, 2), np.int16), True)
    with pytest.raises(TypeError):
        vr.RawVolume(np.zeros((2, 2, 2), np.float64))

    class Shaped:
        Data = np.zeros((2, 2, 2), np.float64)
        TimeLastUpdate = np.uint64(1)
    with pytest.raises(TypeError):
        mex._vr_volume(Shaped())
