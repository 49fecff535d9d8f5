"""The conversion of typed encode (include/hgi_typed.h), restated in numpy (a helper module of tests/test_typed*.py, not a
conftest).  Expected grids are `oracle.encode(quantize(frame, scale, bias), levels, lut, interp)`: never the library under test.

    t = fl32(fl32(x * scale) + bias)      two separately rounded float32 operations
    v = 0 if t is NaN, else clamp(rint(t), 0, 255)      rint rounds half to even; +-inf clamp; denormals are kept
"""
import numpy as np

PAIRS = ((255.0, 0.0), (1.0, 37.25), (-3.5, 300.0))      # the (scale, bias) pairs of the suites


def widen(x):
    """Elements -> float32, exactly.  float16 / float32 arrays as they are; bfloat16 arrives as uint16 bit patterns."""
    x = np.asarray(x)
    if x.dtype == np.uint16:
        return (x.astype(np.uint32) << np.uint32(16)).view(np.float32)
    if x.dtype not in (np.dtype(np.float16), np.dtype(np.float32)):
        raise TypeError("float16, float32 or uint16 (bfloat16 bits), not %s" % x.dtype)
    return x.astype(np.float32)


def quantize(x, scale, bias):
    """The uint8 image the codec encodes for the frame `x`."""
    with np.errstate(all="ignore"):
        m = widen(x) * np.float32(scale)            # rounded to float32
        t = m + np.float32(bias)                    # rounded again: numpy never fuses the two
        v = np.clip(np.rint(t), np.float32(0), np.float32(255))
        v = np.where(np.isnan(t), np.float32(0), v)
    return v.astype(np.uint8)


def bf16_bits(x32):
    """float32 -> bfloat16 bit patterns (uint16), round to nearest even: what torch's .to(bfloat16) does for finite values."""
    u = np.asarray(x32, np.float32).view(np.uint32)
    return ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)
