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


# ------------------------------------------------------------------------- lifting a uint8 design to a typed frame
KINDS = {"float16": np.uint16, "bfloat16": np.uint16, "float32": np.uint32}      # kind -> the dtype of its bit patterns


def elements(kind, bits):
    """Bit patterns -> the element array `quantize` takes."""
    bits = np.ascontiguousarray(bits, KINDS[kind])
    return bits if kind == "bfloat16" else bits.view(np.float16 if kind == "float16" else np.float32)


def conversion_t(x, scale, bias):
    """The float32 `t` of the conversion."""
    with np.errstate(all="ignore"):
        return widen(x) * np.float32(scale) + np.float32(bias)


def _is_tie(t):
    with np.errstate(all="ignore"):
        return np.isfinite(t) & (t - np.floor(t) == np.float32(0.5))


def reachable(kind, scale, bias):
    """2-byte kinds: the pixel values that some finite element converts to."""
    x = elements(kind, np.arange(1 << 16, dtype=np.uint16))
    return np.unique(quantize(x, scale, bias)[np.isfinite(widen(x))])


def preimages(kind, scale, bias, n=4):
    """(256, n) element bit patterns: for each pixel value v up to n distinct finite elements x with quantize(x) == v.
    float16 / bfloat16: out of all 65 536 patterns grouped by `quantize`, the smallest, the largest and the one nearest the
    centre of v's group; float32: the candidates fl32((v + d - bias) / scale), d in {0, -0.49, 0.49, -0.5, 0.5}, that `quantize`
    sends to v.  Where the group holds a tie element (t is exactly k + 0.5 and rounds to v) one is among them.  Missing
    alternates repeat the first.  A value that no finite element reaches raises."""
    out = np.zeros((256, n), KINDS[kind])
    if kind == "float32":
        v = np.arange(256, dtype=np.float64)[:, None]
        d = np.array([0.0, -0.49, 0.49, -0.5, 0.5])[None, :]
        with np.errstate(all="ignore"):
            cand = ((v + d - float(np.float32(bias))) / float(np.float32(scale))).astype(np.float32)
        ok = np.isfinite(cand) & (quantize(cand, scale, bias) == np.arange(256)[:, None])
        tie = ok & _is_tie(conversion_t(cand, scale, bias))
        groups = [(cand[k][ok[k]].view(np.uint32), tie[k][ok[k]]) for k in range(256)]
    else:
        bits = np.arange(1 << 16, dtype=np.uint16)
        x = elements(kind, bits)
        val = widen(x)
        fin = np.isfinite(val)
        q, tie = quantize(x, scale, bias), _is_tie(conversion_t(x, scale, bias))
        groups = []
        for k in range(256):
            m = np.flatnonzero(fin & (q == k))
            m = m[np.argsort(val[m], kind="stable")]
            if m.size:
                centre = (np.float64(val[m[0]]) + np.float64(val[m[-1]])) / 2
                m = m[[0, m.size - 1, int(np.argmin(np.abs(val[m].astype(np.float64) - centre)))] + list(np.flatnonzero(tie[m])[:1])]
            groups.append((bits[m], tie[m]))
    for k, (g, t) in enumerate(groups):
        if g.size == 0:
            raise ValueError("%s under (%r, %r): no finite element converts to %d" % (kind, scale, bias, k))
        order = list(dict.fromkeys(g.tolist()))
        ties = [b for b, is_t in zip(g.tolist(), t.tolist()) if is_t]
        if ties and ties[0] not in order[:n]:
            order[n - 1] = ties[0]
        order = order[:n]
        out[k] = order + [order[0]] * (n - len(order))
    return out


def lift_columns(h, w, n, salt, device=None):
    """The bank column of every position: a seeded function of (x, y), as an (h, w) int64 array (device: a torch tensor there)."""
    if device is None:
        y, x = np.arange(h, dtype=np.int64)[:, None], np.arange(w, dtype=np.int64)[None, :]
    else:
        import torch
        y, x = torch.arange(h, device=device)[:, None], torch.arange(w, device=device)[None, :]
    return ((x * 0x9E3779B1 + y * 0x85EBCA77 + (int(salt) & 0xFFFF) * 0xC2B2AE3D) >> 15) % n


def lift(img, bank, salt):
    """(..., h, w) uint8 -> (..., h, w) element bit patterns: pixel v at (x, y) becomes bank[v, lift_columns(...)[y, x]].
    numpy arrays, or torch tensors on one device (the bank as int16 / int32 bits): indexing only."""
    h, w = img.shape[-2:]
    if isinstance(img, np.ndarray):
        return bank[img.astype(np.intp), lift_columns(h, w, bank.shape[1], salt)]
    return bank[img.long(), lift_columns(h, w, bank.shape[1], salt, img.device)]
