"""The host-pointer calls of the C ABI on caller arrays of EXACTLY the span include/hgi.h promises -- (height - 1) * pitch +
width bytes, np.empty(span), nothing behind the last row -- against the oracle: hgi_encode_u8_pitched / hgi_decode_u8_pitched.
Ordinary calls within the contract: no guard pages, no unmapped memory.  The CPU harness (tests/test_host_routes.py,
profiles/r16_host_routes.md) holds the same calls to the host-span rule of DESIGN.md 4.14 under ASan; this file shows the
real runtime the copies the rule led to.  hgi_decode_scaled_u8 is not called here (the cause of its fault in profiles/r14_typed_coverage.md section 7 is not established), and neither is
hgi_decode_region_u8 (profiles/r16_host_routes.md section 8)."""
import numpy as np
import pytest

from conftest import SEED0

pytestmark = pytest.mark.gpu
SENT = 0xC3
SHAPES = ((130, 33), (257, 131), (1001, 99))
LEVELS = (2, 5, 9)
PADS = (1, 61)


@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    from rustyhgi_amd import _ffi
    return _ffi


@pytest.fixture(scope="module")
def ctx(lib):
    import rustyhgi_amd
    c = rustyhgi_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def coded(oracle):
    """Every (shape, levels): image, table, the oracle's grid and its decode -- computed once, shared, never written."""
    rng = np.random.default_rng(SEED0 + 16)
    out = {}
    for (w, h) in SHAPES:
        img = (np.add.outer(5 * np.arange(h), 3 * np.arange(w)) // 4 + rng.integers(0, 40, (h, w))).astype(np.uint8)
        for levels in LEVELS:
            lut = oracle.linear_lut(levels % 3)[0]
            grid = oracle.encode(img, levels, lut)
            out[(w, h, levels)] = (img, lut, grid, oracle.decode(grid, levels))
            for a in out[(w, h, levels)]:
                a.setflags(write=False)
    return out


def exact_span(rows, pitch, fill):
    """`rows` (h, w) laid out `pitch` apart in an array that ends with its last row; the gaps hold `fill`."""
    h, w = rows.shape
    a = np.empty((h - 1) * pitch + w, np.uint8)
    a[:] = fill
    view = np.lib.stride_tricks.as_strided(a, (h, w), (pitch, 1))
    view[:] = rows
    return a


def sentinel(h, w, pitch):
    a = np.empty((h - 1) * pitch + w, np.uint8)
    a[:] = SENT
    return a


def check_rows(a, want, pitch, what):
    h, w = want.shape
    expect = exact_span(want, pitch, SENT)
    if not (a == expect).all():
        bad = int(np.flatnonzero(a != expect)[0])
        raise AssertionError("%s: byte %d (row %d, column %d of pitch %d) is %d, want %d" % (what, bad, bad // pitch, bad % pitch, pitch, a[bad], expect[bad]))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_pitched_host_calls_on_exact_spans(lib, ctx, coded, shape):
    w, h = shape
    L = lib.lib()
    for levels in LEVELS:
        img, lut, grid, dec = coded[(w, h, levels)]
        for ip in PADS:
            for op in PADS:
                src = exact_span(img, w + ip, 0x11)
                before = src.copy()
                out = sentinel(h, w, w + op)
                lib.check(L.hgi_encode_u8_pitched(ctx.handle, src.ctypes.data, w + ip, w, h, levels, 1, lut.ctypes.data, out.ctypes.data, w + op))
                check_rows(out, grid, w + op, "hgi_encode_u8_pitched %dx%d L%d pitch %d -> %d" % (w, h, levels, w + ip, w + op))
                assert (src == before).all()
                src = exact_span(grid, w + ip, 0x11)
                before = src.copy()
                out = sentinel(h, w, w + op)
                lib.check(L.hgi_decode_u8_pitched(ctx.handle, src.ctypes.data, w + ip, w, h, levels, 1, out.ctypes.data, w + op))
                check_rows(out, dec, w + op, "hgi_decode_u8_pitched %dx%d L%d pitch %d -> %d" % (w, h, levels, w + ip, w + op))
                assert (src == before).all()
