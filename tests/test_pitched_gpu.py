"""GPU suite of pitched frames (hgi_encode_u8_pitched_dev / hgi_decode_u8_pitched_dev and the host forms): every shape, depth,
pitch and alignment must give, read through the output's pitch, the bytes of the packed frame's encode / decode, bit for bit,
and no byte outside the output rows may be written.  Every case reads its input out of a parent buffer whose gaps hold RANDOM
bytes (a leak of foreign data into a prediction shows) and writes into a SENTINEL-filled parent buffer that is checked whole.
Expected bytes: the oracle on the packed copy, or -- only where the oracle is too slow, said in the test's docstring -- the
library's UNIFORM call on the packed copy.  Never the pitched call itself."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, SEED0

pytestmark = pytest.mark.gpu
SENT = 0xC3
GAPS = (1, 3, 16, 61, 128)


@pytest.fixture(scope="module")
def H():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    import rustyhgi_amd
    from rustyhgi_amd import _ffi
    assert _ffi.lib() is not None
    return rustyhgi_amd


@pytest.fixture(scope="module")
def ctx(H):
    import torch
    c = H.Context(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


def assert_same(a, b, what):
    if a.shape != b.shape:
        raise AssertionError("%s: shape %s, want %s" % (what, a.shape, b.shape))
    if not (a == b).all():
        bad = np.argwhere(a != b)
        raise AssertionError("%s: %d mismatches, first at %s: got %d want %d" % (what, len(bad), tuple(bad[0]), a[tuple(bad[0])], b[tuple(bad[0])]))


def lut_for(oracle, q):
    return oracle.noop_lut() if q == "noop" else oracle.linear_lut(int(q))[0]


def rows_index(B, h, w, lead, pitch, fstride):
    return lead + (np.arange(B)[:, None, None] * fstride + np.arange(h)[None, :, None] * pitch + np.arange(w)[None, None, :])


def pitched_dev(ctx, frames, levels, interp, lut, sp, dp, slead=0, dlead=0, sextra=0, dextra=0, seed=1, call=None):
    """The pitched device call on the (B, h, w) numpy `frames` (lut None: decode, else encode).  The input goes into a parent
    buffer of random bytes at offset `slead`, rows `sp` apart, frames a span + `sextra` apart; the output into a sentinel-filled
    parent with `dlead`, `dp`, `dextra`.  Returns the (B, h, w) output frames read through the pitch; asserts that every other
    byte of the output parent still holds the sentinel and that the input parent was not modified."""
    import torch
    from rustyhgi_amd import _ffi
    L = _ffi.lib()
    B, h, w = frames.shape
    sspan, dspan = (h - 1) * sp + w, (h - 1) * dp + w
    sfs, dfs = sspan + sextra, dspan + dextra
    rng = np.random.default_rng(seed)
    src = rng.integers(0, 256, slead + (B - 1) * sfs + sspan + 64, dtype=np.uint8)
    sidx = rows_index(B, h, w, slead, sp, sfs)
    src[sidx] = frames
    total = dlead + (B - 1) * dfs + dspan + 64
    d_src = torch.from_numpy(src).cuda()
    d_dst = torch.full((total,), SENT, dtype=torch.uint8, device="cuda")
    if call is not None:
        call(d_src.data_ptr() + slead, sp, sfs, d_dst.data_ptr() + dlead, dp, dfs)
    elif lut is None:
        _ffi.check(L.hgi_decode_u8_pitched_dev(ctx.handle, d_src.data_ptr() + slead, sp, w, h, levels, interp, d_dst.data_ptr() + dlead, dp,
                                               B, sfs, dfs))
    else:
        lut = np.ascontiguousarray(lut, np.uint8)
        _ffi.check(L.hgi_encode_u8_pitched_dev(ctx.handle, d_src.data_ptr() + slead, sp, w, h, levels, interp, lut.ctypes.data,
                                               d_dst.data_ptr() + dlead, dp, B, sfs, dfs))
    torch.cuda.synchronize()
    host = d_dst.cpu().numpy()
    didx = rows_index(B, h, w, dlead, dp, dfs)
    mask = np.zeros(total, bool)
    mask[didx] = True
    stray = np.nonzero(host[~mask] != SENT)[0]
    what = "%s %dx%dx%d L%d i%d pitches %d/%d leads %d/%d" % ("dec" if lut is None else "enc", B, w, h, levels, interp, sp, dp, slead, dlead)
    assert len(stray) == 0, "%s: %d bytes outside the output rows written" % (what, len(stray))
    assert (d_src.cpu().numpy() == src).all(), what + ": the input parent was modified"
    return host[didx]


def check_both(ctx, oracle, imgs, levels, interp, lut, sp, dp, what, **kw):
    """Encode and decode of the (B, h, w) images through the given layouts against the oracle on the packed frames."""
    grids = np.stack([oracle.encode(im, levels, lut, interp) for im in imgs])
    got = pitched_dev(ctx, imgs, levels, interp, lut, sp, dp, **kw)
    assert_same(got, grids, "encode " + what)
    want = np.stack([oracle.decode(g, levels, interp) for g in grids])
    got = pitched_dev(ctx, grids, levels, interp, None, dp, sp, **kw)      # (the pitches swapped sides)
    assert_same(got, want, "decode " + what)


def test_small_golden_cases_through_pitches(ctx, oracle, golden, small):
    """The tiny / odd shapes of tests/golden/small_cases.npz x their quantizers x both interpolators (the stored grids and
    decodes are the oracle's), pitches width + {1, 3, 16, 61, 128} chosen differently for input and output, base offsets 0 ... 15."""
    n = 0
    for key in golden:
        if ("grid/" + key) not in small:
            continue
        name, lv, q, i = key.split("/")
        levels, interp = int(lv[1:]), int(i[1:])
        img = small["in/" + name]
        h, w = img.shape
        lut = lut_for(oracle, q[1:])
        sp, dp = w + GAPS[n % 5], w + GAPS[(n // 5 + n + 2) % 5]
        kw = dict(slead=n % 16, dlead=(5 * n + 3) % 16, seed=n)
        assert_same(pitched_dev(ctx, img[None], levels, interp, lut, sp, dp, **kw)[0], small["grid/" + key], "encode " + key)
        assert_same(pitched_dev(ctx, small["grid/" + key][None], levels, interp, None, dp, sp, **kw)[0], small["dec/" + key], "decode " + key)
        n += 1
    assert n >= 100


RAGGED = [(w, h) for w in (128, 130, 255, 1918, 1920, 2049) for h in (64, 70, 1080, 1088)]


@pytest.mark.parametrize("w,h", RAGGED)
def test_interior_and_ragged_tiles_levels_1_to_5_against_the_oracle(ctx, oracle, w, h):
    """Frames with interior tiles and every kind of ragged tile, levels 1 ... 5, random quantizer tables on noise (the overflow
    fallback fires constantly), batch 3 with frame strides larger than the span, both interpolators along the list."""
    rng = np.random.default_rng(SEED0 + 11 * w + h)
    for levels in range(1, 6):
        interp = (levels + w) & 1
        imgs = rng.integers(0, 256, (3, h, w), dtype=np.uint8)
        lut = rng.integers(0, 256, 256, dtype=np.uint8)
        sp, dp = w + GAPS[levels % 5], w + GAPS[(levels + 2) % 5]
        check_both(ctx, oracle, imgs, levels, interp, lut, sp, dp, "%dx%d L%d" % (w, h, levels), slead=levels, dlead=16 - levels,
                   sextra=77 + levels, dextra=1000, seed=levels)


def test_aligned_pitch_under_odd_widths(ctx, oracle):
    """The layout the feature exists for: 1918-wide rows at pitch 2048 on a 256-B aligned base (every row starts on a line), and a
    packed-like pitch of width + 1; one-column and one-row frames with large pitches."""
    rng = np.random.default_rng(SEED0 + 5)
    for (w, h, sp, dp) in ((1918, 1080, 2048, 2048), (1918, 200, 1919, 2048), (1, 300, 4096, 17), (300, 1, 1 << 20, 1 << 30), (1, 1, 1, 7)):
        for levels in (3, 4):
            imgs = rng.integers(0, 256, (2, h, w), dtype=np.uint8)
            check_both(ctx, oracle, imgs, levels, 1, oracle.linear_lut(2)[0], sp, dp, "%dx%d pitches %d/%d" % (w, h, sp, dp),
                       sextra=5 if h > 1 else 0, dextra=9 if h > 1 else 0)


DEEP = [(1500, 1100), (600, 5000)]


@pytest.mark.parametrize("w,h", DEEP)
def test_every_depth_route_against_the_oracle(ctx, oracle, w, h):
    """Levels 6, 7, 8 (the cone reads the frame's own lattice through the pitch) and 9, 12, 31 (the stride-256 lattice gathered
    through the pitch into the uniform route's planes), batch 2, against the oracle."""
    rng = np.random.default_rng(SEED0 + w)
    for levels in (6, 7, 8, 9, 12, 31):
        interp = levels & 1
        imgs = rng.integers(0, 256, (2, h, w), dtype=np.uint8)
        lut = oracle.linear_lut(3)[0] if levels % 3 else rng.integers(0, 256, 256, dtype=np.uint8)
        check_both(ctx, oracle, imgs, levels, interp, lut, w + GAPS[levels % 5], w + GAPS[(levels + 3) % 5], "%dx%d L%d" % (w, h, levels),
                   slead=levels % 16, dlead=3, sextra=levels, dextra=4096, seed=levels)


def test_level_zero_is_a_copy_of_the_rows(ctx):
    rng = np.random.default_rng(3)
    imgs = rng.integers(0, 256, (3, 37, 201), dtype=np.uint8)
    lut = np.arange(256, dtype=np.uint8)
    assert_same(pitched_dev(ctx, imgs, 0, 1, lut, 230, 201 + 61, slead=3, dlead=5, sextra=9, dextra=11), imgs, "encode L0")
    assert_same(pitched_dev(ctx, imgs, 0, 0, None, 201 + 1, 512, slead=1, dlead=0, sextra=0, dextra=1), imgs, "decode L0")


def test_crop_identity_and_canvas_window(H, ctx, oracle):
    """Encoding the window (x0, y0, w, h) of a 3 x 2160 x 3840 noise tensor through encode_view equals the oracle's encode of the
    cropped copy, for six windows incl. odd offsets and sizes; decoding into the same window of a canvas equals the oracle's
    decode, the canvas elsewhere untouched."""
    import torch
    from rustyhgi_amd.interpolator import Crossed
    from rustyhgi_amd.quantizator import Linear, QuantizationLevel
    gen = torch.Generator(device="cuda")
    gen.manual_seed(SEED0 + 77)
    parent = torch.randint(0, 256, (3, 2160, 3840), dtype=torch.uint8, device="cuda", generator=gen)
    host = parent.cpu().numpy()
    lut, _ = oracle.linear_lut(oracle.MEDIUM)
    windows = [(0, 0, 3840, 2160), (1920, 1080, 1920, 1080), (1, 3, 1277, 719), (2563, 7, 1277, 2001), (128, 64, 128, 64), (3839, 2159, 1, 1)]
    for n, (x0, y0, w, h) in enumerate(windows):
        levels = (4, 5, 8, 4, 3, 2)[n]
        enc = H.Encoder(Crossed(), Linear.from_level(QuantizationLevel.Medium), levels, context=ctx)
        dec = H.Decoder(Crossed(), context=ctx)
        view = parent[:, y0:y0 + h, x0:x0 + w]
        grids = enc.encode_view(view)
        torch.cuda.synchronize()
        assert grids.is_contiguous() and tuple(grids.shape) == (3, h, w)
        want = np.stack([oracle.encode(host[f, y0:y0 + h, x0:x0 + w], levels, lut) for f in range(3)])
        assert_same(grids.cpu().numpy(), want, "crop %r" % ((x0, y0, w, h),))
        assert (parent.cpu().numpy() == host).all(), "the parent was modified"
        canvas = torch.full((3, 2160 + 9, 3840 + 13), SENT, dtype=torch.uint8, device="cuda")
        r = dec.decode_view(grids, levels, out=canvas[:, y0 + 2:y0 + 2 + h, x0 + 5:x0 + 5 + w])
        torch.cuda.synchronize()
        assert r.data_ptr() == canvas[:, y0 + 2:, x0 + 5:].data_ptr()
        got = canvas.cpu().numpy()
        wantd = np.stack([oracle.decode(want[f], levels) for f in range(3)])
        assert_same(got[:, y0 + 2:y0 + 2 + h, x0 + 5:x0 + 5 + w], wantd, "canvas window %r" % ((x0, y0, w, h),))
        got[:, y0 + 2:y0 + 2 + h, x0 + 5:x0 + 5 + w] = SENT
        assert (got == SENT).all(), "the canvas was written outside the window %r" % ((x0, y0, w, h),)


def test_pitch_equal_to_width_is_the_uniform_call(ctx):
    """pitch == width on both sides: the uniform call's bytes (and its route: the call forwards), on a batch with padded frame
    strides too (there the strides differ per side and the pitched kernels run).  Expected bytes: the uniform call."""
    import torch
    from rustyhgi_amd import _ffi
    L = _ffi.lib()
    w, h, B = 1001, 333, 3
    rng = np.random.default_rng(SEED0 + 13)
    imgs = rng.integers(0, 256, (B, h, w), dtype=np.uint8)
    lut = rng.integers(0, 256, 256, dtype=np.uint8)
    d = torch.from_numpy(imgs).cuda()
    for levels in (0, 4, 7, 10):
        g = torch.empty_like(d)
        o = torch.empty_like(d)
        _ffi.check(L.hgi_encode_u8_dev(ctx.handle, d.data_ptr(), w, h, levels, 1, lut.ctypes.data, g.data_ptr(), B, w * h))
        _ffi.check(L.hgi_decode_u8_dev(ctx.handle, g.data_ptr(), w, h, levels, 1, o.data_ptr(), B, w * h))
        torch.cuda.synchronize()
        grids, outs = g.cpu().numpy(), o.cpu().numpy()
        for extra in (0, 77):
            assert_same(pitched_dev(ctx, imgs, levels, 1, lut, w, w, sextra=extra, dextra=2 * extra), grids, "encode L%d" % levels)
            assert_same(pitched_dev(ctx, grids, levels, 1, None, w, w, sextra=extra, dextra=2 * extra), outs, "decode L%d" % levels)


def test_round_trip_through_views_stays_inside_the_quantizer_bound(H, ctx):
    import torch
    from rustyhgi_amd.interpolator import Crossed
    from rustyhgi_amd.quantizator import Linear, QuantizationLevel
    gen = torch.Generator(device="cuda")
    gen.manual_seed(SEED0 + 5)
    x = torch.randint(0, 256, (4, 700, 900), dtype=torch.uint8, device="cuda", generator=gen)
    for level, bound in ((QuantizationLevel.Lossless, 0), (QuantizationLevel.Medium, 20), (QuantizationLevel.High, 30)):
        for levels in (4, 9):
            enc = H.Encoder(Crossed(), Linear.from_level(level), levels, context=ctx)
            dec = H.Decoder(Crossed(), context=ctx)
            v = x[1:4, 33:650, 101:811]
            back = dec.decode_view(enc.encode_view(v), levels)
            torch.cuda.synchronize()
            err = (back.to(torch.int16) - v.to(torch.int16)).abs().max().item()
            assert err <= bound, (level, levels, err)
    # numpy views take the host calls, frame by frame
    hx = x.cpu().numpy()
    enc = H.Encoder(Crossed(), Linear.from_level(QuantizationLevel.Medium), 5, context=ctx)
    dec = H.Decoder(Crossed(), context=ctx)
    hv = hx[:2, 5:600, 7:500]
    out = np.full((2, 640, 512), SENT, np.uint8)
    g = enc.encode_view(hv)
    r = dec.decode_view(g, 5, out=out[:, 11:606, 3:496])
    tv = x[:2, 5:600, 7:500]
    tg = enc.encode_view(tv)
    torch.cuda.synchronize()
    assert_same(g, tg.cpu().numpy(), "host encode_view against the device call")
    assert_same(r, dec.decode_view(tg, 5).cpu().numpy(), "host decode_view against the device call")
    out[:, 11:606, 3:496] = SENT
    assert (out == SENT).all()


def test_host_calls_against_the_oracle(ctx, oracle):
    from rustyhgi_amd import _ffi
    L = _ffi.lib()
    rng = np.random.default_rng(SEED0 + 9)
    for (w, h) in ((1001, 999), (130, 33), (3, 3000), (2100, 2100)):
        for levels in (2, 5, 9):
            img = rng.integers(0, 256, (h, w + 7), dtype=np.uint8)
            lut = oracle.linear_lut(1)[0]
            grid = np.full((h, w + 3), SENT, np.uint8)
            _ffi.check(L.hgi_encode_u8_pitched(ctx.handle, img.ctypes.data, w + 7, w, h, levels, 1, lut.ctypes.data, grid.ctypes.data, w + 3))
            want = oracle.encode(img[:, :w], levels, lut)
            assert_same(grid[:, :w], want, "host encode %dx%d L%d" % (w, h, levels))
            assert (grid[:, w:] == SENT).all()
            out = np.full((h, w + 61), SENT, np.uint8)
            _ffi.check(L.hgi_decode_u8_pitched(ctx.handle, grid.ctypes.data, w + 3, w, h, levels, 1, out.ctypes.data, w + 61))
            assert_same(out[:, :w], oracle.decode(want, levels), "host decode %dx%d L%d" % (w, h, levels))
            assert (out[:, w:] == SENT).all()


def test_error_cases(H, ctx):
    import torch
    from rustyhgi_amd import _ffi
    L = _ffi.lib()
    w, h = 300, 200
    a = torch.zeros((2 * 512 * h,), dtype=torch.uint8, device="cuda")
    o = torch.full((2 * 512 * h,), SENT, dtype=torch.uint8, device="cuda")
    lut = np.arange(256, dtype=np.uint8)
    ap, op = a.data_ptr(), o.data_ptr()

    def dec(**k):
        v = dict(src=ap, sp=400, w=w, h=h, levels=4, interp=1, dst=op, dp=512, batch=1, sfs=400 * h, dfs=512 * h, c=ctx.handle)
        v.update(k)
        return L.hgi_decode_u8_pitched_dev(v["c"], v["src"], v["sp"], v["w"], v["h"], v["levels"], v["interp"], v["dst"], v["dp"], v["batch"],
                                           v["sfs"], v["dfs"])

    def enc(**k):
        v = dict(src=ap, sp=400, w=w, h=h, levels=4, interp=1, lut=lut.ctypes.data, dst=op, dp=512, batch=1, sfs=400 * h, dfs=512 * h,
                 c=ctx.handle)
        v.update(k)
        return L.hgi_encode_u8_pitched_dev(v["c"], v["src"], v["sp"], v["w"], v["h"], v["levels"], v["interp"], v["lut"], v["dst"], v["dp"],
                                           v["batch"], v["sfs"], v["dfs"])
    E = _ffi.EINVAL
    for call in (dec, enc):
        assert call() == _ffi.OK
        assert call(sp=299) == E and call(dp=299) == E and call(sp=300, dp=300) == _ffi.OK
        assert call(batch=2, sfs=199 * 400 + 299) == E and call(batch=2, sfs=199 * 400 + 300) == _ffi.OK
        assert call(batch=2, dfs=199 * 512 + 299) == E and call(batch=2, dfs=199 * 512 + 300) == _ffi.OK
        assert call(dst=ap + 5) == E and call(dst=ap - 50) == E and call(dst=ap + 199 * 400 + 299) == E
        assert call(dst=ap + 300, dp=400) == E      # two windows side by side in one parent: refused (conservative span test)
        assert call(src=0) == E and call(dst=0) == E
        assert call(levels=32) == E and call(interp=7) == _ffi.EUNSUPPORTED and call(c=None) == E
    assert enc(lut=None) == E
    torch.cuda.synchronize()
    o.fill_(SENT)
    torch.cuda.synchronize()
    for call in (dec, enc):
        assert call(batch=0) == _ffi.OK and call(w=0) == _ffi.OK and call(h=0) == _ffi.OK
    torch.cuda.synchronize()
    assert (o == SENT).all()
    lw = H.Context(0)
    lw.set_path(_ffi.PATH_LEVELWISE)
    assert dec(c=lw.handle) == _ffi.EUNSUPPORTED and b"LEVELWISE" in L.hgi_last_error()
    assert enc(c=lw.handle) == _ffi.EUNSUPPORTED
    lw.close()
    gh = np.zeros((h, 400), np.uint8)
    oh = np.zeros((h, 512), np.uint8)
    assert L.hgi_decode_u8_pitched(ctx.handle, gh.ctypes.data, 299, w, h, 4, 1, oh.ctypes.data, 512) == E
    assert L.hgi_encode_u8_pitched(ctx.handle, gh.ctypes.data, 400, w, h, 4, 1, lut.ctypes.data, oh.ctypes.data, 299) == E
    assert L.hgi_encode_u8_pitched(ctx.handle, gh.ctypes.data, 400, w, h, 4, 1, None, oh.ctypes.data, 512) == E
    assert L.hgi_decode_u8_pitched(ctx.handle, gh.ctypes.data, 400, w, h, 4, 9, oh.ctypes.data, 512) == _ffi.EUNSUPPORTED


def test_reserved_ctx_does_not_grow_and_graph_replay(H, oracle):
    """hgi_ctx_reserve(width, height, levels, batch) covers the pitched calls (the scratch does not grow); a torch.cuda.graph of a
    pitched encode followed by its decode -- one linear chain on one stream, scratch reserved first -- replays to the same bytes
    on new input."""
    import torch
    from rustyhgi_amd import _ffi
    L = _ffi.lib()
    w, h, B = 1300, 700, 2
    sp, gp, op = w + 61, w + 3, w + 128
    rng = np.random.default_rng(SEED0 + 11)
    lut = oracle.linear_lut(2)[0]
    for levels in (4, 8, 12):
        c = H.Context(0)
        _ffi.check(L.hgi_ctx_reserve(c.handle, w, h, levels, B))
        before = c.scratch_bytes()
        src = torch.from_numpy(rng.integers(0, 256, (B, h, sp), dtype=np.uint8)).cuda()
        grid = torch.full((B, h, gp), SENT, dtype=torch.uint8, device="cuda")
        out = torch.full((B, h, op), SENT, dtype=torch.uint8, device="cuda")
        c.set_stream(torch.cuda.current_stream().cuda_stream)

        def chain():
            _ffi.check(L.hgi_encode_u8_pitched_dev(c.handle, src.data_ptr(), sp, w, h, levels, 1, lut.ctypes.data, grid.data_ptr(), gp, B,
                                                   h * sp, h * gp))
            _ffi.check(L.hgi_decode_u8_pitched_dev(c.handle, grid.data_ptr(), gp, w, h, levels, 1, out.data_ptr(), op, B, h * gp, h * op))

        def check(what):
            hs, hg, ho = src.cpu().numpy(), grid.cpu().numpy(), out.cpu().numpy()
            for f in range(B):
                want = oracle.encode(hs[f, :, :w], levels, lut)
                assert_same(hg[f, :, :w], want, "%s L%d grid %d" % (what, levels, f))
                assert_same(ho[f, :, :w], oracle.decode(want, levels), "%s L%d image %d" % (what, levels, f))
            assert (hg[:, :, w:] == SENT).all() and (ho[:, :, w:] == SENT).all()
        chain()
        torch.cuda.synchronize()
        assert c.scratch_bytes() == before, "L%d: %d -> %d" % (levels, before, c.scratch_bytes())
        check("direct")
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            c.set_stream(side.cuda_stream)
            gr = torch.cuda.CUDAGraph()
            torch.cuda.synchronize()
            with torch.cuda.graph(gr, stream=side):
                chain()
        src.copy_(torch.from_numpy(rng.integers(0, 256, (B, h, sp), dtype=np.uint8)).cuda())
        torch.cuda.synchronize()
        gr.replay()
        torch.cuda.synchronize()
        check("graph replay")
        assert c.scratch_bytes() == before
        del gr
        c.close()


def test_large_batch_against_the_uniform_call(ctx):
    """64 windows of 4096 x 4096 inside parents of 4224 x 4160 (the P1 / P2 workload of DESIGN.md 4.9) and one 8192 x 8192 window
    at level 8: the oracle is too slow for these, so the expected bytes are the library's UNIFORM calls on the packed copy."""
    import torch
    from rustyhgi_amd import _ffi
    L = _ffi.lib()
    lut = np.ascontiguousarray(((np.arange(256) + 20) // 41 * 41).astype(np.uint8))
    for (w, h, pw, ph, B, levels) in ((4096, 4096, 4224, 4160, 64, 4), (8192, 8192, 8320, 8256, 1, 8)):
        parent = torch.empty((B, ph, pw), dtype=torch.uint8, device="cuda")
        _ffi.check(L.hgi_synth_u8_dev(ctx.handle, _ffi.SYNTH_NOISE, SEED0 + 41, 0, pw, ph, parent.data_ptr(), B, pw * ph))
        view = parent[:, 37:37 + h, 65:65 + w]
        packed = view.contiguous()
        g = torch.empty_like(packed)
        o = torch.empty_like(packed)
        _ffi.check(L.hgi_encode_u8_dev(ctx.handle, packed.data_ptr(), w, h, levels, 1, lut.ctypes.data, g.data_ptr(), B, w * h))
        _ffi.check(L.hgi_decode_u8_dev(ctx.handle, g.data_ptr(), w, h, levels, 1, o.data_ptr(), B, w * h))
        gp = torch.full((B, ph, pw), SENT, dtype=torch.uint8, device="cuda")
        _ffi.check(L.hgi_encode_u8_pitched_dev(ctx.handle, view.data_ptr(), pw, w, h, levels, 1, lut.ctypes.data,
                                               gp[:, 3:, 128:].data_ptr(), pw, B, pw * ph, pw * ph))
        torch.cuda.synchronize()
        assert torch.equal(gp[:, 3:3 + h, 128:128 + w], g), "%d x %d^2 L%d encode" % (B, w, levels)
        gp[:, 3:3 + h, 128:128 + w] = SENT
        assert bool((gp == SENT).all()), "encode wrote outside the window"
        gp[:, 3:3 + h, 128:128 + w] = g
        op = torch.full((B, ph, pw), SENT, dtype=torch.uint8, device="cuda")
        _ffi.check(L.hgi_decode_u8_pitched_dev(ctx.handle, gp[:, 3:, 128:].data_ptr(), pw, w, h, levels, 1, op[:, 1:, 7:].data_ptr(), pw, B,
                                               pw * ph, pw * ph))
        torch.cuda.synchronize()
        assert torch.equal(op[:, 1:1 + h, 7:7 + w], o), "%d x %d^2 L%d decode" % (B, w, levels)
        op[:, 1:1 + h, 7:7 + w] = SENT
        assert bool((op == SENT).all()), "decode wrote outside the window"
        del parent, view, packed, g, o, gp, op
        torch.cuda.empty_cache()


def test_cli_crop_equals_the_oracle_on_the_cropped_image(oracle, lena, tmp_path):
    """`hgi encode --crop X,Y,W,H`: the archive holds the oracle's grid of the cropped image and the window's size, and decodes
    to the oracle's decode of it; windows outside the image and malformed ones are refused."""
    exe = str(tmp_path / "hgi")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "cli", "hgi_cli.cpp"),
                           "-L", os.path.join(ROOT, "rustyhgi_amd"), "-lhgi_hip", "-lz", "-Wl,-rpath," + os.path.join(ROOT, "rustyhgi_amd"),
                           "-o", exe])
    with open(str(tmp_path / "in.pgm"), "wb") as f:
        f.write(b"P5\n256 256\n255\n" + lena.tobytes())
    run = lambda *a: subprocess.run([exe] + list(a), cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    from rustyhgi_amd import Archive
    for (x, y, w, h, levels) in ((10, 20, 150, 99, 5), (0, 0, 256, 256, 4), (255, 255, 1, 1, 3), (3, 0, 201, 256, 9)):
        r = run("encode", "-i", "in.pgm", "-o", "c.hgi", "-l", str(levels), "-q", "low", "--crop", "%d,%d,%d,%d" % (x, y, w, h))
        assert r.returncode == 0, r.stderr
        with open(str(tmp_path / "c.hgi"), "rb") as f:
            arc = Archive.deserialize_from_reader(f)
        assert (arc.metadata.width, arc.metadata.height, arc.metadata.scale_level) == (w, h, levels)
        want = oracle.encode(lena[y:y + h, x:x + w], levels, oracle.linear_lut(1)[0])
        assert_same(np.asarray(arc.grid.buffer, np.uint8).reshape(h, w), want, "cli --crop %r" % ((x, y, w, h),))
        r = run("decode", "-i", "c.hgi", "-o", "c.pgm")
        assert r.returncode == 0, r.stderr
        data = open(str(tmp_path / "c.pgm"), "rb").read()
        head = ("P5\n%d %d\n255\n" % (w, h)).encode()
        assert data.startswith(head)
        assert_same(np.frombuffer(data[len(head):], np.uint8).reshape(h, w), oracle.decode(want, levels), "decode of the cropped archive")
    for bad in ("0,0,257,1", "250,0,7,7", "0,0,0,5", "1,2,3", "a,b,c,d", "-1,0,5,5", "0,0,4294967296,1"):
        r = run("encode", "-i", "in.pgm", "-o", "bad.hgi", "--crop", bad)
        assert r.returncode != 0 and "--crop" in r.stderr, (bad, r.stderr)
    r = run("decode", "-i", "c.hgi", "-o", "c.pgm", "--crop", "0,0,1,1")
    assert r.returncode != 0      # --crop belongs to encode


def test_cpp_mirror_views(tmp_path):
    """include/hgi.hpp: Encoder::encode_view / Decoder::decode_view against encode / decode of the packed copy
    (tests/cpp/test_pitched_hpp.cpp)."""
    exe = str(tmp_path / "test_pitched_hpp")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_pitched_hpp.cpp"), "-L", os.path.join(ROOT, "rustyhgi_amd"), "-lhgi_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "rustyhgi_amd"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


FORCED_MODES = ["HGI_FORCE_CHECKED=1", "HGI_NO_LATTICE_KERNEL=1", "HGI_NO_LATTICE_KERNEL=1,HGI_FORCE_CHECKED=1"]


@pytest.mark.parametrize("mode", FORCED_MODES)
def test_forced_code_paths_in_a_child_process(mode):
    """The knobs build re-runs the small cases, one ragged shape, the depth routes and the level-0 copy with the byte-checked path
    and / or the host recursion for the lattice planes forced: the bytes must not change."""
    from rustyhgi_amd import _ffi
    knobs = os.path.join(os.path.dirname(_ffi.LIB_PATH), "libhgi_hip_knobs.so")
    assert os.path.exists(knobs)
    env = dict(os.environ, HGI_LIB_PATH=knobs, **dict(kv.split("=") for kv in mode.split(",")))
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(here, "test_pitched_gpu.py"), "-m", "gpu", "-q", "-x",
                        "-p", "no:cacheprovider", "-k",
                        "small_golden or 2049-1080 or 130-70 or every_depth_route or level_zero or aligned_pitch"],
                       env=env, capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, mode + "\n" + r.stdout[-3000:] + r.stderr[-1000:]
