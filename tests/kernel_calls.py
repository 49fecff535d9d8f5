"""The calls of every entry point that has a kernel of its own, as the GPU coverage suites make them (a helper module of
tests/test_operand_coverage_gpu.py, tests/test_geometry_coverage_gpu.py, tests/test_tilewalk_gpu.py and
tests/test_element_coverage_gpu.py, not a conftest).
Outputs with a pitch are written into sentinel-filled parents that are checked whole; inputs with a pitch are read out of
parents of random bytes.  Device tensors are compared on the device; the host report is made only on a mismatch."""
import bisect
import ctypes
import functools

import numpy as np
import pytest

import typed_reference as TR

SENT = 0xC3
PAGE = 4096


@pytest.fixture(scope="module")
def H():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    import rustyhgi_amd
    from rustyhgi_amd import _ffi, _ffi_map, _ffi_recon, _ffi_typed
    assert _ffi.lib() is not None and _ffi_recon.lib() is not None and _ffi_map.lib() is not None      # no fallback exists
    assert _ffi_typed.lib() is not None
    return rustyhgi_amd


@pytest.fixture(scope="module")
def ctxs(H):
    import torch
    from rustyhgi_amd import _ffi
    fused, levelwise = H.Context(0), H.Context(0)
    levelwise.set_path(_ffi.PATH_LEVELWISE)
    for c in (fused, levelwise):
        c.set_stream(torch.cuda.current_stream().cuda_stream)
    yield {"fused": fused, "levelwise": levelwise}
    fused.close()
    levelwise.close()


def assert_same(a, b, what):
    if a.shape != b.shape:
        raise AssertionError("%s: shape %s, want %s" % (what, a.shape, b.shape))
    if not (a == b).all():
        bad = np.argwhere(a != b)
        y, x = bad[0][-2:]
        raise AssertionError("%s: %d mismatches, first at (x=%d, y=%d, x mod 16 = %d): got %d want %d"
                             % (what, len(bad), x, y, x % 16, a[tuple(bad[0])], b[tuple(bad[0])]))


def same_dev(got, want, what):
    """Device tensors compared on the device; the host report only on a mismatch."""
    import torch
    if got.shape != want.shape or not torch.equal(got, want):
        assert_same(got.cpu().numpy(), want.cpu().numpy(), what)


class Plane:
    """h rows of `row` bytes, `pitch` apart, `lead` bytes into a 1-D device buffer: an output plane is filled with the sentinel
    and checked whole, an input plane holds random bytes around its rows.  `tail_w`: the row width of an input whose `tail_n`
    bytes behind the span must share a 4-KiB page with its last byte (three: include/hgi_recon.h, include/hgi_map.h; two, for
    2-byte elements of an odd width: include/hgi_typed.h)."""

    def __init__(self, h, row, pitch, lead=0, random=False, seed=1, tail_w=None, tail_n=3):
        import torch
        self.h, self.row, self.pitch, self.lead = h, row, pitch, lead
        n = lead + (h - 1) * pitch + row + 64
        if random:
            gen = torch.Generator(device="cuda")
            gen.manual_seed(seed)
            self.buf = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda", generator=gen)
        else:
            self.buf = torch.full((n,), SENT, dtype=torch.uint8, device="cuda")
        if tail_w is not None and tail_w % 4:
            end = self.ptr + (h - 1) * pitch + tail_w
            if (end - 1) >> 12 != (end + tail_n - 1) >> 12:
                self.lead += 4
            end = self.ptr + (h - 1) * pitch + tail_w
            assert (end - 1) >> 12 == (end + tail_n - 1) >> 12

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.lead

    def rows(self, buf=None):
        import torch
        return torch.as_strided(self.buf if buf is None else buf, (self.h, self.row), (self.pitch, 1), self.lead)

    def put(self, t):
        self.rows().copy_(t)
        return self

    def intact(self, what):
        c = self.buf.clone()
        self.rows(c).fill_(SENT)
        assert bool((c == SENT).all()), what + ": bytes outside the output rows written"


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).cuda()


def call_list(ctx, encode, ins, outs, shapes, levels, interp, lut=None):
    from rustyhgi_amd import _ffi
    L, n = _ffi.lib(), len(shapes)
    pi, po = (ctypes.c_void_p * n)(*ins), (ctypes.c_void_p * n)(*outs)
    ws, hs = (ctypes.c_uint32 * n)(*[w for w, h in shapes]), (ctypes.c_uint32 * n)(*[h for w, h in shapes])
    if encode:
        _ffi.check(L.hgi_encode_u8_list_dev(ctx.handle, pi, ws, hs, levels, interp, lut.ctypes.data, po, n))
    else:
        _ffi.check(L.hgi_decode_u8_list_dev(ctx.handle, pi, ws, hs, levels, interp, po, n))


def injective_table(E, seed):
    rng = np.random.default_rng(seed + 1000 * E)
    if E == 2:
        return rng.permutation(1 << 16)[:256].astype(np.uint16)
    t = (rng.permutation(1 << 20)[:256].astype(np.uint32) << np.uint32(12)) | rng.integers(0, 4096, 256, dtype=np.uint32)
    assert len(np.unique(t)) == 256
    return t


# ------------------------------------------------------------------------------------------------ entry points
def run_uniform(ctxs, d_img, d_grid, d_dec, levels, interp, lut, what):
    import torch
    from rustyhgi_amd import _ffi
    L = _ffi.lib()
    h, w = d_img.shape
    for path in ("fused", "levelwise"):
        ctx = ctxs[path]
        out = torch.full_like(d_img, 0xA5)
        _ffi.check(L.hgi_encode_u8_dev(ctx.handle, d_img.data_ptr(), w, h, levels, interp, lut.ctypes.data, out.data_ptr(), 1, w * h))
        same_dev(out, d_grid, "%s %s encode" % (what, path))
        out.fill_(0x5A)
        _ffi.check(L.hgi_decode_u8_dev(ctx.handle, d_grid.data_ptr(), w, h, levels, interp, out.data_ptr(), 1, w * h))
        same_dev(out, d_dec, "%s %s decode" % (what, path))


def run_pitched(ctx, d_img, d_grid, d_dec, levels, interp, lut, what, w=None, gaps=(61, 3), leads=(3, 16)):
    """Encode and decode of the first `w` columns through pitches (w = None: the whole frame)."""
    from rustyhgi_amd import _ffi
    L = _ffi.lib()
    h, full = d_img.shape
    w = w or full
    src = Plane(h, w, w + gaps[0], leads[0], random=True, seed=levels).put(d_img[:, :w])
    dst = Plane(h, w, w + gaps[1], leads[1])
    _ffi.check(L.hgi_encode_u8_pitched_dev(ctx.handle, src.ptr, src.pitch, w, h, levels, interp, lut.ctypes.data, dst.ptr, dst.pitch, 1,
                                           h * src.pitch, h * dst.pitch))
    same_dev(dst.rows(), d_grid, what + " pitched encode")
    dst.intact(what + " pitched encode")
    src = Plane(h, w, w + gaps[1], leads[1], random=True, seed=levels + 1).put(d_grid)
    dst = Plane(h, w, w + gaps[0], leads[0])
    _ffi.check(L.hgi_decode_u8_pitched_dev(ctx.handle, src.ptr, src.pitch, w, h, levels, interp, dst.ptr, dst.pitch, 1,
                                           h * src.pitch, h * dst.pitch))
    same_dev(dst.rows(), d_dec, what + " pitched decode")
    dst.intact(what + " pitched decode")


def run_list(ctx, oracle, img, d_img, d_grid, d_dec, levels, interp, lut, what):
    """The frame and an odd-sized cut of it as one list of two."""
    h, w = img.shape
    h2, w2 = min(h, 131), min(w, 517)
    cut = np.ascontiguousarray(img[:h2, :w2])
    g2 = oracle.encode(cut, levels, lut, interp)
    d2 = oracle.decode(g2, levels, interp)
    shapes = [(w, h), (w2, h2)]
    for encode, ins, wants in ((True, [d_img, dev(cut)], [d_grid, dev(g2)]), (False, [d_grid, dev(g2)], [d_dec, dev(d2)])):
        outs = [Plane(1, ww * hh, ww * hh, lead) for (ww, hh), lead in zip(shapes, (7, 1))]
        call_list(ctx, encode, [t.data_ptr() for t in ins], [o.ptr for o in outs], shapes, levels, interp, lut)
        for k, (o, want) in enumerate(zip(outs, wants)):
            name = "%s list %s frame %d" % (what, "encode" if encode else "decode", k)
            same_dev(o.rows().reshape(want.shape), want, name)
            o.intact(name)


def run_recon(d_img, d_grid, d_dec, levels, interp, lut, what, w=None):
    import torch
    from rustyhgi_amd import _ffi_recon as R
    h, full = d_img.shape
    w = w or full
    src = Plane(h, w, w + 16, 5, random=True, seed=levels, tail_w=w).put(d_img[:, :w])
    grid, rec = Plane(h, w, w + 61, 1), Plane(h, w, w + 128, 16)
    R.check(R.lib().hgi_recon_encode_u8_dev(torch.cuda.current_stream().cuda_stream or None, src.ptr, src.pitch, w, h, levels, interp,
                                            lut.ctypes.data, grid.ptr, grid.pitch, rec.ptr, rec.pitch, 1, h * src.pitch,
                                            h * grid.pitch, h * rec.pitch))
    same_dev(grid.rows(), d_grid, what + " recon grid")
    same_dev(rec.rows(), d_dec, what + " recon reconstruction")
    grid.intact(what + " recon grid")
    rec.intact(what + " recon reconstruction")


def run_region(ctx, d_grid, d_dec, levels, interp, what):
    """Two windows that cut the blocks at odd offsets; the second touches the right and bottom edges."""
    from rustyhgi_amd import _ffi
    h, w = d_grid.shape
    x1, y1 = min(37, w - 1), min(21, h - 1)
    rects = [(x1, y1, min(w - x1, 1001), min(h - y1, 333)), (w // 2 + 1, h // 2 + 3, w - w // 2 - 1, h - h // 2 - 3)]
    for (x0, y0, rw, rh) in rects:
        out = Plane(rh, rw, rw + 5, 3)
        _ffi.check(_ffi.lib().hgi_decode_region_u8_dev(ctx.handle, d_grid.data_ptr(), w, h, levels, interp, x0, y0, rw, rh, out.ptr,
                                                       out.pitch, 1, w * h, rh * out.pitch))
        name = "%s region %r" % (what, (x0, y0, rw, rh))
        same_dev(out.rows(), d_dec[y0:y0 + rh, x0:x0 + rw], name)
        out.intact(name)


def run_scaled(ctx, d_grid, d_dec, levels, interp, shift, what):
    from rustyhgi_amd import _ffi
    h, w = d_grid.shape
    sw, sh = -(-w >> shift), -(-h >> shift)
    out = Plane(sh, sw, sw + 13, 1)
    _ffi.check(_ffi.lib().hgi_decode_scaled_u8_dev(ctx.handle, d_grid.data_ptr(), w, h, levels, interp, shift, out.ptr, out.pitch, 1,
                                                   w * h, sh * out.pitch))
    name = "%s scaled s=%d" % (what, shift)
    same_dev(out.rows(), d_dec[::1 << shift, ::1 << shift], name)
    out.intact(name)


def run_mapped(d_grid, d_dec, levels, interp, E, what, w=None):
    import torch
    from rustyhgi_amd import _ffi_map as M
    h, full = d_grid.shape
    w = w or full
    table = injective_table(E, levels)
    d_table = dev(table.view({2: np.int16, 4: np.int32}[E]))
    src = Plane(h, w, w + 3, 2, random=True, seed=levels + E, tail_w=w).put(d_grid[:, :w])
    out = Plane(h, w * E, (w + 16) * E, 2 * E)
    M.check(M.lib().hgi_map_decode_dev(torch.cuda.current_stream().cuda_stream or None, src.ptr, src.pitch, w, h, levels, interp,
                                       d_table.data_ptr(), E, out.ptr, out.pitch, 1, h * src.pitch, h * out.pitch))
    want = d_table[d_dec.long()]
    got = out.rows().contiguous().view(d_table.dtype)
    name = "%s mapped E=%d" % (what, E)
    if not torch.equal(got, want):
        assert_same(got.cpu().numpy(), want.cpu().numpy(), name)
    out.intact(name)


# typed encode: element size -> kinds, kind -> elem_kind of the ABI; the (scale, bias) pairs of the coverage suites.  Under
# (1, 37.25) the element 0.0 means pixel 37, under (-3.5, 300) pixel 255; bfloat16 reaches 224 of the 256 values under the
# latter (tests/test_typed_coverage.py), so it runs under the former alone.
F16, BF16, F32 = "float16", "bfloat16", "float32"
EKIND = {F16: 0, BF16: 1, F32: 0}
ESIZE = {F16: 2, BF16: 2, F32: 4}
PAIR_A, PAIR_B = (1.0, 37.25), (-3.5, 300.0)


def typed_choice(E, n):
    """(kind, pair) of the n-th typed frame of E-byte elements: 2-byte kinds alternate float16 / bfloat16, the pairs alternate
    where the kind allows both."""
    if E == 4:
        return F32, (PAIR_A, PAIR_B)[n % 2]
    return (F16, (PAIR_A, PAIR_B)[(n // 2) % 2]) if n % 2 == 0 else (BF16, PAIR_A)


TYPED_CHOICES = tuple(sorted({typed_choice(E, n) for E in (2, 4) for n in range(4)}))


@functools.lru_cache(maxsize=None)
def bank(kind, pair):
    """tests/typed_reference.py:preimages, read-only (its condition is asserted in tests/test_typed_coverage.py)."""
    b = TR.preimages(kind, *pair)
    b.setflags(write=False)
    return b


@functools.lru_cache(maxsize=None)
def bank_dev(kind, pair):
    return dev(bank(kind, pair).view({2: np.int16, 4: np.int32}[ESIZE[kind]]))


def lift_dev(d_img_u8, kind, pair, salt=0):
    """The design lifted on the device (indexing of the uploaded bank: plumbing): element bit patterns, int16 / int32."""
    return TR.lift(d_img_u8, bank_dev(kind, pair), salt)


def run_typed(d_img_u8, d_grid, levels, interp, lut, E, kind, pair, what, w=None, lifted=None):
    """hgi_typed_encode_dev on the first `w` columns of the design lifted to `kind` elements under the (scale, bias) `pair`
    (`lifted`: the whole design lifted already -- it does not depend on the table).  The frame sits in a parent of random
    bytes, so the gap elements are arbitrary bit patterns, NaN and infinity included."""
    import torch
    from rustyhgi_amd import _ffi_typed as T
    assert ESIZE[kind] == E
    h, full = d_img_u8.shape
    w = w or full
    if lifted is None:
        lifted = lift_dev(d_img_u8, kind, pair)
    src = Plane(h, w * E, (w + 3) * E, 3 * E, random=True, seed=levels + E, tail_w=w * E if E == 2 and w % 2 else None, tail_n=2)
    src.put(lifted[:, :w].contiguous().view(torch.uint8))
    before = src.buf.clone()
    dst = Plane(h, w, w + 61, 5)
    T.check(T.lib().hgi_typed_encode_dev(torch.cuda.current_stream().cuda_stream or None, src.ptr, src.pitch, E, EKIND[kind], pair[0], pair[1],
                                         w, h, levels, interp, lut.ctypes.data, dst.ptr, dst.pitch, 1, h * src.pitch, h * dst.pitch))
    name = "%s typed %s x %r + %r" % (what, kind, pair[0], pair[1])
    same_dev(dst.rows(), d_grid, name)
    dst.intact(name)
    assert torch.equal(src.buf, before), name + ": the image parent was modified"


def run_typed_raw(d_bits, d_want, kind, pair, levels, interp, lut, what, gap=3, lead=3, extra=5, seed=0):
    """hgi_typed_encode_dev on a batch of frames given as element bit patterns, taken as they are (run_typed lifts a uint8 design
    through finite pre-images; this one serves frames that hold NaN, infinities and denormals on purpose).  `d_bits`: (B, h, w)
    int16 / int32 on the device; `d_want`: the (B, h, w) expected grids.  The frames sit `lead` elements into a parent of random
    bytes, rows `gap` elements and frames `extra` elements further apart than they need be; the grids go into a sentinel-filled
    parent, rows and frames apart likewise, that is checked whole; the image parent must come back unchanged.  2-byte elements
    of an odd width are kept off a page's end (the page rule of include/hgi_typed.h)."""
    import torch
    from rustyhgi_amd import _ffi_typed as T
    E = ESIZE[kind]
    B, h, w = d_bits.shape
    assert d_bits.element_size() == E and tuple(d_want.shape) == (B, h, w)
    pitch = (w + gap) * E
    span = (h - 1) * pitch + w * E
    fs = span + extra * E
    gp = w + 61
    gspan = (h - 1) * gp + w
    gfs = gspan + 7
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed + 1)
    buf = torch.randint(0, 256, (lead * E + (B - 1) * fs + span + 72,), dtype=torch.uint8, device="cuda", generator=gen)
    off = lead * E
    if E == 2 and w % 2 and (buf.data_ptr() + off + (B - 1) * fs + span) % PAGE == 0:
        off += 4
    assert (buf.data_ptr() + off) % E == 0
    torch.as_strided(buf, (B, h, w * E), (fs, pitch, 1), off).copy_(d_bits.contiguous().view(torch.uint8).reshape(B, h, w * E))
    before = buf.clone()
    glead = 5
    out = torch.full((glead + (B - 1) * gfs + gspan + 64,), SENT, dtype=torch.uint8, device="cuda")
    T.check(T.lib().hgi_typed_encode_dev(torch.cuda.current_stream().cuda_stream or None, buf.data_ptr() + off, pitch, E, EKIND[kind], pair[0], pair[1],
                                         w, h, levels, interp, lut.ctypes.data, out.data_ptr() + glead, gp, B, fs, gfs))
    name = "%s typed %s x %r + %r L%d" % (what, kind, pair[0], pair[1], levels)
    same_dev(torch.as_strided(out, (B, h, w), (gfs, gp, 1), glead), d_want, name)
    c = out.clone()
    torch.as_strided(c, (B, h, w), (gfs, gp, 1), glead).fill_(SENT)
    assert bool((c == SENT).all()), name + ": bytes outside the grid rows written"
    assert torch.equal(buf, before), name + ": the image parent was modified"


def run_narrowed(ctx, oracle, img, d_img, levels, interp, lut, what, typed=None):
    """The sub 1 and sub 2 designs at width - 1 and width - 2, as views of the same rows: widths 3 and 2 mod 4 take the checked
    path in the core library and every `nvalid` class of the last chunk in the companions.  `typed`: {E: (kind, pair, lifted
    design)} -- the typed call at both widths and element sizes, so also odd widths of 2-byte elements."""
    h, w = img.shape
    for k in (1, 2):
        cut = np.ascontiguousarray(img[:, :w - k])
        grid = oracle.encode(cut, levels, lut, interp)
        d_g, d_d = dev(grid), dev(oracle.decode(grid, levels, interp))
        name = "%s width-%d" % (what, k)
        run_pitched(ctx, d_img, d_g, d_d, levels, interp, lut, name, w=w - k, gaps=(k, k), leads=(0, 0))
        run_recon(d_img, d_g, d_d, levels, interp, lut, name, w=w - k)
        run_mapped(d_g, d_d, levels, interp, 2 * k, name)
        for E, (kind, pair, lifted) in sorted((typed or {}).items()):
            run_typed(d_img, d_g, levels, interp, lut, E, kind, pair, name, w=w - k, lifted=lifted)


class Pool:
    """Byte ranges of one device buffer whose first byte lies on a 4-KiB page boundary, planned on the host.  An OUTPUT pool is
    filled with the sentinel and compared whole with its expected image; an INPUT pool holds nonzero random bytes around its
    rows and must come back unchanged."""

    def __init__(self, output, seed=0):
        self.output, self.seed, self.n, self.items, self.offs = output, seed, 64, [], []

    def add(self, data, pitch=None, stride=None, lead=0, align=1, end_mod=None, tail_safe=False, tag=None, phase=None):
        """data: (frames, h, row bytes).  Returns the offset of frame 0's first byte.  end_mod: the batch ends at this offset
        of its page; tail_safe: the three bytes behind the batch lie in the page of its last byte (rows that are not a multiple
        of 4 bytes: the contract of the companion calls; it serves the two tail bytes of typed encode too, whose last allowed
        placement is end_mod = PAGE - 2: the tail records are then the page's last two bytes).  phase: the offset modulo 16 (a
        multiple of `align`), kept by tail_safe; an end_mod moves it by a multiple of `align`."""
        frames, h, row = data.shape
        pitch = row if pitch is None else pitch
        stride = h * pitch if stride is None else stride
        assert pitch >= row and (frames == 1 or stride >= (h - 1) * pitch + row)
        span = (frames - 1) * stride + (h - 1) * pitch + row
        off = -(-(self.n + lead) // align) * align
        if phase is not None:
            assert phase % align == 0 and 16 % align == 0
            off += (phase - off) % 16
        if end_mod is not None:
            assert (end_mod - span) % align == 0
            off += (end_mod - (off + span)) % PAGE
        if tail_safe:
            while (off + span) % PAGE in (0, PAGE - 2, PAGE - 1):
                off += 4 if phase is None else 16
        assert off % align == 0
        self.items.append((off, span, data, pitch, stride, tag))
        self.offs.append(off)
        self.n = off + span + 7
        return off

    def upload(self):
        import torch
        host = self.image()
        n = host.size
        self.host = host
        self.want = torch.from_numpy(host).cuda()
        raw = torch.empty(n + PAGE, dtype=torch.uint8, device="cuda")
        shift = (-raw.data_ptr()) % PAGE
        self.buf = raw[shift:shift + n]
        if self.output:
            self.buf.fill_(SENT)
        else:
            self.buf.copy_(self.want)
        self.ptr = self.buf.data_ptr()
        assert self.ptr % PAGE == 0
        return self

    def image(self):
        """The expected bytes of the whole buffer (output), or its contents (input)."""
        n = self.n + 64
        # (input: a seeded bank of nonzero bytes, repeated at a period that is no multiple of any pitch or page)
        host = np.full(n, SENT, np.uint8) if self.output else np.resize(np.random.default_rng(0x48474941 + self.seed).integers(1, 256, 1000003, dtype=np.uint8), n)
        for off, span, data, pitch, stride, _ in self.items:
            frames, h, row = data.shape
            np.lib.stride_tricks.as_strided(host[off:], (frames, h, row), (stride, pitch, 1))[...] = data
        return host

    def check(self, what):
        import torch
        if torch.equal(self.buf, self.want):
            return
        got = self.buf.cpu().numpy()
        at = int(np.flatnonzero(got != self.host)[0])
        nbad = int((got != self.host).sum())
        if not self.output:
            raise AssertionError("%s: %d input bytes modified, first at offset %d" % (what, nbad, at))
        k = bisect.bisect_right(self.offs, at) - 1
        if k >= 0:
            off, span, data, pitch, stride, tag = self.items[k]
            frames, h, row = data.shape
            rel = at - off
            f, y, x = rel // stride if frames > 1 else 0, (rel % stride if frames > 1 else rel) // pitch, (rel % stride if frames > 1 else rel) % pitch
            if rel < span and f < frames and y < h and x < row:
                raise AssertionError("%s %s: %d mismatching bytes in the case, first in frame %d at (x=%d, y=%d, x mod 16 = %d) of %d-byte rows: got %d want %d"
                                     % (what, tag, nbad, f, x, y, x % 16, row, got[at], self.host[at]))
            raise AssertionError("%s: bytes outside the output rows written, first %d bytes behind the start of %s (frame %d, row %d, byte %d of a pitch of %d): %d"
                                 % (what, rel, tag, f, y, x, pitch, got[at]))
        raise AssertionError("%s: byte %d in front of the first output written" % (what, at))
