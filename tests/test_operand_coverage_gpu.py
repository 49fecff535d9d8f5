"""GPU suite of the operand-coverage designs (tests/operand_designs.py; what they cover is asserted on the CPU in
tests/test_operand_coverage.py): every design goes through every entry point that has a kernel of its own and is compared with
the oracle bit for bit.  The quantizer designs put every (prediction, pixel) pair in front of every byte lane of the hand-written
quantizer step, the predictor designs every corner quadruple over the edge values in front of the packed averages; a mistake
confined to one lane at p = 255 or to one carry fails here and nowhere else in the suite.

One test case is (design, interpolator, part): `uniform` runs the *_dev calls on a fused and on a level-wise context (and is
what the forced-path children re-run on the knobs build), `variants` the pitched, list, reconstruction, region, scaled and
mapped kernels.  The oracle's grid and decode are computed once per (design, table, interpolator) and shared by both parts.
Outputs with a pitch are written into sentinel-filled parents that are checked whole; inputs with a pitch are read out of
parents of random bytes.  Expected bytes: the oracle.  Never the library under test."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import operand_designs as D

pytestmark = pytest.mark.gpu
SENT = 0xC3
TABLES = D.tables()
TABLES_PLUS = dict(TABLES, nonzero_origin=D.table_nonzero_origin())


def _designs():
    """name -> (frame name, levels, table names, targeted subs)."""
    out = {}
    for name, frame, lv, req in D.quant_designs():
        big = D.quant_frame(frame).size > 12e6
        out[name] = (frame, lv, ("linear2", "identity", "identity_but_255", "random0") if big else tuple(TABLES_PLUS), [s for s, _ in req])
    for frame, (lv, _) in D.PRED_FRAMES.items():
        out["%s_L%d" % (frame, lv)] = (frame, lv, ("identity", "linear2"), [1 << k for k in range(lv)])
    # the lattice kernel (nine levels and more): one design each at 9 and 12 levels
    out["q8_16_L9"] = ("q8_16", 9, ("linear2", "identity"), [8, 16])
    out["pred5_L12"] = ("pred5", 12, ("identity", "linear2"), [1 << k for k in range(5)])
    return out


DESIGNS = _designs()
CASES = [(d, i, part) for d in DESIGNS for i in (1, 0) for part in ("uniform", "variants")]


def frame_of(design):
    f = DESIGNS[design][0]
    return D.pred_frame(f) if f in D.PRED_FRAMES else D.quant_frame(f)


@functools.lru_cache(maxsize=8)
def expected(design, tname, interp):
    """(grid, decode) of the oracle, once per (design, table, interpolator): the two parts of a design run back to back."""
    from oracle import hgi_oracle as O
    O.build()
    _, levels, _, _ = DESIGNS[design]
    grid = O.encode(frame_of(design), levels, TABLES_PLUS[tname], interp)
    return grid, O.decode(grid, levels, interp)


@pytest.fixture(scope="module")
def H():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    import rustyhgi_amd
    from rustyhgi_amd import _ffi, _ffi_map, _ffi_recon
    assert _ffi.lib() is not None and _ffi_recon.lib() is not None and _ffi_map.lib() is not None      # no fallback exists
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
    and checked whole, an input plane holds random bytes around its rows.  `tail_w`: the row width of an input whose three
    bytes behind the span must share a 4-KiB page with its last byte (include/hgi_recon.h, include/hgi_map.h)."""

    def __init__(self, h, row, pitch, lead=0, random=False, seed=1, tail_w=None):
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
            if (end - 1) >> 12 != (end + 2) >> 12:
                self.lead += 4
            end = self.ptr + (h - 1) * pitch + tail_w
            assert (end - 1) >> 12 == (end + 2) >> 12

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


def run_narrowed(ctx, oracle, img, d_img, levels, interp, lut, what):
    """The sub 1 and sub 2 designs at width - 1 and width - 2, as views of the same rows: widths 3 and 2 mod 4 take the checked
    path in the core library and every `nvalid` class of the last chunk in the companions."""
    h, w = img.shape
    for k in (1, 2):
        cut = np.ascontiguousarray(img[:, :w - k])
        grid = oracle.encode(cut, levels, lut, interp)
        d_g, d_d = dev(grid), dev(oracle.decode(grid, levels, interp))
        name = "%s width-%d" % (what, k)
        run_pitched(ctx, d_img, d_g, d_d, levels, interp, lut, name, w=w - k, gaps=(k, k), leads=(0, 0))
        run_recon(d_img, d_g, d_d, levels, interp, lut, name, w=w - k)
        run_mapped(d_g, d_d, levels, interp, 2 * k, name)


@pytest.mark.parametrize("design,interp,part", CASES, ids=["%s-i%d-%s" % c for c in CASES])
def test_design_through_every_entry_point(H, ctxs, oracle, design, interp, part):
    """Every table of the design, one interpolator: `uniform` -- hgi_encode_u8_dev / hgi_decode_u8_dev on a fused and on a
    level-wise context; `variants` -- pitched, frame list, encode with reconstruction (grid and reconstruction), region (two
    windows at odd offsets), scaled at s = 1 and 2 where a targeted level survives the shift, mapped decode with E = 2 and 4
    and an injective table (reconstruction and mapping up to eight levels: their contract); the sub 1 and sub 2 designs also at
    width - 1 and width - 2 under two tables.  All against the oracle, bit for bit."""
    _, levels, tnames, subs = DESIGNS[design]
    img = frame_of(design)
    d_img = dev(img)
    fused = ctxs["fused"]
    for tname in tnames:
        lut = np.ascontiguousarray(TABLES_PLUS[tname])
        grid, dec = expected(design, tname, interp)
        d_grid, d_dec = dev(grid), dev(dec)
        what = "%s %s interp %d" % (design, tname, interp)
        if part == "uniform":
            run_uniform(ctxs, d_img, d_grid, d_dec, levels, interp, lut, what)
            continue
        run_pitched(fused, d_img, d_grid, d_dec, levels, interp, lut, what)
        run_list(fused, oracle, img, d_img, d_grid, d_dec, levels, interp, lut, what)
        run_region(fused, d_grid, d_dec, levels, interp, what)
        for shift in (1, 2):
            if max(subs) >= 1 << shift:
                run_scaled(fused, d_grid, d_dec, levels, interp, shift, what)
        if levels <= 8:
            run_recon(d_img, d_grid, d_dec, levels, interp, lut, what)
            for E in (2, 4):
                run_mapped(d_grid, d_dec, levels, interp, E, what)
        if design.startswith(("q1_", "q2_")) and tname in ("linear2", "identity"):
            run_narrowed(fused, oracle, img, d_img, levels, interp, lut, what)


# ------------------------------------------------------------------------------------ forced paths, knobs build
CHILD_MODES = ["HGI_FORCE_CHECKED=1", "HGI_TILE_H=64", "HGI_TILE_H=32", "HGI_TILE_H=16"]
_child_lost = []


@pytest.mark.parametrize("mode", CHILD_MODES)
def test_forced_code_paths_in_a_child_process(mode):
    """A child process on the KNOBS build re-runs this file's uniform cases with the checked path or one tile height forced (as
    tests/test_parity_gpu.py does for its shapes): the bytes must not depend on it.  Each child has its own timeout; once a
    child has ended by signal or timeout this test fails at once and starts no other."""
    from rustyhgi_amd import _ffi
    assert not _child_lost, "not started: the child under %s ended by signal or timeout" % _child_lost[0]
    knobs = os.path.join(os.path.dirname(_ffi.LIB_PATH), "libhgi_hip_knobs.so")
    assert os.path.exists(knobs), "libhgi_hip_knobs.so is missing: __graft_entry__.build() / `make -C rustyhgi_amd/csrc knobs` builds it"
    env = dict(os.environ, HGI_LIB_PATH=knobs, **dict(kv.split("=") for kv in mode.split(",")))
    cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider",
           "-k", "uniform"]
    try:
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    except subprocess.TimeoutExpired:
        _child_lost.append(mode)
        pytest.fail(mode + ": the child did not finish in 600 s")
    if r.returncode < 0:
        _child_lost.append(mode)
        pytest.fail("%s: the child ended by signal %d\n%s" % (mode, -r.returncode, r.stdout[-2000:] + r.stderr[-1000:]))
    assert r.returncode == 0, mode + "\n" + r.stdout[-3000:] + r.stderr[-1000:]
    assert "%d passed" % (len(CASES) // 2) in r.stdout, r.stdout[-500:]


# ------------------------------------------------------------------------------- graph capture, companion libraries
def test_companion_calls_replay_from_a_graph(H, oracle):
    """include/hgi_recon.h and include/hgi_map.h: "capturable into a graph".  One hgi_recon_encode_u8_dev and one
    hgi_map_decode_dev call (384 x 127, three levels, batch 2, a pitch on every side), each a single kernel, captured on a side
    stream into one graph -- a linear chain -- and replayed twice on pixels, grids and table contents written in place; every
    replay against the oracle, the sentinels around every output row intact."""
    import torch
    from rustyhgi_amd import _ffi_map as M, _ffi_recon as R
    w, h, levels, B, E = 384, 127, 3, 2, 4
    lut = np.ascontiguousarray(TABLES["linear2"])
    sp, gp, rp, mp, op = w + 16, w + 61, w + 128, w + 3, (w + 5) * E
    img = torch.zeros((B, h, sp), dtype=torch.uint8, device="cuda")
    grid = torch.full((B, h, gp), SENT, dtype=torch.uint8, device="cuda")
    rec = torch.full((B, h, rp), SENT, dtype=torch.uint8, device="cuda")
    mgrid = torch.zeros((B, h, mp), dtype=torch.uint8, device="cuda")
    out = torch.full((B, h, op), SENT, dtype=torch.uint8, device="cuda")
    d_table = torch.zeros((256,), dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()

    def chain(stream):
        R.check(R.lib().hgi_recon_encode_u8_dev(stream, img.data_ptr(), sp, w, h, levels, 1, lut.ctypes.data, grid.data_ptr(), gp,
                                                rec.data_ptr(), rp, B, h * sp, h * gp, h * rp))
        M.check(M.lib().hgi_map_decode_dev(stream, mgrid.data_ptr(), mp, w, h, levels, 1, d_table.data_ptr(), E, out.data_ptr(), op, B,
                                           h * mp, h * op))

    with torch.cuda.stream(side):
        chain(side.cuda_stream)          # both code objects loaded before the capture begins
        side.synchronize()
        grid.fill_(SENT)
        rec.fill_(SENT)
        out.fill_(SENT)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            chain(side.cuda_stream)
    rng = np.random.default_rng(0x48474934)
    for rep in range(2):
        pix = rng.integers(0, 256, (B, h, sp), dtype=np.uint8)
        grids = rng.integers(0, 256, (B, h, mp), dtype=np.uint8)
        table = injective_table(E, rep)
        img.copy_(dev(pix))
        mgrid.copy_(dev(grids))
        d_table.copy_(dev(table.view(np.int32)))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        hg, hr, ho = grid.cpu().numpy(), rec.cpu().numpy(), out.cpu().numpy()
        for f in range(B):
            want = oracle.encode(pix[f, :, :w], levels, lut, 1)
            assert_same(hg[f, :, :w], want, "replay %d grid %d" % (rep, f))
            assert_same(hr[f, :, :w], oracle.decode(want, levels, 1), "replay %d reconstruction %d" % (rep, f))
            dec = oracle.decode(np.ascontiguousarray(grids[f, :, :w]), levels, 1)
            assert_same(np.ascontiguousarray(ho[f, :, :w * E]).view(np.uint32), table[dec], "replay %d mapped %d" % (rep, f))
        assert (hg[:, :, w:] == SENT).all() and (hr[:, :, w:] == SENT).all() and (ho[:, :, w * E:] == SENT).all(), "replay %d: sentinels" % rep
        assert (img.cpu().numpy() == pix).all() and (mgrid.cpu().numpy() == grids).all(), "replay %d: an input was modified" % rep
    del g
