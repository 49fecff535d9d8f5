"""GPU suite of the geometry-coverage designs (tests/geometry_designs.py; what they cover is asserted on the CPU in
tests/test_geometry_coverage.py): every shape of the remainder sets R1 and R0 -- every column remainder 1 ... 127 and every row
remainder 1 ... 63 of a ragged tile, with and without an interior neighbour -- and of the deep set D goes through every entry
point that has a kernel of its own and is compared with the oracle bit for bit.  A store mask that is wrong for one
`cols mod 16` on an odd last row of one kernel fails here and nowhere else in the suite.

One test case is (family, set, levels, table, interpolator): a few thousand tiny launches.  All outputs of a case lie in ONE
sentinel-filled device buffer, at their own leads and pitches, and the buffer is compared whole with its expected image on the
device (the host is asked only on a mismatch); all inputs lie in one buffer of nonzero random bytes -- pixels are noise in
[8, 255], so no byte a kernel may wrongly read is 0, the out-of-image value -- which must come back unchanged.  The oracle's
grids and decodes are computed once per (set, levels, table, interpolator) and shared by the families, which run back to back.
The family `typed` feeds hgi_typed_encode_dev the same pixels lifted to float16 / bfloat16 / float32 elements
(tests/typed_reference.py:preimages) under (scale, bias) pairs for which the element 0.0 is not pixel 0.
Expected bytes: the oracle.  Never the library under test."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import geometry_designs as G
import typed_reference as TR
from kernel_calls import EKIND, PAGE, H, Pool, bank, call_list, ctxs, injective_table, typed_choice  # noqa: F401

pytestmark = pytest.mark.gpu
FAMILIES = ("uniform", "pitched", "list", "recon", "mapped", "typed", "scaled", "region")


def tables():
    from oracle import hgi_numpy as N
    return {"identity": np.arange(256, dtype=np.uint8), "linear2": N.linear_lut(2)[0],
            "random": np.random.default_rng(0x48474942).integers(0, 256, 256, dtype=np.uint8)}


TABLES = tables()


def _keys():
    """(set, levels, table, interpolator): R1 and R0 at 1, 2, 4 and 5 levels under Crossed and the identity, at 4 levels also
    linear_lut(2), a random table and LeftTop; D at 6, 7, 8, 9 and 12 levels under Crossed, the identity and linear_lut(2)."""
    keys = [("R", lv, "identity", 1) for lv in (1, 2, 4, 5)]
    keys += [("R", 4, "linear2", 1), ("R", 4, "random", 1), ("R", 4, "identity", 0)]
    keys += [("D", lv, t, 1) for lv in (6, 7, 8, 9, 12) for t in ("identity", "linear2")]
    return keys


# reconstruction, mapped decode and typed encode take up to eight levels: their contract
CASES = [(fam,) + key for key in _keys() for fam in FAMILIES if not (fam in ("recon", "mapped", "typed") and key[1] > 8)]


@functools.lru_cache(maxsize=4)
def expected(setname, levels, tname, interp):
    """[(w, h, pixels, grid, decode)] with two frames each, (2, h, w): the oracle, once per key."""
    from oracle import hgi_oracle as O
    O.build()
    lut = TABLES[tname]
    out = []
    for w, h in G.shape_set(setname):
        img = G.content(w, h, batch=2)
        if levels <= 0:
            out.append((w, h, img, img, img))
            continue
        grid = np.stack([O.encode(img[f], levels, lut, interp) for f in range(2)])
        out.append((w, h, img, grid, np.stack([O.decode(grid[f], levels, interp) for f in range(2)])))
    return out


def _odd(v):
    return v | 1


# ------------------------------------------------------------------------------------------------ the families
def fam_uniform(ctxs, E, levels, interp, lut, what):
    """hgi_encode_u8_dev / hgi_decode_u8_dev on a fused and on a level-wise context: batch 2, frames W * H + 5 apart.  Rows that
    are not a multiple of 4 bytes run at both placements of tests/test_parity_gpu.py::test_odd_width_tail_guard: the batch ends
    in mid-page (the tail path) and exactly on a page end (the byte-checked path)."""
    from rustyhgi_amd import _ffi
    L = _ffi.lib()
    inp, out, calls = Pool(False, levels), Pool(True), []
    for w, h, img, grid, dec in E:
        st = w * h + 5
        for end_mod in (2048, 0) if w % 4 else (2048,):
            i_img = inp.add(img.reshape(2, 1, -1), stride=st, lead=3, end_mod=end_mod)
            i_grid = inp.add(grid.reshape(2, 1, -1), stride=st, lead=1, end_mod=end_mod)
            for path in ("fused", "levelwise"):
                tag = "%d x %d %s, batch ends at %d of its page" % (w, h, path, end_mod)
                calls.append((ctxs[path].handle, w, h, st, i_img, i_grid, out.add(grid.reshape(2, 1, -1), stride=st, lead=5, tag=tag + " encode"),
                              out.add(dec.reshape(2, 1, -1), stride=st, lead=2, tag=tag + " decode")))
    inp.upload(), out.upload()
    for hd, w, h, st, i_img, i_grid, o_enc, o_dec in calls:
        _ffi.check(L.hgi_encode_u8_dev(hd, inp.ptr + i_img, w, h, levels, interp, lut.ctypes.data, out.ptr + o_enc, 2, st))
        _ffi.check(L.hgi_decode_u8_dev(hd, inp.ptr + i_grid, w, h, levels, interp, out.ptr + o_dec, 2, st))
    out.check(what), inp.check(what)
    return 2 * len(calls)


def fam_pitched(ctxs, E, levels, interp, lut, what):
    """hgi_encode_u8_pitched_dev / hgi_decode_u8_pitched_dev: batch 2, a different odd pitch and lead on the two sides."""
    from rustyhgi_amd import _ffi
    L, hd = _ffi.lib(), ctxs["fused"].handle
    inp, out, calls = Pool(False, levels + 100), Pool(True), []
    for w, h, img, grid, dec in E:
        pa, pb = _odd(w + 61), _odd(w + 3)
        sa, sb = h * pa + 7, h * pb + 1
        tag = "%d x %d pitches %d / %d" % (w, h, pa, pb)
        calls.append((w, h, pa, pb, sa, sb, inp.add(img, pa, sa, lead=3), out.add(grid, pb, sb, lead=17, tag=tag + " encode"),
                      inp.add(grid, pb, sb, lead=17), out.add(dec, pa, sa, lead=3, tag=tag + " decode")))
    inp.upload(), out.upload()
    for w, h, pa, pb, sa, sb, i_img, o_enc, i_grid, o_dec in calls:
        _ffi.check(L.hgi_encode_u8_pitched_dev(hd, inp.ptr + i_img, pa, w, h, levels, interp, lut.ctypes.data, out.ptr + o_enc, pb, 2, sa, sb))
        _ffi.check(L.hgi_decode_u8_pitched_dev(hd, inp.ptr + i_grid, pb, w, h, levels, interp, out.ptr + o_dec, pa, 2, sb, sa))
    out.check(what), inp.check(what)
    return 2 * len(calls)


def fam_list(ctxs, E, levels, interp, lut, what):
    """hgi_encode_u8_list_dev / hgi_decode_u8_list_dev: ALL frames of the set in one call per direction, so that the list
    kernels' per-frame tables hold every shape at once; every output at a lead of its own."""
    inp, out = Pool(False, levels + 200), Pool(True)
    shapes = [(w, h) for w, h, _, _, _ in E]
    i_img = [inp.add(img[:1].reshape(1, 1, -1), lead=k % 7) for k, (_, _, img, _, _) in enumerate(E)]
    i_grid = [inp.add(grid[:1].reshape(1, 1, -1), lead=k % 5) for k, (_, _, _, grid, _) in enumerate(E)]
    o_enc = [out.add(grid[:1].reshape(1, 1, -1), lead=1 + k % 13, tag="%d x %d (frame %d of the list) encode" % (w, h, k)) for k, (w, h, _, grid, _) in enumerate(E)]
    o_dec = [out.add(dec[:1].reshape(1, 1, -1), lead=1 + k % 11, tag="%d x %d (frame %d of the list) decode" % (w, h, k)) for k, (w, h, _, _, dec) in enumerate(E)]
    inp.upload(), out.upload()
    call_list(ctxs["fused"], True, [inp.ptr + o for o in i_img], [out.ptr + o for o in o_enc], shapes, levels, interp, lut)
    call_list(ctxs["fused"], False, [inp.ptr + o for o in i_grid], [out.ptr + o for o in o_dec], shapes, levels, interp, lut)
    out.check(what), inp.check(what)
    return 2


def fam_recon(ctxs, E, levels, interp, lut, what):
    """hgi_recon_encode_u8_dev, both outputs: batch 2, a pitch on every side, the input placed as the contract asks for rows that
    are not a multiple of 4 bytes."""
    import torch
    from rustyhgi_amd import _ffi_recon as R
    stream = torch.cuda.current_stream().cuda_stream or None
    inp, out, calls = Pool(False, levels + 300), Pool(True), []
    for w, h, img, grid, dec in E:
        ps, pg, pr = w + 16, w + 61, w + 128
        ss, sg, sr = h * ps + 3, h * pg + 1, h * pr + 5
        tag = "%d x %d" % (w, h)
        calls.append((w, h, ps, pg, pr, ss, sg, sr, inp.add(img, ps, ss, lead=5, tail_safe=w % 4 != 0), out.add(grid, pg, sg, lead=1, tag=tag + " recon grid"),
                      out.add(dec, pr, sr, lead=16, tag=tag + " recon reconstruction")))
    inp.upload(), out.upload()
    for w, h, ps, pg, pr, ss, sg, sr, i_img, o_grid, o_rec in calls:
        R.check(R.lib().hgi_recon_encode_u8_dev(stream, inp.ptr + i_img, ps, w, h, levels, interp, lut.ctypes.data, out.ptr + o_grid, pg,
                                                out.ptr + o_rec, pr, 2, ss, sg, sr))
    out.check(what), inp.check(what)
    return len(calls)


def fam_mapped(ctxs, E, levels, interp, lut, what):
    """hgi_map_decode_dev with 2- and 4-byte elements and an injective table: batch 2, a pitch on both sides."""
    import torch
    from rustyhgi_amd import _ffi_map as M
    stream = torch.cuda.current_stream().cuda_stream or None
    n = 0
    for esz in (2, 4):
        table = injective_table(esz, levels)
        d_table = torch.from_numpy(table.view({2: np.int16, 4: np.int32}[esz]).copy()).cuda()
        inp, out, calls = Pool(False, levels + 400 + esz), Pool(True), []
        for w, h, img, grid, dec in E:
            ps, po = w + 3, (w + 16) * esz
            ss, so = h * ps + 2, h * po + 4 * esz
            want = np.ascontiguousarray(table[dec]).view(np.uint8).reshape(2, h, w * esz)
            calls.append((w, h, ps, po, ss, so, inp.add(grid, ps, ss, lead=2, tail_safe=w % 4 != 0),
                          out.add(want, po, so, lead=2 * esz, align=esz, tag="%d x %d mapped E=%d" % (w, h, esz))))
        inp.upload(), out.upload()
        for w, h, ps, po, ss, so, i_grid, o in calls:
            M.check(M.lib().hgi_map_decode_dev(stream, inp.ptr + i_grid, ps, w, h, levels, interp, d_table.data_ptr(), esz, out.ptr + o, po, 2, ss, so))
        out.check(what), inp.check(what)
        n += len(calls)
    return n


@functools.lru_cache(maxsize=4)
def lifted_set(setname, esz):
    """[(kind, (scale, bias), (2, h, w * esz) bytes)] for every shape of the set: its content lifted to elements that convert to
    exactly that content (tests/typed_reference.py:preimages; the condition is asserted in tests/test_typed_coverage.py).  Kind and
    pair go by the shape's index: float16 / bfloat16 alternate, and so do the pairs where the kind allows both.  Once per (set,
    element size): the frames depend on neither the depth nor the table."""
    out = []
    for k, (w, h) in enumerate(G.shape_set(setname)):
        kind, pair = typed_choice(esz, k)
        frames = TR.lift(G.content(w, h, batch=2), bank(kind, pair), k)
        out.append((kind, pair, np.ascontiguousarray(frames).view(np.uint8).reshape(2, h, w * esz)))
    return out


def typed_cases(E, lifted, esz, levels, interp, lut, what, seed):
    """One pool of inputs, one of outputs and the calls of hgi_typed_encode_dev for the shapes of E (batch 2).  By shape index:
    the image gap cycles through 1, 3, 16 and 61 elements and the first row's address through every multiple of the element
    size below 16, so that row starts take every 16-byte phase; frame strides lie above the span on both sides; the grid is
    placed as fam_pitched places it.  2-byte elements of an odd width read two bytes behind the last frame's span
    (include/hgi_typed.h): they are placed tail_safe, every eighth of them with its span ending 2 bytes before a page end, the
    last placement the contract serves."""
    import torch
    from rustyhgi_amd import _ffi_typed as T
    stream = torch.cuda.current_stream().cuda_stream or None
    inp, out, calls, n_odd = Pool(False, seed), Pool(True), [], 0
    for k, ((w, h, img, grid, dec), (kind, pair, frames)) in enumerate(zip(E, lifted)):
        assert frames.shape == (2, h, w * esz)
        pi, pg = (w + (1, 3, 16, 61)[k % 4]) * esz, _odd(w + 3)
        si, sg = h * pi + 2 * esz, h * pg + 1
        place = {}
        if esz == 2 and w % 2:
            n_odd += 1
            place = dict(end_mod=PAGE - 2) if n_odd % 8 == 0 else dict(tail_safe=True)
        tag = "%d x %d typed %s x %r + %r" % (w, h, kind, pair[0], pair[1])
        calls.append((w, h, EKIND[kind], pair, pi, pg, si, sg, inp.add(frames, pi, si, align=esz, phase=esz * (k % (16 // esz)), **place),
                      out.add(grid, pg, sg, lead=17, tag=tag)))
    inp.upload(), out.upload()
    for w, h, ekind, pair, pi, pg, si, sg, i_img, o in calls:
        T.check(T.lib().hgi_typed_encode_dev(stream, inp.ptr + i_img, pi, esz, ekind, pair[0], pair[1], w, h, levels, interp, lut.ctypes.data,
                                             out.ptr + o, pg, 2, si, sg))
    return inp, out, len(calls)


def fam_typed(ctxs, E, levels, interp, lut, what, setname):
    """hgi_typed_encode_dev with 2- and 4-byte elements (see typed_cases): the shapes' content lifted to float16 / bfloat16 /
    float32 frames under (scale, bias) pairs for which the element 0.0 is NOT pixel 0 -- 37 under (1, 37.25), 255 under
    (-3.5, 300) -- so that a load outside the image that reads an element 0.0 instead of writing pixel 0 changes the grid
    (tests/test_typed_coverage.py shows on which shapes).  The frames of one row are in: their pitch counts as the row."""
    n = 0
    for esz in (2, 4):
        inp, out, calls = typed_cases(E, lifted_set(setname, esz), esz, levels, interp, lut, what, levels + 700 + esz)
        out.check(what), inp.check(what)
        n += calls
    return n


def fam_scaled(ctxs, E, levels, interp, lut, what, key):
    """hgi_decode_scaled_u8_dev at s = 1 and 2.  The sweep is over OUTPUT remainders: for an output shape (sw, sh) of R1 the
    source frames are ((sw << s) - t, (sh << s) - t) with t = 0 and t = 2^s - 1.  The call reads the stride-2^s lattice of the
    grid alone and runs levels - s levels on it, so the source grid is the oracle's grid of an (sw, sh) frame at levels - s levels
    laid on that lattice, every other byte nonzero noise, and the expected output the oracle's decode of it (one frame per call).
    The shapes of D run as they are, batch 2: the oracle's decode, every 2^s-th pixel."""
    from rustyhgi_amd import _ffi
    L, hd = _ffi.lib(), ctxs["fused"].handle
    setname, _, tname, _ = key
    n = 0
    bank = G.filler(1 << 22, levels)
    for s, tail in ((1, False), (1, True), (2, False), (2, True)):
        k = 1 << s
        inp, out, calls = Pool(False, levels + 500 + s), Pool(True), []
        if setname == "D":
            if tail:
                continue
            for w, h, img, grid, dec in E:
                sw, sh = -(-w // k), -(-h // k)
                st = w * h + 3
                calls.append((w, h, sw, sh, 2, st, inp.add(grid.reshape(2, 1, -1), stride=st, lead=1),
                              out.add(np.ascontiguousarray(dec[:, ::k, ::k]), sw + 13, sh * (sw + 13) + 1, lead=1, tag="%d x %d scaled s=%d" % (w, h, s))))
        else:
            t = k - 1 if tail else 0
            for sw, sh, _, g2, d2 in expected("R1", levels - s, tname, interp):
                w, h = (sw << s) - t, (sh << s) - t
                at = (131 * w + 17 * h) % (bank.size - w * h)
                src = bank[at:at + w * h].reshape(1, h, w).copy()
                src[:, ::k, ::k] = g2[:1]
                calls.append((w, h, sw, sh, 1, w * h, inp.add(src.reshape(1, 1, -1), lead=1),
                              out.add(d2[:1], sw + 13, lead=1, tag="%d x %d -> %d x %d scaled s=%d" % (w, h, sw, sh, s))))
        inp.upload(), out.upload()
        for w, h, sw, sh, b, st, i_grid, o in calls:
            _ffi.check(L.hgi_decode_scaled_u8_dev(hd, inp.ptr + i_grid, w, h, levels, interp, s, out.ptr + o, sw + 13, b, st, sh * (sw + 13) + 1))
        out.check(what), inp.check(what)
        n += len(calls)
    return n


def fam_region(ctxs, E, levels, interp, lut, what):
    """hgi_decode_region_u8_dev: the whole frame as the window, and the window (1, 1, W - 1, H - 1); batch 2."""
    from rustyhgi_amd import _ffi
    L, hd = _ffi.lib(), ctxs["fused"].handle
    inp, out, calls = Pool(False, levels + 600), Pool(True), []
    for w, h, img, grid, dec in E:
        st = w * h + 5
        i_grid = inp.add(grid.reshape(2, 1, -1), stride=st, lead=2)
        for x0, y0, rw, rh in ((0, 0, w, h), (1, 1, w - 1, h - 1)):
            if rw and rh:
                calls.append((w, h, st, i_grid, x0, y0, rw, rh, out.add(np.ascontiguousarray(dec[:, y0:y0 + rh, x0:x0 + rw]), rw + 5, rh * (rw + 5) + 2, lead=3,
                                                                      tag="%d x %d region %r" % (w, h, (x0, y0, rw, rh)))))
    inp.upload(), out.upload()
    for w, h, st, i_grid, x0, y0, rw, rh, o in calls:
        _ffi.check(L.hgi_decode_region_u8_dev(hd, inp.ptr + i_grid, w, h, levels, interp, x0, y0, rw, rh, out.ptr + o, rw + 5, 2, st, rh * (rw + 5) + 2))
    out.check(what), inp.check(what)
    return len(calls)


RUN = {"uniform": fam_uniform, "pitched": fam_pitched, "list": fam_list, "recon": fam_recon, "mapped": fam_mapped, "region": fam_region}


@pytest.mark.parametrize("family,setname,levels,tname,interp", CASES, ids=["%s-%s-L%d-%s-i%d" % c for c in CASES])
def test_every_remainder_through_every_entry_point(H, ctxs, family, setname, levels, tname, interp):
    """Every shape of the set through one family of entry points at one depth, table and interpolator (see the families'
    docstrings for the calls), against the oracle, bit for bit, sentinels and inputs intact."""
    import torch
    key = (setname, levels, tname, interp)
    lut = np.ascontiguousarray(TABLES[tname])
    what = "%s %s L%d %s interp %d" % (family, setname, levels, tname, interp)
    if family == "scaled":
        E = expected(*key) if setname == "D" else None
        n = fam_scaled(ctxs, E, levels, interp, lut, what, key)
    elif family == "typed":
        n = fam_typed(ctxs, expected(*key), levels, interp, lut, what, setname)
    else:
        n = RUN[family](ctxs, expected(*key), levels, interp, lut, what)
    torch.cuda.synchronize()
    print("%s: %d calls" % (what, n))


def test_typed_family_notices_one_wrong_pixel(H, oracle):
    """The whole-buffer comparison of the typed family on a 131 x 66 case (4 levels, the identity table, both element sizes) in
    which ONE element of the input -- the last of the second frame -- is a preimage of another pixel value: Pool.check raises
    and names the case.  The same case untouched passes."""
    import torch
    w, h, levels = 131, 66, 4
    img = G.content(w, h, batch=2)
    lut = np.ascontiguousarray(TABLES["identity"])
    grid = np.stack([oracle.encode(img[f], levels, lut, 1) for f in range(2)])
    E = [(w, h, img, grid, None)]
    for esz in (2, 4):
        kind, pair = typed_choice(esz, 1)
        good = np.ascontiguousarray(TR.lift(img, bank(kind, pair), 1))
        inp, out, _ = typed_cases(E, [(kind, pair, good.view(np.uint8).reshape(2, h, w * esz))], esz, levels, 1, lut, "self-check", 770)
        out.check("self-check"), inp.check("self-check")
        bad = good.copy()
        other = (int(img[1, -1, -1]) + 100) % 256
        bad[1, -1, -1] = bank(kind, pair)[other, 0]
        assert TR.quantize(TR.elements(kind, bad[1, -1, -1:]), *pair)[0] == other != img[1, -1, -1]
        inp, out, _ = typed_cases(E, [(kind, pair, bad.view(np.uint8).reshape(2, h, w * esz))], esz, levels, 1, lut, "self-check", 771)
        with pytest.raises(AssertionError, match=r"self-check 131 x 66 typed %s .*first in frame 1 at \(x=130, y=65" % kind):
            out.check("self-check")
        inp.check("self-check")
    torch.cuda.synchronize()


def test_scaled_sources_are_what_the_full_decode_subsamples(oracle):
    """The construction of fam_scaled, on the oracle alone: the decode of a full-size grid, every 2^s-th pixel, equals the
    decode at levels - s of the grid's stride-2^s lattice -- whatever the other bytes of the grid hold."""
    for (sw, sh), levels, s, t in (((129, 65), 4, 1, 0), ((200, 127), 4, 2, 3), ((255, 102), 5, 2, 0), ((131, 66), 2, 1, 1), ((140, 70), 1, 2, 3)):
        k = 1 << s
        w, h = (sw << s) - t, (sh << s) - t
        c = G.content(sw, sh)
        for interp in (1, 0):
            g2 = oracle.encode(c, levels - s, TABLES["linear2"], interp) if levels > s else c
            src = G.filler(w * h, 5).reshape(h, w)
            src[::k, ::k] = g2
            want = oracle.decode(g2, levels - s, interp) if levels > s else c
            assert (oracle.decode(src, levels, interp)[::k, ::k] == want).all(), (sw, sh, levels, s, t, interp)


# ------------------------------------------------------------------------------------------ region window cuts
def _cut_windows():
    """300 x 150: left cuts 112 ... 127 against right cuts 260 ... 275 -- in the frame's own ragged tile -- under four row
    ranges; then every window of 1 ... 16 columns inside one 16-byte chunk at every x0 mod 16."""
    wins = [(112 + i, y0, 260 + j - (112 + i), y1 - y0) for y0, y1 in ((0, 150), (63, 129), (64, 130), (65, 150)) for i in range(16) for j in range(16)]
    wins += [(272 + a, 63, wd, 66) for a in range(16) for wd in range(1, 17 - a)]
    wins += [(128 + a, 1, wd, 149) for a in range(16) for wd in range(1, 17 - a)]
    return wins


def test_region_window_cuts(H, ctxs, oracle):
    """hgi_decode_region_u8_dev on a 300 x 150 frame at 4 levels: 1024 windows whose left and right cuts take every x mod 16
    (the right cut inside the frame's ragged tile), and every window that lies inside one 16-byte chunk, in the ragged tile and
    in an interior one; each against the crop of the oracle's decode, sentinels intact."""
    import torch
    from rustyhgi_amd import _ffi
    L, hd = _ffi.lib(), ctxs["fused"].handle
    w, h, levels = 300, 150, 4
    wins = _cut_windows()
    assert len(wins) == 1024 + 2 * 136 and all(x0 + rw <= w and y0 + rh <= h and rw > 0 and rh > 0 for x0, y0, rw, rh in wins)
    img = G.content(w, h, batch=2)
    for tname, interp in (("linear2", 1), ("identity", 0)):
        grid = np.stack([oracle.encode(img[f], levels, TABLES[tname], interp) for f in range(2)])
        dec = np.stack([oracle.decode(grid[f], levels, interp) for f in range(2)])
        inp, out = Pool(False, 700), Pool(True)
        st = w * h + 5
        i_grid = inp.add(grid.reshape(2, 1, -1), stride=st, lead=2)
        outs = [out.add(np.ascontiguousarray(dec[:, y0:y0 + rh, x0:x0 + rw]), rw + 5, rh * (rw + 5) + 2, lead=3, tag="window %r" % ((x0, y0, rw, rh),))
                for x0, y0, rw, rh in wins]
        inp.upload(), out.upload()
        for (x0, y0, rw, rh), o in zip(wins, outs):
            _ffi.check(L.hgi_decode_region_u8_dev(hd, inp.ptr + i_grid, w, h, levels, interp, x0, y0, rw, rh, out.ptr + o, rw + 5, 2, st, rh * (rw + 5) + 2))
        what = "region cuts %s interp %d" % (tname, interp)
        out.check(what), inp.check(what)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------ forced paths, knobs build
CHILD_MODES = ["HGI_TILE_H=64", "HGI_TILE_H=32", "HGI_TILE_H=16", "HGI_FORCE_CHECKED=1"]
CHILD_CASES = [c for c in CASES if c[0] == "uniform" and c[1] == "R"]
_child_lost = []


@pytest.mark.parametrize("mode", CHILD_MODES)
def test_forced_code_paths_in_a_child_process(mode):
    """On small shapes the release library runs encodes on 16-row and decodes on 32-row tiles.  A child process on the KNOBS
    build re-runs the uniform family's cases of the remainder sets with one tile height or the checked path forced: the bytes
    must not depend on it.  Each child has its own timeout; once a child has ended by signal or timeout this test fails at once
    and starts no other."""
    from rustyhgi_amd import _ffi
    assert not _child_lost, "not started: the child under %s ended by signal or timeout" % _child_lost[0]
    knobs = os.path.join(os.path.dirname(_ffi.LIB_PATH), "libhgi_hip_knobs.so")
    assert os.path.exists(knobs), "libhgi_hip_knobs.so is missing: __graft_entry__.build() / `make -C rustyhgi_amd/csrc knobs` builds it"
    env = dict(os.environ, HGI_LIB_PATH=knobs, **dict(kv.split("=") for kv in mode.split(",")))
    cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider",
           "-k", "test_every_remainder and uniform-R-"]
    try:
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired:
        _child_lost.append(mode)
        pytest.fail(mode + ": the child did not finish in 300 s")
    if r.returncode < 0:
        _child_lost.append(mode)
        pytest.fail("%s: the child ended by signal %d\n%s" % (mode, -r.returncode, r.stdout[-2000:] + r.stderr[-1000:]))
    assert r.returncode == 0, mode + "\n" + r.stdout[-3000:] + r.stderr[-1000:]
    assert "%d passed" % len(CHILD_CASES) in r.stdout, r.stdout[-500:]
