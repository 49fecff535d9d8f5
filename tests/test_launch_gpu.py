"""One call for each instantiation of the core library's tile kernels, through the C entry points: what the launchers' step
from run-time choices to template arguments (rustyhgi_amd/csrc/hgi_launch.h) picks must be the kernel of that interpolator,
table kind, depth and shift.  On these inputs a kernel of another INTERP, IDENT, SEEDED or SH gives other bytes
(test_inputs_tell_the_kernels_apart).  Levels 3 and 6 are the unseeded tile and the cone.  A batch of two 300 x 150 frames:
four interior tiles, a ragged column, a ragged row and a corner each, so both paths of a kernel run; a scaled decode takes
frames whose VIEW is 300 x 150 with 3 and 6 levels of its own.  Outputs with a pitch lie in sentinel-filled parents that are
checked whole.  Expected bytes: the oracle, never the library.

The uniform entry picks a tile height per call (hgi_capi.hip, use_tile_rows): on this batch the release library encodes on
16-row tiles and decodes on 32-row tiles.  The other builds run in one child process per forced height on the knobs build, one
after another.  Seed PLANES without a cone (SEEDED == 1, 64-row tiles only) are what a banded host call starts from
(hgi_capi.hip, host_banded: six fused levels, so from seven levels, on a frame of 4 Mi pixels and more)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import operand_designs as D
from conftest import SEED0
from kernel_calls import H, Plane, call_list, ctxs, dev, same_dev  # noqa: F401

pytestmark = pytest.mark.gpu
B, ROWS, COLS = 2, 150, 300
INTERPS, LEVELS, SHIFTS = (1, 0), (3, 6), (1, 2, 3)
TABLES = {"identity": np.arange(256, dtype=np.uint8), "lossy": D.tables()["random0"]}
BANDED = (7, 2010, 2090)      # levels, rows, columns: banded (>= 4 Mi pixels), deeper than a tile, ragged on both sides
WINDOW = (37, 21, 263, 129)   # x0, y0, columns, rows: one tile wholly inside, the others cut or ragged


def random_frames(seed, *shape):
    a = np.random.default_rng(SEED0 + seed).integers(0, 256, shape, dtype=np.uint8)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def frames(shift=0):
    """Random bytes, images for the encoders and grids for the decoders: (B, ROWS, COLS), or frames whose stride-2^shift lattice is
    ROWS x COLS (the last lattice column and row are the frame's last)."""
    return random_frames(30 + shift, B, ((ROWS - 1) << shift) + 1, ((COLS - 1) << shift) + 1)


@functools.lru_cache(maxsize=None)
def decoded(levels, interp, shift=0):
    from oracle import hgi_oracle as O
    return np.stack([O.decode(np.ascontiguousarray(g), levels, interp) for g in frames(shift)])


@functools.lru_cache(maxsize=None)
def encoded(levels, interp, tname):
    from oracle import hgi_oracle as O
    return np.stack([O.encode(np.ascontiguousarray(a), levels, TABLES[tname], interp) for a in frames()])


@functools.lru_cache(maxsize=None)
def banded(interp, tname):
    """One banded frame, its grid under the table and the decode of the FRAME taken as a grid."""
    from oracle import hgi_oracle as O
    levels, h, w = BANDED
    img = np.ascontiguousarray(random_frames(40, h, w))
    return img, O.encode(img, levels, TABLES[tname], interp), O.decode(img, levels, interp)


def side(data=None, gap=0, lead=0, seed=0, h=ROWS, w=COLS):
    """A side of the batch as one plane of B * h rows, frames h pitches apart: an input around `data`, or an output."""
    p = Plane(B * h, w, w + gap, lead, random=data is not None, seed=seed + 1)
    return p if data is None else p.put(data.reshape(B * h, w))


def check(out, want, what):
    same_dev(out.rows().reshape(want.shape), want, what)
    out.intact(what)


def test_inputs_tell_the_kernels_apart(oracle):
    """Another INTERP, IDENT, SEEDED or SH on the same call means other bytes: the two interpolators and the two depths decode the
    grids differently, the two tables and the two interpolators code the frames differently, and the lattices of a scaled frame
    at the three shifts, cut to a common size, differ."""
    for levels in LEVELS:
        assert (decoded(levels, 1) != decoded(levels, 0)).mean() > 0.25
        for tname in TABLES:
            assert (encoded(levels, 1, tname) != encoded(levels, 0, tname)).mean() > 0.25
        for interp in INTERPS:
            assert (encoded(levels, interp, "identity") != encoded(levels, interp, "lossy")).mean() > 0.25
    for interp in INTERPS:
        assert (decoded(3, interp) != decoded(6, interp)).mean() > 0.25      # a tile that skipped its cone, or built one
        g = frames(3)[0]
        h, w = ROWS // 4, COLS // 4
        cuts = [g[::1 << s, ::1 << s][:h, :w] for s in SHIFTS]
        assert all((a != b).mean() > 0.9 for a in cuts for b in cuts if a is not b)      # a load at another shift's stride


# ------------------------------------------------------------------------------------------------ the uniform entry
@pytest.mark.parametrize("levels", LEVELS)
@pytest.mark.parametrize("tname", sorted(TABLES))
@pytest.mark.parametrize("interp", INTERPS)
def test_uniform_encode_kernels(H, ctxs, oracle, interp, tname, levels):
    from rustyhgi_amd import _ffi
    src, out = dev(frames()), Plane(1, B * ROWS * COLS, B * ROWS * COLS, 16)
    _ffi.check(_ffi.lib().hgi_encode_u8_dev(ctxs["fused"].handle, src.data_ptr(), COLS, ROWS, levels, interp, TABLES[tname].ctypes.data, out.ptr,
                                            B, COLS * ROWS))
    check(out, dev(encoded(levels, interp, tname)), "encode interp %d %s L%d" % (interp, tname, levels))


@pytest.mark.parametrize("levels", LEVELS)
@pytest.mark.parametrize("interp", INTERPS)
def test_uniform_decode_kernels(H, ctxs, oracle, interp, levels):
    from rustyhgi_amd import _ffi
    src, out = dev(frames()), Plane(1, B * ROWS * COLS, B * ROWS * COLS, 16)
    _ffi.check(_ffi.lib().hgi_decode_u8_dev(ctxs["fused"].handle, src.data_ptr(), COLS, ROWS, levels, interp, out.ptr, B, COLS * ROWS))
    check(out, dev(decoded(levels, interp)), "decode interp %d L%d" % (interp, levels))


@pytest.mark.parametrize("tname", sorted(TABLES))
@pytest.mark.parametrize("interp", INTERPS)
def test_seed_plane_kernels_under_a_banded_host_call(H, ctxs, oracle, interp, tname):
    """hgi_encode_u8 on a banded frame of seven levels: six fused levels on seed planes, SEEDED == 1; the decode under the
    identity table's turn alone (it takes no table)."""
    from rustyhgi_amd import _ffi
    levels, h, w = BANDED
    img, grid, dec = banded(interp, tname)
    out = np.full_like(img, 0xA5)
    _ffi.check(_ffi.lib().hgi_encode_u8(ctxs["fused"].handle, img.ctypes.data, w, h, levels, interp, TABLES[tname].ctypes.data, out.ctypes.data))
    assert np.array_equal(out, grid), "banded encode interp %d %s" % (interp, tname)
    if tname == "identity":
        out.fill(0x5A)
        _ffi.check(_ffi.lib().hgi_decode_u8(ctxs["fused"].handle, img.ctypes.data, w, h, levels, interp, out.ctypes.data))
        assert np.array_equal(out, dec), "banded decode interp %d" % interp


_child_lost = []


@pytest.mark.parametrize("rows", (16, 32, 64))
def test_uniform_kernels_of_a_forced_tile_height_in_a_child_process(rows):
    """A child process on the KNOBS build runs the uniform encode and decode cases above with HGI_TILE_H forced.  Each child has
    its own timeout; once a child has ended by signal or timeout this test fails at once and starts no other."""
    from rustyhgi_amd import _ffi
    assert not _child_lost, "not started: the child under HGI_TILE_H=%s ended by signal or timeout" % _child_lost[0]
    knobs = os.path.join(os.path.dirname(_ffi.LIB_PATH), "libhgi_hip_knobs.so")
    assert os.path.exists(knobs), "libhgi_hip_knobs.so is missing: __graft_entry__.build() / `make -C rustyhgi_amd/csrc knobs` builds it"
    env = dict(os.environ, HGI_LIB_PATH=knobs, HGI_TILE_H=str(rows))
    cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider", "-k",
           "test_uniform_encode_kernels or test_uniform_decode_kernels"]
    try:
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        _child_lost.append(rows)
        pytest.fail("HGI_TILE_H=%d: the child did not finish in 120 s" % rows)
    if r.returncode < 0:
        _child_lost.append(rows)
        pytest.fail("HGI_TILE_H=%d: the child ended by signal %d\n%s" % (rows, -r.returncode, r.stdout[-2000:] + r.stderr[-1000:]))
    assert r.returncode == 0, "HGI_TILE_H=%d\n%s" % (rows, r.stdout[-3000:] + r.stderr[-1000:])
    assert "12 passed" in r.stdout, r.stdout[-500:]


# ------------------------------------------------------------------------------------------------ the 64-row variants
@pytest.mark.parametrize("levels", LEVELS)
@pytest.mark.parametrize("interp", INTERPS)
def test_region_kernels(H, ctxs, oracle, interp, levels):
    from rustyhgi_amd import _ffi
    x0, y0, rw, rh = WINDOW
    src, out = dev(frames()), side(gap=5, lead=3, h=rh, w=rw)
    _ffi.check(_ffi.lib().hgi_decode_region_u8_dev(ctxs["fused"].handle, src.data_ptr(), COLS, ROWS, levels, interp, x0, y0, rw, rh, out.ptr,
                                                   out.pitch, B, COLS * ROWS, rh * out.pitch))
    check(out, dev(decoded(levels, interp)[:, y0:y0 + rh, x0:x0 + rw]), "region interp %d L%d" % (interp, levels))


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("levels", LEVELS)
@pytest.mark.parametrize("interp", INTERPS)
def test_scaled_kernels(H, ctxs, oracle, interp, levels, shift):
    """`levels` are the VIEW's: the frame has `shift` more."""
    from rustyhgi_amd import _ffi
    h, w = frames(shift).shape[1:]
    src, out = dev(frames(shift)), side(gap=13, lead=1)
    _ffi.check(_ffi.lib().hgi_decode_scaled_u8_dev(ctxs["fused"].handle, src.data_ptr(), w, h, levels + shift, interp, shift, out.ptr,
                                                   out.pitch, B, w * h, ROWS * out.pitch))
    want = decoded(levels + shift, interp, shift)[:, ::1 << shift, ::1 << shift]
    check(out, dev(want), "scaled interp %d L%d s=%d" % (interp, levels, shift))


@pytest.mark.parametrize("levels", LEVELS)
@pytest.mark.parametrize("tname", sorted(TABLES))
@pytest.mark.parametrize("interp", INTERPS)
def test_list_encode_kernels(H, ctxs, oracle, interp, tname, levels):
    src = dev(frames())
    outs = [Plane(1, ROWS * COLS, ROWS * COLS, lead) for lead in (7, 1)]
    call_list(ctxs["fused"], True, [src[f].data_ptr() for f in range(B)], [o.ptr for o in outs], [(COLS, ROWS)] * B, levels, interp, TABLES[tname])
    want = dev(encoded(levels, interp, tname))
    for f, o in enumerate(outs):
        check(o, want[f], "list encode interp %d %s L%d frame %d" % (interp, tname, levels, f))


@pytest.mark.parametrize("levels", LEVELS)
@pytest.mark.parametrize("interp", INTERPS)
def test_list_decode_kernels(H, ctxs, oracle, interp, levels):
    src = dev(frames())
    outs = [Plane(1, ROWS * COLS, ROWS * COLS, lead) for lead in (7, 1)]
    call_list(ctxs["fused"], False, [src[f].data_ptr() for f in range(B)], [o.ptr for o in outs], [(COLS, ROWS)] * B, levels, interp)
    want = dev(decoded(levels, interp))
    for f, o in enumerate(outs):
        check(o, want[f], "list decode interp %d L%d frame %d" % (interp, levels, f))


@pytest.mark.parametrize("levels", LEVELS)
@pytest.mark.parametrize("tname", sorted(TABLES))
@pytest.mark.parametrize("interp", INTERPS)
def test_pitched_encode_kernels(H, ctxs, oracle, interp, tname, levels):
    from rustyhgi_amd import _ffi
    src, out = side(dev(frames()), gap=61, lead=3, seed=levels), side(gap=3, lead=16)
    _ffi.check(_ffi.lib().hgi_encode_u8_pitched_dev(ctxs["fused"].handle, src.ptr, src.pitch, COLS, ROWS, levels, interp, TABLES[tname].ctypes.data,
                                                    out.ptr, out.pitch, B, ROWS * src.pitch, ROWS * out.pitch))
    check(out, dev(encoded(levels, interp, tname)), "pitched encode interp %d %s L%d" % (interp, tname, levels))


@pytest.mark.parametrize("levels", LEVELS)
@pytest.mark.parametrize("interp", INTERPS)
def test_pitched_decode_kernels(H, ctxs, oracle, interp, levels):
    from rustyhgi_amd import _ffi
    src, out = side(dev(frames()), gap=3, lead=16, seed=levels), side(gap=61, lead=3)
    _ffi.check(_ffi.lib().hgi_decode_u8_pitched_dev(ctxs["fused"].handle, src.ptr, src.pitch, COLS, ROWS, levels, interp, out.ptr, out.pitch, B,
                                                    ROWS * src.pitch, ROWS * out.pitch))
    check(out, dev(decoded(levels, interp)), "pitched decode interp %d L%d" % (interp, levels))
