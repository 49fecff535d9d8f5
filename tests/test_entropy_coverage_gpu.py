"""GPU suite of the entropy-coverage designs (tests/entropy_designs.py; what they cover is asserted on the CPU in
tests/test_entropy_coverage.py): every design goes through the device entropy stage and is compared two ways -- with the restated
stream byte for byte, and, independently, zlib must inflate the device's bytes to the grid's bincode image.  dense15 fills the LDS
stream image of k_token_pack to its last word and holds the 21-bit token; runs puts every piece length in front of every byte of a
lane; threshold makes the host pick each candidate; tails ends the data inside every lane; sharing and scan stand on the words
several writers share and on the block edges of k_huff_scan.  A mistake confined to one of these classes fails here and nowhere
else in the suite.

Entry points: hgi_deflate_grid_dev on every design, hgi_deflate_grids_dev (frames n + 3 bytes apart, the gaps non-zero) and
hgi_deflate_grids_packed_dev on batches, hgi_deflate_grid on dense15 and three tails; every output lies in a sentinel-filled buffer
and no byte behind a stream may be touched.  Two forced paths run as child processes on the knobs build: one workgroup per CU (a
wave then codes the full chunk and shorter ones after it) and stream groups of 1 MiB (the two-set pipeline, four groups of three
frames).  Expected bytes: the restatement and zlib.  Never the library's device path."""
import ctypes
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import entropy_designs as E  # noqa: E402
from kernel_calls import H  # noqa: E402,F401

pytestmark = pytest.mark.gpu
SENT = 0xC3


def align(x, a):
    return (x + a - 1) // a * a


def cap_of(n):
    return n + n // 8 + 1024


def assert_stream(got, grid, want, what):
    """the device's bytes: ordinary DEFLATE of the grid's bincode image (zlib is the judge), and the restated stream"""
    z = zlib.decompressobj(-15)
    assert z.decompress(got) == E.image(grid, grid.shape[1]) and z.eof and not z.unused_data, what + ": zlib does not inflate it to the grid"
    if got != want:
        a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
        m = min(a.size, b.size)
        first = int(np.flatnonzero(a[:m] != b[:m])[0]) if (a[:m] != b[:m]).any() else m
        raise AssertionError("%s: %d bytes, restated %d, first difference at byte %d" % (what, a.size, b.size, first))


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def deflate_one(ctx, ptr, w, h, host=False):
    """hgi_deflate_grid_dev (or the host form) into a sentinel-filled buffer: the stream, nothing touched behind it"""
    from rustyhgi_amd import _ffi
    cap = cap_of(w * h)
    out = np.full(cap + 64, SENT, np.uint8)
    n = ctypes.c_size_t(0)
    fn = _ffi.lib().hgi_deflate_grid if host else _ffi.lib().hgi_deflate_grid_dev
    _ffi.check(fn(ctx.handle, ptr, w, h, out.ctypes.data, cap, ctypes.byref(n)))
    assert (out[n.value:] == SENT).all(), "bytes behind the stream were written"
    return out[:n.value].tobytes()


def strided(ctx, grids):
    """hgi_deflate_grids_dev: frames n + 3 bytes apart with 0xAB between them, output slots filled with the sentinel"""
    from rustyhgi_amd import _ffi
    B, (h, w) = len(grids), grids[0].shape
    n, stride, cap = w * h, w * h + 3, cap_of(w * h) + 5
    flat = np.full(B * stride, 0xAB, np.uint8)
    for f, g in enumerate(grids):
        flat[f * stride:f * stride + n] = g.reshape(-1)
    d = dev(flat)
    out = np.full((B, cap), SENT, np.uint8)
    sizes = (ctypes.c_size_t * B)()
    _ffi.check(_ffi.lib().hgi_deflate_grids_dev(ctx.handle, d.data_ptr(), w, h, B, stride, out.ctypes.data, cap, sizes))
    for f in range(B):
        assert (out[f, sizes[f]:] == SENT).all(), "frame %d: bytes behind sizes[f] were written" % f
    return [out[f, :sizes[f]].tobytes() for f in range(B)]


def packed(ctx, grids, cap=None, expect=0):
    """hgi_deflate_grids_packed_dev on the same layout: 64-byte aligned starts that ascend, zero gaps, nothing behind the packed
    region.  `cap`: the room to declare (the buffer itself is longer and must stay untouched behind it)."""
    from rustyhgi_amd import _ffi
    B, (h, w) = len(grids), grids[0].shape
    n, stride = w * h, w * h + 3
    flat = np.full(B * stride, 0xAB, np.uint8)
    for f, g in enumerate(grids):
        flat[f * stride:f * stride + n] = g.reshape(-1)
    d = dev(flat)
    room = B * (cap_of(n) + 64) if cap is None else cap
    out = np.full(room + 4096, SENT, np.uint8)
    sizes, offs = (ctypes.c_size_t * B)(), (ctypes.c_size_t * B)()
    st = _ffi.lib().hgi_deflate_grids_packed_dev(ctx.handle, d.data_ptr(), w, h, B, stride, out.ctypes.data, room, offs, sizes)
    assert st == expect, (st, _ffi.lib().hgi_last_error())
    assert (out[room:] == SENT).all(), "bytes behind cap were written"
    if st:
        return None
    at = 0
    for f in range(B):
        assert offs[f] == at and offs[f] % 64 == 0, "frame %d at %d, expected %d" % (f, offs[f], at)
        assert not out[offs[f] + sizes[f]:align(offs[f] + sizes[f], 64)].any(), "frame %d: a gap byte is not zero" % f
        at = align(offs[f] + sizes[f], 64)
    assert (out[at:] == SENT).all(), "bytes behind the packed region were written"
    return [out[offs[f]:offs[f] + sizes[f]].tobytes() for f in range(B)], list(offs), list(sizes)


@pytest.fixture(scope="module")
def ctx(H):
    c = H.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------------ every design
@pytest.mark.parametrize("name", E.BATCH + E.SINGLES)
def test_design_through_the_single_frame_call(ctx, name):
    g = E.frame(name)
    h, w = g.shape
    d = dev(g)
    assert_stream(deflate_one(ctx, d.data_ptr(), w, h), g, E.restated(name)[0], name)
    if name.startswith("dense15"):
        assert_stream(deflate_one(ctx, g.ctypes.data, w, h, host=True), g, E.restated(name)[0], name + " (host form)")


@pytest.mark.parametrize("kind", (0, 1))
def test_tails_through_the_single_frame_call(ctx, kind):
    """Every n of 1 ... 1040 and 2047 ... 2050 as a 1 x n frame (kind 0: a run reaches the end of the data; 1: the last byte stands
    alone), read at whatever address it has inside one device buffer of all of them; three of them through the host form."""
    frames = [E.tail_frame(n, kind) for n in E.TAIL_N]
    starts = np.concatenate([[0], np.cumsum([f.size for f in frames])])
    d = dev(np.concatenate([f.reshape(-1) for f in frames]))
    for f, n, at in zip(frames, E.TAIL_N, starts):
        want = E.restate(f, n, census=False)[0]
        assert_stream(deflate_one(ctx, d.data_ptr() + int(at), n, 1), f, want, "tail %d kind %d" % (n, kind))
        if n in (15, 1025, 2050):
            assert_stream(deflate_one(ctx, f.ctypes.data, n, 1, host=True), f, want, "tail %d kind %d (host form)" % (n, kind))


def test_batches_strided_and_packed(ctx):
    """The eleven 512 x 522 designs and the all-zero frame in one call, and pairs of tails."""
    names = E.BATCH + ("zeros",)
    batches = [([E.frame(n) for n in names], [E.restated(n)[0] for n in names], names)]
    for n in (1, 17, 1023, 1025, 2049):
        pair = [E.tail_frame(n, 0), E.tail_frame(n, 1), E.tail_frame(n, 0)]
        batches.append((pair, [E.restate(g, n, census=False)[0] for g in pair], ["tail %d/%d" % (n, k) for k in (0, 1, 0)]))
    for grids, wants, whats in batches:
        got = strided(ctx, grids)
        for g, s, want, what in zip(grids, got, wants, whats):
            assert_stream(s, g, want, what + " (strided batch)")
        got, _, _ = packed(ctx, grids)
        for g, s, want, what in zip(grids, got, wants, whats):
            assert_stream(s, g, want, what + " (packed batch)")


# --------------------------------------------------------------------------------- forced paths, knobs build, children
def child_wgs(H):
    """HGI_ENTROPY_WGS_PER_CU=1 and a batch of half as many frames as the device has CUs: two workgroups a frame, so a wave walks
    chunk c, c + 8, c + 16, ...  The frames are the eight dense15 frames: for each of the four waves one frame makes that wave
    code the 15 360-bit chunk, next the 9 792-bit one and then short ones, and one frame the 9 792-bit chunk, next the 15 360-bit
    one and then short ones (tests/test_entropy_coverage.py asserts that placement): whatever a long chunk leaves in the LDS
    image of the stream, the next one ORs its bits into."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    frames = max(8, cus // 2)
    assert cus < 16 or E.blocks_for(261, frames, cus) == 2, (cus, frames)
    names = [E.DENSE[f % len(E.DENSE)] for f in range(frames)]
    ctx = H.Context(0)
    grids = [E.frame(n) for n in names]
    got = strided(ctx, grids)
    for f, n in enumerate(names):
        assert_stream(got[f], grids[f], E.restated(n)[0], "frame %d (%s)" % (f, n))
    # ... and one frame alone: 66 workgroups, every wave codes at most one chunk
    d = dev(grids[2])
    assert_stream(deflate_one(ctx, d.data_ptr(), E.BW, E.BH), grids[2], E.restated(names[2])[0], "single")
    ctx.close()
    print("child ok: %d CUs, %d frames" % (cus, frames))


def child_groups(H):
    """HGI_ENTROPY_GROUP_MIB=1: the eleven 512 x 522 frames are four groups (3, 3, 3, 2) on two sets of buffers.  Strided and
    packed, every stream equal to the single-frame call's and to the restatement; then a packed call whose cap is one byte short
    in the third group: HGI_EINVAL, nothing behind cap written, and the context serves the next call."""
    from rustyhgi_amd import _ffi
    dev_cap = align(E.BN + E.BN // 4 + 4096, 256)
    group = (1 << 20) // dev_cap
    ngroups = (11 + group - 1) // group
    assert (group, ngroups, (11 + ngroups - 1) // ngroups) == (3, 4, 3)
    ctx = H.Context(0)
    grids = [E.frame(n) for n in E.BATCH]
    wants = [E.restated(n)[0] for n in E.BATCH]
    singles = []
    for g in grids:
        d = dev(g)
        singles.append(deflate_one(ctx, d.data_ptr(), E.BW, E.BH))
    got = strided(ctx, grids)
    for f, n in enumerate(E.BATCH):
        assert got[f] == singles[f], n
        assert_stream(got[f], grids[f], wants[f], n + " (strided, four groups)")
    got, offs, sizes = packed(ctx, grids)
    for f, n in enumerate(E.BATCH):
        assert got[f] == singles[f], n
        assert_stream(got[f], grids[f], wants[f], n + " (packed, four groups)")
    assert all(offs[f + 1] > offs[f] for f in range(10))
    # one byte short of what the first three groups need
    short = align(offs[8] + sizes[8], 64) - 1
    assert offs[6] + sizes[6] < short
    assert packed(ctx, grids, cap=short, expect=_ffi.EINVAL) is None
    assert b"too small" in _ffi.lib().hgi_last_error()
    again, offs2, sizes2 = packed(ctx, grids[::-1])
    assert again == singles[::-1]
    assert strided(ctx, grids) == singles
    ctx.close()
    print("child ok: four groups of %d" % group)


CHILDREN = {"wgs": ("HGI_ENTROPY_WGS_PER_CU=1", child_wgs), "groups": ("HGI_ENTROPY_GROUP_MIB=1", child_groups)}
_child_lost = []


@pytest.mark.parametrize("mode", list(CHILDREN))
def test_forced_paths_in_a_child_process(mode):
    """A child process on the KNOBS build (tests/test_operand_coverage_gpu.py does the same for its paths): see child_wgs and
    child_groups.  Each child has its own timeout; once a child has ended by signal or timeout no other is started."""
    from rustyhgi_amd import _ffi
    assert not _child_lost, "not started: the child under %s ended by signal or timeout" % _child_lost[0]
    knobs = os.path.join(os.path.dirname(_ffi.LIB_PATH), "libhgi_hip_knobs.so")
    assert os.path.exists(knobs), "libhgi_hip_knobs.so is missing: __graft_entry__.build() / `make -C rustyhgi_amd/csrc knobs` builds it"
    env = dict(os.environ, HGI_LIB_PATH=knobs, **dict([CHILDREN[mode][0].split("=")]))
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), mode], env=env, capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        _child_lost.append(mode)
        pytest.fail(mode + ": the child did not finish in 120 s")
    if r.returncode < 0:
        _child_lost.append(mode)
        pytest.fail("%s: the child ended by signal %d\n%s" % (mode, -r.returncode, r.stdout[-2000:] + r.stderr[-1000:]))
    assert r.returncode == 0 and "child ok" in r.stdout, mode + "\n" + r.stdout[-3000:] + r.stderr[-3000:]


if __name__ == "__main__":
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    import rustyhgi_amd
    from rustyhgi_amd import _ffi
    assert _ffi.LIB_PATH.endswith("libhgi_hip_knobs.so") and _ffi.lib() is not None
    CHILDREN[sys.argv[1]][1](rustyhgi_amd)
