"""The uniform kernels' block -> tile walk on the device (rustyhgi_amd/csrc/hgi_tilewalk.h; walked on the CPU by
tests/cpp/test_tilewalk.cpp, and tests/test_geometry_coverage.py shows what the cases below reach).

The WALK cases (tests/geometry_designs.py:walk_cases) are 600 small launches -- 1 ... 3 interior tile columns with and without
a ragged one, 1 ... 24 interior rows of 16-row tiles with and without a ragged one, 1 ... 9 frames -- through
hgi_encode_u8_dev / hgi_decode_u8_dev at three levels, against the oracle.  Every output lies in a sentinel-filled buffer that
is checked whole: a tile that no block reaches leaves sentinels behind, a tile reached twice by different frames' blocks
shows as wrong bytes.  In-process they run on the release library with its own policy (bands of 4 or 8 rows, round-robin
dealing where a launch has eight whole bands); children on the knobs build force 16-row tiles, bands of 1 ... 4 rows, both
XCD dealings and the backwards walk, which the release library reaches on wide or huge frames only."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import geometry_designs as G
from kernel_calls import H, Pool, ctxs  # noqa: F401

pytestmark = pytest.mark.gpu
LEVELS = 3
PARTS = [(ex, tname) for ex in (1, 2, 3) for tname in ("linear2", "identity")]


def table(tname):
    from oracle import hgi_numpy as N
    return np.ascontiguousarray(N.linear_lut(2)[0] if tname == "linear2" else np.arange(256, dtype=np.uint8))


@functools.lru_cache(maxsize=None)
def frames_of(w, h, tname):
    """Nine frames of the shape with their grids and decodes (the oracle): a case of batch b takes the first b."""
    from oracle import hgi_oracle as O
    O.build()
    img = G.content(w, h, batch=9, salt=17)
    grid = np.stack([O.encode(img[f], LEVELS, table(tname), 1) for f in range(9)])
    return img, grid, np.stack([O.decode(grid[f], LEVELS, 1) for f in range(9)])


@pytest.mark.parametrize("ex,tname", PARTS, ids=["ex%d-%s" % p for p in PARTS])
def test_walk_cases_against_the_oracle(H, ctxs, ex, tname):
    """The WALK cases with `ex` interior tile columns under one table, both directions, Crossed, three levels.  Inputs end in
    mid-page, so that frames whose rows are not a multiple of 4 bytes keep their interior tiles."""
    import torch
    from rustyhgi_amd import _ffi
    L, hd, lut = _ffi.lib(), ctxs["fused"].handle, table(tname)
    inp, out, calls = Pool(False, 800 + ex), Pool(True), []
    for w, h, b in G.walk_cases():
        if w // 128 != ex:
            continue
        img, grid, dec = frames_of(w, h, tname)
        tag = "%d x %d batch %d" % (w, h, b)
        calls.append((w, h, b, inp.add(img[:b].reshape(b, 1, -1), lead=3, end_mod=2048), out.add(grid[:b].reshape(b, 1, -1), lead=5, tag=tag + " encode"),
                      inp.add(grid[:b].reshape(b, 1, -1), lead=1, end_mod=2048), out.add(dec[:b].reshape(b, 1, -1), lead=2, tag=tag + " decode")))
    assert len(calls) == 200
    inp.upload(), out.upload()
    for w, h, b, i_img, o_enc, i_grid, o_dec in calls:
        _ffi.check(L.hgi_encode_u8_dev(hd, inp.ptr + i_img, w, h, LEVELS, 1, lut.ctypes.data, out.ptr + o_enc, b, w * h))
        _ffi.check(L.hgi_decode_u8_dev(hd, inp.ptr + i_grid, w, h, LEVELS, 1, out.ptr + o_dec, b, w * h))
    what = "walk cases ex %d %s" % (ex, tname)
    out.check(what), inp.check(what)
    torch.cuda.synchronize()


# (forced band, HGI_XCD_MODE, HGI_DEC_REVERSE)
CHILD_MODES = [(1, 1, 0), (2, 1, 0), (3, 1, 0), (4, 1, 0), (3, 0, 0), (2, 1, 1)]
_child_lost = []


@pytest.mark.parametrize("band,xmode,reverse", CHILD_MODES, ids=["band%d-xmode%d-reverse%d" % m for m in CHILD_MODES])
def test_walk_cases_under_forced_bands_in_a_child_process(band, xmode, reverse):
    """A child process on the KNOBS build re-runs the WALK cases on 16-row tiles with bands of `band` rows in both directions,
    one XCD dealing and, once, the decoder's backwards walk.  Each child has its own timeout; once a child has ended by signal
    or timeout this test fails at once and starts no other."""
    from rustyhgi_amd import _ffi
    assert not _child_lost, "not started: the child under %s ended by signal or timeout" % (_child_lost[0],)
    knobs = os.path.join(os.path.dirname(_ffi.LIB_PATH), "libhgi_hip_knobs.so")
    assert os.path.exists(knobs), "libhgi_hip_knobs.so is missing: __graft_entry__.build() / `make -C rustyhgi_amd/csrc knobs` builds it"
    mode = dict(HGI_TILE_H="16", HGI_ENC_BAND=str(band), HGI_DEC_BAND=str(band), HGI_XCD_MODE=str(xmode))
    if reverse:
        mode["HGI_DEC_REVERSE"] = "1"
    env = dict(os.environ, HGI_LIB_PATH=knobs, **mode)
    cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider", "-k", "against_the_oracle"]
    try:
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired:
        _child_lost.append(mode)
        pytest.fail("%r: the child did not finish in 300 s" % (mode,))
    if r.returncode < 0:
        _child_lost.append(mode)
        pytest.fail("%r: the child ended by signal %d\n%s" % (mode, -r.returncode, r.stdout[-2000:] + r.stderr[-1000:]))
    assert r.returncode == 0, "%r\n%s" % (mode, r.stdout[-3000:] + r.stderr[-1000:])
    assert "%d passed" % len(PARTS) in r.stdout, r.stdout[-500:]
