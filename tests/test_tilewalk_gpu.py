"""The uniform kernels' block -> tile walk on the device (rustyhgi_amd/csrc/hgi_tilewalk.h; walked on the CPU by
tests/cpp/test_tilewalk.cpp, and tests/test_geometry_coverage.py shows what the cases below reach).

The WALK cases (tests/geometry_designs.py:walk_cases) are 600 small launches -- 1 ... 3 interior tile columns with and without
a ragged one, 1 ... 24 interior rows of 16-row tiles with and without a ragged one, 1 ... 9 frames -- through
hgi_encode_u8_dev / hgi_decode_u8_dev at three levels, against the oracle.  Every output lies in a sentinel-filled buffer that
is checked whole: a tile that no block reaches leaves sentinels behind, a tile reached twice by different frames' blocks
shows as wrong bytes.  In-process they run on the release library with its own policy (bands of 4 or 8 rows, round-robin
dealing where a launch has eight whole bands); children on the knobs build force 16-row tiles, bands of 1 ... 4 rows, both
XCD dealings and the backwards walk, which the release library reaches on wide or huge frames only.

hgi_typed_encode_dev takes its block -> tile map from the pitched plan (rustyhgi_amd/typed/hgi_typed_plan.h): the same cases go
through it in-process, with a pitch on both sides.  Its library has no knobs build, so it has no children."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import geometry_designs as G
import typed_reference as TR
from kernel_calls import EKIND, H, Pool, bank, ctxs, typed_choice  # noqa: F401

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


@pytest.mark.parametrize("ex", (1, 2, 3))
def test_walk_cases_through_typed_encode(H, ex):
    """The WALK cases with `ex` interior tile columns through hgi_typed_encode_dev at three levels, Crossed: element size
    alternating 2 / 4 by case, the table linear_lut(2) / identity by pairs of cases, the frames lifted to elements that convert
    to exactly the cases' pixels (tests/typed_reference.py:preimages) and read through a pitch, the grids written through one;
    one sentinel-filled buffer compared whole, the inputs unchanged."""
    import torch
    from rustyhgi_amd import _ffi_typed as T
    stream = torch.cuda.current_stream().cuda_stream or None
    inp, out, calls = Pool(False, 810 + ex), Pool(True), []
    for k, (w, h, b) in enumerate(c for c in G.walk_cases() if c[0] // 128 == ex):
        esz, tname = (2, 4)[k % 2], ("linear2", "identity")[(k // 2) % 2]
        kind, pair = typed_choice(esz, k // 2)
        img, grid, _ = frames_of(w, h, tname)
        frames = np.ascontiguousarray(TR.lift(img[:b], bank(kind, pair), k)).view(np.uint8).reshape(b, h, w * esz)
        pi, pg = (w + (1, 3, 16, 61)[k % 4]) * esz, (w + 3) | 1
        si, sg = h * pi + 2 * esz, h * pg + 1
        calls.append((w, h, b, esz, EKIND[kind], pair, table(tname), pi, pg, si, sg,
                      inp.add(frames, pi, si, align=esz, phase=esz * (k % (16 // esz)), tail_safe=esz == 2 and w % 2 == 1),
                      out.add(grid[:b], pg, sg, lead=17, tag="%d x %d batch %d typed %s %s" % (w, h, b, kind, tname))))
    assert len(calls) == 200
    inp.upload(), out.upload()
    for w, h, b, esz, ekind, pair, lut, pi, pg, si, sg, i_img, o in calls:
        T.check(T.lib().hgi_typed_encode_dev(stream, inp.ptr + i_img, pi, esz, ekind, pair[0], pair[1], w, h, LEVELS, 1, lut.ctypes.data,
                                             out.ptr + o, pg, b, si, sg))
    what = "typed walk cases ex %d" % ex
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
