"""One call for each of the 36 kernels of the four companion libraries (8 + 8 + 16 + 4), through the C entry points: what the
launchers' step from run-time choices to template arguments (rustyhgi_amd/companion/hgi_tile.h) picks must be the kernel of
that interpolator, table kind, depth and element size.  On these inputs a kernel of another INTERP, IDENT, SEEDED or E gives
other bytes.  Levels 3 and 6 are the unseeded tile and the cone.  A batch of two 300 x 150 frames: four interior tiles, a
ragged column, a ragged row and a corner each, so both paths of a kernel run.  Every side has a pitch of its own on a
4-byte-aligned base; inputs sit in parents of random bytes, outputs in sentinel-filled parents that are checked whole.
Expected bytes: the oracle.  Never libhgi_hip.so, never the library under test."""
import functools

import numpy as np
import pytest

import operand_designs as D
import typed_reference as TR
from conftest import SEED0
from kernel_calls import BF16, EKIND, ESIZE, F16, F32, PAIR_A, Plane, bank, dev, injective_table, same_dev

pytestmark = pytest.mark.gpu
B, H, W = 2, 150, 300
INTERPS, LEVELS = (1, 0), (3, 6)
TABLES = {"identity": np.arange(256, dtype=np.uint8), "lossy": D.tables()["random0"]}


@functools.lru_cache(maxsize=None)
def frames():
    """(B, H, W) random bytes: images for the encoders, grids for the decoders."""
    a = np.random.default_rng(SEED0 + 20).integers(0, 256, (B, H, W), dtype=np.uint8)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def decoded(levels, interp):
    from oracle import hgi_oracle as O
    return np.stack([O.decode(np.ascontiguousarray(g), levels, interp) for g in frames()])


@functools.lru_cache(maxsize=None)
def encoded(source, levels, interp, tname):
    """The oracle's grids of the frames themselves (source == "frames") or of their decode."""
    from oracle import hgi_oracle as O
    imgs = frames() if source == "frames" else decoded(levels, interp)
    return np.stack([O.encode(np.ascontiguousarray(a), levels, TABLES[tname], interp) for a in imgs])


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream or None


def side(row, gap, lead, data=None, seed=0):
    """A side of the batch as one plane of B * H rows, frames H pitches apart: an input around `data`, or an output."""
    p = Plane(B * H, row, row + gap, lead, random=data is not None, seed=seed + 1)
    return p if data is None else p.put(data.reshape(B * H, row))


def check(out, want, what):
    same_dev(out.rows().reshape(want.shape), want, what)
    out.intact(what)


@pytest.mark.parametrize("levels", LEVELS)
@pytest.mark.parametrize("tname", sorted(TABLES))
@pytest.mark.parametrize("interp", INTERPS)
def test_recon_kernels(oracle, interp, tname, levels):
    from rustyhgi_amd import _ffi_recon as R
    src = side(W, 20, 4, dev(frames()), seed=levels)
    grid, rec = side(W, 60, 8), side(W, 128, 16)
    R.check(R.lib().hgi_recon_encode_u8_dev(stream(), src.ptr, src.pitch, W, H, levels, interp, TABLES[tname].ctypes.data, grid.ptr, grid.pitch,
                                            rec.ptr, rec.pitch, B, H * src.pitch, H * grid.pitch, H * rec.pitch))
    want = encoded("frames", levels, interp, tname)
    what = "recon interp %d %s L%d" % (interp, tname, levels)
    check(grid, dev(want), what + " grid")
    check(rec, dev(np.stack([oracle.decode(g, levels, interp) for g in want])), what + " reconstruction")


@pytest.mark.parametrize("E", (2, 4))
@pytest.mark.parametrize("levels", LEVELS)
@pytest.mark.parametrize("interp", INTERPS)
def test_map_kernels(oracle, interp, levels, E):
    import torch
    from rustyhgi_amd import _ffi_map as M
    d_table = dev(injective_table(E, levels).view({2: np.int16, 4: np.int32}[E]))
    src = side(W, 12, 4, dev(frames()), seed=levels + E)
    out = side(W * E, 16 * E, 4 * E)
    M.check(M.lib().hgi_map_decode_dev(stream(), src.ptr, src.pitch, W, H, levels, interp, d_table.data_ptr(), E, out.ptr, out.pitch, B,
                                       H * src.pitch, H * out.pitch))
    want = d_table[dev(decoded(levels, interp)).long()].contiguous().view(torch.uint8).reshape(B, H, W * E)
    check(out, want, "map interp %d L%d E=%d" % (interp, levels, E))


TYPED = [(i, t, lv, k) for i in INTERPS for t in sorted(TABLES) for lv in LEVELS for k in (F16, F32)] + [(1, "lossy", 6, BF16)]


@pytest.mark.parametrize("interp,tname,levels,kind", TYPED)
def test_typed_kernels(oracle, interp, tname, levels, kind):
    import torch
    from rustyhgi_amd import _ffi_typed as T
    E = ESIZE[kind]
    bits = TR.lift(frames(), bank(kind, PAIR_A), levels)      # finite elements whose pixels are the frames'
    img = TR.quantize(TR.elements(kind, bits), *PAIR_A)
    want = np.stack([oracle.encode(np.ascontiguousarray(a), levels, TABLES[tname], interp) for a in img])
    d_bits = dev(bits.view({2: np.int16, 4: np.int32}[E])).view(torch.uint8)
    src = side(W * E, 6 * E, 4 * E, d_bits, seed=levels + E)
    before = src.buf.clone()
    grid = side(W, 60, 8)
    T.check(T.lib().hgi_typed_encode_dev(stream(), src.ptr, src.pitch, E, EKIND[kind], PAIR_A[0], PAIR_A[1], W, H, levels, interp,
                                         TABLES[tname].ctypes.data, grid.ptr, grid.pitch, B, H * src.pitch, H * grid.pitch))
    what = "typed interp %d %s L%d %s" % (interp, tname, levels, kind)
    check(grid, dev(want), what)
    assert torch.equal(src.buf, before), what + ": the image parent was modified"


@pytest.mark.parametrize("levels", LEVELS)
@pytest.mark.parametrize("interp", INTERPS)
def test_requant_kernels(oracle, interp, levels):
    from rustyhgi_amd import _ffi_requant as Q
    src = side(W, 36, 4, dev(frames()), seed=levels)
    dst = side(W, 60, 8)
    Q.check(Q.lib().hgi_requant_dev(stream(), src.ptr, src.pitch, W, H, levels, interp, TABLES["lossy"].ctypes.data, dst.ptr, dst.pitch, B,
                                    H * src.pitch, H * dst.pitch))
    check(dst, dev(encoded("decoded", levels, interp, "lossy")), "requant interp %d L%d" % (interp, levels))
