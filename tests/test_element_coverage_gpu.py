"""GPU suite of the element-coverage designs (tests/element_designs.py; what they cover is asserted on the CPU in
tests/test_element_coverage.py): for every kind and (scale, bias) pair a rotation batch -- as many frames as the class bank has
elements, position (x, y) of frame f holding element (a x + b y + f) mod n -- so that every position of the 293 x 191 frame,
hence every site at which the kernel converts (the chunk conversions of its own rows by byte lane, the halo-row chunk, the
halo-column singles, the cone's points), meets every float class once: ties both ways and their neighbours, negative and
too-large elements, infinities, the three NaNs, both zeros, a denormal whose product counts, products that overflow, elements
that an fma would convert to another pixel.  Each of the sixteen instantiations of the typed kernel runs every kind its element
size serves under every pair of the kind; the lossless instantiations under the identity, the others under identity_but_255 and
under the lossy random0, without which what a tile converts only to reconstruct its halo could not reach the grid.  The same
batches go through the composed route of Encoder.encode_typed at nine levels.
Expected bytes: oracle.encode(typed_reference.quantize(frame)).  Never the library under test."""
import functools

import numpy as np
import pytest

import element_designs as E
import typed_reference as TR
from kernel_calls import ESIZE, H, run_typed_raw  # noqa: F401

pytestmark = pytest.mark.gpu
TABLES = E.tables()
CASES = [(i, d, s, e, kind) for (i, d, s, e), (kinds, _, _) in sorted(E.instantiations().items()) for kind in kinds]
COMPOSED = [(kind, p) for kind in E.KINDS for p in E.KIND_PAIRS[kind]]
SIGNED = {2: np.int16, 4: np.int32}


def calls_of(interp, ident, seeded, esz, kind):
    """[(pair name, levels, table name)] of one instantiation and kind (tests/element_designs.py:instantiations)."""
    kinds, levels, tnames = E.instantiations()[interp, ident, seeded, esz]
    assert kind in kinds
    return [(p, lv, t) for p in E.KIND_PAIRS[kind] for lv in levels for t in tnames]


_stage = []


def upload(a):
    """A host array to the device through ONE page-locked staging buffer, allocated on first use and reused.  Why pinned: the
    module makes some three hundred uploads of 1.7 - 7 MB, and from pageable arrays each would have the runtime pin and release
    a fresh range of the heap.  Copies between the device and fresh pageable memory are where whole-suite runs of this project
    have met faults of unknown cause (profiles/r18_element_coverage.md, section 9); this file makes none."""
    import torch
    a = np.ascontiguousarray(a)
    flat = a.reshape(-1).view(np.uint8)
    if not _stage or _stage[0].numel() < flat.size:
        _stage[:] = [torch.empty((max(flat.size, 8 << 20),), dtype=torch.uint8).pin_memory()]
    _stage[0].numpy()[:flat.size] = flat
    out = torch.empty((flat.size,), dtype=torch.uint8, device="cuda")
    out.copy_(_stage[0][:flat.size])      # blocking: the buffer is free again on return
    return out.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[a.dtype.itemsize]).reshape(a.shape)


@functools.lru_cache(maxsize=None)
def frames(kind, pname):
    """(bits on the device as int16 / int32, reference pixels on the host), (n, h, w) each."""
    bits, px = E.rotation(kind, pname)
    assert (px == TR.quantize(TR.elements(kind, bits), *E.f32pair(pname))).all()
    return upload(bits.view(SIGNED[ESIZE[kind]])), px


def expected(kind, pname, levels, interp, tname):
    """The oracle's grids of the batch, on the device.  Not cached: every (kind, pair, levels, interpolator, table) occurs in
    exactly one case, and the self-check computes its own."""
    from oracle import hgi_oracle as O
    O.build()
    _, px = frames(kind, pname)
    return upload(np.stack([O.encode(f, levels, TABLES[tname], interp) for f in px]))


@pytest.mark.parametrize("interp,ident,seeded,esz,kind", CASES, ids=["i%d-%s-s%d-E%d-%s" % (i, "ident" if d else "table", s, e, k) for i, d, s, e, k in CASES])
def test_every_class_at_every_site(H, interp, ident, seeded, esz, kind):
    """One instantiation k_enc_typed<INTERP, IDENT, SEEDED, E> and one kind: the rotation batch of every pair of the kind, at
    the depths and under the tables of the instantiation, bit for bit against the oracle; sentinels and inputs intact."""
    import torch
    n = 0
    for pname, levels, tname in calls_of(interp, ident, seeded, esz, kind):
        lut = np.ascontiguousarray(TABLES[tname])
        assert bool((lut == np.arange(256)).all()) == ident and (levels >= 6) == (seeded == 2) and ESIZE[kind] == esz
        d_bits, _ = frames(kind, pname)
        run_typed_raw(d_bits, expected(kind, pname, levels, interp, tname), kind, E.f32pair(pname), levels, interp, lut,
                      "%s %s" % (pname, tname), gap=(1, 3, 16, 61)[n % 4], lead=1 + n % 7, extra=2 + n % 5, seed=n)
        n += 1
    torch.cuda.synchronize()
    print("i%d ident %d seeded %d E%d %s: %d batches" % (interp, ident, seeded, esz, kind, n))


@pytest.mark.parametrize("kind", E.KINDS)
def test_composed_route_at_nine_levels(H, kind):
    """Encoder.encode_typed at nine levels, which the launch refuses: the torch conversion (mul, add, where(isnan), round,
    clamp) and encode_view promise the same bytes.  The same rotation batches, one call per pair, Crossed and Medium -- a
    lossy table, so what the deep levels reconstruct from reaches the grid."""
    import torch
    from oracle import hgi_oracle as O
    from rustyhgi_amd.interpolator import Crossed
    from rustyhgi_amd.quantizator import Linear, QuantizationLevel
    O.build()
    tdt = {E.F16: torch.float16, E.BF16: torch.bfloat16, E.F32: torch.float32}[kind]
    lut = O.linear_lut(O.MEDIUM)[0]
    enc = H.Encoder(Crossed(), Linear(QuantizationLevel.Medium), 9)
    assert (enc._lut == lut).all()
    for k, p in COMPOSED:
        if k != kind:
            continue
        d_bits, px = frames(kind, p)
        x = d_bits.view(tdt)
        before = d_bits.clone()
        scale, bias = E.f32pair(p)
        got = enc.encode_typed(x, scale, bias)
        torch.cuda.synchronize()
        want = np.stack([O.encode(f, 9, lut, 1) for f in px])
        if not torch.equal(got, upload(want)):      # the host report only on a mismatch
            a = got.cpu().numpy()
            f, y, xx = np.argwhere(a != want)[0]
            idx = (E.rotation_index(*E.SHAPE, px.shape[0])[y, xx] + f) % px.shape[0]
            raise AssertionError("composed %s under %s: %d mismatches, first in frame %d at (x=%d, y=%d), whose element is the class %r"
                                 % (kind, p, int((a != want).sum()), f, xx, y, E.bank(kind, p)[0][idx]))
        assert torch.equal(d_bits, before)


def test_the_harness_notices_one_element_of_another_class(H):
    """The float16 batch under (1, 37.25) at five levels with ONE element of the uploaded frames -- the last of the last frame --
    replaced by a quiet NaN, an element of another class and pixel: the comparison raises and names a position next to it.  The batch
    as it is passes."""
    import torch
    kind, pname, levels, tname = E.F16, "A", 5, "identity_but_255"
    names, bank_bits, bank_px = E.bank(kind, pname)
    d_bits, px = frames(kind, pname)
    want = expected(kind, pname, levels, 1, tname)
    lut = np.ascontiguousarray(TABLES[tname])
    run_typed_raw(d_bits, want, kind, E.f32pair(pname), levels, 1, lut, "self-check")
    nan = int(bank_bits[names.index("qnan")])
    assert bank_px[names.index("qnan")] == 0 != px[-1, -1, -1]
    bad = d_bits.clone()
    bad[-1, -1, -1] = int(np.array([nan], np.uint16).view(np.int16)[0])
    with pytest.raises(AssertionError, match=r"self-check typed float16 .* mismatches, first at \(x=29\d, y=1[89]\d"):
        run_typed_raw(bad, want, kind, E.f32pair(pname), levels, 1, lut, "self-check")
    torch.cuda.synchronize()
