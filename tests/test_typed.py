"""CPU suite of typed encode (libhgi_typed.so, include/hgi_typed.h, Encoder.encode_typed, rustyhgi_amd.affine_inverse): the
companion library exports its three entry points and nothing else, names no tuning switch and reads no environment; the ctypes
table matches the header; the C entry point and the Python mirror refuse bad arguments before they touch a device; the kernel
unit compiles for gfx950 within its declared register budgets, with no static LDS, no scratch and no fused multiply-add, and
passes tools/check_isa.py; the two-sided host plan and the interval test hold under ASan / UBSan (a stand-alone program); the
conversion restated in tests/typed_reference.py is the torch CPU composition on every 16-bit pattern and inverts affine_table."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import typed_reference as TR
import companion_layer as CL
from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))

TYPED_DIR = os.path.join(ROOT, "rustyhgi_amd", "typed")
NAMES = ("hgi_typed_encode_dev", "hgi_typed_last_error", "hgi_typed_version")
ARGS = ["hip_stream", "d_img", "img_pitch", "elem_size", "elem_kind", "scale", "bias", "width", "height", "levels", "interp", "lut", "d_grid",
        "grid_pitch", "batch", "img_frame_stride", "grid_frame_stride"]


@pytest.fixture(scope="module")
def T():
    return CL.binding("typed")


def _header():
    return CL.header("typed")


def test_library_exports_exactly_the_three_entry_points(T):
    nm = shutil.which("nm")
    assert nm, "binutils nm is needed to list the exports"
    out = subprocess.check_output([nm, "-D", "--defined-only", T.LIB_PATH], text=True)
    exported = sorted(l.split()[-1].split("@")[0] for l in out.splitlines() if l.strip())
    assert exported == sorted(NAMES), exported
    script = open(os.path.join(TYPED_DIR, "hgi_typed.map")).read()
    assert re.search(r"global:\s*hgi_typed_\*;", script) and re.search(r"local:\s*\*;", script)
    declared = set(re.findall(r"HGI_API\s+[\w\s\*]+?\b(hgi_\w+)\s*\(", _header()))
    assert declared == set(NAMES) == set(s[0] for s in T.SYMBOLS)
    version = T.lib().hgi_typed_version()
    assert version.startswith(b"hgi_typed 1.0") and b"gfx950" in version
    # stateless and switch-free: no tuning-constant or switch name in the object, no environment read in the sources, nothing
    # of libhgi_hip.so linked
    strings = shutil.which("strings")
    assert strings, "binutils strings is needed to search the object for switch names"
    text = subprocess.check_output([strings, T.LIB_PATH], text=True)
    assert re.findall(r"HGI_[A-Z0-9_]+", text) == []
    CL.check_sources(TYPED_DIR, ["Makefile", "hgi_fused_typed_enc.hip", "hgi_typed.hip", "hgi_typed.map", "hgi_typed_kernels.h", "hgi_typed_plan.h"])
    mk = CL.makefile(TYPED_DIR, "typed", "hgi_fused_enc.hip")
    assert "-fvisibility=hidden" in mk and "-lhgi_hip" not in mk and "--version-script=hgi_typed.map" in mk
    for dep in re.findall(r'#include "(?:\.\./csrc/)?(hgi_[\w.]+)"', open(os.path.join(ROOT, "rustyhgi_amd", "csrc", "hgi_fused_impl.h")).read()):
        assert "$(CSRC)/" + dep in mk, dep + " is included by the tile procedure and missing from the Makefile's dependencies"
    for dep in ("hgi_fused_impl.h", "hgi_fused_enc.hip", "hgi_fused_pitched.h", "hgi_pitched.h", "hgi_kernels.h"):
        assert "$(CSRC)/" + dep in mk, dep
    readelf = shutil.which("readelf")
    assert readelf, "binutils readelf is needed to list what the library links"
    assert "libhgi_hip" not in subprocess.check_output([readelf, "-d", T.LIB_PATH], text=True)


def test_ctypes_table_matches_the_header(T):
    from rustyhgi_amd import _ffi
    ctype_of = {"const void *": _ffi._vp, "void *": _ffi._vp, "uint32_t": _ffi._u32, "size_t": _ffi._sz, "hgi_interp": _ffi._int,
                "float": ctypes.c_float, "const uint8_t *": _ffi._vp}
    m = re.search(r"HGI_API\s+hgi_status\s+hgi_typed_encode_dev\s*\(([^)]*)\)", _header())
    assert m
    decl = [" ".join(a.split()) for a in m.group(1).split(",")]
    want, names = [], []
    for a in decl:
        a = re.sub(r"^(.*?)(\w+)\[256\]$", r"\1*\2", a)      # `const uint8_t lut[256]` is a pointer
        t = re.sub(r"\s*\*\s*", " *", re.match(r"(.*?)\s*\w+$", a).group(1)).strip()
        assert t in ctype_of, a
        want.append(ctype_of[t])
        names.append(re.search(r"(\w+)$", a).group(1))
    assert names == ARGS
    table = dict((s[0], s) for s in T.SYMBOLS)
    _, res, got = table["hgi_typed_encode_dev"]
    assert len(decl) == 17 and res is _ffi._int and got == want, decl
    for n in ("hgi_typed_last_error", "hgi_typed_version"):
        assert re.search(r"HGI_API\s+const\s+char\s*\*\s*" + n + r"\s*\(\s*void\s*\)", _header()), n
        assert table[n][1] is ctypes.c_char_p and table[n][2] == []
    # the header takes hgi_status / hgi_interp from hgi.h and declares no type of its own
    assert '#include "hgi.h"' in open(os.path.join(ROOT, "include", "hgi_typed.h")).read()
    assert not re.search(r"\b(typedef|struct|enum)\b", _header())


def test_c_abi_refuses_bad_arguments_without_a_device(T):
    """Every HGI_EINVAL / HGI_EUNSUPPORTED rule of include/hgi_typed.h, decided before the first HIP call: the buffers here are
    host memory (or plain numbers where the shape is too large to exist) and are never touched -- a call that reached the
    launch would fail with HGI_EDEVICE on a machine without a GPU, or write, and neither happens."""
    from rustyhgi_amd import _ffi
    L = T.lib()
    im, g = np.zeros(8192, np.uint8), np.zeros(4096, np.uint8)
    lut = np.arange(256, dtype=np.uint8)
    I, G, LUT = im.ctypes.data + (-im.ctypes.data) % 4, g.ctypes.data, lut.ctypes.data
    E, U = _ffi.EINVAL, _ffi.EUNSUPPORTED
    err = L.hgi_typed_last_error

    def call(img=I, ip=72, elem=2, kind=0, scale=255.0, bias=0.0, w=32, h=8, levels=2, interp=1, lut=LUT, grid=G, gp=40, batch=1, ifs=600,
             gfs=320, stream=None):
        return L.hgi_typed_encode_dev(stream, img, ip, elem, kind, scale, bias, w, h, levels, interp, lut, grid, gp, batch, ifs, gfs)

    far = dict(img=1 << 50, grid=2 << 50)      # plain numbers: shapes too large to exist
    # HGI_EINVAL
    assert call(lut=None) == E and b"lut" in err()
    assert call(img=None) == E and call(grid=None) == E and b"NULL" in err()
    assert call(levels=32) == E and b"levels" in err()
    assert call(levels=2 ** 32 - 1) == E
    for elem in (0, 1, 3, 8):
        assert call(elem=elem, ip=32 * max(elem, 1)) == E and b"elem_size" in err(), elem
    assert call(kind=2) == E and b"elem_kind" in err()
    assert call(kind=2 ** 32 - 1) == E and b"elem_kind" in err()
    assert call(kind=1, elem=4, ip=128) == E and b"bfloat16" in err()
    assert call(img=I + 1) == E and b"aligned" in err()                       # an odd d_img at E = 2
    assert call(img=I + 2, elem=4, ip=128) == E and b"aligned" in err()
    assert call(ip=62) == E and b"image pitch" in err()                       # short
    assert call(ip=65) == E and b"multiple" in err()                          # not whole elements
    assert call(elem=4, ip=130) == E and b"multiple" in err()
    assert call(elem=4, ip=124) == E and b"image pitch" in err()
    assert call(gp=31) == E and b"grid pitch" in err()
    assert call(batch=2, gfs=7 * 40 + 31) == E and b"grid frame stride" in err()
    assert call(batch=2, ifs=7 * 72 + 62) == E and b"image frame stride" in err()
    assert call(batch=2, ifs=7 * 72 + 65) == E and b"multiple" in err()
    assert call(batch=2 ** 31) == E and b"batch" in err()
    for bad in (float("nan"), float("inf"), float("-inf"), 1e39):             # 1e39 is infinite as a float32
        assert call(scale=bad) == E and b"finite" in err(), bad
        assert call(bias=bad) == E and b"finite" in err(), bad
    # more tiles than a launch holds: 65536 x 32768 tiles of one frame (numbers only)
    assert call(w=128 << 16, h=64 << 15, gp=128 << 16, ip=256 << 16, **far) == E and b"tiles" in err()
    # any overlap of the two byte intervals (conservative)
    assert call(grid=I) == E and b"overlaps" in err()
    assert call(grid=I + 7 * 72 + 63) == E and b"overlaps" in err()            # the image's last byte
    assert call(grid=I - (7 * 40 + 31)) == E and b"overlaps" in err()          # the grid's last byte
    assert call(batch=2, ifs=7 * 72 + 64, grid=I + 2 * (7 * 72 + 64) - 2) == E  # the second image frame's last bytes
    assert call(elem=4, ip=128, grid=I + 7 * 128 + 127) == E and b"overlaps" in err()
    # HGI_EUNSUPPORTED: depth, 32-bit offsets on either side, the interpolator, the page rule
    for levels in (0, 9, 31):
        assert call(levels=levels) == U and b"levels" in err()
    for side in ("gp", "ip"):      # (8 + 192) * 2^25 >= 2^32 on one side at a time (numbers only)
        assert call(**{side: 1 << 25}, **far) == U and b"32-bit" in err(), side
    assert call(gp=1 << 32, **far) == U and b"32-bit" in err()      # a pitch >= 2^32
    assert call(ip=1 << 32, **far) == U and b"32-bit" in err()
    # the byte pitch is what counts: 2^24 elements of 4 bytes are refused
    assert call(elem=4, ip=4 << 24, **far) == U
    assert call(interp=7, **far) == U and b"interpolator" in err()
    assert call(interp=-1, **far) == U
    # 2-byte elements of an odd width whose span ends a page: the two tail bytes leave it (synthetic addresses)
    raw, page = CL.page_aligned(3 * 4096)
    w, h, ip = 31, 8, 72
    span = (h - 1) * ip + 2 * w
    assert call(img=page + 4096 - span, w=w) == U and b"tail" in err() and b"4-KiB" in err()
    assert call(img=page + 4096 - span, w=w, kind=1) == U and b"tail" in err()
    assert call(batch=2, ifs=span + 6, img=page + 2 * 4096 - (span + 6) - span, w=w) == U and b"tail" in err()
    assert call(img=(1 << 50) + 4096 - span, grid=2 << 50, w=w) == U and b"tail" in err()
    # ... the order of the two classes: a refusal of the first class when a rule of each is broken
    assert call(img=page + 4096 - span, w=w, gp=30) == E
    assert call(levels=0, elem=3) == E and call(levels=9, grid=I) == E and call(interp=7, scale=float("nan")) == E
    assert call(levels=9, lut=None) == E and call(ip=1 << 32, kind=2, **far) == E
    # empty calls succeed and do nothing (NULL buffers are fine there)
    assert call(batch=0) == _ffi.OK and call(w=0) == _ffi.OK and call(h=0) == _ffi.OK
    assert call(batch=0, img=None, grid=None, lut=None) == _ffi.OK
    # ... whatever their other arguments are: the empty test is decided first
    for kw in (dict(levels=0), dict(levels=9), dict(levels=32), dict(lut=None), dict(interp=7), dict(gp=1, ip=1), dict(grid=I), dict(elem=3),
               dict(img=I + 1), dict(kind=9), dict(scale=float("nan"))):
        assert call(batch=0, **kw) == _ffi.OK and call(w=0, **kw) == _ffi.OK and call(h=0, **kw) == _ffi.OK, kw
    assert (im == 0).all() and (g == 0).all() and (raw == 0).all()


def test_entry_point_decides_every_rule_before_the_first_hip_call():
    """hgi_typed.hip: in the entry point no HIP call stands before the launch, and the launch stands behind the last refusal."""
    CL.check_rule_order("typed", "hgi_typed_encode_dev", "launch_encode_typed")


@pytest.mark.timeout(900)
def test_typed_unit_is_within_its_budgets(tmp_path):
    """k_enc_typed<interp, identity, unseeded | cone, E>: sixteen kernels and no other, the encoder's SDWA byte chains really
    there, the hazard rules of tools/check_isa.py, no scratch, no spills, no DPP, no traps, no static LDS (the table's place is
    counted from LDS offset 0), the VGPRs within the waves per SIMD each kernel declares -- DESIGN.md 4.12: five, the byte
    encoder's -- and the conversion as the header words it: float32 denormals kept, a multiply and an add
    and never a fused one, round to nearest even, one saturating conversion."""
    import check_isa
    path = CL.isa("typed", tmp_path)
    r = check_isa.check(path)
    assert r["kernels"] == 16, r
    assert r["partial_writes"] > 400, r
    assert r["scratch_bytes"] == 0 and r["vgpr_spills"] == 0, r
    assert r["adjacent_dependent"] == 0 and r["store_data_overwritten"] == 0 and r["dpp"] == 0 and r["traps"] == 0, r
    text = open(path).read()
    assert len(set(re.findall(r"\b(_Z\w*k_enc_typed\w*):", text))) == 16
    assert "k_enc_tiles" not in text and "k_enc_pitched" not in text and "k_enc_recon" not in text
    assert not re.search(r"\bv_(pk_)?(fma|fmac|mac|mad)_(f32|legacy_f32)", text), "the conversion's two operations must stay two"
    assert "v_mul_f32" in text and "v_add_f32" in text and "v_rndne_f32" in text and "v_cvt_u32_f32" in text and "v_cvt_f32_f16" in text
    assert re.search(r"buffer_store_dwordx4 .* nt", text)
    res = CL.resources(text, "k_enc_typed")
    assert len(res) == 16, res
    assert len(re.findall(r"\.amdhsa_float_denorm_mode_32 3\b", text)) == 16 and not re.search(r"\.amdhsa_float_denorm_mode_32 [012]\b", text)
    # 512 VGPRs per SIMD lane, allocated in eights: waves w -> at most (512 / w) rounded down to a multiple of 8
    budget = {(0, 4): 96, (0, 2): 96, (2, 4): 96, (2, 2): 96}      # (SEEDED, E) -> five waves per SIMD, the byte encoder's
    seen = set()
    for k, (vgprs, lds, scratch) in res.items():
        m = re.search(r"k_enc_typedILi(\d)ELb(\d)ELi(\d)ELi(\d)E", k)
        assert m, k
        interp, ident, seeded, e = (int(v) for v in m.groups())
        seen.add((interp, ident, seeded, e))
        assert lds == 0 and scratch == 0, (k, lds, scratch)
        assert vgprs <= budget[(seeded, e)], (k, vgprs)
    assert seen == {(i, d, s, e) for i in (0, 1) for d in (0, 1) for s in (0, 2) for e in (2, 4)}
    src = CL.unit_source("typed", "hgi_fused_enc.hip")      # ... the uniform encoder's dynamic LDS, nothing added
    assert "constexpr int kTypedWavesPerEu = HGI_ENC_WAVES_PER_EU;" in src
    assert "amdgpu_waves_per_eu(kTypedWavesPerEu)" in src


def test_plan_and_intervals_under_asan_ubsan(tmp_path):
    """tests/cpp/test_typed_plan.cpp, a stand-alone program: random shapes, pitches, strides, addresses, batches and element
    sizes; every block walked through the map, every 32-bit offset of both sides bounded against the records, the fits, page
    and interval rules against brute force."""
    CL.run_plan_program("typed", tmp_path)


def _torch_quantize(x, scale, bias):
    """The torch CPU composition: clamp(round(x * scale + bias), 0, 255), NaN -> 0."""
    import torch
    t = torch.add(torch.mul(x.to(torch.float32), float(np.float32(scale))), float(np.float32(bias)))
    v = torch.where(torch.isnan(t), torch.zeros_like(t), t).round().clamp(0, 255)
    return v.to(torch.uint8).numpy()


def test_quantize_restates_the_torch_composition():
    """All 65 536 float16 patterns, all 65 536 bfloat16 patterns and 2^20 random float32 bit patterns (with the specials of the
    GPU suite), under the three (scale, bias) pairs and (1, 0)."""
    torch = pytest.importorskip("torch")
    u16 = np.arange(1 << 16, dtype=np.uint16)
    rng = np.random.default_rng(0x48474950)
    u32 = rng.integers(0, 1 << 32, 1 << 20, dtype=np.uint64).astype(np.uint32)
    u32[:8] = (0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0x7FA00001, 0xFFC12345, 0x00600000)
    halves = np.arange(256, dtype=np.float32) + np.float32(0.5)
    u32[8:8 + 768] = np.concatenate([np.nextafter(halves, np.float32(-1e9)), halves, np.nextafter(halves, np.float32(1e9))]).view(np.uint32)
    cases = ((u16.view(np.float16), torch.from_numpy(u16.view(np.float16).copy())),
             (u16, torch.from_numpy(u16.view(np.int16).copy()).view(torch.bfloat16)),
             (u32.view(np.float32), torch.from_numpy(u32.view(np.float32).copy())))
    for scale, bias in TR.PAIRS + ((1.0, 0.0),):
        for x, t in cases:
            got, want = TR.quantize(x, scale, bias), _torch_quantize(t, scale, bias)
            assert got.dtype == np.uint8 and (got == want).all(), (scale, bias, x.dtype, int((got != want).sum()))
    # the widening is exact: bfloat16 bit patterns through torch and through the helper
    assert (TR.widen(u16).view(np.uint32) == torch.from_numpy(u16.view(np.int16).copy()).view(torch.bfloat16).float().numpy().view(np.uint32)).all()
    # ties go to even, NaN to 0, infinities clamp, denormals count
    f = lambda *v: np.array(v, np.float32)
    assert TR.quantize(f(0.5, 1.5, 2.5, 253.5, 254.5, 255.5, -0.5), 1.0, 0.0).tolist() == [0, 2, 2, 254, 254, 255, 0]
    assert TR.quantize(f(np.nan, -np.nan, np.inf, -np.inf, 1e30, -1e30), 1.0, 0.0).tolist() == [0, 0, 255, 0, 255, 0]
    assert TR.quantize(f(np.inf, -np.inf), 0.0, 0.0).tolist() == [0, 0]
    assert TR.quantize(np.array([0.75 * 2.0 ** -126], np.float32), 2.0 ** 127, 0.0).tolist() == [2]
    # bf16_bits is torch's rounding
    x32 = rng.standard_normal(1 << 16).astype(np.float32) * np.float32(100)
    assert (TR.bf16_bits(x32) == torch.from_numpy(x32).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)).all()


def test_the_conversion_inverts_the_tables():
    """quantize(affine_table(dtype), 255, 0) == arange(256) for the three dtypes; the mean / std table (0.449, 0.226) is inverted
    by affine_inverse at float16 and float32."""
    torch = pytest.importorskip("torch")
    import rustyhgi_amd
    from rustyhgi_amd.mapping import affine_inverse, affine_table
    assert rustyhgi_amd.affine_inverse is affine_inverse
    ramp = np.arange(256, dtype=np.uint8)
    for dtype in (np.float16, np.float32):
        assert (TR.quantize(affine_table(dtype), 255.0, 0.0) == ramp).all(), dtype
    bf = affine_table(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert (TR.quantize(bf, 255.0, 0.0) == ramp).all()
    s, b = 1 / 255 / 0.226, -0.449 / 0.226
    scale, bias = affine_inverse(s, b)
    assert isinstance(scale, np.float32) and isinstance(bias, np.float32)
    assert scale == np.float32(1) / np.float32(s) and bias == -np.float32(b) / np.float32(s)
    for dtype in (np.float16, np.float32):
        assert (TR.quantize(affine_table(dtype, s, b), scale, bias) == ramp).all(), dtype
    d0, d1 = affine_inverse()
    assert d0 == np.float32(1) / np.float32(1 / 255) and d1 == 0


def _encoder(levels=4):
    from rustyhgi_amd import Encoder
    from rustyhgi_amd.interpolator import Crossed
    from rustyhgi_amd.quantizator import Linear, QuantizationLevel
    return Encoder(Crossed(), Linear(QuantizationLevel.Medium), levels)      # constructing it touches no device


def test_python_mirror_refuses_bad_arguments_before_any_device_call(T):
    torch = pytest.importorskip("torch")
    call = _encoder().encode_typed
    base = torch.zeros((3, 64, 160), dtype=torch.float16)
    v = base[:, 8:40, 16:100]
    for bad in (np.zeros((3, 8, 8), np.float16), None, [[1.0]], base.to(torch.float64), base.to(torch.uint8), base.to(torch.int16)):
        with pytest.raises(ValueError):
            call(bad)
    for bad in (base[:, :, ::2], base.reshape(-1), base.transpose(1, 2), base[None]):
        with pytest.raises(ValueError):
            call(bad)
    for kw in (dict(scale=float("nan")), dict(bias=float("inf")), dict(scale=1e39)):
        with pytest.raises(ValueError, match="finite"):
            call(v, **kw)
    other = torch.zeros((3, 64, 200), dtype=torch.uint8)
    for buf in (other[:, 8:40, 16:99], other[:2, 8:40, 16:100], other[:, 8:40, 16:184:2], other[:, 8:40, 16:100].to(torch.int8),
                np.zeros((3, 32, 84), np.uint8), torch.zeros((3, 32, 84), dtype=torch.float16)):
        with pytest.raises(ValueError, match="out"):
            call(v, out=buf)
    # shared memory: a uint8 window of the frames' own storage
    alias = base.view(torch.uint8)[:, 8:40, 16:100]
    with pytest.raises(ValueError, match="shares memory"):
        call(v, out=alias)
    # a valid view passes the layout checks and only then meets the CPU tensor
    with pytest.raises(ValueError, match="GPU"):
        call(v)
    with pytest.raises(ValueError, match="GPU"):
        call(v.to(torch.bfloat16), out=other[:, 8:40, 16:100])
    # empty views need no device
    r = call(base[:, :0])
    assert tuple(r.shape) == (3, 0, 160) and r.dtype == torch.uint8
    r = call(torch.zeros((5, 0), dtype=torch.float32))
    assert tuple(r.shape) == (5, 0)


def test_build_entry_builds_the_companion_library():
    CL.check_build_entry("typed", after="map")
