"""Element-coverage designs (a helper module of tests/test_element_coverage*.py, not a conftest).

Where tests/operand_designs.py enumerates the VALUES the per-pixel code meets and tests/geometry_designs.py the SHAPES, this
module enumerates the FLOAT CLASSES the conversion of typed encode meets (include/hgi_typed.h):

    t = fl32(fl32(x * scale) + bias)      two roundings, never an fma
    v = 0 if t is NaN, else clamp(rint(t), 0, 255)      half to even, +-inf clamp, denormals kept

and the SITES at which the kernel converts.  Everything is defined from the header, tests/typed_reference.py and the oracle:

1. `convert`: the twin of typed_reference.quantize with the thirteen mutants of the rule; `fma32`, the exact single rounding;
2. `bank`: per kind and (scale, bias) pair the class bank -- element bit patterns found by search, one per class the pair
   expresses, and ordinary in-range elements up to a prime size; `exemption`: the (mutant, kind, pair) that provably equal
   the contract, each with its proof;
3. `rotation`: a batch of n frames (n the bank's size) in which position (x, y) of frame f holds element (a x + b y + f) mod n;
4. `sites`: the read set of every tile of a shape by site class, restated from the file header of
   rustyhgi_amd/typed/hgi_fused_typed_enc.hip and DESIGN.md 4.12 -- which positions a tile reads through which conversion,
   not what it computes;
5. `census`: a (site, mutant) is killed when the oracle's grid of the view -- the reference pixels with the site's positions
   replaced by the mutant's -- differs from the reference grid inside the tile, for some frame of the batch.
"""
import fractions
import functools

import numpy as np

import operand_designs as D
import typed_reference as TR

F16, BF16, F32 = "float16", "bfloat16", "float32"
KINDS = (F16, BF16, F32)
LEFTTOP, CROSSED = 0, 1
TW, TH = 128, 64

# name -> (scale, bias).  `fma`: the product is inexact, so one rounding can differ from two.  `A`, `B`: the pairs of the
# coverage suites, under which the element 0.0 is pixel 37 / 255.  `den127`, `den23`: power-of-two scales that lift a
# denormal element to a product >= 0.5 (float32 and bfloat16 share the exponent range; a float16 denormal is m * 2^-24);
# 2^127 also makes finite elements overflow.  `zero`: scale 0 turns +-inf into NaN, and every finite element into the tie 36.5.
PAIRS = {"fma": (0.1, 0.05), "fmb": (0.9, 0.35), "A": (1.0, 37.25), "B": (-3.5, 300.0), "den127": (2.0 ** 127, 0.0), "den23": (2.0 ** 23, 0.0),
         "zero": (0.0, 36.5)}
# bfloat16 under B reaches 224 of the 256 values (tests/test_typed_coverage.py): it runs under the others
KIND_PAIRS = {F16: ("fma", "A", "B", "den23", "den127", "zero"), BF16: ("fma", "fmb", "A", "den127", "zero"),
              F32: ("fma", "A", "B", "den127", "zero")}
MUTANTS = ("fma", "half_away", "half_up", "trunc", "nan_to_255", "nan_as_zero_element", "neg_wraps", "over_wraps", "inf_to_0",
           "ftz_input", "f16_denormal_flushed", "kind_swapped", "minus_zero_as_nan")
CLASSES = ("finite_tie", "tie_down", "tie_down_below", "tie_down_above", "tie_up", "tie_up_below", "tie_up_above", "negative", "over", "pinf",
           "ninf", "qnan", "snan", "negnan", "pzero", "nzero", "denormal", "overflow_pos", "overflow_neg", "fma")
SPECIALS = {      # kind -> class -> bit pattern
    F16: dict(pinf=0x7C00, ninf=0xFC00, qnan=0x7E00, snan=0x7D01, negnan=0xFE55, pzero=0x0000, nzero=0x8000),
    BF16: dict(pinf=0x7F80, ninf=0xFF80, qnan=0x7FC0, snan=0x7FA1, negnan=0xFFC5, pzero=0x0000, nzero=0x8000),
    F32: dict(pinf=0x7F800000, ninf=0xFF800000, qnan=0x7FC00000, snan=0x7FA00001, negnan=0xFFC12345, pzero=0x00000000, nzero=0x80000000),
}
EXP_MASK = {F16: 0x7C00, BF16: 0x7F80, F32: 0x7F800000}
SIGN = {F16: 0x8000, BF16: 0x8000, F32: 0x80000000}


def f32pair(name):
    s, b = PAIRS[name]
    return float(np.float32(s)), float(np.float32(b))


# ------------------------------------------------------------------------------------------ exact single rounding
def round_fraction_to_f32(v):
    """A rational, rounded ONCE to float32 (nearest, ties to even; denormals kept; overflow to infinity)."""
    if v == 0:
        return np.float32(0.0)
    a = abs(v)
    e = a.numerator.bit_length() - a.denominator.bit_length()      # 2^(e-1) < a < 2^(e+1)
    if a < fractions.Fraction(2) ** e:
        e -= 1
    q = fractions.Fraction(2) ** (max(e, -126) - 23)
    r = round(a / q) * q                                             # round(Fraction) rounds half to even
    out = np.float32(np.inf) if r >= fractions.Fraction(2) ** 128 else np.float32(float(r))
    return -out if v < 0 else out


def fma32_exact(x, scale, bias):
    """fl32(x * scale + bias) of three float32 scalars, the exact sum rounded once (fractions.Fraction: Python 3.10 has no
    math.fma, and a double-precision sum rounds twice)."""
    x, s, b = np.float32(x), np.float32(scale), np.float32(bias)
    if not np.isfinite(x):
        with np.errstate(all="ignore"):
            return x * s + b
    return round_fraction_to_f32(fractions.Fraction(float(x)) * fractions.Fraction(float(s)) + fractions.Fraction(float(b)))


def fma32(x, scale, bias):
    """fma32_exact over an array.  The product of two float32 is exact in float64; the float64 sum s with its two-sum error e
    holds the exact value s + e; rounding s to float32 is rounding the exact value unless s lies exactly half way between two
    float32 and e != 0 (|e| is at most half an ulp of s, so it cannot carry s across any other boundary): those elements,
    and no others, are recomputed with fractions."""
    x = np.asarray(x, np.float32)
    s64, b64 = np.float64(np.float32(scale)), np.float64(np.float32(bias))
    with np.errstate(all="ignore"):
        two = x * np.float32(scale) + np.float32(bias)
        p = x.astype(np.float64) * s64
        s = p + b64
        bb = s - p
        e = (p - (s - bb)) + (b64 - bb)
        r = s.astype(np.float32)
        up, dn = np.nextafter(r, np.float32(np.inf)), np.nextafter(r, np.float32(-np.inf))
        mid = (s == (r.astype(np.float64) + up.astype(np.float64)) / 2) | (s == (r.astype(np.float64) + dn.astype(np.float64)) / 2)
    fin = np.isfinite(x)
    out = np.where(fin, r, two)
    for i in np.flatnonzero((fin & mid & (e != 0)).reshape(-1)):
        out.reshape(-1)[i] = fma32_exact(x.reshape(-1)[i], scale, bias)
    return out


# ---------------------------------------------------------------------------- the conversion and its mutants
def convert(kind, bits, scale, bias, mutant=None):
    """Bit patterns -> pixels: typed_reference.quantize restated step by step, with the mutants of each step.
    `fma` one rounding; `half_away` / `half_up` / `trunc` the rounding (half_up is floor(t + 0.5) in float32); `nan_to_255`,
    `nan_as_zero_element` (NaN takes the pixel of 0.0) the NaN rule; `neg_wraps` / `over_wraps` an integer conversion and
    & 255 instead of the clamp on one side; `inf_to_0` an infinite t; `ftz_input` a float32-denormal input flushed;
    `f16_denormal_flushed` a float16 denormal flushed before widening; `kind_swapped` float16 read as bfloat16 and the
    reverse; `minus_zero_as_nan` the element -0.0 taken for a NaN."""
    assert mutant is None or mutant in MUTANTS
    bits = np.ascontiguousarray(bits, TR.KINDS[kind])
    read_as = kind
    if mutant == "kind_swapped" and kind != F32:
        read_as = BF16 if kind == F16 else F16
    if mutant == "f16_denormal_flushed" and kind == F16:
        bits = np.where((bits & 0x7C00) == 0, bits & 0x8000, bits).astype(np.uint16)
    x = TR.widen(TR.elements(read_as, bits))
    s, b = np.float32(scale), np.float32(bias)
    with np.errstate(all="ignore"):
        if mutant == "ftz_input":
            x = np.where(np.abs(x) < np.float32(2.0 ** -126), np.copysign(np.float32(0), x), x)
        t = fma32(x, s, b) if mutant == "fma" else x * s + b
        nan = np.isnan(t)
        if mutant == "minus_zero_as_nan":
            nan = nan | ((x == 0) & np.signbit(x))
        tie = np.isfinite(t) & (t - np.floor(t) == np.float32(0.5))
        if mutant == "half_away":
            r = np.where(tie, np.trunc(t) + np.sign(t), np.rint(t))
        elif mutant == "half_up":
            r = np.floor(t + np.float32(0.5))
        elif mutant == "trunc":
            r = np.trunc(t)
        else:
            r = np.rint(t)
        r = np.where(nan, np.float32(0), r)
        v = np.clip(r, np.float32(0), np.float32(255)).astype(np.int64)
        i = np.clip(r.astype(np.float64), -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64)      # a saturating integer conversion
        if mutant == "neg_wraps":
            v = np.where(r < 0, i & 255, v)
        if mutant == "over_wraps":
            v = np.where(r > 255, i & 255, v)
        if mutant == "inf_to_0":
            v = np.where(np.isinf(t), 0, v)
        nan_pixel = 0
        if mutant == "nan_to_255":
            nan_pixel = 255
        elif mutant == "nan_as_zero_element":
            nan_pixel = int(TR.quantize(np.zeros(1, np.float32), scale, bias)[0])
        v = np.where(nan, nan_pixel, v)
    return v.astype(np.uint8)


def _pow2_or_zero(s):
    s = abs(float(np.float32(s)))
    return s == 0.0 or float(np.log2(s)).is_integer()


def exemption(mutant, kind, pname):
    """The proof that `mutant` IS the contract for every element of `kind` under the pair, or None.  Nothing is exempt by
    count; tests/test_element_coverage.py checks every proof about a 2-byte kind on all 65 536 patterns."""
    scale, bias = f32pair(pname)
    zero_px = int(TR.quantize(np.zeros(1, np.float32), scale, bias)[0])
    if mutant == "kind_swapped" and kind == F32:
        return "float32 has one kind: there is nothing to swap"
    if mutant == "f16_denormal_flushed":
        if kind != F16:
            return "the mutant flushes float16 denormals; this kind has none"
        if abs(scale) <= 3.5:
            return ("a float16 denormal is below 2^-14: times |scale| <= 3.5 it moves t by less than 2^-12 from bias, and no bias in "
                    "use (0.05, 37.25, 300, 36.5 under scale 0) lies within 2^-12 of a rounding boundary it is not on")
    if mutant == "ftz_input":
        if kind == F16:
            return "every float16 widens to zero or a NORMAL float32 (2^-24 and up): no input is a float32 denormal"
        if abs(scale) <= 3.5:
            return ("a float32 denormal is below 2^-126: times |scale| <= 3.5 its product is below 2^-124, less than half an ulp of "
                    "every bias in use, so t is what 0.0 gives")
    if mutant == "fma":
        if _pow2_or_zero(scale):
            return "scale is 0 or a power of two >= 1: the product is exact (overflow included), so rounding once is rounding twice"
        if kind != F32 and pname == "B":
            return "a significand of 11 bits or fewer times 3.5 (3 bits) fits 24 bits: the product is exact"
    if scale == 0.0:
        if mutant in ("trunc", "neg_wraps", "over_wraps"):
            return "scale 0: t is bias = 36.5 or NaN -- never negative, never above 255, and trunc(36.5) = 36 is the even neighbour"
        if mutant == "inf_to_0":
            return "scale 0: t is bias or NaN, never infinite"
    if kind == F16 and pname == "den127" and mutant in ("half_away", "half_up", "trunc", "neg_wraps", "over_wraps"):
        return ("a nonzero float16 is at least 2^-24 in magnitude: times 2^127 t is an integer of 2^103 and more, which no rounding "
                "moves and whose saturated integer conversion has the low byte of the clamp (0x7fffffff -> 255, 0x80000000 -> 0)")
    if mutant == "nan_as_zero_element" and zero_px == 0:
        return "the element 0.0 is pixel 0 under this pair, which is what a NaN gives"
    if mutant == "minus_zero_as_nan" and zero_px == 0:
        return "the element -0.0 is pixel clamp(rint(bias)) = 0 under this pair, which is what a NaN gives"
    return None


# --------------------------------------------------------------------------------------------------- the banks
def _candidates(kind, scale, bias):
    """The pool the classes are searched in: every pattern of a 2-byte kind; float32: the specials, the elements
    fl32((v + d - bias) / scale) for v = -200 ... 455 and d around the rounding boundaries, a walk of +-40 ulp around each
    (the fma elements lie there), the denormal range and a few huge elements."""
    if kind != F32:
        return np.arange(1 << 16, dtype=np.uint16)
    pool = [np.array(list(SPECIALS[F32].values()), np.uint32)]
    huge = np.array([4.0, -4.0, 1e30, -1e30, 3.0e38, -3.0e38, 1e-30, -1e-30], np.float32)
    den = np.array([0.75 * 2.0 ** -126] + [(k + d) * 2.0 ** -127 for k in range(0, 6) for d in (0.25, 0.5, 0.75)], np.float32)
    pool += [huge.view(np.uint32), den.view(np.uint32), np.arange(1, 64, dtype=np.uint32), np.arange(1, 64, dtype=np.uint32) | np.uint32(0x80000000)]
    if scale != 0:
        v = np.arange(-200, 456, dtype=np.float64)[:, None]
        d = np.array([0.0, -0.49, 0.49, -0.5, 0.5, 0.25, -0.25])[None, :]
        with np.errstate(all="ignore"):
            c = ((v + d - bias) / scale).astype(np.float32).reshape(-1)
        c = c[np.isfinite(c)].view(np.uint32).astype(np.int64)
        walk = (c[:, None] + np.arange(-40, 41)[None, :]).reshape(-1)
        pool.append(walk[(walk > 0) & (walk < (1 << 32))].astype(np.uint32))
    else:
        pool.append(np.array([1.0, -1.0, 100.0, -7.5, 0.3, 65504.0], np.float32).view(np.uint32))
    return np.unique(np.concatenate(pool))


def _neighbour(kind, b, step, scale, bias):
    """The nearest bit pattern on one side of the tie element `b` whose t is not the tie's: one ulp away, or, where t is coarser
    than the element (float32 under scale 1: several elements round to the same t), the first one past those."""
    t = lambda c: TR.conversion_t(TR.elements(kind, np.array([c], TR.KINDS[kind])), scale, bias)[0]
    c = b + step
    while t(c) == t(b):
        c += step
    return c


def _first(mask, order):
    idx = order[mask[order]]
    return int(idx[0]) if idx.size else None


@functools.lru_cache(maxsize=None)
def bank(kind, pname):
    """(names, bits, pixels): one element per class the pair expresses, found by search in `_candidates`, then ordinary
    elements of typed_reference.preimages (where the pair reaches every value; otherwise of the pool) up to a prime size.
    The pixel of every element is typed_reference.quantize's."""
    scale, bias = f32pair(pname)
    dt = TR.KINDS[kind]
    pool = _candidates(kind, scale, bias)
    x = TR.widen(TR.elements(kind, pool))
    with np.errstate(all="ignore"):
        m = x * np.float32(scale)
        t = m + np.float32(bias)
        fl = np.floor(t)
    q = TR.quantize(TR.elements(kind, pool), scale, bias).astype(np.int64)
    fin = np.isfinite(x) & (x != 0)
    with np.errstate(all="ignore"):
        tie = fin & np.isfinite(t) & (t - fl == np.float32(0.5)) & (t > 1) & (t < 254)
        fl = np.where(np.isfinite(fl), fl, 0)
        ri = np.clip(np.rint(np.where(np.isfinite(t), t, 0)).astype(np.float64), -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64)
    # nearest a middle pixel value first: deterministic, and away from the clamps
    order = np.argsort(np.abs(q - 100) * (1 << 33) + pool.astype(np.int64), kind="stable")
    mant = pool & dt(~(EXP_MASK[kind] | SIGN[kind]) & (0xFFFF if kind != F32 else 0xFFFFFFFF))
    is_den = ((pool & dt(EXP_MASK[kind])) == 0) & (mant != 0)
    names, bits = [], []

    def add(name, i):
        if i is not None:
            names.append(name)
            bits.append(int(pool[i]) if not isinstance(i, tuple) else i[0])

    if scale == 0:      # every finite element is the same tie: one class, `finite_tie`, whatever the element
        tie = fin = is_den = np.zeros(pool.size, bool)
        add("finite_tie", ({F16: 0x3C00, BF16: 0x3F80, F32: 0x3F800000}[kind],))      # 1.0
    for name, want_even in (("tie_down", True), ("tie_up", False)):
        i = _first(tie & ((fl % 2 == 0) == want_even), order)
        add(name, i)
        if i is not None:      # the elements one ulp either side of it
            add(name + "_below", (_neighbour(kind, int(pool[i]), -1, scale, bias),))
            add(name + "_above", (_neighbour(kind, int(pool[i]), 1, scale, bias),))
    # three more ties going down, at other pixel values: half_away and half_up move nothing else, and only by one, which a
    # Crossed prediction passes on a quarter of the time -- the sites of few positions need more than one such element
    down = tie & (fl % 2 == 0)
    for k, v in enumerate((30, 170, 230)):
        i = _first(down & ~np.isin(pool, np.array(bits, np.int64)), np.argsort(np.abs(q - v) * (1 << 33) + pool.astype(np.int64), kind="stable"))
        add("tie_down%d" % (k + 2), i)
    add("negative", _first(fin & np.isfinite(t) & (t <= -1.5) & (t >= -200) & (ri & 255 != 0), order))
    add("over", _first(fin & np.isfinite(m) & np.isfinite(t) & (t > 256.5) & (t < 1e6) & (ri & 255 != 255), order))
    for name in ("pinf", "ninf", "qnan", "snan", "negnan", "pzero", "nzero"):
        add(name, (SPECIALS[kind][name],))
    add("denormal", _first(is_den & (np.abs(m) >= 0.5) & (q >= 1), np.argsort(np.abs(q - 2) * (1 << 33) + pool.astype(np.int64), kind="stable")))
    # four more, at other pixel values where the kind has them (a float32 or bfloat16 denormal times 2^127 stays below 2): a
    # flushed denormal moves its pixel by two at the most, and an element's neighbours in a rotation frame are always the same
    # elements, so whether a Crossed prediction passes that on is decided once per element, not once per position
    for k, v in enumerate((200, 60, 1, 130)):
        i = _first(is_den & (np.abs(m) >= 0.5) & (q >= 1) & ~np.isin(pool, np.array(bits, np.int64)),
                   np.argsort(np.abs(q - v) * (1 << 33) + np.abs(pool.astype(np.int64) - (0x555 if kind == F16 else 0x55 if kind == BF16 else 0x555555)), kind="stable"))
        add("denormal%d" % (k + 2), i)
    add("overflow_pos", _first(np.isfinite(x) & (m == np.inf), order))
    add("overflow_neg", _first(np.isfinite(x) & (m == -np.inf), order))
    if exemption("fma", kind, pname) is None:
        inr = fin & (t > 0.6) & (t < 254.4)
        sub = np.flatnonzero(inr)
        diff = np.zeros(pool.size, bool)
        diff[sub] = (convert(kind, pool[sub], scale, bias, "fma") != q[sub]) & ~np.isin(pool[sub], np.array(bits, np.int64))
        hits = order[diff[order]][:6]
        for k, i in enumerate(hits):
            add("fma" if k == 0 else "fma%d" % (k + 1), int(i))
    # ordinary in-range elements
    want = (3, 64, 129, 200, 254, 17, 90, 171, 230, 45, 111, 150, 188, 212, 75, 30)
    if scale == 0:      # finite elements of every size and sign; 0x7C00 is finite as bfloat16 and an infinity as float16
        vals = np.array([-1.0, 100.0, -7.5, 0.3, 65504.0, 2.0 ** -20], np.float32)
        ordinary = ([0x7C00] if kind == BF16 else []) + [int(b) for b in {F16: vals.astype(np.float16).view(np.uint16), BF16: TR.bf16_bits(vals), F32: vals.view(np.uint32)}[kind]]
    else:
        try:
            pre = TR.preimages(kind, scale, bias)
            ordinary = [int(pre[v, 2]) for v in want]
        except ValueError:      # the pair does not reach every value: the nearest values the pool reaches
            ok = np.isfinite(x) & np.isfinite(t) & ~((t - fl) == np.float32(0.5)) & (t > 0.6) & (t < 254.4)
            reach = np.unique(q[ok])
            ordinary = [int(pool[_first(ok & (q == int(reach[np.argmin(np.abs(reach - v))])), order)]) for v in want if reach.size]
    n = len(names) + 6
    while any(n % p == 0 for p in range(2, n)):
        n += 1
    k = 0
    while len(names) < n:
        names.append("ordinary%d" % k)
        bits.append(ordinary[k % len(ordinary)] if ordinary else SPECIALS[kind]["pzero"])
        k += 1
    bits = np.array(bits, dt)
    pixels = TR.quantize(TR.elements(kind, bits), scale, bias)
    bits.setflags(write=False)
    pixels.setflags(write=False)
    return tuple(names), bits, pixels


def kills(kind, pname, mutant):
    """The indices of the bank's elements whose pixel the mutant changes."""
    names, bits, pixels = bank(kind, pname)
    return np.flatnonzero(convert(kind, bits, *f32pair(pname), mutant) != pixels)


# ------------------------------------------------------------------------------------------------ the rotation
SHAPE = (293, 191)      # (w, h): two interior tile columns and rows, a ragged column 37 wide, a ragged row 63 high
ROT = (5, 3)


def rotation_index(w, h, n, rot=ROT):
    """(h, w): the bank index of position (x, y) in frame 0; frame f holds (index + f) mod n.  a, b coprime to n."""
    a, b = rot
    assert np.gcd(a, n) == 1 and np.gcd(b, n) == 1
    y, x = np.arange(h, dtype=np.int64)[:, None], np.arange(w, dtype=np.int64)[None, :]
    return (a * x + b * y) % n


def rotation(kind, pname, shape=SHAPE, rot=ROT):
    """(n, h, w) element bit patterns and their (n, h, w) reference pixels."""
    _, bits, pixels = bank(kind, pname)
    n = bits.size
    idx = (rotation_index(shape[0], shape[1], n, rot)[None] + np.arange(n)[:, None, None]) % n
    return bits[idx], pixels[idx]


# --------------------------------------------------------------------------------------------------- the sites
HALO = (0, 4, 8, 16, 32, 64)      # hoff(): the offsets of the halo rows below and the halo columns right of a tile
CONE_NX, CONE_NY = (10, 6, 4, 3, 3), (6, 4, 3, 3, 3)      # cone_n(128, t), cone_n(64, t): points per dimension of level t


def split_levels(levels):
    """(k, up): up to five levels the tile holds the pyramid; six to eight are four levels under a cone of levels - 4."""
    assert 1 <= levels <= 8
    return (levels, 0) if levels < 6 else (4, levels - 4)


@functools.lru_cache(maxsize=None)
def sites(w, h, levels):
    """{(tx, ty): (ragged, {site: (ys, xs)})}: the positions inside the image every 128 x 64 tile reads through each site
    class, from the shape alone.  Sites: ("even", lane) / ("odd", lane) the tile's own rows by byte lane x mod 16 (px_pack4 of
    the row-group batches); ("hrow", lane) the chunks of the halo rows TH + {0, 4, 8, 16, 32}[:nh] (px_pack4 behind the first
    batch); ("hcol", off) the single elements right of the tile (px1), on the tile's even rows and its halo rows, +16 / +32 /
    +64 on the rows that are multiples of it from four / five / six levels in the tile; ("cone",) the points of the
    stride-16 plane above the tile that lie outside its own 10 x 6 frame, levels 1 ... up (px1 in cone_convert_typed)."""
    k, up = split_levels(levels)
    nh = k if k >= 2 else 1
    out = {}
    sw, sh = ((w - 1) >> 4) + 1, ((h - 1) >> 4) + 1
    for ty in range(-(-h // TH)):
        for tx in range(-(-w // TW)):
            X0, Y0 = tx * TW, ty * TH
            s = {}

            def put(key, pts):
                pts = [(y, x) for y, x in pts if y < h and x < w]
                if pts:
                    a = np.array(sorted(set(pts)), np.int64)
                    s[key] = (a[:, 0], a[:, 1])

            for lane in range(16):
                cols = range(X0 + lane, X0 + TW, 16)
                put(("even", lane), [(Y0 + y, x) for y in range(0, TH, 2) for x in cols])
                put(("odd", lane), [(Y0 + y, x) for y in range(1, TH, 2) for x in cols])
                put(("hrow", lane), [(Y0 + TH + HALO[r], x) for r in range(nh) for x in cols])
            hys = list(range(0, TH, 2)) + [TH + HALO[r] for r in range(nh)]
            for off in HALO:
                need = {0: 1, 4: 1, 8: 1, 16: 4, 32: 5, 64: 6}[off]
                if k >= need:
                    put(("hcol", off), [(Y0 + hy, X0 + TW + off) for hy in hys if off < 16 or hy % off == 0])
            A, B = X0 >> 4, Y0 >> 4
            pts = []
            for t in range(1, up + 1):
                mk = (1 << t) - 1
                for iy in range(CONE_NY[t]):
                    for ix in range(CONE_NX[t]):
                        x, y = (A & ~mk) + (ix << t), (B & ~mk) + (iy << t)
                        framed = A <= x < A + CONE_NX[0] and B <= y < B + CONE_NY[0]
                        if x < sw and y < sh and not framed:
                            pts.append((y << 4, x << 4))
            put(("cone",), pts)
            out[tx, ty] = (not (X0 + TW <= w and Y0 + TH <= h), s)
    return out


def site_classes(levels):
    """Every site class a tile can have at `levels`, in a fixed order."""
    k, up = split_levels(levels)
    nh = k if k >= 2 else 1
    keys = [(f, lane) for f in ("even", "odd", "hrow") for lane in range(16)]
    keys += [("hcol", off) for off, need in ((0, 1), (4, 1), (8, 1), (16, 4), (32, 5), (64, 6)) if k >= need]
    return keys + ([("cone",)] if up else [])


# -------------------------------------------------------------------------------------------------- the census
def tables():
    """identity for the IDENT instantiations; identity_but_255 and random0 of tests/operand_designs.py for the others.
    Under a lossless table the reconstruction IS the image, so what a tile reads only to reconstruct its halo (the halo rows
    and columns beyond +0, the cone) cannot reach its grid: those sites are live only under a lossy table, and random0, where
    any change of a prediction changes the reconstruction, is the one the census of those sites runs under."""
    t = D.tables()
    return {name: t[name] for name in ("identity", "identity_but_255", "random0")}


def census(ref, index, n, mutant_pixels, killed_elems, levels, interp, lut, shape=SHAPE, want=None, frames=None):
    """{(site, ragged): tile} for the killed (site, tile class) pairs.  `ref`: (n, h, w) reference pixels; `index`:
    rotation_index; `mutant_pixels`: the bank's pixels under the mutant; `killed_elems`: the bank indices it changes.
    For every tile T and site S the view of frame f is ref[f] with the positions of S holding what the mutant makes of them;
    only frames whose view differs from ref[f] are encoded, and a pair is left at its first kill.  One tile per view: a
    neighbour's positions can lie in T's halo, so views of several tiles would interact.  What is encoded is the window
    of the view that holds everything T reads (`window`): the grid of T is a function of those positions alone, and up to five
    levels the window is a fraction of the frame.  `want`: the (site, ragged) pairs to decide (default: all); `frames`: the
    frames to try (default: all)."""
    from oracle import hgi_oracle as O
    w, h = shape
    st = sites(w, h, levels)
    grids = {}
    killed = {}
    is_k = np.zeros(n, bool)
    is_k[killed_elems] = True
    order = sorted(st, key=lambda txy: (txy != (1, 1), txy))      # the tile with neighbours on every side first
    for txy in order:
        ragged, s = st[txy]
        X0, Y0 = txy[0] * TW, txy[1] * TH
        wx, wy, x1, y1 = window(w, h, levels, txy)
        for key, (ys, xs) in s.items():
            if (key, ragged) in killed or (want is not None and (key, ragged) not in want):
                continue
            base = index[ys, xs]
            for f in (range(n) if frames is None else frames):
                e = (base + f) % n
                hit = is_k[e]
                if not hit.any():
                    continue
                view = ref[f, wy:y1, wx:x1].copy()
                view[ys[hit] - wy, xs[hit] - wx] = mutant_pixels[e[hit]]
                if (f, txy) not in grids:
                    grids[f, txy] = O.encode(ref[f, wy:y1, wx:x1], levels, lut, interp)[Y0 - wy:Y0 - wy + TH, X0 - wx:X0 - wx + TW]
                g = O.encode(view, levels, lut, interp)
                if (g[Y0 - wy:Y0 - wy + TH, X0 - wx:X0 - wx + TW] != grids[f, txy]).any():
                    killed[key, ragged] = txy
                    break
    return killed


def window(w, h, levels, txy):
    """(x0, y0, x1, y1): the part of the frame a tile's grid depends on.  Up to five levels it is the tile and its halo, 32
    columns and rows beyond the tile at the most (`sites`; the tile's origin is a multiple of every step, so the window's
    lattices are the frame's); under the cone it is the whole frame."""
    if levels > 5:
        return 0, 0, w, h
    X0, Y0 = txy[0] * TW, txy[1] * TH
    return X0, Y0, min(w, X0 + TW + 33), min(h, Y0 + TH + 33)


def available(levels, shape=SHAPE):
    """{(site, ragged)}: the pairs some tile of the shape has."""
    out = set()
    for ragged, s in sites(shape[0], shape[1], levels).values():
        out |= {(key, ragged) for key in s}
    return out


# ------------------------------------------------------------------------------------ the GPU module's table
def instantiations():
    """(INTERP, IDENT, SEEDED, E) -> (kinds, levels, tables): what tests/test_element_coverage_gpu.py iterates over.  Every
    kind runs every pair of KIND_PAIRS.  SEEDED 0 runs five levels (the deepest pyramid a tile holds: the +32 singles),
    SEEDED 2 eight (up = 4) and six (2-byte kinds, up = 2) or seven (float32, up = 3)."""
    out = {}
    for interp in (LEFTTOP, CROSSED):
        for ident in (False, True):
            for seeded in (0, 2):
                for E in (2, 4):
                    kinds = (F16, BF16) if E == 2 else (F32,)
                    levels = (5,) if seeded == 0 else (8, 6 if E == 2 else 7)
                    out[interp, ident, seeded, E] = (kinds, levels, ("identity",) if ident else ("identity_but_255", "random0"))
    return out
