"""Entropy-coverage designs (a helper module of tests/test_entropy_coverage*.py, not a conftest).

Where tests/operand_designs.py enumerates the VALUES the per-pixel code meets and tests/geometry_designs.py the SHAPES, this module
enumerates the TOKENS the device entropy stage (rustyhgi_amd/csrc/hgi_entropy.hip, hgi_entropy_host.hip) meets: every code
length, every piece length at every byte of a lane, every candidate threshold, every tail, the fullest chunk the LDS stream image
is sized for.  Everything here is defined from the frames and from a restatement of the stage's rule, never from the library's
device path:

1. `restate`: the rule of tests/test_entropy.py:stage_stream again, vectorised in numpy (stage_stream's per-bit packer takes
   seconds for 60 KB; the designs reach 8 MiB) -- tokens per 1 KiB chunk, pieces of 258, thresholds 3 / 4 / 6 / 10 with the
   smallest payload winning and the first winning a tie, eight literals of the u64 length in front and of the u64 width behind,
   least significant bit first.  Code lengths and the block header come from hgi_huffman_plan: host code, fuzzed separately
   (tests/cpp/fuzz_huffman.cpp); the device does not choose them.  `restate` also returns the CENSUS of the frame: chosen
   threshold, code length of every used symbol, the set of (piece length, start mod 16, match or literals), the bits and the
   start phase of every chunk.
2. `MUTANTS`: the same rule with one thing wrong (tests/test_entropy_coverage.py shows each is told apart by a design).
3. the designs: named frames, built from seeds and from the rule alone.
4. the cases the suite compared byte for byte before these designs existed (tests/test_parity_gpu.py), restated, for the
   "reached today" census of profiles/r17_entropy_coverage.md.
"""
import ctypes
import functools
import struct

import numpy as np

NSYM, CHUNK, PIECE = 286, 1024, 258
THRESHOLDS = (3, 4, 6, 10)                    # kMatchThresholdHost (rustyhgi_amd/csrc/hgi_huffman_host.h)
LBASE = np.array([3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258])
LBITS = np.array([0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0])
# length 0 .. 258 -> index of its length symbol (RFC 1951 3.2.5); lengths below 3 have none
_LSYM = np.searchsorted(LBASE, np.arange(259), side="right") - 1
SEED = 0x48474937

# what a mutant changes: (piece limit, thresholds, chunk cut, tie rule, 15-bit code, order of extra bits, chunk's first byte)
RULE = dict(piece=PIECE, thresholds=THRESHOLDS, cut=True, last_wins=False, drop15=False, extra_first=False, first_continues=False)
MUTANTS = {
    "piece_257": dict(piece=257),
    "thr3_is_4": dict(thresholds=(4, 4, 6, 10)),
    "thr4_is_3": dict(thresholds=(3, 3, 6, 10)),
    "thr4_is_5": dict(thresholds=(3, 5, 6, 10)),
    "thr6_is_5": dict(thresholds=(3, 4, 5, 10)),
    "thr6_is_7": dict(thresholds=(3, 4, 7, 10)),
    "thr10_is_9": dict(thresholds=(3, 4, 6, 9)),
    "thr10_is_11": dict(thresholds=(3, 4, 6, 11)),
    "run_crosses_chunk_end": dict(cut=False),
    "last_wins_tie": dict(last_wins=True),
    "top_bit_of_15_dropped": dict(drop15=True),
    "extra_bits_first": dict(extra_first=True),
    "first_byte_continues": dict(first_continues=True),
}


def plan(hist):
    """hgi_huffman_plan (include/hgi.h): code lengths, reversed canonical codes, block header and its length in bits."""
    from rustyhgi_amd import _ffi
    hist = np.ascontiguousarray(hist, np.uint64)
    lens, codes, header = np.zeros(NSYM, np.uint8), np.zeros(NSYM, np.uint16), np.zeros(640, np.uint8)
    bits = ctypes.c_size_t(0)
    _ffi.check(_ffi.lib().hgi_huffman_plan(hist.ctypes.data, lens.ctypes.data, codes.ctypes.data, header.ctypes.data, header.size,
                                           ctypes.byref(bits)))
    return lens.astype(np.int64), codes.astype(np.int64), header, bits.value


def pieces(data, rule=RULE):
    """The pieces of a frame's runs, from the bytes alone: (start, length, is the run's first) of every piece, in order.  A
    byte that equals its predecessor inside its chunk continues a run; the continuing bytes of a run are cut into pieces of 258
    from the run's second byte on."""
    d = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else data.reshape(-1)
    n = d.size
    if n == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, bool)
    idx = np.arange(n, dtype=np.int64)
    first = (idx % CHUNK) == 0
    cont = np.zeros(n, bool)
    cont[1:] = d[1:] == d[:-1]
    if rule["cut"] and not rule["first_continues"]:
        cont &= ~first
    # where the piece count of a continuing byte starts: behind its head, or (mutant: the chunk's first byte continues) at the chunk
    restart = cont & first & rule["cut"]
    origin = np.where(~cont, idx + 1, np.where(restart, idx, 0))
    origin = np.maximum.accumulate(origin)
    # the first position behind a continuing byte that does not continue its piece count
    stop = np.where(~cont | restart, idx, n)
    stop = np.minimum.accumulate(stop[::-1])[::-1]
    stop = np.append(stop[1:], n)                    # for byte i: the first stop behind it
    o = idx - origin
    start = cont & (o % rule["piece"] == 0)
    at = idx[start]
    length = np.minimum(stop[at] - at, rule["piece"])
    return at, length, o[at] == 0


def token_stream(data, min_match, rule=RULE):
    """(position, symbol, extra bits, extra value) of every token of the frame's bytes, in order -- literals and matches."""
    d = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else data.reshape(-1)
    at, length, _ = pieces(d, rule)
    is_match = length >= min_match
    m_at, m_len = at[is_match], length[is_match]
    # bytes covered by a match emit nothing: +1 at the piece's start, -1 behind its end
    cover = np.zeros(d.size + 1, np.int32)
    np.add.at(cover, m_at, 1)
    np.add.at(cover, m_at + m_len, -1)
    lit = np.cumsum(cover[:-1]) == 0
    pos = np.concatenate([np.flatnonzero(lit), m_at])
    ls = _LSYM[m_len]
    sym = np.concatenate([d[lit].astype(np.int64), 257 + ls])
    ebits = np.concatenate([np.zeros(int(lit.sum()), np.int64), LBITS[ls]])
    extra = np.concatenate([np.zeros(int(lit.sum()), np.int64), m_len - LBASE[ls]])
    order = np.argsort(pos, kind="stable")
    return pos[order], sym[order], ebits[order], extra[order]


def pack_bits(values, nbits, start_bits, head):
    """Tokens of nbits[i] <= 21 bits, least significant bit first, behind `start_bits` bits of `head` (bytes)."""
    off = start_bits + np.concatenate([[0], np.cumsum(nbits)[:-1]]) if len(nbits) else np.zeros(0, np.int64)
    total = start_bits + int(nbits.sum())
    nbytes = (total + 7) // 8
    out = np.zeros(nbytes + 4, np.float64)
    out[:len(head)] = head
    v = values.astype(np.int64) << (off & 7)          # < 2^29: four bytes; tokens do not overlap, so adding is OR-ing
    b = off >> 3
    for k in range(4):
        out += np.bincount(b + k, weights=((v >> (8 * k)) & 255).astype(np.float64), minlength=nbytes + 4)[:nbytes + 4]
    assert out.max() <= 255
    return out[:nbytes].astype(np.uint8).tobytes()


def restate(grid_bytes, width, rule=None, census=True):
    """(stream, census) of a grid under the stage's rule (or a mutant of it)."""
    rule = dict(RULE, **(rule or {}))
    d = np.frombuffer(bytes(grid_bytes), np.uint8) if not isinstance(grid_bytes, np.ndarray) else np.ascontiguousarray(grid_bytes).reshape(-1)
    n = d.size
    prefix = np.frombuffer(struct.pack("<Q", n), np.uint8).astype(np.int64)
    suffix = np.frombuffer(struct.pack("<Q", width), np.uint8).astype(np.int64)
    best, payloads = None, []
    for mm in rule["thresholds"]:
        pos, sym, ebits, extra = token_stream(d, mm, rule)
        hist = np.bincount(np.concatenate([sym, prefix, suffix, [256]]), minlength=NSYM)
        lens, codes, header, hbits = plan(hist)
        payload = int((hist * lens).sum() + ebits.sum() + (sym > 256).sum())
        payloads.append(payload)
        if best is None or payload < best[0] or (rule["last_wins"] and payload == best[0]):
            best = (payload, mm, pos, sym, ebits, extra, hist, lens, codes, header, hbits)
        if n == 0:
            break
    payload, mm, pos, sym, ebits, extra, hist, lens, codes, header, hbits = best
    code = codes.copy()
    if rule["drop15"]:
        code[lens == 15] &= 0x3FFF
    match = sym > 256

    def coded(s, eb, ex, m):
        if rule["extra_first"]:
            return ex | (code[s] << eb), lens[s] + eb + m          # (the distance code is one zero bit)
        return code[s] | (ex << lens[s]), lens[s] + eb + m

    zeros8 = np.zeros(8, np.int64)
    pv, pn = coded(prefix, zeros8, zeros8, zeros8)
    tv, tn = coded(sym, ebits, extra, match.astype(np.int64))
    sv, sn = coded(np.append(suffix, 256), np.zeros(9, np.int64), np.zeros(9, np.int64), np.zeros(9, np.int64))
    stream = pack_bits(np.concatenate([pv, tv, sv]), np.concatenate([pn, tn, sn]), hbits, header[:(hbits + 7) // 8])
    if not census:
        return stream, None
    base_bits = hbits + int(pn.sum())
    nchunks = (n + CHUNK - 1) // CHUNK
    chunk_bits = np.bincount(pos // CHUNK, weights=tn.astype(np.float64), minlength=nchunks).astype(np.int64)
    chunk_off = np.concatenate([[0], np.cumsum(chunk_bits)[:-1]]) if nchunks else np.zeros(0, np.int64)
    p_at, p_len, p_first = pieces(d, rule)
    used = np.flatnonzero(hist)
    c = dict(threshold=mm, payloads=payloads, n=n, width=width, base_bits=base_bits, stream_bits=hbits + payload,
             lit_lens={int(s): int(lens[s]) for s in used if s < 256},
             len_lens={int(s): int(lens[s]) for s in used if s > 256},
             eob_len=int(lens[256]),
             pieces=set(zip(p_len.tolist(), (p_at % 16).tolist(), (p_len >= mm).tolist())),
             first_pieces=set(zip(p_len[p_first].tolist(), (p_at[p_first] % 16).tolist(), (p_len[p_first] >= mm).tolist())),
             match_lengths=set(p_len[p_len >= mm].tolist()),
             chunk_bits=chunk_bits, chunk_phase=(base_bits + chunk_off) % 32,
             end_phase=int((base_bits + chunk_bits.sum()) % 32),
             max_token_bits=int(tn.max()) if len(tn) else 0)
    return stream, c


def word_census(c):
    """(most chunk starts in one 32-bit word of the stream, most whole chunks inside one word) of a census"""
    start = c["base_bits"] + np.concatenate([[0], np.cumsum(c["chunk_bits"])])
    a, b = start[:-1], start[1:]
    whole = (a // 32)[(a // 32) == ((b - 1) // 32)]
    return int(np.bincount(a // 32).max()), int(np.bincount(whole).max()) if whole.size else 0


def image(grid_bytes, width):
    """The bincode image of Grid { buffer, width }: what every stream must inflate to."""
    b = bytes(grid_bytes) if not isinstance(grid_bytes, np.ndarray) else grid_bytes.tobytes()
    return struct.pack("<Q", len(b)) + b + struct.pack("<Q", width)


# ------------------------------------------------------------------- the cases compared byte for byte before these designs
def _run_structured(rng, n, max_run, nvalues):
    """tests/test_parity_gpu.py:_run_structured"""
    out = np.empty(n + max_run, np.uint8)
    at = 0
    while at < n:
        r = int(rng.integers(1, max_run + 1))
        out[at:at + r] = min(int(rng.geometric(0.35)) - 1, nvalues - 1)
        at += r
    return out[:n]


NAMED = ("lena", "runs12", "runs40", "runs700", "zeros", "ones", "noise", "ragged", "one_byte", "fifteen", "kib_plus_one", "two_values")


def named_case(case, lena_grid=None):
    """The grids of test_device_entropy_stream_equals_the_restated_one (the same seeds).  lena_grid: the oracle's encode of
    LENA's 160 x 96 corner, three levels, Medium -- the one case that needs the oracle."""
    from conftest import SEED0
    rng = np.random.default_rng(SEED0 + 77)
    if case == "lena":
        grid = lena_grid
    elif case.startswith("runs"):
        m = int(case[4:])
        grid = _run_structured(rng, 200 * 123, m, 5 if m < 100 else 3).reshape(123, 200)
    elif case == "zeros":
        grid = np.zeros((70, 300), np.uint8)
    elif case == "ones":
        grid = np.full((37, 259), 1, np.uint8)
    elif case == "noise":
        grid = rng.integers(0, 256, (64, 200), dtype=np.uint8)
    elif case == "ragged":
        grid = _run_structured(rng, 61 * 107, 9, 4).reshape(61, 107)
    elif case == "one_byte":
        grid = np.full((1, 1), 7, np.uint8)
    elif case == "fifteen":
        grid = np.zeros((3, 5), np.uint8)
    elif case == "kib_plus_one":
        grid = np.zeros((1, 1025), np.uint8)
    else:
        grid = (rng.integers(0, 8, (90, 90)) == 0).astype(np.uint8) * 255
    return np.ascontiguousarray(grid)


def random_cases():
    """The thirty grids of test_device_entropy_random_shapes_byte_exact (the same seed, drawn in the same order)."""
    from conftest import SEED0
    rng = np.random.default_rng(SEED0 + 101)
    out = []
    for case in range(30):
        w, h = int(rng.integers(1, 400)), int(rng.integers(1, 150))
        if case == 0:
            w, h = 1024, 3
        kind = case % 5
        if kind == 0:
            grid = (rng.geometric(0.6, (h, w)) - 1).astype(np.uint8)
        elif kind == 1:
            grid = _run_structured(rng, w * h, int(rng.integers(2, 30)), 6).reshape(h, w)
        elif kind == 2:
            grid = rng.integers(0, 256, (h, w), dtype=np.uint8)
        elif kind == 3:
            grid = _run_structured(rng, w * h, 600, 2).reshape(h, w)
        else:
            grid = np.where(rng.random((h, w)) < 0.03, rng.integers(1, 256, (h, w)), 0).astype(np.uint8)
        out.append(np.ascontiguousarray(grid))
    return out


# ------------------------------------------------------------------------------------------------------------- designs
# The common frame of the batches: 512 x 522 = 261 chunks of 1 KiB (why this size: dense15 below).
BW, BH = 512, 522
BN = BW * BH


def _spread(values, k):
    """A fixed permutation of a sorted array (i -> i * k mod m, k coprime to m): equal values end up apart.  No generator is
    involved, so the frame -- and with it the code the planner builds -- does not depend on the numpy version."""
    m = values.size
    assert np.gcd(k, m) == 1
    return values[(np.arange(m, dtype=np.int64) * k) % m]


def soup(counts, k=7919):
    """Bytes with exactly `counts[v]` of every value v and no piece of 3 or more: the non-zero bytes, spread, each preceded by
    one zero (some by two, or by none, as the count of zeros asks), so under every threshold every byte is a literal."""
    others = np.concatenate([np.full(int(c), v, np.uint8) for v, c in sorted(counts.items()) if v and c] or [np.zeros(0, np.uint8)])
    z, m = int(counts.get(0, 0)), others.size
    assert 0 <= z <= 2 * m, (z, m)
    while np.gcd(k, m) != 1:
        k += 1
    others = _spread(others, k)
    i = np.arange(m + 1, dtype=np.int64)
    extra = np.diff(i * (z - m) // m)                  # groups with a second zero, evenly spread
    out = np.zeros(z + m, np.uint8)
    out[np.cumsum(2 + extra) - 1] = others
    assert pieces(out)[1].max() < 3
    return out


DENSE_RARE = np.arange(128, 256, dtype=np.uint8)
DENSE_RUNS = tuple(range(195, 211)) + tuple(range(227, 256, 4))      # sixteen of symbol 283, eight of symbol 284 (5 extra bits each)
# literal -> code length the design asks for; total weight 2^18 - 7, every weight 2^(18 - length) but those of the end of
# block (1) -- so the planner's Huffman tree IS these lengths, with nothing for its length limiter to repair
DENSE_LENS = {0: 1, 2: 2, 4: 3, 20: 4, 1: 5, 3: 6, 5: 7, 6: 9, 7: 10, 8: 11, 9: 12, 10: 14, 11: 14}


LONG2 = {6: 512, 7: 256, 8: 128, 9: 64, 5: 64}         # the second long chunk: every literal of 9 ... 12 bits, and 64 of 7 bits
LONG2_BITS = 512 * 9 + 256 * 10 + 128 * 11 + 64 * 12 + 64 * 7          # 9 792: 306 words of the stream image


@functools.lru_cache(maxsize=None)
def _dense_chunks(long_first):
    """dense15, as 261 chunks.  Chunk 0 is the 128 rare values eight times over (cyclic: no byte equals its neighbour): with the
    rare values at 15 bits it is 1024 x 15 = 15 360 bits, the bound the LDS stream image of k_token_pack is sized for.  A second
    long chunk (LONG2: 9 792 bits) lies eight chunks behind it -- or, `long_first`, eight chunks in front of it: when a frame gets
    two workgroups one wave codes both, one after the other, and the second meets whatever the first left in the image.  The
    other chunks hold the `chain' values at 1 ... 7 bits, two literals at 14 bits, and 24 runs of zeros whose single pieces take
    the length symbols 283 (14 bits: a 20-bit token) and 284 (15 bits: the 21-bit token).  The frame is 512 x 522 so that the
    token histogram -- the bytes, minus what the matches cover, plus the eight literals of the length, the eight of the width
    and the end of block -- comes out at the weights above."""
    hist = {v: 1 << (18 - l) for v, l in DENSE_LENS.items()}
    for b in struct.pack("<QQ", BN, BW):
        hist[b] -= 1                                   # the literals in front of and behind the grid's own
    hist[0] -= len(DENSE_RUNS)                         # the runs' heads
    hist[2] -= 2 * len(DENSE_RUNS)                     # the bytes that fence a run
    for v, c in LONG2.items():
        hist[v] -= c
    free = soup(hist)
    assert free.size + 2 * CHUNK + sum(L + 3 for L in DENSE_RUNS) == BN
    out = np.zeros(BN, np.uint8)
    taken = np.zeros(BN, bool)
    out[:CHUNK] = np.resize(DENSE_RARE, CHUNK)
    taken[:CHUNK] = True
    at = (253 if long_first else 8) * CHUNK
    out[at:at + CHUNK:2] = 6                           # every other byte; the rest between them, spread: no two neighbours alike
    out[at + 1:at + CHUNK:2] = _spread(np.concatenate([np.full(c, v, np.uint8) for v, c in LONG2.items() if v != 6]), 101)
    taken[at:at + CHUNK] = True
    for j, L in enumerate(DENSE_RUNS):                 # one run per chunk, its head at a different byte of its lane each time
        at = (3 + 10 * j) * CHUNK + 5 + 37 * j % 600
        out[at], out[at + L + 2] = 2, 2                # (the zeros between them: head + L continuing bytes)
        taken[at:at + L + 3] = True
    out[~taken] = free
    return out.reshape(-1, CHUNK)


def dense15(rot=0, long_first=False):
    """dense15 with its chunks rotated: the full chunk is chunk `rot`.  Chunks are coded independently and the histogram does
    not change, so every rotation has the same code and the same chunks in another order -- at other bit offsets, and in the
    hands of other waves."""
    return np.ascontiguousarray(np.roll(_dense_chunks(bool(long_first)), rot, axis=0)).reshape(BH, BW)


def dense_phase(rot, census0):
    """Start phase of the full chunk of a dense15 frame rotated by `rot`, from the census of the unrotated one."""
    bits = np.roll(census0["chunk_bits"], rot)
    return int((census0["base_bits"] + bits[:rot].sum()) % 32)


# the dense15 frames of the suite: a = the second long chunk behind the full one, b = in front of it; the full chunk's index
# (what phases and waves these give is asserted in tests/test_entropy_coverage.py, not assumed)
DENSE = ("dense15_a12", "dense15_a173", "dense15_b200", "dense15_b27", "dense15_a10", "dense15_a199", "dense15_b13", "dense15_b174")


def dense_of(name):
    """name -> (long chunk first, rotation)"""
    return name[8] == "b", int(name[9:])


def lengths_8_13():
    """109 x 75, the literal code lengths dense15 has no room for: weights 2^(13 - length), 4096 ... 64 for 1 ... 7 bits, 32
    for 8 bits and 32 symbols of weight one -- 31 literals and the end of block -- at 13 bits."""
    w, h = 109, 75
    hist = {v: 1 << (13 - l) for v, l in {0: 1, 2: 2, 4: 3, 20: 4, 1: 5, 3: 6, 5: 7, 6: 8}.items()}
    ones = set(struct.pack("<QQ", w * h, w)) - {0}
    ones |= set(range(200, 200 + 31 - len(ones)))
    hist.update({v: 1 for v in ones})
    for b in struct.pack("<QQ", w * h, w):
        hist[b] -= 1
    g = soup(hist, k=101)
    assert g.size == w * h
    return g.reshape(h, w)


# ---- runs: every piece length 1 ... 258 headed at every byte of a lane
RUN_LONG = (259, 260, 261, 262, 263, 264, 265, 266, 267, 268, 270, 300, 516, 517, 518, 519, 520, 774, 775, 776, 777, 778, 1020, 1021, 1022, 1023)


@functools.lru_cache(maxsize=None)
def _runs_frames():
    """Three 512 x 522 frames.  A: noise filler (literals are dear: short pieces pay as matches); B, C: a filler of two values
    and runs of zeros.  Between them: a run of every length 1 ... 258 (continuing bytes) headed at every byte 0 ... 15 of a lane;
    the long runs of RUN_LONG (second, third and fourth pieces, every kind of leftover); runs that end with their chunk and runs
    that a chunk end cuts; the lanes with the most piece starts."""
    rng = np.random.default_rng(SEED + 1)
    frames, n_frames = [], 3
    jobs = [(L, k) for L in range(1, 259) for k in range(16)]
    jobs = [jobs[i] for i in _spread(np.arange(len(jobs)), 1031)]
    per_frame = (len(jobs) + n_frames - 1) // n_frames
    for f in range(n_frames):
        if f == 0:
            fill = rng.integers(1, 256, BN + 1).astype(np.uint8)
            fill[1:][fill[1:] == fill[:-1]] ^= 0x55          # no accidental runs: x ^ 0x55 != x, and a pair is harmless
        else:
            fill = np.where(np.arange(BN + 1) % 2 == 0, 1 + f, 7).astype(np.uint8)
        out = fill[:BN].copy()

        def place(head_at, length, value=0):
            """a run of 1 + length bytes headed at head_at; the bytes around it differ from it"""
            out[head_at:head_at + 1 + length] = value
            return head_at + 1 + length

        # fixed patterns first: whole chunks 0 ... 7
        out[0:CHUNK] = np.resize(np.repeat(np.arange(60, 120, dtype=np.uint8), 2), CHUNK)                  # aabbccdd...
        out[CHUNK:2 * CHUNK] = np.concatenate([[9], np.resize(np.repeat(np.arange(60, 120, dtype=np.uint8), 2), CHUNK - 1)])      # xaabbcc...
        out[2 * CHUNK:3 * CHUNK] = np.resize(np.repeat(np.arange(60, 120, dtype=np.uint8), 4), CHUNK)      # aaaabbbbccccdddd
        out[3 * CHUNK:4 * CHUNK] = np.resize(np.repeat(np.arange(60, 120, dtype=np.uint8), 5), CHUNK)      # pieces of 4 at every phase
        at = 4 * CHUNK
        # a run that ends with its chunk, and one that a chunk end cuts (the next chunk's first byte is then a literal)
        for L in (1, 2, 3, 5, 9, 12, 100, 258, 300)[f::3] + (4 + f,):
            at = (at // CHUNK + 1) * CHUNK
            place(at + CHUNK - 1 - L, L)                     # ends at byte 1023
            at += CHUNK
            place(at + CHUNK - 1 - L, L + 1 + L)             # L continuing bytes, the cut, a literal, L more
            at += 2 * CHUNK
        for L in RUN_LONG[f::3]:
            at = (at // CHUNK + 1) * CHUNK
            head = at + (0 if L >= 1020 else (5 * L + f) % 16)
            place(head, L)
            at = head + L + 2
        for L, k in jobs[f * per_frame:(f + 1) * per_frame]:
            p = at + (k - at) % 16
            if p % CHUNK + L > CHUNK - 2:                    # does not fit in front of the chunk's end: the next chunk
                p = (p // CHUNK + 1) * CHUNK + k
            at = place(p, L) + 1
        assert at <= BN, at
        frames.append(out.reshape(BH, BW))
    return tuple(frames)


# ---- threshold: frames on which each candidate wins, and one on which two tie
def _value_runs(seed, nrun, nvalues, gap, lengths, n=BN):
    """runs of 1 + L bytes, L drawn from `lengths`, of a value drawn from 0 ... nrun - 1, between `gap` bytes drawn from
    nrun ... nrun + nvalues - 1 (no two bytes alike in a row but inside a run)"""
    rng = np.random.default_rng(seed)
    out = np.empty(n + 64, np.uint8)
    at, last = 0, -1
    while at < n:
        for _ in range(gap):
            v = int(rng.integers(0, nvalues))
            if nrun + v == last:
                v = (v + 1) % nvalues
            out[at] = last = nrun + v
            at += 1
        L = int(lengths[int(rng.integers(0, len(lengths)))])
        v = int(rng.integers(0, nrun))
        if v == last:
            v = (v + 1) % nrun
        out[at:at + 1 + L] = last = v
        at += 1 + L
    return out[:n]


_SIX = (1, 2, 3, 4, 5) + (6, 7, 8, 9) * 4 + (10, 11, 12)            # pieces of 6 ... 9 common (short codes), 3 ... 5 in runs of a 1-bit value
_TEN = tuple(range(1, 14)) + tuple(range(14, 80, 3))                # many length symbols, each rare: a match is dear
# threshold -> (run values, filler values, filler bytes between runs, continuing bytes of a run)
THRESHOLD_PARAMS = {3: (16, 8, 1, range(1, 14)), 4: (2, 8, 1, range(1, 14)), 6: (1, 8, 1, _SIX), 10: (1, 8, 1, _TEN)}


def threshold_frame(t):
    nrun, nvalues, gap, lengths = THRESHOLD_PARAMS[t]
    return _value_runs(SEED + 10 + t, nrun, nvalues, gap, list(lengths)).reshape(BH, BW)


def threshold_tie():
    """23 bytes on which thresholds 3 and 4 (and with them 6 and 10) cost the same 106 bits with different tokens -- three
    pieces of 3 as matches or as literals: the first must win."""
    d = []
    for i in range(3):
        d += [i % 2] * 4 + [10 + i]
    return np.array(d + list(range(100, 108)), np.uint8).reshape(1, -1)


# ---- tails: every length of the last chunk
TAIL_N = tuple(range(1, 1041)) + (2047, 2048, 2049, 2050)


def tail_frame(n, kind):
    """1 x n.  kind 0: the last bytes are a run that reaches the end of the data; kind 1: the last byte stands alone."""
    d = _value_runs(SEED + 100 + n, 3, 5, 1, (1, 2, 3, 4, 7, 12, 40), n)
    r = 2 + n % 18
    d[max(0, n - r):] = 77
    if kind == 1:
        d[n - 1] = 78
    return d.reshape(1, n)


# ---- sharing: chunks of 17 bits, several to a 32-bit word of the stream
SHARING_N = {"share_30720": 30720, "share_25601": 25601, "share_33793": 33793, "share_end0": 30727, "share_end31": 30725}


def sharing_frame(name):
    return np.zeros((1, SHARING_N[name]), np.uint8)


# ---- scan: the block edges of k_huff_scan (1024 chunks per block, eight blocks per super-block)
SCAN_SHAPES = {1024: (1024, 1024), 1025: (1025, 1024), 8192: (2048, 4096), 8193: (8193, 1024)}


def scan_frame(nchunks):
    """A period of three chunks: zeros (17 bits), a chunk without runs, a chunk of short runs."""
    w, h = SCAN_SHAPES[nchunks]
    i = np.arange(CHUNK)
    period = np.concatenate([np.zeros(CHUNK, np.uint8), (i * 7 % 13 + 1).astype(np.uint8), (i // 5 % 3).astype(np.uint8)])
    return np.resize(period, w * h).reshape(h, w)


# ---- the registry
BATCH = tuple(list(DENSE[:4]) + ["runs_a", "runs_b", "runs_c"] + ["threshold_%d" % t for t in THRESHOLDS])
SINGLES = tuple(list(DENSE[4:]) + ["zeros", "lengths_8_13", "threshold_tie"] + list(SHARING_N)
                + ["scan_%d" % c for c in SCAN_SHAPES])


def frame(name):
    """name -> (H, W) uint8 array.  BATCH: the eleven 512 x 522 frames; SINGLES: the others (the tails have tail_frame)."""
    if name.startswith("dense15_"):
        return dense15(dense_of(name)[1], dense_of(name)[0])
    if name.startswith("runs_"):
        return _runs_frames()["abc".index(name[5])]
    if name == "threshold_tie":
        return threshold_tie()
    if name.startswith("threshold_"):
        return threshold_frame(int(name[10:]))
    if name == "zeros":
        return np.zeros((BH, BW), np.uint8)
    if name == "lengths_8_13":
        return lengths_8_13()
    if name in SHARING_N:
        return sharing_frame(name)
    if name.startswith("scan_"):
        return scan_frame(int(name[5:]))
    raise KeyError(name)


@functools.lru_cache(maxsize=32)
def restated(name):
    """(stream, census) of a named design, once per process."""
    g = frame(name)
    return restate(g, g.shape[1])


# ---- how the stage deals chunks to waves (rustyhgi_amd/csrc/hgi_entropy.hip: blocks_for and the kernels' chunk walk), restated
def blocks_for(nchunks, frames, resident):
    return max(1, min(resident // frames, (nchunks + 3) // 4))


def wave_walk(nchunks, blocks, block, wave):
    """the chunks one wave of one workgroup codes, in order"""
    return list(range(block * 4 + wave, nchunks, blocks * 4))
