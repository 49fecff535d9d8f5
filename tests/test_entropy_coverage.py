"""What the device entropy stage (rustyhgi_amd/csrc/hgi_entropy.hip: k_token_hist, k_token_count, k_huff_scan, k_token_pack; the
group pipeline of hgi_entropy_host.hip) is fed by the designs of tests/entropy_designs.py, measured on the frames and on a
restatement of the stage's rule alone (CPU; the library's device path is not touched -- only hgi_huffman_plan, the host's code
construction, which the device does not choose).

The byte-exact cases the suite had (a dozen named grids, thirty random ones of at most 60 KB) never held a 15-bit code, never
filled more than 8 205 of the 15 360 bits the LDS stream image of k_token_pack is sized for and never chose threshold 6.  This
file asserts, from the census of each design, that the designs do: the restatement is first shown to equal
tests/test_entropy.py:stage_stream byte for byte on every one of those earlier cases, every design's restated stream is inflated
by zlib, and thirteen mutants of the rule are each told apart by a design.  tests/test_entropy_coverage_gpu.py pushes the same
frames through every entry point.  Figures (run with -s): profiles/r17_entropy_coverage.md."""
import zlib

import numpy as np
import pytest

import entropy_designs as E
from test_entropy import stage_stream


def inflate(stream):
    z = zlib.decompressobj(-15)
    out = z.decompress(stream)
    assert z.eof and not z.unused_data
    return out


@pytest.fixture(scope="module")
def lena_grid(oracle, lena):
    return oracle.encode(lena[:96, :160].copy(), 3, oracle.linear_lut(2)[0])


# ------------------------------------------------------------------------------------- the restatement is the rule
@pytest.mark.parametrize("case", E.NAMED)
def test_restatement_equals_stage_stream_on_the_named_cases(lena_grid, case):
    g = E.named_case(case, lena_grid)
    assert E.restate(g, g.shape[1], census=False)[0] == stage_stream(g.tobytes(), g.shape[1])


@pytest.mark.parametrize("part", range(5))
def test_restatement_equals_stage_stream_on_the_random_shapes(part):
    grids = E.random_cases()
    assert len(grids) == 30
    for g in grids[part::5]:
        assert E.restate(g, g.shape[1], census=False)[0] == stage_stream(g.tobytes(), g.shape[1]), g.shape


def test_restatement_of_an_empty_grid():
    g = np.zeros((0, 5), np.uint8)
    s = E.restate(g, 5)[0]
    assert s == stage_stream(b"", 5) and inflate(s) == E.image(g, 5)


def test_census_of_the_earlier_cases(lena_grid):
    """`Reached today' in profiles/r17_entropy_coverage.md: the census of the byte-exact cases the suite had before the designs."""
    grids = [E.named_case(c, lena_grid) for c in E.NAMED] + E.random_cases()
    cs = [E.restate(g, g.shape[1])[1] for g in grids]
    lit = max(max(c["lit_lens"].values()) for c in cs)
    ln = max(max(c["len_lens"].values(), default=0) for c in cs)
    bits = max(int(c["chunk_bits"].max()) for c in cs)
    thr = sorted({c["threshold"] for c in cs})
    lengths = max(len(c["match_lengths"]) for c in cs)
    tok = max(c["max_token_bits"] for c in cs)
    print("earlier cases: longest literal code %d, longest length code %d, widest token %d, most bits in a chunk %d, thresholds %s, "
          "most distinct match lengths in a case %d" % (lit, ln, tok, bits, thr, lengths))
    assert (lit, ln, tok, bits, thr) == (14, 13, 18, 8205, [3, 4, 10]) and lengths < 254


# ------------------------------------------------------------------------------------------------ every design inflates
@pytest.mark.parametrize("name", E.BATCH + E.SINGLES)
def test_restated_stream_of_a_design_is_ordinary_deflate(name):
    g = E.frame(name)
    stream, c = E.restated(name)
    assert inflate(stream) == E.image(g, g.shape[1])
    assert len(stream) == (c["stream_bits"] + 7) // 8
    # the stream fits the scratch the stage gives a frame (hgi_entropy_host.hip: deflate_geom)
    assert c["stream_bits"] // 8 + 64 <= g.size + g.size // 4 + 4096


def test_the_batch_is_one_size():
    assert len(E.BATCH) == 11 and all(E.frame(n).shape == (E.BH, E.BW) for n in E.BATCH + ("zeros",))
    assert len({E.frame(n).tobytes() for n in E.BATCH}) == 11


# ------------------------------------------------------------------------------------------------------------- dense15
def test_dense15_fills_the_stream_image():
    """A chunk of exactly 1024 x 15 bits, every literal of it 15 bits, starting at bit 0, at bit 31 and at more phases of its
    first word; the 21-bit and the 20-bit match token; for each of a workgroup's four waves, when a frame gets two workgroups, a
    frame in which that wave codes the full chunk, next the second long chunk and then short ones, and a frame in which it codes
    the second long chunk, next the full one and then short ones."""
    phases, order = set(), set()
    c0 = {lf: E.restate(E.dense15(0, lf), E.BW)[1] for lf in (False, True)}
    for name in E.DENSE:
        long_first, rot = E.dense_of(name)
        g = E.frame(name)
        c = E.restated(name)[1]
        long2 = (rot - 8 if long_first else rot + 8)
        assert 0 <= long2 < 261
        assert c["chunk_bits"].size == 261 and int(c["chunk_bits"][rot]) == 15360 and int(c["chunk_bits"][long2]) == E.LONG2_BITS
        assert np.sort(c["chunk_bits"])[-3] < 2100                       # every other chunk is short: 66 words or fewer
        assert set(g.reshape(-1, E.CHUNK)[rot].tolist()) == set(E.DENSE_RARE.tolist())
        assert all(c["lit_lens"][int(v)] == 15 for v in E.DENSE_RARE)
        assert c["chunk_phase"][rot] == E.dense_phase(rot, c0[long_first])
        phases.add(int(c["chunk_phase"][rot]))
        # the widest match token: 15-bit code + 5 extra bits + the distance bit, and the 20-bit one
        assert c["len_lens"] == {283: 14, 284: 15} and c["max_token_bits"] == 21
        assert {L for L, _, m in c["pieces"] if m} == set(E.DENSE_RUNS)
        assert {k: v for k, v in c["lit_lens"].items() if k in E.DENSE_LENS} == E.DENSE_LENS
        assert c["eob_len"] == 15 and len(set(c["payloads"])) == 1 and c["threshold"] == 3
        # two workgroups per frame: wave w of workgroup b walks b * 4 + w, + 8, + 16, ...
        walk = E.wave_walk(261, 2, rot % 8 // 4, rot % 4)
        first, second = (long2, rot) if long_first else (rot, long2)
        assert walk[walk.index(first) + 1] == second and len(walk) - walk.index(second) > 5
        order.add((rot % 4, long_first))
    print("dense15: phases of the full chunk %s, stream %d bytes" % (sorted(phases), len(E.restated(E.DENSE[0])[0])))
    assert {0, 31} <= phases and len(phases) >= 4
    assert order == {(w, lf) for w in range(4) for lf in (False, True)}
    assert {0, 31} <= {int(E.restated(n)[1]["chunk_phase"][E.dense_of(n)[1]]) for n in E.BATCH[:4]}
    # sh0 + chunk_total at its bound: the last word of the image that holds a bit
    assert (31 + 15360 + 31) // 32 == 481 <= (1024 * 15 + 31) // 32 + 4 and (E.LONG2_BITS + 31) // 32 == 306 > 257


def test_every_code_length_occurs_on_a_literal():
    lens = set(E.restated(E.DENSE[0])[1]["lit_lens"].values()) | set(E.restated("lengths_8_13")[1]["lit_lens"].values())
    assert lens == set(range(1, 16))
    c = E.restated("lengths_8_13")[1]
    assert sorted(c["lit_lens"].values()).count(13) == 31 and c["eob_len"] == 13 and c["lit_lens"][6] == 8


# ---------------------------------------------------------------------------------------------------------------- runs
def test_runs_reach_every_piece_at_every_lane_byte():
    names = ("runs_a", "runs_b", "runs_c")
    first, every, lengths = set(), set(), set()
    for n in names:
        c = E.restated(n)[1]
        first |= c["first_pieces"]
        every |= c["pieces"]
        lengths |= c["match_lengths"]
    # every first piece 1 ... 258 with the run's head at every byte of a lane (the piece starts one byte on)
    have = {(L, (s - 1) % 16) for L, s, _ in first}
    assert have >= {(L, k) for L in range(1, 259) for k in range(16)}
    assert {L for L, s, _ in first if s == 0} == set(range(1, 259))          # headed by a lane's last byte: starts at byte 0 of the next
    assert lengths == set(range(3, 259))
    print("runs: %d classes (length, start mod 16, match) of first pieces, %d of all pieces" % (len(first), len(every)))
    # second, third and fourth pieces, and every kind of leftover behind a piece of 258
    left, depth = set(), set()
    ends_with_chunk = cut_by_chunk = 0
    eight = {0: 0, 1: 0}
    four_matches = 0
    for n in names:
        d = E.frame(n).reshape(-1)
        thr = E.restated(n)[1]["threshold"]
        at, ln, is_first = E.pieces(d)
        nth = np.zeros(at.size, np.int64)
        for i in range(1, at.size):
            if not is_first[i]:
                assert at[i] == at[i - 1] + 258 and ln[i - 1] == 258
                nth[i] = nth[i - 1] + 1
                left.add(int(ln[i]))
        depth |= set(nth.tolist())
        end = at + ln
        at_chunk_end = end[(end % E.CHUNK == 0) & (end < d.size)]
        cut_by_chunk += int((d[at_chunk_end] == d[at_chunk_end - 1]).sum())
        ends_with_chunk += int((d[at_chunk_end] != d[at_chunk_end - 1]).sum())
        per_lane = np.bincount(at // 16, minlength=d.size // 16)
        for lane in np.flatnonzero(per_lane == 8):
            eight[int(at[at // 16 == lane][0] % 2)] += 1
        per_lane_m = np.bincount(at[ln >= thr] // 16, minlength=d.size // 16)
        four_matches += int((per_lane_m >= 4).sum())
    # continuing bytes 259 ... 262, 516 ... 520, 774 ... 778, 1020 ... 1023 of one run
    totals = set()
    for n in names:
        d = E.frame(n).reshape(-1)
        at, ln, is_first = E.pieces(d)
        run = np.cumsum(is_first) - 1
        totals |= set(np.bincount(run, weights=ln).astype(np.int64).tolist())
    assert totals >= set(E.RUN_LONG) and {259, 260, 261, 262, 516, 520, 774, 778, 1020, 1023} <= totals
    assert depth == {0, 1, 2, 3}
    assert left >= {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 42, 246, 247, 248, 249, 258}
    assert ends_with_chunk >= 9 and cut_by_chunk >= 9
    assert eight[0] >= 60 and eight[1] >= 60 and four_matches >= 60
    print("runs: leftovers %s; runs ending with their chunk %d, cut by it %d; lanes of eight starts %s, of four matches %d"
          % (sorted(left), ends_with_chunk, cut_by_chunk, eight, four_matches))


# ----------------------------------------------------------------------------------------------------------- threshold
def test_each_threshold_is_chosen_and_a_tie_goes_to_the_first():
    for i, t in enumerate(E.THRESHOLDS):
        c = E.restated("threshold_%d" % t)[1]
        p = c["payloads"]
        assert c["threshold"] == t and all(p[i] < q for j, q in enumerate(p) if j != i), (t, p)
        # pieces on both sides of the threshold, as matches and as literals
        assert {(L, L >= t) for L in range(1, 13)} <= {(L, m) for L, _, m in c["pieces"]}
        print("threshold_%d: payloads %s" % (t, p))
    g = E.threshold_tie()
    s, c = E.restated("threshold_tie")
    assert c["payloads"][0] == c["payloads"][1] == min(c["payloads"]) and c["threshold"] == 3
    assert E.restate(g, g.shape[1], dict(thresholds=(4, 4, 6, 10)))[0] != s       # the same payload, other tokens
    assert any(m for _, _, m in c["pieces"])


# --------------------------------------------------------------------------------------------------------------- tails
def test_tails_end_inside_every_lane():
    assert set(E.TAIL_N) == set(range(1, 1041)) | {2047, 2048, 2049, 2050}
    cnt = set()
    for n in E.TAIL_N:
        for kind in (0, 1):
            g = E.tail_frame(n, kind)
            assert g.shape == (1, n)
            s, c = E.restate(g, n)
            assert inflate(s) == E.image(g, n)
            at, ln, _ = E.pieces(g)
            reaches_end = bool(at.size) and int(at[-1] + ln[-1]) == n
            assert reaches_end == (kind == 0 and n > 1 and n % E.CHUNK != 1), (n, kind)
        cnt.add((n % E.CHUNK) % 16)
    assert cnt == set(range(16))


# ------------------------------------------------------------------------------------------------------------- sharing
def test_sharing_frames_put_several_chunks_in_a_word():
    """A chunk of 1024 zeros is five tokens of 17 bits under the best code, so a 32-bit word of the stream takes the end of one
    chunk, a whole chunk and the start of a third -- and, where the last chunk is one byte, two whole chunks and the tail.  (Five
    tokens a chunk is the least there is: 1023 continuing bytes are three pieces of 258 and one of 249.)"""
    c = E.restated("share_30720")[1]
    assert set(c["chunk_bits"].tolist()) == {17}
    assert E.word_census(c) == (2, 1)
    for name, end in (("share_25601", 0), ("share_33793", 31)):
        c = E.restated(name)[1]
        assert int(c["chunk_bits"][-1]) == 2 and E.word_census(c) == (2, 2) and c["end_phase"] == end
    assert E.restated("share_end0")[1]["end_phase"] == 0 and E.restated("share_end31")[1]["end_phase"] == 31
    assert E.word_census(E.restated("zeros")[1])[0] == 2


# ---------------------------------------------------------------------------------------------------------------- scan
def test_scan_frames_stand_on_the_block_edges():
    for nchunks, (w, h) in E.SCAN_SHAPES.items():
        assert (w * h + E.CHUNK - 1) // E.CHUNK == nchunks
        c = E.restated("scan_%d" % nchunks)[1]
        assert c["chunk_bits"].size == nchunks and len(set(c["chunk_bits"][:3].tolist())) == 3
    assert set(E.SCAN_SHAPES) == {1024, 1025, 8 * 1024, 8 * 1024 + 1}


# ------------------------------------------------------------------------------------------------------------- mutants
MUTANT_FRAMES = (E.DENSE[0], "runs_a", "runs_b", "runs_c", "threshold_3", "threshold_4", "threshold_6", "threshold_10", "threshold_tie",
                 "lengths_8_13", "zeros", "share_30720", "share_25601", "share_33793", "share_end0", "share_end31", "scan_1025")
MUTANT_TAILS = tuple(range(1, 41)) + tuple(range(255, 266)) + tuple(range(1020, 1041)) + (2047, 2048, 2049, 2050)


@pytest.mark.parametrize("mutant", list(E.MUTANTS))
def test_a_mutant_of_the_rule_is_told_apart(lena_grid, mutant):
    """The restated rule with one thing wrong gives another stream on at least one design.  Printed: the designs that tell it
    apart and whether any of the earlier byte-exact cases did (the table of profiles/r17_entropy_coverage.md)."""
    rule = E.MUTANTS[mutant]
    killed = [n for n in MUTANT_FRAMES if E.restate(E.frame(n), E.frame(n).shape[1], rule, census=False)[0] != E.restated(n)[0]]
    tails = 0
    for n in MUTANT_TAILS:
        for kind in (0, 1):
            g = E.tail_frame(n, kind)
            tails += E.restate(g, n, rule, census=False)[0] != E.restate(g, n, census=False)[0]
    earlier = [E.named_case(c, lena_grid) for c in E.NAMED] + E.random_cases()
    old = sum(E.restate(g, g.shape[1], rule, census=False)[0] != E.restate(g, g.shape[1], census=False)[0] for g in earlier)
    print("%-24s designs: %s; tails %d of %d; earlier cases %d of %d" % (mutant, ", ".join(killed) or "-", tails, 2 * len(MUTANT_TAILS), old,
                                                                           len(earlier)))
    assert killed or tails
