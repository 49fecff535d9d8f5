#!/usr/bin/env python3
"""Generates tests/golden/sviews_refusals.json: the status and the full hgi_sviews_last_error() text of a fixed list of refused
calls to libhgi_sviews.so, recorded from the library built in this tree.  tests/test_sviews.py replays the list and asserts
status and text, so that neither a message nor the order in which the rules are decided can drift unseen.

A refused call touches no buffer and reaches no launch: device pointers are plain numbers, the plan's own memory (h_plan, info)
is the replayer's.  No device is needed: the plan makes no HIP call, and the launch entry decides its argument rules before the
first one.

RULES lists one entry per rule of include/hgi_sviews.h, in the header's order: the plan entry's, then the launch entry's; PAIRS
one per adjacent pair of rules that a single call can break together -- the earlier rule's text is what gets recorded.  Before
anything is written the generator checks that every call is refused with the status its rule has, that each solo text holds
the words of ITS rule, and that the solo texts are all different.

A call is {"fn": "plan" | "decode", ...}:
  plan:   views = [[src, dst, width, height, src_pitch, dst_pitch], ...] or null; shift; h_plan / info: true (the replayer's
          memory) or null; plan_bytes: "enough" or a number
  decode: info = the views of a valid plan to make first (at `shift`), or null, then `damage` = {field: value} written into it;
          d_plan: a number or null; levels, interp
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

OUT = os.path.join(HERE, "sviews_refusals.json")
A, B, C, D = 1 << 50, 2 << 50, 3 << 50, 4 << 50      # plain numbers, far apart
OKV = [A, B, 300, 200, 320, 160]                     # one served grid at shift 1: a 150 x 100 image, rows 160 apart
BIG = [A, B, 0xFFFFFFFF, 0xFFFFFFFF, 1 << 32, 1 << 32]      # 2^49 output tiles at shift 1


def plan(views=(OKV,), shift=1, h_plan=True, info=True, plan_bytes="enough"):
    return dict(fn="plan", views=None if views is None else [list(v) for v in views], shift=shift, h_plan=h_plan, info=info, plan_bytes=plan_bytes)


def launch(info=(OKV,), shift=1, damage=None, d_plan=D, levels=4, interp=1):
    return dict(fn="decode", info=None if info is None else [list(v) for v in info], shift=shift, damage=damage or {}, d_plan=d_plan, levels=levels,
                interp=interp)


def edit(v, **kw):
    names = ("src", "dst", "width", "height", "src_pitch", "dst_pitch")
    return [kw.get(n, x) for n, x in zip(names, v)]


EINVAL, EUNSUPPORTED = "HGI_EINVAL", "HGI_EUNSUPPORTED"
# (rule, status, words of its text, call) in the order in which the rules are decided
RULES = [
    ("null_argument", EINVAL, "NULL argument", plan(views=None)),
    ("plan_bytes", EINVAL, "plan_bytes 8 <", plan(plan_bytes=8)),
    ("shift_range", EINVAL, "shift 32 out of range", plan(shift=32)),
    ("null_entry", EINVAL, "view 1: NULL src", plan(views=(OKV, edit(OKV, src=0, dst=C)))),
    ("src_pitch", EINVAL, "view 0: source pitch 299 < width 300", plan(views=(edit(OKV, src_pitch=299),))),
    ("dst_pitch", EINVAL, "view 0: destination pitch 149 < scaled width 150", plan(views=(edit(OKV, dst_pitch=149),))),
    ("tiles", EINVAL, "more tiles than a launch holds", plan(views=(edit(BIG, dst=D),))),
    ("out_out", EINVAL, "the outputs of views 0 and 1 share bytes", plan(views=(OKV, edit(OKV, src=C, dst=B + 99 * 160 + 149)))),
    ("out_in", EINVAL, "the output of view 1 shares bytes with the grid of view 0", plan(views=(OKV, edit(OKV, src=C, dst=A + 100, dst_pitch=320)))),
    ("shift_zero", EUNSUPPORTED, "shift 0 is full resolution", plan(views=(edit(OKV, dst_pitch=320),), shift=0)),
    ("read32", EUNSUPPORTED, "view 0: its grid's offsets do not fit", plan(views=(edit(OKV, src_pitch=1 << 31),))),
    ("write32", EUNSUPPORTED, "view 1: its output's offsets do not fit", plan(views=(OKV, edit(OKV, src=C, dst=D, dst_pitch=1 << 32)))),
    ("info_null", EINVAL, "info is NULL", launch(info=None)),
    ("info_inconsistent", EINVAL, "info is not what hgi_sviews_plan wrote", launch(damage=dict(magic=0x12345678))),
    ("d_plan_null", EINVAL, "d_plan is NULL", launch(d_plan=None)),
    ("d_plan_aligned", EINVAL, "d_plan is not 16-byte aligned", launch(d_plan=D + 8)),
    ("levels_range", EINVAL, "levels 32 out of range", launch(levels=32)),
    ("interp", EINVAL, "interpolator 7 unknown", launch(interp=7)),
    ("levels_zero", EUNSUPPORTED, "levels 0: nothing to decode", launch(levels=0)),
    ("levels_shift", EUNSUPPORTED, "levels 2 <= shift 2", launch(shift=2, levels=2)),
    ("depth", EUNSUPPORTED, "levels 10 - shift 1", launch(levels=10)),
]
PAIRS = [
    ("null_argument", "plan_bytes", plan(views=None, plan_bytes=8)),
    ("plan_bytes", "shift_range", plan(plan_bytes=8, shift=40)),
    ("shift_range", "null_entry", plan(views=(edit(OKV, src=0),), shift=32)),
    ("null_entry", "src_pitch", plan(views=(edit(OKV, dst=0, src_pitch=31),))),
    ("src_pitch", "dst_pitch", plan(views=(edit(OKV, src_pitch=299, dst_pitch=3),))),
    ("dst_pitch", "tiles", plan(views=(edit(OKV, dst_pitch=149), edit(BIG, dst=D)))),
    ("tiles", "out_out", plan(views=(BIG, edit(BIG, src=C)))),
    ("out_out", "out_in", plan(views=(edit(OKV, dst=A + 100, dst_pitch=320), edit(OKV, src=C, dst=D), edit(OKV, src=C + (1 << 30), dst=D + 8)))),
    ("out_in", "shift_zero", plan(views=(edit(OKV, dst=A, dst_pitch=320),), shift=0)),
    ("shift_zero", "read32", plan(views=(edit(OKV, src_pitch=1 << 33, dst_pitch=320),), shift=0)),
    ("read32", "write32", plan(views=(edit(OKV, src_pitch=1 << 31, dst=D, dst_pitch=1 << 32),))),
    ("info_inconsistent", "d_plan_null", launch(damage=dict(plan_bytes=1), d_plan=None)),
    ("d_plan_aligned", "levels_range", launch(d_plan=D + 4, levels=40)),
    ("levels_range", "interp", launch(levels=32, interp=-1)),
    ("interp", "levels_zero", launch(interp=7, levels=0)),
    ("interp", "depth", launch(interp=2, levels=31)),
]
INFEASIBLE = {("info_null", "info_inconsistent"): "a NULL info has no field to be inconsistent",
              ("d_plan_null", "d_plan_aligned"): "NULL is aligned",
              ("levels_zero", "levels_shift"): "levels has one value", ("levels_shift", "depth"): "levels has one value"}
EXTRAS = [
    ("null_argument", "h_plan", plan(h_plan=None)),
    ("null_argument", "info", plan(info=None)),
    ("null_entry", "dst", plan(views=(edit(OKV, dst=0),))),
    ("dst_pitch", "shift 2: the image is 75 wide", plan(views=(edit(OKV, dst_pitch=74),), shift=2)),
    ("out_out", "different pitches", plan(views=(OKV, edit(OKV, src=C, dst=B + 400, dst_pitch=224)))),
    ("out_out", "side by side is fine, one byte nearer is not", plan(views=(edit(OKV, dst_pitch=320), edit(OKV, src=C, dst=B + 149, dst_pitch=320)))),
    ("out_in", "in place", plan(views=(edit(OKV, dst=A, dst_pitch=320),))),
    ("out_in", "an off-lattice byte of the grid", plan(views=(OKV, edit(OKV, src=C, dst=A + 199 * 320 + 299, width=1, height=1)))),
    ("out_in", "different pitches", plan(views=(OKV, edit(OKV, src=C, dst=A + 10, dst_pitch=321)))),
    ("read32", "a span of 2^32", plan(views=(edit(OKV, height=2, src_pitch=(1 << 32) - 300),))),
    ("read32", "shift 25: a tile's columns", plan(views=(OKV,), shift=25)),
    ("info_inconsistent", "block count", launch(damage=dict(edge_tiles=0, interior_tiles=0))),
    ("info_inconsistent", "offset", launch(damage=dict(edge_prefix_offset=0))),
    ("info_inconsistent", "shift 0 on a plan with grids", launch(damage=dict(shift=0))),
    ("info_inconsistent", "shift 32", launch(damage=dict(shift=32))),
    ("info_inconsistent", "the view lists' magic", launch(damage=dict(magic=0x56494731))),
    ("info_inconsistent", "the mapped view lists' magic", launch(damage=dict(magic=0x564D4731))),
    ("levels_shift", "levels below the shift", launch(shift=3, levels=1)),
    ("depth", "levels 31", launch(levels=31)),
]


def main():
    import test_sviews
    from rustyhgi_amd import _ffi
    status_of = {EINVAL: _ffi.EINVAL, EUNSUPPORTED: _ffi.EUNSUPPORTED}
    rules = dict((r[0], r) for r in RULES)
    assert set((a, b) for a, b, _ in PAIRS) | set(INFEASIBLE) >= set(
        (x[0], y[0]) for x, y in zip(RULES, RULES[1:]) if x[3]["fn"] == y[3]["fn"]), "an adjacent pair is missing"
    entries = []

    def record(kind, rule, other, note, call):
        st, text = test_sviews.replay(call)
        _, want, words, _ = rules[rule]
        assert st == status_of[want], (kind, rule, other, note, st, text)
        if kind == "solo":
            assert words in text, (rule, text)
        else:      # the same statement as the rule's solo call: its first words
            assert text.split(":")[0].split(" ")[0] == words.split(":")[0].split(" ")[0] or words[:12] in text, (kind, rule, other, note, text)
        entries.append(dict(kind=kind, rule=rule, also_breaks=other, note=note, call=call, status=st, error=text))

    for rule, _, _, call in RULES:
        record("solo", rule, None, "", call)
    assert len(set(e["error"] for e in entries)) == len(RULES), "two rules share a text"
    for a, b, call in PAIRS:
        record("pair", a, b, "", call)
    for rule, note, call in EXTRAS:
        record("extra", rule, None, note, call)
    with open(OUT, "w") as fh:
        json.dump(dict(comment="recorded by tests/golden/make_sviews_refusals.py; replayed by tests/test_sviews.py",
                       pointers="plain numbers (null: NULL)", calls=entries), fh, indent=1)
        fh.write("\n")
    print("%d refused calls -> %s" % (len(entries), OUT))


if __name__ == "__main__":
    main()
