#!/usr/bin/env python3
"""Generates tests/golden/tviews_refusals.json: the status and the full hgi_tviews_last_error() text of a fixed list of refused
calls to libhgi_tviews.so, recorded from the library built in this tree.  tests/test_tviews.py replays the list and asserts
status and text, so that neither a message nor the order in which the rules are decided can drift unseen.

A refused call touches no buffer and reaches no launch: device pointers are plain numbers, the plan's own memory (h_plan, info)
and the table are the replayer's.  No device is needed: the plan makes no HIP call, and the launch entry decides its argument
rules before the first one.

RULES lists one entry per `fail(` statement an argument can reach (rustyhgi_amd/tviews/hgi_tviews.hip): the plan entry's, then
the launch entry's judge; PAIRS one per adjacent pair of rules that a single call can break together -- the earlier rule's text
is what gets recorded.  Before anything is written the generator checks that the statements found in the source are as many as
the rules listed (plus the HGI_EDEVICE one and the unreachable default of the verdict switch), that each solo text matches a
format string of ITS statement, that every format string is met, and that no call returns HGI_OK.

A call is {"fn": "plan" | "encode", ...}:
  plan:   views = [[src, dst, width, height, src_pitch, dst_pitch], ...] or null; elem: the element size; h_plan / info: true
          (the replayer's memory) or null; plan_bytes: "enough" or a number
  encode: info = the views of a valid plan to make first (with `elem`), or null, then `damage` = {field: value} written into it;
          d_plan: a number or null; lut: true (256 bytes of the replayer's) or null; kind; scale, bias: float32 values as
          text ("inf", "nan" included); levels, interp
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

from make_views_refusals import fail_statements, format_regex      # noqa: E402  (the parser of fail( statements, shared)

OUT = os.path.join(HERE, "tviews_refusals.json")
A, B, C, D = 1 << 50, 2 << 50, 3 << 50, 4 << 50      # plain numbers, page aligned, far apart
OKV = [A, B, 32, 8, 192, 40]                          # one served view at E = 4 (and at E = 2): frame rows 192 bytes apart, grid rows 40
TAIL = [A + 4096 - (7 * 80 + 62), B, 31, 8, 80, 40]   # E = 2, an odd width, the frame's span ends on a page boundary
BIG = [A, B, 128 << 16, 64 << 15, 4 * (128 << 16), 128 << 16]      # 2^31 tiles


def plan(views=(OKV,), elem=4, h_plan=True, info=True, plan_bytes="enough"):
    return dict(fn="plan", views=None if views is None else [list(v) for v in views], elem=elem, h_plan=h_plan, info=info, plan_bytes=plan_bytes)


def launch(info=(OKV,), elem=4, damage=None, d_plan=D, lut=True, kind=0, scale="255.0", bias="0.0", levels=2, interp=1):
    return dict(fn="encode", info=None if info is None else [list(v) for v in info], elem=elem, damage=damage or {}, d_plan=d_plan, lut=lut, kind=kind,
                scale=scale, bias=bias, levels=levels, interp=interp)


def edit(v, **kw):
    names = ("src", "dst", "width", "height", "src_pitch", "dst_pitch")
    return [kw.get(n, x) for n, x in zip(names, v)]


# (rule, call) in the order in which the rules are decided
RULES = [
    ("null_argument", plan(views=None)),
    ("plan_bytes", plan(plan_bytes=8)),
    ("elem_size", plan(elem=3)),
    ("null_entry", plan(views=(OKV, edit(OKV, src=0, dst=C)))),
    ("src_align", plan(views=(OKV, edit(OKV, src=C + 2, dst=D)))),
    ("src_pitch_align", plan(views=(edit(OKV, src_pitch=194),))),
    ("src_pitch", plan(views=(edit(OKV, src_pitch=124),))),
    ("dst_pitch", plan(views=(edit(OKV, dst_pitch=31),))),
    ("tiles", plan(views=(BIG,))),
    ("out_out", plan(views=(OKV, edit(OKV, src=C, dst=B + 7 * 40 + 31)))),
    ("out_in", plan(views=(OKV, edit(OKV, src=C, dst=A + 100, dst_pitch=192)))),
    ("fits32", plan(views=(edit(OKV, src_pitch=1 << 25),))),
    ("tail", plan(views=(OKV, edit(TAIL, src=TAIL[0] + (1 << 40), dst=C)), elem=2)),
    ("info_null", launch(info=None)),
    ("info_inconsistent", launch(damage=dict(magic=0x12345678))),
    ("d_plan_null", launch(d_plan=None)),
    ("d_plan_aligned", launch(d_plan=D + 8)),
    ("lut_null", launch(lut=None)),
    ("elem_kind", launch(kind=2)),
    ("bf16_elem", launch(kind=1)),
    ("scale_bias", launch(scale="inf")),
    ("levels_range", launch(levels=32)),
    ("interp", launch(interp=7)),
    ("levels_launch", launch(levels=9)),
]
PAIRS = [
    ("null_argument", "plan_bytes", plan(views=None, plan_bytes=8)),
    ("plan_bytes", "elem_size", plan(plan_bytes=8, elem=3)),
    ("elem_size", "null_entry", plan(views=(edit(OKV, src=0),), elem=8)),
    ("null_entry", "src_align", plan(views=(edit(OKV, src=A + 2, dst=0),))),
    ("src_align", "src_pitch_align", plan(views=(edit(OKV, src=A + 2, src_pitch=193),))),
    ("src_pitch_align", "src_pitch", plan(views=(edit(OKV, src_pitch=101),))),
    ("src_pitch", "dst_pitch", plan(views=(edit(OKV, src_pitch=124, dst_pitch=31),))),
    ("dst_pitch", "tiles", plan(views=(edit(OKV, dst_pitch=31), BIG))),
    ("tiles", "out_out", plan(views=(BIG, edit(BIG, src=C)))),
    ("out_out", "out_in", plan(views=(edit(OKV, dst=A + 100, dst_pitch=192), edit(OKV, src=C, dst=D), edit(OKV, src=C + 4096, dst=D + 8)))),
    ("out_in", "fits32", plan(views=(edit(OKV, dst=A, src_pitch=1 << 25, dst_pitch=1 << 25),))),
    ("fits32", "tail", plan(views=(edit(TAIL, dst_pitch=1 << 25),), elem=2)),
    ("info_inconsistent", "d_plan_null", launch(damage=dict(plan_bytes=1), d_plan=None)),
    ("d_plan_aligned", "lut_null", launch(d_plan=D + 4, lut=None)),
    ("lut_null", "elem_kind", launch(lut=None, kind=2)),
    ("bf16_elem", "scale_bias", launch(kind=1, scale="nan")),
    ("scale_bias", "levels_range", launch(bias="inf", levels=40)),
    ("levels_range", "interp", launch(levels=32, interp=-1)),
    ("interp", "levels_launch", launch(interp=7, levels=0)),
]
INFEASIBLE = {("info_null", "info_inconsistent"): "a NULL info has no field to be inconsistent",
              ("d_plan_null", "d_plan_aligned"): "NULL is aligned",
              ("elem_kind", "bf16_elem"): "a kind above 1 is not bfloat16"}
EXTRAS = [
    ("null_argument", "h_plan", plan(h_plan=None)),
    ("null_argument", "info", plan(info=None)),
    ("elem_size", "0", plan(elem=0)),
    ("elem_size", "1: the view lists' job", plan(elem=1)),
    ("null_entry", "dst", plan(views=(edit(OKV, dst=0),))),
    ("src_align", "E = 2, an odd address", plan(views=(edit(OKV, src=A + 1),), elem=2)),
    ("src_pitch_align", "E = 2", plan(views=(edit(OKV, src_pitch=65),), elem=2)),
    ("src_pitch", "E = 2: one element short", plan(views=(edit(OKV, src_pitch=62),), elem=2)),
    ("src_pitch", "the view lists' byte pitch", plan(views=(edit(OKV, src_pitch=48),))),
    ("dst_pitch", "the grid's pitch is in bytes of pixels", plan(views=(edit(OKV, dst_pitch=28),), elem=2)),
    ("out_out", "different pitches", plan(views=(OKV, edit(OKV, src=C, dst=B + 100, dst_pitch=56)))),
    ("out_out", "side by side is fine, one byte nearer is not", plan(views=(edit(OKV, dst_pitch=64), edit(OKV, src=C, dst=B + 31, dst_pitch=64)))),
    ("out_in", "in place", plan(views=(edit(OKV, dst=A, dst_pitch=192),))),
    ("out_in", "different pitches", plan(views=(OKV, edit(OKV, src=C, dst=A + 10)))),
    ("out_in", "a grid on the last byte of a frame row", plan(views=(OKV, edit(OKV, src=C, dst=A + 127, dst_pitch=192, width=4, src_pitch=16)))),
    ("out_in", "E = 2: a frame row is 64 bytes", plan(views=(OKV, edit(OKV, src=C, dst=A + 63, dst_pitch=192, width=4, src_pitch=16)), elem=2)),
    ("fits32", "grid side", plan(views=(edit(OKV, dst_pitch=1 << 25),))),
    ("fits32", "a byte pitch of 2^32", plan(views=(edit(OKV, src_pitch=1 << 32),))),
    ("tail", "alone", plan(views=(TAIL,), elem=2)),
    ("info_inconsistent", "block count", launch(damage=dict(edge_tiles=0, interior_tiles=0))),
    ("info_inconsistent", "offset", launch(damage=dict(edge_prefix_offset=0))),
    ("info_inconsistent", "element size", launch(damage=dict(elem_size=1))),
    ("info_inconsistent", "the view lists' magic", launch(damage=dict(magic=0x56494731))),
    ("info_inconsistent", "the mapped view lists' magic", launch(damage=dict(magic=0x564D4731))),
    ("scale_bias", "bfloat16 passes the kind rules on a 2-byte plan: the scale decides", launch(elem=2, kind=1, scale="-inf")),
    ("scale_bias", "a NaN bias", launch(bias="nan")),
    ("levels_launch", "levels 0", launch(levels=0)),
    ("levels_launch", "levels 31", launch(levels=31)),
]


def main():
    import test_tviews
    from rustyhgi_amd import _ffi
    status_of = {"HGI_EINVAL": _ffi.EINVAL, "HGI_EUNSUPPORTED": _ffi.EUNSUPPORTED}
    stmts = [(s[0], [f for f in s[1] if " " in f]) for s in fail_statements(os.path.join(ROOT, "rustyhgi_amd", "tviews", "hgi_tviews.hip"))
             if s[0] != "HGI_EDEVICE"]      # (one-word literals are arguments of a format, not formats)
    assert stmts[-1][1] == ["unknown verdict"], stmts[-1]      # the default of the verdict switch: no argument reaches it
    del stmts[-1]
    # source order: the launch entry's judge stands in front of the plan entry
    judge = [s for s in stmts if any(k in " ".join(s[1]) for k in ("info is", "d_plan", "lut is NULL", "elem_kind", "scale and bias", "levels %u", "interpolator"))]
    ordered = [s for s in stmts if s not in judge] + judge
    assert len(judge) == 11 and len(ordered) == len(RULES), (len(judge), len(ordered), len(RULES))
    index = dict((k, i) for i, (k, _) in enumerate(RULES))
    assert set((a, b) for a, b, _ in PAIRS) | set(INFEASIBLE) >= set(
        (x[0], y[0]) for x, y in zip(RULES, RULES[1:]) if x[1]["fn"] == y[1]["fn"]), "an adjacent pair is missing"
    entries, matched = [], set()

    def record(kind, rule, other, note, call):
        st, text = test_tviews.replay(call)
        want, fmts = ordered[index[rule]]
        hit = [f for f in fmts if format_regex(f).match(text)]
        assert st == status_of[want] and hit, (kind, rule, other, note, st, text)
        matched.update((index[rule], f) for f in hit)
        entries.append(dict(kind=kind, rule=rule, also_breaks=other, note=note, call=call, status=st, error=text))

    for rule, call in RULES:
        record("solo", rule, None, "", call)
    for a, b, call in PAIRS:
        record("pair", a, b, "", call)
    for rule, note, call in EXTRAS:
        record("extra", rule, None, note, call)
    unmatched = [(RULES[i][0], f) for i, (_, fmts) in enumerate(ordered) for f in fmts if (i, f) not in matched]
    assert not unmatched, unmatched
    with open(OUT, "w") as fh:
        json.dump(dict(comment="recorded by tests/golden/make_tviews_refusals.py; replayed by tests/test_tviews.py",
                       pointers="plain numbers (null: NULL)", calls=entries), fh, indent=1)
        fh.write("\n")
    print("%d refused calls -> %s" % (len(entries), OUT))


if __name__ == "__main__":
    main()
