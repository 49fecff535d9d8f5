#!/usr/bin/env python3
"""Generates tests/golden/rviews_refusals.json: the status and the full hgi_rviews_last_error() text of a fixed list of refused
calls to libhgi_rviews.so, recorded from the library built in this tree.  tests/test_rviews.py replays the list and asserts
status and text, so that neither a message nor the order in which the rules are decided can drift unseen.

A refused call touches no buffer and reaches no launch: device pointers are plain numbers, the plan's own memory (h_plan, info)
is the replayer's.  No device is needed: the plan makes no HIP call, and the launch entry decides its argument rules before the
first one.

RULES lists one entry per rule of include/hgi_rviews.h, in the header's order: the plan entry's, then the launch entry's; PAIRS
one per adjacent pair of rules that a single call can break together -- the earlier rule's text is what gets recorded.  Before
anything is written the generator checks that every call is refused with the status its rule has, that each solo text holds
the words of ITS rule, and that the solo texts are all different.

A call is {"fn": "plan" | "encode", ...}:
  plan:   triples = [[src, grid, recon, width, height, src_pitch, grid_pitch, recon_pitch], ...] or null; h_plan / info: true (the
          replayer's memory) or null; plan_bytes: "enough" or a number
  encode: info = the triples of a valid plan to make first, or null, then `damage` = {field: value} written into it; d_plan: a
          number or null; levels, interp; lut: "medium", "identity" or null
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

OUT = os.path.join(HERE, "rviews_refusals.json")
A, B, C, D = 1 << 50, 2 << 50, 3 << 50, 4 << 50      # plain numbers, far apart
OKV = [A, B, C, 300, 200, 320, 304, 384]             # one served frame: 300 x 200, three pitches
FAR = 1 << 40                                        # a second entry of the same shape, this far behind the first on every side
BIG = [A, B, C, 0xFFFFFFFF, 0xFFFFFFFF, 1 << 32, 1 << 32, 1 << 32]      # 2^49 tiles
NAMES = ("src", "grid", "recon", "width", "height", "src_pitch", "grid_pitch", "recon_pitch")
PAGE_END = (A & ~4095) + 64 * 4096                   # a source span that ends here ends with its 4-KiB page


def plan(triples=(OKV,), h_plan=True, info=True, plan_bytes="enough"):
    return dict(fn="plan", triples=None if triples is None else [list(t) for t in triples], h_plan=h_plan, info=info, plan_bytes=plan_bytes)


def launch(info=(OKV,), damage=None, d_plan=D, levels=4, interp=1, lut="medium"):
    return dict(fn="encode", info=None if info is None else [list(t) for t in info], damage=damage or {}, d_plan=d_plan, levels=levels, interp=interp,
                lut=lut)


def edit(t, **kw):
    return [kw.get(n, x) for n, x in zip(NAMES, t)]


def far(t, **kw):
    """The entry moved FAR on every side, then edited."""
    return edit(edit(t, src=t[0] + FAR, grid=t[1] + FAR, recon=t[2] + FAR), **kw)


EINVAL, EUNSUPPORTED = "HGI_EINVAL", "HGI_EUNSUPPORTED"
TAIL = far(OKV, width=299, src=PAGE_END - (199 * 320 + 299))
# (rule, status, words of its text, call) in the order in which the rules are decided
RULES = [
    ("null_argument", EINVAL, "NULL argument", plan(triples=None)),
    ("plan_bytes", EINVAL, "plan_bytes 8 <", plan(plan_bytes=8)),
    ("null_entry", EINVAL, "view 1: NULL recon", plan(triples=(OKV, far(OKV, recon=0)))),
    ("src_pitch", EINVAL, "view 0: source pitch 299 < width 300", plan(triples=(edit(OKV, src_pitch=299),))),
    ("grid_pitch", EINVAL, "view 0: grid pitch 299 < width 300", plan(triples=(edit(OKV, grid_pitch=299),))),
    ("recon_pitch", EINVAL, "view 1: reconstruction pitch 3 < width 300", plan(triples=(OKV, far(OKV, recon_pitch=3)))),
    ("tiles", EINVAL, "more tiles than a launch holds", plan(triples=(BIG,))),
    ("out_out", EINVAL, "the grid of view 0 and the reconstruction of view 1 share bytes", plan(triples=(OKV, far(OKV, recon=B + 199 * 304 + 299, recon_pitch=304)))),
    ("out_in", EINVAL, "the reconstruction of view 1 shares bytes with the input of view 0", plan(triples=(OKV, far(OKV, recon=A + 100, recon_pitch=320)))),
    ("fits32", EUNSUPPORTED, "view 1: its offsets do not fit", plan(triples=(OKV, far(OKV, recon=D, recon_pitch=1 << 32)))),
    ("tail", EUNSUPPORTED, "view 1: width 299 is not a multiple of 4", plan(triples=(OKV, TAIL))),
    ("info_null", EINVAL, "info is NULL", launch(info=None)),
    ("info_inconsistent", EINVAL, "info is not what hgi_rviews_plan wrote", launch(damage=dict(magic=0x12345678))),
    ("d_plan_null", EINVAL, "d_plan is NULL", launch(d_plan=None)),
    ("d_plan_aligned", EINVAL, "d_plan is not 16-byte aligned", launch(d_plan=D + 8)),
    ("lut_null", EINVAL, "lut is NULL", launch(lut=None)),
    ("levels_range", EINVAL, "levels 32 out of range", launch(levels=32)),
    ("interp", EINVAL, "interpolator 7 unknown", launch(interp=7)),
    ("levels", EUNSUPPORTED, "levels 9: one launch serves 1..=8 levels", launch(levels=9)),
]
PAIRS = [
    ("null_argument", "plan_bytes", plan(triples=None, plan_bytes=8)),
    ("plan_bytes", "null_entry", plan(triples=(edit(OKV, src=0),), plan_bytes=8)),
    ("null_entry", "src_pitch", plan(triples=(edit(OKV, grid=0, src_pitch=31),))),
    ("src_pitch", "grid_pitch", plan(triples=(edit(OKV, src_pitch=299, grid_pitch=3),))),
    ("grid_pitch", "recon_pitch", plan(triples=(edit(OKV, grid_pitch=299, recon_pitch=3),))),
    ("recon_pitch", "tiles", plan(triples=(edit(OKV, recon_pitch=299), BIG))),
    ("tiles", "out_out", plan(triples=(BIG, edit(BIG, src=D)))),
    ("out_out", "out_in", plan(triples=(edit(OKV, grid=A + 100, grid_pitch=320), far(OKV), edit(far(OKV), src=D, grid=C + FAR + 8, grid_pitch=384)))),
    ("out_in", "fits32", plan(triples=(edit(OKV, grid=A, grid_pitch=320), far(OKV, recon=D, recon_pitch=1 << 32)))),
    ("fits32", "tail", plan(triples=(edit(OKV, recon=D, recon_pitch=1 << 32), TAIL))),
    ("info_inconsistent", "d_plan_null", launch(damage=dict(plan_bytes=1), d_plan=None)),
    ("d_plan_aligned", "lut_null", launch(d_plan=D + 4, lut=None)),
    ("lut_null", "levels_range", launch(lut=None, levels=40)),
    ("levels_range", "interp", launch(levels=32, interp=-1)),
    ("interp", "levels", launch(interp=7, levels=0)),
    # one rule of each kind in one call: the HGI_EINVAL text is what gets recorded
    ("recon_pitch", "fits32", plan(triples=(OKV, far(OKV, recon_pitch=3, grid=D, grid_pitch=1 << 32)))),
    ("out_out", "tail", plan(triples=(OKV, edit(TAIL, grid=C + 5, grid_pitch=384)))),
    ("d_plan_null", "levels", launch(d_plan=None, levels=9)),
]
INFEASIBLE = {("info_null", "info_inconsistent"): "a NULL info has no field to be inconsistent",
              ("d_plan_null", "d_plan_aligned"): "NULL is aligned"}
EXTRAS = [
    ("null_argument", "h_plan", plan(h_plan=None)),
    ("null_argument", "info", plan(info=None)),
    ("null_entry", "src", plan(triples=(edit(OKV, src=0),))),
    ("null_entry", "grid", plan(triples=(edit(OKV, grid=0),))),
    ("out_out", "grid against recon of the same entry", plan(triples=(OKV, far(OKV, recon=B + FAR + 100 * 304 + 7, recon_pitch=304)))),
    ("out_out", "grid against grid", plan(triples=(OKV, far(OKV, grid=B + 1)))),
    ("out_out", "recon against recon", plan(triples=(OKV, far(OKV, recon=C + 199 * 384 + 299)))),
    ("out_out", "recon of an earlier entry against grid of a later one", plan(triples=(edit(OKV, recon=B + FAR + 199 * 304, recon_pitch=304), far(OKV)))),
    ("out_out", "side by side in one parent's rows is fine, one byte nearer is not", plan(triples=(edit(OKV, grid=B, recon=B + 299, grid_pitch=1024, recon_pitch=1024),))),
    ("out_out", "the same windows at different pitches", plan(triples=(edit(OKV, grid=B, recon=B + 300, grid_pitch=1024, recon_pitch=1025),))),
    ("out_in", "a grid against an input", plan(triples=(OKV, far(OKV, grid=A + 64, grid_pitch=320)))),
    ("out_in", "in place", plan(triples=(edit(OKV, recon=A, recon_pitch=320),))),
    ("out_in", "different pitches", plan(triples=(OKV, far(OKV, grid=A + 300, grid_pitch=321)))),
    ("fits32", "only the source pitch over the bound", plan(triples=(edit(OKV, src_pitch=1 << 32),))),
    ("fits32", "only the grid pitch over the bound", plan(triples=(edit(OKV, grid=D, grid_pitch=10956600),))),
    ("tail", "two bytes in front of the page's end", plan(triples=(OKV, edit(TAIL, src=TAIL[0] - 2)))),
    ("info_inconsistent", "block count", launch(damage=dict(edge_tiles=0, interior_tiles=0))),
    ("info_inconsistent", "offset", launch(damage=dict(edge_prefix_offset=0))),
    ("info_inconsistent", "recon_offset", launch(damage=dict(recon_offset=0))),
    ("info_inconsistent", "plan_bytes without the third sides", launch(damage=dict(plan_bytes=64 + 32))),
    ("info_inconsistent", "reserved", launch(damage=dict(reserved=1))),
    ("info_inconsistent", "the view lists' magic", launch(damage=dict(magic=0x56494731))),
    ("info_inconsistent", "the mapped view lists' magic", launch(damage=dict(magic=0x564D4731))),
    ("info_inconsistent", "the typed view lists' magic", launch(damage=dict(magic=0x56544731))),
    ("info_inconsistent", "the scaled view lists' magic", launch(damage=dict(magic=0x56534731))),
    ("levels", "levels 0", launch(levels=0)),
    ("levels", "levels 31", launch(levels=31)),
    ("levels", "levels 0 under the identity table", launch(levels=0, lut="identity")),
]


def main():
    import test_rviews
    from rustyhgi_amd import _ffi
    status_of = {EINVAL: _ffi.EINVAL, EUNSUPPORTED: _ffi.EUNSUPPORTED}
    rules = dict((r[0], r) for r in RULES)
    assert set((a, b) for a, b, _ in PAIRS) | set(INFEASIBLE) >= set(
        (x[0], y[0]) for x, y in zip(RULES, RULES[1:]) if x[3]["fn"] == y[3]["fn"]), "an adjacent pair is missing"
    entries = []

    def record(kind, rule, other, note, call):
        st, text = test_rviews.replay(call)
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
        json.dump(dict(comment="recorded by tests/golden/make_rviews_refusals.py; replayed by tests/test_rviews.py",
                       pointers="plain numbers (null: NULL)", calls=entries), fh, indent=1)
        fh.write("\n")
    print("%d refused calls -> %s" % (len(entries), OUT))


if __name__ == "__main__":
    main()
