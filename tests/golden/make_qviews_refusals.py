#!/usr/bin/env python3
"""Generates tests/golden/qviews_refusals.json: the status and the full hgi_qviews_last_error() text of a fixed list of refused
calls to libhgi_qviews.so, recorded from the library built in this tree.  tests/test_qviews.py replays the list and asserts
status and text, so that neither a message nor the order in which the rules are decided can drift unseen.

A refused call touches no buffer and reaches no launch: d_plan is a plain number, the info is made by hgi_views_plan of
libhgi_views.so (the plan of this library IS the view lists') in the replayer's memory, and so is the table.  No device is
needed: the judgement (rustyhgi_amd/qviews/hgi_qviews_plan.h, qviews_judge) makes no HIP call and stands in front of the launch.

RULES lists one entry per refusal of qviews_judge, in the order in which they are decided; PAIRS one per adjacent pair of rules
that a single call can break together -- the earlier rule's text is what gets recorded.  Before anything is written the
generator checks that the refusals found in the header are as many as the rules listed and in their order, that each solo text
matches the format string of ITS refusal and its status, and that no call returns HGI_OK.

A call is {info, damage, d_plan, lut, levels, interp}: info = the views [[src, dst, width, height, src_pitch, dst_pitch], ...] of a
valid plan to make first, or null, then `damage` = {field: value} written into it; d_plan: a number or null; lut: "coarse",
"identity", "identity^N" (the identity with the lowest bit of entry N flipped) or null; levels, interp.
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

from make_views_refusals import format_regex      # noqa: E402  (format string -> regular expression, shared)

OUT = os.path.join(HERE, "qviews_refusals.json")
A, B, D = 1 << 50, 2 << 50, 4 << 50      # plain numbers, page aligned, far apart
OKV = [A, B, 300, 200, 320, 301]         # one served pair of grids


def launch(info=(OKV,), damage=None, d_plan=D, lut="coarse", levels=4, interp=1):
    return dict(info=None if info is None else [list(v) for v in info], damage=damage or {}, d_plan=d_plan, lut=lut, levels=levels, interp=interp)


# (rule, call) in the order in which the rules are decided
RULES = [
    ("info_null", launch(info=None)),
    ("info_inconsistent", launch(damage=dict(magic=0x12345678))),
    ("d_plan_null", launch(d_plan=None)),
    ("d_plan_aligned", launch(d_plan=D + 8)),
    ("lut_null", launch(lut=None)),
    ("levels_range", launch(levels=32)),
    ("interp", launch(interp=7)),
    ("levels_launch", launch(levels=9)),
    ("identity", launch(lut="identity")),
]
PAIRS = [
    ("info_inconsistent", "d_plan_null", launch(damage=dict(plan_bytes=1), d_plan=None)),
    ("d_plan_aligned", "lut_null", launch(d_plan=D + 4, lut=None)),
    ("lut_null", "levels_range", launch(lut=None, levels=40)),
    ("levels_range", "interp", launch(levels=32, interp=-1)),
    ("interp", "levels_launch", launch(interp=7, levels=0)),
    ("levels_launch", "identity", launch(levels=9, lut="identity")),
    # the identity table behind every HGI_EINVAL rule, not only its neighbour
    ("info_null", "identity", launch(info=None, lut="identity")),
    ("info_inconsistent", "identity", launch(damage=dict(edge_tiles=0, interior_tiles=0), lut="identity")),
    ("d_plan_null", "identity", launch(d_plan=None, lut="identity")),
    ("d_plan_aligned", "identity", launch(d_plan=D + 1, lut="identity")),
    ("levels_range", "identity", launch(levels=32, lut="identity")),
    ("interp", "identity", launch(interp=2, lut="identity")),
]
INFEASIBLE = {("info_null", "info_inconsistent"): "a NULL info has no field to be inconsistent",
              ("d_plan_null", "d_plan_aligned"): "NULL is aligned"}
EXTRAS = [
    ("info_inconsistent", "block count", launch(damage=dict(edge_tiles=0, interior_tiles=0))),
    ("info_inconsistent", "offset", launch(damage=dict(edge_prefix_offset=0))),
    ("info_inconsistent", "a reserved word that is set (the sibling infos' element size)", launch(damage=dict(reserved=4))),
    ("info_inconsistent", "the mapped view lists' magic", launch(damage=dict(magic=0x564D4731))),
    ("info_inconsistent", "the typed view lists' magic", launch(damage=dict(magic=0x56544731))),
    ("info_inconsistent", "a refused plan's info: all zero", launch(damage=dict(magic=0, count=0, edge_tiles=0, interior_tiles=0, max_width=0, plan_bytes=0,
                                                                               edge_prefix_offset=0, interior_prefix_offset=0))),
    ("levels_launch", "levels 0", launch(levels=0)),
    ("levels_launch", "levels 31", launch(levels=31)),
    ("levels_launch", "levels 0 under the identity table: the depth decides", launch(levels=0, lut="identity")),
    ("identity", "LeftTop, one level", launch(lut="identity", levels=1, interp=0)),
    ("identity", "the cone's depths", launch(lut="identity", levels=8)),
]


def refusals():
    """The refusals of qviews_judge in source order: [(status name, verdict name, format string)]."""
    src = open(os.path.join(ROOT, "rustyhgi_amd", "qviews", "hgi_qviews_plan.h")).read()
    body = src[src.index("inline QViewsJudged qviews_judge("):]
    return [(m.group(2), m.group(3), m.group(1)) for m in
            re.finditer(r'snprintf\(j\.text, sizeof\(j\.text\), "((?:[^"\\]|\\.)*)".*?return refuse\((HGI_\w+), (kQViews\w+)\);', body, flags=re.S)]


def main():
    import test_qviews
    from rustyhgi_amd import _ffi
    status_of = {"HGI_EINVAL": _ffi.EINVAL, "HGI_EUNSUPPORTED": _ffi.EUNSUPPORTED}
    ordered = refusals()
    assert len(ordered) == len(RULES), (len(ordered), len(RULES))
    assert [s for s, _, _ in ordered] == ["HGI_EINVAL"] * 7 + ["HGI_EUNSUPPORTED"] * 2, ordered
    index = dict((k, i) for i, (k, _) in enumerate(RULES))
    assert set((a, b) for a, b, _ in PAIRS) | set(INFEASIBLE) >= set((x[0], y[0]) for x, y in zip(RULES, RULES[1:])), "an adjacent pair is missing"
    entries, matched = [], set()

    def record(kind, rule, other, note, call):
        st, text = test_qviews.replay(call)
        want, _, fmt = ordered[index[rule]]
        assert st == status_of[want] and format_regex(fmt).match(text), (kind, rule, other, note, st, text)
        matched.add(index[rule])
        entries.append(dict(kind=kind, rule=rule, also_breaks=other, note=note, call=call, status=st, error=text))

    for rule, call in RULES:
        record("solo", rule, None, "", call)
    for a, b, call in PAIRS:
        record("pair", a, b, "", call)
    for rule, note, call in EXTRAS:
        record("extra", rule, None, note, call)
    assert matched == set(range(len(RULES)))
    with open(OUT, "w") as fh:
        json.dump(dict(comment="recorded by tests/golden/make_qviews_refusals.py; replayed by tests/test_qviews.py",
                       pointers="plain numbers (null: NULL)", calls=entries), fh, indent=1)
        fh.write("\n")
    print("%d refused calls -> %s" % (len(entries), OUT))


if __name__ == "__main__":
    main()
