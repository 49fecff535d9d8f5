#!/usr/bin/env python3
"""Generates tests/golden/views_refusals.json: the status and the full hgi_views_last_error() text of a fixed list of refused
calls to libhgi_views.so, recorded from the library built in this tree.  tests/test_views.py replays the list and asserts status
and text, so that neither a message nor the order in which the rules are decided can drift unseen.

A refused call touches no buffer and reaches no launch: device pointers are plain numbers, the plan's own memory (h_plan, info)
is the replayer's, `lut` is a real 256-byte host array.  No device is needed: the plan makes no HIP call, and the launch entries
decide their argument rules before the first one.

RULES lists one entry per `fail(` statement an argument can reach, in source order (rustyhgi_amd/views/hgi_views.hip): the plan
entry's, then the launch entries' shared judge; PAIRS one per adjacent pair of rules that a single call can break together --
the earlier rule's text is what gets recorded.  Before anything is written the generator checks that the statements found in the
source are as many as the rules listed (plus the two HGI_EDEVICE ones and the unreachable default of the verdict switch), that
each solo text matches a format string of ITS statement, and that no call returns HGI_OK.

A call is {"fn": "plan" | "encode" | "decode", ...}:
  plan:   views = [[src, dst, width, height, src_pitch, dst_pitch], ...] or null; h_plan / info: true (the replayer's memory) or
          null; plan_bytes: "enough" or a number
  launch: info = the views of a valid plan to make first, or null, then `damage` = {field: value} written into it;
          d_plan: a number or null; levels, interp; lut: "ramp" or null (encode only)
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

OUT = os.path.join(HERE, "views_refusals.json")
A, B, C, D = 1 << 50, 2 << 50, 3 << 50, 4 << 50      # plain numbers, page aligned, far apart
OKV = [A, B, 32, 8, 40, 48]                           # one served view
TAIL = [A + 4096 - (7 * 40 + 30), B, 30, 8, 40, 48]   # width % 4 != 0, the last source byte on the last byte of a page
BIG = [A, B, 128 << 16, 64 << 15, 128 << 16, 128 << 16]      # 2^31 tiles


def plan(views=(OKV,), h_plan=True, info=True, plan_bytes="enough"):
    return dict(fn="plan", views=None if views is None else [list(v) for v in views], h_plan=h_plan, info=info, plan_bytes=plan_bytes)


def launch(fn="encode", info=(OKV,), damage=None, d_plan=D, levels=2, interp=1, lut="ramp"):
    c = dict(fn=fn, info=None if info is None else [list(v) for v in info], damage=damage or {}, d_plan=d_plan, levels=levels, interp=interp)
    if fn == "encode":
        c["lut"] = lut
    return c


def edit(v, **kw):
    names = ("src", "dst", "width", "height", "src_pitch", "dst_pitch")
    return [kw.get(n, x) for n, x in zip(names, v)]


# (rule, call) in the order of the fail( statements
RULES = [
    ("null_argument", plan(views=None)),
    ("plan_bytes", plan(plan_bytes=8)),
    ("null_entry", plan(views=(OKV, edit(OKV, src=0, dst=C)))),
    ("src_pitch", plan(views=(edit(OKV, src_pitch=31),))),
    ("dst_pitch", plan(views=(edit(OKV, dst_pitch=31),))),
    ("tiles", plan(views=(BIG,))),
    ("out_out", plan(views=(OKV, edit(OKV, src=C, dst=B + 7 * 48 + 31)))),
    ("out_in", plan(views=(OKV, edit(OKV, src=C, dst=A + 100)))),
    ("fits32", plan(views=(edit(OKV, dst_pitch=1 << 25),))),
    ("tail", plan(views=(OKV, edit(TAIL, src=TAIL[0] + (1 << 40), dst=C)))),
    ("info_null", launch(info=None)),
    ("info_inconsistent", launch(damage=dict(magic=0x12345678))),
    ("d_plan_null", launch(d_plan=None)),
    ("d_plan_aligned", launch(d_plan=D + 8)),
    ("lut_null", launch(lut=None)),
    ("levels_range", launch(levels=32)),
    ("interp", launch(interp=7)),
    ("levels_launch", launch(levels=9)),
]
PAIRS = [
    ("null_argument", "plan_bytes", plan(views=None, plan_bytes=8)),
    ("plan_bytes", "null_entry", plan(views=(edit(OKV, src=0),), plan_bytes=8)),
    ("null_entry", "src_pitch", plan(views=(edit(OKV, dst=0, src_pitch=31),))),
    ("src_pitch", "dst_pitch", plan(views=(edit(OKV, src_pitch=31, dst_pitch=30),))),
    ("dst_pitch", "tiles", plan(views=(edit(OKV, dst_pitch=31), BIG))),
    ("tiles", "out_out", plan(views=(BIG, edit(BIG, src=C)))),
    ("out_out", "out_in", plan(views=(edit(OKV, dst=A + 100), edit(OKV, src=C, dst=D), edit(OKV, src=C + 4096, dst=D + 5)))),
    ("out_in", "fits32", plan(views=(edit(OKV, dst=A, src_pitch=1 << 25, dst_pitch=1 << 25),))),
    ("fits32", "tail", plan(views=(edit(TAIL, dst_pitch=1 << 25),))),
    ("info_inconsistent", "d_plan_null", launch(damage=dict(plan_bytes=1), d_plan=None)),
    ("d_plan_aligned", "lut_null", launch(d_plan=D + 4, lut=None)),
    ("lut_null", "levels_range", launch(lut=None, levels=40)),
    ("levels_range", "interp", launch(levels=32, interp=-1)),
    ("interp", "levels_launch", launch(interp=7, levels=0)),
    ("d_plan_aligned", "levels_range", launch(fn="decode", d_plan=D + 4, levels=32)),      # (the decode entry has no table)
]
INFEASIBLE = {("info_null", "info_inconsistent"): "a NULL info has no field to be inconsistent",
              ("d_plan_null", "d_plan_aligned"): "NULL is aligned"}
EXTRAS = [
    ("null_argument", "h_plan", plan(h_plan=None)),
    ("null_argument", "info", plan(info=None)),
    ("null_entry", "dst", plan(views=(edit(OKV, dst=0),))),
    ("out_out", "different pitches", plan(views=(OKV, edit(OKV, src=C, dst=B + 100, dst_pitch=56)))),
    ("out_out", "side by side is fine, one column further is not", plan(views=(edit(OKV, dst_pitch=64), edit(OKV, src=C, dst=B + 31, dst_pitch=64)))),
    ("out_in", "in place", plan(views=(edit(OKV, dst=A, dst_pitch=40),))),
    ("out_in", "different pitches", plan(views=(OKV, edit(OKV, src=B + 10, src_pitch=41, dst=C)))),
    ("fits32", "source side", plan(views=(edit(OKV, src_pitch=1 << 25),))),
    ("fits32", "pitch 2^32", plan(views=(edit(OKV, src_pitch=1 << 32),))),
    ("tail", "one byte earlier", plan(views=(edit(TAIL, src=TAIL[0] - 1),))),
    ("info_inconsistent", "block count", launch(damage=dict(edge_tiles=0, interior_tiles=0))),
    ("info_inconsistent", "offset", launch(damage=dict(edge_prefix_offset=0))),
    ("info_inconsistent", "decode", launch(fn="decode", damage=dict(reserved=1))),
    ("levels_launch", "levels 0", launch(levels=0)),
    ("levels_launch", "decode, levels 31", launch(fn="decode", levels=31)),
]


def fail_statements(path):
    """The `fail(HGI_..., "...", ...)` statements of a source file in order: [(status name, [string literals])]."""
    src = open(path).read()
    found = []
    for m in re.finditer(r"\bfail\(\s*(HGI_\w+)\s*,", src):
        i, depth, lits = m.end(), 1, []
        while depth:
            c = src[i]
            if c == '"':
                j = i + 1
                while src[j] != '"':
                    j += 2 if src[j] == "\\" else 1
                lits.append(src[i + 1:j])
                i = j
            elif c == "(":
                depth += 1
            elif c == ")":
                depth -= 1
            i += 1
        found.append((m.group(1), lits))
    return found


def format_regex(fmt):
    out = ""
    for part in re.split(r"(%zu|%llu|%u|%d|%s)", fmt):
        out += {"%zu": r"\d+", "%llu": r"\d+", "%u": r"\d+", "%d": r"-?\d+", "%s": r".*"}.get(part, re.escape(part))
    return re.compile("^" + out + "$", re.S)


def main():
    import test_views
    from rustyhgi_amd import _ffi
    status_of = {"HGI_EINVAL": _ffi.EINVAL, "HGI_EUNSUPPORTED": _ffi.EUNSUPPORTED}
    stmts = [(s[0], [f for f in s[1] if " " in f]) for s in fail_statements(os.path.join(ROOT, "rustyhgi_amd", "views", "hgi_views.hip"))
             if s[0] != "HGI_EDEVICE"]      # (one-word literals are arguments of a format, not formats)
    assert stmts[-1][1] == ["unknown verdict"], stmts[-1]      # the default of the verdict switch: no argument reaches it
    del stmts[-1]
    # source order: the launch entries' judge stands in front of the plan entry
    judge = [s for s in stmts if any(k in " ".join(s[1]) for k in ("info is", "d_plan", "lut is NULL", "levels %u", "interpolator"))]
    ordered = [s for s in stmts if s not in judge] + judge
    assert len(ordered) == len(RULES), (len(ordered), len(RULES))
    index = dict((k, i) for i, (k, _) in enumerate(RULES))
    assert set((a, b) for a, b, _ in PAIRS) | set(INFEASIBLE) >= set(
        (x[0], y[0]) for x, y in zip(RULES, RULES[1:]) if (x[1]["fn"] == "plan") == (y[1]["fn"] == "plan")), "an adjacent pair is missing"
    entries, matched = [], set()

    def record(kind, rule, other, note, call):
        st, text = test_views.replay(call)
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
        json.dump(dict(comment="recorded by tests/golden/make_views_refusals.py; replayed by tests/test_views.py",
                       pointers="plain numbers (null: NULL); lut: ramp = the identity table, 256 host bytes", calls=entries), fh, indent=1)
        fh.write("\n")
    print("%d refused calls -> %s" % (len(entries), OUT))


if __name__ == "__main__":
    main()
