#!/usr/bin/env python3
"""Generates tests/golden/companion_refusals.json: the status and the full *_last_error() text of a fixed list of refused calls
to the four companion libraries (libhgi_recon.so, libhgi_map.so, libhgi_typed.so, libhgi_requant.so), recorded from the
libraries built in this tree.  tests/test_companion.py replays the list and asserts status and text, so that neither a
message nor the order in which the rules are decided can drift unseen.

A refused call touches no buffer and reaches no launch: pointers are plain numbers, `lut` alone is a real 256-byte host array
(requantize reads it for its identity rule).  No device is needed.

The list is built from the `rules` of LIBS below: one entry per `return fail(...)` statement of an entry point, IN SOURCE ORDER, with the
arguments that break that rule alone.  From it come
  * one call per rule (`solo`);
  * one call per adjacent pair of rules that breaks both (`pair`): the earlier rule's text is what gets recorded;
  * the extra calls of EXTRAS (a second message of one statement, further ways into a rule).
Before anything is written the generator checks itself against the sources: the statements found in hgi_<lib>.hip are as many
as the rules listed, each solo call's text matches a format string of ITS statement, each pair's text matches the earlier
statement, every format string outside the HGI_EDEVICE statement is matched by some recorded text, and no call returns HGI_OK.
Two kinds of exception are written down here and checked to be exactly these:
  * UNREACHABLE: "the call does not take the buffer path" stands behind the 32-bit rule and the tail rule in every entry
    point, and pitched_plan's `fast` is false only when one of the two fails -- the statement is a guard that no argument
    reaches;
  * INFEASIBLE pairs: two rules that no single call can break together.
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

OUT = os.path.join(HERE, "companion_refusals.json")

# plain numbers, page aligned, 2^50 apart: no shape below spans that much
A, B, C, D = 1 << 50, 2 << 50, 3 << 50, 4 << 50
BIG = dict(batch=(1 << 31) - 1)                    # with a 2^34 stride on one side: a call that spans more than 2^64 bytes
TILES = dict(w=128 << 16, h=64 << 15, batch=1)     # 65536 x 32768 tiles of one frame: more than a launch holds

LIBS = {
    "recon": dict(
        fn="hgi_recon_encode_u8_dev", err="hgi_recon_last_error",
        args=["stream", "img", "ip", "w", "h", "levels", "interp", "lut", "grid", "gp", "rec", "rp", "batch", "ifs", "gfs", "rfs"],
        base=dict(stream=None, img=A, ip=40, w=32, h=8, levels=2, interp=1, lut="ramp", grid=B, gp=48, rec=C, rp=36, batch=2,
                  ifs=320, gfs=384, rfs=300),
        rules=[
            ("levels_range", dict(levels=32)),
            ("interp", dict(interp=7)),
            ("lut_null", dict(lut=None)),
            ("levels_launch", dict(levels=9)),
            ("null_buffer", dict(img=None)),
            ("img_pitch", dict(ip=31)),
            ("grid_pitch", dict(gp=31)),
            ("recon_pitch", dict(rp=31)),
            ("batch", dict(batch=1 << 31)),
            ("img_stride", dict(ifs=311)),
            ("grid_stride", dict(gfs=367)),
            ("recon_stride", dict(rfs=283)),
            ("span_size", dict(BIG, ifs=1 << 34)),
            ("in_place", dict(rec=A)),
            ("grid_on_img", dict(grid=A + 100)),
            ("recon_on_img", dict(rec=A + 100)),
            ("recon_on_grid", dict(rec=B + 10)),
            ("tiles", dict(TILES, ip=1 << 23, gp=1 << 23, rp=1 << 23)),
            ("fits32", dict(gp=1 << 25, batch=1)),
            ("tail", dict(w=30, batch=1, img=A + 4096 - (7 * 40 + 30))),
            ("not_fast", None),
        ],
        pairs={
            ("in_place", "grid_on_img"): dict(rec=A, grid=A + 1),
            ("grid_on_img", "recon_on_img"): dict(grid=A + 100, rec=A + 200),
            ("recon_on_img", "recon_on_grid"): dict(rec=A + 600, grid=A + 700),      # the image ends at A + 632
            ("fits32", "tail"): dict(gp=1 << 25, w=30, batch=1, img=A + 4096 - (7 * 40 + 30)),
        },
        infeasible={},
        extras=[
            ("levels_launch", "levels 0", dict(levels=0)),
            ("null_buffer", "grid", dict(grid=None)),
            ("null_buffer", "recon", dict(rec=None)),
            ("span_size", "one frame", dict(batch=1, h=(1 << 32) - 1, ip=1 << 63)),
            ("fits32", "pitch 2^32", dict(rp=1 << 32, batch=1)),
        ]),
    "map": dict(
        fn="hgi_map_decode_dev", err="hgi_map_last_error",
        args=["stream", "grid", "gp", "w", "h", "levels", "interp", "table", "elem", "out", "op", "batch", "gfs", "ofs"],
        base=dict(stream=None, grid=B, gp=40, w=32, h=8, levels=2, interp=1, table=D, elem=2, out=A, op=72, batch=2, gfs=320, ofs=600),
        rules=[
            ("levels_range", dict(levels=32)),
            ("interp", dict(interp=7)),
            ("elem_size", dict(elem=3)),
            ("null_buffer", dict(grid=None)),
            ("out_aligned", dict(out=A + 1)),
            ("out_pitch_elems", dict(op=73)),
            ("out_stride_elems", dict(ofs=601)),
            ("grid_pitch", dict(gp=31)),
            ("out_pitch", dict(op=62)),
            ("batch", dict(batch=1 << 31)),
            ("grid_stride", dict(gfs=311)),
            ("out_stride", dict(ofs=566)),
            ("span_size", dict(BIG, gfs=1 << 34)),
            ("table_on_out", dict(table=A + 10)),
            ("table_on_grid", dict(table=B + 10)),
            ("out_on_grid", dict(out=B + 10)),
            ("tiles", dict(TILES, gp=1 << 23, op=1 << 24)),
            ("levels_launch", dict(levels=9)),
            ("fits32", dict(op=1 << 25, batch=1)),
            ("tail", dict(w=30, batch=1, grid=B + 4096 - (7 * 40 + 30))),
            ("not_fast", None),
        ],
        pairs={
            ("table_on_out", "table_on_grid"): dict(table=A + 10, grid=A + 300),
            ("table_on_grid", "out_on_grid"): dict(table=B - 500, out=B + 100),      # the table ends at B + 12
        },
        infeasible={},
        extras=[
            ("elem_size", "elem 8", dict(elem=8, op=256)),
            ("null_buffer", "table", dict(table=None)),
            ("null_buffer", "out", dict(out=None)),
            ("out_aligned", "elem 4", dict(out=A + 2, elem=4, op=128, ofs=1100)),
            ("levels_launch", "levels 0", dict(levels=0)),
            ("fits32", "grid side", dict(gp=1 << 25, batch=1)),
        ]),
    "typed": dict(
        fn="hgi_typed_encode_dev", err="hgi_typed_last_error",
        args=["stream", "img", "ip", "elem", "kind", "scale", "bias", "w", "h", "levels", "interp", "lut", "grid", "gp", "batch", "ifs", "gfs"],
        base=dict(stream=None, img=A, ip=72, elem=2, kind=0, scale=255.0, bias=0.0, w=32, h=8, levels=2, interp=1, lut="ramp", grid=B,
                  gp=40, batch=2, ifs=600, gfs=320),
        rules=[
            ("lut_null", dict(lut=None)),
            ("null_buffer", dict(img=None)),
            ("levels_range", dict(levels=32)),
            ("elem_size", dict(elem=3)),
            ("elem_kind", dict(kind=2)),
            ("bf16_size", dict(kind=1, elem=4, ip=128, ifs=1100)),
            ("finite", dict(scale="nan")),
            ("img_aligned", dict(img=A + 1)),
            ("img_pitch_elems", dict(ip=73)),
            ("img_stride_elems", dict(ifs=601)),
            ("img_pitch", dict(ip=62)),
            ("grid_pitch", dict(gp=31)),
            ("batch", dict(batch=1 << 31)),
            ("img_stride", dict(ifs=564)),
            ("grid_stride", dict(gfs=311)),
            ("span_size", dict(BIG, ifs=1 << 34)),
            ("grid_on_img", dict(grid=A + 100)),
            ("tiles", dict(TILES, gp=1 << 23, ip=1 << 24)),
            ("levels_launch", dict(levels=9)),
            ("fits32", dict(gp=1 << 25, batch=1)),
            ("interp", dict(interp=7)),
            ("tail", dict(w=31, batch=1, img=A + 4096 - (7 * 72 + 62))),
            ("not_fast", None),
        ],
        pairs={},
        infeasible={("elem_kind", "bf16_size"): "elem_kind > 1 and elem_kind == 1 exclude one another"},
        extras=[
            ("null_buffer", "grid", dict(grid=None)),
            ("finite", "bias inf", dict(bias="inf")),
            ("img_aligned", "elem 4", dict(img=A + 2, elem=4, ip=128, ifs=1100)),
            ("levels_launch", "levels 0", dict(levels=0)),
            ("fits32", "image side", dict(ip=1 << 25, batch=1)),
            ("interp", "negative", dict(interp=-1)),
            ("tail", "bfloat16", dict(w=31, batch=1, kind=1, img=A + 4096 - (7 * 72 + 62))),
        ]),
    "requant": dict(
        fn="hgi_requant_dev", err="hgi_requant_last_error",
        args=["stream", "src", "sp", "w", "h", "levels", "interp", "lut", "dst", "dp", "batch", "sfs", "dfs"],
        base=dict(stream=None, src=A, sp=40, w=32, h=8, levels=2, interp=1, lut="inverted", dst=B, dp=48, batch=2, sfs=320, dfs=384),
        rules=[
            ("lut_null", dict(lut=None)),
            ("null_buffer", dict(src=None)),
            ("levels_range", dict(levels=32)),
            ("src_pitch", dict(sp=31)),
            ("dst_pitch", dict(dp=31)),
            ("batch", dict(batch=1 << 31)),
            ("src_stride", dict(sfs=311)),
            ("dst_stride", dict(dfs=367)),
            ("span_size", dict(BIG, sfs=1 << 34)),
            ("overlap", dict(dst=A + 100)),
            ("tiles", dict(TILES, sp=1 << 23, dp=1 << 23)),
            ("levels_launch", dict(levels=9)),
            ("interp", dict(interp=7)),
            ("fits32", dict(dp=1 << 25, batch=1)),
            ("tail", dict(w=30, batch=1, src=A + 4096 - (7 * 40 + 30))),
            ("not_fast", None),
            ("identity", dict(lut="ramp")),
        ],
        pairs={("tail", "identity"): dict(w=30, batch=1, src=A + 4096 - (7 * 40 + 30), lut="ramp")},      # across the guard
        infeasible={},
        extras=[
            ("null_buffer", "dst", dict(dst=None)),
            ("overlap", "in place", dict(dst=A)),
            ("levels_launch", "levels 0", dict(levels=0)),
            ("fits32", "source side", dict(sp=1 << 25, batch=1)),
        ]),
}
UNREACHABLE = "not_fast"


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
    """A printf format of the entry points (%u, %zu, %d, %s) as a regular expression over the whole text."""
    out = ""
    for part in re.split(r"(%zu|%u|%d|%s)", fmt):
        out += {"%zu": r"\d+", "%u": r"\d+", "%d": r"-?\d+", "%s": r".*"}.get(part, re.escape(part))
    return re.compile("^" + out + "$", re.S)


def luts():
    import numpy as np
    ramp = np.arange(256, dtype=np.uint8)
    return {"ramp": ramp, "inverted": (255 - ramp).astype(np.uint8)}


def run(lib, spec, values, tables):
    """One call: (status, text).  `values`: the full argument dict of a fixture entry."""
    argv = []
    for name in spec["args"]:
        v = values[name]
        if name == "lut" and v is not None:
            v = tables[v].ctypes.data
        elif name in ("scale", "bias"):
            v = float(v)
        argv.append(v)
    st = getattr(lib, spec["fn"])(*argv)
    return st, getattr(lib, spec["err"])().decode("utf-8")


def main():
    import importlib
    tables = luts()
    from rustyhgi_amd import _ffi
    status_of = {"HGI_EINVAL": _ffi.EINVAL, "HGI_EUNSUPPORTED": _ffi.EUNSUPPORTED}
    entries = []
    for name, spec in LIBS.items():
        lib = importlib.import_module("rustyhgi_amd._ffi_" + name).lib()
        stmts = [s for s in fail_statements(os.path.join(ROOT, "rustyhgi_amd", name, "hgi_%s.hip" % name)) if s[0] != "HGI_EDEVICE"]
        rules = spec["rules"]
        assert len(stmts) == len(rules), (name, len(stmts), len(rules))
        index = dict((key, i) for i, (key, _) in enumerate(rules))
        matched = set()

        def record(kind, rule, other, note, over):
            merged = dict(spec["base"], **over)
            values = dict((k, merged[k]) for k in spec["args"])
            st, text = run(lib, spec, values, tables)
            want_st, fmts = stmts[index[rule]]
            hit = [f for f in fmts if format_regex(f).match(text)]
            assert st == status_of[want_st] and hit, (name, kind, rule, other, st, text)
            matched.update((index[rule], f) for f in hit)
            entries.append(dict(lib=name, fn=spec["fn"], kind=kind, rule=rule, also_breaks=other, note=note, args=values, status=st, error=text))

        for key, over in rules:
            if over is None:
                assert key == UNREACHABLE, key
                continue
            record("solo", key, None, "", over)
        reach = [(k, o) for k, o in rules if o is not None]
        for (ka, oa), (kb, ob) in zip(reach, reach[1:]):
            if (ka, kb) in spec["infeasible"]:
                continue
            both = spec["pairs"].get((ka, kb), dict(ob, **oa))
            record("pair", ka, kb, "", both)
        assert set(spec["pairs"]) <= set(zip((k for k, _ in reach), (k for k, _ in reach[1:]))), name
        for key, note, over in spec["extras"]:
            record("extra", key, None, note, over)
        unmatched = [(i, f) for i, (_, fmts) in enumerate(stmts) for f in fmts if (i, f) not in matched]
        assert [rules[i][0] for i, _ in unmatched] == [UNREACHABLE], (name, unmatched)
    assert all(e["status"] != 0 for e in entries)
    with open(OUT, "w") as fh:
        json.dump(dict(comment="recorded by tests/golden/make_companion_refusals.py; replayed by tests/test_companion.py",
                       pointers="plain numbers (null: NULL); lut: the name of a 256-byte host table (ramp: i, inverted: 255 - i); "
                                "scale / bias: numbers or the strings nan / inf",
                       calls=entries), fh, indent=1)
        fh.write("\n")
    print("%d refused calls -> %s" % (len(entries), OUT))


if __name__ == "__main__":
    main()
