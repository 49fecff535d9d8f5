"""What the four companion libraries share (rustyhgi_amd/companion/): the host rules of hgi_sides.h under ASan / UBSan (a
stand-alone program), and the refusals of the four entry points, replayed from tests/golden/companion_refusals.json: every recorded call returns
the recorded status and leaves the recorded *_last_error() text, character for character.  The list (tests/golden/
make_companion_refusals.py) holds one call per `fail(` statement of the four entry points that an argument can reach, and one
per adjacent pair of rules that breaks both, so both the messages and the order in which the rules are decided are pinned.
No call reaches a launch: pointers are plain numbers, and no device is needed."""
import importlib
import json
import os
import subprocess

import numpy as np
import pytest

import companion_layer as CL
from conftest import GOLDEN_DIR, ROOT

LIBS = ("recon", "map", "typed", "requant")

with open(os.path.join(GOLDEN_DIR, "companion_refusals.json")) as _f:
    CALLS = json.load(_f)["calls"]


@pytest.fixture(scope="module")
def libs():
    """The four bindings, each library built first if it is missing."""
    out = {}
    for name in LIBS:
        ffi = importlib.import_module("rustyhgi_amd._ffi_" + name)
        if not os.path.exists(ffi.LIB_PATH):
            subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "rustyhgi_amd", name), "-j4", "all"])
        out[name] = ffi
    return out


def test_the_list_covers_the_four_libraries():
    for name in LIBS:
        mine = [c for c in CALLS if c["lib"] == name]
        assert sum(c["kind"] == "solo" for c in mine) >= 15 and sum(c["kind"] == "pair" for c in mine) >= 14, name
    from rustyhgi_amd import _ffi
    assert all(c["status"] in (_ffi.EINVAL, _ffi.EUNSUPPORTED) for c in CALLS)      # refused before any device call


def test_every_recorded_refusal_repeats_its_status_and_text(libs):
    ramp = np.arange(256, dtype=np.uint8)
    tables = {"ramp": ramp, "inverted": (255 - ramp).astype(np.uint8)}
    frozen = dict((k, v.copy()) for k, v in tables.items())
    for c in CALLS:
        ffi = libs[c["lib"]]
        table = dict((s[0], s) for s in ffi.SYMBOLS)
        names = c["args"]
        assert len(names) == len(table[c["fn"]][2])
        argv = []
        for (key, v), ctype in zip(names.items(), table[c["fn"]][2]):
            if key == "lut" and v is not None:
                v = tables[v].ctypes.data
            elif key in ("scale", "bias"):
                v = float(v)
            argv.append(v)
        st = getattr(ffi.lib(), c["fn"])(*argv)
        text = ffi.last_error()
        where = "%s %s %s %s %s" % (c["lib"], c["kind"], c["rule"], c["also_breaks"] or "", c["note"])
        assert st == c["status"], (where, st, text)
        assert text == c["error"], (where, text)
    for k in tables:
        assert (tables[k] == frozen[k]).all()


def test_sides_under_asan_ubsan(tmp_path):
    """tests/cpp/test_sides.cpp, a stand-alone program: the byte intervals against brute force (rows of bytes and of 2- and
    4-byte elements, the table), the page rule at every byte in front of a page end for 2 and 3 tail bytes, the 32-bit bound at
    its boundary, the split of the pyramid -- once for the four libraries."""
    exe = str(tmp_path / "test_sides")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "cpp", "test_sides.cpp"), "-o", exe])
    p = subprocess.run([exe, "1500", "0x48474939"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "1500 cases, 0 failures" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]


def test_shared_layer_is_headers_and_a_make_fragment():
    """rustyhgi_amd/companion/ holds exactly its three files, no library of its own, and plain C++ where g++ must read it."""
    CL.check_sources(CL.COMPANION_DIR, CL.COMPANION_FILES)
    sides = open(os.path.join(CL.COMPANION_DIR, "hgi_sides.h")).read()
    assert "hip" not in sides.replace("../csrc/hgi_pitched.h", "").replace("csrc/hgi_capi.hip", "").replace("libhgi_hip.so", "")
    mk = open(os.path.join(CL.COMPANION_DIR, "companion.mk")).read()
    assert "libhgi_$(NAME)$(VARIANT).so" in mk and "-shared" in mk and "companion.so" not in mk
