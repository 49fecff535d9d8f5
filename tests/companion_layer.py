"""What the CPU suites of the four companion libraries (test_recon.py, test_mapped.py, test_typed.py, test_requant.py) check in
common about their sources and their build, and the steps they all take: a companion's directory, rustyhgi_amd/companion/,
which all four include, and the launch layer of rustyhgi_amd/csrc/ under it.  `name` is recon, map, typed or requant throughout."""
import importlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

COMPANION_DIR = os.path.join(ROOT, "rustyhgi_amd", "companion")
COMPANION_FILES = ["companion.mk", "hgi_entry.h", "hgi_sides.h", "hgi_tile.h"]
CSRC_DIR = os.path.join(ROOT, "rustyhgi_amd", "csrc")
LAUNCH_FILES = ["hgi_launch.h", "hgi_launch_policy.h", "hgi_dec_chain.h"]      # what hgi_tile.h takes from csrc/ beside the tile procedure
KERNEL_UNIT = {"recon": "hgi_fused_recon_enc.hip", "map": "hgi_fused_map_dec.hip", "typed": "hgi_fused_typed_enc.hip",
               "requant": "hgi_fused_requant.hip"}
ENC_LDS = "(size_t)buf_bytes(nh) + ((rbuf_bytes(nh) + 15) & ~15) + 256"      # the uniform encoder's dynamic LDS, nothing added


def unit_dir(name):
    return os.path.join(ROOT, "rustyhgi_amd", name)


def binding(name):
    """The ctypes binding of a library, with the library built first if it is missing."""
    mod = importlib.import_module("rustyhgi_amd._ffi_" + name)
    if not os.path.exists(mod.LIB_PATH):
        subprocess.check_call(["make", "-s", "-C", unit_dir(name), "-j4", "all"])
    mod.lib()
    return mod


def header(name):
    """include/hgi_<name>.h without its comments."""
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hgi_%s.h" % name)).read(), flags=re.S)


def page_aligned(n):
    raw = np.zeros(n + 8192, np.uint8)
    off = (-raw.ctypes.data) % 4096
    return raw, raw.ctypes.data + off


def check_sources(directory, listing=None):
    """Stateless and switch-free sources: no environment read, no tuning switch, no device allocation, no ctx -- in every file
    of `directory` and of the shared layer; and exactly the files expected, where a listing is given."""
    for d, want in ((directory, listing), (COMPANION_DIR, COMPANION_FILES)):
        files = sorted(f for f in os.listdir(d) if os.path.isfile(os.path.join(d, f)))
        if want is not None:
            assert files == sorted(want), (d, files)
        for fn in files:
            src = open(os.path.join(d, fn)).read()
            assert "getenv" not in src and "KNOBS_ENV" not in src and "HGI_KNOB(" not in src, (d, fn)
            assert "hipMalloc" not in src and "hgi_ctx" not in src, (d, fn)      # no device allocation, no ctx
    # the shared headers name no switch either (the `strings` check of each library sees what they compile to)
    for d, fn in [(COMPANION_DIR, f) for f in ("hgi_entry.h", "hgi_sides.h", "hgi_tile.h")] + [(CSRC_DIR, f) for f in LAUNCH_FILES]:
        assert not re.search(r'"[^"\n]*HGI_[A-Z0-9_]+[^"\n]*"', open(os.path.join(d, fn)).read()), fn


def makefile(directory, name, fused):
    """The text make reads for a companion: its Makefile -- NAME, the direction's FUSED unit and the include, nothing else --
    followed by companion.mk with the two variables expanded."""
    mk = open(os.path.join(directory, "Makefile")).read()
    code = [l.strip() for l in mk.splitlines() if l.strip() and not l.startswith("#")]
    assert code == ["NAME := " + name, "FUSED := " + fused, "include ../companion/companion.mk"], code
    shared = open(os.path.join(COMPANION_DIR, "companion.mk")).read()
    assert len(re.findall(r"\$\(CSRC\)/hgi_fused_impl\.h", shared)) == 1, "the tile procedure's dependency list stands once"
    assert len(re.findall(r"\$\(COMPANION\)/hgi_tile\.h", shared)) == 1, "the kernel units depend on the shared tile layer"
    return mk + shared.replace("$(NAME)", name).replace("$(FUSED)", fused)


def unit_source(name, fused):
    """The text of a kernel unit, after what all four have in common: the direction's tile procedure included without its
    launchers, the shared tile layer behind it, and the launch through the launch layer that header includes from csrc/ --
    launch_tile_kernel makes the static-LDS check of hgi_launch.h once per instantiation.  An encoder-side unit takes its dynamic
    LDS from enc_lds_bytes, where the uniform encoder's formula stands once."""
    src = open(os.path.join(unit_dir(name), KERNEL_UNIT[name])).read()
    assert '#include "../csrc/%s"' % fused in src and '#include "../csrc/hgi_fused_pitched.h"' in src
    assert "#define HGI_FUSED_NO_LAUNCHERS 1" in src
    assert src.index("hgi_fused_pitched.h") < src.index('#include "../companion/hgi_tile.h"')
    assert "launch_tile_kernel<" in src and "hipLaunchKernelGGL" not in src and "#define" not in src[src.index("\nhipError_t launch_"):]
    tile = open(os.path.join(COMPANION_DIR, "hgi_tile.h")).read()
    launch = open(os.path.join(CSRC_DIR, "hgi_launch.h")).read()
    assert '#include "hgi_entry.h"' in tile and '#include "../csrc/hgi_launch.h"' in tile
    assert "static_lds_is_empty(reinterpret_cast" in launch
    assert "hipFuncGetAttributes" in launch and "sharedSizeBytes == 0" in launch
    assert launch.count(ENC_LDS) == 1 and ENC_LDS not in src and ENC_LDS not in tile
    if fused == "hgi_fused_enc.hip":
        assert "enc_lds_bytes(t.nh)" in src
    return src


def check_rule_order(name, entry, launcher):
    """hgi_<name>.hip: in the entry point no HIP call stands before the launch, the launch stands behind the last refusal, the
    empty call is decided first and every HGI_EINVAL rule stands before the first HGI_EUNSUPPORTED one."""
    src = open(os.path.join(unit_dir(name), "hgi_%s.hip" % name)).read()
    body = src[src.index("hgi_status %s(" % entry):src.index("const char *hgi_%s_last_error" % name)]
    first_hip = min(m.start() for m in re.finditer(r"\bhip[A-Z]\w*\s*\(|%s\s*\(" % launcher, body))
    assert body[first_hip:].startswith(launcher + "(")
    assert "return fail(HGI_EINVAL" not in body[first_hip:] and "return fail(HGI_EUNSUPPORTED" not in body[first_hip:]
    assert body.index("return HGI_OK;") < body.index("return fail(")
    assert max(m.start() for m in re.finditer(r"fail\(HGI_EINVAL", body)) < min(m.start() for m in re.finditer(r"fail\(HGI_EUNSUPPORTED", body))


def isa(name, tmp_path):
    """The device-only listing of a kernel unit for gfx950."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = str(tmp_path / KERNEL_UNIT[name].replace(".hip", ".s"))
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S",
                           os.path.join(unit_dir(name), KERNEL_UNIT[name]), "-o", out], stderr=subprocess.DEVNULL)
    return out


def resources(text, kernel):
    """{mangled name: (VGPRs, static LDS bytes, scratch bytes)} of the kernels of a listing whose name holds `kernel`."""
    res = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s*(\d+).*?\.name:\s*(\S+).*?\.private_segment_fixed_size:\s*(\d+).*?\.vgpr_count:\s*(\d+)",
                         text, flags=re.S):
        if kernel in m.group(2):
            res[m.group(2)] = (int(m.group(4)), int(m.group(1)), int(m.group(3)))
    return res


def run_plan_program(name, tmp_path, flags=()):
    """tests/cpp/test_<name>_plan.cpp, a stand-alone program, under ASan / UBSan: 1500 random cases, none may fail."""
    exe = str(tmp_path / ("test_%s_plan" % name))
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", *flags, "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "cpp", "test_%s_plan.cpp" % name), "-o", exe])
    p = subprocess.run([exe, "1500", "0x48474939"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "1500 cases, 0 failures" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]


def check_build_entry(name, after=None):
    """build() makes the library (behind that of `after`, where given) and git ignores its objects."""
    src = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert '"rustyhgi_amd", "%s"' % name in src
    if after:
        assert src.index('"rustyhgi_amd", "%s"' % after) < src.index('"rustyhgi_amd", "%s"' % name)
    assert "rustyhgi_amd/%s/_obj*/" % name in open(os.path.join(ROOT, ".gitignore")).read()
