"""Source facts of the one launch layer (rustyhgi_amd/csrc/hgi_launch.h, hgi_launch_policy.h): the eight tile
launchers of the core library go through it as the companions' do (tests/companion_layer.py:unit_source), and what it holds
stands once across both trees.  What the layer picks on the device: tests/test_launch_gpu.py; the policy's values:
tests/cpp/test_launch_policy.cpp (tests/test_sanitizers.py)."""
import os
import re

from conftest import ROOT

PKG = os.path.join(ROOT, "rustyhgi_amd")
CSRC = os.path.join(PKG, "csrc")
# unit -> its tile launchers
LAUNCHERS = {"hgi_fused_impl.h": ["HGI_TILED(launch_decode_fused)", "HGI_TILED(launch_encode_fused)"],
             "hgi_fused_region.hip": ["launch_decode_region"], "hgi_fused_scaled.hip": ["launch_decode_scaled"],
             "hgi_fused_list_dec.hip": ["launch_decode_list"], "hgi_fused_list_enc.hip": ["launch_encode_list"],
             "hgi_fused_pitched_dec.hip": ["launch_decode_pitched"], "hgi_fused_pitched_enc.hip": ["launch_encode_pitched"]}
ENC_LDS = "buf_bytes(nh) + ((rbuf_bytes(nh) + 15) & ~15) + 256"


def sources():
    """{path: text} of every C++ / HIP file of the package."""
    out = {}
    for d, _, files in os.walk(PKG):
        if "_obj" in d:
            continue
        for fn in files:
            if fn.endswith((".h", ".hip")):
                out[os.path.join(d, fn)] = open(os.path.join(d, fn)).read()
    return out


def function(src, name):
    """The text of the function `hipError_t <name>(...)`: from its first line to the closing brace in column 0."""
    at = src.index("\nhipError_t %s(" % name)
    return src[at:src.index("\n}\n", at) + 3]


def test_every_core_tile_launcher_goes_through_the_launch_layer():
    assert sum(len(v) for v in LAUNCHERS.values()) == 8
    for unit, names in LAUNCHERS.items():
        src = open(os.path.join(CSRC, unit)).read()
        first = src.index("\nhipError_t HGI_TILED(launch_" if unit == "hgi_fused_impl.h" else "\nhipError_t launch_")
        assert "#define" not in src[first:], unit
        for name in names:
            body = function(src, name)
            assert "hipLaunchKernelGGL" not in body and "hipFuncGetAttributes" not in body, name
            assert body.count("return with_choices(") == 1 and body.count("launch_tile_kernel<k_") == 1, name
            assert "interp_choice(interp)" in body, name
            assert "rbuf_bytes" not in body and not re.search(r"HGI_DEC_\w*WAVES|8192|65536", body), name      # no LDS formula, no policy
            if "_decode_" in name or "decode_fused" in name:
                assert body.count("dec_resident_tiles(") == 1 and "lds_for_waves((size_t)buf_bytes(nh), " in body, name
            else:
                assert "lds_for_waves(enc_lds_bytes(nh), HGI_KNOB(HGI_ENC_WAVES, 0))" in body, name
    # the placement probe's number stands in front of the policy (hgi_planes.hip)
    assert "resident_tiles >= 0 ? resident_tiles : dec_resident_tiles(" in open(os.path.join(CSRC, "hgi_fused_impl.h")).read()
    # the 64-row-only seed planes: an `if constexpr` inside the lambda, in both directions
    assert open(os.path.join(CSRC, "hgi_fused_impl.h")).read().count("if constexpr (SE == 1 && TH != 64) return hipErrorInvalidValue;") == 2


def test_what_the_layer_holds_stands_once():
    src = sources()
    where = lambda text: sorted(os.path.relpath(p, PKG) for p, s in src.items() if text in s)      # noqa: E731
    assert where(ENC_LDS) == ["csrc/hgi_launch.h"] and src[os.path.join(CSRC, "hgi_launch.h")].count(ENC_LDS) == 1
    assert where("hipFuncGetAttributes(&") == ["csrc/hgi_launch.h"]      # the static-LDS check has one body
    assert where("sharedSizeBytes") == ["csrc/hgi_launch.h"]
    assert where("hipError_t with_choices(") == ["csrc/hgi_launch.h"] and where("hipError_t launch_tile_kernel(") == ["csrc/hgi_launch.h"]
    assert where("void dec_chain(") == ["csrc/hgi_dec_chain.h"] and where("void dec_fine_rows(") == ["csrc/hgi_fused_impl.h"]
    # the policy: its numbers are defined in one header and named in one function
    policy = src[os.path.join(CSRC, "hgi_launch_policy.h")]
    for name in ("HGI_DEC_SHALLOW_WAVES", "HGI_DEC_DEEP_WAVES", "HGI_DEC_STREAM_WAVES", "HGI_DEC_STREAM_WAVES_WIDE", "HGI_DEC_STREAM_WAVES_L1"):
        assert where("#define %s " % name) == ["csrc/hgi_launch_policy.h"], name
        assert re.search(r"#ifndef %s\n#define %s \d+ " % (name, name), policy), name      # a -D on the command line still wins
        code = {p: [l for l in s.splitlines() if re.search(r"\b%s\b" % name, l.split("//")[0]) and not l.startswith("#")] for p, s in src.items()}
        assert sorted(os.path.relpath(p, PKG) for p, ls in code.items() if ls) == ["csrc/hgi_launch_policy.h"], name
    rule = policy[policy.index("inline int dec_resident_tiles("):]
    rule = rule[:rule.index("\n}\n")]
    named = [l for l in policy.splitlines() if "HGI_DEC_STREAM_WAVES_WIDE" in l.split("//")[0] and not l.startswith("#")]
    assert len(named) == 1 and named[0] in rule
    assert rule.index("HGI_KNOB(HGI_DEC_WAVES, -1)") < rule.index("tiles < 8192") < rule.index("!seeded") < rule.index("65536")
    assert where("tiles < 8192") == ["csrc/hgi_launch_policy.h"]
    # plain C++: no HIP name in the policy header
    assert not re.search(r"\bhip[A-Z_]\w*|__device__|__global__", policy)


def test_the_makefiles_know_the_new_headers():
    for mk, prefix in (("csrc/Makefile", ""), ("companion/companion.mk", "$(CSRC)/")):
        text = open(os.path.join(PKG, mk)).read()
        rule = [l for l in text.splitlines() if l.startswith("$(OBJ)/%.o:")]
        assert len(rule) == 1
        for h in ("hgi_launch_policy.h", "hgi_launch.h", "hgi_dec_chain.h"):
            assert prefix + h in rule[0].split(), (mk, h)
