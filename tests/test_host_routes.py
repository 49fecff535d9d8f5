"""The host layer behind include/hgi.h on the CPU, under ASan + UBSan, against the oracle (profiles/r16_host_routes.md).

csrc/hgi_capi.hip is compiled UNCHANGED with plain g++ against tests/cpp/hostsim/hip/hip_runtime.h and linked with a simulated
runtime (hostsim.cpp: exact-size poisoned device blocks, streams as FIFOs run under eager / awaited-last / awaited-first /
seeded random schedules, 2-D copies held to the host-span rule of DESIGN.md 4.14), reference launches for every launch_* of
csrc/hgi_kernels.h (sim_kernels.cpp, on the level restatement of ref_levels.h) and the oracle.  The program
(test_host_routes.cpp) has a main of its own; nothing is preloaded.  Its groups run as separate processes -- the knobs are read
once per process -- a few at a time.

The mutants are textual substitutions on a temporary copy of hgi_capi.hip, each of which must make the program fail; a
pattern that no longer occurs exactly once fails the test."""
import os
import subprocess
import time
from concurrent.futures import ThreadPoolExecutor

import pytest

from conftest import ROOT

SIM = os.path.join(ROOT, "tests", "cpp", "hostsim")
CAPI = os.path.join(ROOT, "rustyhgi_amd", "csrc", "hgi_capi.hip")
FLAGS = ["-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
         "-DHGI_KNOBS_ENV", "-I", SIM]
SAN_ENV = {"ASAN_OPTIONS": "detect_leaks=0:abort_on_error=1:halt_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}
KNOBS = ("HGI_TILE_H", "HGI_NO_BANDS", "HGI_TEST_BAND_HOLD", "HGI_NO_LATTICE_KERNEL", "HGI_FORCE_CHECKED", "HGI_LATTICE_MAX",
         "HGI_TILE16_MAX", "HGI_ENC_L1_TILE_ROWS")

# (id, arguments, knobs)
RUNS = [(g, [g], {}) for g in ("selfcheck", "host", "dev", "lists", "batch", "scratch", "refusals")]
RUNS += [("%s-tile%d" % (g, th), [g], {"HGI_TILE_H": str(th)}) for th in (16, 32, 64) for g in ("host", "dev")]
RUNS += [("%s-no_lattice_kernel" % g, [g], {"HGI_NO_LATTICE_KERNEL": "1"}) for g in ("host", "dev", "scratch")]
RUNS += [("lists-force_checked", ["lists"], {"HGI_FORCE_CHECKED": "1"})]
RUNS += [("banded%d" % i, ["banded", str(i)], {}) for i in range(5)]
RUNS += [("banded%d-band_hold" % i, ["banded", str(i)], {"HGI_TEST_BAND_HOLD": "1"}) for i in range(5)]
RUNS += [("banded%d-no_bands" % i, ["banded", str(i)], {"HGI_NO_BANDS": "1"}) for i in range(5)]

# (id, pattern, replacement, the group that has to notice)
MUTANTS = [
    ("r12_upload_restored",
     "HIP_TRY(hipMemcpy(d_in, rows.data(), cn, hipMemcpyHostToDevice));",
     "HIP_TRY(hipMemcpy2DAsync(d_in, w, grid, (size_t)w << shift, w, sh, hipMemcpyHostToDevice, c->stream));", ["host"]),
    ("banded_without_wait_on_ev_band",
     "hipError_t r = hipStreamWaitEvent(down, c->ev_band[b], 0);", "hipError_t r = hipSuccess;", ["banded", "1"]),
    ("batch_without_wait_on_ev_free",
     "if (j >= (size_t)kSlots) e = hipStreamWaitEvent(up, c->ev_free[sl], 0);", "", ["batch"]),
    ("ws_need_encode_two_planes",
     "return 3 * plane_bytes(g, batch) + ws_need_encode(", "return 2 * plane_bytes(g, batch) + ws_need_encode(", ["dev"]),
    ("list_ring_without_wait_on_ev_list",
     "HIP_TRY(hipEventSynchronize(c->ev_list[i]));", "", ["lists"]),
    ("banded_upload_with_64_halo_rows",
     "constexpr size_t kHaloRows = 65;", "constexpr size_t kHaloRows = 64;", ["banded", "0"]),
    ("pitched_download_as_one_rectangle",
     "HIP_TRY(copy_host_rows(out, out_pitch, d_out, w, w, h, hipMemcpyDeviceToHost, c->stream));",
     "HIP_TRY(hipMemcpy2DAsync(out, out_pitch, d_out, w, w, h, hipMemcpyDeviceToHost, c->stream));", ["host"]),
    ("levelwise_copy_past_the_last_frame",
     "HIP_TRY(launch_copy(img, rec, (batch - 1) * stride + (size_t)w * h, c->stream));",
     "HIP_TRY(launch_copy(img, rec, batch * stride, c->stream));", ["dev"]),
]


def _compile(src, obj, lang):
    cc = ["gcc", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if lang == "c" else ["g++"] + FLAGS + ["-x", "c++"]
    return subprocess.Popen(cc + ["-c", src, "-o", obj], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def _link(objs, exe):
    subprocess.check_call(["g++", "-fsanitize=address,undefined"] + objs + ["-lpthread", "-o", exe])


def _run(exe, args, knobs):
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(SAN_ENV)
    env.update(knobs)
    t0 = time.time()
    try:
        p = subprocess.run([exe] + args, env=env, capture_output=True, text=True, timeout=600)
        return p.returncode, p.stdout, p.stderr, time.time() - t0
    except subprocess.TimeoutExpired as e:
        return -1, (e.stdout or b"").decode(errors="replace"), "timed out after 600 s", time.time() - t0


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    """Builds the program, then runs every group and every mutant, a few processes at a time."""
    d = str(tmp_path_factory.mktemp("hostsim"))
    t0 = time.time()
    units = [(CAPI, "capi.o", "c++"), (os.path.join(SIM, "hostsim.cpp"), "hostsim.o", "c++"), (os.path.join(SIM, "sim_kernels.cpp"), "simk.o", "c++"),
             (os.path.join(SIM, "test_host_routes.cpp"), "test.o", "c++"), (os.path.join(ROOT, "oracle", "hgi_oracle.c"), "oracle.o", "c")]
    procs = [(src, _compile(src, os.path.join(d, obj), lang)) for src, obj, lang in units]
    source = open(CAPI).read()
    mutants = {}
    for name, pattern, replacement, args in MUTANTS:
        n = source.count(pattern)
        if n != 1:
            mutants[name] = ("stale", "the pattern %r occurs %d times in hgi_capi.hip, not once" % (pattern, n))
            continue
        path = os.path.join(d, name + ".hip")
        with open(path, "w") as f:
            f.write(source.replace(pattern, replacement))
        # (the copy includes the library's headers by name)
        procs.append((path, subprocess.Popen(["g++"] + FLAGS + ["-I", os.path.dirname(CAPI), "-x", "c++", "-c", path, "-o", os.path.join(d, name + ".o")],
                                             stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    for src, p in procs:
        out = p.communicate()[0]
        assert p.returncode == 0, "compiling %s failed:\n%s" % (src, out[-4000:])
    common = [os.path.join(d, o) for o in ("hostsim.o", "simk.o", "test.o", "oracle.o")]
    exe = os.path.join(d, "test_host_routes")
    _link([os.path.join(d, "capi.o")] + common, exe)
    jobs = [("run:" + rid, exe, args, knobs) for rid, args, knobs in RUNS]
    for name, _, _, args in MUTANTS:
        if name in mutants:
            continue
        mexe = os.path.join(d, name)
        _link([os.path.join(d, name + ".o")] + common, mexe)
        jobs.append(("mutant:" + name, mexe, args, {}))
    built = time.time() - t0
    jobs.sort(key=lambda j: 0 if "banded2" in j[0] else 1 if "banded3" in j[0] or "batch" in j[0] else 2)      # the longest first
    with ThreadPoolExecutor(max_workers=max(2, min(8, os.cpu_count() or 2))) as pool:
        results = dict(zip([j[0] for j in jobs], pool.map(lambda j: _run(j[1], j[2], j[3]), jobs)))
    for name, v in mutants.items():
        results["mutant:" + name] = v
    print("\nhost routes: built in %.0f s, %d processes in %.0f s wall" % (built, len(jobs), time.time() - t0 - built))
    for key in sorted(results):
        if key.startswith("run:"):
            rc, out, err, secs = results[key]
            census = [l for l in out.splitlines() if l.startswith(("census", "banded ", "batch ", "scratch:", "refusals:", "selfcheck:"))]
            print("  %-28s rc %d  %5.1f s  %s" % (key[4:], rc, secs, census[-1] if census else ""))
    return results


@pytest.mark.parametrize("rid", [r[0] for r in RUNS])
def test_group(harness, rid):
    rc, out, err, secs = harness["run:" + rid]
    assert rc == 0 and "host routes ok" in out, out[-3000:] + err[-4000:]
    assert "FINDING" not in out and "FAIL" not in out, out[-3000:]
    assert "runtime error" not in err and "AddressSanitizer" not in err and "LeakSanitizer" not in err, err[-4000:]


@pytest.mark.parametrize("name", [m[0] for m in MUTANTS])
def test_mutant_is_killed(harness, name):
    r = harness["mutant:" + name]
    assert r[0] != "stale", r[1]
    rc, out, err, secs = r
    evidence = [l for l in (out + err).splitlines() if l.startswith(("FINDING", "FAIL", "hostsim:")) or "AddressSanitizer" in l]
    print("\nmutant %s: rc %d in %.1f s; %s" % (name, rc, secs, evidence[0] if evidence else "no evidence line"))
    assert rc not in (0, -1) and evidence, "the mutant %s survived:\n%s" % (name, out[-2000:] + err[-2000:])
