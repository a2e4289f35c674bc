"""The Level-3 gates of the LD_PRELOAD hook (hipblas?syrk / herk / syr2k / her2k / symm / hemm / trmm / trsm and the _64 twins) characterised on the CPU:
gemmul8_amd/csrc/oz2_hook.cpp, the mocks of tests/sanitize (mock_gpu.cpp, mock_level3.cpp) and tests/sanitize/level3_driver.cpp are built with the
compiler, flags and ASan + UBSan options of test_sanitizers.py::test_hook_under_asan_ubsan and linked into stand-alone programs; every scenario of the
driver runs in a process of its own, and what it prints -- each call, where it went (the native stub or the C ABI entry, with every scalar argument),
the hook's notices and its statistics -- is compared byte for byte with tests/golden/hook_level3_transcript.json.

The golden file was recorded with this harness from the hook as it stood BEFORE its four Level-3 gates were folded into one (try_level3): it is the
proof that the fold changed no decision, no argument, no workspace size, no notice and no count.  It maps each scenario to the lines of its transcript,
one string a line, so that a change of the hook that changes a notice on purpose shows in the file's diff line by line."""
import json
import os
import subprocess

import pytest

from test_sanitizers import FLAGS, ROOT, SAN, _run

SCENARIOS = ["all", "unselected", "moduli-range", "fp8", "limit", "ieee", "floor-number", "floor-auto", "declined", "failed", "screens", "no-entry"]
GOLDEN = os.path.join(ROOT, "tests", "golden", "hook_level3_transcript.json")


def build(d):
    """The hook, the two mocks (mock_level3.cpp also without the C ABI entries) and the driver linked against either, in directory d."""
    clang = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(clang):
        pytest.skip("ROCm clang++ not available")
    common = [clang, "-std=c++20", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-fPIC", "-Wno-unused-value", "-Wno-deprecated-declarations"]
    lib = lambda name: os.path.join(d, "lib" + name + ".so")
    _run(common + ["-O1", "-shared", os.path.join(SAN, "mock_gpu.cpp"), "-o", lib("mockgpu")])
    _run(common + FLAGS + ["-shared", os.path.join(ROOT, "gemmul8_amd", "csrc", "oz2_hook.cpp"), "-o", lib("hook_san"), "-ldl", "-lpthread"])
    _run(common + FLAGS + ["-shared", os.path.join(SAN, "mock_level3.cpp"), "-o", lib("mocklevel3"), "-ldl"])
    _run(common + FLAGS + ["-shared", "-DMOCK_LEVEL3_NATIVES_ONLY", os.path.join(SAN, "mock_level3.cpp"), "-o", lib("mocklevel3_natives"), "-ldl"])
    for exe, level3 in (("level3_driver", "-lmocklevel3"), ("level3_driver_natives", "-lmocklevel3_natives")):
        _run(common + FLAGS + [os.path.join(SAN, "level3_driver.cpp"), "-o", os.path.join(d, exe), "-L" + d, "-lhook_san", level3, "-lmockgpu",
                               "-Wl,-rpath," + d, "-lpthread"])


def transcript(d, scenario):
    """stdout and stderr of one scenario, merged in order (the driver's stdout is unbuffered)."""
    exe = os.path.join(d, "level3_driver_natives" if scenario == "no-entry" else "level3_driver")
    p = subprocess.run([exe, scenario], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1", LD_LIBRARY_PATH=d))
    assert p.returncode == 0, p.stdout[-4000:]
    return p.stdout


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("level3"))
    build(d)
    return d


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_covers_every_scenario(golden):
    assert sorted(golden) == sorted(SCENARIOS)


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_transcript(built, golden, scenario):
    got, w = transcript(built, scenario), golden[scenario]
    if got != "".join(line + "\n" for line in w):
        g = got.splitlines()
        first = next((i for i, (a, b) in enumerate(zip(g, w)) if a != b), min(len(g), len(w)))
        pytest.fail("scenario %s: the transcript differs from the recorded one at line %d (%d lines against %d)\n  recorded: %s\n  now:      %s"
                    % (scenario, first + 1, len(g), len(w), w[first] if first < len(w) else "<end>", g[first] if first < len(g) else "<end>"))
