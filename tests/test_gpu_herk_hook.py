"""-m gpu: hipblas{C,Z}herk under LD_PRELOAD (tests/cpp/test_hook_herk.cpp, compiled here): emulated calls equal the direct
gemmul8_herk bit for bit, leave the other triangle alone and store +0.0 over a NaN on the diagonal's imaginary parts; the FP8 backend and
k > 2^17 reach the native routine (exact small-integer answer) with the log line; GEMMUL8_HOOK_STATS counts the HERK calls on a line of its own.
The program runs as a child process under a time limit, and a test stops at its first non-zero status."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_hook_herk.cpp")
LIB = os.path.join(ROOT, "gemmul8_amd", "lib", "libgemmul8.so")
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hook_herk") / "test_hook_herk")
    subprocess.run([HIPCC, "-std=c++20", "-O2", "-Wno-unused-value", "-x", "hip", "--offload-arch=gfx950", SRC, "-o", out, "-lhipblas", "-ldl"], check=True)
    return out


def run(args, env_extra):
    env = dict(os.environ)
    env.pop("GEMMUL8_MIN_FLOPS", None)
    env.update({"GEMMUL8_NUM_MOD_Z": "15", "GEMMUL8_NUM_MOD_C": "8", "GEMMUL8_HOOK_STATS": "1"})
    env.update(env_extra)
    env["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    # the preload is set for the program alone: `timeout` does not carry the HIP runtime the library binds to
    p = subprocess.run(["timeout", "-k", "10", "120", "env", "LD_PRELOAD=" + LIB] + args, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(p.stdout)
    assert p.returncode == 0 and "ALL OK" in p.stdout, (p.returncode, p.stdout[-2000:])
    return p.stdout


def test_hooked_herk_equals_the_direct_call(exe):
    out = run([exe, "emu"], {})
    assert "bitwise" in out
    assert "stats: emulated 4 HERK calls" in out and "native 0 HERK calls" in out, out[-2000:]
    assert "SYRK calls" not in out   # the SYRK line is printed only when a SYRK was seen


def test_fp8_backend_reaches_the_native_routine(exe):
    out = run([exe, "native", "64"], {"GEMMUL8_BACKEND": "1"})
    assert "passed to the native routine" in out and "HERK is emulated on the INT8 backend" in out
    assert "stats: emulated 0 HERK calls" in out and "native 2 HERK calls" in out, out[-2000:]


def test_k_beyond_the_range_reaches_the_native_routine(exe):
    out = run([exe, "native", str((1 << 17) + 8)], {})
    assert "passed to the native routine" in out and "HERK is emulated on the INT8 backend" in out
    assert "stats: emulated 0 HERK calls" in out and "native 2 HERK calls" in out, out[-2000:]


def test_ieee_nonfinite_mode_reaches_the_native_routine(exe):
    """GEMMUL8_NONFINITE=ieee promises BLAS-like NaN / Inf propagation and gemmul8_herk has no such mode: the hook leaves HERK to the native routine (exact
    small-integer answer), says so once and counts the calls as native"""
    out = run([exe, "native", "64"], {"GEMMUL8_NONFINITE": "ieee"})
    assert "passed to the native routine" in out and out.count("GEMMUL8_NONFINITE=ieee: HERK has no NaN / Inf propagation mode and is NOT emulated") == 1
    assert "stats: emulated 0 HERK calls" in out and "native 2 HERK calls" in out, out[-2000:]
