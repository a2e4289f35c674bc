"""-m gpu: hipblas{C,Z}her2k under LD_PRELOAD (tests/cpp/test_hook_her2k.cpp, compiled here): emulated calls -- both entry points, the _64 forms, host and
device pointer mode -- equal the direct gemmul8_her2k bit for bit and leave the other triangle alone; the FP8 backend, k > 2^17 and
GEMMUL8_NONFINITE=ieee reach the native routine (exact small-integer answer) and say so once; a numeric GEMMUL8_MIN_FLOPS is a floor on 8 n (n + 1) k;
GEMMUL8_HOOK_STATS counts the HER2K calls on a line of its own."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_hook_her2k.cpp")
LIB = os.path.join(ROOT, "gemmul8_amd", "lib", "libgemmul8.so")
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hook_her2k") / "test_hook_her2k")
    subprocess.run([HIPCC, "-std=c++20", "-O2", "-Wno-unused-value", "-x", "hip", "--offload-arch=gfx950", SRC, "-o", out, "-lhipblas", "-ldl"], check=True)
    return out


def run(cmd, env_extra):
    env = dict(os.environ)
    env.pop("GEMMUL8_MIN_FLOPS", None)
    env.update({"LD_PRELOAD": LIB, "GEMMUL8_NUM_MOD_Z": "15", "GEMMUL8_NUM_MOD_C": "8", "GEMMUL8_HOOK_STATS": "1"})
    env.update(env_extra)
    env["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    print(p.stdout)
    assert p.returncode == 0 and "ALL OK" in p.stdout, p.stdout[-2000:]
    return p.stdout


def test_hooked_her2k_equals_the_direct_call_in_both_pointer_modes(exe):
    out = run([exe, "emu"], {})
    assert "bitwise" in out
    assert "stats: emulated 6 HER2K calls" in out and "native 0 HER2K calls" in out, out[-2000:]
    assert "SYRK calls" not in out and "HERK calls" not in out and "SYR2K calls" not in out   # a routine that was not seen has no line


def test_fp8_backend_reaches_the_native_routine(exe):
    out = run([exe, "native", "64"], {"GEMMUL8_BACKEND": "1"})
    assert "passed to the native routine" in out and out.count("HER2K is emulated on the INT8 backend") == 1
    assert "stats: emulated 0 HER2K calls" in out and "native 2 HER2K calls" in out, out[-2000:]


def test_k_beyond_the_range_reaches_the_native_routine(exe):
    out = run([exe, "native", str((1 << 17) + 8)], {})
    assert "passed to the native routine" in out and out.count("HER2K is emulated on the INT8 backend for k <= 131072 only") == 1
    assert "stats: emulated 0 HER2K calls" in out and "native 2 HER2K calls" in out, out[-2000:]


def test_floor_on_8_n_n1_k(exe):
    """GEMMUL8_MIN_FLOPS as a number is a floor on 8 n (n + 1) k: 8 * 8 * 9 * 64 = 36864 is below 37000 -> native, exact, and said once; the emulated
    program's 8 * 300 * 301 * 200 = 144480000 meets a floor of exactly that -> all six calls emulated"""
    out = run([exe, "native", "64"], {"GEMMUL8_MIN_FLOPS": "37000"})
    assert "native 2 HER2K calls" in out and out.count("HER2K n = 8, k = 64") == 1 and "stays on the native routine" in out, out[-2000:]
    assert "no HER2K scan has been fitted" in out
    out = run([exe, "emu"], {"GEMMUL8_MIN_FLOPS": "144480000"})
    assert "emulated 6 HER2K calls" in out and "stays on the native routine" not in out, out[-2000:]


def test_ieee_nonfinite_mode_reaches_the_native_routine(exe):
    """GEMMUL8_NONFINITE=ieee promises BLAS-like NaN / Inf propagation and gemmul8_her2k has no such mode: the hook leaves HER2K to the native routine (exact
    small-integer answer), says so once and counts the calls as native"""
    out = run([exe, "native", "64"], {"GEMMUL8_NONFINITE": "ieee"})
    assert "passed to the native routine" in out and out.count("GEMMUL8_NONFINITE=ieee: HER2K has no NaN / Inf propagation mode and is NOT emulated") == 1
    assert "stats: emulated 0 HER2K calls" in out and "native 2 HER2K calls" in out, out[-2000:]
