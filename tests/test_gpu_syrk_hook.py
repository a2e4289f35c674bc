"""-m gpu: hipblas{S,D}syrk under LD_PRELOAD (tests/cpp/test_hook_syrk.cpp, compiled here): emulated calls equal the direct gemmul8_syrk bit for
bit and leave the other triangle alone; the FP8 backend and k > 2^17 reach the native routine (exact small-integer answer); GEMMUL8_HOOK_STATS
counts the SYRK calls."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_hook_syrk.cpp")
LIB = os.path.join(ROOT, "gemmul8_amd", "lib", "libgemmul8.so")
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hook_syrk") / "test_hook_syrk")
    subprocess.run([HIPCC, "-std=c++20", "-O2", "-Wno-unused-value", "-x", "hip", "--offload-arch=gfx950", SRC, "-o", out, "-lhipblas", "-ldl"], check=True)
    return out


def run(cmd, env_extra):
    env = dict(os.environ)
    env.pop("GEMMUL8_MIN_FLOPS", None)
    env.update({"LD_PRELOAD": LIB, "GEMMUL8_NUM_MOD_D": "15", "GEMMUL8_NUM_MOD_S": "8", "GEMMUL8_HOOK_STATS": "1"})
    env.update(env_extra)
    env["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    print(p.stdout)
    assert p.returncode == 0 and "ALL OK" in p.stdout, p.stdout[-2000:]
    return p.stdout


def test_hooked_syrk_equals_the_direct_call(exe):
    out = run([exe, "emu"], {})
    assert "bitwise" in out
    assert "stats: emulated 4 SYRK calls" in out and "native 0 SYRK calls" in out, out[-2000:]


def test_fp8_backend_reaches_the_native_routine(exe):
    out = run([exe, "native", "64"], {"GEMMUL8_BACKEND": "1"})
    assert "passed to the native routine" in out and "SYRK is emulated on the INT8 backend" in out
    assert "stats: emulated 0 SYRK calls" in out and "native 2 SYRK calls" in out, out[-2000:]


def test_k_beyond_the_range_reaches_the_native_routine(exe):
    out = run([exe, "native", str((1 << 17) + 8)], {})
    assert "passed to the native routine" in out
    assert "stats: emulated 0 SYRK calls" in out and "native 2 SYRK calls" in out, out[-2000:]


def test_floor_on_n_n1_k(exe):
    """GEMMUL8_MIN_FLOPS as a number is a floor on n (n + 1) k: 8 * 9 * 64 = 4608 is below 5000 -> native, exact"""
    out = run([exe, "native", "64"], {"GEMMUL8_MIN_FLOPS": "5000"})
    assert "native 2 SYRK calls" in out and "stays on the native routine" in out, out[-2000:]


def test_ieee_nonfinite_mode_reaches_the_native_routine(exe):
    """GEMMUL8_NONFINITE=ieee promises BLAS-like NaN / Inf propagation and gemmul8_syrk has no such mode: the hook leaves SYRK to the native routine (exact
    small-integer answer), says so once and counts the calls as native"""
    out = run([exe, "native", "64"], {"GEMMUL8_NONFINITE": "ieee"})
    assert "passed to the native routine" in out and out.count("GEMMUL8_NONFINITE=ieee: SYRK has no NaN / Inf propagation mode and is NOT emulated") == 1
    assert "stats: emulated 0 SYRK calls" in out and "native 2 SYRK calls" in out, out[-2000:]
