"""-m gpu: hipblas{S,D,C,Z}trsm through the hook, with the program (tests/cpp/test_hook_trsm.cpp, compiled here) LINKED against libgemmul8.so in front of
hipBLAS -- the link-time integration of INTEGRATION.md; nothing is preloaded.  Emulated calls of all four types and one `_64` twin, in place on B, equal
the direct gemmul8_trsm bit for bit; the FP8 backend, GEMMUL8_NONFINITE=ieee and a moduli count out of range reach the native routine (exact
small-integer answer) and say so once; a numeric GEMMUL8_MIN_FLOPS is a floor on m n ka and `auto` declines below the measured order; GEMMUL8_HOOK_STATS
prints a TRSM line only when such a call was seen."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_hook_trsm.cpp")
SYMM_SRC = os.path.join(ROOT, "tests", "cpp", "test_hook_symm.cpp")
LIBDIR = os.path.join(ROOT, "gemmul8_amd", "lib")
HIPCC = "/opt/rocm/bin/hipcc"


def _build(tmp, src, name):
    out = str(tmp / name)
    subprocess.run([HIPCC, "-std=c++20", "-O2", "-Wno-unused-value", "-x", "hip", "--offload-arch=gfx950", src, "-o", out, "-L" + LIBDIR,
                    "-Wl,-rpath," + LIBDIR, "-lgemmul8", "-lhipblas"], check=True)
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("hook_trsm"), SRC, "test_hook_trsm")


def run(cmd, env_extra):
    env = dict(os.environ)
    for name in ("GEMMUL8_MIN_FLOPS", "LD_PRELOAD", "GEMMUL8_BACKEND", "GEMMUL8_NONFINITE"):
        env.pop(name, None)
    env.update({"GEMMUL8_NUM_MOD_S": "7", "GEMMUL8_NUM_MOD_D": "15", "GEMMUL8_NUM_MOD_C": "8", "GEMMUL8_NUM_MOD_Z": "14", "GEMMUL8_HOOK_STATS": "1"})
    env.update(env_extra)
    env["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    assert "LD_PRELOAD" not in env
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    print(p.stdout)
    assert p.returncode == 0 and "ALL OK" in p.stdout, p.stdout[-2000:]
    return p.stdout


def test_hooked_trsm_equals_the_direct_call_for_every_type(exe):
    out = run([exe, "emu"], {})
    assert "bitwise" in out
    assert "stats: emulated 5 TRSM calls" in out and "native 0 TRSM calls" in out, out[-2000:]
    assert "SYMM calls" not in out and "HEMM calls" not in out and "SYRK calls" not in out   # a routine that was not seen has no line


def test_every_type_is_emulated_and_exact(exe):
    out = run([exe, "exact", "sdcz"], {})
    assert "stats: emulated 4 TRSM calls" in out and "native 0 TRSM calls" in out, out[-2000:]


def test_no_trsm_line_when_no_trsm_call_was_seen(tmp_path):
    """the SYMM program of the suite calls no TRSM"""
    out = run([_build(tmp_path, SYMM_SRC, "test_hook_symm"), "exact", "d"], {})
    assert "stats: emulated 1 SYMM calls" in out and "TRSM calls" not in out, out[-2000:]


def test_fp8_backend_reaches_the_native_routine(exe):
    out = run([exe, "exact", "dz"], {"GEMMUL8_BACKEND": "1"})
    assert "exact small-integer result" in out
    assert out.count("TRSM is emulated on the INT8 backend") == 1, out[-2000:]
    assert "stats: emulated 0 TRSM calls" in out and "native 2 TRSM calls" in out, out[-2000:]


def test_ieee_nonfinite_mode_reaches_the_native_routine(exe):
    """GEMMUL8_NONFINITE=ieee promises BLAS-like NaN / Inf propagation and gemmul8_trsm has no such mode"""
    out = run([exe, "exact", "sc"], {"GEMMUL8_NONFINITE": "ieee"})
    assert "exact small-integer result" in out
    assert out.count("GEMMUL8_NONFINITE=ieee: TRSM has no NaN / Inf propagation mode and is NOT emulated") == 1, out[-2000:]
    assert "stats: emulated 0 TRSM calls" in out and "native 2 TRSM calls" in out, out[-2000:]


def test_moduli_count_out_of_range_reaches_the_native_routine(exe):
    out = run([exe, "exact", "sd"], {"GEMMUL8_NUM_MOD_S": "14"})
    assert out.count("GEMMUL8_NUM_MOD_S=14 is outside 2..13: STRSM calls use the native routine") == 1, out[-2000:]
    assert "stats: emulated 1 TRSM calls" in out and "native 1 TRSM calls" in out, out[-2000:]


def test_floor_on_m_n_ka(exe):
    """GEMMUL8_MIN_FLOPS as a number is a floor on m n ka, the routine's own flop count: the program's 8 * 8 * 8 = 512 is below 513 -> native, said once; a
    floor of exactly 512 is met -> emulated.  The answer is the exact one either way."""
    out = run([exe, "exact", "dz"], {"GEMMUL8_MIN_FLOPS": "513"})
    assert "native 2 TRSM calls" in out and "emulated 0 TRSM calls" in out, out[-2000:]
    assert out.count("DTRSM m = 8, n = 8, order of A = 8") == 1 and out.count("stays on the native routine") == 1, out[-2000:]
    out = run([exe, "exact", "dz"], {"GEMMUL8_MIN_FLOPS": "512"})
    assert "emulated 2 TRSM calls" in out and "stays on the native routine" not in out, out[-2000:]


def test_auto_declines_an_order_below_the_measured_crossover(exe):
    """GEMMUL8_MIN_FLOPS=auto: an order of 8 is below any order at which the emulated routine was measured to win (profiles/trsm_ab.json)"""
    out = run([exe, "exact", "sd"], {"GEMMUL8_MIN_FLOPS": "auto"})
    assert "native 2 TRSM calls" in out and "emulated 0 TRSM calls" in out, out[-2000:]
    assert out.count("stays on the native routine") == 1, out[-2000:]
