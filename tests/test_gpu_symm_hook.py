"""-m gpu: hipblasDsymm / hipblasZhemm through the hook, with the program (tests/cpp/test_hook_symm.cpp, compiled here) LINKED against libgemmul8.so in
front of hipBLAS -- the link-time integration of INTEGRATION.md; nothing is preloaded.  Emulated calls, one `_64` twin each, equal the direct gemmul8_symm /
gemmul8_hemm bit for bit; the FP8 backend and GEMMUL8_NONFINITE=ieee reach the native routine (exact small-integer answer) and say so once; a numeric
GEMMUL8_MIN_FLOPS is a floor on 2 m n ka; GEMMUL8_HOOK_STATS prints a SYMM and a HEMM line only for routines that were seen."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_hook_symm.cpp")
LIBDIR = os.path.join(ROOT, "gemmul8_amd", "lib")
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hook_symm") / "test_hook_symm")
    subprocess.run([HIPCC, "-std=c++20", "-O2", "-Wno-unused-value", "-x", "hip", "--offload-arch=gfx950", SRC, "-o", out, "-L" + LIBDIR,
                    "-Wl,-rpath," + LIBDIR, "-lgemmul8", "-lhipblas"], check=True)
    return out


def run(cmd, env_extra):
    env = dict(os.environ)
    for name in ("GEMMUL8_MIN_FLOPS", "LD_PRELOAD", "GEMMUL8_BACKEND", "GEMMUL8_NONFINITE"):
        env.pop(name, None)
    env.update({"GEMMUL8_NUM_MOD_D": "15", "GEMMUL8_NUM_MOD_Z": "14", "GEMMUL8_HOOK_STATS": "1"})
    env.update(env_extra)
    env["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    assert "LD_PRELOAD" not in env
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    print(p.stdout)
    assert p.returncode == 0 and "ALL OK" in p.stdout, p.stdout[-2000:]
    return p.stdout


def test_hooked_symm_and_hemm_equal_the_direct_calls(exe):
    out = run([exe, "emu"], {})
    assert "bitwise" in out
    assert "stats: emulated 2 SYMM calls" in out and "native 0 SYMM calls" in out, out[-2000:]
    assert "stats: emulated 2 HEMM calls" in out and "native 0 HEMM calls" in out, out[-2000:]
    assert "SYRK calls" not in out and "HERK calls" not in out and "SYR2K calls" not in out   # a routine that was not seen has no line


def test_stats_lines_only_for_routines_seen(exe):
    out = run([exe, "exact", "d"], {})
    assert "stats: emulated 1 SYMM calls" in out and "HEMM calls" not in out, out[-2000:]
    out = run([exe, "exact", "z"], {})
    assert "stats: emulated 1 HEMM calls" in out and "SYMM calls" not in out, out[-2000:]


def test_fp8_backend_reaches_the_native_routine(exe):
    out = run([exe, "exact", "dz"], {"GEMMUL8_BACKEND": "1"})
    assert "exact small-integer result" in out
    assert out.count("SYMM is emulated on the INT8 backend") == 1 and out.count("HEMM is emulated on the INT8 backend") == 1, out[-2000:]
    assert "stats: emulated 0 SYMM calls" in out and "native 1 SYMM calls" in out and "emulated 0 HEMM calls" in out and "native 1 HEMM calls" in out, out[-2000:]


def test_ieee_nonfinite_mode_reaches_the_native_routine(exe):
    """GEMMUL8_NONFINITE=ieee promises BLAS-like NaN / Inf propagation and gemmul8_symm / gemmul8_hemm have no such mode"""
    out = run([exe, "exact", "dz"], {"GEMMUL8_NONFINITE": "ieee"})
    assert "exact small-integer result" in out
    for name in ("SYMM", "HEMM"):
        assert out.count(f"GEMMUL8_NONFINITE=ieee: {name} has no NaN / Inf propagation mode and is NOT emulated") == 1, out[-2000:]
    assert "stats: emulated 0 SYMM calls" in out and "native 1 SYMM calls" in out and "emulated 0 HEMM calls" in out and "native 1 HEMM calls" in out, out[-2000:]


def test_floor_on_2_m_n_ka(exe):
    """GEMMUL8_MIN_FLOPS as a number is a floor on 2 m n ka: the program's 2 * 8 * 8 * 8 = 1024 is below 1025 -> native, said once per routine; a floor of
    exactly 1024 is met -> emulated.  The answer is the exact one either way."""
    out = run([exe, "exact", "dz"], {"GEMMUL8_MIN_FLOPS": "1025"})
    assert "native 1 SYMM calls" in out and "native 1 HEMM calls" in out and "emulated 0 SYMM calls" in out and "emulated 0 HEMM calls" in out, out[-2000:]
    assert out.count("DSYMM m = 8, n = 8, order of A = 8") == 1 and out.count("ZHEMM m = 8, n = 8, order of A = 8") == 1, out[-2000:]
    assert out.count("stays on the native routine") == 2
    out = run([exe, "exact", "dz"], {"GEMMUL8_MIN_FLOPS": "1024"})
    assert "emulated 1 SYMM calls" in out and "emulated 1 HEMM calls" in out and "stays on the native routine" not in out, out[-2000:]
