"""-m gpu: the pointer-array batched GEMMs (hipblas{D,Z}gemmBatched, hipblasDgemmBatched_64, hipblasGemmBatchedEx, rocblas_dgemm_batched) through the
hook, with the program (tests/cpp/test_hook_batched_ptr.cpp, compiled here) LINKED against libgemmul8.so in front of hipBLAS and rocBLAS -- the
link-time integration of INTEGRATION.md; nothing is preloaded.  Emulated calls on 7 scattered items equal direct gemmul8_gemm calls per item bit for bit,
also when GEMMUL8_BATCH_WORKSPACE_MB cuts the batch into three chunks; GEMMUL8_BATCH_FUSED=0, a moduli count out of range and a call below a numeric
GEMMUL8_MIN_FLOPS reach the native routine (exact small-integer product) and say so once; with GEMMUL8_HOOK_ROCBLAS=1 the rocBLAS name is served, and a
call that enters at the hipBLAS name is counted once."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_hook_batched_ptr.cpp")
LIBDIR = os.path.join(ROOT, "gemmul8_amd", "lib")
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hook_batched_ptr") / "test_hook_batched_ptr")
    subprocess.run([HIPCC, "-std=c++20", "-O2", "-Wno-unused-value", "-x", "hip", "--offload-arch=gfx950", SRC, "-o", out, "-L" + LIBDIR,
                    "-Wl,-rpath," + LIBDIR, "-lgemmul8", "-lhipblas", "-lrocblas"], check=True)
    return out


def run(cmd, env_extra):
    env = dict(os.environ)
    for name in ("GEMMUL8_MIN_FLOPS", "LD_PRELOAD", "GEMMUL8_BACKEND", "GEMMUL8_NONFINITE", "GEMMUL8_BATCH_FUSED", "GEMMUL8_BATCH_WORKSPACE_MB", "GEMMUL8_DIST",
                 "GEMMUL8_HOOK_ROCBLAS"):
        env.pop(name, None)
    env.update({"GEMMUL8_NUM_MOD_S": "7", "GEMMUL8_NUM_MOD_D": "15", "GEMMUL8_NUM_MOD_C": "8", "GEMMUL8_NUM_MOD_Z": "14", "GEMMUL8_HOOK_STATS": "1"})
    env.update(env_extra)
    env["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    assert "LD_PRELOAD" not in env
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    print(p.stdout)
    assert p.returncode == 0 and "ALL OK" in p.stdout, p.stdout[-2000:]
    return p.stdout


def test_hooked_calls_equal_direct_calls_per_item(exe):
    out = run([exe, "emu"], {})
    assert "bitwise" in out
    assert "stats: emulated 4 GEMM calls" in out and "native 0 GEMM calls" in out, out[-2000:]
    assert "using the native routine" not in out


def test_three_workspace_chunks_give_the_same_bits(exe):
    out = run([exe, "chunks"], {})
    assert out.count("3 items per chunk") == 3 and "three chunks == direct" in out
    assert "stats: emulated 3 GEMM calls" in out and "native 0 GEMM calls" in out, out[-2000:]


def test_exact_product_is_emulated_by_default(exe):
    out = run([exe, "exact"], {})
    assert "exact small-integer result" in out
    assert "stats: emulated 2 GEMM calls" in out and "native 0 GEMM calls" in out, out[-2000:]


def test_unfused_batches_reach_the_native_routine(exe):
    """GEMMUL8_BATCH_FUSED=0 selects the stream lanes, which walk item addresses on the host: not for arrays in device memory"""
    out = run([exe, "exact"], {"GEMMUL8_BATCH_FUSED": "0"})
    assert "exact small-integer result" in out
    assert out.count("GEMMUL8_BATCH_FUSED=0: only the fused path can serve a pointer-array batch") == 1, out[-2000:]
    assert out.count("using the native routine") == 1
    assert "stats: emulated 0 GEMM calls" in out and "native 2 GEMM calls" in out, out[-2000:]


def test_moduli_count_out_of_range_reaches_the_native_routine(exe):
    out = run([exe, "exact"], {"GEMMUL8_NUM_MOD_D": "21"})
    assert "exact small-integer result" in out
    assert out.count("the moduli count of GEMMUL8_NUM_MOD_{S,D,C,Z} is outside the type's range (21)") == 1, out[-2000:]
    assert out.count("using the native routine") == 1
    assert "stats: emulated 0 GEMM calls" in out and "native 2 GEMM calls" in out, out[-2000:]


def test_call_below_a_numeric_floor_reaches_the_native_routine(exe):
    """2 m n k = 1024 per item: below 1025 -> native, said once by the floor; a floor of exactly 1024 is met -> emulated"""
    out = run([exe, "exact"], {"GEMMUL8_MIN_FLOPS": "1025"})
    assert "exact small-integer result" in out
    assert out.count("stays on the native routine") == 1 and "DGEMM 8 x 8 x 8 (batch 4" in out, out[-2000:]
    assert "stats: emulated 0 GEMM calls" in out and "native 2 GEMM calls" in out, out[-2000:]
    out = run([exe, "exact"], {"GEMMUL8_MIN_FLOPS": "1024"})
    assert "stats: emulated 2 GEMM calls" in out and "stays on the native routine" not in out, out[-2000:]


def test_rocblas_name_is_served_when_asked(exe):
    out = run([exe, "rocblas"], {"GEMMUL8_HOOK_ROCBLAS": "1"})
    assert "rocblas_dgemm_batched on 7 scattered items == direct" in out
    assert "stats: emulated 1 GEMM calls" in out and "native 0 GEMM calls" in out, out[-2000:]


def test_a_hipblas_call_is_counted_once_with_the_rocblas_names_hooked(exe):
    """emulated at the hipBLAS name: one call; declined there (GEMMUL8_BATCH_FUSED=0): the pass-through arrives at the rocBLAS name inside the native
    scope and is not counted again"""
    out = run([exe, "exact"], {"GEMMUL8_HOOK_ROCBLAS": "1"})
    assert "stats: emulated 2 GEMM calls" in out and "native 0 GEMM calls" in out, out[-2000:]
    out = run([exe, "exact"], {"GEMMUL8_HOOK_ROCBLAS": "1", "GEMMUL8_BATCH_FUSED": "0"})
    assert "exact small-integer result" in out
    assert "stats: emulated 0 GEMM calls" in out and "native 2 GEMM calls" in out, out[-2000:]
