"""gemmul8_amd -- Python plumbing over the C ABI of libgemmul8.so (MI355X-native Ozaki-II GEMM emulation).

The product is the shared library (hand-written HIP for gfx950, gemmul8_amd/csrc) behind
include/gemmul8_c.h / include/gemmul8.hpp.  This package only (1) loads it with ctypes, (2) passes
torch device pointers / HIP streams through the C ABI, and (3) hosts the moduli-sharded multi-GPU
driver (gemmul8_amd.dist) on torch.distributed.  There is NO CPU fallback: if the library is missing
every entry point raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libgemmul8.so")

S, D, Cx, Z = 0, 1, 2, 3
INT8, FP8 = 0, 1
OPS = {"N": 0, "T": 1, "C": 2}
UPLO = {"L": 0, "U": 1}
SIDE = {"L": 0, "R": 1}
DIAG = {"N": 0, "U": 1}


class Layout(C.Structure):
    """Mirror of struct gemmul8_layout (include/gemmul8_c.h)."""
    _fields_ = [
        ("kp", C.c_size_t), ("mp", C.c_size_t), ("num_mat", C.c_size_t), ("parts", C.c_size_t),
        ("sizeA", C.c_size_t), ("sizeB", C.c_size_t), ("sizeC", C.c_size_t),
        ("A_lo", C.c_void_p), ("B_lo", C.c_void_p),
        ("part_strideA", C.c_size_t), ("part_strideB", C.c_size_t),
        ("A_bound", C.c_void_p), ("B_bound", C.c_void_p),
        ("sftA", C.c_void_p), ("sftB", C.c_void_p),
        ("C_mid", C.c_void_p), ("scratch", C.c_void_p), ("scratch_bytes", C.c_size_t),
        ("lo_format", C.c_size_t),
    ]


_lib = None

EXPORTS = ["gemmul8_version", "gemmul8_work_size", "gemmul8_gemm", "gemmul8_get_layout", "gemmul8_scale",
           "gemmul8_scale_bounds", "gemmul8_scale_finish", "gemmul8_lowprec_gemm", "gemmul8_crt", "gemmul8_set_fp8_bound_mode", "gemmul8_set_nonfinite_mode",
           "gemmul8_hook_would_emulate", "gemmul8_reload_knobs", "gemmul8_abi_version", "gemmul8_layout_bytes", "gemmul8_syrk", "gemmul8_herk", "gemmul8_syr2k",
           "gemmul8_symm", "gemmul8_hemm", "gemmul8_her2k", "gemmul8_trmm", "gemmul8_trsm", "gemmul8_trsm_work_size", "gemmul8_trsm_leaf",
           "gemmul8_gemm_batched_ptr"]

ABI_VERSION = 7  # GEMMUL8_ABI_VERSION of include/gemmul8_c.h this module's struct mirrors were written against


def _bind_hip_runtime():
    """libgemmul8.so carries no DT_NEEDED on the HIP runtime: it must bind to the SAME libamdhip64 the
    process already uses (PyTorch bundles its own copy; two runtimes do not share device pointers).
    Promote the loaded copy to RTLD_GLOBAL, or load the system one if none is mapped yet."""
    try:
        import torch  # noqa: F401  (maps torch/lib/libamdhip64.so)
    except Exception:
        pass
    path = None
    with open("/proc/self/maps") as f:
        for line in f:
            if "libamdhip64" in line:
                path = line.split()[-1]
                break
    if path is None:
        path = "/opt/rocm/lib/libamdhip64.so"
    C.CDLL(path, mode=C.RTLD_GLOBAL)
    return path


def lib():
    """Load libgemmul8.so (fails loudly if it has not been built: run __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} not found: the HIP extension is not built (python -c 'import __graft_entry__ as g; g.build()')")
    _bind_hip_runtime()
    _lib = bind(C.CDLL(LIB_PATH))
    return _lib


def bind(L):
    """Declare the C-ABI signatures (include/gemmul8_c.h) on a loaded library object: libgemmul8.so, or a laboratory build of it
    (tools/build_probes.sh, tools/experiments/) that a measurement script wants to drive through the same helpers."""
    L.gemmul8_version.restype = C.c_char_p
    L.gemmul8_abi_version.restype = C.c_int
    L.gemmul8_layout_bytes.restype = C.c_size_t
    if L.gemmul8_abi_version() != ABI_VERSION or L.gemmul8_layout_bytes() != C.sizeof(Layout):
        raise RuntimeError(f"libgemmul8.so has ABI version {L.gemmul8_abi_version()} / a {L.gemmul8_layout_bytes()}-byte gemmul8_layout; this module mirrors "
                           f"version {ABI_VERSION} / {C.sizeof(Layout)} bytes: rebuild the library (python -c 'import __graft_entry__ as g; g.build()')")
    L.gemmul8_work_size.restype = C.c_size_t
    L.gemmul8_work_size.argtypes = [C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, C.c_uint, C.c_int, C.c_int,
                                    C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.gemmul8_gemm.restype = C.c_int
    L.gemmul8_gemm.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_size_t,
                               C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                               C.c_size_t, C.c_uint, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                               C.c_int, C.c_int, C.POINTER(C.c_double)]
    L.gemmul8_get_layout.restype = C.c_int
    L.gemmul8_get_layout.argtypes = [C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, C.c_uint, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(Layout)]
    L.gemmul8_scale.restype = C.c_int
    L.gemmul8_scale.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_size_t,
                                C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_uint, C.c_int, C.c_uint, C.c_uint,
                                C.POINTER(Layout), C.c_int, C.c_int]
    L.gemmul8_scale_bounds.restype = C.c_int
    L.gemmul8_scale_bounds.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_size_t,
                                       C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_uint, C.c_size_t, C.c_size_t,
                                       C.POINTER(Layout), C.c_int, C.c_int]
    L.gemmul8_scale_finish.restype = C.c_int
    L.gemmul8_scale_finish.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_size_t,
                                       C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_uint, C.c_int, C.c_uint, C.c_uint,
                                       C.POINTER(Layout), C.c_int, C.c_int]
    L.gemmul8_lowprec_gemm.restype = C.c_int
    L.gemmul8_lowprec_gemm.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, C.c_uint,
                                       C.c_uint, C.c_uint, C.POINTER(Layout)]
    L.gemmul8_crt.restype = C.c_int
    L.gemmul8_crt.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_uint, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t,
                              C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    L.gemmul8_work_size_batched.restype = C.c_size_t
    L.gemmul8_work_size_batched.argtypes = [C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, C.c_uint, C.c_size_t]
    L.gemmul8_batched_item_bytes.restype = C.c_size_t
    L.gemmul8_batched_item_bytes.argtypes = [C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, C.c_uint]
    L.gemmul8_gemm_batched.restype = C.c_int
    L.gemmul8_gemm_batched.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p,
                                       C.c_void_p, C.c_size_t, C.c_longlong, C.c_void_p, C.c_size_t, C.c_longlong, C.c_void_p,
                                       C.c_void_p, C.c_size_t, C.c_longlong, C.c_size_t, C.c_uint, C.c_int, C.c_void_p]
    L.gemmul8_gemm_batched_ptr.restype = C.c_int
    L.gemmul8_gemm_batched_ptr.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p,
                                           C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_uint,
                                           C.c_int, C.c_void_p]
    L.gemmul8_syrk.restype = C.c_int
    L.gemmul8_syrk.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t,
                               C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint, C.c_int, C.c_void_p, C.POINTER(C.c_double)]
    L.gemmul8_herk.restype = C.c_int
    L.gemmul8_herk.argtypes = L.gemmul8_syrk.argtypes
    L.gemmul8_syr2k.restype = C.c_int
    L.gemmul8_syr2k.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint, C.c_int, C.c_void_p, C.POINTER(C.c_double)]
    L.gemmul8_her2k.restype = C.c_int
    L.gemmul8_her2k.argtypes = L.gemmul8_syr2k.argtypes
    L.gemmul8_symm.restype = C.c_int
    L.gemmul8_symm.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                               C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint, C.c_int, C.c_void_p, C.POINTER(C.c_double)]
    L.gemmul8_hemm.restype = C.c_int
    L.gemmul8_hemm.argtypes = L.gemmul8_symm.argtypes
    L.gemmul8_trmm.restype = C.c_int
    L.gemmul8_trmm.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t,
                               C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_uint, C.c_int, C.c_void_p, C.POINTER(C.c_double)]
    L.gemmul8_trsm.restype = C.c_int
    L.gemmul8_trsm.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t,
                               C.c_void_p, C.c_size_t, C.c_uint, C.c_int, C.c_void_p, C.POINTER(C.c_double)]
    L.gemmul8_trsm_work_size.restype = C.c_size_t
    L.gemmul8_trsm_work_size.argtypes = [C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_uint]
    L.gemmul8_trsm_leaf.restype = C.c_int
    L.gemmul8_trsm_leaf.argtypes = []
    L.gemmul8_set_fp8_bound_mode.restype = C.c_int
    L.gemmul8_set_fp8_bound_mode.argtypes = [C.c_int]
    L.gemmul8_set_nonfinite_mode.restype = C.c_int
    L.gemmul8_set_nonfinite_mode.argtypes = [C.c_int]
    L.gemmul8_hook_would_emulate.restype = C.c_int
    L.gemmul8_hook_would_emulate.argtypes = [C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, C.c_uint, C.c_int, C.c_size_t]
    L.gemmul8_reload_knobs.restype = None
    L.gemmul8_reload_knobs.argtypes = []
    L.gemmul8_add_f64.restype = C.c_int
    L.gemmul8_add_f64.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    L.gemmul8_add_row_bias.restype = C.c_int
    L.gemmul8_add_row_bias.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
    return L


NONFINITE_REFERENCE, NONFINITE_IEEE = 0, 1


def set_nonfinite_mode(mode):
    """Process-wide handling of NaN / Inf operands in gemm / gemm_batched (include/gemmul8_c.h, gemmul8_set_nonfinite_mode): 0 = the
    default (operands assumed finite), 1 = BLAS-like propagation ("ieee").  Returns the previous mode; anything else raises ValueError."""
    prev = lib().gemmul8_set_nonfinite_mode(int(mode))
    if prev < 0:
        raise ValueError(f"non-finite mode {mode!r}: 0 or 1")
    return prev


def work_size(is_complex, backend, m, n, k, num_moduli, enA=False, enB=False):
    wa, wb = C.c_size_t(0), C.c_size_t(0)
    tot = lib().gemmul8_work_size(int(is_complex), backend, m, n, k, num_moduli, int(enA), int(enB), C.byref(wa), C.byref(wb))
    return tot, wa.value, wb.value


def check(rc, what="gemmul8"):
    if rc != 0:
        raise RuntimeError(f"{what} failed with status {rc}")


def _dtype_code(t):
    import torch
    return {torch.float32: S, torch.float64: D, torch.complex64: Cx, torch.complex128: Z}[t]


def gemm(A, B, num_moduli, fastmode=False, backend=INT8, opA="N", opB="N", alpha=1.0, beta=0.0, C_out=None, work=None,
         timers=False, stream=None):
    """C = alpha*op(A)*op(B) + beta*C through the C ABI.

    A, B (and C_out) are COLUMN-MAJOR matrices held as torch tensors of shape (cols, rows) -- i.e. the
    tensor is the transpose view of the BLAS matrix, contiguous, so that `ld` = tensor.shape[1].
    Returns (C, timers_ns or None, work)."""
    import numpy as np
    import torch
    assert A.is_cuda and B.is_cuda and A.is_contiguous() and B.is_contiguous()
    dt = A.dtype
    if B.dtype != dt or (C_out is not None and (C_out.dtype != dt or not C_out.is_contiguous())):
        raise TypeError("A, B and C_out must share one dtype and be contiguous")
    lda, ldb = A.shape[1], B.shape[1]
    m, k = (lda, A.shape[0]) if opA == "N" else (A.shape[0], lda)
    kb, n = (ldb, B.shape[0]) if opB == "N" else (B.shape[0], ldb)
    assert k == kb, (k, kb)
    if C_out is None:
        C_out = torch.zeros((n, m), dtype=dt, device=A.device)
    if work is None:
        tot, _, _ = work_size(dt.is_complex, backend, m, n, k, num_moduli)
        work = torch.empty(tot, dtype=torch.uint8, device=A.device)
    np_dt = {torch.float32: np.float32, torch.float64: np.float64, torch.complex64: np.complex64, torch.complex128: np.complex128}[dt]
    al = np.array([alpha], dtype=np_dt)
    be = np.array([beta], dtype=np_dt)
    tm = (C.c_double * 4)() if timers else None
    st = stream if stream is not None else torch.cuda.current_stream(A.device).cuda_stream
    rc = lib().gemmul8_gemm(st, _dtype_code(dt), backend, OPS[opA], OPS[opB], m, n, k, al.ctypes.data, A.data_ptr(), lda,
                            B.data_ptr(), ldb, be.ctypes.data, C_out.data_ptr(), C_out.shape[1], num_moduli, int(fastmode),
                            work.data_ptr(), None, None, 0, 0, 0, 0, tm)
    check(rc, "gemmul8_gemm")
    return C_out, (list(tm) if timers else None), work


def syrk(A, num_moduli, uplo="L", trans="N", fastmode=False, alpha=1.0, beta=0.0, C_out=None, work=None, stream=None, timers=False):
    """One triangle of C = alpha*A*A^T + beta*C (trans "N", A is n x k) or alpha*A^T*A + beta*C (trans "T", A is k x n; plain transpose
    for complex types too) through gemmul8_syrk: INT8 backend, the triangle `uplo` ("L" / "U", diagonal included) bit-identical to
    `gemm(A, A, opA=trans, opB="T" if trans == "N" else "N")`, the other strict triangle of C_out neither read nor written.
    A and C_out are column-major matrices held as tensors of shape (cols, rows), as in `gemm`; a fresh C_out is zero-filled.
    Returns (C, timers_ns or None, work)."""
    import numpy as np
    import torch
    assert A.is_cuda and A.is_contiguous()
    dt = A.dtype
    if C_out is not None and (C_out.dtype != dt or not C_out.is_contiguous()):
        raise TypeError("A and C_out must share one dtype and be contiguous")
    lda = A.shape[1]
    n, k = (lda, A.shape[0]) if trans == "N" else (A.shape[0], lda)
    if C_out is None:
        C_out = torch.zeros((n, n), dtype=dt, device=A.device)
    if work is None:
        tot, _, _ = work_size(dt.is_complex, INT8, n, n, k, num_moduli)
        work = torch.empty(tot, dtype=torch.uint8, device=A.device)
    np_dt = {torch.float32: np.float32, torch.float64: np.float64, torch.complex64: np.complex64, torch.complex128: np.complex128}[dt]
    al = np.array([alpha], dtype=np_dt)
    be = np.array([beta], dtype=np_dt)
    tm = (C.c_double * 4)() if timers else None
    st = stream if stream is not None else torch.cuda.current_stream(A.device).cuda_stream
    rc = lib().gemmul8_syrk(st, _dtype_code(dt), INT8, UPLO[uplo], OPS[trans], n, k, al.ctypes.data, A.data_ptr(), lda, be.ctypes.data,
                            C_out.data_ptr(), C_out.shape[1], num_moduli, int(fastmode), work.data_ptr(), tm)
    check(rc, "gemmul8_syrk")
    return C_out, (list(tm) if timers else None), work


def herk(A, num_moduli, uplo="L", trans="N", fastmode=False, alpha=1.0, beta=0.0, C_out=None, work=None, stream=None, timers=False):
    """One triangle of C = alpha*A*A^H + beta*C (trans "N", A is n x k) or alpha*A^H*A + beta*C (trans "C", A is k x n) through gemmul8_herk:
    complex types, INT8 backend, REAL alpha and beta.  Off the diagonal the triangle `uplo` is bit-identical to
    `gemm(A, A, opA=trans, opB="C" if trans == "N" else "N", alpha=alpha, beta=beta)`; a diagonal entry holds that GEMM's real part and +0.0 as its
    imaginary part (the incoming one is ignored); the other strict triangle of C_out is neither read nor written.
    A and C_out are column-major matrices held as tensors of shape (cols, rows), as in `gemm`; a fresh C_out is zero-filled.
    Returns (C, timers_ns or None, work)."""
    import numpy as np
    import torch
    assert A.is_cuda and A.is_contiguous()
    dt = A.dtype
    if not dt.is_complex:
        raise TypeError("herk takes complex64 / complex128 (use syrk for the real types)")
    if trans not in ("N", "C"):
        raise ValueError("trans is 'N' or 'C'")
    if C_out is not None and (C_out.dtype != dt or not C_out.is_contiguous()):
        raise TypeError("A and C_out must share one dtype and be contiguous")
    lda = A.shape[1]
    n, k = (lda, A.shape[0]) if trans == "N" else (A.shape[0], lda)
    if C_out is None:
        C_out = torch.zeros((n, n), dtype=dt, device=A.device)
    if work is None:
        tot, _, _ = work_size(True, INT8, n, n, k, num_moduli)
        work = torch.empty(tot, dtype=torch.uint8, device=A.device)
    np_dt = np.float32 if dt == torch.complex64 else np.float64
    al = np.array([alpha], dtype=np_dt)
    be = np.array([beta], dtype=np_dt)
    tm = (C.c_double * 4)() if timers else None
    st = stream if stream is not None else torch.cuda.current_stream(A.device).cuda_stream
    rc = lib().gemmul8_herk(st, _dtype_code(dt), INT8, UPLO[uplo], OPS[trans], n, k, al.ctypes.data, A.data_ptr(), lda, be.ctypes.data,
                            C_out.data_ptr(), C_out.shape[1], num_moduli, int(fastmode), work.data_ptr(), tm)
    check(rc, "gemmul8_herk")
    return C_out, (list(tm) if timers else None), work


def syr2k_work_size(is_complex, n, k, num_moduli):
    """Bytes of workspace gemmul8_syr2k needs: that of the equivalent GEMM, whose inner dimension is twice k rounded up to a multiple of 256."""
    return work_size(is_complex, INT8, n, n, 2 * ((k + 255) // 256 * 256), num_moduli)[0]


def syr2k(A, B, num_moduli, uplo="L", trans="N", fastmode=False, alpha=1.0, beta=0.0, C_out=None, work=None, stream=None, timers=False):
    """One triangle of C = alpha*(A*B^T + B*A^T) + beta*C (trans "N", A and B are n x k) or alpha*(A^T*B + B^T*A) + beta*C (trans "T", A and B are
    k x n; plain transpose for complex types too) through gemmul8_syr2k: INT8 backend, the triangle `uplo` ("L" / "U", diagonal included) bit-identical
    to `gemm(P, Q, opA=trans, opB="T" if trans == "N" else "N")` with P = [A, Z, B, Z], Q = [B, Z, A, Z] along k (Z: zeros up to a multiple of 256), the
    other strict triangle of C_out neither read nor written.  A, B and C_out are column-major matrices held as tensors of shape (cols, rows), as in `gemm`;
    A and B may have different leading dimensions (pass views through `lda` = tensor.stride(0)) or be the same tensor; a fresh C_out is zero-filled.
    Returns (C, timers_ns or None, work)."""
    import numpy as np
    import torch
    dt = A.dtype
    for X in (A, B):
        assert X.is_cuda and X.dim() == 2 and X.stride(1) == 1 and X.stride(0) >= X.shape[1]
    if B.dtype != dt or B.shape != A.shape or (C_out is not None and (C_out.dtype != dt or C_out.dim() != 2 or C_out.stride(1) != 1)):
        raise TypeError("A, B and C_out must share one dtype, A and B one shape, and every column must be contiguous")
    n, k = (A.shape[1], A.shape[0]) if trans == "N" else (A.shape[0], A.shape[1])
    if C_out is None:
        C_out = torch.zeros((n, n), dtype=dt, device=A.device)
    if work is None:
        work = torch.empty(syr2k_work_size(dt.is_complex, n, k, num_moduli), dtype=torch.uint8, device=A.device)
    np_dt = {torch.float32: np.float32, torch.float64: np.float64, torch.complex64: np.complex64, torch.complex128: np.complex128}[dt]
    al = np.array([alpha], dtype=np_dt)
    be = np.array([beta], dtype=np_dt)
    tm = (C.c_double * 4)() if timers else None
    st = stream if stream is not None else torch.cuda.current_stream(A.device).cuda_stream
    rc = lib().gemmul8_syr2k(st, _dtype_code(dt), INT8, UPLO[uplo], OPS[trans], n, k, al.ctypes.data, A.data_ptr(), A.stride(0), B.data_ptr(), B.stride(0),
                             be.ctypes.data, C_out.data_ptr(), C_out.stride(0), num_moduli, int(fastmode), work.data_ptr(), tm)
    check(rc, "gemmul8_syr2k")
    return C_out, (list(tm) if timers else None), work


def her2k_work_size(n, k, num_moduli):
    """Bytes of workspace gemmul8_her2k needs: that of the equivalent complex GEMM (n, n, k)."""
    return work_size(True, INT8, n, n, k, num_moduli)[0]


def her2k(A, B, num_moduli, uplo="L", trans="N", fastmode=False, alpha=1.0, beta=0.0, C_out=None, work=None, stream=None, timers=False):
    """One triangle of C = alpha*A*B^H + conj(alpha)*B*A^H + beta*C (trans "N", A and B are n x k) or alpha*A^H*B + conj(alpha)*B^H*A + beta*C
    (trans "C", A and B are k x n) through gemmul8_her2k: complex types, INT8 backend, a COMPLEX alpha and a REAL beta.  With
    W = `gemm(A, B, opA=trans, opB="C" if trans == "N" else "N")` every stored entry is alpha*W[i,j] + conj(alpha*W[j,i]) + beta*C[i,j] in the fused form
    include/gemmul8_c.h states; the diagonal's imaginary part is +0.0 (the incoming one is ignored); the other strict triangle of C_out is neither read
    nor written.  A, B and C_out are column-major matrices held as tensors of shape (cols, rows), as in `gemm`; A and B may have different leading
    dimensions (views: `lda` = tensor.stride(0)) or be the same tensor; a fresh C_out is zero-filled.  Returns (C, timers_ns or None, work)."""
    import numpy as np
    import torch
    dt = A.dtype
    if not dt.is_complex:
        raise TypeError("her2k takes complex64 / complex128 (use syr2k for the real types)")
    if trans not in ("N", "C"):
        raise ValueError("trans is 'N' or 'C'")
    for X in (A, B):
        assert X.is_cuda and X.dim() == 2 and X.stride(1) == 1 and X.stride(0) >= X.shape[1]
    if B.dtype != dt or B.shape != A.shape or (C_out is not None and (C_out.dtype != dt or C_out.dim() != 2 or C_out.stride(1) != 1)):
        raise TypeError("A, B and C_out must share one dtype, A and B one shape, and every column must be contiguous")
    n, k = (A.shape[1], A.shape[0]) if trans == "N" else (A.shape[0], A.shape[1])
    if C_out is None:
        C_out = torch.zeros((n, n), dtype=dt, device=A.device)
    if work is None:
        work = torch.empty(her2k_work_size(n, k, num_moduli), dtype=torch.uint8, device=A.device)
    al = np.array([alpha], dtype=np.complex64 if dt == torch.complex64 else np.complex128)
    be = np.array([beta], dtype=np.float32 if dt == torch.complex64 else np.float64)
    tm = (C.c_double * 4)() if timers else None
    st = stream if stream is not None else torch.cuda.current_stream(A.device).cuda_stream
    rc = lib().gemmul8_her2k(st, _dtype_code(dt), INT8, UPLO[uplo], OPS[trans], n, k, al.ctypes.data, A.data_ptr(), A.stride(0), B.data_ptr(), B.stride(0),
                             be.ctypes.data, C_out.data_ptr(), C_out.stride(0), num_moduli, int(fastmode), work.data_ptr(), tm)
    check(rc, "gemmul8_her2k")
    return C_out, (list(tm) if timers else None), work


def symm_work_size(is_complex, m, n, side, num_moduli):
    """Bytes of workspace gemmul8_symm / gemmul8_hemm need: that of the equivalent GEMM, whose inner dimension is the order of A (m for side "L", n for "R")."""
    return work_size(is_complex, INT8, m, n, m if SIDE[side] == 0 else n, num_moduli)[0]


def _symm(name, A, B, num_moduli, side, uplo, fastmode, alpha, beta, C_out, work, stream, timers):
    import numpy as np
    import torch
    dt = A.dtype
    for X in (A, B):
        assert X.is_cuda and X.dim() == 2 and X.stride(1) == 1 and X.stride(0) >= X.shape[1]
    if B.dtype != dt or A.shape[0] != A.shape[1] or (C_out is not None and (C_out.dtype != dt or C_out.dim() != 2 or C_out.stride(1) != 1)):
        raise TypeError("A, B and C_out must share one dtype, A must be square, and every column must be contiguous")
    n, m = B.shape
    ka = m if SIDE[side] == 0 else n
    if A.shape[0] != ka:
        raise ValueError(f"A is of order {A.shape[0]}, side {side!r} of an {m} x {n} B needs {ka}")
    if C_out is None:
        C_out = torch.zeros((n, m), dtype=dt, device=A.device)
    if work is None:
        work = torch.empty(symm_work_size(dt.is_complex, m, n, side, num_moduli), dtype=torch.uint8, device=A.device)
    np_dt = {torch.float32: np.float32, torch.float64: np.float64, torch.complex64: np.complex64, torch.complex128: np.complex128}[dt]
    al = np.array([alpha], dtype=np_dt)
    be = np.array([beta], dtype=np_dt)
    tm = (C.c_double * 4)() if timers else None
    st = stream if stream is not None else torch.cuda.current_stream(A.device).cuda_stream
    rc = getattr(lib(), name)(st, _dtype_code(dt), INT8, SIDE[side], UPLO[uplo], m, n, al.ctypes.data, A.data_ptr(), A.stride(0), B.data_ptr(), B.stride(0),
                              be.ctypes.data, C_out.data_ptr(), C_out.stride(0), num_moduli, int(fastmode), work.data_ptr(), tm)
    check(rc, name)
    return C_out, (list(tm) if timers else None), work


def symm(A, B, num_moduli, side="L", uplo="L", fastmode=False, alpha=1.0, beta=0.0, C_out=None, work=None, stream=None, timers=False):
    """C = alpha*A*B + beta*C (side "L", A is m x m) or alpha*B*A + beta*C (side "R", A is n x n) with a SYMMETRIC A of which only the triangle `uplo`
    ("L" / "U") is read, through gemmul8_symm: INT8 backend, plain transpose for complex types too; bit-identical to
    `gemm(Afull, B)` (side "L") / `gemm(B, Afull, opB="T")` (side "R") with the full matrix materialised, which this call never does.
    A, B and C_out are column-major matrices held as tensors of shape (cols, rows), as in `gemm`; views with a larger leading dimension are taken
    through tensor.stride(0); a fresh C_out is zero-filled.  Returns (C, timers_ns or None, work)."""
    return _symm("gemmul8_symm", A, B, num_moduli, side, uplo, fastmode, alpha, beta, C_out, work, stream, timers)


def hemm(A, B, num_moduli, side="L", uplo="L", fastmode=False, alpha=1.0, beta=0.0, C_out=None, work=None, stream=None, timers=False):
    """`symm` with a HERMITIAN A through gemmul8_hemm: complex types, complex alpha and beta; the mirrored triangle is the conjugate of the stored one and
    the imaginary parts of the stored diagonal count as 0.  Bit-identical to `gemm(Afull, B)` (side "L") / `gemm(B, Afull, opB="C")` (side "R")."""
    if not A.dtype.is_complex:
        raise TypeError("hemm takes complex64 / complex128 (use symm for the real types)")
    return _symm("gemmul8_hemm", A, B, num_moduli, side, uplo, fastmode, alpha, beta, C_out, work, stream, timers)


def trmm_work_size(is_complex, m, n, side, num_moduli):
    """Bytes of workspace gemmul8_trmm needs: that of the equivalent GEMM, whose inner dimension is the order of A (m for side "L", n for "R")."""
    return work_size(is_complex, INT8, m, n, m if SIDE[side] == 0 else n, num_moduli)[0]


def trmm(A, B, num_moduli, side="L", uplo="L", trans="N", diag="N", alpha=1, fastmode=False, C_out=None, work=None, stream=None, timers=False):
    """C = alpha*op(A)*B (side "L", A is m x m) or alpha*B*op(A) (side "R", A is n x n) with a TRIANGULAR A through gemmul8_trmm: only the triangle `uplo`
    ("L" / "U") of A is read -- under diag "U" not even its diagonal, which counts as ones -- and the other half is zero; trans "N" / "T" / "C".  INT8
    backend; bit-identical to `gemm(M, B)` (side "L") / `gemm(B, Mt, opB="T")` (side "R") with M = op(Atri) / its plain transpose Mt materialised, which
    this call never does, at about half of that GEMM's matrix work.  There is no beta: C is never read.  C_out=None allocates; C_out=B is the in-place form
    of classic BLAS.  alpha: a number, or a one-element device tensor of A's dtype.  A, B and C_out are column-major matrices held as tensors of shape
    (cols, rows), as in `gemm`; views with a larger leading dimension are taken through tensor.stride(0).  Returns (C, timers_ns or None, work)."""
    import numpy as np
    import torch
    dt = A.dtype
    for X in (A, B):
        assert X.is_cuda and X.dim() == 2 and X.stride(1) == 1 and X.stride(0) >= X.shape[1]
    if B.dtype != dt or A.shape[0] != A.shape[1] or (C_out is not None and (C_out.dtype != dt or C_out.dim() != 2 or C_out.stride(1) != 1)):
        raise TypeError("A, B and C_out must share one dtype, A must be square, and every column must be contiguous")
    n, m = B.shape
    ka = m if SIDE[side] == 0 else n
    if A.shape[0] != ka:
        raise ValueError(f"A is of order {A.shape[0]}, side {side!r} of an {m} x {n} B needs {ka}")
    if C_out is None:
        C_out = torch.empty((n, m), dtype=dt, device=A.device)
    elif tuple(C_out.shape) != (n, m):
        raise ValueError(f"C_out is {tuple(C_out.shape)}, the product is {(n, m)}")
    if work is None:
        work = torch.empty(trmm_work_size(dt.is_complex, m, n, side, num_moduli), dtype=torch.uint8, device=A.device)
    if isinstance(alpha, torch.Tensor):
        if not alpha.is_cuda or alpha.dtype != dt or alpha.numel() != 1:
            raise TypeError("a tensor alpha is one element of A's dtype on the device")
        al_ptr = alpha.data_ptr()
    else:
        np_dt = {torch.float32: np.float32, torch.float64: np.float64, torch.complex64: np.complex64, torch.complex128: np.complex128}[dt]
        al = np.array([alpha], dtype=np_dt)
        al_ptr = al.ctypes.data
    tm = (C.c_double * 4)() if timers else None
    st = stream if stream is not None else torch.cuda.current_stream(A.device).cuda_stream
    rc = lib().gemmul8_trmm(st, _dtype_code(dt), INT8, SIDE[side], UPLO[uplo], OPS[trans], DIAG[diag], m, n, al_ptr, A.data_ptr(), A.stride(0),
                            B.data_ptr(), B.stride(0), C_out.data_ptr(), C_out.stride(0), num_moduli, int(fastmode), work.data_ptr(), tm)
    check(rc, "gemmul8_trmm")
    return C_out, (list(tm) if timers else None), work


def trsm_work_size(is_complex, m, n, side, num_moduli):
    """Bytes of workspace gemmul8_trsm needs: the largest workspace of the recipe's GEMMs, rounded up to 64, plus a 64-byte tail."""
    return lib().gemmul8_trsm_work_size(int(is_complex), INT8, SIDE[side], m, n, num_moduli)


def trsm(A, B, num_moduli, side="L", uplo="L", trans="N", diag="N", alpha=1, fastmode=False, work=None, stream=None, timers=False):
    """Solves op(A) X = alpha*B (side "L", A is m x m) or X op(A) = alpha*B (side "R", A is n x n) with a TRIANGULAR A through gemmul8_trsm, IN PLACE: B
    is overwritten with X.  Only the triangle `uplo` of A is read -- under diag "U" not even its diagonal; trans "N" / "T" / "C".  INT8 backend.  The
    result is the recipe include/gemmul8_c.h states (tests/trsm_util.py is its model): a recursive blocking whose updates are `gemm` calls on sub-matrix
    views and whose diagonal blocks of order <= TRSM_LEAF are solved by substitution in the element type.  alpha: a number, or a one-element device tensor
    of A's dtype.  A and B are column-major matrices held as tensors of shape (cols, rows), as in `gemm`; views with a larger leading dimension are taken
    through tensor.stride(0).  Returns (B, timers_ns or None, work); timers_ns[2] is the time of the leaf solves."""
    import numpy as np
    import torch
    dt = A.dtype
    for X in (A, B):
        assert X.is_cuda and X.dim() == 2 and X.stride(1) == 1 and X.stride(0) >= X.shape[1]
    if B.dtype != dt or A.shape[0] != A.shape[1]:
        raise TypeError("A and B must share one dtype, A must be square, and every column must be contiguous")
    n, m = B.shape
    ka = m if SIDE[side] == 0 else n
    if A.shape[0] != ka:
        raise ValueError(f"A is of order {A.shape[0]}, side {side!r} of an {m} x {n} B needs {ka}")
    if work is None:
        work = torch.empty(trsm_work_size(dt.is_complex, m, n, side, num_moduli), dtype=torch.uint8, device=A.device)
    if isinstance(alpha, torch.Tensor):
        if not alpha.is_cuda or alpha.dtype != dt or alpha.numel() != 1:
            raise TypeError("a tensor alpha is one element of A's dtype on the device")
        al_ptr = alpha.data_ptr()
    else:
        np_dt = {torch.float32: np.float32, torch.float64: np.float64, torch.complex64: np.complex64, torch.complex128: np.complex128}[dt]
        al = np.array([alpha], dtype=np_dt)
        al_ptr = al.ctypes.data
    tm = (C.c_double * 4)() if timers else None
    st = stream if stream is not None else torch.cuda.current_stream(A.device).cuda_stream
    rc = lib().gemmul8_trsm(st, _dtype_code(dt), INT8, SIDE[side], UPLO[uplo], OPS[trans], DIAG[diag], m, n, al_ptr, A.data_ptr(), A.stride(0),
                            B.data_ptr(), B.stride(0), num_moduli, int(fastmode), work.data_ptr(), tm)
    check(rc, "gemmul8_trsm")
    return B, (list(tm) if timers else None), work


def __getattr__(name):
    if name == "TRSM_LEAF":  # the leaf order of gemmul8_trsm, read from the library
        return lib().gemmul8_trsm_leaf()
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def gemm_batched(A, B, num_moduli, fastmode=False, opA="N", opB="N", alpha=1.0, beta=0.0, C_out=None, work=None, stream=None, backend=INT8):
    """A strided batch as ONE set of launches (gemmul8_gemm_batched).  A, B (and C_out): contiguous tensors of shape
    (batch, cols, rows) -- each item a column-major matrix as in `gemm`; a batch dimension of 1 on A or B broadcasts (stride 0).
    Returns (C, work).  Bit-identical to calling `gemm` per item."""
    import numpy as np
    import torch
    assert A.is_cuda and B.is_cuda and A.is_contiguous() and B.is_contiguous() and A.dim() == 3 and B.dim() == 3
    dt = A.dtype
    batch = max(A.shape[0], B.shape[0])
    assert A.shape[0] in (1, batch) and B.shape[0] in (1, batch) and B.dtype == dt
    lda, ldb = A.shape[2], B.shape[2]
    m, k = (lda, A.shape[1]) if opA == "N" else (A.shape[1], lda)
    kb, n = (ldb, B.shape[1]) if opB == "N" else (B.shape[1], ldb)
    assert k == kb, (k, kb)
    if C_out is None:
        C_out = torch.zeros((batch, n, m), dtype=dt, device=A.device)
    assert C_out.is_contiguous() and C_out.dtype == dt and C_out.shape[0] == batch
    if work is None:
        work = torch.empty(lib().gemmul8_work_size_batched(int(dt.is_complex), backend, m, n, k, num_moduli, batch), dtype=torch.uint8, device=A.device)
    np_dt = {torch.float32: np.float32, torch.float64: np.float64, torch.complex64: np.complex64, torch.complex128: np.complex128}[dt]
    al, be = np.array([alpha], dtype=np_dt), np.array([beta], dtype=np_dt)
    st = stream if stream is not None else torch.cuda.current_stream(A.device).cuda_stream
    sa = 0 if A.shape[0] == 1 else A.shape[1] * A.shape[2]
    sb = 0 if B.shape[0] == 1 else B.shape[1] * B.shape[2]
    rc = lib().gemmul8_gemm_batched(st, _dtype_code(dt), backend, OPS[opA], OPS[opB], m, n, k, al.ctypes.data, A.data_ptr(), lda, sa, B.data_ptr(), ldb, sb,
                                    be.ctypes.data, C_out.data_ptr(), C_out.shape[2], C_out.shape[1] * C_out.shape[2], batch, num_moduli,
                                    int(fastmode), work.data_ptr())
    check(rc, "gemmul8_gemm_batched")
    return C_out, work


def gemm_batched_ptr(As, Bs, num_moduli, fastmode=False, opA="N", opB="N", alpha=1.0, beta=0.0, Cs=None, work=None, stream=None, backend=INT8,
                     m=None, n=None, k=None, lda=None, ldb=None, ldc=None, dtype=None):
    """A pointer-array batch as ONE set of launches (gemmul8_gemm_batched_ptr): item b is Cs[b] = alpha op(As[b]) op(Bs[b]) + beta Cs[b].

    As, Bs, Cs: sequences of `batch` tensors, each operand's of one shape, dtype and leading dimension -- column-major matrices held as tensors of shape
    (cols, rows) as in `gemm`; views (tensor.stride(0) is the leading dimension), scattered allocations and the same tensor repeated are all fine for As and
    Bs; the Cs must not overlap.  Cs=None allocates the outputs.  The three device arrays of addresses are built with one host-to-device copy per operand,
    allocated and copied ON THE STREAM THE CALL RUNS ON (`stream`: a raw stream handle, default torch's current stream): the copies are ordered before the
    kernels that read the arrays, and the allocator hands their memory out again only to later work of that stream.

    Alternatively As, Bs, Cs are int64 device tensors of `batch` addresses each (nothing is copied; the kernels read them in stream order, under graph
    capture at every replay); m, n, k, lda, ldb, ldc and dtype are then given explicitly.

    Returns (Cs, work).  Bit-identical to calling `gemm` per item.  Item addresses are not validated."""
    import numpy as np
    import torch
    if isinstance(As, torch.Tensor) != isinstance(Bs, torch.Tensor) or (Cs is not None and isinstance(Cs, torch.Tensor) != isinstance(As, torch.Tensor)):
        raise TypeError("As, Bs and Cs are all sequences of tensors or all int64 device tensors of addresses")
    if isinstance(As, torch.Tensor):
        if Cs is None or None in (m, n, k, lda, ldb, ldc, dtype):
            raise TypeError("address tensors need Cs, m, n, k, lda, ldb, ldc and dtype")
        for X in (As, Bs, Cs):
            if not (X.is_cuda and X.dtype == torch.int64 and X.dim() == 1 and X.is_contiguous() and X.numel() == As.numel()):
                raise TypeError("address arrays are contiguous one-dimensional int64 device tensors of one length")
        dt, batch, dev = dtype, As.numel(), As.device
        pa, pb, pc = As, Bs, Cs
        call_stream = torch.cuda.ExternalStream(stream, device=dev) if stream is not None else torch.cuda.current_stream(dev)
    else:
        As, Bs = list(As), list(Bs)
        batch = len(As)
        if batch == 0 or len(Bs) != batch:
            raise ValueError("As and Bs hold the same number (>= 1) of items")
        dt, dev = As[0].dtype, As[0].device
        call_stream = torch.cuda.ExternalStream(stream, device=dev) if stream is not None else torch.cuda.current_stream(dev)

        def common(Xs, what):
            for X in Xs:
                if not (X.is_cuda and X.device == dev and X.dtype == dt and X.dim() == 2 and X.stride(1) == 1 and X.stride(0) >= X.shape[1] and
                        X.shape == Xs[0].shape and X.stride(0) == Xs[0].stride(0)):
                    raise TypeError(f"the items of {what} are device matrices of one dtype, shape and leading dimension with contiguous columns")
            return Xs[0].shape, Xs[0].stride(0)
        (ca, ra), lda = common(As, "As")
        (cb, rb), ldb = common(Bs, "Bs")
        m, k = (ra, ca) if opA == "N" else (ca, ra)
        kb, n = (rb, cb) if opB == "N" else (cb, rb)
        if k != kb:
            raise ValueError(f"inner dimensions differ: {k} and {kb}")
        if Cs is None:
            Cs = [torch.zeros((n, m), dtype=dt, device=dev) for _ in range(batch)]
        Cs = list(Cs)
        if len(Cs) != batch:
            raise ValueError("Cs holds one tensor per item")
        (cc, rc_), ldc = common(Cs, "Cs")
        if (cc, rc_) != (n, m):
            raise ValueError(f"the items of Cs are {(cc, rc_)}, the products are {(n, m)}")
        # one host-to-device copy per operand, on the call's stream
        with torch.cuda.stream(call_stream):
            pa, pb, pc = [torch.tensor([X.data_ptr() for X in Xs], dtype=torch.int64).to(dev) for Xs in (As, Bs, Cs)]
    if work is None:
        work = torch.empty(lib().gemmul8_work_size_batched(int(dt.is_complex), backend, m, n, k, num_moduli, batch), dtype=torch.uint8, device=dev)
    np_dt = {torch.float32: np.float32, torch.float64: np.float64, torch.complex64: np.complex64, torch.complex128: np.complex128}[dt]
    al, be = np.array([alpha], dtype=np_dt), np.array([beta], dtype=np_dt)
    rc = lib().gemmul8_gemm_batched_ptr(call_stream.cuda_stream, _dtype_code(dt), backend, OPS[opA], OPS[opB], m, n, k, al.ctypes.data, pa.data_ptr(), lda, pb.data_ptr(), ldb,
                                        be.ctypes.data, pc.data_ptr(), ldc, batch, num_moduli, int(fastmode), work.data_ptr())
    check(rc, "gemmul8_gemm_batched_ptr")
    return Cs, work
