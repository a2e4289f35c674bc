/*
 * gemmul8_c.h -- C ABI of the MI355X-native Ozaki-scheme-II GEMM emulator (libgemmul8.so).
 *
 * This is the drop-in boundary for the hot path of RIKEN-RCCS/GEMMul8: plain pointers and sizes,
 * no C++ / torch types.  The C++ template API of include/gemmul8.hpp (gemmul8::workSize / gemm /
 * gemmLt, reference GEMMul8/include/gemmul8.hpp:25-151) and the LD_PRELOAD hipBLAS hook
 * (reference GEMMul8/src/hook.cu:846-1055) are thin layers over these entry points.
 *
 * Conventions: column-major BLAS semantics, all matrix pointers are DEVICE pointers, `stream` is a
 * hipStream_t passed as void*.  Every function returns 0 on success, a negative GEMMUL8_E_* code
 * on bad arguments, or a positive hipError_t if the HIP runtime failed.
 */
#ifndef GEMMUL8_C_H
#define GEMMUL8_C_H

#include <stddef.h>
#include <stdint.h>

#if defined(__GNUC__)
#define GEMMUL8_API __attribute__((visibility("default")))
#else
#define GEMMUL8_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* element type of A, B, C (reference: template parameter T of gemmul8::gemm, gemmul8.hpp:98) */
enum { GEMMUL8_S = 0, GEMMUL8_D = 1, GEMMUL8_C = 2, GEMMUL8_Z = 3 };
/* low-precision engine (reference: enum class Backend, gemmul8.hpp:19-20) */
enum { GEMMUL8_INT8 = 0, GEMMUL8_FP8 = 1 };
/* op(X): 0/1/2, or the hipblasOperation_t values 111/112/113 (both accepted) */
enum { GEMMUL8_OP_N = 0, GEMMUL8_OP_T = 1, GEMMUL8_OP_C = 2 };

enum {
    GEMMUL8_OK = 0,
    GEMMUL8_E_NUM_MODULI = -1, /* num_moduli outside 2..20 */
    GEMMUL8_E_ARG = -2,        /* null pointer / bad enum / k > 2^17 */
    GEMMUL8_E_UNSUPPORTED = -3, /* combination not built */
    GEMMUL8_E_INTERNAL = -4     /* resource failure that is NOT a property of the arguments (allocation, transport): a multi-rank caller
                                  must not treat it as "every rank declines" */
};

/* Workspace bytes; same formula as the reference so callers' allocations stay valid.
 * Replaces gemmul8::workSize<is_Complex,backend> (include/gemmul8.hpp:25-35,
 * src/gemmul8_real.hpp:8-47, src/gemmul8_complex.hpp:8-47). */
GEMMUL8_API size_t gemmul8_work_size(int is_complex, int backend, size_t m, size_t n, size_t k, unsigned num_moduli,
                         int enable_skip_scalA, int enable_skip_scalB, size_t *workSizeA, size_t *workSizeB);

/* Whole emulated GEMM: C = alpha*op(A)*op(B) + beta*C.
 * Replaces gemmul8::gemm<T,backend> / gemmLt<T,backend> (include/gemmul8.hpp:98-151,
 * src/gemmul8_real.hpp:52-211, src/gemmul8_complex.hpp:52-226).
 * alpha/beta may be host or device pointers (detected like inverse_scaling_real.hpp:211-213).
 * timers_ns: NULL = fully asynchronous; else 4 doubles [scaling, low-prec GEMM, requantise (always
 * 0: fused into the GEMM epilogue), inverse scaling] in ns, measured with events (one host sync). */
GEMMUL8_API int gemmul8_gemm(void *stream, int dtype, int backend, int op_A, int op_B, size_t m, size_t n, size_t k,
                 const void *alpha, const void *A, size_t lda, const void *B, size_t ldb, const void *beta, void *C,
                 size_t ldc, unsigned num_moduli, int fastmode, void *work, void *workA, void *workB,
                 int enable_skip_scalA, int enable_skip_scalB, int skip_scalA, int skip_scalB, double *timers_ns);

/* Where the intermediates of the last/next gemmul8_gemm call live inside the workspaces (device
 * pointers; same carving as src/gemmul8_real.hpp:95-107).  Used by the parity tests and by the
 * moduli-sharded multi-GPU driver. */
typedef struct gemmul8_layout {
    size_t kp, mp;             /* padded k and m (multiples of 256) */
    size_t num_mat;            /* low-precision planes per part */
    size_t parts;              /* 1 (real) or 3 (complex: Re, Im, Re+Im) */
    size_t sizeA, sizeB, sizeC;/* elements per plane: kp*mp, kp*n, mp*n */
    void *A_lo, *B_lo;         /* plane (part,q) at X_lo + (part*num_mat_total + q)*sizeX, num_mat_total = num_mat (+1 if skip enabled) ... see part_strideX */
    size_t part_strideA, part_strideB; /* bytes between Re/Im/Re+Im plane sets */
    void *A_bound, *B_bound;   /* accurate-mode 7-bit bound planes (alias plane 0 unless skip enabled) */
    int16_t *sftA, *sftB;      /* negated shift exponents (non-finite mode 1: INT16_MIN for a flagged row / column) */
    void *C_mid;               /* N residue planes [n][mp] (complex: interleaved re,im) */
    void *scratch;             /* the reference's C_hi region (free for row/col maxima etc.) */
    size_t scratch_bytes;
    size_t lo_format;          /* encoding of the A_lo / B_lo residue planes: 0 = one byte per element (int8 residues / e4m3 pieces), row r at
                                  r * kp; 1 = FP6 panel images of the FP8 backend's pieces (csrc/oz2_gemm_f6.hip; n >= 64, skip-scaling
                                  not enabled -- cached planes may meet a partner of another shape --, unless GEMMUL8_FP8_PLANES=e4m3): same plane offsets and strides, 3/4 of each plane used.  The bound planes stay bytes. */
} gemmul8_layout;

GEMMUL8_API int gemmul8_get_layout(int dtype, int backend, size_t m, size_t n, size_t k, unsigned num_moduli, void *work, void *workA,
                       void *workB, int enable_skip_scalA, int enable_skip_scalB, gemmul8_layout *out);

/* ABI guard.  gemmul8_get_layout fills sizeof(gemmul8_layout) bytes of the CALLER's struct: a binding compiled against an older header
 * (the struct grew by lo_format in version 5) would be overrun.  GEMMUL8_ABI_VERSION is bumped whenever a struct of this header grows or a
 * signature changes; a binding checks gemmul8_abi_version() == GEMMUL8_ABI_VERSION (C / C++) or gemmul8_layout_bytes() against the size of
 * its own mirror of the struct (ctypes: gemmul8_amd/__init__.py does) before it calls anything else. */
#define GEMMUL8_ABI_VERSION 7   /* 7: gemmul8_add_f64; gemmul8_dist_engine grew by add_f64 */
GEMMUL8_API int gemmul8_abi_version(void);
GEMMUL8_API size_t gemmul8_layout_bytes(void);

/* ---- phase-level entry points (one per kernel family) -------------------------------------- */

/* Shifts + residue planes of both operands for moduli [t_begin, t_end).  fastmode=0 runs the
 * accurate path (extract, bound GEMM with max epilogue, shift).  Replaces fast::scaling /
 * accu::scaling (src/scaling_fast_real.hpp:222-268, src/scaling_accu_real.hpp:380-457 and the
 * complex variants). */
GEMMUL8_API int gemmul8_scale(void *stream, int dtype, int backend, int op_A, int op_B, size_t m, size_t n, size_t k, const void *A,
                  size_t lda, const void *B, size_t ldb, unsigned num_moduli, int fastmode, unsigned t_begin,
                  unsigned t_end, const gemmul8_layout *L, int skipA, int skipB);

/* The two halves of gemmul8_scale, split where a multi-GPU run must exchange data:
 *  _bounds (accurate mode only): 7-bit bound planes of A and B, then the bound GEMM restricted to
 *          columns [col_begin, col_end) of op(B); leaves int32 rowmax[mp] at L->scratch and colmax[pad256(n)]
 *          right behind it (zero outside the computed columns) -- ranks combine them with one
 *          all-reduce(MAX) over the (mp + pad256(n)) int32 words;
 *  _finish: final shifts (from the maxima, or the fast-mode norms) and the residue planes. */
GEMMUL8_API int gemmul8_scale_bounds(void *stream, int dtype, int backend, int op_A, int op_B, size_t m, size_t n, size_t k,
                                     const void *A, size_t lda, const void *B, size_t ldb, unsigned num_moduli, size_t col_begin,
                                     size_t col_end, const gemmul8_layout *L, int skipA, int skipB);
GEMMUL8_API int gemmul8_scale_finish(void *stream, int dtype, int backend, int op_A, int op_B, size_t m, size_t n, size_t k,
                                     const void *A, size_t lda, const void *B, size_t ldb, unsigned num_moduli, int fastmode,
                                     unsigned t_begin, unsigned t_end, const gemmul8_layout *L, int skipA, int skipB);

/* Low-precision GEMMs of moduli [t_begin, t_end) with the requantise epilogue: fills C_mid planes.
 * Replaces gemm_low_prec_* + conv_hi2mid (src/matmult.hpp:120-389, src/conv_hi2mid_real.hpp,
 * src/conv_hi2mid_complex.hpp; loop at src/gemmul8_real.hpp:144-191).  k is the inner dimension the layout was made for: a k whose
 * padding differs from L->kp is GEMMUL8_E_ARG (the FP8 backend chooses its exact-accumulation form from it). */
GEMMUL8_API int gemmul8_lowprec_gemm(void *stream, int dtype, int backend, size_t m, size_t n, size_t k, unsigned num_moduli,
                         unsigned t_begin, unsigned t_end, const gemmul8_layout *L);

/* CRT accumulation + inverse scaling + axpby on an arbitrary column block: C_mid planes given by
 * pointer/stride so that a GPU can finish the columns it owns after an exchange of residue planes.
 * Replaces inverse_scaling (src/inverse_scaling_real.hpp:242-278, inverse_scaling_complex.hpp). */
GEMMUL8_API int gemmul8_crt(void *stream, int dtype, int backend, unsigned num_moduli, size_t m, size_t n, const void *C_mid,
                size_t ld_mid, size_t plane_stride, const int16_t *sftA, const int16_t *sftB, const void *alpha,
                const void *beta, void *C, size_t ldc);

/* A strided batch of GEMMs (same shape, alpha / beta shared; strides in ELEMENTS of the matrix type, as in
 * hipblas{S,D,C,Z}gemmStridedBatched) as ONE set of launches: every kernel of the pipeline takes the item from gridDim.z, the
 * persistent GEMM kernels run over the items' residue planes in one launch.  `work` holds gemmul8_work_size_batched bytes (the items'
 * workspaces are consecutive blocks of gemmul8_batched_item_bytes).  Both backends (FP8: k <= 65536 as in gemmul8_gemm).
 * Bit-identical to per-item gemmul8_gemm calls.  No counterpart in the reference (it hooks no batched entry point). */
GEMMUL8_API size_t gemmul8_batched_item_bytes(int is_complex, int backend, size_t m, size_t n, size_t k, unsigned num_moduli);
GEMMUL8_API size_t gemmul8_work_size_batched(int is_complex, int backend, size_t m, size_t n, size_t k, unsigned num_moduli, size_t batch);
GEMMUL8_API int gemmul8_gemm_batched(void *stream, int dtype, int backend, int op_A, int op_B, size_t m, size_t n, size_t k,
                         const void *alpha, const void *A, size_t lda, long long strideA, const void *B, size_t ldb,
                         long long strideB, const void *beta, void *C, size_t ldc, long long strideC, size_t batch,
                         unsigned num_moduli, int fastmode, void *work);

/* The same batch with the items' addresses in three POINTER ARRAYS (hipblas{S,D,C,Z}gemmBatched): item b is
 * C_array[b] = alpha * op(A_array[b]) * op(B_array[b]) + beta * C_array[b], all items of one shape, lda / ldb / ldc, alpha and beta.
 *   - A_array, B_array, C_array hold `batch` pointers each in DEVICE-accessible memory.  They are read by the kernels in stream order (each
 *     item's workgroups load their own entries), never by the host: no copy back, no synchronisation, capturable in a HIP graph.
 *   - `work` is the strided form's workspace (gemmul8_work_size_batched); argument checks, the k limits (2^17; FP8: 65536), degenerate sizes
 *     (m, n, k or batch == 0: GEMMUL8_OK, nothing touched) and the 65535-item launch chunks are those of gemmul8_gemm_batched, in the same order.
 *     Both backends, both modes, both non-finite modes.
 *   - The result is bit-identical to `batch` calls of gemmul8_gemm on the items.
 *   - Items may share or alias A and B (the same pointer many times is the broadcast case).  The C windows must not overlap each other or
 *     any A / B.  Nothing outside the m x n windows of C is written.
 *   - Each item pointer needs the alignment of its element type only (16-byte forms are chosen per item inside the kernels).
 *   - Item pointers are NOT validated: the library cannot tell a null or dangling entry from a valid one, a kernel will simply use it.
 *   - The arrays must stay unchanged until the call's kernels have run.  Under graph capture they are read at every REPLAY: what the
 *     arrays hold then is what the replay computes on.
 * No counterpart in the reference. */
GEMMUL8_API int gemmul8_gemm_batched_ptr(void *stream, int dtype, int backend, int op_A, int op_B, size_t m, size_t n, size_t k,
                         const void *alpha, const void *const *A_array, size_t lda, const void *const *B_array, size_t ldb,
                         const void *beta, void *const *C_array, size_t ldc, size_t batch, unsigned num_moduli, int fastmode,
                         void *work);

/* Symmetric rank-k update of one triangle: C = alpha*A*A^T + beta*C (trans = N, A is n x k) or C = alpha*A^T*A + beta*C (trans = T, A is
 * k x n; for the complex types too this is the plain transpose: SYRK, not HERK).  trans takes 0 / 1 or the hipblasOperation_t values 111 / 112,
 * uplo GEMMUL8_LOWER / GEMMUL8_UPPER or the hipblasFillMode_t values 122 / 121.  All four element types, INT8 backend only (GEMMUL8_FP8:
 * GEMMUL8_E_UNSUPPORTED -- the FP6 panel images of the two operands differ in layout).
 *   - The triangle named by uplo, diagonal included, holds bit for bit what
 *     gemmul8_gemm(dtype, GEMMUL8_INT8, trans, trans == N ? T : N, n, n, k, alpha, A, lda, A, lda, beta, C, ldc, ...) in non-finite mode 0 puts there;
 *     no byte of the other strict triangle of C or of the ldc padding is read or written; beta == 0 never reads C.
 *   - A is read, bounded and quantised once, the residue GEMMs run over the 256 x 256 tiles that touch the triangle only (about half the work of the
 *     GEMM; the accurate mode's bound GEMM stays the full square).
 *   - `work` holds gemmul8_work_size(is_complex, backend, n, n, k, num_moduli, 0, 0, NULL, NULL) bytes: the equivalent GEMM's workspace.
 *   - alpha / beta host or device pointers, timers_ns, stream order and capture safety (timers_ns == NULL) as in gemmul8_gemm.
 *   - n == 0 or k == 0: GEMMUL8_OK, C untouched.  Bad uplo / trans, a null pointer, k > 2^17: GEMMUL8_E_ARG.
 *   - gemmul8_set_nonfinite_mode is ignored: the call behaves as mode 0.
 * No counterpart in the reference (it emulates GEMM only). */
enum { GEMMUL8_LOWER = 0, GEMMUL8_UPPER = 1 };
GEMMUL8_API int gemmul8_syrk(void *stream, int dtype, int backend, int uplo, int trans, size_t n, size_t k, const void *alpha, const void *A,
                             size_t lda, const void *beta, void *C, size_t ldc, unsigned num_moduli, int fastmode, void *work,
                             double *timers_ns);

/* Hermitian rank-k update of one triangle: C = alpha*A*A^H + beta*C (trans = N, A is n x k) or C = alpha*A^H*A + beta*C (trans = C, A is k x n).
 * dtype GEMMUL8_C / GEMMUL8_Z only (S / D: GEMMUL8_E_ARG -- BLAS has no real HERK); trans takes 0 / 2 or the hipblasOperation_t values 111 / 113
 * (T, 1 / 112: GEMMUL8_E_ARG); uplo as in gemmul8_syrk.  alpha and beta point to REAL scalars (float for C, double for Z), host or device, detected
 * as elsewhere.  INT8 backend only (GEMMUL8_FP8: GEMMUL8_E_UNSUPPORTED).
 *   - Every OFF-DIAGONAL entry of the triangle named by uplo holds, bit for bit, what
 *     gemmul8_gemm(dtype, GEMMUL8_INT8, trans, trans == N ? C : N, n, n, k, (alpha, 0), A, lda, A, lda, (beta, 0), C, ldc, ...) in non-finite mode 0
 *     puts there.
 *   - A DIAGONAL entry holds that GEMM's real part bit for bit and +0.0 as its imaginary part.  The incoming imaginary part of a diagonal entry counts
 *     as 0 whatever the memory holds: a NaN there reaches neither component.
 *   - No byte of the other strict triangle of C or of the ldc padding is read or written; beta == 0 never reads C.
 *   - A is read, bounded and quantised ONCE.  HERK is not SYRK with a flag: in the GEMM of A with its own conjugate transpose the two sides share their
 *     shifts, their bound planes and their Re residue planes, but where one side holds the residues of Im and Re + Im the conjugated side holds those of
 *     -Im (the byte-wise negation; for the modulus 256 the byte -128 maps to itself) and of Re - Im, which no plane of the other side has.  The one
 *     operand pass therefore writes five plane sets: Re, Im, Re + Im into A's planes and -Im, Re - Im into parts 1 and 2 of the equivalent GEMM's B
 *     planes (that GEMM's workspace layout; part 0 of its B planes stays unwritten).
 *   - The result is NOT bitwise Hermitian: Re C of the equivalent GEMM is bitwise symmetric and its diagonal's imaginary part is exactly zero, but Im C
 *     is not bitwise antisymmetric (the CRT's reduction modulo P is not an odd function).  Every stored entry is therefore computed as the GEMM computes
 *     that entry -- row i of the left factor, row j of the right one -- and never mirrored or negated from the other triangle
 *     (tests/test_herk_premise.py pins all of this on the oracle).
 *   - The residue GEMMs run over the 256 x 256 tiles that touch the triangle only; the accurate mode's bound GEMM stays the full square.
 *   - `work`, timers_ns, stream order, capture safety, n == 0 or k == 0, null pointers and k > 2^17 as in gemmul8_syrk.
 *   - gemmul8_set_nonfinite_mode is ignored: the call behaves as mode 0.
 * No counterpart in the reference (it emulates GEMM only). */
GEMMUL8_API int gemmul8_herk(void *stream, int dtype, int backend, int uplo, int trans, size_t n, size_t k, const void *alpha, const void *A,
                             size_t lda, const void *beta, void *C, size_t ldc, unsigned num_moduli, int fastmode, void *work,
                             double *timers_ns);

/* Symmetric rank-2k update of one triangle: C = alpha*(A*B^T + B*A^T) + beta*C (trans = N, A and B are n x k) or
 * C = alpha*(A^T*B + B^T*A) + beta*C (trans = T, A and B are k x n); the plain transpose for the complex types too (HER2K, which applies alpha to one term
 * and conj(alpha) to the other, is not one GEMM with one scalar: it is gemmul8_her2k below, by another route).  All four types; uplo and trans as in gemmul8_syrk (N / T only,
 * the 0 / 1 and the hipBLAS values).  INT8 backend only (GEMMUL8_FP8: GEMMUL8_E_UNSUPPORTED, for gemmul8_syrk's reason).
 *   - The identity: A B^T + B A^T = P Q^T with P = [A, Z, B, Z] and Q = [B, Z, A, Z], Z = the n x (kh - k) zero block, kh = k rounded up to a multiple
 *     of 256 -- P and Q are n x 2 kh, and the second half of each starts on a 256 boundary (trans = T: everything transposed, P^T Q).
 *   - The triangle named by uplo, diagonal included, holds bit for bit what
 *     gemmul8_gemm(dtype, GEMMUL8_INT8, trans, trans == N ? T : N, n, n, 2 kh, alpha, P, ldP, Q, ldQ, beta, C, ldc, ...) in non-finite mode 0 puts
 *     there with P and Q materialised.  No byte of the other strict triangle of C or of the ldc padding is read or written; beta == 0 never reads C.
 *   - P and Q are never materialised: A and B are read where they lie, once per phase each, and every element leaves to the planes of both sides (Q's planes
 *     are P's with the two K halves swapped).  The residue GEMMs run over the 256 x 256 tiles that touch the triangle only; the accurate mode's bound
 *     GEMM stays the full square.
 *   - Row i of A and row i of B (trans = T: the columns) share ONE shift, as the rows of P do: a row of A far smaller than the same row of B loses bits
 *     that it would keep in a GEMM of its own.  The error is bounded against |P| |Q|^T = |A| |B|^T + |B| |A|^T, as for any GEMM of this library.
 *   - A == B (the same pointer) is allowed.
 *   - `work` holds gemmul8_work_size(is_complex, GEMMUL8_INT8, n, n, 2 kh, num_moduli, 0, 0, NULL, NULL) bytes: the equivalent GEMM's workspace.
 *   - alpha / beta host or device pointers, timers_ns, stream order and capture safety (timers_ns == NULL) as in gemmul8_syrk.
 *   - n == 0 or k == 0: GEMMUL8_OK, C untouched.  Bad uplo / trans, a null pointer, k > 2^16 (the equivalent GEMM's inner dimension 2 kh must stay
 *     <= 2^17): GEMMUL8_E_ARG, answered before any HIP call.
 *   - gemmul8_set_nonfinite_mode is ignored: the call behaves as mode 0.
 * No counterpart in the reference (it emulates GEMM only). */
GEMMUL8_API int gemmul8_syr2k(void *stream, int dtype, int backend, int uplo, int trans, size_t n, size_t k, const void *alpha, const void *A,
                              size_t lda, const void *B, size_t ldb, const void *beta, void *C, size_t ldc, unsigned num_moduli, int fastmode,
                              void *work, double *timers_ns);

/* Hermitian rank-2k update of one triangle: C = alpha*A*B^H + conj(alpha)*B*A^H + beta*C (trans = N, A and B are n x k) or
 * C = alpha*A^H*B + conj(alpha)*B^H*A + beta*C (trans = C, A and B are k x n).  dtype GEMMUL8_C / GEMMUL8_Z only (S / D: GEMMUL8_E_ARG); trans takes
 * 0 / 2 or the hipblasOperation_t values 111 / 113 (T, 1 / 112: GEMMUL8_E_ARG); uplo as in gemmul8_syrk.  alpha points to a COMPLEX scalar of the element
 * type, beta to a REAL one (float / double); both on the host or both on the device, detected as elsewhere.  INT8 backend only (GEMMUL8_FP8:
 * GEMMUL8_E_UNSUPPORTED -- the pair CRT is built for int8 residues).
 *   - The route: the second term is the conjugate transpose of the first.  With W = op(A) op(B)^H -- ONE ordinary GEMM over the full square, inner
 *     dimension k -- C_ij = alpha W_ij + conj(alpha W_ji) + beta C_ij.  A and B are scaled as that GEMM scales them (each keeps its own row shifts, every
 *     element is quantised once, k <= 2^17), and alpha is applied behind the CRT, where it costs no bits.
 *   - These are the bits.  Let W be what gemmul8_gemm(dtype, GEMMUL8_INT8, trans, trans == N ? C : N, n, n, k, 1, A, lda, B, ldb, 0, W, n, ...) writes in
 *     non-finite mode 0, W_ij = (x, y), W_ji = (u, v), the old C_ij = (cx, cy) [cy counts as 0 on the diagonal whatever the memory holds; (cx, cy) count as
 *     0 and are not read when beta == 0], alpha = (ar, ai).  In the element type, one rounding each:
 *         p = x + u,  q = y - v,  r = y + v,  t = x - u
 *         Re = fma(beta, cx, fma(-ai, r, ar * p))
 *         Im = fma(beta, cy, fma( ai, t, ar * q))        (diagonal: Im = +0.0)
 *   - No byte of the other strict triangle of C or of the ldc padding is read or written; beta == 0 never reads C.
 *   - A == B (the same pointer) is allowed.
 *   - `work` holds gemmul8_work_size(1, GEMMUL8_INT8, n, n, k, num_moduli, 0, 0, NULL, NULL) bytes: the equivalent GEMM's workspace.
 *   - timers_ns, stream order and capture safety (timers_ns == NULL) as in gemmul8_syrk.
 *   - n == 0 or k == 0: GEMMUL8_OK, C untouched.  Bad uplo / trans / dtype / backend, a null pointer, k > 2^17: GEMMUL8_E_ARG, answered before any HIP
 *     call; num_moduli out of the type's range: GEMMUL8_E_NUM_MODULI.
 *   - gemmul8_set_nonfinite_mode is ignored: the call behaves as mode 0.
 * No counterpart in the reference (it emulates GEMM only). */
GEMMUL8_API int gemmul8_her2k(void *stream, int dtype, int backend, int uplo, int trans, size_t n, size_t k, const void *alpha, const void *A,
                              size_t lda, const void *B, size_t ldb, const void *beta, void *C, size_t ldc, unsigned num_moduli, int fastmode,
                              void *work, double *timers_ns);

/* Product with a symmetric matrix of which ONE triangle is stored: C = alpha*A*B + beta*C (side = LEFT, A is m x m) or C = alpha*B*A + beta*C
 * (side = RIGHT, A is n x n); B and C are m x n, ka = the order of A.  All four types (the plain transpose for the complex types); side takes 0 / 1 or
 * the hipblasSideMode_t values 141 / 142, uplo as in gemmul8_syrk.  alpha and beta are of the element type, host or device, detected as elsewhere.
 * INT8 backend only (GEMMUL8_FP8: GEMMUL8_E_UNSUPPORTED -- the FP6 panel writer has no symmetric form).
 *   - The materialised matrix: Afull is the ka x ka matrix BLAS defines from the triangle named by uplo, Afull(i,j) = Afull(j,i) = the stored entry.
 *     gemmul8_hemm: the mirrored entry is the conjugate and the diagonal is the real part of the stored diagonal -- the stored imaginary part of a
 *     diagonal entry counts as 0, whatever the memory holds.  No byte of the other strict triangle of A or of the lda padding is ever read: a NaN there,
 *     or in HEMM's diagonal imaginary parts, reaches nothing.  Afull is never materialised: the scaling kernels read A through the triangle, in place.
 *   - Bit identity: the whole m x n window of C holds, bit for bit, what gemmul8_gemm puts there in non-finite mode 0 on the INT8 backend with Afull
 *     materialised --
 *       LEFT:   gemmul8_gemm(dtype, GEMMUL8_INT8, N, N, m, n, m, alpha, Afull, ka, B, ldb, beta, C, ldc, ...);
 *       RIGHT:  gemmul8_gemm(dtype, GEMMUL8_INT8, N, T, m, n, n, alpha, B, ldb, Afull, ka, beta, C, ldc, ...), gemmul8_hemm: the same with (N, C).
 *     Afull^T = Afull (HEMM: Afull^H = Afull), so the RIGHT form is BLAS's B*A.  It is stated with T / C because in both cases the symmetric operand
 *     then enters the scaling kernels in the ROW-STRIDED form: the fast mode's round-up sums depend on the lane an element lands in -- the only part of
 *     the scaling whose bits depend on the operand's form -- so both sides have ONE summation order to reproduce, the strided form's (lane ty of a row
 *     takes columns ty, ty + 32, ... ascending, then the width-32 tree).  In accurate mode the bits do not depend on the form (maxima, and per-element
 *     bytes given the shift; tests/test_symm_premise.py pins this on the oracle).
 *   - `work` holds gemmul8_work_size(is_complex, GEMMUL8_INT8, m, n, ka, num_moduli, 0, 0, NULL, NULL) bytes: the equivalent GEMM's workspace.
 *   - beta == 0 never reads C; no byte of the ldc padding is written; A and B are never written; C must not overlap A or B.
 *   - m == 0 or n == 0: GEMMUL8_OK, C untouched.  Bad side / uplo, a null pointer, ka > 2^17, dtype or backend out of range: GEMMUL8_E_ARG, answered
 *     before any HIP call; num_moduli out of the type's range: GEMMUL8_E_NUM_MODULI.
 *   - timers_ns, stream order and capture safety (timers_ns == NULL) as in gemmul8_gemm.
 *   - gemmul8_set_nonfinite_mode is ignored: the call behaves as mode 0.
 * No counterpart in the reference (it emulates GEMM only). */
enum { GEMMUL8_LEFT = 0, GEMMUL8_RIGHT = 1 };
GEMMUL8_API int gemmul8_symm(void *stream, int dtype, int backend, int side, int uplo, size_t m, size_t n, const void *alpha, const void *A,
                             size_t lda, const void *B, size_t ldb, const void *beta, void *C, size_t ldc, unsigned num_moduli, int fastmode,
                             void *work, double *timers_ns);
/* The same with a Hermitian A (see "the materialised matrix" above): dtype GEMMUL8_C / GEMMUL8_Z only (S / D: GEMMUL8_E_ARG -- BLAS has no real HEMM);
 * alpha and beta are COMPLEX scalars of the element type (unlike gemmul8_herk). */
GEMMUL8_API int gemmul8_hemm(void *stream, int dtype, int backend, int side, int uplo, size_t m, size_t n, const void *alpha, const void *A,
                             size_t lda, const void *B, size_t ldb, const void *beta, void *C, size_t ldc, unsigned num_moduli, int fastmode,
                             void *work, double *timers_ns);

/* Product with a triangular matrix: C = alpha*op(A)*B (side = LEFT, A is m x m) or C = alpha*B*op(A) (side = RIGHT, A is n x n); B and C are m x n,
 * ka = the order of A.  All four types; transA is N, T or C (0 / 1 / 2 or the hipblasOperation_t values 111 / 112 / 113; for the real types C is T), side
 * and uplo as in gemmul8_symm, diag GEMMUL8_NON_UNIT / GEMMUL8_UNIT or the hipblasDiagType_t values 131 / 132.  alpha is of the element type, host or
 * device, detected as elsewhere; there is no beta.  INT8 backend only (GEMMUL8_FP8: GEMMUL8_E_UNSUPPORTED -- the FP6 panel writer has no triangular form).
 *   - The materialised matrix: Atri is the ka x ka matrix BLAS defines -- the stored entries of the triangle named by uplo, exact zeros in the other strict
 *     triangle and, under GEMMUL8_UNIT, ones on the diagonal (the stored diagonal is then not read).  M = op(Atri), conjugated for C; Mt is the plain
 *     transpose of M.  No byte of the other strict triangle of A, of the lda padding or, under UNIT, of the diagonal is ever read: a NaN there reaches
 *     nothing.  Neither Atri nor M is ever materialised: the scaling kernels read A through the triangle, in place, and take the other half as zero
 *     without a load.
 *   - Bit identity: the whole m x n window of C holds, bit for bit, what gemmul8_gemm puts there in non-finite mode 0 on the INT8 backend with M
 *     materialised --
 *       LEFT:   gemmul8_gemm(dtype, GEMMUL8_INT8, N, N, m, n, m, alpha, M, ka, B, ldb, 0, C, ldc, ...);
 *       RIGHT:  gemmul8_gemm(dtype, GEMMUL8_INT8, N, T, m, n, n, alpha, B, ldb, Mt, ka, 0, C, ldc, ...).
 *     Stated this way for gemmul8_symm's reason: on either side and for every transA the triangular operand enters the scaling kernels in the
 *     ROW-STRIDED form, so the fast mode's round-up sums have one lane order to reproduce.  An element the plain kernel reads as an explicit zero of M
 *     either enters the same lane's sum in its place as a zero (produced without a load) or, where a column is zero for every row a workgroup handles,
 *     is absent from it: the sums are of non-negative terms rounded up, and x + 0 == x holds for them exactly.
 *   - The residue GEMMs run, for every 256 x 256 tile, only the 128-wide K-steps in which the tile's rows (LEFT) or columns (RIGHT) of M can hold a
 *     non-zero; a product of residues of zeros adds exactly 0 to an int32 accumulator, so no bit of the residue planes changes.
 *   - `work` holds gemmul8_work_size(is_complex, GEMMUL8_INT8, m, n, ka, num_moduli, 0, 0, NULL, NULL) bytes: the equivalent GEMM's workspace.
 *   - C is never read (its incoming bytes do not matter); no byte of the ldc padding is written; A is never written.  C == B with ldc == ldb is allowed
 *     -- the in-place form of classic BLAS: B is read in the scaling phase only and C is written by the CRT only, in stream order.  Any other overlap of
 *     C with A or B is the caller's error.
 *   - m == 0 or n == 0: GEMMUL8_OK, C untouched.  Bad side / uplo / transA / diag, a null pointer, ka > 2^17, dtype or backend out of range:
 *     GEMMUL8_E_ARG, answered before any HIP call; num_moduli out of the type's range: GEMMUL8_E_NUM_MODULI.
 *   - timers_ns, stream order and capture safety (timers_ns == NULL) as in gemmul8_gemm.
 *   - gemmul8_set_nonfinite_mode is ignored: the call behaves as mode 0.
 * No counterpart in the reference (it emulates GEMM only). */
enum { GEMMUL8_NON_UNIT = 0, GEMMUL8_UNIT = 1 };
GEMMUL8_API int gemmul8_trmm(void *stream, int dtype, int backend, int side, int uplo, int transA, int diag, size_t m, size_t n, const void *alpha,
                             const void *A, size_t lda, const void *B, size_t ldb, void *C, size_t ldc, unsigned num_moduli, int fastmode, void *work,
                             double *timers_ns);

/* Solve with a triangular matrix, in place: op(A) X = alpha B (side = LEFT, A is m x m) or X op(A) = alpha B (side = RIGHT, A is n x n); B is m x n and is
 * overwritten with X -- the in-place form of BLAS; ka = the order of A.  All four types; side, uplo, transA, diag and their spellings as in gemmul8_trmm;
 * alpha is of the element type.  INT8 backend only (GEMMUL8_FP8: GEMMUL8_E_UNSUPPORTED).  ka <= 2^17.
 *   - The result is a recipe, bit for bit.  M = op(Atri) (Atri: the stored triangle; under GEMMUL8_UNIT its diagonal is not read and counts as ones; transA = C
 *     conjugates an entry as it is read) is never materialised; M is lower triangular iff (uplo == LOWER) == (transA == N).  L = gemmul8_trsm_leaf().
 *     solve(M, Bblk, s) on a diagonal block of order r, with a pending scale s (the caller's alpha, or none):
 *       r <= L: the leaf solve below.  Otherwise h = the largest L * 2^j strictly below r, M11 is h x h, and B splits the same way (rows: LEFT, columns: RIGHT):
 *         LEFT,  M lower:  X1 = solve(M11, B1, s);  B2 = gemm(-1 * M21 * X1 + beta * B2);  X2 = solve(M22, B2, none)
 *         LEFT,  M upper:  X2 = solve(M22, B2, s);  B1 = gemm(-1 * M12 * X2 + beta * B1);  X1 = solve(M11, B1, none)
 *         RIGHT, M upper:  X1 first;  B2 = gemm(-1 * X1 * M12 + beta * B2);  then X2
 *         RIGHT, M lower:  X2 first;  B1 = gemm(-1 * X2 * M21 + beta * B1);  then X1
 *       beta = s where a scale is pending, else 1: the scale reaches every element of B exactly once, at its first touch.  Every gemm is gemmul8_gemm
 *       (GEMMUL8_INT8, this call's num_moduli and fastmode, non-finite mode 0) on the sub-matrix views; the off-diagonal block of M -- a rectangle inside the
 *       stored triangle -- is read where it lies in A, through op = transA.
 *     The leaf solve (order r <= L, one right-hand side; LEFT, M lower):
 *         for i = 0 .. r-1:  acc = s (x) b_i  (no scale pending: acc = b_i);  for j = 0 .. i-1 ascending: acc = acc (-) (m_ij (x) x_j);
 *                            x_i = acc (UNIT)  or  acc (/) m_ii (NON_UNIT)
 *       LEFT, M upper: i descending, j descending from r-1 to i+1.  RIGHT, M upper: x_j = (s b_j - sum_{i<j} x_i m_ij) / m_jj, j and i ascending.  RIGHT, M
 *       lower: both descending.  Every (x), (-), (/) is ONE correctly rounded IEEE operation of the element type; nothing is contracted into an FMA.  Complex
 *       types: the product is the textbook four products and two sums (ar*br - ai*bi, ar*bi + ai*br); the quotient is the textbook
 *       den = dr*dr + di*di; ((ar*dr + ai*di) / den, (ai*dr - ar*di) / den), each operation rounded once -- NOT scaled against overflow: unsafe for |m_ii|
 *       outside about 2^+-500 (Z) / 2^+-60 (C).  tests/trsm_util.py is this recipe in Python.
 *   - Bytes never read: no byte of the other strict triangle of A, of the lda padding or, under UNIT, of the diagonal -- a NaN there reaches nothing.
 *   - Bytes never written: A is never written; no byte of B outside the m x n window is written.  B must not overlap A.
 *   - alpha lives on the host or on the device, detected as elsewhere.  A HOST alpha equal to zero sets the window to +0 without reading A, as BLAS does.  A
 *     DEVICE alpha takes the recipe as it stands (a zero there multiplies: a NaN or Inf of B or A propagates); the constants -1 and 1 the GEMMs need beside
 *     it are written by a kernel, in stream order, into the 64-byte tail of `work`.
 *   - `work` holds gemmul8_trsm_work_size(is_complex, GEMMUL8_INT8, side, m, n, num_moduli) bytes: the maximum of gemmul8_work_size over the recipe's GEMMs
 *     (over both orientations of M: the size does not ask for uplo / transA), rounded up to a multiple of 64, plus the 64-byte tail.
 *   - timers_ns: four doubles; slots 0 / 1 / 3 are summed over the GEMMs, slot 2 holds the leaf solves (the slot that is always 0 elsewhere); one host
 *     synchronisation per GEMM and per leaf.  NULL: fully asynchronous and capture-safe.
 *   - A zero on a non-unit diagonal gives Inf / NaN, as IEEE division gives; nothing is checked.
 *   - m == 0 or n == 0: GEMMUL8_OK, nothing touched.  Argument errors and their order as in gemmul8_trmm, answered before any HIP call.
 *   - gemmul8_set_nonfinite_mode is ignored: the GEMMs behave as mode 0.
 * No counterpart in the reference (it emulates GEMM only). */
GEMMUL8_API size_t gemmul8_trsm_work_size(int is_complex, int backend, int side, size_t m, size_t n, unsigned num_moduli);
GEMMUL8_API int gemmul8_trsm_leaf(void); /* the leaf order L: 64 or 128, a build-time constant */
GEMMUL8_API int gemmul8_trsm(void *stream, int dtype, int backend, int side, int uplo, int transA, int diag, size_t m, size_t n, const void *alpha,
                             const void *A, size_t lda, void *B, size_t ldb, unsigned num_moduli, int fastmode, void *work, double *timers_ns);

/* D(i, j) += bias[i] for a column-major m x n real matrix: the broadcast bias of a hipblasLtMatmul BIAS epilogue, applied by the hook after
 * the emulated GEMM (one more rounding than the vendor's fused form).  S / D only.  No counterpart in the reference. */
GEMMUL8_API int gemmul8_add_row_bias(void *stream, int dtype, size_t m, size_t n, void *D, size_t ldd, const void *bias);

/* Multi-GPU exchange variant (A) of the moduli-sharded plan (include/gemmul8_dist.h): the rank's FP64 partial CRT sums over its
 * moduli [t_begin, t_end) -- C_mid points at plane t_begin -- as two double planes (hi: error-free chain, lo: rounded chain;
 * same FMAs and order as gemmul8_crt restricted to those moduli), written in column blocks of col_block columns, block b at
 * out + b * block_stride doubles, column c of a block at c * ld_out (the reduce-scatter unit of rank b); and the finish on the
 * SUMMED partials: mod-P reduction, scalbn, axpby as in gemmul8_crt.  No counterpart in the reference (it has no multi-GPU code);
 * the arithmetic is src/inverse_scaling_real.hpp:8-89 split at the accumulator. */
GEMMUL8_API int gemmul8_crt_partial(void *stream, int dtype, int backend, unsigned num_moduli, unsigned t_begin, unsigned t_end, size_t m,
                        size_t n, const void *C_mid, size_t ld_mid, size_t plane_stride, double *out_hi, double *out_lo,
                        size_t ld_out, size_t col_block, size_t block_stride);
GEMMUL8_API int gemmul8_crt_finish(void *stream, int dtype, int backend, unsigned num_moduli, size_t m, size_t n, const double *in_hi,
                       const double *in_lo, size_t ld_in, const int16_t *sftA, const int16_t *sftB, const void *alpha,
                       const void *beta, void *C, size_t ldc);

/* dst[i] += src[i], i < count, on FP64 arrays (16-byte aligned): the running sum of reduced partial planes when the fp64sum plan of
 * include/gemmul8_dist.h exchanges its partial sums in moduli groups (GEMMUL8_DIST_FP64_GROUPS).  No counterpart in the reference. */
GEMMUL8_API int gemmul8_add_f64(void *stream, double *dst, const double *src, size_t count);

/* FP8 backend, accurate mode: inflation of the bound GEMM's sums before the row / column maxima are taken.
 *   0 (default)  ku = 7 * 2^-13 + 4 (k+1) * 2^-24: covers how gfx950's v_mfma_scale_f32_16x16x128_f8f6f4 accumulates (products aligned
 *                to the largest of a group of 8 with 13 bits below it, truncating) -- with the reference's formula the bound can come
 *                out up to 1.2e-3 LOW, which can raise a shift by one and wrap the CRT;
 *                plus an absolute 7 kp 2^-14 (bound-plane units): a group of 8 products is aligned to the largest sum of the operands' exponent
 *                FIELDS, and an e4m3 subnormal carries the field of 2^-6 -- beside such a reference only 10 bits below the true largest product survive.
 *                Complex types: the mixed-sign product C0 = (|Ar|-|Ai|)(|Br|-|Bi|) of the bound of |Re C| is inflated by
 *                ku (|C0| + 2 (|Ar||Bi| + |Ai||Br|)) -- the engine's error on C0 scales with the magnitudes of its terms;
 *   1            ku = (k+1) * 2^-24, the reference's IEEE-FP32 summation bound (GEMMul8/src/find_max.hpp:82-96), and its ku C0 for complex;
 *   2            mode 0's ku with the reference's complex combination (the round-3 default; kept for tests/test_gpu_fp8_bound.py).
 * Process-wide; returns the previous mode (>= 0) or GEMMUL8_E_ARG.  The hook sets mode 1 when GEMMUL8_FP8_BOUND=reference. */
GEMMUL8_API int gemmul8_set_fp8_bound_mode(int mode);

/* Non-finite operands (NaN, +-Inf) in gemmul8_gemm and gemmul8_gemm_batched (and so gemmul8::gemm / gemmLt and the hook's direct paths).
 *   0 (default)  every operand is assumed finite; nothing defines what C holds when one is not (the reference's behaviour; the cheapest path).
 *   1 ("ieee")   BLAS-like propagation.  A row i of op(A) (m x k) is FLAGGED if one of its elements is NaN or +-Inf, a column j of op(B)
 *                (k x n) likewise; a complex element counts when either component does.
 *     1. clean entries (row i and column j unflagged) are bit-identical to the mode-0 result of the same call on A' and B': op(A) with every
 *        flagged row set to zero, op(B) with every flagged column set to zero.  A non-finite C under beta != 0 propagates through
 *        fma(beta, C, alpha AB) as in mode 0; beta == 0 does not read C.
 *     2. a flagged entry is alpha * s + fl(beta * C[i,j]) (alpha * s when beta == 0), s = the IEEE sum over k of op(A)[i,k] op(B)[k,j] in the
 *        element type (complex: the textbook componentwise products, conjugated per op, and the textbook product alpha * s).  Every such s is
 *        NaN or +-Inf, and its class does not depend on the order of the sum: NaN if a term is NaN, an Inf meets a 0, or +Inf and -Inf both
 *        occur; otherwise the sign of the infinite terms.  (Finite terms whose sum overflows are not covered.)
 *     3. alpha == 0 (also a device-resident alpha: tested on the device): A and B do not enter, C = beta * C everywhere.
 *     4. skip-scaling: the flags live in the shift arrays (gemmul8_layout.sftA / sftB hold INT16_MIN for a flagged row / column), so a
 *        cached operand keeps them with its planes and a call that reuses the cache behaves as if it had seen the operand again.
 *     5. no host synchronisation (stream-ordered, capture-safe) and no extra workspace: gemmul8_work_size and the layout do not change.
 *                Cost: one extra read of A and B (the flag launch) and one launch after the CRT that reads op(A)'s flagged rows against all of
 *                op(B) and op(B)'s flagged columns against all of op(A): (flagged rows x n + flagged columns x m) x k element pairs.
 * The phase-level entry points (gemmul8_scale*, gemmul8_lowprec_gemm, gemmul8_crt*) and the multi-GPU plans (include/gemmul8_dist.h, the
 * hook under GEMMUL8_DIST) ignore the mode and behave as mode 0.  Process-wide; returns the previous mode (>= 0) or GEMMUL8_E_ARG for anything
 * but 0 and 1.  The hook sets mode 1 when GEMMUL8_NONFINITE=ieee. */
GEMMUL8_API int gemmul8_set_nonfinite_mode(int mode);

/* What the hook does with a GEMM of this shape under the CURRENT value of GEMMUL8_MIN_FLOPS (oz2_hook.cpp below_floor): 1 = emulated,
 * 0 = handed to the native routine, GEMMUL8_E_ARG on bad arguments.  GEMMUL8_MIN_FLOPS unset, empty or 0: every selected call is emulated
 * (the reference's behaviour: its hook has no floor) -- always 1; "auto": the fitted cost model (tools/fit_floor.py,
 * profiles/sweeps/r04b_floor_scan_*.csv) decides per shape; a number: a plain floor on 2 m n k.  batch = items of a strided batch (1 for a
 * plain call).  No counterpart in the reference. */
GEMMUL8_API int gemmul8_hook_would_emulate(int dtype, int backend, size_t m, size_t n, size_t k, unsigned num_moduli, int fastmode,
                                           size_t batch);

/* 1 if `version` (a rocblas_get_version_string result) is a rocBLAS release the opt-in interposition of rocblas_internal_gemm_template
 * (GEMMUL8_HOOK_ROCBLAS=1; an internal, unversioned rocBLAS symbol) was tested with, else 0: with any other rocBLAS that symbol is passed
 * through untouched.  No counterpart in the reference (it hooks the hipBLAS names only). */
GEMMUL8_API int gemmul8_hook_rocblas_version_tested(const char *version);

/* Testing / A-B knobs (GEMMUL8_EPI_NT, _BOUND_TILE, _CPLX_BOUND_LAUNCHES, _CPLX_CHUNK, _CRT_KERNEL, _MAP_COLBLOCK; INTEGRATION.md
 * "Testing switches"): every one selects between bit-identical code paths.  They are parsed from the environment ONCE, at the first
 * launch; a test harness that changes the environment inside one process calls this afterwards.  No counterpart in the reference. */
GEMMUL8_API void gemmul8_reload_knobs(void);

/* Library identification (build arch, version) */
GEMMUL8_API const char *gemmul8_version(void);

#ifdef __cplusplus
}
#endif
#endif
