// Internal launcher prototypes (host side) of the HIP kernels.  The public boundary is
// include/gemmul8_c.h (C ABI) and include/gemmul8.hpp (C++ API); nothing here is exported.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "oz2_device.hpp"
#include "oz2_knobs.hpp"

namespace oz2 {

enum DType { kF32 = 0, kF64 = 1, kC32 = 2, kC64 = 3 };
inline bool is_complex(int dt) { return dt >= 2; }
inline bool is_f32(int dt) { return dt == kF32 || dt == kC32; }
inline size_t padding256(size_t x) { return (x + 255) / 256 * 256; }
inline unsigned planes_of(int backend, int t) { return backend == kINT8 ? 1u : (t < 6 ? 2u : 3u); }
inline unsigned num_mat(int backend, unsigned N) {
    unsigned s = 0;
    for (unsigned t = 0; t < N; ++t) s += planes_of(backend, (int)t);
    return s;
}
ModTable make_mod_table(int backend);

// Batched calls (gemmul8_gemm_batched: the items of a strided batch as ONE set of launches).  Every launcher puts the item index in
// gridDim.z (the persistent GEMM kernels fold it into their tile index); item b works on workspace + b * ws and on operand + b *
// xstride (a launcher argument, 0 by default).  Set by the batched driver around the phase calls of one host thread.
struct BatchCtx {
    unsigned batch = 1;
    size_t ws = 0;                // bytes between the items' workspaces
    size_t sa = 0, sb = 0, sc = 0;  // bytes between the items' A, B, C
    // pointer-array batch (gemmul8_gemm_batched_ptr): a non-null array holds the items' operand addresses in DEVICE memory and replaces base + b * stride
    // for that operand.  Only kernels read the arrays (item blockIdx.z loads its own entry); the host never does, so nothing that the strided path decides
    // on the host from an operand's address (16-byte forms, the one-read extract) may be decided for such an operand.  The entries are not validated.
    const void* const* pa = nullptr;
    const void* const* pb = nullptr;
    void* const* pc = nullptr;
};
inline thread_local BatchCtx g_batch;

// ---- INT8 MFMA GEMM (oz2_gemm_i8.hip)
hipError_t launch_gemm_i8_mod(hipStream_t stream, const int8_t* A, const int8_t* B, size_t strideA, size_t strideB, size_t kp, size_t m,
                              size_t n, int t_begin, int t_end, int8_t* out, size_t ldo, size_t strideO, bool stream_out, int tri = 0, int krange = 0);
                              // stream_out: the planes are read next by the CRT pass only (non-temporal stores allowed, see the definition)
                              // tri (both launches): 1 / 2 = m == n and only the 256 x 256 tiles that touch the lower / upper triangle are computed
                              // (the triangular walk of oz2_gemm_common.hpp; the other tiles of `out` are not written)
                              // krange (both launches; KRange in oz2_gemm_common.hpp, tri == 0): every tile runs only the K-steps in which the triangular
                              // operand of gemmul8_trmm can be non-zero; all of `out` is written, with the bits of the full-K launch
hipError_t launch_gemm_i8_cplx(hipStream_t stream, const int8_t* A, const int8_t* B, size_t strideA, size_t strideB, size_t kp, size_t m,
                               size_t n, int t_begin, int t_end, const int8_t* rx, const int8_t* ry, size_t strideR, int8_t* out,
                               size_t ldo, size_t strideO, int tri = 0, int krange = 0);
hipError_t launch_gemm_i8_max(hipStream_t stream, int nseg, const int8_t* const* A, const int8_t* const* B, size_t kp, size_t m, size_t n,
                              int* rowmax, int* colmax, int mid_seg = 0);

// 128 x 128-tile form of the bound GEMM for products whose 256 x 256 tiles would not fill the chip (oz2_gemm_i8_small.hip)
hipError_t launch_gemm_i8_max_small(hipStream_t stream, int nseg, const int8_t* const* A, const int8_t* const* B, size_t kp, size_t m, size_t n,
                                    int* rowmax, int* colmax, int mid_seg = 0);

// ---- FP8 MFMA GEMM (oz2_gemm_f8.hip)
hipError_t launch_gemm_f8(hipStream_t stream, int which, const int8_t* A, const int8_t* B, size_t strideA, size_t strideB, size_t kp, size_t m,
                          size_t n, int t_begin, int t_end, int16_t* out, size_t ldo, size_t strideO, const int16_t* r0, const int16_t* r1,
                          size_t strideR, const int16_t* rx = nullptr, const int16_t* ry = nullptr);
// the same residue GEMMs on FP6 (e2m3) panel images of the operand planes (oz2_gemm_f6.hip): same `which`, same outputs, twice the matrix rate
hipError_t launch_gemm_f6(hipStream_t stream, int which, const int8_t* A, const int8_t* B, size_t strideA, size_t strideB, size_t kp, size_t m,
                          size_t n, int t_begin, int t_end, int16_t* out, size_t ldo, size_t strideO, const int16_t* r0, const int16_t* r1,
                          size_t strideR, const int16_t* rx = nullptr, const int16_t* ry = nullptr);
void set_f8_bound_mode(int mode);  // 0 = engine-safe inflation (default), 1 = the reference's (k+1) * 2^-24
int get_f8_bound_mode();
hipError_t launch_gemm_f8_max(hipStream_t stream, const int8_t* A, const int8_t* B, size_t kp, size_t k, size_t m, size_t n, int* rowmax,
                              int* colmax);
hipError_t launch_gemm_f8_bound_cplx(hipStream_t stream, int stage, const int8_t* A, const int8_t* B, size_t kp, size_t k, size_t m, size_t n,
                                     float* fbuf, size_t ldf, int* rowmax, int* colmax);

// ---- scale / quantise (oz2_scale.hip).  An operand has `rows` logical rows (m for A, n for B) of
// length k; K-major: element (r,kk) at X[r*ld+kk]; row-strided: X[kk*ld+r].  lo planes are
// [rows_pad][kp] int8, zero-filled for kk in [k,kp).
// zero `bytes` (a multiple of 4, 4-byte aligned) with a kernel: hipMemsetAsync nodes misbehave under HIP-graph replay on ROCm 7.2
// (tests/test_gpu_graph.py), and a kernel launch is cheaper on the host than the runtime's memset path
hipError_t launch_zero(hipStream_t stream, void* p, size_t bytes);
// gemmul8_symm / gemmul8_hemm: an operand in SYMMETRIC FORM has rows == k and its logical element (r, kk) is Afull(r, kk), the matrix BLAS defines from ONE
// stored triangle of a column-major array X: kSymLower: X[kk*ld + r] where r >= kk, else the mirrored X[r*ld + kk]; kSymUpper: X[kk*ld + r] where r <= kk,
// else X[r*ld + kk].  herm: the mirrored half is conjugated and the stored diagonal's imaginary part counts as 0.  No element of the other strict
// triangle is read.  Such an operand enters the kernels as a row-strided one (kmajor == false); INT8 planes, mode 0, a single GEMM.
//
// gemmul8_trmm: the TRIANGULAR form is the same descriptor with one of the kTri* bits set on kSymLower / kSymUpper (which triangle of X is stored).  Every
// (r, kk) region of the logical operand is then one of three things: taken from the stored address X[kk*ld + r], taken from the transposed address
// X[r*ld + kk], or ZERO without a load -- and the diagonal is the stored one or, with kTriUnit, 1 without a load:
//   kTriStored    live half = the stored side of the diagonal at the stored address (the operand is Atri), the mirrored side is zero;
//   kTriMirrored  live half = the mirrored side at the transposed address (the operand is Atri^T), the stored side is zero.
// herm is not used with the triangular form; a conjugated operand (op = C) sets the operand's own `conj` flag.
// No element of the other strict triangle of X is read in either case.
enum SymForm { kSymNone = 0, kSymLower = 1, kSymUpper = 2, kSymBase = 3, kTriStored = 4, kTriMirrored = 8, kTriAny = 12, kTriUnit = 16 };
// the triangular operand's live columns of row r: kk <= r (true) or kk >= r (false)
__host__ __device__ inline bool tri_live_below(int sym) { return ((sym & kSymBase) == kSymLower) == ((sym & kTriStored) != 0); }
// one operand of the accurate mode's extract launches; rows == 0 = absent (skip-scaling)
struct ExtractOperand {
    bool kmajor = false, conj = false;
    size_t rows = 0;
    const void* X = nullptr;
    size_t ld = 0;
    int8_t* lo = nullptr;      // bound plane(s)
    size_t part_stride = 0;    // complex: bytes between the |Re|, |Im|, |Re| - |Im| planes
    int16_t* sft0 = nullptr;   // preliminary shifts (workspace array) ...
    int16_t* sft0_keep = nullptr;  // ... and their scratch copy (what the finalize folded into the quantise launch reads)
    size_t xstride = 0;        // batched launch: bytes between the items' operands
    void* amax = nullptr;      // row-strided operand: `parts` partial row-maxima arrays, pstride elements apart
    unsigned parts = 1;
    size_t pstride = 0;
    bool one_read = false;     // row-strided operand: row maxima and bound plane from one read (no amax_pair_kernel pass, `amax` unused); needs extract_one_read_ok
    int sym = kSymNone;        // symmetric form (SymForm); keeps the two-pass form (not one_read)
    bool herm = false;
    const void* const* xptr = nullptr;  // pointer-array batch (BatchCtx::pa / pb): item z's operand is xptr[z], X and xstride are not used; never one_read
};
bool extract_one_read_ok(int dtype, int backend, size_t kp);  // the one-read form exists: real types, INT8 planes, a single GEMM, kp <= 8192
unsigned amax_parts_for(size_t rows, size_t k, size_t max_parts);
hipError_t launch_amax_pair(hipStream_t stream, int dtype, size_t k, const ExtractOperand& A, const ExtractOperand& B);  // row-strided operands that keep the row-maxima pass (not one_read)
hipError_t launch_extract_pair(hipStream_t stream, int dtype, int backend, size_t k, size_t kp, const ExtractOperand& A, const ExtractOperand& B, void* zero_p,
                               size_t zero_bytes);
hipError_t launch_shift_finalize(hipStream_t stream, int backend, unsigned N, size_t rowsA, const int* maxA, int16_t* sftA, size_t rowsB,
                                 const int* maxB, int16_t* sftB, bool nf = false);
// one operand of the quantise / fast-shift launches; rows == 0 = absent (skip-scaling: the cached planes and shifts are kept)
struct QuantOperand {
    bool kmajor = false, conj = false;
    size_t rows = 0;
    const void* X = nullptr;
    size_t ld = 0;
    int16_t* sft = nullptr;   // fast shift: written; quantise: read (negated final shifts)
    int8_t* lo = nullptr;
    size_t plane_stride = 0, part_stride = 0;
    size_t xstride = 0;       // batched launch: bytes between the items' operands
    size_t f6_rows = 0;       // FP8 backend: > 0 = write FP6 panel images (oz2_gemm_f6.hip) of a plane with this many image rows (A: mp, B: n)
    // accurate mode, quantise only: fin_max != nullptr folds the shift finalize into the launch -- the final shifts are derived from the preliminary
    // ones (fin_sft0: the scratch copy the extract kept) and the bound maxima, and published to `sft` by the launch itself
    const int16_t* fin_sft0 = nullptr;
    const int* fin_max = nullptr;
    float fin_log2P = 0.0f;
    bool nf = false;  // non-finite mode 1 (oz2_nonfinite.hip): a row whose shift is kNonfiniteSft gets zero planes (the finalize keeps the sentinel)
    // gemmul8_herk (complex types, INT8 planes, the only operand of its launch): lo2 != nullptr = the same read also writes the conjugate twin's Im and
    // Re + Im plane sets (the residues of -Im and Re - Im) to parts 1 and 2 of a second plane array with these strides; its part 0 is not written
    int8_t* lo2 = nullptr;
    size_t plane_stride2 = 0, part_stride2 = 0;
    int sym = kSymNone;  // symmetric form (SymForm): the launches that carry such an operand are the *_sym_pair kernels of oz2_scale.hip
    bool herm = false;
    const void* const* xptr = nullptr;  // pointer-array batch (BatchCtx::pa / pb): item z's operand is xptr[z], X and xstride are not used
};
// FP8 backend: the residue planes are FP6 panel images whenever B's last row block fits its share of the reference's plane size
// (16-row granules at 3/4 byte per element: n >= 45; 64 keeps whole wave tiles); GEMMUL8_FP8_PLANES=e4m3 keeps the e4m3 byte planes
inline bool f6_planes_ok(size_t n) { return n >= 64 && knobs().fp8_planes != 1; }
// both operands in ONE launch each (the A and B halves are independent; at launch-bound sizes every dispatch costs 5-10 us)
hipError_t launch_fast_shift_pair(hipStream_t stream, int dtype, int backend, unsigned N, size_t k, const QuantOperand& A, const QuantOperand& B);
hipError_t launch_quantise_pair(hipStream_t stream, int dtype, int backend, int t_begin, int t_end, size_t k, size_t kp, const QuantOperand& A,
                                const QuantOperand& B);

// ---- gemmul8_syr2k: the operand is the K-concatenation [A.X | S.X2] of two matrices of one form (A.kmajor) with A.rows rows, each k long and zero-filled
// to kp = padding256(k).  INT8 planes, mode 0, a single GEMM.  Plane rows are 2 kp bytes apart; an element of X goes to columns [0, kp) of A.lo and, the
// same bytes, to columns [kp, 2 kp) of S.lo2; an element of X2 the other way round: the planes of [X | X2] and of [X2 | X] from one read of X and of X2.
struct Seg2Planes {
    const void* X2 = nullptr;
    size_t ld2 = 0;
    int8_t* lo2 = nullptr;
    size_t plane_stride2 = 0, part_stride2 = 0;
};
// one shift per row of the concatenation, to A.sft: every lane runs its loop over X's row, then X2's -- the plain form's order on the materialised rows
hipError_t launch_fast_shift_seg2(hipStream_t stream, int dtype, unsigned N, size_t k, const QuantOperand& A, const Seg2Planes& S);
// row-strided operands: A.amax holds the partial row maxima of BOTH matrices (launch_amax_pair on (X, X2), A.parts arrays in all); K-major: in the kernel
hipError_t launch_extract_seg2(hipStream_t stream, int dtype, size_t k, size_t kp, const ExtractOperand& A, const Seg2Planes& S, void* zero_p, size_t zero_bytes);
hipError_t launch_quantise_seg2(hipStream_t stream, int dtype, int t_begin, int t_end, size_t k, size_t kp, const QuantOperand& A, const Seg2Planes& S);

// ---- non-finite mode 1 (gemmul8_set_nonfinite_mode; oz2_nonfinite.hip)
// the shift of a flagged row of op(A) / column of op(B) (one holding a NaN or an Inf): no mode-0 shift comes near it (a few thousand at most),
// and the CRT's scalbn(R, sftA[i] + sftB[j]) of the finite R is +-0 with it
constexpr int16_t kNonfiniteSft = INT16_MIN;
constexpr int kNonfiniteShift = -(int)kNonfiniteSft;  // the same as a (positive) row shift of the quantisers
// one operand of the flag launch; rows == 0 = absent (skip-scaling: the cached shifts keep their flags)
struct FlagOperand {
    bool kmajor = false;
    size_t rows = 0;
    const void* X = nullptr;
    size_t ld = 0;
    size_t xstride = 0;         // batched launch: bytes between the items' operands
    int16_t* sft = nullptr;     // the shifts (fast mode: final; accurate mode: preliminary) ...
    int16_t* sft_keep = nullptr;  // ... and, accurate mode, their scratch copy
    int8_t* bound = nullptr;    // accurate mode: bound plane(s), zeroed for a flagged row before the bound GEMM
    size_t kp = 0, parts = 0, part_stride = 0;
    const void* const* xptr = nullptr;  // pointer-array batch (BatchCtx::pa / pb): item z's operand is xptr[z], X and xstride are not used
};
// flags both operands in ONE launch: reads every element once; run after the shifts are written and before anything consumes them
hipError_t launch_flag_pair(hipStream_t stream, int dtype, size_t k, const FlagOperand& A, const FlagOperand& B);
// after the CRT: C[i,j] = alpha * s + C[i,j] for every entry in a flagged row or column (s: the IEEE sum of op(A)[i,:] op(B)[:,j]); ops 0/1/2
hipError_t launch_nonfinite_patch(hipStream_t stream, int dtype, int opA, int opB, size_t m, size_t n, size_t k, const void* alpha, bool alpha_on_device,
                                  const void* A, size_t lda, const void* B, size_t ldb, const int16_t* sftA, const int16_t* sftB, void* C, size_t ldc);

// ---- CRT accumulation + inverse scaling (oz2_crt.hip)
hipError_t launch_crt(hipStream_t stream, int dtype, int backend, unsigned N, size_t m, size_t n, const void* Cmid, size_t ld_mid,
                      size_t plane_stride, const int16_t* sftA, const int16_t* sftB, const void* alpha, const void* beta,
                      bool scalars_on_device, void* C, size_t ldc);
// the same for one triangle of a square C (tri: 1 = i >= j, 2 = i <= j; INT8 residues): the other strict triangle of C and the residue tiles
// behind it are neither read nor written; the entries of the triangle carry the bits launch_crt gives them.
// herm (complex types; gemmul8_herk): alpha / beta point to REAL scalars (host: widened to (alpha, 0), (beta, 0) here; device: one real each is read), an
// off-diagonal entry carries the bits launch_crt gives it with the widened scalars, a diagonal entry that real part and +0.0 -- its incoming imaginary
// part counts as 0 (a NaN there reaches neither component)
hipError_t launch_crt_tri(hipStream_t stream, int dtype, unsigned N, size_t n, int tri, const void* Cmid, size_t ld_mid, size_t plane_stride,
                          const int16_t* sftA, const int16_t* sftB, const void* alpha, const void* beta, bool scalars_on_device, void* C, size_t ldc,
                          bool herm = false);
// gemmul8_her2k (complex types, INT8 residues): C_mid holds the FULL square W = op(A) op(B)^H; every stored entry (i, j) of the triangle `tri` becomes
// alpha W_ij + conj(alpha W_ji) + beta C_ij from the reconstructed W_ij (shifts sftA[i] + sftB[j]) and W_ji (sftA[j] + sftB[i]) -- the formula and the
// tile-pair kernel are above crt_her2k_kernel.  alpha points to a COMPLEX scalar, beta to a REAL one (device: two values and one).  Diagonal: the incoming
// imaginary part counts as 0, +0.0 is stored.  The other strict triangle of C is neither read nor written; beta == 0 never reads C.
hipError_t launch_crt_her2k(hipStream_t stream, int dtype, unsigned N, size_t n, int tri, const void* Cmid, size_t ld_mid, size_t plane_stride,
                            const int16_t* sftA, const int16_t* sftB, const void* alpha, const void* beta, bool scalars_on_device, void* C, size_t ldc);

// ---- gemmul8_trsm (oz2_trsm.hip): the leaf solve of one diagonal block of M = op(Atri), of order r <= trsm_leaf_order(), against nrhs right-hand sides, in
// place.  A: element (0, 0) of the block in the stored array; B: the block's first row (left) or first column (!left) of the window.  scaled: every element
// of B is multiplied by alpha (host value or device pointer) before anything else.  Only the stored triangle lower_a of the block is addressed, and under
// `unit` not its diagonal.
int trsm_leaf_order();
hipError_t launch_trsm_leaf(hipStream_t stream, int dtype, bool left, bool lower_a, int transA, bool unit, unsigned r, size_t nrhs, const void* A, size_t lda,
                            void* B, size_t ldb, bool scaled, const void* alpha, bool alpha_on_device);
// -1 at tail, +1 at tail + 16 bytes, in the element type: the scalars of gemmul8_trsm's GEMMs beside a device-resident alpha
hipError_t launch_trsm_consts(hipStream_t stream, int dtype, void* tail);
hipError_t launch_trsm_zero_fill(hipStream_t stream, int dtype, size_t m, size_t n, void* B, size_t ldb);  // +0 over the m x n window

hipError_t launch_row_bias(hipStream_t stream, int dtype, size_t m, size_t n, void* D, size_t ldd, const void* bias);
hipError_t launch_add_f64(hipStream_t stream, double* dst, const double* src, size_t count);  // dst += src (16-byte aligned arrays)

// multi-GPU exchange variant (A): per-rank FP64 partial CRT sums + the finish on the summed partials (oz2_crt.hip)
hipError_t launch_crt_partial(hipStream_t stream, int dtype, int backend, unsigned N, unsigned t_begin, unsigned t_end, size_t m, size_t n,
                              const void* Cmid, size_t ld_mid, size_t plane_stride, double* out_hi, double* out_lo, size_t ld_out,
                              size_t col_block, size_t block_stride);
hipError_t launch_crt_finish(hipStream_t stream, int dtype, int backend, unsigned N, size_t m, size_t n, const double* in_hi,
                             const double* in_lo, size_t ld_in, const int16_t* sftA, const int16_t* sftB, const void* alpha,
                             const void* beta, bool scalars_on_device, void* C, size_t ldc);

}  // namespace oz2
