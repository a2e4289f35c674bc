// Mode 1 of gemmul8_set_nonfinite_mode ("ieee"): BLAS-like propagation of NaN / Inf operands (include/gemmul8_c.h).
//
// A row of op(A) (a column of op(B)) holding a NaN or an Inf is FLAGGED: its shift in sftA (sftB) becomes kNonfiniteSft.  Then
//   * the quantisers write zero planes for it (oz2_scale.hip, StageArgs::nf) and the accurate mode's bound planes of it are zero (flag
//     launch below, before the bound GEMM): the clean rows and columns see the operands A' / B' with the flagged ones set to zero;
//   * the CRT's scalbn(R, sftA[i] + sftB[j]) of the always-finite R is +-0 in every flagged entry, so the CRT leaves fl(beta * C) there
//     (C, 0 in its fast forms) -- no change to the CRT kernels;
//   * the patch launch after the CRT adds alpha * s, s = the IEEE sum over k of op(A)[i,k] op(B)[k,j], to every flagged entry.
// Neither launch reads anything back to the host: the grids come from the shapes, the flags live in the shift arrays (and so travel with
// skip-scaling's cached planes).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "oz2_kernels.h"

namespace oz2 {

namespace {

template <typename T> struct NF;
template <> struct NF<float> {
    using U = float;
    static constexpr bool cplx = false;
    __device__ static unsigned bad(float x) { return (__float_as_uint(x) & 0x7F800000u) == 0x7F800000u ? 1u : 0u; }
    __device__ static float re(float x) { return x; }
    __device__ static float im(float) { return 0.0f; }
};
template <> struct NF<double> {
    using U = double;
    static constexpr bool cplx = false;
    __device__ static unsigned bad(double x) { return ((unsigned)(__double_as_longlong(x) >> 32) & 0x7FF00000u) == 0x7FF00000u ? 1u : 0u; }
    __device__ static double re(double x) { return x; }
    __device__ static double im(double) { return 0.0; }
};
template <> struct NF<float2> {
    using U = float;
    static constexpr bool cplx = true;
    __device__ static unsigned bad(float2 x) { return NF<float>::bad(x.x) | NF<float>::bad(x.y); }
    __device__ static float re(float2 x) { return x.x; }
    __device__ static float im(float2 x) { return x.y; }
};
template <> struct NF<double2> {
    using U = double;
    static constexpr bool cplx = true;
    __device__ static unsigned bad(double2 x) { return NF<double>::bad(x.x) | NF<double>::bad(x.y); }
    __device__ static double re(double2 x) { return x.x; }
    __device__ static double im(double2 x) { return x.y; }
};

// ------------------------------------------------------------------ flag launch
struct FlagArgs {
    const void* X;
    size_t ld, rows, k, bx;
    int kmajor;
    int16_t* sft;
    int16_t* sft_keep;     // accurate mode: the scratch copy of the preliminary shifts (what the finalize folded into the quantise reads)
    int8_t* bound;         // accurate mode: bound plane(s), [rows][kp] bytes; nullptr in fast mode
    size_t kp, parts, part_stride;
    unsigned blocks;
    const void* const* xp;  // pointer-array batch: item z's operand is xp[z] (X and bx are not used)
};

constexpr unsigned kStridedRows = 32;  // row-strided operand: 32 rows x 8 k-lanes per workgroup

// the workgroup's rows are final here: publish the sentinel and zero the bound-plane rows of the flagged ones (exactly what A' / B' give)
__device__ __forceinline__ void flag_rows(const FlagArgs& o, size_t r0, const unsigned* fl, unsigned nrows, size_t zw) {
    for (unsigned q = 0; q < nrows; ++q) {
        if (!fl[q]) continue;  // (LDS value: uniform)
        const size_t r = r0 + q;
        if (threadIdx.x == 0) {
            ((int16_t*)((char*)o.sft + zw))[r] = kNonfiniteSft;
            if (o.sft_keep) ((int16_t*)((char*)o.sft_keep + zw))[r] = kNonfiniteSft;
        }
        if (o.bound) {
            for (size_t p = 0; p < o.parts; ++p) {
                uint4* row = (uint4*)(o.bound + zw + p * o.part_stride + r * o.kp);  // kp: a multiple of 256
                for (size_t w = threadIdx.x; w < o.kp / 16; w += 256) row[w] = uint4{0u, 0u, 0u, 0u};
            }
        }
    }
}

// PTR (the *_ptr_* kernels of a pointer-array batch, instantiations of their own: a loaded pointer is a generic one to the compiler and would turn the
// loads of every kernel into flat loads): item z's operand is o.xp[z] where the operand has an array
template <typename T, bool PTR = false> __device__ __forceinline__ void flag_body(const FlagArgs& o, unsigned bid, size_t bw) {
    __shared__ unsigned fl[kStridedRows];
    const size_t zw = (size_t)blockIdx.z * bw;
    const T* X = (const T*)((const char*)o.X + (size_t)blockIdx.z * o.bx);
    if constexpr (PTR)
        if (o.xp) X = (const T*)o.xp[blockIdx.z];
    if (o.kmajor) {  // one workgroup per row, lanes along k
        const size_t r = bid;
        const T* x = X + r * o.ld;
        unsigned bad = 0u;
        size_t kk = threadIdx.x;
        for (; kk + 768 < o.k; kk += 1024) {
            const T v0 = x[kk], v1 = x[kk + 256], v2 = x[kk + 512], v3 = x[kk + 768];
            bad |= NF<T>::bad(v0) | NF<T>::bad(v1) | NF<T>::bad(v2) | NF<T>::bad(v3);
        }
        for (; kk < o.k; kk += 256) bad |= NF<T>::bad(x[kk]);
        fl[0] = __syncthreads_or(bad) ? 1u : 0u;
        __syncthreads();
        flag_rows(o, r, fl, 1, zw);
        return;
    }
    // row-strided: element (r, kk) at X[kk * ld + r]; 32 consecutive rows per workgroup, 8 k-lanes
    const size_t r0 = (size_t)bid * kStridedRows;
    const unsigned rl = threadIdx.x & (kStridedRows - 1), kl = threadIdx.x / kStridedRows;
    if (threadIdx.x < kStridedRows) fl[threadIdx.x] = 0u;
    __syncthreads();
    const size_t r = r0 + rl;
    unsigned bad = 0u;
    if (r < o.rows) {
        const T* x = X + r;
        size_t kk = kl;
        for (; kk + 24 < o.k; kk += 32) {
            const T v0 = x[kk * o.ld], v1 = x[(kk + 8) * o.ld], v2 = x[(kk + 16) * o.ld], v3 = x[(kk + 24) * o.ld];
            bad |= NF<T>::bad(v0) | NF<T>::bad(v1) | NF<T>::bad(v2) | NF<T>::bad(v3);
        }
        for (; kk < o.k; kk += 8) bad |= NF<T>::bad(x[kk * o.ld]);
    }
    if (bad) fl[rl] = 1u;  // (benign race: every writer stores 1)
    __syncthreads();
    const unsigned nrows = (unsigned)(o.rows - r0 < kStridedRows ? o.rows - r0 : kStridedRows);
    flag_rows(o, r0, fl, nrows, zw);
}

template <typename T> __global__ void __launch_bounds__(256) flag_pair_kernel(const FlagArgs a, const FlagArgs b, size_t bw) {
    if (blockIdx.x < a.blocks) flag_body<T>(a, blockIdx.x, bw);
    else flag_body<T>(b, blockIdx.x - a.blocks, bw);
}
template <typename T> __global__ void __launch_bounds__(256) flag_ptr_pair_kernel(const FlagArgs a, const FlagArgs b, size_t bw) {
    if (blockIdx.x < a.blocks) flag_body<T, true>(a, blockIdx.x, bw);
    else flag_body<T, true>(b, blockIdx.x - a.blocks, bw);
}

// ------------------------------------------------------------------ patch launch
// Workgroups [0, nR): flagged rows of op(A); group (rg, cc) takes rows [256 rg, 256 rg + 256) and the 64 columns of chunk cc.
// Workgroups [nR, nR + nC): flagged columns of op(B); group (cg, rc) takes columns [256 cg, +256) and the 64 rows of chunk rc, except the
// flagged rows (the row groups own the entries where both are flagged).  A workgroup whose 256 shifts hold no sentinel returns after one load.
// Per flagged entry the four waves sum contiguous quarters of k, the quarters are added in LDS: the order of the sum is fixed but is not the
// order of any BLAS -- what the contract fixes is the class (NaN / +Inf / -Inf), which no order changes (finite overflow aside).
struct PatchArgs {
    const void* A;
    const void* B;
    void* C;
    size_t lda, ldb, ldc, m, n, k;
    int opA, opB;  // 0 = N, 1 = T, 2 = C
    const int16_t* sftA;
    const int16_t* sftB;
    double alpha[2];
    const void* alpha_dev;  // device-resident alpha (nullptr: the host value above)
    unsigned chunksN, chunksM, nR;
    size_t sa, sb, sc, bw;  // batched launch: bytes between the items' A, B, C, workspaces
    const void* const* pa;  // pointer-array batch (BatchCtx): a non-null array replaces base + z * stride for its operand
    const void* const* pb;
    void* const* pc;
};

// PTR = true: the instantiation of a pointer-array batch (a template parameter: see flag_body)
template <typename T, bool PTR = false> __global__ void __launch_bounds__(256) nonfinite_patch_kernel(const PatchArgs p) {
    using E = NF<T>;
    using U = typename E::U;
    __shared__ unsigned list[256];
    __shared__ unsigned cnt;
    __shared__ U red[2][4][64];
    U alr, ali;
    if (p.alpha_dev) {
        alr = ((const U*)p.alpha_dev)[0];
        ali = E::cplx ? ((const U*)p.alpha_dev)[1] : (U)0;
    } else {
        alr = (U)p.alpha[0], ali = (U)p.alpha[1];
    }
    if (alr == (U)0 && ali == (U)0) return;  // alpha == 0: A and B do not enter the result (the CRT left beta * C)
    const int16_t* sftA = (const int16_t*)((const char*)p.sftA + (size_t)blockIdx.z * p.bw);
    const int16_t* sftB = (const int16_t*)((const char*)p.sftB + (size_t)blockIdx.z * p.bw);
    const T* A = (const T*)((const char*)p.A + (size_t)blockIdx.z * p.sa);
    const T* B = (const T*)((const char*)p.B + (size_t)blockIdx.z * p.sb);
    U* C = (U*)((char*)p.C + (size_t)blockIdx.z * p.sc);
    if constexpr (PTR) {  // a pointer-array batch: the arrays replace base + z * stride, each on its own
        if (p.pa) A = (const T*)p.pa[blockIdx.z];
        if (p.pb) B = (const T*)p.pb[blockIdx.z];
        if (p.pc) C = (U*)p.pc[blockIdx.z];
    }
    const bool rowpart = blockIdx.x < p.nR;
    const unsigned bid = rowpart ? blockIdx.x : blockIdx.x - p.nR;
    const unsigned grp = bid / (rowpart ? p.chunksN : p.chunksM), chunk = bid - grp * (rowpart ? p.chunksN : p.chunksM);
    const size_t f = (size_t)grp * 256 + threadIdx.x;
    const size_t flen = rowpart ? p.m : p.n;
    if (threadIdx.x == 0) cnt = 0u;
    __syncthreads();
    if (f < flen && (rowpart ? sftA : sftB)[f] == kNonfiniteSft) list[atomicAdd(&cnt, 1u)] = (unsigned)threadIdx.x;
    __syncthreads();
    const unsigned nf = cnt;
    if (nf == 0) return;
    const unsigned lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const size_t o = (size_t)chunk * 64 + lane;  // the other index: a column (row part) or a row (column part)
    const size_t olen = rowpart ? p.n : p.m;
    const size_t kq = (p.k + 3) / 4, k0 = w * kq, k1 = k0 + kq < p.k ? k0 + kq : p.k;
    const bool cjA = p.opA == 2, cjB = p.opB == 2;
    for (unsigned q = 0; q < nf; ++q) {
        const size_t fi = (size_t)grp * 256 + list[q];
        const size_t i = rowpart ? fi : o, j = rowpart ? o : fi;
        // column part: a flagged row belongs to the row part
        const bool live = o < olen && (rowpart || sftA[i] != kNonfiniteSft);
        U sr = 0, si = 0;
        if (live) {
            for (size_t kk = k0; kk < k1; ++kk) {
                const T a = p.opA == 0 ? A[i + kk * p.lda] : A[kk + i * p.lda];
                const T b = p.opB == 0 ? B[kk + j * p.ldb] : B[j + kk * p.ldb];
                if constexpr (E::cplx) {
                    const U ar = E::re(a), ai = cjA ? -E::im(a) : E::im(a), br = E::re(b), bi = cjB ? -E::im(b) : E::im(b);
                    sr += ar * br - ai * bi;
                    si += ar * bi + ai * br;
                } else {
                    sr += a * b;
                }
            }
        }
        red[0][w][lane] = sr;
        red[1][w][lane] = si;
        __syncthreads();
        if (w == 0 && live) {
            const U s0 = ((red[0][0][lane] + red[0][1][lane]) + red[0][2][lane]) + red[0][3][lane];
            if constexpr (E::cplx) {
                const U s1 = ((red[1][0][lane] + red[1][1][lane]) + red[1][2][lane]) + red[1][3][lane];
                U* c = C + 2 * (i + j * p.ldc);
                const U cr = c[0], ci = c[1];
                c[0] = (alr * s0 - ali * s1) + cr;
                c[1] = (alr * s1 + ali * s0) + ci;
            } else {
                U* c = C + (i + j * p.ldc);
                *c = alr * s0 + *c;
            }
        }
        __syncthreads();
    }
}

template <typename T> hipError_t launch_flag_pair_t(hipStream_t stream, size_t k, const FlagOperand& A, const FlagOperand& B) {
    auto mk = [k](const FlagOperand& o) {
        FlagArgs f{};
        if (!o.rows) return f;
        f = FlagArgs{o.X, o.ld, o.rows, k, o.xstride, o.kmajor ? 1 : 0, o.sft, o.sft_keep, o.bound, o.kp, o.parts, o.part_stride, 0u, o.xptr};
        f.blocks = (unsigned)(o.kmajor ? o.rows : (o.rows + kStridedRows - 1) / kStridedRows);
        return f;
    };
    const FlagArgs a = mk(A), b = mk(B);
    if (a.blocks + b.blocks == 0) return hipSuccess;
    if (a.xp || b.xp) hipLaunchKernelGGL(flag_ptr_pair_kernel<T>, dim3(a.blocks + b.blocks, 1, g_batch.batch), dim3(256), 0, stream, a, b, g_batch.ws);
    else hipLaunchKernelGGL(flag_pair_kernel<T>, dim3(a.blocks + b.blocks, 1, g_batch.batch), dim3(256), 0, stream, a, b, g_batch.ws);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_flag_pair(hipStream_t stream, int dtype, size_t k, const FlagOperand& A, const FlagOperand& B) {
    if ((A.rows && A.kmajor && A.rows > 0x7FFFFFFFull) || (B.rows && B.kmajor && B.rows > 0x7FFFFFFFull) || A.rows + B.rows > 0x7FFFFFFFull)
        return hipErrorInvalidConfiguration;
    switch (dtype) {
    case kF32: return launch_flag_pair_t<float>(stream, k, A, B);
    case kF64: return launch_flag_pair_t<double>(stream, k, A, B);
    case kC32: return launch_flag_pair_t<float2>(stream, k, A, B);
    case kC64: return launch_flag_pair_t<double2>(stream, k, A, B);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_nonfinite_patch(hipStream_t stream, int dtype, int opA, int opB, size_t m, size_t n, size_t k, const void* alpha, bool alpha_on_device,
                                  const void* A, size_t lda, const void* B, size_t ldb, const int16_t* sftA, const int16_t* sftB, void* C, size_t ldc) {
    if (m == 0 || n == 0 || k == 0) return hipSuccess;
    PatchArgs p{};
    p.A = A, p.B = B, p.C = C;
    p.lda = lda, p.ldb = ldb, p.ldc = ldc, p.m = m, p.n = n, p.k = k;
    p.opA = opA, p.opB = opB;
    p.sftA = sftA, p.sftB = sftB;
    if (alpha_on_device) {
        p.alpha_dev = alpha;
    } else if (is_f32(dtype)) {
        p.alpha[0] = ((const float*)alpha)[0];
        if (is_complex(dtype)) p.alpha[1] = ((const float*)alpha)[1];
    } else {
        p.alpha[0] = ((const double*)alpha)[0];
        if (is_complex(dtype)) p.alpha[1] = ((const double*)alpha)[1];
    }
    p.chunksN = (unsigned)((n + 63) / 64);
    p.chunksM = (unsigned)((m + 63) / 64);
    const size_t nR = (m + 255) / 256 * p.chunksN, nC = (n + 255) / 256 * p.chunksM;
    if (nR + nC > 0x7FFFFFFFull) return hipErrorInvalidConfiguration;
    p.nR = (unsigned)nR;
    p.sa = g_batch.sa, p.sb = g_batch.sb, p.sc = g_batch.sc, p.bw = g_batch.ws;
    p.pa = g_batch.pa, p.pb = g_batch.pb, p.pc = g_batch.pc;
    const dim3 grid((unsigned)(nR + nC), 1, g_batch.batch);
    const bool ptr = p.pa || p.pb || p.pc;
#define OZ2_PATCH(T)                                                                                       \
    do {                                                                                                   \
        if (ptr) hipLaunchKernelGGL((nonfinite_patch_kernel<T, true>), grid, dim3(256), 0, stream, p);     \
        else hipLaunchKernelGGL((nonfinite_patch_kernel<T, false>), grid, dim3(256), 0, stream, p);        \
    } while (0)
    switch (dtype) {
    case kF32: OZ2_PATCH(float); break;
    case kF64: OZ2_PATCH(double); break;
    case kC32: OZ2_PATCH(float2); break;
    case kC64: OZ2_PATCH(double2); break;
#undef OZ2_PATCH
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace oz2
