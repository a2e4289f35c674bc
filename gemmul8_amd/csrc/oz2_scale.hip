// Scale / quantise kernels of the Ozaki-II emulation for gfx950 (HBM-bound byte/integer work).
//
// Replaces (paths relative to /root/reference/GEMMul8/src):
//   extract (accurate mode, 7-bit bounds) scaling_accu_real.hpp:23-136, scaling_accu_complex.hpp:6-126
//   accurate-mode shift                   scaling_accu_real.hpp:6-18,142-226
//   fast-mode shift                       scaling_fast_real.hpp:6-49, find_max.hpp:258-341
//   quantise + all-moduli residues        scaling_fast_real.hpp:54-164, scaling_fast_complex.hpp:9-133,
//                                         scaling.hpp:99-280, mod.hpp:8-98,194-355,638-877
//
// Layout in HBM: plane = [rows padded to 256][kp] bytes, row r contiguous in k, zero-filled for
// k <= kk < kp.  A row-strided operand (A with op N, B with op T/C: element (r,kk) at X[kk*ld+r]) is
// read with lanes along r (coalesced), staged RAW through LDS and re-read with lanes along k, so
// that every store is 256 contiguous bytes per wave; a K-major operand needs no staging.  Each
// thread owns 4 consecutive k and emits one dword per plane (the reference's char4 granularity),
// num_moduli is a run-time loop bound (no per-N template instantiation).
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include <algorithm>
#include <type_traits>

#include "oz2_kernels.h"

namespace oz2 {

ModTable make_mod_table(int backend) {
    ModTable T;
    for (int t = 0; t < 20; ++t) {
        const int p = backend == kINT8 ? GEMMUL8_MODULI_INT8[t] : GEMMUL8_MODULI_FP8[t];
        T.mc[t].p = p;
        T.mc[t].invp = 1.0f / (float)p;
        unsigned c[16];
        long long pw = 1;
        for (int i = 0; i < 16; ++i) {
            c[i] = i < 15 ? (unsigned)(pw % p) : 0u;
            pw = (pw % p) * 256;
        }
        for (int i = 0; i < 4; ++i) {
            unsigned lo = 0, hi = 0;
            for (int j = 0; j < 4; ++j) {
                const unsigned cj = c[4 * i + j];
                lo |= (backend == kINT8 ? cj : (cj & 31u)) << (8 * j);
                hi |= (backend == kINT8 ? 0u : (cj >> 5)) << (8 * j);
            }
            T.mc[t].cb[i] = lo;
            T.mc[t].cbh[i] = hi;
        }
        auto pow2 = [p](int e) {  // 2^e mod p
            long long r = 1;
            for (int i = 0; i < e; ++i) r = (r * 2) % p;
            return (int)r;
        };
        T.mc[t].k56 = (unsigned)((p - pow2(56)) % p);
        T.mc[t].k120 = (unsigned)((p - pow2(120)) % p);
    }
    return T;
}

// ------------------------------------------------------------------ element traits
template <typename T> struct ET;
template <> struct ET<float> {
    using U = float;
    static constexpr bool cplx = false;
    __device__ static double re(float v) { return (double)v; }
    __device__ static double im(float) { return 0.0; }
    __device__ static float zero() { return 0.f; }
};
template <> struct ET<double> {
    using U = double;
    static constexpr bool cplx = false;
    __device__ static double re(double v) { return v; }
    __device__ static double im(double) { return 0.0; }
    __device__ static double zero() { return 0.0; }
};
template <> struct ET<float2> {
    using U = float;
    static constexpr bool cplx = true;
    __device__ static double re(float2 v) { return (double)v.x; }
    __device__ static double im(float2 v) { return (double)v.y; }
    __device__ static float2 zero() { return make_float2(0.f, 0.f); }
};
template <> struct ET<double2> {
    using U = double;
    static constexpr bool cplx = true;
    __device__ static double re(double2 v) { return v.x; }
    __device__ static double im(double2 v) { return v.y; }
    __device__ static double2 zero() { return make_double2(0.0, 0.0); }
};

template <typename U> __device__ __forceinline__ U wave_max(U v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const U o = __shfl_xor(v, off);
        v = o > v ? o : v;
    }
    return v;
}

// ------------------------------------------------------------------ stage kernel (extract / quantise)
enum { MODE_BOUND = 0, MODE_MOD = 1 };

// INT8 residue planes leave as one dword per lane and plane.  16-byte stores (a 4 x 4 dword transpose over the lane quads) measured slower, quantise pair
// 8192^2 x 14 planes 702 vs 672 us (profiles/archive/r03_hbm_ab.txt): the kernel is bound by VALU issue, not by its store pattern.
// K-major operands: a thread's 4 consecutive elements come as 16-byte non-temporal loads (672 -> 660 us against element-wise loads).

// Operand loads are non-temporal.  Plain loads measured: no gain where the operands would fit the Infinity Cache (8192^2 x 256 ... 2048, 4096^2), and -5 % of
// the whole call at 8192^2 x 1024, where they evict the operand planes the GEMMs are about to read.
// v[0..3] = x[k0 .. k0+3], zero beyond k: 16-byte loads when the four elements exist and start on a 16-byte boundary
// NT: non-temporal (the data is read once); false where the same workgroup re-reads the row right away (two-pass bound extract: with nt
// loads in the maxima pass the second pass went back to HBM -- ZGEMM 8192^3 bounds phase 2.58 -> 2.81 ms)
template <typename T, bool NT = true> __device__ __forceinline__ void load4(const T* x, size_t k0, size_t k, T (&v)[4]) {
    const T* p = x + k0;
    if (k0 + 4 <= k && (reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
        typedef unsigned V4 __attribute__((ext_vector_type(4)));
        constexpr int NQ = (int)(4 * sizeof(T) / 16);
        V4 r[NQ];
#pragma unroll
        for (int i = 0; i < NQ; ++i) r[i] = NT ? __builtin_nontemporal_load((const V4*)p + i) : ((const V4*)p)[i];
        __builtin_memcpy(v, r, sizeof(r));
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (k0 + e < k) ? p[e] : ET<T>::zero();
    }
}

struct StageArgs {
    const void* X;
    size_t ld;
    size_t rows, k, kp;
    int8_t* lo;
    size_t plane_stride;  // bytes between moduli planes (MODE_MOD)
    size_t part_stride;   // bytes between Re / Im / Re+Im plane sets
    const int16_t* sft;   // MODE_MOD: negated final shifts
    int16_t* sft0;        // MODE_BOUND: written (maxUFP - ilogb(amax))
    unsigned* zero_p;     // MODE_BOUND (first operand of extract_pair_kernel): the launch also zero-fills zero_words 32-bit words from here (the maxima arrays
    unsigned zero_words;  //   of the bounds phase: the bound GEMM's atomicMax targets) -- instead of a launch of its own
    int16_t* sft0_keep;   // MODE_BOUND: a second copy of sft0 in the scratch region (never overwritten by the final shifts: what the fused finalize reads)
    // MODE_MOD, accurate mode: the shift finalize (scaling_accu_real.hpp:6-18) folded into the quantise launch -- fin_max != nullptr: every workgroup
    // derives its rows' final shifts from (fin_sft0, fin_max) itself, the workgroup of a row's first k chunk stores the negated value to fin_out (= the
    // workspace's sft array, which `sft` then does not have to hold yet).  One launch less per accurate-mode call (4-5 us at launch-bound sizes).
    const int16_t* fin_sft0;
    const int* fin_max;
    int16_t* fin_out;
    float fin_log2P;
    int fin_float_max;
    const void* amax;     // MODE_BOUND, strided: per-row amax bit patterns (U-sized unsigned), amax_parts partial arrays amax_pstride elements apart
    unsigned amax_parts;  //   (round 6: amax_pair_kernel writes one array per k split, no atomics and no zero-fill; the extract takes their maximum)
    size_t amax_pstride;
    int backend;
    int conj;
    int t_begin, t_end;
    int sqrtp[6];
    ModTable mt;
    double pairP[10], pairInvP[10];  // MODE_MOD, float-domain residues: product of the moduli pair (t_begin + 2j, t_begin + 2j + 1) and RN(1 / it)
    size_t bx, bw;        // batched launch (gridDim.z items): bytes between the items' operands X / between their workspaces
    int f6;               // MODE_MOD, FP8 backend: 1 = the planes are FP6 panel images (oz2_gemm_f6.hip), 0 = e4m3 bytes, K-major rows
    unsigned f6_last;     // index of the plane's last 256-row block ...
    unsigned f6_rp_last;  // ... and its rows in the images (A: 256, B: its rows rounded up to 16)
    int nf;               // MODE_MOD, non-finite mode 1 (oz2_nonfinite.hip): a row whose shift is the sentinel gets zero planes, the finalize keeps it
    // MODE_MOD, quantise_twin_kernel (gemmul8_herk; complex types, INT8 planes): the conjugate twin's Im and Re+Im plane sets -- the residues of -Im and
    // of Re - Im of the SAME loaded elements -- go to parts 1 and 2 of a second plane array with strides of its own (its part 0 is not written)
    int8_t* lo2;
    size_t plane_stride2, part_stride2;
    // SEG2 kernels (gemmul8_syr2k; INT8 planes): the operand is the K-concatenation [X | X2] of two matrices of the same form, each k long and zero-filled
    // to kp (a multiple of 256: the seam).  Plane rows are `pitch` = 2 kp bytes apart; an element of segment s at k0 goes to column s kp + k0 of `lo` and,
    // the same bytes, to column (1 - s) kp + k0 of `lo2` (plane_stride2 / part_stride2): the planes of [X | X2] and of [X2 | X] from one read of each
    const void* X2;
    size_t ld2;
    size_t pitch;
    // pointer-array batch (gemmul8_gemm_batched_ptr; read by the *_ptr_* kernels only): non-null = item z's operand is xp[z] (device memory; X and bx are
    // not used).  Last, so that no other field moves.
    const void* const* xp;
};
// item blockIdx.z of a batched launch: every workspace pointer moves by bw, the operand by bx (both 0 for a single GEMM).  The offsets
// are applied at the few points of use: a modified COPY of the argument block lands in scratch memory (the quantise kernels ran 6x
// slower that way).
#define OZ2_ZW ((size_t)blockIdx.z * a.bw)
#define OZ2_ZX ((size_t)blockIdx.z * a.bx)
// The operand of item blockIdx.z.  PTR = false (every kernel but the *_ptr_* ones): X + z * bx, the only form those kernels hold.  PTR = true (the kernels of a
// pointer-array batch, instantiations of their own): from the pointer array when the operand has one (one wave-uniform load), else the strided rule.  A pointer
// loaded from memory is a generic one to the compiler, and merged into one expression with it the operand loads become flat loads: hence the instantiations.
// Item pointers are not validated.  OZ2_XB is used inside templates that have a `PTR` parameter.
template <bool PTR> __device__ __forceinline__ const char* item_base(const void* X, const void* const* xp, size_t bx) {
    if constexpr (PTR) return xp ? (const char*)xp[blockIdx.z] : (const char*)X + (size_t)blockIdx.z * bx;
    else return (const char*)X + (size_t)blockIdx.z * bx;
}
#define OZ2_XB(a_) item_base<PTR>((a_).X, (a_).xp, (a_).bx)
__device__ __forceinline__ int fused_final_shift(const StageArgs& a, size_t row, bool writer, size_t zw) {
    const int s0 = ((const int16_t*)((const char*)a.fin_sft0 + zw))[row];
    if (a.nf && s0 == kNonfiniteSft) {  // flagged row (non-finite mode 1): the sentinel stays
        if (writer) ((int16_t*)((char*)a.fin_out + zw))[row] = kNonfiniteSft;
        return kNonfiniteShift;
    }
    const int amax = ((const int*)((const char*)a.fin_max + zw))[row];  // INT8: int32 maximum; FP8: bit pattern of a non-negative float
    int f = 0;
    if (amax > 0) {
        const float l = __log2f(a.fin_float_max ? __int_as_float(amax) : __int2float_rn(amax));
        f = __float2int_rd(__fmaf_rd(-0x1.000006p-1f, l, a.fin_log2P));
    }
    const int16_t neg = (int16_t)(-(s0 + f));
    if (writer) ((int16_t*)((char*)a.fin_out + zw))[row] = neg;
    return -(int)neg;
}

// MODE_MOD: the (positive) shift of a row.  Plain form: the workspace's negated final shifts.  Fused finalize (a.fin_max): the same arithmetic as
// shift_finalize_kernel below on (sft0, bound maximum); `writer` (exactly one thread per row over the whole grid) publishes the negated final shift.
#define OZ2_ROW_SHIFT(a_, row_, writer_)                                                                                        \
    ((a_).fin_max == nullptr ? -(int)((const int16_t*)((const char*)(a_).sft + OZ2_ZW))[(row_)] : fused_final_shift((a_), (row_), (writer_), OZ2_ZW))


// FP8 residue planes: residues up to +-544 are split into 2-3 e4m3 planes of integers <= 16 (mod.hpp:159-189, 361-410)
__device__ __forceinline__ void put_fp8_planes(const StageArgs& a, int8_t* o, int t, const int (&rr)[4]) {
    if (t < 6) {
        const int sq = a.sqrtp[t];
        const float inv = 1.0f / (float)sq;
        float hi[4], lo[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) fp8_split_sq(rr[e], sq, inv, hi[e], lo[e]);
        *(unsigned*)o = fp8x2_from_floats(hi[0], hi[1]) | (fp8x2_from_floats(hi[2], hi[3]) << 16);
        *(unsigned*)(o + a.plane_stride) = fp8x2_from_floats(lo[0], lo[1]) | (fp8x2_from_floats(lo[2], lo[3]) << 16);
    } else {
        int hi[4], lo[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) fp8_split_kara(rr[e], hi[e], lo[e]);
        *(unsigned*)o = fp8x2_from_ints(hi[0], hi[1]) | (fp8x2_from_ints(hi[2], hi[3]) << 16);
        *(unsigned*)(o + a.plane_stride) = fp8x2_from_ints(lo[0], lo[1]) | (fp8x2_from_ints(lo[2], lo[3]) << 16);
        *(unsigned*)(o + 2 * a.plane_stride) =
            fp8x2_from_ints(hi[0] + lo[0], hi[1] + lo[1]) | (fp8x2_from_ints(hi[2] + lo[2], hi[3] + lo[3]) << 16);
    }
}

// FP6 panel images (oz2_gemm_f6.hip): the same integers as e2m3 codes, sign << 5 | |v|, four codes = 24 bits per lane.  A lane quad holds 16
// consecutive k of a row = 96 bits = three dwords of the 24-byte fragment of (row, K group): lane j < 3 of the quad assembles dword j from its
// own 24 bits and its right neighbour's (one quad-permute DPP move) and stores it at its own address o (f6_lane_addr below); lane 3 stores nothing.
__device__ __forceinline__ unsigned f6_code(int v) { return (unsigned)(v < 0 ? 32 - v : v); }
__device__ __forceinline__ void put_f6_word(int8_t* o, const int (&v)[4]) {
    const unsigned w = f6_code(v[0]) | (f6_code(v[1]) << 6) | (f6_code(v[2]) << 12) | (f6_code(v[3]) << 18);
    const unsigned nb = (unsigned)__builtin_amdgcn_update_dpp(0, (int)w, 0xF9, 0xF, 0xF, true);  // quad_perm [1, 2, 3, 3]
    const unsigned j = threadIdx.x & 3u;
    const unsigned d = (w >> (8u * j)) | (nb << (24u - 8u * j));
    if (j < 3u) *(unsigned*)o = d;
}
__device__ __forceinline__ void put_f6_planes(const StageArgs& a, int8_t* o, int t, const int (&rr)[4]) {
    int hi[4], lo[4];
    if (t < 6) {
        const int sq = a.sqrtp[t];
        const float inv = 1.0f / (float)sq;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float h, l;
            fp8_split_sq(rr[e], sq, inv, h, l);
            hi[e] = (int)h, lo[e] = (int)l;
        }
        put_f6_word(o, hi);
        put_f6_word(o + a.plane_stride, lo);
    } else {
        int sm[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) fp8_split_kara(rr[e], hi[e], lo[e]), sm[e] = hi[e] + lo[e];
        put_f6_word(o, hi);
        put_f6_word(o + a.plane_stride, lo);
        put_f6_word(o + 2 * a.plane_stride, sm);
    }
}
// byte offset, inside a plane, of the dword that THIS lane stores for the 16 k starting at k0 & ~15 of `row` (lane j = threadIdx.x & 3 holds
// k0 = (k0 & ~15) + 4 j): dword 3 h + j of the fragment (h = the half of the K group), see the image layout in oz2_gemm_f6.hip
__device__ __forceinline__ size_t f6_lane_offset(const StageArgs& a, size_t row, size_t k0) {
    const unsigned tb = (unsigned)(row >> 8), r = (unsigned)row & 255u;
    const unsigned kt = (unsigned)(k0 >> 7), qf = ((unsigned)k0 >> 5) & 3u, h = ((unsigned)k0 >> 4) & 1u;
    const unsigned d = 3u * h + (threadIdx.x & 3u);
    const unsigned rp = tb == a.f6_last ? a.f6_rp_last : 256u;
    const size_t panel = (size_t)tb * 256u * (a.kp / 4 * 3) + (size_t)kt * rp * 96u;
    const unsigned inner = d < 4u ? (qf * rp + r) * 16u + 4u * d : 64u * rp + ((qf >> 1) * 2u * rp + 2u * r + (qf & 1u)) * 8u + 4u * (d - 4u);
    return panel + inner;
}

// The same planes from residues kept as FLOATS (round 5).  The FP6 writer is VALU-bound (config 3: 3.0 ms against ~1.3 ms of memory time) and the retired integer
// form spent ~20 operations per value and modulus: residue (fma, mad, add), int -> float, split (mul, rint, fma), float -> int twice, two sign-magnitude
// codes (sub, cmp, select each), shifts and ors.  Every quantity here is an integer below 2^24, so the whole chain runs in fp32 with the SAME quotients:
//   residue  q = fma(R, RN(1/p), 1.5 * 2^23) - 1.5 * 2^23 (the very rounding of residue_from_small), r = fma(-q, p, R)              3
//   split    squares: hi = rint(r / s), lo = fma(-s, hi, r) (fp8_split_sq);  Karatsuba: hi = copysign(ceil(|r| / 16), r), lo = fma(-16, hi, r)   3
//   code     c = v < 0 ? 32 - v : v as a float (a negative zero stays a zero)                                                           3 per piece
//   word     ((c3 * 64 + c2) * 64 + c1) * 64 + c0 by three fma (exact: < 2^24), ONE float -> int conversion per four codes               1 per piece
// ~14 operations.  Bit-identical planes (the GPU parity tests and the fuzz sweep compare every code with the oracle's integers).
__device__ __forceinline__ float residue_wide_f(float Rf, const ModConst& mc, float pf) {
    const float q = fmaf(Rf, mc.invp, 12582912.0f) - 12582912.0f;
    float r = fmaf(-q, pf, Rf);
    if (!(mc.p & 1)) r = (r == -0.5f * pf) ? 0.5f * pf : r;  // (uniform) even p: a tie takes +p/2, as residue_from_small
    return r;
}
__device__ __forceinline__ float wrapping_f(float a, float pf, float hf) { return a > hf ? a - pf : (a < -hf ? a + pf : a); }
__device__ __forceinline__ void put_f6_word_f(int8_t* o, const float (&v)[4]) {
    float c[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) c[e] = v[e] < 0.0f ? 32.0f - v[e] : v[e];
    const unsigned w = (unsigned)fmaf(fmaf(fmaf(c[3], 64.0f, c[2]), 64.0f, c[1]), 64.0f, c[0]);
    const unsigned nb = (unsigned)__builtin_amdgcn_update_dpp(0, (int)w, 0xF9, 0xF, 0xF, true);  // quad_perm [1, 2, 3, 3]
    const unsigned j = threadIdx.x & 3u;
    const unsigned d = (w >> (8u * j)) | (nb << (24u - 8u * j));
    if (j < 3u) *(unsigned*)o = d;
}
__device__ __forceinline__ void put_f6_planes_f(const StageArgs& a, int8_t* o, int t, const float (&r)[4]) {
    float hi[4], lo[4];
    if (t < 6) {
        const float sq = (float)a.sqrtp[t], inv = 1.0f / sq;
#pragma unroll
        for (int e = 0; e < 4; ++e) hi[e] = rintf(r[e] * inv), lo[e] = fmaf(-sq, hi[e], r[e]);
        put_f6_word_f(o, hi);
        put_f6_word_f(o + a.plane_stride, lo);
    } else {
        float sm[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            hi[e] = copysignf(ceilf(fabsf(r[e]) * 0.0625f), r[e]);
            lo[e] = fmaf(-16.0f, hi[e], r[e]);
            sm[e] = hi[e] + lo[e];
        }
        put_f6_word_f(o, hi);
        put_f6_word_f(o + a.plane_stride, lo);
        put_f6_word_f(o + 2 * a.plane_stride, sm);
    }
}

// Quantise + all residues of four consecutive k in the FLOATING-POINT domain.  The quantise kernels are bound by VALU issue, not by HBM
// (profiles/archive/r03_hbm_ab.txt, r03_valu_rates.txt): the byte-wise integer path (retired) spent ~37 operations per element on trunc(x * 2^s) = +-M * 2^E and
// ~7.75 per residue (two v_dot4_u32_u8 over the bytes of M, sign correction, quotient step, packing).  Here:
//   xs = trunc(ldexp(x, s))                       2 FP64 operations per element; exact (a power-of-two scaling, then v_trunc_f64)
//   level 1, per PAIR of moduli, P = p_t * p_t+1:  R = fma(-rint(xs * RN(1/P)), P, xs)      3 FP64 operations per pair
//        q = rint(..) need not be the nearest integer: R = xs - q P is formed EXACTLY by the fma (an integer below 2^53) and
//        R == xs (mod P); |R| <= P/2 + 2 for |xs| < 2^53.  |xs| >= 2^53 (num_moduli > 15 only; wave-uniform test): |R| <= |xs| 2^-52
//        < 2^40, and one more step of the same form brings it to |R| <= P/2 + 1.
//   level 2, per modulus: a single-fma quotient on the SIGNED R (|R| < 2^20.2: exact in fp32):
//        qf = fma(float(R), RN(1/p), 1.5 * 2^23) rounds to 1.5 * 2^23 + q, q = rint(R / p) exactly (|R| * |RN(1/p) - 1/p| < 2^-4.9 / p
//        stays clear of the 1/(2p) tie distance of an odd p; p = 256 / 1024: a tie gives +-p/2, the same byte / fixed below);
//        its low 24 bits are 2^22 + q, so v_mad_i32_i24(bits, -p, R) = (R - q p) - p 2^22: the canonical residue in the low byte,
//        the full value after adding p << 22 (mod 2^32).
// ~10 operations per residue and 2 per element instead of ~14.7 and ~37: the kernels become HBM-bound.  Bit-identical planes
// (tests/test_gpu_parity.py and the fuzz sweep compare every byte with the oracle).
template <bool WIDE> __device__ __forceinline__ int residue_from_small(int Ri, float Rf, const ModConst& mc) {
    const float qf = fmaf(Rf, mc.invp, 12582912.0f);
    int r;
    asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(r) : "v"(__float_as_int(qf)), "s"(-mc.p), "v"(Ri));
    if constexpr (WIDE) {
        r += (int)((unsigned)mc.p << 22);
        if (!(mc.p & 1)) r = (r == -(mc.p >> 1)) ? (mc.p >> 1) : r;
    }
    return r;  // !WIDE: only the low byte is meaningful (the value is off by p * 2^22)
}

// TWIN (quantise_twin_kernel): out2 = the element's place in the twin's planes.  The twin's chain is the one a.conj selects, run on -xi: trunc, rint and the
// exact fma are odd functions under round-to-nearest, so its level-1 remainder is -I to the bit and only the level-2 quotient (whose magic-number sum rounds
// ties to even, and whose even-p tie is one-sided) is run again, on (-Ri, -Fi) -- the bytes a second pass over the operand with the other `conj` would write.
// SEG2 (the syr2k kernels): out2 = the element's place in the second plane array, which gets the SAME bytes, all three plane sets of a complex type.
template <typename T, bool TWIN = false, bool SEG2 = false> __device__ __forceinline__ void emit4_mod_float(const StageArgs& a, int8_t* out, [[maybe_unused]] int8_t* out2, const T (&v)[4], int s) {
    using E = ET<T>;
    double xr[4], xi[4];
    bool big = false;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        xr[e] = trunc(ldexp(E::re(v[e]), s));
        big |= fabs(xr[e]) >= 0x1.0p53;
        if constexpr (E::cplx) {
            xi[e] = trunc(ldexp(E::im(v[e]), s));
            if (a.conj) xi[e] = -xi[e];
            big |= fabs(xi[e]) >= 0x1.0p53;
        } else {
            xi[e] = 0.0;
        }
    }
    auto run = [&]<bool WIDE, bool BIG>() {
        for (int t = a.t_begin; t < a.t_end; t += 2) {
            const double P = a.pairP[(t - a.t_begin) >> 1], invP = a.pairInvP[(t - a.t_begin) >> 1];
            int Rr[4], Ri[4];
            float Fr[4], Fi[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                double R = fma(-rint(xr[e] * invP), P, xr[e]);
                if constexpr (BIG) R = fma(-rint(R * invP), P, R);
                Rr[e] = (int)R, Fr[e] = (float)R;
                if constexpr (E::cplx) {
                    double I = fma(-rint(xi[e] * invP), P, xi[e]);
                    if constexpr (BIG) I = fma(-rint(I * invP), P, I);
                    Ri[e] = (int)I, Fi[e] = (float)I;
                }
            }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int tt = t + u;
                if (tt >= a.t_end) break;
                const ModConst mc = a.mt.mc[tt];
                if constexpr (WIDE) {
                    if (a.f6) {  // (uniform) FP6 panel images from float residues: see put_f6_planes_f
                        const float pf = (float)mc.p, hf = (float)(mc.p >> 1);
                        float fr[4], fi[4], fs[4];
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            fr[e] = residue_wide_f(Fr[e], mc, pf);
                            if constexpr (E::cplx) fi[e] = residue_wide_f(Fi[e], mc, pf), fs[e] = wrapping_f(fr[e] + fi[e], pf, hf);
                        }
                        int8_t* o = out + (size_t)(tt < 6 ? 2 * tt : 12 + 3 * (tt - 6)) * a.plane_stride;
                        put_f6_planes_f(a, o, tt, fr);
                        if constexpr (E::cplx) {
                            put_f6_planes_f(a, o + a.part_stride, tt, fi);
                            put_f6_planes_f(a, o + 2 * a.part_stride, tt, fs);
                        }
                        continue;
                    }
                }
                int rr[4], ri[4], rs[4];
                [[maybe_unused]] int rn[4], rd[4];  // TWIN: the residues of -Im and of Re - Im
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    rr[e] = residue_from_small<WIDE>(Rr[e], Fr[e], mc);
                    if constexpr (E::cplx) {
                        ri[e] = residue_from_small<WIDE>(Ri[e], Fi[e], mc);
                        rs[e] = WIDE ? wrapping(rr[e] + ri[e], mc.p) : wrapping((int)(int8_t)rr[e] + (int)(int8_t)ri[e], mc.p);
                        if constexpr (TWIN && !WIDE) {
                            rn[e] = residue_from_small<WIDE>(-Ri[e], -Fi[e], mc);
                            rd[e] = wrapping((int)(int8_t)rr[e] + (int)(int8_t)rn[e], mc.p);
                        }
                    }
                }
                if constexpr (WIDE) {
                    int8_t* o = out + (size_t)(tt < 6 ? 2 * tt : 12 + 3 * (tt - 6)) * a.plane_stride;
                    if (a.f6) {  // never taken: FP6 panel images left through the float chain above.  The compiler drops the branch; the source keeps it because
                                 // deleting it renumbers basic blocks in the assembly listing, and the switch retirement was held to byte-identical listings
                        put_f6_planes(a, o, tt, rr);
                        if constexpr (E::cplx) {
                            put_f6_planes(a, o + a.part_stride, tt, ri);
                            put_f6_planes(a, o + 2 * a.part_stride, tt, rs);
                        }
                    } else {
                        put_fp8_planes(a, o, tt, rr);
                        if constexpr (E::cplx) {
                            put_fp8_planes(a, o + a.part_stride, tt, ri);
                            put_fp8_planes(a, o + 2 * a.part_stride, tt, rs);
                        }
                    }
                } else {
                    auto pack = [](const int (&r)[4]) {
                        return ((unsigned)r[0] & 0xFFu) | (((unsigned)r[1] & 0xFFu) << 8) | (((unsigned)r[2] & 0xFFu) << 16) | ((unsigned)r[3] << 24);
                    };
                    int8_t* o = out + (size_t)tt * a.plane_stride;
                    *(unsigned*)o = pack(rr);
                    if constexpr (E::cplx) {
                        *(unsigned*)(o + a.part_stride) = pack(ri);
                        *(unsigned*)(o + 2 * a.part_stride) = pack(rs);
                        if constexpr (TWIN) {
                            int8_t* o2 = out2 + (size_t)tt * a.plane_stride2;
                            *(unsigned*)(o2 + a.part_stride2) = pack(rn);
                            *(unsigned*)(o2 + 2 * a.part_stride2) = pack(rd);
                        }
                    }
                    if constexpr (SEG2) {
                        int8_t* o2 = out2 + (size_t)tt * a.plane_stride2;
                        *(unsigned*)o2 = pack(rr);
                        if constexpr (E::cplx) {
                            *(unsigned*)(o2 + a.part_stride2) = pack(ri);
                            *(unsigned*)(o2 + 2 * a.part_stride2) = pack(rs);
                        }
                    }
                }
            }
        }
    };
    const bool anybig = __any(big);
    if constexpr (TWIN || SEG2) {  // INT8 planes only
        if (anybig) run.template operator()<false, true>();
        else run.template operator()<false, false>();
        return;
    }
    if (a.backend == kFP8) {
        if (anybig) run.template operator()<true, true>();
        else run.template operator()<true, false>();
    } else {
        if (anybig) run.template operator()<false, true>();
        else run.template operator()<false, false>();
    }
}

template <typename T, int MODE, bool TWIN = false, bool SEG2 = false>
__device__ __forceinline__ void emit4(const StageArgs& a, size_t row, size_t k0, const T (&vin)[4], int s, [[maybe_unused]] unsigned seg = 0) {
    using E = ET<T>;
    if constexpr (SEG2) {  // INT8 planes at a pitch, written twice (k0: inside segment `seg`)
        int8_t* const o1 = a.lo + OZ2_ZW + row * a.pitch + (seg ? a.kp : 0) + k0;
        int8_t* const o2 = a.lo2 + OZ2_ZW + row * a.pitch + (seg ? 0 : a.kp) + k0;
        if constexpr (MODE == MODE_BOUND) {
            unsigned wr = 0, wi = 0, wd = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {  // the INT8 bound bytes of the plain form below
                auto ub = [&](double x) { return (int)ceil(ldexp(fabs(x), s)); };
                const int br = ub(E::re(vin[e]));
                wr |= ((unsigned)br & 0xFFu) << (8 * e);
                if constexpr (E::cplx) {
                    const int bi = ub(E::im(vin[e]));
                    wi |= ((unsigned)bi & 0xFFu) << (8 * e);
                    wd |= ((unsigned)(br - bi) & 0xFFu) << (8 * e);
                }
            }
            *(unsigned*)o1 = wr, *(unsigned*)o2 = wr;
            if constexpr (E::cplx) {
                *(unsigned*)(o1 + a.part_stride) = wi, *(unsigned*)(o2 + a.part_stride2) = wi;
                *(unsigned*)(o1 + 2 * a.part_stride) = wd, *(unsigned*)(o2 + 2 * a.part_stride2) = wd;
            }
        } else {
            emit4_mod_float<T, false, true>(a, o1, o2, vin, s);
        }
        return;
    }
    T v[4] = {vin[0], vin[1], vin[2], vin[3]};
    if (MODE == MODE_MOD && a.nf && s == kNonfiniteShift) {  // flagged row (non-finite mode 1): zero planes, the sentinel never reaches ldexp
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = E::zero();
        s = 0;
    }
    int8_t* out = a.lo + OZ2_ZW + ((MODE == MODE_MOD && a.f6) ? f6_lane_offset(a, row, k0) : row * a.kp + k0);
    if constexpr (MODE == MODE_BOUND) {
        if (a.backend == kFP8) {
            // e4m3 round-up of |x|*2^s (< 2^8), computed in the input precision (scaling.hpp:77-82); complex: planes
            // |Re|, |Im| and fp8_e4m3_ru(|Re| - |Im|) of the two rounded values (sub_ru_8bit, scaling_accu_complex.hpp:7-10:
            // the difference of two e4m3 numbers is exact in fp16/fp32; the helper's "+1 encoding step" is applied
            // literally, also for negative differences)
            using U = typename E::U;
            unsigned wr = 0, wi = 0, wd = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const U x = (U)E::re(v[e]);
                const U sc = sizeof(U) == 8 ? (U)scalbn(fabs((double)x), s) : (U)scalbnf(fabsf((float)x), s);
                const unsigned br = fp8_round_up<U>(sc);
                wr |= br << (8 * e);
                if constexpr (E::cplx) {
                    const U y = (U)E::im(v[e]);
                    const U sd = sizeof(U) == 8 ? (U)scalbn(fabs((double)y), s) : (U)scalbnf(fabsf((float)y), s);
                    const unsigned bi = fp8_round_up<U>(sd);
                    wi |= bi << (8 * e);
                    wd |= (fp8_round_up<float>(fp8_to_float(br) - fp8_to_float(bi)) & 0xFFu) << (8 * e);
                }
            }
            *(unsigned*)out = wr;
            if constexpr (E::cplx) {
                *(unsigned*)(out + a.part_stride) = wi;
                *(unsigned*)(out + 2 * a.part_stride) = wd;
            }
            return;
        }
        unsigned wr = 0, wi = 0, wd = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            // ceil(|x| * 2^s) in FP64 (v_ldexp_f64, v_ceil_f64, v_cvt_i32_f64: exact, the value is below 2^7 by construction of s) instead of
            // the ~25 integer operations of the bit-field form
            auto ub = [&](double x) { return (int)ceil(ldexp(fabs(x), s)); };
            const int br = ub(E::re(v[e]));
            wr |= ((unsigned)br & 0xFFu) << (8 * e);
            if constexpr (E::cplx) {
                const int bi = ub(E::im(v[e]));
                wi |= ((unsigned)bi & 0xFFu) << (8 * e);
                wd |= ((unsigned)(br - bi) & 0xFFu) << (8 * e);
            }
        }
        *(unsigned*)out = wr;
        if constexpr (E::cplx) {
            *(unsigned*)(out + a.part_stride) = wi;
            *(unsigned*)(out + 2 * a.part_stride) = wd;
        }
    } else {
        emit4_mod_float<T, TWIN>(a, out, TWIN ? a.lo2 + OZ2_ZW + row * a.kp + k0 : nullptr, v, s);
    }
}

// K-major operand: one 256-thread block per row; thread = 4 consecutive k per 1024-wide sweep
template <typename T, int MODE, bool TWIN = false, bool PTR = false>
__device__ __forceinline__ void stage_kmajor_body(const StageArgs& a, const unsigned bid) {
    using E = ET<T>;
    using U = typename E::U;
    if constexpr (MODE == MODE_MOD) {
        if (a.f6) {
            // FP6 panel images: one workgroup per (8 rows, one 128-element K-step), the K-step index fastest: the eight rows' 16-byte X slots and
            // 8-byte Y slot pairs of a K group are adjacent in the image, so every plane leaves as complete 128-byte lines (row by row, a K-step's
            // 96 bytes of one row are scattered over six lines that seven other rows complete later)
            const unsigned nks = (unsigned)(a.kp / 128);
            const unsigned rg = bid / nks;
            const size_t row = (size_t)rg * 8 + (threadIdx.x >> 5);
            const size_t k0 = (size_t)(bid - rg * nks) * 128 + (size_t)(threadIdx.x & 31) * 4;
            if (row >= a.rows) return;  // (uniform over the 32 lanes of a row)
            const T* x = (const T*)OZ2_XB(a) + row * a.ld;
            const int s = OZ2_ROW_SHIFT(a, row, bid == rg * nks && (threadIdx.x & 31) == 0);
            T v[4];
            load4<T>(x, k0, a.k, v);
            emit4<T, MODE, TWIN>(a, row, k0, v, s);
            return;
        }
    }
    if constexpr (MODE == MODE_MOD && sizeof(T) <= 8) {  // (16-byte elements measured 4 % better with the row loop)
        // quantise: one workgroup per 1024-wide k chunk of a row, the chunk index fastest: the workgroups in flight walk through
        // memory together (one row after the other) instead of streaming ~2000 rows at once
        const unsigned nch = (unsigned)(a.kp / 1024 + (a.kp % 1024 != 0));
        const size_t row = bid / nch;
        const size_t k0 = (size_t)(bid - row * nch) * 1024 + (size_t)threadIdx.x * 4;
        if (k0 >= a.kp) return;
        const T* x = (const T*)OZ2_XB(a) + row * a.ld;
        const int s = OZ2_ROW_SHIFT(a, row, k0 == 0);
        T v[4];
        load4<T>(x, k0, a.k, v);
        emit4<T, MODE, TWIN>(a, row, k0, v, s);
        return;
    }
    const size_t row = bid;
    const T* x = (const T*)OZ2_XB(a) + row * a.ld;
    int s;
    if constexpr (MODE == MODE_BOUND) {
        __shared__ U sm[4];
        // rows that fit NC x 1024 elements stay in registers between the amax pass and the extract pass: one read of the row
        constexpr int NC = sizeof(T) == 16 ? 4 : 8;
        if (a.kp <= (size_t)1024 * NC) {
            T vb[NC][4];
            U am = 0;
#pragma unroll
            for (int it = 0; it < NC; ++it) {
                const size_t k0 = (size_t)threadIdx.x * 4 + (size_t)it * 1024;
                load4<T>(x, k0, a.k, vb[it]);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const U ar = (U)fabs(E::re(vb[it][e])), ai = (U)fabs(E::im(vb[it][e]));
                    am = ar > am ? ar : am;
                    am = ai > am ? ai : am;
                }
            }
            am = wave_max(am);
            if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = am;
            __syncthreads();
            am = sm[0];
            am = sm[1] > am ? sm[1] : am;
            am = sm[2] > am ? sm[2] : am;
            am = sm[3] > am ? sm[3] : am;
            s = (a.backend == kINT8 ? 5 : 7) - ilogb0(am);
            if (threadIdx.x == 0) {
                ((int16_t*)((char*)a.sft0 + OZ2_ZW))[row] = (int16_t)s;
                if (a.sft0_keep) ((int16_t*)((char*)a.sft0_keep + OZ2_ZW))[row] = (int16_t)s;
            }
#pragma unroll
            for (int it = 0; it < NC; ++it) {
                const size_t k0 = (size_t)threadIdx.x * 4 + (size_t)it * 1024;
                if (k0 < a.kp) emit4<T, MODE, TWIN>(a, row, k0, vb[it], s);
            }
            return;
        }
        U am = 0;
        for (size_t k0 = (size_t)threadIdx.x * 4; k0 < a.k; k0 += 2048) {  // two 4-element groups in flight per thread
            T v0[4], v1[4];
            load4<T, false>(x, k0, a.k, v0);
            load4<T, false>(x, k0 + 1024 < a.k ? k0 + 1024 : k0, a.k, v1);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const U ar = (U)fabs(E::re(v0[e])), ai = (U)fabs(E::im(v0[e])), br = (U)fabs(E::re(v1[e])), bi = (U)fabs(E::im(v1[e]));
                am = ar > am ? ar : am;
                am = ai > am ? ai : am;
                am = br > am ? br : am;
                am = bi > am ? bi : am;
            }
        }
        am = wave_max(am);
        if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = am;
        __syncthreads();
        am = sm[0];
        am = sm[1] > am ? sm[1] : am;
        am = sm[2] > am ? sm[2] : am;
        am = sm[3] > am ? sm[3] : am;
        s = (a.backend == kINT8 ? 5 : 7) - ilogb0(am);
        if (threadIdx.x == 0) {
            ((int16_t*)((char*)a.sft0 + OZ2_ZW))[row] = (int16_t)s;
            if (a.sft0_keep) ((int16_t*)((char*)a.sft0_keep + OZ2_ZW))[row] = (int16_t)s;
        }
    } else {
        s = OZ2_ROW_SHIFT(a, row, threadIdx.x == 0);
    }
    for (size_t k0 = (size_t)threadIdx.x * 4; k0 < a.kp; k0 += 1024) {
        T v[4];
        load4<T>(x, k0, a.k, v);
        emit4<T, MODE, TWIN>(a, row, k0, v, s);
    }
}

// K-major operand of the SEG2 kernels (StageArgs::X2): row r of [X | X2] is row r of X, then row r of X2.  MODE_BOUND: one workgroup per row, the row's
// maximum over BOTH segments (one shift per row of the concatenation), then the bytes of both -- the two-pass form of stage_kmajor_body, the second pass
// re-reading what the first left in the cache.  MODE_MOD: the workgroups of stage_kmajor_body per segment, segment 0's chunks of a row first; a chunk starts
// at a multiple of 1024 inside its own segment, so none straddles the seam.
template <typename T, int MODE> __device__ __forceinline__ void stage_kmajor_seg2_body(const StageArgs& a, const unsigned bid) {
    using E = ET<T>;
    using U = typename E::U;
    const T* const X0 = (const T*)((const char*)a.X + OZ2_ZX);
    const T* const X1 = (const T*)((const char*)a.X2 + OZ2_ZX);
    if constexpr (MODE == MODE_MOD && sizeof(T) <= 8) {
        const unsigned nch = (unsigned)(a.kp / 1024 + (a.kp % 1024 != 0));
        const size_t row = bid / (2 * nch);
        unsigned ch = bid - (unsigned)row * 2 * nch;
        const unsigned seg = ch >= nch;
        ch -= seg * nch;
        const size_t k0 = (size_t)ch * 1024 + (size_t)threadIdx.x * 4;
        if (k0 >= a.kp) return;
        const T* x = seg ? X1 + row * a.ld2 : X0 + row * a.ld;
        const int s = OZ2_ROW_SHIFT(a, row, seg == 0 && k0 == 0);
        T v[4];
        load4<T>(x, k0, a.k, v);
        emit4<T, MODE, false, true>(a, row, k0, v, s, seg);
    } else {
        const size_t row = bid;
        const T* const x0 = X0 + row * a.ld;
        const T* const x1 = X1 + row * a.ld2;
        int s;
        if constexpr (MODE == MODE_BOUND) {
            __shared__ U sm[4];
            U am = 0;
            for (unsigned seg = 0; seg < 2; ++seg) {
                const T* x = seg ? x1 : x0;
                for (size_t k0 = (size_t)threadIdx.x * 4; k0 < a.k; k0 += 1024) {
                    T v[4];
                    load4<T, false>(x, k0, a.k, v);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const U ar = (U)fabs(E::re(v[e])), ai = (U)fabs(E::im(v[e]));
                        am = ar > am ? ar : am;
                        am = ai > am ? ai : am;
                    }
                }
            }
            am = wave_max(am);
            if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = am;
            __syncthreads();
            am = sm[0];
            am = sm[1] > am ? sm[1] : am;
            am = sm[2] > am ? sm[2] : am;
            am = sm[3] > am ? sm[3] : am;
            s = 5 - ilogb0(am);
            if (threadIdx.x == 0) {
                ((int16_t*)((char*)a.sft0 + OZ2_ZW))[row] = (int16_t)s;
                if (a.sft0_keep) ((int16_t*)((char*)a.sft0_keep + OZ2_ZW))[row] = (int16_t)s;
            }
        } else {
            s = OZ2_ROW_SHIFT(a, row, threadIdx.x == 0);
        }
        for (unsigned seg = 0; seg < 2; ++seg) {
            const T* x = seg ? x1 : x0;
            for (size_t k0 = (size_t)threadIdx.x * 4; k0 < a.kp; k0 += 1024) {
                T v[4];
                load4<T>(x, k0, a.k, v);
                emit4<T, MODE, false, true>(a, row, k0, v, s, seg);
            }
        }
    }
}

// Row-strided operand: 1-D grid of ceil(kp/TK) * ceil(rows/TR) workgroups, the row-tile index fastest (a 2-D grid would cap the
// row-tile count at 65535, i.e. operands of ~1M rows); 256 threads; tile TR rows x TK k staged RAW in LDS
template <typename T> struct StageTile {
    // 16.6 KiB of LDS per workgroup for every type (8 workgroups per CU): 32 rows x 128 k of float, 16 rows x 128 k of the 8-byte types (a 16-row read
    // segment of doubles is still one full 128-B cache line), 8 rows x 128 k of the 16-byte types (128-byte runs per row and plane on the way out; 16 rows x
    // 64 k = 64-byte runs measured slower)
#ifndef OZ2_STAGE_TR8
#define OZ2_STAGE_TR8 16  // rows per tile of the 8-byte element types
#endif
    static constexpr int TR = sizeof(T) == 4 ? 32 : sizeof(T) == 16 ? 8 : OZ2_STAGE_TR8;
    static constexpr int TK = 128;
};
// SEG2 (the syr2k kernels): twice the k tiles, those of X first, then those of X2; the row maxima (MODE_BOUND) are those of both matrices' partial arrays
template <typename T, int MODE, bool TWIN = false, bool SEG2 = false, bool PTR = false>
__device__ __forceinline__ void stage_strided_body(const StageArgs& a, const unsigned bid) {
    using E = ET<T>;
    using U = typename E::U;
    constexpr int TR = StageTile<T>::TR, TK = StageTile<T>::TK;
    constexpr int PITCH = TK + (sizeof(T) >= 16 ? 1 : 16 / sizeof(T));  // rows stay 16-B aligned
    constexpr int CH = TK / 4;                                          // 4-wide k chunks per row
    constexpr int RPP = 256 / CH;                                       // rows per pass
    __shared__ __attribute__((aligned(16))) T tile[TR][PITCH];
    using UBm = typename std::conditional<sizeof(U) == 8, unsigned long long, unsigned>::type;
    [[maybe_unused]] __shared__ UBm rowam[TR];
    // the row-tile index is the fast grid dimension: the workgroups in flight read whole columns (one sequential window of the operand) and write 4 adjacent
    // 128-byte runs per row and plane (k-tile index fastest: quantise A 314 vs 283 us)
    const unsigned nrt = (unsigned)((a.rows + TR - 1) / TR);
    const unsigned kt = bid / nrt, rt = bid - kt * nrt;
    const size_t r0 = (size_t)rt * TR;
    [[maybe_unused]] unsigned seg = 0;
    if constexpr (SEG2) seg = kt >= (unsigned)(a.kp / TK);
    const size_t kb = (size_t)(kt - seg * (unsigned)(a.kp / TK)) * TK;  // (inside the segment)
    const void* const Xs = SEG2 && seg ? a.X2 : a.X;
    const size_t ld = SEG2 && seg ? a.ld2 : a.ld;
    if constexpr (MODE == MODE_BOUND) {
        // row maxima of the tile's rows = the maximum over the k splits' partial arrays (amax_pair_kernel): 256 threads = TR rows x PL lanes, one
        // load per lane and partial (non-negative IEEE patterns order like unsigned integers), published to the passes below by the tile's barrier
        constexpr int PL = 256 / TR;
        const int rr = threadIdx.x / PL, pp = threadIdx.x % PL;
        UBm v = 0;
        if (r0 + rr < a.rows) {
            const UBm* am = (const UBm*)((const char*)a.amax + OZ2_ZW) + r0 + rr;
            for (unsigned q = pp; q < a.amax_parts; q += PL) {
                const UBm w = am[(size_t)q * a.amax_pstride];
                v = w > v ? w : v;
            }
        }
#pragma unroll
        for (int d = PL / 2; d >= 1; d >>= 1) {
            const UBm w = __shfl_xor(v, d);
            v = w > v ? w : v;
        }
        if (pp == 0) rowam[rr] = v;
    }
    if constexpr (sizeof(T) <= 8) {
        // 4- and 8-byte elements: a lane fetches RPL = 4 / 2 consecutive rows with one 16-byte load (a half / a quarter of the load
        // instructions, 1 KiB per wave instruction) when the rows exist and the group is 16-byte aligned; all loads of the tile are in
        // flight at once.  (float operands took the one-element-per-lane path until round 3: quantise A 222 us = 3.3 TB/s at 8192^2,
        // against 5.4 TB/s for double.)
        constexpr int RPL = 16 / (int)sizeof(T);
        constexpr int RP = TR / RPL;     // row groups per column
        constexpr int KY = 256 / RP;     // k values fetched per pass
        const int rp = threadIdx.x % RP, ky = threadIdx.x / RP;
        const size_t row = r0 + RPL * rp;
        const T* x = (const T*)(SEG2 ? (const char*)Xs + OZ2_ZX : OZ2_XB(a)) + row;
        const bool pair_ok = row + RPL - 1 < a.rows && ((reinterpret_cast<uintptr_t>(x) | (ld * sizeof(T))) & 15u) == 0;
        typedef unsigned V4 __attribute__((ext_vector_type(4)));
        V4 buf[TK / KY];
#pragma unroll
        for (int it = 0; it < TK / KY; ++it) {
            const size_t kg = kb + ky + KY * it;
            V4 v = {0u, 0u, 0u, 0u};
            if (kg < a.k) {
                if (pair_ok) {
                    v = __builtin_nontemporal_load((const V4*)(x + kg * ld));
                } else {
#pragma unroll
                    for (int e = 0; e < RPL; ++e) {
                        const T t = (row + e < a.rows) ? x[kg * ld + e] : E::zero();
                        __builtin_memcpy((char*)&v + e * sizeof(T), &t, sizeof(T));
                    }
                }
            }
            buf[it] = v;
        }
#pragma unroll
        for (int it = 0; it < TK / KY; ++it) {
            const int kk = ky + KY * it;
#pragma unroll
            for (int e = 0; e < RPL; ++e) __builtin_memcpy(&tile[RPL * rp + e][kk], (const char*)&buf[it] + e * sizeof(T), sizeof(T));
        }
    } else {
        constexpr int KY = 256 / TR;  // k values fetched per pass
        const int rx = threadIdx.x % TR, ky = threadIdx.x / TR;
        const size_t row = r0 + rx;
        const T* x = (const T*)(SEG2 ? (const char*)Xs + OZ2_ZX : OZ2_XB(a)) + row;
#pragma unroll 4
        for (int it = 0; it < TK / KY; ++it) {
            const int kk = ky + KY * it;
            const size_t kg = kb + kk;
            tile[rx][kk] = (row < a.rows && kg < a.k) ? x[kg * ld] : E::zero();
        }
    }
    __syncthreads();
    const int c = threadIdx.x % CH;
#pragma unroll 1
    for (int pass = 0; pass < TR / RPP; ++pass) {
        const int rl = pass * RPP + threadIdx.x / CH;
        const size_t row = r0 + rl;
        if (row >= a.rows) continue;
        int s;
        if constexpr (MODE == MODE_BOUND) {
            const UBm bits = rowam[rl];
            U am;
            __builtin_memcpy(&am, &bits, sizeof(U));
            s = (a.backend == kINT8 ? 5 : 7) - ilogb0(am);
            if (kt == 0 && c == 0) {
                ((int16_t*)((char*)a.sft0 + OZ2_ZW))[row] = (int16_t)s;
                if (a.sft0_keep) ((int16_t*)((char*)a.sft0_keep + OZ2_ZW))[row] = (int16_t)s;
            }
        } else {
            s = OZ2_ROW_SHIFT(a, row, kt == 0 && c == 0);
        }
        T v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = tile[rl][c * 4 + e];
        emit4<T, MODE, TWIN, SEG2>(a, row, kb + c * 4, v, s, seg);
    }
}

// Row-strided operand, MODE_BOUND, INT8 planes, real types: the bound plane from ONE read of the operand (no row-maxima pass before it).  One workgroup owns
// a panel of TR rows over all of k and walks its 128-wide k tiles in order, the raw loads of OZ2_PANEL_DEPTH tiles in flight.  A row's shift is only known after
// its last tile, so tile t is written with the PROVISIONAL shift s_t = 5 - ilogb0(maximum of the row over tiles 0 .. t) >= s0, and
//     ceil(ceil(y 2^d) / 2^d) = ceil(y)   (real y >= 0, integer d >= 0)
// turns a byte written with s_t = s0 + d into the byte of s0 exactly: a' = (a'' + 2^d - 1) >> d.  After the last tile the workgroup re-reads from the PLANE
// (an eighth of the operand's bytes, its own stores of a moment ago) the tiles of its rows that were written before a larger binade appeared, and nothing
// where every tile already held the row's top binade.  The steps E_t - E_(t-1) of the running exponent are kept per (row, tile) as one byte in LDS.
// (int)ceil(ldexp(|x|, s0)) departs from the real-number value only where ldexp is inexact or the maximum is not finite: rows with s0 + (smallest exponent of
// a nonzero element) < -1022 (a lower bound of that exponent is enough: a subnormal counts as 2^-1074) or with an infinite maximum are recomputed from a second
// read of the row with the final s0 -- by the code of the two-pass form, so that every byte and every shift is the two-pass form's for all inputs.
constexpr int kPanelMaxTiles = 64;  // k tiles per row of the step table (kp <= 8192); a longer k keeps the two-pass form (extract_one_read_ok)
#ifndef OZ2_PANEL_DEPTH
#define OZ2_PANEL_DEPTH 4  // tiles whose raw loads are in flight (16 registers each); 2 / 3 / 4 measured: DESIGN.md 3.4
#endif
template <typename T> __device__ __forceinline__ void stage_panel_body(const StageArgs& a, const unsigned bid) {
    static_assert(!ET<T>::cplx, "real operands");
    constexpr int TR = StageTile<T>::TR, TK = StageTile<T>::TK;
    constexpr int CH = TK / 4, RPP = 256 / CH, NP = TR / RPP;  // 4-wide k chunks per row, rows per pass, passes: thread (pass, threadIdx.x) owns the same (row, chunk) in every tile
    constexpr int RPL = 16 / (int)sizeof(T), RP = TR / RPL, KY = 256 / RP, NL = TK / KY;  // the load mapping of stage_strided_body
    constexpr int D = OZ2_PANEL_DEPTH;
    constexpr int kNone = INT_MIN;  // exponent of "no nonzero element yet"
    constexpr int PITCH = TK + 16 / (int)sizeof(T);  // rows stay 16-B aligned
    __shared__ __attribute__((aligned(16))) T tile[TR][PITCH];  // (a tile of its own: the strided body's array stays what every other kernel has)
    __shared__ unsigned char step[TR][kPanelMaxTiles];
    const unsigned nkt = (unsigned)(a.kp / TK);
    const size_t r0 = (size_t)bid * TR;
    const int rp = threadIdx.x % RP, ky = threadIdx.x / RP;
    const size_t lrow = r0 + RPL * rp;
    const T* X = (const T*)((const char*)a.X + OZ2_ZX);
    const T* x = X + lrow;
    const bool pair_ok = lrow + RPL - 1 < a.rows && ((reinterpret_cast<uintptr_t>(x) | (a.ld * sizeof(T))) & 15u) == 0;
    typedef unsigned V4 __attribute__((ext_vector_type(4)));
    const int c = threadIdx.x % CH, rg = threadIdx.x / CH;
    int ex[NP];                         // running exponent of the row maximum (every lane of the row's 32 holds it); NaN never wins, Inf is INT_MAX
    [[maybe_unused]] unsigned mnk[NP];  // this lane's smallest high word of a nonzero |x| (double)
#pragma unroll
    for (int p = 0; p < NP; ++p) ex[p] = kNone, mnk[p] = 0xFFFFFFFFu;
    // Pipelined walk (a condition uniform over the workgroup): every row of the panel exists and every 16-byte row group is aligned -- the loads of a tile that
    // lies inside k are then UNCONDITIONAL.  A load under a per-lane condition is merged with its other arm in the destination registers, and the compiler then waits for all
    // loads in flight (vmcnt(0)) before every such merge: no pipeline at all.  The k tail and ragged / unaligned panels take the guarded loads.
    const unsigned nfull = (unsigned)(a.k / TK);
    auto fetch_guarded = [&](unsigned t, V4 (&b)[NL]) {
#pragma unroll
        for (int it = 0; it < NL; ++it) {
            const size_t kg = (size_t)t * TK + ky + KY * it;
            V4 v = {0u, 0u, 0u, 0u};
            if (kg < a.k) {
                if (pair_ok) {
                    v = __builtin_nontemporal_load((const V4*)(x + kg * a.ld));
                } else {
#pragma unroll
                    for (int e = 0; e < RPL; ++e) {
                        const T q = (lrow + e < a.rows) ? x[kg * a.ld + e] : (T)0;
                        __builtin_memcpy((char*)&v + e * sizeof(T), &q, sizeof(T));
                    }
                }
            }
            b[it] = v;
        }
    };
    auto to_lds = [&](const V4 (&b)[NL]) {
#pragma unroll
        for (int it = 0; it < NL; ++it) {
            const int kk = ky + KY * it;
#pragma unroll
            for (int e = 0; e < RPL; ++e) __builtin_memcpy(&tile[RPL * rp + e][kk], (const char*)&b[it] + e * sizeof(T), sizeof(T));
        }
    };
    // tile t is in LDS: running exponents, the step table, the provisional bytes
    auto consume = [&]<bool FAST>(unsigned t) {
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const int rl = p * RPP + rg;
            T v[4];
            T lm = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                v[e] = tile[rl][c * 4 + e];
                const T ax = sizeof(T) == 8 ? (T)fabs((double)v[e]) : (T)fabsf((float)v[e]);
                lm = ax > lm ? ax : lm;
                if constexpr (sizeof(T) == 8) {
                    const unsigned hw = (unsigned)__double2hiint((double)ax);
                    mnk[p] = (v[e] != (T)0 && hw < mnk[p]) ? hw : mnk[p];
                }
            }
            int key = lm == (T)0 ? kNone : lm == (T)INFINITY ? INT_MAX : ilogb0(lm);
#pragma unroll
            for (int off = CH / 2; off > 0; off >>= 1) key = max(key, __shfl_xor(key, off));
            const int prev = ex[p];
            ex[p] = max(prev, key);
            if (c == 0) step[rl][t] = (unsigned char)(prev == kNone ? 0 : min(min(ex[p], 4096) - min(prev, 4096), 255));
            if (FAST || r0 + rl < a.rows) emit4<T, MODE_BOUND>(a, r0 + rl, (size_t)t * TK + c * 4, v, ex[p] == kNone ? 5 : 5 - min(ex[p], 4096));
        }
    };
    unsigned tdone = 0;  // tiles consumed by the pipelined loop
    if (r0 + TR <= a.rows && ((reinterpret_cast<uintptr_t>(X + r0) | (a.ld * sizeof(T))) & 15u) == 0) {
        auto fetch = [&](unsigned t, V4 (&b)[NL]) {
#pragma unroll
            for (int it = 0; it < NL; ++it) b[it] = __builtin_nontemporal_load((const V4*)(x + ((size_t)t * TK + ky + KY * it) * a.ld));
        };
        V4 buf[D][NL];
#pragma unroll
        for (int j = 0; j < D; ++j) {
#pragma unroll
            for (int it = 0; it < NL; ++it) buf[j][it] = V4{0u, 0u, 0u, 0u};
            if ((unsigned)j < nfull) fetch((unsigned)j, buf[j]);
        }
        for (unsigned t0 = 0; t0 < nfull; t0 += D) {
#pragma unroll
            for (int j = 0; j < D; ++j) {
                const unsigned t = t0 + j;
                if (t < nfull) {  // (uniform)
                    to_lds(buf[j]);
                    if (t + D < nfull) fetch(t + D, buf[j]);
                    __syncthreads();
                    consume.template operator()<true>(t);
                    __syncthreads();
                }
            }
        }
        tdone = nfull;
    }
    // the k tail (a partial tile, the zero tiles up to kp) and every tile of a ragged or unaligned panel: guarded loads, one tile at a time
    for (unsigned t = tdone; t < nkt; ++t) {
        V4 b[NL];
        fetch_guarded(t, b);
        to_lds(b);
        __syncthreads();
        consume.template operator()<false>(t);
        __syncthreads();
    }
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const int rl = p * RPP + rg;
        const size_t row = r0 + rl;
        if (row >= a.rows) continue;
        const int s0 = ex[p] == kNone ? 5 : ex[p] == INT_MAX ? 5 - ilogb0((T)INFINITY) : 5 - ex[p];  // = 5 - ilogb0(row maximum): ilogb is monotone
        if (c == 0) {
            ((int16_t*)((char*)a.sft0 + OZ2_ZW))[row] = (int16_t)s0;
            if (a.sft0_keep) ((int16_t*)((char*)a.sft0_keep + OZ2_ZW))[row] = (int16_t)s0;
        }
        bool hazard = ex[p] == INT_MAX;
        if constexpr (sizeof(T) == 8) {
            unsigned mk = mnk[p];
#pragma unroll
            for (int off = CH / 2; off > 0; off >>= 1) mk = min(mk, (unsigned)__shfl_xor((int)mk, off));
            const int emin = (mk >> 20) == 0 ? -1074 : (int)(mk >> 20) - 1023;  // a lower bound; NaN / Inf words never lower it
            hazard = hazard || (ex[p] != kNone && mk != 0xFFFFFFFFu && s0 + emin < -1022);
        }
        if (hazard) {  // (uniform over the row's 32 lanes)
            for (unsigned t = 0; t < nkt; ++t) {
                const size_t k0 = (size_t)t * TK + c * 4;
                T v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = (k0 + e < a.k) ? X[(k0 + e) * a.ld + row] : (T)0;
                emit4<T, MODE_BOUND>(a, row, k0, v, s0);
            }
            continue;
        }
        unsigned d = 0;  // s_t - s0 of tile t - 1
        for (int t = (int)nkt - 1; t >= 1; --t) {
            d = min(d + step[rl][t], 64u);
            if (d == 0) continue;
            unsigned* q = (unsigned*)(a.lo + OZ2_ZW + row * a.kp + (size_t)(t - 1) * TK + c * 4);
            const unsigned w = *q;  // four bytes <= 64 each: the per-byte sums below stay below 256
            *q = d >= 8 ? (((w + 0x7F7F7F7Fu) >> 7) & 0x01010101u) : (((w + ((1u << d) - 1u) * 0x01010101u) >> d) & ((0xFFu >> d) * 0x01010101u));
        }
    }
}

// accurate-mode extract (MODE_BOUND) of BOTH operands in one launch (round 6; workgroups [0, nA) work on a, the rest on b; either share may be empty).  The
// row maxima of row-strided operands come from amax_pair_kernel's partial arrays (no atomics, hence nothing to zero for them); the zero-fill of the bound GEMM's
// maxima arrays rides on this launch (zero_p / zero_words of `a`).
template <typename T> __global__ void __launch_bounds__(256) extract_pair_kernel(const StageArgs a, const StageArgs b, const unsigned nA, const int kmA, const int kmB) {
    if (a.zero_words) {
        unsigned* zp = (unsigned*)((char*)a.zero_p + OZ2_ZW);
        for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < a.zero_words; i += gridDim.x * 256u) zp[i] = 0u;
    }
    if (blockIdx.x < nA) {
        if (kmA) stage_kmajor_body<T, MODE_BOUND>(a, blockIdx.x);
        else stage_strided_body<T, MODE_BOUND>(a, blockIdx.x);
    } else {
        if (kmB) stage_kmajor_body<T, MODE_BOUND>(b, blockIdx.x - nA);
        else stage_strided_body<T, MODE_BOUND>(b, blockIdx.x - nA);
    }
}
// the same for a pointer-array batch (gemmul8_gemm_batched_ptr): instantiations of the bodies that take an item's operand from StageArgs::xp
template <typename T> __global__ void __launch_bounds__(256) extract_ptr_pair_kernel(const StageArgs a, const StageArgs b, const unsigned nA, const int kmA, const int kmB) {
    if (a.zero_words) {
        unsigned* zp = (unsigned*)((char*)a.zero_p + OZ2_ZW);
        for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < a.zero_words; i += gridDim.x * 256u) zp[i] = 0u;
    }
    if (blockIdx.x < nA) {
        if (kmA) stage_kmajor_body<T, MODE_BOUND, false, true>(a, blockIdx.x);
        else stage_strided_body<T, MODE_BOUND, false, false, true>(a, blockIdx.x);
    } else {
        if (kmB) stage_kmajor_body<T, MODE_BOUND, false, true>(b, blockIdx.x - nA);
        else stage_strided_body<T, MODE_BOUND, false, false, true>(b, blockIdx.x - nA);
    }
}
// The same launch when an operand takes the one-read form (real types).  Operand form (fA / fB): 0 = row-strided after amax_pair_kernel, 1 = K-major,
// 2 = row-strided from one read (stage_panel_body).  A kernel of its own: the panel body's registers (4 instead of 5 workgroups per CU) would otherwise be
// paid by every call of extract_pair_kernel, also where no operand takes the form (1024^3, launch-bound: +0.9 us measured with one kernel for both).
enum { FORM_STRIDED = 0, FORM_KMAJOR = 1, FORM_PANEL = 2 };
template <typename T> __device__ __forceinline__ void extract_body(const StageArgs& a, const unsigned bid, const int form) {
    if (form == FORM_KMAJOR) return stage_kmajor_body<T, MODE_BOUND>(a, bid);
    if (form == FORM_PANEL) return stage_panel_body<T>(a, bid);
    stage_strided_body<T, MODE_BOUND>(a, bid);
}
template <typename T> __global__ void __launch_bounds__(256) extract_panel_pair_kernel(const StageArgs a, const StageArgs b, const unsigned nA, const int fA, const int fB) {
    if (a.zero_words) {
        unsigned* zp = (unsigned*)((char*)a.zero_p + OZ2_ZW);
        for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < a.zero_words; i += gridDim.x * 256u) zp[i] = 0u;
    }
    if (blockIdx.x < nA) extract_body<T>(a, blockIdx.x, fA);
    else extract_body<T>(b, blockIdx.x - nA, fB);
}
// quantise (MODE_MOD) of BOTH operands in one launch: workgroups [0, nA) work on a, the rest on b; either share may be empty (skip-scaling,
// single-operand callers).  The two halves are independent and at launch-bound sizes each of them is a ~5-10 us dispatch (1024^3: 12.7 + 9.5 us,
// together ... see DESIGN.md 3.2); the form of each operand (K-major / row-strided) is a uniform run-time branch, registers and LDS are the
// maximum of the two forms (40 / 47 VGPRs, 0 / 16.6 KiB for double).
template <typename T> __global__ void __launch_bounds__(256) quantise_pair_kernel(const StageArgs a, const StageArgs b, const unsigned nA, const int kmA, const int kmB) {
    if (blockIdx.x < nA) {
        if (kmA) stage_kmajor_body<T, MODE_MOD>(a, blockIdx.x);
        else stage_strided_body<T, MODE_MOD>(a, blockIdx.x);
    } else {
        if (kmB) stage_kmajor_body<T, MODE_MOD>(b, blockIdx.x - nA);
        else stage_strided_body<T, MODE_MOD>(b, blockIdx.x - nA);
    }
}
// the same for a pointer-array batch
template <typename T> __global__ void __launch_bounds__(256) quantise_ptr_pair_kernel(const StageArgs a, const StageArgs b, const unsigned nA, const int kmA, const int kmB) {
    if (blockIdx.x < nA) {
        if (kmA) stage_kmajor_body<T, MODE_MOD, false, true>(a, blockIdx.x);
        else stage_strided_body<T, MODE_MOD, false, false, true>(a, blockIdx.x);
    } else {
        if (kmB) stage_kmajor_body<T, MODE_MOD, false, true>(b, blockIdx.x - nA);
        else stage_strided_body<T, MODE_MOD, false, false, true>(b, blockIdx.x - nA);
    }
}
// gemmul8_herk: ONE complex operand, whose every loaded element leaves as five plane sets -- Re, Im, Re + Im at a.lo as above, and the conjugate
// twin's -Im and Re - Im at a.lo2 (emit4_mod_float<T, true>): the planes of both sides of op(A) op(A)^H from one read of A
template <typename T> __global__ void __launch_bounds__(256) quantise_twin_kernel(const StageArgs a, const int km) {
    static_assert(ET<T>::cplx, "complex operands");
    if (km) stage_kmajor_body<T, MODE_MOD, true>(a, blockIdx.x);
    else stage_strided_body<T, MODE_MOD, true>(a, blockIdx.x);
}
// gemmul8_syr2k: ONE operand that is the K-concatenation of two matrices (StageArgs::X2), whose every loaded element leaves twice -- to the planes of
// [X | X2] at a.lo and, K halves swapped, to those of [X2 | X] at a.lo2: both sides of X X2^T + X2 X^T from one read of X and one of X2.  Kernels of
// their own, as the twin kernel is: extract_pair_kernel and quantise_pair_kernel keep their registers.
template <typename T> __global__ void __launch_bounds__(256) extract_seg2_kernel(const StageArgs a, const int km) {
    if (a.zero_words) {
        unsigned* zp = (unsigned*)((char*)a.zero_p + OZ2_ZW);
        for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < a.zero_words; i += gridDim.x * 256u) zp[i] = 0u;
    }
    if (km) stage_kmajor_seg2_body<T, MODE_BOUND>(a, blockIdx.x);
    else stage_strided_body<T, MODE_BOUND, false, true>(a, blockIdx.x);
}
template <typename T> __global__ void __launch_bounds__(256) quantise_seg2_kernel(const StageArgs a, const int km) {
    if (km) stage_kmajor_seg2_body<T, MODE_MOD>(a, blockIdx.x);
    else stage_strided_body<T, MODE_MOD, false, true>(a, blockIdx.x);
}
static_assert(2 * sizeof(StageArgs) + 16 <= 4096, "two argument blocks must fit the 4 KiB kernel-argument segment");

// ---- FP6 panel images of REAL operands: one lane = one fragment (round 5).  The generic stage kernels above give a lane four consecutive k; for the
// FP6 images that form is bound by VALU issue (config 3: 2.4 ms for 7 GB, ~19 operations per value and modulus, half of them the sign-magnitude codes,
// their 6-bit packing and the quad shuffle that assembles a dword).  Here a lane owns the 32 consecutive k of one row that make ONE fragment of the image
// (oz2_gemm_f6.hip: 16 bytes in the X region + 8 in the Y region), and gfx950 converts and packs them in hardware: v_cvt_scalef32_2xpk16_fp6_f32 takes
// two 16-float operands a, b and a scale and returns the 32 e2m3 codes of a[0]/scale, b[0]/scale, a[1]/scale, ... in six registers -- with scale 8 the code
// of an integer |v| <= 16 is sign << 5 | |v| (tools/ubench/cvt_fp6.hip; a negative zero keeps its sign bit: the same value for the MFMA).  What is left per
// value and modulus is the residue (3) and the split (3) in packed fp32 plus two FP64 operations per pair: the kernel runs at the HBM side.
//   * workgroup = 64 rows x one 128-element K-step, wave q = fragment column q: a wave's 64 X slots are one contiguous KiB, its Y slots 512 bytes in 8-byte pieces;
//   * row-strided operand (k strided by ld): lane = row, 32 coalesced loads; K-major operand: coalesced 16-byte loads of 8 rows x 128 bytes per instruction,
//     transposed through a wave-private LDS tile (row pitch 144 bytes: conflict-free 16-byte reads), 128 bytes of every row at a time.
typedef float v16f __attribute__((ext_vector_type(16)));
typedef unsigned v6u __attribute__((ext_vector_type(6)));
// (Complex operands take the generic stage kernels, four k per lane.  A complex form of this kernel was built in round 5 -- the fragment in two halves of 16 k,
// three plane sets per value -- and needs 282-314 registers: the 16-float operand tuples of the pack instruction with half their lanes as padding fragment
// the register file; one wave per SIMD: not kept.)
template <typename T, bool PTR = false> __device__ __forceinline__ void stage_f6_body(const StageArgs& a, const unsigned bid, const bool kmajor, char* tile /* this wave's 64 x 144 bytes */) {
    static_assert(!ET<T>::cplx, "real operands");
    constexpr int EPL = 16 / (int)sizeof(T);   // elements per 16-byte piece
    constexpr int CH = 128 / (int)sizeof(T);   // elements per 128-byte chunk of a row
    const unsigned lane = threadIdx.x & 63u, q = threadIdx.x >> 6;
    const unsigned nks = (unsigned)(a.kp / 128), nrb = (unsigned)((a.rows + 63) / 64);
    unsigned rb, kt;
    if (kmajor) rb = bid / nks, kt = bid - rb * nks;   // the workgroups in flight walk along the rows' memory
    else kt = bid / nrb, rb = bid - kt * nrb;           // ... down the columns'
    const size_t r0 = (size_t)rb * 64, row = r0 + lane, k0 = (size_t)kt * 128 + (size_t)q * 32;
    const T* X = (const T*)OZ2_XB(a);
    typedef unsigned V4 __attribute__((ext_vector_type(4)));
    T v[32];
    if (kmajor) {
        const unsigned pc = lane & 7u, pr = lane >> 3;
#pragma unroll
        for (int c = 0; c < 32 / CH; ++c) {
            V4 buf[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const size_t r = r0 + pr + 8 * j, kk = k0 + (size_t)c * CH + (size_t)pc * EPL;
                const T* src = X + r * a.ld + kk;
                V4 t = {0u, 0u, 0u, 0u};
                if (r < a.rows) {
                    if (kk + EPL <= a.k && (reinterpret_cast<uintptr_t>(src) & 15u) == 0) {
                        t = __builtin_nontemporal_load((const V4*)src);
                    } else {
                        T e[EPL];
#pragma unroll
                        for (int u = 0; u < EPL; ++u) e[u] = kk + u < a.k ? src[u] : ET<T>::zero();
                        __builtin_memcpy(&t, e, 16);
                    }
                }
                buf[j] = t;
            }
            if (c > 0) __builtin_amdgcn_wave_barrier();  // (the tile is re-used: every lane has read its row of the previous chunk -- LDS operations of a wave execute in order)
#pragma unroll
            for (int j = 0; j < 8; ++j) *(V4*)(tile + (pr + 8 * j) * 144 + pc * 16) = buf[j];
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const V4 t = *(const V4*)(tile + lane * 144 + i * 16);
                __builtin_memcpy(&v[c * CH + i * EPL], &t, 16);
            }
        }
    } else {
        const T* src = X + row;
#pragma unroll
        for (int kk = 0; kk < 32; ++kk) {
            const size_t kg = k0 + kk;
            v[kk] = (row < a.rows && kg < a.k) ? __builtin_nontemporal_load(src + kg * a.ld) : ET<T>::zero();
        }
    }
    if (row >= a.rows) return;
    int s = OZ2_ROW_SHIFT(a, row, k0 == 0);   // (k0 == 0: K-step 0, fragment column 0 -- one lane per row over the grid)
    if (a.nf && s == kNonfiniteShift) {  // flagged row (non-finite mode 1): zero planes
#pragma unroll
        for (int e = 0; e < 32; ++e) v[e] = ET<T>::zero();
        s = 0;
    }
    // xs = trunc(x 2^s): exact; a float operand's xs is a float again (24 significant bits), kept in 32 registers and widened pair by pair
    using XS = typename std::conditional<sizeof(T) == 4, float, double>::type;
    XS xs[32];
    bool big = false;
#pragma unroll
    for (int e = 0; e < 32; ++e) {
        if constexpr (sizeof(T) == 4) xs[e] = truncf(ldexpf(v[e], s));
        else xs[e] = trunc(ldexp((double)v[e], s));
        big |= fabs((double)xs[e]) >= 0x1.0p53;
    }
    // this lane's fragment in plane 0: X slot (q Rp + r), Y slot ((q >> 1) 2 Rp + 2 r + (q & 1))
    const unsigned tb = (unsigned)(row >> 8), r = (unsigned)row & 255u;
    const unsigned rp = tb == a.f6_last ? a.f6_rp_last : 256u;
    int8_t* const panel = a.lo + OZ2_ZW + (size_t)tb * 256u * (a.kp / 4 * 3) + (size_t)kt * rp * 96u;
    int8_t* const ox = panel + (size_t)(q * rp + r) * 16u;
    int8_t* const oy = panel + 64u * (size_t)rp + (size_t)((q >> 1) * 2u * rp + 2u * r + (q & 1u)) * 8u;
    auto put = [&](int plane, const float (&w)[32]) {
        v16f ev, od;
#pragma unroll
        for (int i = 0; i < 16; ++i) ev[i] = w[2 * i], od[i] = w[2 * i + 1];
        const v6u c = __builtin_amdgcn_cvt_scalef32_2xpk16_fp6_f32(ev, od, 8.0f);
        typedef unsigned V2 __attribute__((ext_vector_type(2)));
        *(V4*)(ox + (size_t)plane * a.plane_stride) = V4{c[0], c[1], c[2], c[3]};
        *(V2*)(oy + (size_t)plane * a.plane_stride) = V2{c[4], c[5]};
    };
    // (the loops over the 32 values are cut into groups of eight by scheduling barriers: left alone the scheduler interleaves all 32 chains and the
    // kernel needs 263 registers -- one wave per SIMD)
    auto run = [&]<bool BIG>() {
        for (int t = a.t_begin; t < a.t_end; t += 2) {
            const double P = a.pairP[(t - a.t_begin) >> 1], invP = a.pairInvP[(t - a.t_begin) >> 1];
            float Rf[32];
#pragma unroll
            for (int g8 = 0; g8 < 4; ++g8) {
#pragma unroll
                for (int e = 8 * g8; e < 8 * g8 + 8; ++e) {
                    const double x = (double)xs[e];
                    double R = fma(-rint(x * invP), P, x);
                    if constexpr (BIG) R = fma(-rint(R * invP), P, R);
                    Rf[e] = (float)R;
                }
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll 1
            for (int u = 0; u < 2; ++u) {
                const int tt = t + u;
                if (tt >= a.t_end) break;
                const ModConst mc = a.mt.mc[tt];
                const float pf = (float)mc.p;
                const bool even = !(mc.p & 1);  // (uniform; p = 1024 only) a tie takes +p/2
                const bool sqm = tt < 6;
                float lo[32], hi[32];
                // the residue of every value first (into lo): q = the quotient of residue_from_small, r = R - q p; for the one even modulus (p = 1024) a tie
                // (-p/2) takes +p/2 -- in a real branch (written as a select the compiler ran it for every modulus: a third of the block)
                if (even) {
                    asm volatile("" ::: "memory");
#pragma unroll
                    for (int e = 0; e < 32; ++e) {
                        const float qq = fmaf(Rf[e], mc.invp, 12582912.0f) - 12582912.0f;
                        const float rr = fmaf(-qq, pf, Rf[e]);
                        lo[e] = rr == -0.5f * pf ? 0.5f * pf : rr;
                    }
                } else {
#pragma unroll
                    for (int g8 = 0; g8 < 4; ++g8) {
#pragma unroll
                        for (int e = 8 * g8; e < 8 * g8 + 8; ++e) {
                            const float qq = fmaf(Rf[e], mc.invp, 12582912.0f) - 12582912.0f;
                            lo[e] = fmaf(-qq, pf, Rf[e]);
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
                if (sqm) {  // fp8_split_sq: hi = rint(r / s), lo = r - s hi
                    const float sq = (float)a.sqrtp[tt], inv = 1.0f / sq;
#pragma unroll
                    for (int g8 = 0; g8 < 4; ++g8) {
#pragma unroll
                        for (int e = 8 * g8; e < 8 * g8 + 8; ++e) {
                            hi[e] = rintf(lo[e] * inv);
                            lo[e] = fmaf(-sq, hi[e], lo[e]);
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    }
                } else {    // fp8_split_kara: hi = sign(r) ceil(|r| / 16), lo = r - 16 hi
#pragma unroll
                    for (int g8 = 0; g8 < 4; ++g8) {
#pragma unroll
                        for (int e = 8 * g8; e < 8 * g8 + 8; ++e) {
                            hi[e] = copysignf(ceilf(fabsf(lo[e]) * 0.0625f), lo[e]);
                            lo[e] = fmaf(-16.0f, hi[e], lo[e]);
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
                const int plane = sqm ? 2 * tt : 12 + 3 * (tt - 6);
                put(plane, hi);
                put(plane + 1, lo);
                if (!sqm) {
#pragma unroll
                    for (int e = 0; e < 32; ++e) hi[e] += lo[e];
                    put(plane + 2, hi);
                }
            }
        }
    };
    if (__any(big)) run.template operator()<true>();
    else run.template operator()<false>();
}
template <typename T> __global__ void __launch_bounds__(256) quantise_f6_pair_kernel(const StageArgs a, const StageArgs b, const unsigned nA, const int kmA, const int kmB) {
    __shared__ __attribute__((aligned(16))) char tile[4][64 * 144];
    char* const mine = tile[threadIdx.x >> 6];
    if (blockIdx.x < nA) stage_f6_body<T>(a, blockIdx.x, kmA != 0, mine);
    else stage_f6_body<T>(b, blockIdx.x - nA, kmB != 0, mine);
}
// the same for a pointer-array batch
template <typename T> __global__ void __launch_bounds__(256) quantise_f6_ptr_pair_kernel(const StageArgs a, const StageArgs b, const unsigned nA, const int kmA, const int kmB) {
    __shared__ __attribute__((aligned(16))) char tile[4][64 * 144];
    char* const mine = tile[threadIdx.x >> 6];
    if (blockIdx.x < nA) stage_f6_body<T, true>(a, blockIdx.x, kmA != 0, mine);
    else stage_f6_body<T, true>(b, blockIdx.x - nA, kmB != 0, mine);
}

// per-row amax of row-strided operands, BOTH operands in one launch (round 6): workgroup = 64 rows x one of `parts` k splits, 256 threads = 64 rows x 4 k-lanes;
// the maxima of split y go to the partial array y (amax + y * pstride): no atomics, nothing to zero; the extract takes the maximum over the splits.
struct AmaxOperand {
    const void* X;
    size_t ld, rows, bx;
    void* amax;
    size_t pstride;
    unsigned parts, row_groups;
};
// the operand of amax_ptr_pair_kernel (a pointer-array batch): non-null xp = item z's operand is xp[z].  A type of its own: AmaxOperand keeps its layout.
struct AmaxPtrOperand : AmaxOperand {
    const void* const* xp;
};
template <typename T, typename O = AmaxOperand> __device__ __forceinline__ void amax_strided_body(const O& o, const unsigned bid, size_t k, size_t bw) {
    const T* X;  // batched launch: item blockIdx.z
    if constexpr (std::is_same<O, AmaxPtrOperand>::value) X = (const T*)item_base<true>(o.X, o.xp, o.bx);
    else X = (const T*)((const char*)o.X + blockIdx.z * o.bx);
    using E = ET<T>;
    using U = typename E::U;
    using UB = typename std::conditional<sizeof(U) == 8, unsigned long long, unsigned>::type;
    UB* amax = (UB*)((char*)o.amax + blockIdx.z * bw);
    const unsigned by = bid / o.row_groups, bxr = bid - by * o.row_groups;  // the row group is the fast index: the workgroups in flight read whole columns
    const size_t rows = o.rows, ld = o.ld;
    // a lane owns RPL consecutive rows = 16 bytes of a column (one 16-byte load when they exist and are aligned); 64 rows per workgroup,
    // the remaining lanes spread over KL k-lanes
    constexpr int RPL = 16 / (int)sizeof(T);
    constexpr int LPC = 64 / RPL, KL = 256 / LPC;
    __shared__ U sm[KL][64];
    const int rl = threadIdx.x % LPC, ky = threadIdx.x / LPC;
    const size_t row0 = (size_t)bxr * 64 + (size_t)rl * RPL;
    const size_t kper = (k + o.parts - 1) / o.parts;
    const size_t kbeg = (size_t)by * kper, kend = (kbeg + kper < k) ? kbeg + kper : k;
    U am[RPL];
#pragma unroll
    for (int j = 0; j < RPL; ++j) am[j] = 0;
    auto take = [&](const T& v, int j) {
        const U ar = (U)fabs(E::re(v)), ai = (U)fabs(E::im(v));
        am[j] = ar > am[j] ? ar : am[j];
        am[j] = ai > am[j] ? ai : am[j];
    };
    if (row0 < rows) {
        const T* x = X + row0;
        const bool vec = RPL > 1 && row0 + RPL <= rows && ((reinterpret_cast<uintptr_t>(x) | (ld * sizeof(T))) & 15u) == 0;
        size_t kk = kbeg + ky;
        if (vec) {
            typedef unsigned V4 __attribute__((ext_vector_type(4)));
            for (; kk + 3 * KL < kend; kk += 4 * KL) {  // four strided 16-byte loads in flight per thread
                V4 raw[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) raw[u] = *(const V4*)(x + (kk + (size_t)KL * u) * ld);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    T v[RPL];
                    __builtin_memcpy(v, &raw[u], 16);
#pragma unroll
                    for (int j = 0; j < RPL; ++j) take(v[j], j);
                }
            }
            for (; kk < kend; kk += KL) {
                T v[RPL];
                const V4 raw = *(const V4*)(x + kk * ld);
                __builtin_memcpy(v, &raw, 16);
#pragma unroll
                for (int j = 0; j < RPL; ++j) take(v[j], j);
            }
        } else {
            for (; kk < kend; kk += KL) {
#pragma unroll
                for (int j = 0; j < RPL; ++j)
                    if (row0 + j < rows) take(x[kk * ld + j], j);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < RPL; ++j) sm[ky][rl * RPL + j] = am[j];
    __syncthreads();
    const size_t row = (size_t)bxr * 64 + threadIdx.x;
    if (threadIdx.x < 64 && row < rows) {
        U m = sm[0][threadIdx.x];
#pragma unroll
        for (int y = 1; y < KL; ++y) m = sm[y][threadIdx.x] > m ? sm[y][threadIdx.x] : m;
        UB bits;
        __builtin_memcpy(&bits, &m, sizeof(U));
        amax[(size_t)by * o.pstride + row] = bits;  // (an empty k split writes 0: the identity of the maximum)
    }
}
template <typename T> __global__ void __launch_bounds__(256) amax_pair_kernel(const AmaxOperand a, const AmaxOperand b, const unsigned nA, size_t k, size_t bw) {
    if (blockIdx.x < nA) amax_strided_body<T>(a, blockIdx.x, k, bw);
    else amax_strided_body<T>(b, blockIdx.x - nA, k, bw);
}
// the same for a pointer-array batch
template <typename T> __global__ void __launch_bounds__(256) amax_ptr_pair_kernel(const AmaxPtrOperand a, const AmaxPtrOperand b, const unsigned nA, size_t k, size_t bw) {
    if (blockIdx.x < nA) amax_strided_body<T, AmaxPtrOperand>(a, blockIdx.x, k, bw);
    else amax_strided_body<T, AmaxPtrOperand>(b, blockIdx.x - nA, k, bw);
}

template <typename T, int MODE> static size_t stage_blocks(bool kmajor, const StageArgs& a) {
    if (a.rows == 0) return 0;
    if (kmajor && MODE == MODE_MOD && a.f6) return ((a.rows + 7) / 8) * (a.kp / 128);
    if (kmajor) return a.rows * ((MODE == MODE_MOD && sizeof(T) <= 8) ? (a.kp + 1023) / 1024 : 1);
    return (a.kp / StageTile<T>::TK) * ((a.rows + StageTile<T>::TR - 1) / StageTile<T>::TR);
}
template <typename T> static hipError_t launch_quantise_stage(hipStream_t stream, bool kmA, const StageArgs& a, bool kmB, const StageArgs& b) {
    if constexpr (!ET<T>::cplx) {
        // real operands, FP6 panel images on both sides (an operand that is skipped has no rows): one lane per fragment
        if ((a.rows == 0 || a.f6) && (b.rows == 0 || b.f6) && (a.rows != 0 || b.rows != 0) && (a.rows ? a.backend : b.backend) == kFP8) {
            const size_t nA = a.rows ? ((a.rows + 63) / 64) * (a.kp / 128) : 0, nB = b.rows ? ((b.rows + 63) / 64) * (b.kp / 128) : 0;
            if (nA + nB > 0x7FFFFFFFull) return hipErrorInvalidConfiguration;
            if (a.xp || b.xp) hipLaunchKernelGGL(quantise_f6_ptr_pair_kernel<T>, dim3((unsigned)(nA + nB), 1, g_batch.batch), dim3(256), 0, stream, a, b, (unsigned)nA, (int)kmA, (int)kmB);
            else hipLaunchKernelGGL(quantise_f6_pair_kernel<T>, dim3((unsigned)(nA + nB), 1, g_batch.batch), dim3(256), 0, stream, a, b, (unsigned)nA, (int)kmA, (int)kmB);
            return hipGetLastError();
        }
    }
    const size_t nA = stage_blocks<T, MODE_MOD>(kmA, a), nB = stage_blocks<T, MODE_MOD>(kmB, b);
    if (nA + nB == 0) return hipSuccess;
    if (nA + nB > 0x7FFFFFFFull) return hipErrorInvalidConfiguration;
    if (a.xp || b.xp) hipLaunchKernelGGL(quantise_ptr_pair_kernel<T>, dim3((unsigned)(nA + nB), 1, g_batch.batch), dim3(256), 0, stream, a, b, (unsigned)nA, (int)kmA, (int)kmB);
    else hipLaunchKernelGGL(quantise_pair_kernel<T>, dim3((unsigned)(nA + nB), 1, g_batch.batch), dim3(256), 0, stream, a, b, (unsigned)nA, (int)kmA, (int)kmB);
    return hipGetLastError();
}

__global__ void __launch_bounds__(256) zero_words_kernel(unsigned* p, size_t nwords, size_t bw) {
    p = (unsigned*)((char*)p + blockIdx.z * bw);
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < nwords) p[i] = 0u;
}

hipError_t launch_zero(hipStream_t stream, void* p, size_t bytes) {
    const size_t nwords = bytes / 4;
    if (nwords == 0) return hipSuccess;
    hipLaunchKernelGGL(zero_words_kernel, dim3((unsigned)((nwords + 255) / 256), 1, g_batch.batch), dim3(256), 0, stream, (unsigned*)p, nwords, g_batch.ws);
    return hipGetLastError();
}

// k splits of the row-maxima pass of a row-strided operand: enough workgroups to fill the chip (~2048) -- the per-thread chain of dependent strided loads,
// not bandwidth, bounds that kernel when the grid is small -- at least 16 k values per workgroup, at most 32 splits (the extract reduces them per tile)
// and at most what the caller's scratch holds (max_parts).
unsigned amax_parts_for(size_t rows, size_t k, size_t max_parts) {
    const size_t row_groups = (rows + 63) / 64;
    size_t ks = (2048 + row_groups - 1) / row_groups;
    ks = std::min(ks, (k + 15) / 16);
    ks = std::min<size_t>(ks, 32);
    ks = std::min(ks, max_parts);
    return (unsigned)std::max<size_t>(ks, 1);
}

static StageArgs extract_args(int backend, size_t k, size_t kp, const ExtractOperand& o) {
    StageArgs a{};
    a.bx = o.xstride;
    a.xp = o.xptr;
    a.bw = g_batch.ws;
    a.X = o.X;
    a.ld = o.ld;
    a.rows = o.rows;
    a.k = k;
    a.kp = kp;
    a.lo = o.lo;
    a.part_stride = o.part_stride;
    a.sft0 = o.sft0;
    a.sft0_keep = o.sft0_keep;
    a.amax = o.amax;
    a.amax_parts = o.parts;
    a.amax_pstride = o.pstride;
    a.backend = backend;
    a.conj = o.conj;
    return a;
}
template <typename T> static hipError_t launch_amax_pair_t(hipStream_t stream, size_t k, const ExtractOperand& A, const ExtractOperand& B) {
    auto mk = [](const ExtractOperand& o) {
        AmaxOperand q{};
        if (o.rows && !o.kmajor && !o.one_read) q = AmaxOperand{o.X, o.ld, o.rows, o.xstride, o.amax, o.pstride, o.parts, (unsigned)((o.rows + 63) / 64)};
        return q;
    };
    const AmaxOperand a = mk(A), b = mk(B);
    const size_t nA = (size_t)a.row_groups * a.parts, nB = (size_t)b.row_groups * b.parts;
    if (nA + nB == 0) return hipSuccess;
    if (nA + nB > 0x7FFFFFFFull) return hipErrorInvalidConfiguration;
    if (A.xptr || B.xptr) {
        const AmaxPtrOperand pa{a, A.xptr}, pb{b, B.xptr};
        hipLaunchKernelGGL(amax_ptr_pair_kernel<T>, dim3((unsigned)(nA + nB), 1, g_batch.batch), dim3(256), 0, stream, pa, pb, (unsigned)nA, k, g_batch.ws);
    } else hipLaunchKernelGGL(amax_pair_kernel<T>, dim3((unsigned)(nA + nB), 1, g_batch.batch), dim3(256), 0, stream, a, b, (unsigned)nA, k, g_batch.ws);
    return hipGetLastError();
}
// an operand in symmetric form (ExtractOperand::sym / QuantOperand::sym): the *_sym_pair launches at the end of this file
static hipError_t launch_amax_sym_pair(hipStream_t stream, int dtype, size_t k, const ExtractOperand& A, const ExtractOperand& B);
static hipError_t launch_extract_sym_pair(hipStream_t stream, int dtype, int backend, size_t k, size_t kp, const ExtractOperand& A, const ExtractOperand& B,
                                          void* zero_p, size_t zero_bytes);
static hipError_t launch_fast_shift_sym_pair(hipStream_t stream, int dtype, int backend, unsigned N, size_t k, const QuantOperand& A, const QuantOperand& B);
static hipError_t launch_quantise_sym_pair(hipStream_t stream, int dtype, int backend, int t_begin, int t_end, size_t k, size_t kp, const QuantOperand& A,
                                           const QuantOperand& B);

hipError_t launch_amax_pair(hipStream_t stream, int dtype, size_t k, const ExtractOperand& A, const ExtractOperand& B) {
    if (A.sym || B.sym) return launch_amax_sym_pair(stream, dtype, k, A, B);
    switch (dtype) {
    case kF32: return launch_amax_pair_t<float>(stream, k, A, B);
    case kF64: return launch_amax_pair_t<double>(stream, k, A, B);
    case kC32: return launch_amax_pair_t<float2>(stream, k, A, B);
    case kC64: return launch_amax_pair_t<double2>(stream, k, A, B);
    }
    return hipErrorInvalidValue;
}
template <typename T> static size_t extract_blocks(int form, const StageArgs& a) {
    if (form == FORM_PANEL) return (a.rows + StageTile<T>::TR - 1) / StageTile<T>::TR;  // one workgroup per row panel
    return stage_blocks<T, MODE_BOUND>(form == FORM_KMAJOR, a);
}
template <typename T> static hipError_t launch_extract_pair_t(hipStream_t stream, int kmA, StageArgs a, int kmB, const StageArgs& b, void* zero_p, size_t zero_bytes) {
    const size_t nA = extract_blocks<T>(kmA, a), nB = extract_blocks<T>(kmB, b);
    if (nA + nB == 0) return zero_bytes ? launch_zero(stream, zero_p, zero_bytes) : hipSuccess;
    if (nA + nB > 0x7FFFFFFFull) return hipErrorInvalidConfiguration;
    if (zero_p && zero_bytes) a.zero_p = (unsigned*)zero_p, a.zero_words = (unsigned)(zero_bytes / 4);
    if constexpr (!ET<T>::cplx) {
        if (kmA == FORM_PANEL || kmB == FORM_PANEL) {
            hipLaunchKernelGGL(extract_panel_pair_kernel<T>, dim3((unsigned)(nA + nB), 1, g_batch.batch), dim3(256), 0, stream, a, b, (unsigned)nA, kmA, kmB);
            return hipGetLastError();
        }
    }
    if (a.xp || b.xp) hipLaunchKernelGGL(extract_ptr_pair_kernel<T>, dim3((unsigned)(nA + nB), 1, g_batch.batch), dim3(256), 0, stream, a, b, (unsigned)nA, kmA, kmB);
    else hipLaunchKernelGGL(extract_pair_kernel<T>, dim3((unsigned)(nA + nB), 1, g_batch.batch), dim3(256), 0, stream, a, b, (unsigned)nA, kmA, kmB);
    return hipGetLastError();
}
// where the one-read panel body (stage_panel_body) exists: real types, INT8 planes, a single GEMM, k within the step table
bool extract_one_read_ok(int dtype, int backend, size_t kp) {
    return (dtype == kF32 || dtype == kF64) && backend == kINT8 && g_batch.batch == 1 && kp / StageTile<double>::TK <= (size_t)kPanelMaxTiles;
}
// extract of both operands (rows == 0: absent) in ONE launch; zero_p / zero_bytes: words the launch also zero-fills (the bound GEMM's maxima arrays)
hipError_t launch_extract_pair(hipStream_t stream, int dtype, int backend, size_t k, size_t kp, const ExtractOperand& A, const ExtractOperand& B, void* zero_p,
                               size_t zero_bytes) {
    if (A.sym || B.sym) return launch_extract_sym_pair(stream, dtype, backend, k, kp, A, B, zero_p, zero_bytes);
    const StageArgs a = extract_args(backend, k, kp, A), b = extract_args(backend, k, kp, B);
    auto form = [&](const ExtractOperand& o) { return o.kmajor ? FORM_KMAJOR : o.one_read ? FORM_PANEL : FORM_STRIDED; };
    if ((A.one_read || B.one_read) && !extract_one_read_ok(dtype, backend, kp)) return hipErrorInvalidValue;
    const int fA = form(A), fB = form(B);
    switch (dtype) {
    case kF32: return launch_extract_pair_t<float>(stream, fA, a, fB, b, zero_p, zero_bytes);
    case kF64: return launch_extract_pair_t<double>(stream, fA, a, fB, b, zero_p, zero_bytes);
    case kC32: return launch_extract_pair_t<float2>(stream, fA, a, fB, b, zero_p, zero_bytes);
    case kC64: return launch_extract_pair_t<double2>(stream, fA, a, fB, b, zero_p, zero_bytes);
    }
    return hipErrorInvalidValue;
}

static StageArgs quantise_args(int backend, int t_begin, int t_end, size_t k, size_t kp, const QuantOperand& o) {
    StageArgs a{};
    a.bx = o.xstride;
    a.xp = o.xptr;
    a.bw = g_batch.ws;
    a.X = o.X;
    a.ld = o.ld;
    a.rows = o.rows;
    a.k = k;
    a.kp = kp;
    a.lo = o.lo;
    a.plane_stride = o.plane_stride;
    a.part_stride = o.part_stride;
    a.sft = o.sft;
    if (o.fin_max) {  // accurate mode: shift finalize folded into this launch
        a.fin_sft0 = o.fin_sft0;
        a.fin_max = o.fin_max;
        a.fin_out = o.sft;
        a.fin_log2P = o.fin_log2P;
        a.fin_float_max = backend == kFP8 ? 1 : 0;
    }
    a.backend = backend;
    a.conj = o.conj;
    a.nf = o.nf ? 1 : 0;
    a.t_begin = t_begin;
    a.t_end = t_end;
    a.mt = make_mod_table(backend);
    for (int t = t_begin, j = 0; t < t_end && j < 10; t += 2, ++j) {
        const double P = (double)a.mt.mc[t].p * (t + 1 < t_end ? (double)a.mt.mc[t + 1].p : 1.0);
        a.pairP[j] = P;
        a.pairInvP[j] = 1.0 / P;
    }
    for (int t = 0; t < 6; ++t) a.sqrtp[t] = GEMMUL8_SQRT_MODULI_FP8[t];
    if (backend == kFP8 && o.f6_rows > 0) {
        a.f6 = 1;
        a.f6_last = (unsigned)((o.f6_rows - 1) / 256);
        a.f6_rp_last = (unsigned)((o.f6_rows - 256 * (size_t)a.f6_last + 15) / 16 * 16);
    }
    return a;
}

static hipError_t launch_quantise_twin(hipStream_t stream, int dtype, int t_begin, int t_end, size_t k, size_t kp, const QuantOperand& A) {
    StageArgs a = quantise_args(kINT8, t_begin, t_end, k, kp, A);
    a.lo2 = A.lo2, a.plane_stride2 = A.plane_stride2, a.part_stride2 = A.part_stride2;
    const size_t nA = dtype == kC32 ? stage_blocks<float2, MODE_MOD>(A.kmajor, a) : stage_blocks<double2, MODE_MOD>(A.kmajor, a);
    if (nA > 0x7FFFFFFFull) return hipErrorInvalidConfiguration;
    const dim3 grid((unsigned)nA, 1, g_batch.batch);
    if (dtype == kC32) hipLaunchKernelGGL(quantise_twin_kernel<float2>, grid, dim3(256), 0, stream, a, (int)A.kmajor);
    else hipLaunchKernelGGL(quantise_twin_kernel<double2>, grid, dim3(256), 0, stream, a, (int)A.kmajor);
    return hipGetLastError();
}

// ---- gemmul8_syr2k: the operand passes over [A.X | S.X2] (kp = the padded length of ONE segment; plane rows are 2 kp apart)
template <typename T, int MODE> static size_t seg2_blocks(bool kmajor, const StageArgs& a) {
    if (kmajor) return a.rows * ((MODE == MODE_MOD && sizeof(T) <= 8) ? 2 * ((a.kp + 1023) / 1024) : 1);
    return 2 * (a.kp / StageTile<T>::TK) * ((a.rows + StageTile<T>::TR - 1) / StageTile<T>::TR);
}
static void seg2_args(StageArgs& a, size_t kp, const Seg2Planes& S) {
    a.X2 = S.X2, a.ld2 = S.ld2, a.pitch = 2 * kp;
    a.lo2 = S.lo2, a.plane_stride2 = S.plane_stride2, a.part_stride2 = S.part_stride2;
}
template <typename T, int MODE> static hipError_t launch_seg2_t(hipStream_t stream, bool kmajor, const StageArgs& a) {
    const size_t nb = seg2_blocks<T, MODE>(kmajor, a);
    if (nb == 0 || nb > 0x7FFFFFFFull) return hipErrorInvalidConfiguration;
    if constexpr (MODE == MODE_BOUND) hipLaunchKernelGGL(extract_seg2_kernel<T>, dim3((unsigned)nb), dim3(256), 0, stream, a, (int)kmajor);
    else hipLaunchKernelGGL(quantise_seg2_kernel<T>, dim3((unsigned)nb), dim3(256), 0, stream, a, (int)kmajor);
    return hipGetLastError();
}
template <int MODE> static hipError_t launch_seg2(hipStream_t stream, int dtype, bool kmajor, const StageArgs& a) {
    if (g_batch.batch != 1 || a.rows == 0 || a.kp % 256 != 0 || !a.X2 || !a.lo2) return hipErrorInvalidValue;
    switch (dtype) {
    case kF32: return launch_seg2_t<float, MODE>(stream, kmajor, a);
    case kF64: return launch_seg2_t<double, MODE>(stream, kmajor, a);
    case kC32: return launch_seg2_t<float2, MODE>(stream, kmajor, a);
    case kC64: return launch_seg2_t<double2, MODE>(stream, kmajor, a);
    }
    return hipErrorInvalidValue;
}
hipError_t launch_extract_seg2(hipStream_t stream, int dtype, size_t k, size_t kp, const ExtractOperand& A, const Seg2Planes& S, void* zero_p, size_t zero_bytes) {
    if (A.one_read || A.conj) return hipErrorInvalidValue;
    StageArgs a = extract_args(kINT8, k, kp, A);
    seg2_args(a, kp, S);
    if (zero_p && zero_bytes) a.zero_p = (unsigned*)zero_p, a.zero_words = (unsigned)(zero_bytes / 4);
    return launch_seg2<MODE_BOUND>(stream, dtype, A.kmajor, a);
}
hipError_t launch_quantise_seg2(hipStream_t stream, int dtype, int t_begin, int t_end, size_t k, size_t kp, const QuantOperand& A, const Seg2Planes& S) {
    if (t_end <= t_begin) return hipSuccess;
    if (A.conj || A.f6_rows || A.nf || A.lo2) return hipErrorInvalidValue;
    StageArgs a = quantise_args(kINT8, t_begin, t_end, k, kp, A);
    seg2_args(a, kp, S);
    return launch_seg2<MODE_MOD>(stream, dtype, A.kmajor, a);
}

hipError_t launch_quantise_pair(hipStream_t stream, int dtype, int backend, int t_begin, int t_end, size_t k, size_t kp, const QuantOperand& A,
                                const QuantOperand& B) {
    if ((A.rows == 0 && B.rows == 0) || t_end <= t_begin) return hipSuccess;
    if (A.sym || B.sym) return launch_quantise_sym_pair(stream, dtype, backend, t_begin, t_end, k, kp, A, B);
    if (A.lo2 || B.lo2) {  // the twin form: A alone, complex, INT8 byte planes, mode 0
        if (B.rows || B.lo2 || A.rows == 0 || !is_complex(dtype) || backend != kINT8 || A.f6_rows || A.nf) return hipErrorInvalidValue;
        return launch_quantise_twin(stream, dtype, t_begin, t_end, k, kp, A);
    }
    const StageArgs a = quantise_args(backend, t_begin, t_end, k, kp, A), b = quantise_args(backend, t_begin, t_end, k, kp, B);
    switch (dtype) {
    case kF32: return launch_quantise_stage<float>(stream, A.kmajor, a, B.kmajor, b);
    case kF64: return launch_quantise_stage<double>(stream, A.kmajor, a, B.kmajor, b);
    case kC32: return launch_quantise_stage<float2>(stream, A.kmajor, a, B.kmajor, b);
    case kC64: return launch_quantise_stage<double2>(stream, A.kmajor, a, B.kmajor, b);
    }
    return hipErrorInvalidValue;
}

// ------------------------------------------------------------------ accurate-mode shift from the bound maxima
// rows of A (blocks 0 .. blocksA-1) and columns of B (the remaining blocks) in ONE launch; either count may be 0
__global__ void shift_finalize_kernel(size_t rowsA, const int* maxA, int16_t* sftA, unsigned blocksA, size_t rowsB, const int* maxB,
                                      int16_t* sftB, float log2P, int float_max, size_t bw, int nf) {
    {  // batched launch: item blockIdx.z (all four arrays live in the item's workspace)
        const size_t o = blockIdx.z * bw;
        maxA = (const int*)((const char*)maxA + o), maxB = (const int*)((const char*)maxB + o);
        sftA = (int16_t*)((char*)sftA + o), sftB = (int16_t*)((char*)sftB + o);
    }
    const bool isB = blockIdx.x >= blocksA;
    const size_t r = (size_t)(isB ? blockIdx.x - blocksA : blockIdx.x) * blockDim.x + threadIdx.x;
    if (r >= (isB ? rowsB : rowsA)) return;
    const int amax = (isB ? maxB : maxA)[r];  // INT8: int32 maximum; FP8: bit pattern of a non-negative float
    int f = 0;  // all-zero row/column: the reference is undefined here (log2(0)); any shift is valid
    if (amax > 0) {
        const float l = __log2f(float_max ? __int_as_float(amax) : __int2float_rn(amax));
        f = __float2int_rd(__fmaf_rd(-0x1.000006p-1f, l, log2P));
    }
    int16_t* sft = isB ? sftB : sftA;
    if (nf && sft[r] == kNonfiniteSft) return;  // flagged (non-finite mode 1): the sentinel stays
    sft[r] = (int16_t)(-((int)sft[r] + f));
}
hipError_t launch_shift_finalize(hipStream_t stream, int backend, unsigned N, size_t rowsA, const int* maxA, int16_t* sftA, size_t rowsB,
                                 const int* maxB, int16_t* sftB, bool nf) {
    const unsigned bA = (unsigned)((rowsA + 255) / 256), bB = (unsigned)((rowsB + 255) / 256);
    if (bA + bB == 0) return hipSuccess;
    const float log2P = backend == kINT8 ? GEMMUL8_LOG2P_INT8[N - 2] : GEMMUL8_LOG2P_FP8[N - 2];
    hipLaunchKernelGGL(shift_finalize_kernel, dim3(bA + bB, 1, g_batch.batch), dim3(256), 0, stream, rowsA, maxA, sftA, bA, rowsB, maxB, sftB, log2P,
                       backend == kFP8 ? 1 : 0, g_batch.ws, nf ? 1 : 0);
    return hipGetLastError();
}

// ------------------------------------------------------------------ fast-mode shifts
// The round-up sums are order dependent; both kernels keep the reference's order so that the
// shifts are the ones its HIP build would produce: per-lane strided chains, width-32 shuffle
// trees, then a tree over the group sums (find_max.hpp:258-341, template_math.hpp:179-212).
template <typename U> __device__ __forceinline__ U add_ru(U a, U b);
template <> __device__ __forceinline__ float add_ru<float>(float a, float b) { return __fadd_ru(a, b); }
template <> __device__ __forceinline__ double add_ru<double>(double a, double b) { return __dadd_ru(a, b); }
template <typename U> __device__ __forceinline__ U sqr_add_ru(U x, U s);
template <> __device__ __forceinline__ float sqr_add_ru<float>(float x, float s) { return __fmaf_ru(x, x, s); }
template <> __device__ __forceinline__ double sqr_add_ru<double>(double x, double s) { return __fma_ru(x, x, s); }

template <typename U> __device__ __forceinline__ U tree32_sum_ru(U v) {  // result valid in lane (l & 31) == 0
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) v = add_ru<U>(v, __shfl_down(v, off, 32));
    return v;
}
template <typename U> __device__ __forceinline__ U tree32_max(U v) {
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) {
        const U o = __shfl_down(v, off, 32);
        v = o > v ? o : v;
    }
    return v;
}

__device__ __forceinline__ int fast_sft(double amax, double vecnrm, float log2P) {
    const int exponent = ilogb0(vecnrm);
    const float vecnrmf = __double2float_ru(scalbn(vecnrm, -exponent));
    const float log2vsum = __fadd_ru(__log2f(vecnrmf), (float)exponent);
    const float log2vnrm = __fmul_ru(0x1.000006p-1f, log2vsum);
    const float exp1 = __fsub_rd(__fsub_rd(log2P, 1.5f), fmaxf(1.0f, log2vnrm));
    return __float2int_rd(exp1) - ilogb0((float)amax);
}
__device__ __forceinline__ int fast_sft(float amax, float vecnrm, float log2P) {
    const float log2vsum = __log2f(vecnrm);
    const float log2vnrm = __fmul_ru(0x1.000006p-1f, log2vsum);
    const float exp1 = __fsub_rd(__fsub_rd(log2P, 1.5f), fmaxf(1.0f, log2vnrm));
    return __float2int_rd(exp1) - ilogb0(amax);
}

// K-major: one 256-thread block per row (scaling_fast_real.hpp:142-164)
// SEG2 (gemmul8_syr2k): the row of the K-concatenation [X | Z | X2], Z = the zero columns that bring X's k to a multiple of 256: every lane keeps its
// accumulators and runs its loop over X's row, then over X2's.  Element j of X2 sits in column pad256(k) + j of the concatenation, which is lane j % 256
// again, and a zero leaves a round-up sum as it is: the order of the reduction is the one the plain form has on the materialised concatenation.
template <typename T, bool SEG2 = false>
__device__ __forceinline__ void fast_shift_kmajor_body(const T* X, size_t ld, size_t k, int16_t* sft, float log2P, const unsigned bid, [[maybe_unused]] const T* X2 = nullptr,
                                                       [[maybe_unused]] size_t ld2 = 0) {
    using E = ET<T>;
    using U = typename E::U;
    __shared__ U samax[32], ssum[32];
    U amax = 0, sum = 0;
    auto segment = [&](const T* x) {
        size_t i = threadIdx.x;
        for (; i + 3 * 256 < k; i += 4 * 256) {  // four loads ahead of their (sequential) round-up FMAs
            T v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = x[i + 256 * u];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const U ar = (U)fabs(E::re(v[u]));
                amax = ar > amax ? ar : amax;
                sum = sqr_add_ru<U>(ar, sum);
                if constexpr (E::cplx) {
                    const U ai = (U)fabs(E::im(v[u]));
                    amax = ai > amax ? ai : amax;
                    sum = sqr_add_ru<U>(ai, sum);
                }
            }
        }
        for (; i < k; i += 256) {
            const T v = x[i];
            const U ar = (U)fabs(E::re(v));
            amax = ar > amax ? ar : amax;
            sum = sqr_add_ru<U>(ar, sum);
            if constexpr (E::cplx) {
                const U ai = (U)fabs(E::im(v));
                amax = ai > amax ? ai : amax;
                sum = sqr_add_ru<U>(ai, sum);
            }
        }
    };
    segment(X + (size_t)bid * ld);
    if constexpr (SEG2) segment(X2 + (size_t)bid * ld2);
    amax = tree32_max(amax);
    sum = tree32_sum_ru(sum);
    if ((threadIdx.x & 31) == 0) {
        samax[threadIdx.x >> 5] = amax;
        ssum[threadIdx.x >> 5] = sum;
    }
    __syncthreads();
    if (threadIdx.x < 32) {
        amax = threadIdx.x < 8 ? samax[threadIdx.x] : (U)0;
        sum = threadIdx.x < 8 ? ssum[threadIdx.x] : (U)0;
        amax = tree32_max(amax);
        sum = tree32_sum_ru(sum);
        if (threadIdx.x == 0) sft[bid] = (int16_t)(-fast_sft(amax, sum, log2P));
    }
}

// Row-strided (scaling_fast_real.hpp:27-49: 32 rows x 32 k-lanes per block).  The reduction ORDER is the reference's: lane ty of a row adds
// the squares of columns ty, ty + 32, ... in sequence, then a width-32 tree over the 32 lanes.  Geometry here: 256 threads = 8 lanes per
// column x 32 k-lanes; a lane owns RPL = 16 / sizeof(T) consecutive rows (one 16-byte load per column when aligned), a workgroup 8 RPL rows
// = one 128-byte line per column -- 512 workgroups for 8192 rows of doubles where the 32 x 32 form had 256 and 8-byte loads.  The loads of
// eight chain steps are issued ahead of their round-up FMAs: the chain itself is sequential, and with one load per step it ran at one
// memory latency per element (289 us for 1024 x 16384 doubles; 128 MiB).
// SEG2: as above -- lane ty of a row takes columns ty, ty + 32, ... of X, then of X2 (pad256(k) is a multiple of 32).
template <typename T, bool SEG2 = false>
__device__ __forceinline__ void fast_shift_strided_body(const T* X, size_t ld, size_t rows, size_t k, int16_t* sft, float log2P, const unsigned bid,
                                                        [[maybe_unused]] const T* X2 = nullptr, [[maybe_unused]] size_t ld2 = 0) {
    using E = ET<T>;
    using U = typename E::U;
    constexpr int RPL = 16 / (int)sizeof(T), RPB = 8 * RPL;
    __shared__ U samax[32][RPB + 1], ssum[32][RPB + 1];
    const int tx = threadIdx.x & 7, ty = threadIdx.x >> 3;
    const size_t row0 = (size_t)bid * RPB + (size_t)tx * RPL;
    U amax[RPL], sum[RPL];
#pragma unroll
    for (int j = 0; j < RPL; ++j) amax[j] = 0, sum[j] = 0;
    auto take = [&](const T& v, int j) {
        const U ar = (U)fabs(E::re(v));
        amax[j] = ar > amax[j] ? ar : amax[j];
        sum[j] = sqr_add_ru<U>(ar, sum[j]);
        if constexpr (E::cplx) {
            const U ai = (U)fabs(E::im(v));
            amax[j] = ai > amax[j] ? ai : amax[j];
            sum[j] = sqr_add_ru<U>(ai, sum[j]);
        }
    };
    auto segment = [&](const T* Xs, const size_t lds) {
        if (row0 < rows) {
            const T* x = Xs + row0;
            const bool vec = row0 + RPL <= rows && ((reinterpret_cast<uintptr_t>(x) | (lds * sizeof(T))) & 15u) == 0;
            size_t col = ty;
            if (vec) {
                typedef unsigned V4 __attribute__((ext_vector_type(4)));
                // loads in flight per thread: 8 x 16 bytes; 4-byte elements have half as many workgroups (8 x 4 rows each: 256 at 8192 rows,
                // one per CU), so they keep 16 in flight (8192^2 float: 88 us = 3.0 TB/s with 8).  The order of the accumulation -- columns
                // ascending per thread -- does not depend on the depth.
                constexpr int UNR = sizeof(T) == 4 ? 16 : 8;
                if constexpr (UNR > 8) {
                    for (; col + (UNR - 1) * 32 < k; col += UNR * 32) {
                        V4 raw[UNR];
#pragma unroll
                        for (int u = 0; u < UNR; ++u) raw[u] = *(const V4*)(x + (col + 32 * u) * lds);
#pragma unroll
                        for (int u = 0; u < UNR; ++u) {
                            T v[RPL];
                            __builtin_memcpy(v, &raw[u], 16);
#pragma unroll
                            for (int j = 0; j < RPL; ++j) take(v[j], j);
                        }
                    }
                }
                for (; col + 7 * 32 < k; col += 8 * 32) {
                    V4 raw[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) raw[u] = *(const V4*)(x + (col + 32 * u) * lds);
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        T v[RPL];
                        __builtin_memcpy(v, &raw[u], 16);
#pragma unroll
                        for (int j = 0; j < RPL; ++j) take(v[j], j);
                    }
                }
                for (; col < k; col += 32) {
                    T v[RPL];
                    const V4 raw = *(const V4*)(x + col * lds);
                    __builtin_memcpy(v, &raw, 16);
#pragma unroll
                    for (int j = 0; j < RPL; ++j) take(v[j], j);
                }
            } else {
                for (; col < k; col += 32) {
#pragma unroll
                    for (int j = 0; j < RPL; ++j)
                        if (row0 + j < rows) take(x[col * lds + j], j);
                }
            }
        }
    };
    segment(X, ld);
    if constexpr (SEG2) segment(X2, ld2);
#pragma unroll
    for (int j = 0; j < RPL; ++j) {
        samax[ty][tx * RPL + j] = amax[j];
        ssum[ty][tx * RPL + j] = sum[j];
    }
    __syncthreads();
    // thread r * 32 + l holds lane l of row r: width-32 trees, 8 rows per sweep
    const int ll = threadIdx.x & 31;
    for (int rr = threadIdx.x >> 5; rr < RPB; rr += 8) {
        const U s = tree32_sum_ru(ssum[ll][rr]);
        const U m = tree32_max(samax[ll][rr]);
        const size_t row = (size_t)bid * RPB + rr;
        if (row < rows && ll == 0) sft[row] = (int16_t)(-fast_sft(m, s, log2P));
    }
}

// both operands in one launch: workgroups [0, a.blocks) take the rows of A, the rest the columns of B; either share may be empty
struct ShiftOperand {
    const void* X;
    size_t ld, rows, bx;
    int16_t* sft;
    unsigned blocks;
    int kmajor;
};
// the operand of fast_shift_ptr_pair_kernel (a pointer-array batch): non-null xp = item z's operand is xp[z].  A type of its own: ShiftOperand keeps its layout.
struct ShiftPtrOperand : ShiftOperand {
    const void* const* xp;
};
template <typename T> __global__ void __launch_bounds__(256) fast_shift_pair_kernel(const ShiftOperand a, const ShiftOperand b, size_t k, float log2P, size_t bw) {
    const bool isB = blockIdx.x >= a.blocks;
    const ShiftOperand& o = isB ? b : a;  // (kernel arguments: a scalar select per field, no copy)
    const unsigned bid = isB ? blockIdx.x - a.blocks : blockIdx.x;
    const T* X = (const T*)((const char*)o.X + blockIdx.z * o.bx);  // batched launch: item blockIdx.z
    int16_t* sft = (int16_t*)((char*)o.sft + blockIdx.z * bw);
    if (o.kmajor) fast_shift_kmajor_body<T>(X, o.ld, k, sft, log2P, bid);
    else fast_shift_strided_body<T>(X, o.ld, o.rows, k, sft, log2P, bid);
}
// the same for a pointer-array batch: the item's operand from ShiftOperand::xp where the operand has an array
template <typename T> __global__ void __launch_bounds__(256) fast_shift_ptr_pair_kernel(const ShiftPtrOperand a, const ShiftPtrOperand b, size_t k, float log2P, size_t bw) {
    const bool isB = blockIdx.x >= a.blocks;
    const ShiftPtrOperand& o = isB ? b : a;
    const unsigned bid = isB ? blockIdx.x - a.blocks : blockIdx.x;
    const T* X = (const T*)item_base<true>(o.X, o.xp, o.bx);
    int16_t* sft = (int16_t*)((char*)o.sft + blockIdx.z * bw);
    if (o.kmajor) fast_shift_kmajor_body<T>(X, o.ld, k, sft, log2P, bid);
    else fast_shift_strided_body<T>(X, o.ld, o.rows, k, sft, log2P, bid);
}

// gemmul8_syr2k: one shift per row of [X | Z | X2] (a.X, b.X: the same form, the same rows), written to a.sft
template <typename T> __global__ void __launch_bounds__(256) fast_shift_seg2_kernel(const ShiftOperand a, const ShiftOperand b, size_t k, float log2P) {
    if (a.kmajor) fast_shift_kmajor_body<T, true>((const T*)a.X, a.ld, k, a.sft, log2P, blockIdx.x, (const T*)b.X, b.ld);
    else fast_shift_strided_body<T, true>((const T*)a.X, a.ld, a.rows, k, a.sft, log2P, blockIdx.x, (const T*)b.X, b.ld);
}

hipError_t launch_fast_shift_pair(hipStream_t stream, int dtype, int backend, unsigned N, size_t k, const QuantOperand& A, const QuantOperand& B) {
    if (A.rows == 0 && B.rows == 0) return hipSuccess;
    if (A.sym || B.sym) return launch_fast_shift_sym_pair(stream, dtype, backend, N, k, A, B);
    const float log2P = backend == kINT8 ? GEMMUL8_LOG2P_INT8[N - 2] : GEMMUL8_LOG2P_FP8[N - 2];
    const size_t rpb = 8 * (16 / (is_f32(dtype) ? 4 : 8) / (is_complex(dtype) ? 2 : 1));  // rows per workgroup of the row-strided form
    auto operand = [&](const QuantOperand& o) {
        const size_t blocks = o.kmajor ? o.rows : (o.rows + rpb - 1) / rpb;
        return ShiftOperand{o.X, o.ld, o.rows, o.xstride, o.sft, (unsigned)blocks, o.kmajor ? 1 : 0};
    };
    if (A.rows + B.rows > 0x7FFFFFFFull) return hipErrorInvalidConfiguration;
    const ShiftOperand a = operand(A), b = operand(B);
    dim3 grid(a.blocks + b.blocks, 1, g_batch.batch);
    const ShiftPtrOperand pa{a, A.xptr}, pb{b, B.xptr};
#define OZ2_FAST_SHIFT(T)                                                                                                           \
    do {                                                                                                                            \
        if (A.xptr || B.xptr) hipLaunchKernelGGL(fast_shift_ptr_pair_kernel<T>, grid, dim3(256), 0, stream, pa, pb, k, log2P, g_batch.ws); \
        else hipLaunchKernelGGL(fast_shift_pair_kernel<T>, grid, dim3(256), 0, stream, a, b, k, log2P, g_batch.ws);                  \
    } while (0)
    switch (dtype) {
    case kF32: OZ2_FAST_SHIFT(float); break;
    case kF64: OZ2_FAST_SHIFT(double); break;
    case kC32: OZ2_FAST_SHIFT(float2); break;
    case kC64: OZ2_FAST_SHIFT(double2); break;
#undef OZ2_FAST_SHIFT
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_fast_shift_seg2(hipStream_t stream, int dtype, unsigned N, size_t k, const QuantOperand& A, const Seg2Planes& S) {
    if (g_batch.batch != 1 || A.rows == 0 || !S.X2) return hipErrorInvalidValue;
    const float log2P = GEMMUL8_LOG2P_INT8[N - 2];
    const size_t rpb = 8 * (16 / (is_f32(dtype) ? 4 : 8) / (is_complex(dtype) ? 2 : 1));  // rows per workgroup of the row-strided form
    const size_t blocks = A.kmajor ? A.rows : (A.rows + rpb - 1) / rpb;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidConfiguration;
    const ShiftOperand a{A.X, A.ld, A.rows, 0, A.sft, (unsigned)blocks, A.kmajor ? 1 : 0}, b{S.X2, S.ld2, A.rows, 0, nullptr, 0, a.kmajor};
    const dim3 grid((unsigned)blocks);
    switch (dtype) {
    case kF32: hipLaunchKernelGGL(fast_shift_seg2_kernel<float>, grid, dim3(256), 0, stream, a, b, k, log2P); break;
    case kF64: hipLaunchKernelGGL(fast_shift_seg2_kernel<double>, grid, dim3(256), 0, stream, a, b, k, log2P); break;
    case kC32: hipLaunchKernelGGL(fast_shift_seg2_kernel<float2>, grid, dim3(256), 0, stream, a, b, k, log2P); break;
    case kC64: hipLaunchKernelGGL(fast_shift_seg2_kernel<double2>, grid, dim3(256), 0, stream, a, b, k, log2P); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// ------------------------------------------------------------------ symmetric form (gemmul8_symm / gemmul8_hemm; SymForm in oz2_kernels.h)
// The operand is Afull, the ka x ka matrix BLAS defines from ONE stored triangle of X, and it enters the scaling as a row-strided operand with rows == k == ka:
// logical element (r, kk) lies at X[kk*ld + r] on the stored side of the diagonal and at X[r*ld + kk] on the mirrored side (HEMM: conjugated there, and the
// diagonal's imaginary part counts as 0).  Afull is never materialised and no element of the other strict triangle is read.  Every kernel here is element-wise
// the strided form's (same bytes given the same values); the fast mode's round-up sums keep fast_shift_strided_body's order.  A general operand that shares a
// launch with the symmetric one takes its usual body (K-major) or the symmetric body with sym == kSymNone (row-strided: every tile is a stored tile, loaded
// as stage_strided_body loads it) -- one LDS tile per kernel.
struct SymStageArgs : StageArgs {
    int sym;   // SymForm
    int herm;  // complex types: mirrored half conjugated, real diagonal
};
static_assert(2 * sizeof(SymStageArgs) + 16 <= 4096, "two argument blocks must fit the 4 KiB kernel-argument segment");

template <typename T> __device__ __forceinline__ T sym_conj(T v) {
    if constexpr (ET<T>::cplx) v.y = -v.y;
    return v;
}
// the address rule: logical element (r, kk) of the operand (sym == kSymNone: the plain row-strided element)
template <typename T> __device__ __forceinline__ T sym_one() {
    T v = ET<T>::zero();
    if constexpr (ET<T>::cplx) v.x = 1;
    else v = 1;
    return v;
}
template <typename T> __device__ __forceinline__ T sym_at(const T* X, size_t ld, size_t r, size_t kk, int sym, int herm) {
    const int base = sym & kSymBase;
    const bool stored = base == kSymNone || (base == kSymLower ? r >= kk : r <= kk);
    if (sym & kTriAny) {  // triangular form (gemmul8_trmm): the dead half and a unit diagonal without a load
        if (r == kk) {
            if (sym & kTriUnit) return sym_one<T>();
        } else if (stored != ((sym & kTriStored) != 0)) {
            return ET<T>::zero();
        }
        return (sym & kTriStored) ? X[kk * ld + r] : X[r * ld + kk];  // (op = C: the operand's own `conj` flag, applied where the planes are written)
    }
    T v = stored ? X[kk * ld + r] : X[r * ld + kk];
    if constexpr (ET<T>::cplx) {
        if (herm) {
            if (!stored) v.y = -v.y;
            if (r == kk) v.y = 0;  // whatever the memory holds
        }
    }
    return v;
}

// Row-strided staging (the LDS tile and the emit pass of stage_strided_body) with one of three loaders per tile, chosen uniformly for the workgroup:
//   stored    tile strictly on the stored side of the diagonal: stage_strided_body's loads, 16 bytes down the columns;
//   mirrored  tile strictly on the other side: its rows are contiguous along kk at X[r*ld + kk] -- 16-byte loads along kk straight into the tile rows
//             (four per thread, all in flight), conjugated for HEMM; no column-strided scalar loads;
//   diagonal  a tile the diagonal crosses (at most 128 / TR + 1 row tiles per k tile): the address per element.
// Scalar loads where the base or ld is not 16-byte aligned; rows and columns past ka read as zero.
template <typename T, int MODE> __device__ __forceinline__ void stage_sym_body(const SymStageArgs& a, const unsigned bid) {
    using E = ET<T>;
    using U = typename E::U;
    constexpr int TR = StageTile<T>::TR, TK = StageTile<T>::TK;
    constexpr int PITCH = TK + (sizeof(T) >= 16 ? 1 : 16 / sizeof(T));  // rows stay 16-B aligned
    constexpr int CH = TK / 4;                                          // 4-wide k chunks per row
    constexpr int RPP = 256 / CH;                                       // rows per pass
    __shared__ __attribute__((aligned(16))) T tile[TR][PITCH];
    using UBm = typename std::conditional<sizeof(U) == 8, unsigned long long, unsigned>::type;
    [[maybe_unused]] __shared__ UBm rowam[TR];
    typedef unsigned V4 __attribute__((ext_vector_type(4)));
    const unsigned nrt = (unsigned)((a.rows + TR - 1) / TR);
    const unsigned kt = bid / nrt, rt = bid - kt * nrt;  // the row-tile index is the fast one, as in stage_strided_body
    const size_t r0 = (size_t)rt * TR, kb = (size_t)kt * TK;
    const T* const X = (const T*)((const char*)a.X + OZ2_ZX);
    const size_t ld = a.ld;
    enum { TILE_STORED = 0, TILE_MIRRORED = 1, TILE_DIAGONAL = 2, TILE_DEAD = 3 };
    int cls = TILE_STORED;
    if (a.sym != kSymNone) {  // (uniform)
        const bool above = r0 + TR - 1 < kb, below = r0 > kb + TK - 1;  // every r < every kk / every r > every kk of the tile
        const bool lower = (a.sym & kSymBase) == kSymLower;
        cls = (lower ? below : above) ? TILE_STORED : (lower ? above : below) ? TILE_MIRRORED : TILE_DIAGONAL;
        // triangular form: a tile strictly on the dead side of the diagonal is zero WITHOUT a load; the emit pass below writes its plane bytes (the
        // bytes of zeros: the planes of the whole operand are written by this launch, nothing relies on an earlier fill)
        if ((a.sym & kTriAny) && cls != TILE_DIAGONAL && (cls == TILE_STORED) != ((a.sym & kTriStored) != 0)) cls = TILE_DEAD;
    }
    if constexpr (MODE == MODE_BOUND) {  // row maxima of the tile's rows = the maximum over the k splits' partial arrays (amax_sym_pair_kernel)
        constexpr int PL = 256 / TR;
        const int rr = threadIdx.x / PL, pp = threadIdx.x % PL;
        UBm v = 0;
        if (r0 + rr < a.rows) {
            const UBm* am = (const UBm*)((const char*)a.amax + OZ2_ZW) + r0 + rr;
            for (unsigned q = pp; q < a.amax_parts; q += PL) {
                const UBm w = am[(size_t)q * a.amax_pstride];
                v = w > v ? w : v;
            }
        }
#pragma unroll
        for (int d = PL / 2; d >= 1; d >>= 1) {
            const UBm w = __shfl_xor(v, d);
            v = w > v ? w : v;
        }
        if (pp == 0) rowam[rr] = v;
    }
    if (cls == TILE_DEAD) {
        for (int i = threadIdx.x; i < TR * TK; i += 256) tile[i / TK][i % TK] = E::zero();
    } else if (cls == TILE_MIRRORED) {
        constexpr int EPV = sizeof(T) >= 16 ? 1 : 16 / (int)sizeof(T);  // elements per 16-byte piece
        constexpr int VPR = TK / EPV;                                   // pieces per tile row
        constexpr int NV = TR * VPR / 256;                              // pieces per thread (4 for every type)
        static_assert(NV * 256 == TR * VPR && EPV * sizeof(T) == 16, "tile = whole 16-byte pieces per thread");
        const bool vec_ok = ((reinterpret_cast<uintptr_t>(X) | (ld * sizeof(T))) & 15u) == 0;
        V4 buf[NV];
#pragma unroll
        for (int it = 0; it < NV; ++it) {
            const int idx = (int)threadIdx.x + 256 * it;
            const size_t row = r0 + idx / VPR, kg = kb + (size_t)(idx % VPR) * EPV;
            V4 v = {0u, 0u, 0u, 0u};
            if (row < a.rows && kg < a.k) {
                const T* p = X + row * ld + kg;
                if (vec_ok && kg + EPV <= a.k) {
                    v = __builtin_nontemporal_load((const V4*)p);
                } else {
#pragma unroll
                    for (int e = 0; e < EPV; ++e) {
                        const T t = (kg + e < a.k) ? p[e] : E::zero();
                        __builtin_memcpy((char*)&v + e * sizeof(T), &t, sizeof(T));
                    }
                }
            }
            buf[it] = v;
        }
#pragma unroll
        for (int it = 0; it < NV; ++it) {
            const int idx = (int)threadIdx.x + 256 * it;
            if constexpr (E::cplx) {
                if (a.herm) {  // (uniform)
                    T t[EPV];
                    __builtin_memcpy(t, &buf[it], 16);
#pragma unroll
                    for (int e = 0; e < EPV; ++e) t[e] = sym_conj(t[e]);
                    __builtin_memcpy(&buf[it], t, 16);
                }
            }
            *(V4*)&tile[idx / VPR][(idx % VPR) * EPV] = buf[it];
        }
    } else if (cls == TILE_DIAGONAL) {
        constexpr int KY = 256 / TR;  // k values fetched per pass
        const int rx = threadIdx.x % TR, ky = threadIdx.x / TR;
        const size_t row = r0 + rx;
#pragma unroll 4
        for (int it = 0; it < TK / KY; ++it) {
            const int kk = ky + KY * it;
            const size_t kg = kb + kk;
            tile[rx][kk] = (row < a.rows && kg < a.k) ? sym_at<T>(X, ld, row, kg, a.sym, a.herm) : E::zero();
        }
    } else if constexpr (sizeof(T) <= 8) {  // stored: the loads of stage_strided_body
        constexpr int RPL = 16 / (int)sizeof(T);
        constexpr int RP = TR / RPL;     // row groups per column
        constexpr int KY = 256 / RP;     // k values fetched per pass
        const int rp = threadIdx.x % RP, ky = threadIdx.x / RP;
        const size_t row = r0 + RPL * rp;
        const T* x = X + row;
        const bool pair_ok = row + RPL - 1 < a.rows && ((reinterpret_cast<uintptr_t>(x) | (ld * sizeof(T))) & 15u) == 0;
        V4 buf[TK / KY];
#pragma unroll
        for (int it = 0; it < TK / KY; ++it) {
            const size_t kg = kb + ky + KY * it;
            V4 v = {0u, 0u, 0u, 0u};
            if (kg < a.k) {
                if (pair_ok) {
                    v = __builtin_nontemporal_load((const V4*)(x + kg * ld));
                } else {
#pragma unroll
                    for (int e = 0; e < RPL; ++e) {
                        const T t = (row + e < a.rows) ? x[kg * ld + e] : E::zero();
                        __builtin_memcpy((char*)&v + e * sizeof(T), &t, sizeof(T));
                    }
                }
            }
            buf[it] = v;
        }
#pragma unroll
        for (int it = 0; it < TK / KY; ++it) {
            const int kk = ky + KY * it;
#pragma unroll
            for (int e = 0; e < RPL; ++e) __builtin_memcpy(&tile[RPL * rp + e][kk], (const char*)&buf[it] + e * sizeof(T), sizeof(T));
        }
    } else {
        constexpr int KY = 256 / TR;
        const int rx = threadIdx.x % TR, ky = threadIdx.x / TR;
        const size_t row = r0 + rx;
        const T* x = X + row;
#pragma unroll 4
        for (int it = 0; it < TK / KY; ++it) {
            const int kk = ky + KY * it;
            const size_t kg = kb + kk;
            tile[rx][kk] = (row < a.rows && kg < a.k) ? x[kg * ld] : E::zero();
        }
    }
    __syncthreads();
    const int c = threadIdx.x % CH;
#pragma unroll 1
    for (int pass = 0; pass < TR / RPP; ++pass) {
        const int rl = pass * RPP + threadIdx.x / CH;
        const size_t row = r0 + rl;
        if (row >= a.rows) continue;
        int s;
        if constexpr (MODE == MODE_BOUND) {
            const UBm bits = rowam[rl];
            U am;
            __builtin_memcpy(&am, &bits, sizeof(U));
            s = (a.backend == kINT8 ? 5 : 7) - ilogb0(am);
            if (kt == 0 && c == 0) {
                ((int16_t*)((char*)a.sft0 + OZ2_ZW))[row] = (int16_t)s;
                if (a.sft0_keep) ((int16_t*)((char*)a.sft0_keep + OZ2_ZW))[row] = (int16_t)s;
            }
        } else {
            s = OZ2_ROW_SHIFT(a, row, kt == 0 && c == 0);
        }
        T v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = tile[rl][c * 4 + e];
        emit4<T, MODE>(a, row, kb + c * 4, v, s);
    }
}
template <typename T> __global__ void __launch_bounds__(256) extract_sym_pair_kernel(const SymStageArgs a, const SymStageArgs b, const unsigned nA, const int kmA, const int kmB) {
    if (a.zero_words) {
        unsigned* zp = (unsigned*)((char*)a.zero_p + OZ2_ZW);
        for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < a.zero_words; i += gridDim.x * 256u) zp[i] = 0u;
    }
    if (blockIdx.x < nA) {
        if (kmA) stage_kmajor_body<T, MODE_BOUND>(a, blockIdx.x);
        else stage_sym_body<T, MODE_BOUND>(a, blockIdx.x);
    } else {
        if (kmB) stage_kmajor_body<T, MODE_BOUND>(b, blockIdx.x - nA);
        else stage_sym_body<T, MODE_BOUND>(b, blockIdx.x - nA);
    }
}
template <typename T> __global__ void __launch_bounds__(256) quantise_sym_pair_kernel(const SymStageArgs a, const SymStageArgs b, const unsigned nA, const int kmA, const int kmB) {
    if (blockIdx.x < nA) {
        if (kmA) stage_kmajor_body<T, MODE_MOD>(a, blockIdx.x);
        else stage_sym_body<T, MODE_MOD>(a, blockIdx.x);
    } else {
        if (kmB) stage_kmajor_body<T, MODE_MOD>(b, blockIdx.x - nA);
        else stage_sym_body<T, MODE_MOD>(b, blockIdx.x - nA);
    }
}

// Row maxima of a symmetric-form operand as partial arrays, amax_pair_kernel's scheme (workgroup = 64 rows x one k split; no atomics, nothing to zero).  The
// split's columns on the mirrored side of ALL 64 rows are read along kk (16 lanes = 128 contiguous bytes of a row, four rows per lane); the others -- stored
// for every row, or crossed by the diagonal -- with lanes along the rows through the address rule.
struct AmaxSymOperand : AmaxOperand {
    int sym, herm;
};
template <typename T> __device__ __forceinline__ void amax_sym_body(const AmaxSymOperand& o, const unsigned bid, size_t k, size_t bw) {
    const T* X = (const T*)((const char*)o.X + blockIdx.z * o.bx);
    using E = ET<T>;
    using U = typename E::U;
    using UB = typename std::conditional<sizeof(U) == 8, unsigned long long, unsigned>::type;
    UB* amax = (UB*)((char*)o.amax + blockIdx.z * bw);
    const unsigned by = bid / o.row_groups, bxr = bid - by * o.row_groups;
    const size_t rows = o.rows, ld = o.ld;
    __shared__ U sm[5][64];
    const size_t R0 = (size_t)bxr * 64;
    const size_t kper = (k + o.parts - 1) / o.parts;
    const size_t kbeg = (size_t)by * kper, kend = (kbeg + kper < k) ? kbeg + kper : k;
    size_t sb, se, mb, me;  // columns read along the rows [sb, se) / along kk [mb, me)
    if ((o.sym & kSymBase) == kSymLower) sb = kbeg, se = kend < R0 + 64 ? kend : R0 + 64, mb = kbeg > R0 + 64 ? kbeg : R0 + 64, me = kend;
    else mb = kbeg, me = kend < R0 ? kend : R0, sb = kbeg > R0 ? kbeg : R0, se = kend;
    if (o.sym & kTriStored) {  // triangular form: the mirrored side of all 64 rows is zero -- not read (a maximum does not notice a zero)
        me = mb;
    } else if (o.sym & kTriMirrored) {  // the stored side is zero: only the columns the diagonal crosses in these 64 rows go through the address rule
        if ((o.sym & kSymBase) == kSymLower) sb = sb > R0 ? sb : R0;
        else se = se < R0 + 64 ? se : R0 + 64;
    }
    auto take = [](const T& v, U& am) {
        const U ar = (U)fabs(E::re(v)), ai = (U)fabs(E::im(v));
        am = ar > am ? ar : am;
        am = ai > am ? ai : am;
    };
    {
        const int rl = threadIdx.x & 63, ky = threadIdx.x >> 6;
        const size_t row = R0 + rl;
        U am = 0;
        if (row < rows) {
            size_t kk = sb + ky;
            for (; kk + 12 < se; kk += 16) {  // four loads in flight per thread
                T v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = sym_at<T>(X, ld, row, kk + 4 * u, o.sym, o.herm);
#pragma unroll
                for (int u = 0; u < 4; ++u) take(v[u], am);
            }
            for (; kk < se; kk += 4) take(sym_at<T>(X, ld, row, kk, o.sym, o.herm), am);
        }
        sm[ky][rl] = am;
    }
    {
        const int kl = threadIdx.x & 15, rq = threadIdx.x >> 4;
        U am[4] = {0, 0, 0, 0};
        for (size_t kk = mb + kl; kk < me; kk += 16) {
            T v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const size_t row = R0 + rq + 16 * j;
                v[j] = row < rows ? X[row * ld + kk] : E::zero();  // (the conjugate has the same magnitudes)
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) take(v[j], am[j]);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int off = 8; off > 0; off >>= 1) {
                const U w = __shfl_xor(am[j], off);
                am[j] = w > am[j] ? w : am[j];
            }
            if (kl == 0) sm[4][rq + 16 * j] = am[j];
        }
    }
    __syncthreads();
    const size_t row = R0 + threadIdx.x;
    if (threadIdx.x < 64 && row < rows) {
        U m = sm[0][threadIdx.x];
#pragma unroll
        for (int y = 1; y < 5; ++y) m = sm[y][threadIdx.x] > m ? sm[y][threadIdx.x] : m;
        UB bits;
        __builtin_memcpy(&bits, &m, sizeof(U));
        amax[(size_t)by * o.pstride + row] = bits;
    }
}
template <typename T> __global__ void __launch_bounds__(256) amax_sym_pair_kernel(const AmaxSymOperand a, const AmaxSymOperand b, const unsigned nA, size_t k, size_t bw) {
    const bool isB = blockIdx.x >= nA;
    const AmaxSymOperand& o = isB ? b : a;
    const unsigned bid = isB ? blockIdx.x - nA : blockIdx.x;
    if (o.sym != kSymNone) amax_sym_body<T>(o, bid, k, bw);
    else amax_strided_body<T>(o, bid, k, bw);
}

// Fast-mode shift of a symmetric-form operand: fast_shift_strided_body's geometry and, exactly, its accumulation order -- lane ty of a row adds the squares of
// columns ty, ty + 32, ... ascending, then the width-32 trees -- with every element fetched through the address rule (eight chain steps of loads ahead of
// their round-up FMAs; the depth does not enter the order).
template <typename T>
__device__ __forceinline__ void fast_shift_sym_body(const T* X, size_t ld, size_t rows, size_t k, int16_t* sft, float log2P, const unsigned bid, const int sym, const int herm) {
    using E = ET<T>;
    using U = typename E::U;
    constexpr int RPL = 16 / (int)sizeof(T), RPB = 8 * RPL;
    __shared__ U samax[32][RPB + 1], ssum[32][RPB + 1];
    const int tx = threadIdx.x & 7, ty = threadIdx.x >> 3;
    const size_t row0 = (size_t)bid * RPB + (size_t)tx * RPL;
    U amax[RPL], sum[RPL];
#pragma unroll
    for (int j = 0; j < RPL; ++j) amax[j] = 0, sum[j] = 0;
    auto take = [&](const T& v, int j) {
        const U ar = (U)fabs(E::re(v));
        amax[j] = ar > amax[j] ? ar : amax[j];
        sum[j] = sqr_add_ru<U>(ar, sum[j]);
        if constexpr (E::cplx) {
            const U ai = (U)fabs(E::im(v));
            amax[j] = ai > amax[j] ? ai : amax[j];
            sum[j] = sqr_add_ru<U>(ai, sum[j]);
        }
    };
    // Triangular form (gemmul8_trmm): an element the plain kernel reads as an explicit zero of the materialised matrix adds nothing to this lane's sums --
    // max(a, 0) = a, and the round-up sum of a non-negative s and 0 * 0 is s exactly (x + 0 == x) --, so the columns that are dead for ALL rows of the
    // block are not visited at all (the code relies on that identity there); inside the visited range a dead element enters the same lane's sum, in its
    // place, as the zero sym_at returns without a load.  The live elements keep their lane (column mod 32) and their ascending order.
    size_t cbeg = 0, cend = k;
    if (sym & kTriAny) {
        if (tri_live_below(sym)) cend = row0 + RPL < k ? row0 + RPL : k;  // live: kk <= r
        else cbeg = row0 / 32 * 32;                                        // live: kk >= r
    }
    if (row0 < rows) {
        size_t col = cbeg + ty;
        for (; col + 7 * 32 < cend; col += 8 * 32) {
            T v[8][RPL];
#pragma unroll
            for (int u = 0; u < 8; ++u)
#pragma unroll
                for (int j = 0; j < RPL; ++j) v[u][j] = row0 + j < rows ? sym_at<T>(X, ld, row0 + j, col + 32 * u, sym, herm) : E::zero();
#pragma unroll
            for (int u = 0; u < 8; ++u)
#pragma unroll
                for (int j = 0; j < RPL; ++j) take(v[u][j], j);
        }
        for (; col < cend; col += 32) {
#pragma unroll
            for (int j = 0; j < RPL; ++j)
                if (row0 + j < rows) take(sym_at<T>(X, ld, row0 + j, col, sym, herm), j);
        }
    }
#pragma unroll
    for (int j = 0; j < RPL; ++j) {
        samax[ty][tx * RPL + j] = amax[j];
        ssum[ty][tx * RPL + j] = sum[j];
    }
    __syncthreads();
    const int ll = threadIdx.x & 31;
    for (int rr = threadIdx.x >> 5; rr < RPB; rr += 8) {
        const U s = tree32_sum_ru(ssum[ll][rr]);
        const U m = tree32_max(samax[ll][rr]);
        const size_t row = (size_t)bid * RPB + rr;
        if (row < rows && ll == 0) sft[row] = (int16_t)(-fast_sft(m, s, log2P));
    }
}
struct ShiftSymOperand : ShiftOperand {
    int sym, herm;
};
template <typename T> __global__ void __launch_bounds__(256) fast_shift_sym_pair_kernel(const ShiftSymOperand a, const ShiftSymOperand b, size_t k, float log2P, size_t bw) {
    const bool isB = blockIdx.x >= a.blocks;
    const ShiftSymOperand& o = isB ? b : a;
    const unsigned bid = isB ? blockIdx.x - a.blocks : blockIdx.x;
    const T* X = (const T*)((const char*)o.X + blockIdx.z * o.bx);
    int16_t* sft = (int16_t*)((char*)o.sft + blockIdx.z * bw);
    if (o.kmajor) fast_shift_kmajor_body<T>(X, o.ld, k, sft, log2P, bid);
    else if (o.sym != kSymNone) fast_shift_sym_body<T>(X, o.ld, o.rows, k, sft, log2P, bid, o.sym, o.herm);
    else fast_shift_strided_body<T>(X, o.ld, o.rows, k, sft, log2P, bid);
}

// a symmetric-form operand is square (rows == k), row-strided, on INT8 planes, in a single GEMM; its partner is any general operand
static bool sym_operand_ok(int sym, bool herm, bool kmajor, size_t rows, size_t k, int dtype) {
    if (sym == kSymNone) return !herm;
    const int base = sym & kSymBase, tri = sym & kTriAny;
    if ((sym & ~(kSymBase | kTriAny | kTriUnit)) || (tri != 0 && tri != kTriStored && tri != kTriMirrored) || (tri == 0 && (sym & kTriUnit)) || (tri != 0 && herm))
        return false;
    return (base == kSymLower || base == kSymUpper) && !kmajor && rows == k && (!herm || is_complex(dtype));
}
template <typename T> static hipError_t launch_amax_sym_pair_t(hipStream_t stream, size_t k, const ExtractOperand& A, const ExtractOperand& B) {
    auto mk = [](const ExtractOperand& o) {
        AmaxSymOperand q{};
        if (o.rows && !o.kmajor) {
            q.X = o.X, q.ld = o.ld, q.rows = o.rows, q.bx = o.xstride, q.amax = o.amax, q.pstride = o.pstride, q.parts = o.parts;
            q.row_groups = (unsigned)((o.rows + 63) / 64), q.sym = o.sym, q.herm = o.herm ? 1 : 0;
        }
        return q;
    };
    const AmaxSymOperand a = mk(A), b = mk(B);
    const size_t nA = (size_t)a.row_groups * a.parts, nB = (size_t)b.row_groups * b.parts;
    if (nA + nB == 0) return hipSuccess;
    if (nA + nB > 0x7FFFFFFFull) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(amax_sym_pair_kernel<T>, dim3((unsigned)(nA + nB)), dim3(256), 0, stream, a, b, (unsigned)nA, k, (size_t)0);
    return hipGetLastError();
}
static hipError_t launch_amax_sym_pair(hipStream_t stream, int dtype, size_t k, const ExtractOperand& A, const ExtractOperand& B) {
    if (g_batch.batch != 1 || A.one_read || B.one_read || !sym_operand_ok(A.sym, A.herm, A.kmajor, A.rows, k, dtype) ||
        !sym_operand_ok(B.sym, B.herm, B.kmajor, B.rows, k, dtype))
        return hipErrorInvalidValue;
    switch (dtype) {
    case kF32: return launch_amax_sym_pair_t<float>(stream, k, A, B);
    case kF64: return launch_amax_sym_pair_t<double>(stream, k, A, B);
    case kC32: return launch_amax_sym_pair_t<float2>(stream, k, A, B);
    case kC64: return launch_amax_sym_pair_t<double2>(stream, k, A, B);
    }
    return hipErrorInvalidValue;
}
static SymStageArgs sym_args(const StageArgs& s, int sym, bool herm) {
    SymStageArgs a{};
    static_cast<StageArgs&>(a) = s;
    a.sym = sym, a.herm = herm ? 1 : 0;
    return a;
}
template <typename T, int MODE> static hipError_t launch_stage_sym_pair_t(hipStream_t stream, bool kmA, SymStageArgs a, bool kmB, const SymStageArgs& b, void* zero_p, size_t zero_bytes) {
    const size_t nA = stage_blocks<T, MODE>(kmA, a), nB = stage_blocks<T, MODE>(kmB, b);
    if (nA + nB == 0 || nA + nB > 0x7FFFFFFFull) return hipErrorInvalidConfiguration;
    if constexpr (MODE == MODE_BOUND) {
        if (zero_p && zero_bytes) a.zero_p = (unsigned*)zero_p, a.zero_words = (unsigned)(zero_bytes / 4);
        hipLaunchKernelGGL(extract_sym_pair_kernel<T>, dim3((unsigned)(nA + nB)), dim3(256), 0, stream, a, b, (unsigned)nA, (int)kmA, (int)kmB);
    } else {
        hipLaunchKernelGGL(quantise_sym_pair_kernel<T>, dim3((unsigned)(nA + nB)), dim3(256), 0, stream, a, b, (unsigned)nA, (int)kmA, (int)kmB);
    }
    return hipGetLastError();
}
template <int MODE> static hipError_t launch_stage_sym_pair(hipStream_t stream, int dtype, bool kmA, const SymStageArgs& a, bool kmB, const SymStageArgs& b, void* zero_p,
                                                            size_t zero_bytes) {
    switch (dtype) {
    case kF32: return launch_stage_sym_pair_t<float, MODE>(stream, kmA, a, kmB, b, zero_p, zero_bytes);
    case kF64: return launch_stage_sym_pair_t<double, MODE>(stream, kmA, a, kmB, b, zero_p, zero_bytes);
    case kC32: return launch_stage_sym_pair_t<float2, MODE>(stream, kmA, a, kmB, b, zero_p, zero_bytes);
    case kC64: return launch_stage_sym_pair_t<double2, MODE>(stream, kmA, a, kmB, b, zero_p, zero_bytes);
    }
    return hipErrorInvalidValue;
}
static hipError_t launch_extract_sym_pair(hipStream_t stream, int dtype, int backend, size_t k, size_t kp, const ExtractOperand& A, const ExtractOperand& B,
                                          void* zero_p, size_t zero_bytes) {
    if (g_batch.batch != 1 || backend != kINT8 || A.one_read || B.one_read || !sym_operand_ok(A.sym, A.herm, A.kmajor, A.rows, k, dtype) ||
        !sym_operand_ok(B.sym, B.herm, B.kmajor, B.rows, k, dtype))
        return hipErrorInvalidValue;
    const SymStageArgs a = sym_args(extract_args(backend, k, kp, A), A.sym, A.herm), b = sym_args(extract_args(backend, k, kp, B), B.sym, B.herm);
    return launch_stage_sym_pair<MODE_BOUND>(stream, dtype, A.kmajor, a, B.kmajor, b, zero_p, zero_bytes);
}
static hipError_t launch_quantise_sym_pair(hipStream_t stream, int dtype, int backend, int t_begin, int t_end, size_t k, size_t kp, const QuantOperand& A,
                                           const QuantOperand& B) {
    if (g_batch.batch != 1 || backend != kINT8 || A.lo2 || B.lo2 || A.f6_rows || B.f6_rows || A.nf || B.nf ||
        !sym_operand_ok(A.sym, A.herm, A.kmajor, A.rows, k, dtype) || !sym_operand_ok(B.sym, B.herm, B.kmajor, B.rows, k, dtype))
        return hipErrorInvalidValue;
    const SymStageArgs a = sym_args(quantise_args(backend, t_begin, t_end, k, kp, A), A.sym, A.herm),
                       b = sym_args(quantise_args(backend, t_begin, t_end, k, kp, B), B.sym, B.herm);
    return launch_stage_sym_pair<MODE_MOD>(stream, dtype, A.kmajor, a, B.kmajor, b, nullptr, 0);
}
static hipError_t launch_fast_shift_sym_pair(hipStream_t stream, int dtype, int backend, unsigned N, size_t k, const QuantOperand& A, const QuantOperand& B) {
    if (g_batch.batch != 1 || backend != kINT8 || !sym_operand_ok(A.sym, A.herm, A.kmajor, A.rows, k, dtype) || !sym_operand_ok(B.sym, B.herm, B.kmajor, B.rows, k, dtype))
        return hipErrorInvalidValue;
    const float log2P = GEMMUL8_LOG2P_INT8[N - 2];
    const size_t rpb = 8 * (16 / (is_f32(dtype) ? 4 : 8) / (is_complex(dtype) ? 2 : 1));  // rows per workgroup of the row-strided forms
    auto operand = [&](const QuantOperand& o) {
        const size_t blocks = o.kmajor ? o.rows : (o.rows + rpb - 1) / rpb;
        ShiftSymOperand q{};
        q.X = o.X, q.ld = o.ld, q.rows = o.rows, q.bx = o.xstride, q.sft = o.sft, q.blocks = (unsigned)blocks, q.kmajor = o.kmajor ? 1 : 0;
        q.sym = o.sym, q.herm = o.herm ? 1 : 0;
        return q;
    };
    if (A.rows + B.rows > 0x7FFFFFFFull) return hipErrorInvalidConfiguration;
    const ShiftSymOperand a = operand(A), b = operand(B);
    const dim3 grid(a.blocks + b.blocks);
    switch (dtype) {
    case kF32: hipLaunchKernelGGL(fast_shift_sym_pair_kernel<float>, grid, dim3(256), 0, stream, a, b, k, log2P, (size_t)0); break;
    case kF64: hipLaunchKernelGGL(fast_shift_sym_pair_kernel<double>, grid, dim3(256), 0, stream, a, b, k, log2P, (size_t)0); break;
    case kC32: hipLaunchKernelGGL(fast_shift_sym_pair_kernel<float2>, grid, dim3(256), 0, stream, a, b, k, log2P, (size_t)0); break;
    case kC64: hipLaunchKernelGGL(fast_shift_sym_pair_kernel<double2>, grid, dim3(256), 0, stream, a, b, k, log2P, (size_t)0); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace oz2
