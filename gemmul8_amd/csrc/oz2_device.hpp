// Device-side helpers shared by the HIP kernels of the Ozaki-II emulation (gfx950 only).
//
// What the reference does with compile-time unrolled templates over num_moduli
// (GEMMul8/src/mod.hpp:638-877, scaling.hpp:237-280) is done with num_moduli as a run-time loop bound; the residues of the
// scaled operands come from the two-level floating-point reduction of oz2_scale.hip (emit4_mod_float).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tables.inc"

namespace oz2 {

constexpr int kINT8 = 0;
constexpr int kFP8 = 1;

// per-modulus constants (built on the host, passed by value in kernargs).  The kernels read p and invp; the remaining fields are the constants of the
// byte-wise integer residue (v_dot4_u32_u8 over the bytes of trunc(x 2^s); retired for the floating-point reduction, CPU models in
// tests/test_residue_math.py) and keep the layout of the kernel-argument blocks.
struct ModConst {
    int p;        // modulus
    float invp;   // RN(1/p)
    unsigned cb[4];  // cb[i] = bytes (c_{4i}, .., c_{4i+3}), c_j = 256^j mod p in [0, p) for the INT8 moduli (p <= 256), the LOW 5
                     // bits of it for the FP8 moduli (p <= 1089); byte 15 is 0
    unsigned cbh[4]; // FP8 moduli: the high part c_j >> 5 (< 35); 0 for INT8
    unsigned k56;    //              (-2^56) mod p in [0, p): correction for the 56-bit two's complement of a negative value
    unsigned k120;   //              (-2^120) mod p: the same for the 120-bit form used when E > 0
};
struct ModTable {
    ModConst mc[20];
};

__device__ __forceinline__ int ilogb0(double x) { return x == 0.0 ? 0 : ilogb(x); }
__device__ __forceinline__ int ilogb0(float x) { return x == 0.0f ? 0 : ilogbf(x); }

// wrapping (mod.hpp:8-12)
__device__ __forceinline__ int wrapping(int a, int p) {
    const int h = p >> 1;
    return (a > h) ? a - p : ((a < -h) ? a + p : a);
}

// symmetric residue of an int32 accumulator: the reference's mod_small (mod.hpp:15-21,58-60);
// result in [-p/2, p/2] with the same representative (checked exhaustively in tests)
__device__ __forceinline__ int mod_i32_sym(int a, int p, int pinv32) {
    const int rem = a - p * __mulhi(a, pinv32);
    return wrapping(rem, p);
}

// The same residue for ODD p and ANY int32 a with full-rate instructions only (v_mul_hi/v_mul_lo_u32 are quarter rate; FP64
// VALU runs at the FP32 rate on gfx950): ONE quotient step in FP64.  a*invp is within 2^-21 of a/p, which is at least 1/(2p)
// away from a rounding tie for odd p, so q = rint(a/p) exactly and a - q*p (integers below 2^53: the fma is exact) is the
// canonical representative in [-(p-1)/2, (p-1)/2] -- identical to mod_i32_sym (CPU model over the whole int32 range in
// tests/test_residue_math.py, bit-for-bit by the GPU parity tests).  Five instructions against ten for two fp32 steps.
__device__ __forceinline__ int mod_i32_sym_odd_f64(int a, double p, double invp) {
    const double x = (double)a;
    const double q = rint(x * invp);
    return (int)fma(-q, p, x);
}
// 0 <= s < 2^22, odd p: s * |RN(1/p) - 1/p| <= 2^22 2^-24 / p < 1/(2p), so fma(s, RN(1/p), 2^23) rounds (RN-even at unit spacing) to
// 2^23 + q with q = rint(s / p) exactly; the low 24 bits of its bit pattern are q, which v_mad_i32_i24(bits, -p, s) = s - q p turns
// into the canonical residue in [-(p-1)/2, (p-1)/2].  (The asm pins the full-rate 24-bit multiply-add: left to itself the compiler sees that only the low bits of
// the result are kept and picks the quarter-rate v_mul_lo_u32 / v_mad_u64_u32.)
__device__ __forceinline__ int mod_small_sym_u(unsigned s, int p, float invp) {
    const float qf = fmaf((float)s, invp, 8388608.0f);
    int r;
    asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(r) : "v"(__float_as_int(qf)), "s"(-p), "v"(s));
    return r;
}
// |a| < 2^16: one exact step
__device__ __forceinline__ int mod_small_sym_odd(int a, int p, float invp) {
    return a - __mul24((int)rintf((float)a * invp), p);
}

// ---------------------------------------------------------------- OCP FP8 e4m3 helpers (FP8 backend)
// two small integers (|v| <= 16, exactly representable) -> two e4m3 bytes in the low half of the result
__device__ __forceinline__ unsigned fp8x2_from_ints(int a, int b) {
    return (unsigned)__builtin_amdgcn_cvt_pk_fp8_f32((float)a, (float)b, 0, false) & 0xFFFFu;
}
// smallest e4m3 value >= a for 0 <= a < 448 (restates fp8_e4m3_ru, scaling.hpp:48-54: RN conversion, then
// one encoding step up if the result fell below a)
template <typename U> __device__ __forceinline__ unsigned fp8_round_up(U a) {
    unsigned r = (unsigned)__builtin_amdgcn_cvt_pk_fp8_f32((float)a, 0.0f, 0, false) & 0xFFu;
    const float y = __builtin_amdgcn_cvt_f32_fp8((int)r, 0);
    return r + ((U)y < a ? 1u : 0u);
}
__device__ __forceinline__ float fp8_to_float(unsigned byte) { return __builtin_amdgcn_cvt_f32_fp8((int)byte, 0); }

// FP8 residue splitting (mod.hpp:159-189).  Square moduli p = s^2 (t < 6): a = s*hi + lo, hi = rint(a/s);
// otherwise a = 16*hi + lo with hi = sign(a)*ceil(|a|/16) and a third value hi + lo.
// (hi keeps the sign of zero: rintf(-0.09) = -0.0f is stored as the e4m3 byte 0x80, exactly like the reference)
__device__ __forceinline__ void fp8_split_sq(int a, int s, float inv_s, float& hi, float& lo) {
    const float af = (float)a;
    hi = rintf(af * inv_s);
    lo = fmaf(-(float)s, hi, af);
}
__device__ __forceinline__ unsigned fp8x2_from_floats(float a, float b) {
    return (unsigned)__builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false) & 0xFFFFu;
}
__device__ __forceinline__ void fp8_split_kara(int a, int& hi, int& lo) {
    const unsigned absu = (unsigned)(a < 0 ? -a : a);
    const int q = (int)((absu + 15u) >> 4);
    hi = a < 0 ? -q : q;
    lo = a - 16 * hi;
}

}  // namespace oz2
