// INT8 x INT8 -> INT32 "TN" GEMM on gfx950 MFMA with fused epilogues (Ozaki-II hot loop).
//
// Replaces the vendor-BLAS call sites of the reference (GEMMul8/src/matmult.hpp:120-175 i8x1,
// :213-302 i8x3) AND the separate requantise pass (src/conv_hi2mid_real.hpp:9-25,
// src/conv_hi2mid_complex.hpp:9-127) / the bound-matrix max passes
// (src/scaling_accu_real.hpp:142-226, src/scaling_accu_complex.hpp:132-224): the INT32 accumulators
// never leave registers.
//
//   C(i,j) = sum over K-segments s, kk:  A_s(i,kk) * B_s(j,kk)        operands K-contiguous ("TN")
//   EPI_MOD  : out(i,j)  = int8( symmetric residue of C mod p_t )                      (real C_mid, complex X/Y partials)
//   EPI_CPLX : C = Z = (Ar+Ai)(Br+Bi); reads the residues rx, ry of X = ArBr, Y = AiBi written by two
//              EPI_MOD launches and stores interleaved (Cr, Ci) = (X-Y, Z-X-Y) mod p_t   (conv_hi2mid_complex.hpp:9-26)
//   EPI_MAX  : rowmax[i] = max_j C(i,j), colmax[j] = max_i C(i,j) (atomicMax)           (accurate-mode bound GEMM)
// Up to 3 K-segments are concatenated (virtual K = nseg*kp): the complex bound matrices
// ArBi+AiBr and ArBi+AiBr+(Ar-Ai)(Br-Bi) are single GEMMs this way.
//
// Kernel structure (CDNA4), see DESIGN.md 3.1 for the measurements behind each choice:
//  * PERSISTENT: one workgroup per CU loops over 256x256 output tiles.  12 waves: 8 CONSUMER waves (2(M) x 4(N), wave tile
//    128x64 = 8x4 v_mfma_i32_16x16x64_i8 accumulator tiles = 128 registers/lane) + 4 PRODUCER waves (one per SIMD) that only
//    issue the LDS-DMA (global_load_lds_dwordx4, SGPR base + one VGPR offset per instruction), so the matrix pipe's feeders
//    never block on the VMEM queue and spend no VALU cycles on addresses.  168 VGPRs -> 3 waves/SIMD.
//  * BK = 128 bytes (every DMA row segment is a full 128-B line: the global->LDS path does 127 GB/s/CU with 128-B segments,
//    68 with 64-B ones).  LDS = a 2.5-stage ring of five 32 KiB operand panels: panel h = 2g + isB of K-step g in slot h % 5;
//    during K-step g the A producers fetch A(g+2), 2 instructions in every slot, the B producers B(g+1), 4 instructions in
//    slots 0-3 (smooth issue matters as much as depth: see the producer branch).
//  * LDS rows are 128 B; the 16-B chunk index is XOR-swizzled with (row>>1)&7 on the DMA SOURCE address
//    (the destination must stay lane-linear) and on the ds_read_b128 address: every 16-lane read group hits
//    16 distinct 16-B bank slots (SQ_LDS_BANK_CONFLICT = 0).
//  * Ping-pong schedule (k > 4096; K-step-barrier schedule below that, see launch<EPI>): each consumer alternates a LOAD segment
//    (4-8 ds_read_b128) and an MFMA segment (16 MFMAs, s_setprio 1), four of each per K-step, one s_barrier after each; the wm=1 half runs one segment behind the wm=0 half
//    so on every SIMD one wave feeds the matrix pipe while its partner reads LDS.  With g counting K-steps across tiles:
//      slot(wm=0: L_j(g)) = 8g+2j, M_j -> +1 (j = 0..3); wm=1 one slot later; the producers drain what K-step g+1 needs in slot 8g+7.
//      WAR: the slots refilled during K-step g held panels of K-steps g-1 (-> B(g+1)) and g-2/g-1 (-> A(g+2)), last read in
//           wm=1's L3(g-1) (slot 8g-1) < the first DMA of K-step g (slot 8g).
//      RAW: the producers' vmcnt wait + barrier closes slot 8g+7; wm=0's L0(g+1) opens slot 8g+8.
//  * Workgroup -> tile mapping is XCD-aware and chunked (oz2_gemm_common.hpp): the 32 CUs of an XCD share 8+4 operand
//    panels through their L2 (measured TCC hit rate 81 %) and all XCDs work on one plane, so misses land in the Infinity Cache.
//  * Cost split measured with real-data probes (tools/experiments/probes; 16x16x64 kernel, k = 8192): the board's
//    power-limited ceiling for this instruction on residue data is 3.97 POP/s, MFMA + barriers alone reach 93 % of it; the
//    L2 -> LDS operand path costs 13 %, the per-segment barriers 7 %, the epilogue 6 %, the LDS reads 5 %.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <cstdlib>
#include <type_traits>

#include "oz2_crt_common.hpp"
#include "oz2_gemm_common.hpp"
#include "oz2_gemm_i8_epi.hpp"
#include "oz2_kernels.h"

namespace oz2 {

#ifndef OZ2_PB
#define OZ2_PB 4
#endif
#ifndef OZ2_KBAR_MAX_KP
#define OZ2_KBAR_MAX_KP 5120  // padded k up to which the K-step-barrier schedule is used (see launch<EPI>); 0 = never, 1 << 30 = always.  Round 4 (after the epilogue / tile-prologue work): +1.0 / +1.3 % at k = 4608 / 5120 on 8192^2 x 14 planes, +0.5 % at 5120 on 16384^2 x 6; at 6144 +0.9 % / -1.1 %, at 7168 0 / -1.3 %, at 8192 -1.3 % (profiles/archive/r04_gemm_ab_kbar_threshold.txt)
#endif
#ifndef OZ2_SBS_DEFAULT
#define OZ2_SBS_DEFAULT 1  // whether the residue launches of the ping-pong schedule take gemm_i8_sbs_kernel when GEMMUL8_GEMM_SBS is unset (see launch<EPI>)
#endif
#ifndef OZ2_SBS_MAX_TILES
#define OZ2_SBS_MAX_TILES 1024  // ... for planes of at most this many 256 x 256 tiles.  Interleaved against the parent build, 14 planes of a real quantise pass, 25 pairs: 8192^2 x 6144 / 8192 launch -1.68 / -1.31 % (22 / 7.5 s.e.), whole call 8192^2 x 6144 / 8192 -1.35 / -0.98 % (16 / 10.5 s.e.); 16384^2 x 8192 (4096 tiles) launch +0.85 % SLOWER (5.5 s.e.; +0.39 % on a second box): off there (profiles/r10_sbs_epilogue_ab.txt)
#endif
#ifndef OZ2_SLEEP_A
#define OZ2_SLEEP_A 4  // s_sleep units (64 clocks) between the A producers' 8 groups of 2 LDS-DMA instructions
#endif
#ifndef OZ2_SLEEP_B
#define OZ2_SLEEP_B 4  // ... between the B producers' 4 groups of 4
#endif
constexpr int RING_LDS_BYTES = 5 * TILE_BYTES;  // five 32 KiB operand panels = the whole 160 KiB of LDS

// Persistent, wave-specialised kernel: one workgroup per CU (all 160 KiB of LDS) loops over tiles vb = blockIdx.x,
// blockIdx.x + gridDim.x, ...; 8 consumer waves (2 x 4, each 128 x 64 of the 256 x 256 tile) run MFMA + epilogue, 4
// producer waves only issue LDS-DMA into a 2.5-stage ring of operand panels (see the producer branch): A panels are fetched
// two K-steps ahead with their 16 instructions per wave spread evenly over the K-step, B panels one K-step ahead -- smooth
// issue matters as much as depth (all 16 in one slot: +7 % kernel time; the ring with even issue: -6..9 % against the
// two-stage pipeline at every k).  The K pipeline runs straight through tile boundaries: while the consumers
// are in the last K-step and the epilogue of a tile the producers already fetch the first K-tile of the next one, the
// epilogue's stores drain behind the next tile's MFMAs, and there is no workgroup launch / LDS re-allocation between
// tiles -- a non-persistent version of this kernel lost ~11 us of a ~120 us tile to those three.
// FUSE: always 0 in libgemmul8.so.  The laboratory build of tools/experiments/fused_crt instantiates FUSE = 1 | 2 (double | float output): the
// TILE-STATIONARY order -- a workgroup runs all args.planes residue planes of one output tile back to back and accumulates the CRT of the
// tile inside the kernel (bit-exact, measured 10-28 % slower than the two-launch path: DESIGN.md 3.4).
struct NoCrt {
    int unused;
};
#ifdef OZ2_LAB_FUSED_CRT
#include OZ2_LAB_FUSED_CRT  // i8_crt_tail, i8_producer_crt
#endif
// Re-initialisation of the accumulators by the (idle) matrix pipe, sub-block by sub-block BEHIND the epilogue's reads (round 6): as soon as the residue
// epilogue has reduced the four accumulator tiles of a sub-block (hook phase 0), four MFMAs on all-zero fragments with C = the start value rewrite them --
// 32 matrix instructions per wave and tile on a pipe that has nothing else to do, instead of 128 v_mov_b32 at the head of the next tile on the vector
// ALU that the two waves' epilogues (~650 instructions each) are bound by.
template <bool ZERO> struct MfmaReinitHook {  // ZERO: the start value is 0 (short-K launches, the only instantiation): the C operand is the inline constant
    v4i (*acc)[4];
    int acc0;
    __device__ __forceinline__ void operator()(int sb, int phase) const {
        if (phase != 0) return;
        const int tj = sb >> 1, tg = sb & 1;
        const v4i z = {0, 0, 0, 0};
        const v4i c = ZERO ? v4i{0, 0, 0, 0} : v4i{acc0, acc0, acc0, acc0};
        __builtin_amdgcn_sched_barrier(0);  // not above the reduction's last read of these registers (a hoisted definition needs a second register set)
#pragma unroll
        for (int ti = 0; ti < 4; ++ti)  // B = the dead accumulator tile itself (times an all-zero A): four DISTINCT instructions -- on identical operands the
            acc[tg * 4 + ti][tj] = __builtin_amdgcn_mfma_i32_16x16x64_i8(z, acc[tg * 4 + ti][tj], c, 0, 0, 0);  // compiler keeps one and copies its result three times
    }
};
// SMALLK: the launch has K <= 512 (accumulators start at 0, three-instruction residue); the epilogue form is a compile-time property of the kernel
#define OZ2_I8_KR 0
#define OZ2_I8_SBS 0
#define OZ2_I8_KERNEL_HEAD                                       \
    template <int EPI, bool KBAR, int FUSE, bool SMALLK = false> \
    __global__ void __launch_bounds__(WS_THREADS) gemm_i8_kernel(const GemmArgs args, const std::conditional_t<FUSE != 0, CrtArgs, NoCrt> crt)
#include "oz2_gemm_i8_kernel.inc"
#undef OZ2_I8_KERNEL_HEAD
// The ping-pong schedule with the two wave halves' tile epilogues SIDE BY SIDE (see OZ2_I8_SBS in the kernel text): the residue launch above
// OZ2_KBAR_MAX_KP takes it (launch<EPI_MOD>, GEMMUL8_GEMM_SBS).  A kernel of its own name, <EPI_MOD, false, 0, false> its only instantiation.
#undef OZ2_I8_SBS
#define OZ2_I8_SBS 1
#define OZ2_I8_KERNEL_HEAD                               \
    template <int EPI, bool KBAR, int FUSE, bool SMALLK> \
    __global__ void __launch_bounds__(WS_THREADS) gemm_i8_sbs_kernel(const GemmArgs args, const NoCrt crt)
#include "oz2_gemm_i8_kernel.inc"
#undef OZ2_I8_SBS
#define OZ2_I8_SBS 0
#undef OZ2_I8_KR
#undef OZ2_I8_KERNEL_HEAD
// The K-RANGED form of the same kernel (gemmul8_trmm; krange = a KRange of oz2_gemm_common.hpp, never 0): a tile runs only the K-steps [k0, k1) of its
// range.  Producer and consumer waves derive the (scalar) range from the tile they map anyway.  The producers' panel sequence is the concatenation of the
// tiles' ranges: kin starts at the tile's k0, PRODUCER_ADVANCE moves to the next tile at k1 -- which carries the look-ahead across the tile boundary: the
// next tile's first panels are fetched under the current tile's last K-steps and epilogue as before --, the producers' barrier loop and the consumers' K loop
// both run k1 - k0 steps of the tile, and the ring's slots advance per panel issued / per K-step run, so they count the K-steps actually run.  SMALLK and
// acc0 stay launch properties derived from kp: fewer K-steps only make their bounds looser.  Residue launches of one K segment only (never the bound GEMM).
// A kernel of its own NAME, compiled from the same text: every other launch keeps its symbol and its code (tests/test_kernel_resources.py counts them).
#define OZ2_I8_KR 1
#define OZ2_I8_KERNEL_HEAD                           \
    template <int EPI, bool KBAR, int FUSE, bool SMALLK> \
    __global__ void __launch_bounds__(WS_THREADS) gemm_i8_kr_kernel(const GemmArgs args, const NoCrt crt, const int krange)
#include "oz2_gemm_i8_kernel.inc"
#undef OZ2_I8_KR
#undef OZ2_I8_SBS
#undef OZ2_I8_KERNEL_HEAD

static void fill_common(GemmArgs& a, size_t kp, size_t m, size_t n) {
    a.kp = (int)kp;
    a.m = (int)m;
    a.n = (int)n;
    a.tiles_m = (int)((m + BM - 1) / BM);
    a.tiles_n = (int)((n + BN - 1) / BN);
    for (int t = 0; t < 20; ++t) {
        const int p = GEMMUL8_MODULI_INT8[t];
        a.moduli[t] = p;
        a.pinv32[t] = (int)(4294967296ull / (unsigned long long)p);
        a.dotw[t] = 1u | ((256u % p) << 8) | ((65536u % p) << 16) | ((16777216u % p) << 24);
        a.dotc[t] = (unsigned)((p - (int)(2147483648u % (unsigned)p)) % p);
    }
}

static int num_cus() {
    static int n = 0;
    if (!n) {
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess || prop.multiProcessorCount <= 0) return 256;
        n = prop.multiProcessorCount;
    }
    return n;
}

template <int EPI, bool KBAR, int FUSE = 0, bool SMALLK = false, bool KR = false, bool SBS = false>
static hipError_t launch_sched(hipStream_t stream, GemmArgs& a, const std::conditional_t<FUSE != 0, CrtArgs, NoCrt>& crt = {}, [[maybe_unused]] int krange = 0) {
    // the attribute belongs to the function on ONE device; setting it is idempotent, so concurrent first calls from several host
    // threads only need the flag itself to be race-free
    static std::atomic<bool> attr_set_dev[64];
    int dev_ = 0;
    if (hipGetDevice(&dev_) != hipSuccess || dev_ < 0 || dev_ >= 64) dev_ = 0;
    if (!attr_set_dev[dev_].load(std::memory_order_acquire)) {
        const void* fn;
        if constexpr (KR) fn = (const void*)gemm_i8_kr_kernel<EPI, KBAR, FUSE, SMALLK>;
        else if constexpr (SBS) fn = (const void*)gemm_i8_sbs_kernel<EPI, KBAR, FUSE, SMALLK>;
        else fn = (const void*)gemm_i8_kernel<EPI, KBAR, FUSE, SMALLK>;
        hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, RING_LDS_BYTES);
        if (e != hipSuccess) return e;
        attr_set_dev[dev_].store(true, std::memory_order_release);
    }
    // persistent: one workgroup per CU; a multiple of 8 keeps "workgroup b runs on XCD b % 8" aligned with map_tile.
    // Measured interleaved against one-workgroup-per-tile launches of the same kernel (tools/gemm_ab.py, 8192 x 8192 x k,
    // 14 planes): 13 % faster at k = 256, 7 % at k = 2048, 1 % at k = 8192.
    int grid = num_cus() & ~7;
    if (const int want = knobs().gemm_cus; want > 0 && want < grid) grid = want;  // measurement switch (oz2_knobs.hpp): same results
    if (grid <= 0) grid = 8;
    if (a.total_tiles < grid) grid = a.total_tiles;
    if constexpr (KR) hipLaunchKernelGGL((gemm_i8_kr_kernel<EPI, KBAR, FUSE, SMALLK>), dim3(grid), dim3(WS_THREADS), RING_LDS_BYTES, stream, a, crt, krange);
    else if constexpr (SBS) hipLaunchKernelGGL((gemm_i8_sbs_kernel<EPI, KBAR, FUSE, SMALLK>), dim3(grid), dim3(WS_THREADS), RING_LDS_BYTES, stream, a, crt);
    else hipLaunchKernelGGL((gemm_i8_kernel<EPI, KBAR, FUSE, SMALLK>), dim3(grid), dim3(WS_THREADS), RING_LDS_BYTES, stream, a, crt);
    return hipGetLastError();
}

// Two schedules of the same tile loop (bit-identical results): with a workgroup barrier after every LOAD / MFMA segment (ping-pong)
// or with one barrier per K-step.  Interleaved on one box (tools/gemm_ab.py, 8192^2 x k, 14 planes, profiles/archive/r02_sched_ab.txt): the
// K-step-barrier form is faster by 10 / 7.5 / 4.7 / 2.4 % at k = 512 / 1024 / 2048 / 4096 (tile boundaries -- epilogue beside the
// other half's first K-steps -- overlap better) and 2.4 % slower at k = 8192, where the board is power-bound and removing stalls
// buys nothing while the s_sleep-paced LDS-DMA is a little less smooth than the barrier-paced one.
// tri: 0 = every tile, 1 / 2 = only the tiles of the lower / upper triangle of a square product (make_tile_map_tri; diagonal tiles whole)
// krange (KRange, oz2_gemm_common.hpp): != 0 = every tile runs only the K-steps of its range (gemmul8_trmm; the rectangle walk, a single item)
template <int EPI> static hipError_t launch(hipStream_t stream, GemmArgs& a, int planes, int tri = 0, int krange = 0) {
    // batched call: the items' planes are one long plane sequence (item-major), the persistent tile loop runs over all of them
    a.ppi = planes;
    a.m_ppi = map_magic((unsigned)planes);
    a.bstride = g_batch.ws;
    planes *= (int)g_batch.batch;
    if (tri != 0 && (EPI == EPI_MAX || a.tiles_m != a.tiles_n)) return hipErrorInvalidValue;
    if (krange != 0 && (EPI == EPI_MAX || tri != 0 || a.nseg != 1 || g_batch.batch != 1 || krange < kKrALower || krange > kKrBLow)) return hipErrorInvalidValue;
    // (the ranged operand is square: its tile count along the ranged dimension is kp / 256, which keeps every range non-empty and inside [0, KT))
    if (krange != 0 && (krange <= kKrAUpper ? a.tiles_m : a.tiles_n) != a.kp / 256) return hipErrorInvalidValue;
    a.total_tiles = tri ? planes * (a.tiles_m * (a.tiles_m + 1) / 2) : planes * a.tiles_m * a.tiles_n;
    if (a.total_tiles <= 0) return hipSuccess;
    a.colblock = tri ? 0 : map_colblock((size_t)a.tiles_n, (size_t)a.kp * (size_t)a.nseg);  // no column blocks in the triangular walk
    a.map = tri ? make_tile_map_tri(a.tiles_m, tri) : make_tile_map(a.tiles_m, a.tiles_n, a.colblock);
    a.acc0 = (size_t)a.kp * (size_t)a.nseg <= 512 ? 0 : (int)0x80000000u;  // RED_ODD_SMALL needs |sum| < 2^23
    // (the bound GEMM keeps the ping-pong schedule at every k.  In round 2 its K-step-barrier instantiation spilled accumulators INSIDE
    // the MFMA loop; with the round-3 source it no longer does, but the single-plane launch still runs slower with it: bounds phase
    // 88.4 -> 92.4 us at 3072^3, 130.9 -> 134.6 at 4096^3, equal at 2048^3 and 8192^3.  round-3 A/B: profiles/archive/r03_bound_ab.txt)
    // (A float-pattern accumulator form for K <= 256 -- two instead of three instructions per accumulator in the residue epilogue -- was built in round 6:
    // bit-identical, measured neutral, -1 / -2 % at 8192^2 x 128 / 256 and +1 % at 16384^2 x 256, profiles/r06_short_k_epilogue_ab.txt: retired.)
    if constexpr (EPI != EPI_MAX) {
        if (krange != 0) {  // the same three schedules, K-ranged
            if (a.acc0 == 0) return launch_sched<EPI, true, 0, true, true>(stream, a, {}, krange);
            if (a.kp <= OZ2_KBAR_MAX_KP) return launch_sched<EPI, true, 0, false, true>(stream, a, {}, krange);
            return launch_sched<EPI, false, 0, false, true>(stream, a, {}, krange);
        }
        if (a.acc0 == 0) return launch_sched<EPI, true, 0, true>(stream, a);  // K <= 512
        if (a.kp * a.nseg <= OZ2_KBAR_MAX_KP) return launch_sched<EPI, true>(stream, a);
    }
    // the ping-pong schedule.  Its residue launch (any tile walk) has a second form, the two halves' epilogues side by side (gemm_i8_sbs_kernel):
    // GEMMUL8_GEMM_SBS=0|1 forces one of them, bit-identical planes (tests/test_gpu_gemm_sbs.py)
    if constexpr (EPI == EPI_MOD) {
        if (const int sbs = knobs().gemm_sbs; sbs == 1 || (sbs < 0 && OZ2_SBS_DEFAULT && a.tiles_m * a.tiles_n <= OZ2_SBS_MAX_TILES)) return launch_sched<EPI_MOD, false, 0, false, false, true>(stream, a);
    }
    return launch_sched<EPI, false>(stream, a);
}

// Non-temporal residue stores.  The residue planes are written once and read once, by the CRT pass, N planes later; written with the
// default policy they are allocated in the 256 MiB Infinity Cache on their way to HBM and push out the operand planes A_lo / B_lo,
// which the quantise kernels have just left there and which every plane's 32 x 32 tiles re-read through eight L2s.  When ALL operand
// planes of the launch fit the Infinity Cache, keeping them there is worth 8-14 % of the WHOLE call (8192^2: k = 256 / 512 / 1024
// 0.917 -> 0.815 / 1.059 -> 0.940 / 1.470 -> 1.285 ms; 16384^2: k = 256 / 512 3.22 -> 2.88 / 3.88 -> 3.59 ms); when they do not fit
// there is nothing to protect and the CRT pass loses the tail of C_mid it would have found in the cache (-0.5 ... -2 % from k = 1536
// at 8192^2, k = 1024 at 16384^2); with small outputs (4096^2 and below) it is a wash.  profiles/archive/r03_epi_nt_grid.txt
static int nt_residue_planes(const GemmArgs& a, int planes, bool stream_out, bool automatic = true) {
    if (const int force = knobs().epi_nt; force >= 0) return force == 1 && stream_out ? planes : 0;  // testing switch: one policy for all planes (same results)
    if (!stream_out || !automatic) return 0;
    const size_t all = (size_t)planes * g_batch.batch;
    const size_t operands = all * (a.strideA + a.strideB), residues = all * a.strideO;
    // (keeping the default policy for the last 2-6 planes, so that the CRT finds them in the cache, non-temporal stores for the
    // leading planes of launches whose operands do NOT fit, and walking the planes last to first -- the order the quantise kernels
    // left them in the cache -- were all measured: no consistent gain, profiles/archive/r03_epi_nt_keep.txt; between 240 and ~450 MiB of
    // operand planes the sign of the effect differs from box to box, -2 ... +4 %)
    return residues >= ((size_t)256 << 20) && operands <= ((size_t)240 << 20) ? planes : 0;
}

hipError_t launch_gemm_i8_mod(hipStream_t stream, const int8_t* A, const int8_t* B, size_t strideA, size_t strideB, size_t kp, size_t m,
                              size_t n, int t_begin, int t_end, int8_t* out, size_t ldo, size_t strideO, bool stream_out, int tri, int krange) {
    GemmArgs a{};
    a.A[0] = A;
    a.B[0] = B;
    a.nseg = 1;
    a.strideA = strideA;
    a.strideB = strideB;
    a.t_begin = t_begin;
    a.out = out;
    a.ldo = ldo;
    a.strideO = strideO;
    fill_common(a, kp, m, n);
    a.nt_planes = nt_residue_planes(a, t_end - t_begin, stream_out);
    return launch<EPI_MOD>(stream, a, t_end - t_begin, tri, krange);
}

hipError_t launch_gemm_i8_cplx(hipStream_t stream, const int8_t* A, const int8_t* B, size_t strideA, size_t strideB, size_t kp, size_t m,
                               size_t n, int t_begin, int t_end, const int8_t* rx, const int8_t* ry, size_t strideR, int8_t* out,
                               size_t ldo, size_t strideO, int tri, int krange) {
    GemmArgs a{};
    a.A[0] = A;
    a.B[0] = B;
    a.nseg = 1;
    a.strideA = strideA;
    a.strideB = strideB;
    a.t_begin = t_begin;
    a.out = out;
    a.ldo = ldo;
    a.strideO = strideO;
    a.rx = rx;
    a.ry = ry;
    a.strideR = strideR;
    fill_common(a, kp, m, n);
    // (the size rule of nt_residue_planes LOSES 1-3 % of the whole call on this launch -- ZGEMM 8192^2 x 512 ... 8192, 14 moduli; CGEMM x 768 ...
    // 2048, 7 moduli: the operand planes of the three parts never fit the Infinity Cache together, and the CRT finds more of the
    // interleaved plane there with the default policy -- so the combine launch keeps the default policy unless GEMMUL8_EPI_NT forces it)
    a.nt_planes = nt_residue_planes(a, t_end - t_begin, true, false);
    return launch<EPI_CPLX>(stream, a, t_end - t_begin, tri, krange);
}

#ifndef OZ2_MAX_SMALL_TILES
#define OZ2_MAX_SMALL_TILES 128  // the bound GEMM takes the 128 x 128-tile kernel when (batch x) its 256 x 256 tiles number at most this (of 256 CUs): bounds phase 33 -> 28 / 41 -> 32 / 66 -> 55 us at 512^3 / 1024^3 / 2048^3, but 98 -> 111 us at 3072^3 (144 tiles), profiles/archive/r03_bound_ab.txt
#endif
// mid_seg > 0: the row / column maxima are taken twice per tile -- of the partial sums after the first mid_seg K-segments and of the
// full sums.  The complex bound (max over the elements of C1 = ArBi + AiBr and of C1 + C0, C0 = (Ar-Ai)(Br-Bi)) is then ONE launch over
// three segments with mid_seg = 2 (three real GEMMs of work) instead of a 2-segment and a 3-segment launch (five).
hipError_t launch_gemm_i8_max(hipStream_t stream, int nseg, const int8_t* const* A, const int8_t* const* B, size_t kp, size_t m, size_t n,
                              int* rowmax, int* colmax, int mid_seg) {
    {
        // GEMMUL8_BOUND_TILE = 128 | 256 forces one kernel (tests run every case through both; the maxima are identical)
        const int force = knobs().bound_tile;
        const size_t tiles = ((m + BM - 1) / BM) * ((n + BN - 1) / BN) * g_batch.batch;
        const bool small = force == 128 ? true : force == 256 ? false : tiles <= (size_t)OZ2_MAX_SMALL_TILES;
        if (small) return launch_gemm_i8_max_small(stream, nseg, A, B, kp, m, n, rowmax, colmax, mid_seg);
    }
    GemmArgs a{};
    for (int s = 0; s < nseg; ++s) a.A[s] = A[s], a.B[s] = B[s];
    a.nseg = nseg;
    a.rowmax = rowmax;
    a.colmax = colmax;
    a.kt_mid = mid_seg > 0 && mid_seg < nseg ? mid_seg * (int)(kp / BK) : 0;
    fill_common(a, kp, m, n);
    return launch<EPI_MAX>(stream, a, 1);
}

}  // namespace oz2
