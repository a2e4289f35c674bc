// The body of the persistent residue / bound GEMM kernel, included by oz2_gemm_i8.hip once per kernel NAME behind the includer's template head and
// signature (OZ2_I8_KERNEL_HEAD): gemm_i8_kernel with OZ2_I8_KR 0 -- the text every launch before gemmul8_trmm compiled, token for token -- and
// gemm_i8_kr_kernel with OZ2_I8_KR 1, the K-ranged form (see there).  Everything the K ranges add sits behind #if OZ2_I8_KR or in a hook macro that is
// empty without it.  gemm_i8_sbs_kernel with OZ2_I8_SBS 1 is the ping-pong schedule with the two halves' epilogues SIDE BY SIDE: the lagging half
// (wm = 1) takes the last barrier of a tile -- the one behind the MFMAs of segment (ks2, ah) = (1, 1) of the tile's last K-step -- behind its epilogue
// and the next tile's accumulator initialisation instead of in front of them (behind #if OZ2_I8_SBS; everything else is the same text).
OZ2_I8_KERNEL_HEAD {
#ifndef OZ2_LAB_FUSED_CRT
    static_assert(FUSE == 0, "the in-kernel CRT forms are laboratory code: tools/experiments/fused_crt");
#endif
    static_assert(FUSE == 0 || EPI == EPI_MOD, "the CRT tail follows the real requantise epilogue");
    static_assert(offsetof(CrtArgs, Cmid) == 0 && alignof(CrtArgs) == 8, "i8_crt_tail locates the block in the kernel-argument segment");
    (void)crt;
#if OZ2_I8_KR
    static_assert(EPI != EPI_MAX && FUSE == 0, "K ranges: residue launches of a single K segment");
#define OZ2_I8_MAP_TILE(vb_) map_tile<true, true>((vb_), total, args.map)
#define OZ2_I8_KSTEPS(tmap_) tile_ksteps(tmap_)
#else
#define OZ2_I8_MAP_TILE(vb_) map_tile<EPI != EPI_MAX>((vb_), total, args.map)
#define OZ2_I8_KSTEPS(tmap_) KT
#endif
    const int planes_per_tile = FUSE ? args.planes : 1;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int KT1 = args.kp / BK;    // K-steps per segment
    const int KT = KT1 * args.nseg;  // K-steps per tile
    const int total = args.total_tiles;
    const int G = gridDim.x;
#if OZ2_I8_KR
    (void)KT;  // (one K segment: a tile's K-steps come from its range)
    // K-steps of a tile: the count both the producers' barrier loop and the consumers' K loop run for it
    auto tile_ksteps = [&](const TileMap& t) {
        int k0, k1;
        tile_krange(krange, KT1, t.tm, t.tn, k0, k1);
        return __builtin_amdgcn_readfirstlane(k1 - k0);
    };
#endif

    if (wave >= 8) {  // ------------------------------ producer waves: LDS-DMA only
#ifdef OZ2_LAB_FUSED_CRT
        if constexpr (KBAR && FUSE != 0) {
            i8_producer_crt<FUSE>((__attribute__((address_space(3))) char*)smem,  // CRT on the producer waves: out of line (see there)
                                  (const __attribute__((address_space(4))) char*)__builtin_amdgcn_kernarg_segment_ptr());
            return;
        }
#endif
#if OZ2_I8_KR
#define OZ2_PRODUCER_MAP_TILE(vb_) OZ2_I8_MAP_TILE(vb_)
#define OZ2_PRODUCER_KR_DECL() int kfirst = 0, kend = KT1  /* the K range of the tile whose panels are fetched next */
#define OZ2_PRODUCER_KR_SET(tmap_) tile_krange(krange, KT1, (tmap_).tm, (tmap_).tn, kfirst, kend)
#define OZ2_PRODUCER_KR_ENTER() kin = kfirst
#define OZ2_PRODUCER_KEND kend
#endif
#include "oz2_gemm_i8_producer.inc"
        if constexpr (KBAR) {
        // ONE workgroup barrier per K-step (see the consumer branch).  Without per-segment barriers to pace them the producers space
        // their instructions with s_sleep (64 clocks per unit): bursts of LDS-DMA cost (all 16 at once: +7 % kernel time).
        for (int vb = blockIdx.x; vb < total; vb += G) {
#if OZ2_I8_KR
            const int nk = OZ2_I8_KSTEPS(OZ2_I8_MAP_TILE(vb));
            for (int kt = 0; kt < nk; ++kt) {
#else
            for (int kt = 0; kt < KT * planes_per_tile; ++kt) {
#endif
                const bool issued = more && OZ2_HOOK_DMA_ON(vb == (int)blockIdx.x);
                if (issued) {
                    PRODUCER_BEGIN();
                    if (isB) {  // needed next K-step: 4 groups of 4 in the first part of the K-step
#pragma unroll
                        for (int gq = 0; gq < 4; ++gq) {
#pragma unroll
                            for (int q = 0; q < 4; ++q) PRODUCER_DMA(fsrc, gq * 4 + q, fdst);
                            __builtin_amdgcn_s_sleep(OZ2_SLEEP_B);
                        }
                    } else {    // needed in two K-steps: 8 groups of 2 over the whole K-step
#pragma unroll
                        for (int gq = 0; gq < 8; ++gq) {
#pragma unroll
                            for (int q = 0; q < 2; ++q) PRODUCER_DMA(fsrc, gq * 2 + q, fdst);
                            __builtin_amdgcn_s_sleep(OZ2_SLEEP_A);
                        }
                    }
                    PRODUCER_ADVANCE();
                }
                // the panel needed NEXT K-step must have landed: for the A producers everything except the 16 instructions just issued
                if (!isB && issued) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
                else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
            }
        }
        } else {
        for (int vb = blockIdx.x; vb < total; vb += G) {
#if OZ2_I8_KR
            const int nk = OZ2_I8_KSTEPS(OZ2_I8_MAP_TILE(vb));
            for (int kt = 0; kt < nk; ++kt) {
#else
            for (int kt = 0; kt < KT * planes_per_tile; ++kt) {
#endif
                // A producers: A(g+2); B producers: B(g+1); afterwards the panel needed NEXT K-step must have landed, which
                // for the A producers means everything except the 16 instructions just issued
                const bool issued = more && OZ2_HOOK_DMA_ON(vb == (int)blockIdx.x);
                if (issued) PRODUCER_BEGIN();
#pragma unroll
                for (int sl = 0; sl < 8; ++sl) {
                    // B (needed next K-step): 4 instructions in each of slots 0-3; A (needed in two K-steps): 2 in every slot.
                    // Bursts cost: all 16 in slot 0 is 7 % slower than the spread issue.
                    if (issued) {
                        if (isB) {
                            constexpr int PB = OZ2_PB;  // slots over which B's 16 instructions are spread
#pragma unroll
                            for (int q = 0; q < 16; ++q)
                                if (q * PB / 16 == sl) PRODUCER_DMA(fsrc, q, fdst);
                        } else {
#pragma unroll
                            for (int q = 0; q < 2; ++q) PRODUCER_DMA(fsrc, sl * 2 + q, fdst);
                        }
                    }
                    if (sl == 7 && issued) PRODUCER_ADVANCE();
                    if (sl == 7) {
                        if (!isB && issued) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
                        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    }
                    __builtin_amdgcn_s_barrier();
                }
            }
        }
        __builtin_amdgcn_s_barrier();
        }
#include "oz2_gemm_i8_producer_undef.inc"
        return;
    }

    // ------------------------------ consumer waves
    // Matrix instruction: v_mfma_i32_16x16x64_i8 (A / B operand: lane l = row l & 15, K bytes 16 (l >> 4) .. + 15 of a 64-byte K
    // slice; result: column l & 15, rows 4 (l >> 4) + r).  At the board's power cap it sustains 3.95-3.98 POP/s on uniformly
    // distributed residues where v_mfma_i32_32x32x32_i8 holds 3.45 (tools/ubench/mfma_shapes.hip, profiles/archive/r02_mfma_shapes.txt):
    // the same MACs with a quarter of the accumulator registers read and written per instruction.  Wave tile 128 x 64 = 8 x 4
    // accumulator tiles (128 registers); a K-step (128 bytes) is four segments (K half ks2) x (row half ah) of 16 MFMAs: the B
    // fragments of a K half are loaded in its first segment and kept for the second, the A fragments of 64 rows per segment.
    const int wm = wave >> 2, wn = wave & 3;
    const int r16 = lane & 15;
    const int q = lane >> 4;
    const int sw = (r16 >> 1) & 7;
    const int a_base = (wm * 128 + r16) * BK;
    const int b_base = (wn * 64 + r16) * BK;

    if constexpr (KBAR) {
    // K-step-barrier schedule: ONE workgroup barrier per K-step -- the only one the LDS ring needs (RAW: the producers' vmcnt wait for
    // panel g + 1 precedes it; WAR: every read of K-step g precedes it, every refill of those slots follows it).  The two waves of a
    // SIMD stay in anti-phase by construction instead of by per-segment barriers: the wm = 0 half runs L0 M0 L1 M1 L2 M2 L3 M3 inside
    // a K-step, the wm = 1 half M3' L0 M0 L1 M1 L2 M2 L3 (M3' = the last MFMA segment of the PREVIOUS K-step, whose fragments it
    // keeps in registers across the barrier), so one wave's LDS reads always sit beside the other's MFMAs, and when both have MFMAs
    // ready they simply share the pipe.  The per-segment barriers of the ping-pong version cost ~7 % (every hand-over idles the
    // matrix pipe for the barrier latency: mfma-only probe 3.70 vs 3.97 POP/s free-running).
    __builtin_amdgcn_s_barrier();  // K-tile 0 published by the producers
    // the whole persistent loop is instantiated once per half (WM1 = lagging half) so that each gets its own register allocation
    auto run = [&]<bool WM1>() {
        int sA = 0;  // slot of A(g); B(g) sits in the next slot (mod 5)
        // MFMA_REINIT: the accumulators live across the tile loop; the v_mov initialisation runs once, every later tile finds them rewritten by
        // the matrix pipe behind the previous epilogue (MfmaReinitHook)
        constexpr bool MFMA_REINIT = SMALLK && EPI == EPI_MOD && FUSE == 0;  // SMALLK only: with a register C operand (start value -2^31) the form measured -0.6 ... -1.6 % at k = 1024 / 2048 (profiles/r06_short_k_epilogue_ab.txt)
        v4i acc[8][4];
        if constexpr (MFMA_REINIT) {
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = v4i{args.acc0, args.acc0, args.acc0, args.acc0};
        }
        for (int vb = blockIdx.x; vb < total; vb += G) {
            const TileMap tmap = OZ2_I8_MAP_TILE(vb);
            const PlaneRef pref = (FUSE || EPI == EPI_MAX) ? PlaneRef{0, 0} : plane_ref(args, tmap.plane);  // (the bound GEMM looks its plane up at the epilogue: one value less across its K loop)
            const PlaneConsts pcon = (FUSE || EPI == EPI_MAX) ? PlaneConsts{} : plane_consts(args, pref);  // fetched here: the latency passes behind the K loop
            for (int pl = 0; pl < planes_per_tile; ++pl) {
            v4i af[4], bf[4];
            // (Peeling the first K-step of short-K launches, its MFMAs taking the inline constant 0 as their C operand instead of the 128 v_mov_b32 per wave and
            // tile, was tried in rounds 4 and 6: the compiler then moves seven accumulator quads through scratch INSIDE the peeled K-step, 140 bytes.  Withdrawn.)
            if constexpr (!MFMA_REINIT) {
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[i][j] = v4i{EPI == EPI_MAX ? 0 : args.acc0, EPI == EPI_MAX ? 0 : args.acc0, EPI == EPI_MAX ? 0 : args.acc0, EPI == EPI_MAX ? 0 : args.acc0};
            }
// The fragment reads of a segment are issued in the order the MFMAs use them (pinned: the scheduler otherwise issues the first-used fragment last) and the
// waits in front of the MFMAs are the compiler's own per-fragment lgkmcnt(3..0): the first four MFMAs of a segment start when THEIR fragment has landed.  No
// barrier covers the read latency in this schedule (in the ping-pong schedule one does: there the same change is neutral).  8192^2 x 14 planes, interleaved,
// 25 rounds: k = 256 / 512 / 1024: +0.4 / +0.8 / +1.5 %, neutral from 2048 (profiles/r04f_kbar_partial_wait_ab.txt)
#define OZ2_KBAR_PIN() __builtin_amdgcn_sched_barrier(0)
#define OZ2_KBAR_WAIT() do {} while (0)
#define OZ2_LOAD_SEG(seg_)                                                                                                   \
    do {                                                                                                                     \
        const int coff_ = (((((seg_) >> 1) << 2) | q) ^ sw) << 4;                                                            \
        if (((seg_) & 1) == 0) {                                                                                             \
            _Pragma("unroll") for (int j = 0; j < 4; ++j) bf[j] = *(const v4i*)(curB + j * 16 * BK + coff_);                 \
        }                                                                                                                    \
        _Pragma("unroll") for (int i = 0; i < 4; ++i) { af[i] = *(const v4i*)(curA + (((seg_) & 1) * 4 + i) * 16 * BK + coff_); OZ2_KBAR_PIN(); } \
    } while (0)
#define OZ2_MMA_SEG(seg_)                                                                                            \
    do {                                                                                                                     \
        OZ2_KBAR_WAIT();                                                                   \
        __builtin_amdgcn_sched_barrier(0);                                                                                   \
        __builtin_amdgcn_s_setprio(1);                                                                                       \
        _Pragma("unroll") for (int i = 0; i < 4; ++i) _Pragma("unroll") for (int jj = 0; jj < 4; ++jj) {                     \
            const int j = (i & 1) ? 3 - jj : jj; /* serpentine: see the ping-pong branch */                                   \
            acc[((seg_) & 1) * 4 + i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(af[i], bf[j], acc[((seg_) & 1) * 4 + i][j], 0, 0, 0); \
        }                                                                                                                    \
        __builtin_amdgcn_s_setprio(0);                                                                                       \
        __builtin_amdgcn_sched_barrier(0);                                                                                   \
    } while (0)
#define OZ2_SET_PANELS()                                                                                                     \
    const char* curA = smem + sA * TILE_BYTES + a_base;                                                                      \
    const char* curB = smem + (sA == 4 ? 0 : sA + 1) * TILE_BYTES + b_base;                                                  \
    sA = sA + 2 >= 5 ? sA - 3 : sA + 2
            // EPI_MAX with kt_mid: two phases per tile (K-steps [0, kt_mid) and [kt_mid, KT)), the maxima epilogue after each; the
            // accumulators run through.  Every other instantiation: one phase.
            int kt = 0;
            const int nph = (EPI == EPI_MAX && args.kt_mid > 0) ? 2 : 1;
            for (int ph = 0; ph < nph; ++ph) {
            const int kt_end = (EPI == EPI_MAX && ph + 1 < nph) ? args.kt_mid : OZ2_I8_KSTEPS(tmap);
            auto kstep = [&]() {
                OZ2_SET_PANELS();
#pragma unroll
                for (int seg = 0; seg < 4; ++seg) {
                    OZ2_LOAD_SEG(seg);
                    // the lagging half crosses the K-step barrier between its last LOAD and its last MFMA segment (all its LDS reads of the
                    // K-step precede the barrier; the fragments cross it in registers): same instruction stream, shifted by one segment
                    if (WM1 && seg == 3) {
                        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                        __builtin_amdgcn_sched_barrier(0);
                        __builtin_amdgcn_s_barrier();
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    OZ2_MMA_SEG(seg);
                }
                if (!WM1) {
                    __builtin_amdgcn_s_barrier();
                    __builtin_amdgcn_sched_barrier(0);
                }
            };
            for (; kt < kt_end; ++kt) kstep();
#undef OZ2_SET_PANELS
#undef OZ2_LOAD_SEG
#undef OZ2_MMA_SEG
#undef OZ2_KBAR_PIN
#undef OZ2_KBAR_WAIT
#if OZ2_HOOK_SKIP_EPILOGUE
            (void)tmap;  // laboratory probe: no epilogue; the accumulators stay live
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) asm volatile("" ::"v"(acc[i][j]));
#else
            int lane_e = lane;
            if constexpr (EPI == EPI_MOD) {  // (the complex combine keeps the live lane id: recomputed there, 116 bytes of accumulator spills appear in its K loop)
            // The lane id of the epilogue is RECOMPUTED here (two v_mbcnt behind an opaque asm, so that it is not hoisted): kept live across the K loop it was
            // spilled (12 bytes of scratch), and the reload's vmcnt(0) made every tile wait for the PREVIOUS tile's residue stores to be acknowledged --
            // free behind a long K loop, a stall of the order of the store latency at k <= 1024 where the K loop is 2-8 us (round 6).  The consumer waves
            // issue no other VMEM loads, so no vmcnt wait is left on their path at all.
            asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane_e));
            } else {
                __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
            }
            if constexpr (FUSE != 0) i8_epilogue<EPI, NoHook, -1>(acc, args, PlaneRef{0, pl}, tmap.tm * BM + (WM1 ? 128 : 0), tmap.tn * BN + wn * 64, lane_e);
            else if constexpr (EPI == EPI_MAX) i8_epilogue<EPI, NoHook, 0>(acc, args, plane_ref(args, tmap.plane), PlaneConsts{}, tmap.tm * BM + (WM1 ? 128 : 0), tmap.tn * BN + wn * 64, lane_e);
            else if constexpr (MFMA_REINIT) i8_epilogue<EPI, MfmaReinitHook<true>, (int)SMALLK>(acc, args, pref, pcon, tmap.tm * BM + (WM1 ? 128 : 0), tmap.tn * BN + wn * 64, lane_e, MfmaReinitHook<true>{acc, args.acc0});
            else i8_epilogue<EPI, NoHook, (int)SMALLK>(acc, args, pref, pcon, tmap.tm * BM + (WM1 ? 128 : 0), tmap.tn * BN + wn * 64, lane_e);
#endif
            }  // phase
            }
            // FUSE: the producer waves accumulate the CRT of this tile during the next one; they read the residue planes one K-step
            // after the barrier that follows this wait
            if constexpr (FUSE != 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        if constexpr (FUSE != 0) __builtin_amdgcn_s_barrier();  // the last tile's residues are complete: the producers drain
    };
    if (wm == 0) run.template operator()<false>();
    else run.template operator()<true>();
    } else {
    __builtin_amdgcn_s_barrier();               // K-tile 0 published by the producers
    if (wm == 1) __builtin_amdgcn_s_barrier();  // trailing half: one segment behind
    int sA = 0;                                  // slot of A(g); B(g) sits in the next slot (mod 5)
#if OZ2_I8_SBS
    // Epilogues side by side.  With G the barrier behind the leading half's last MFMA segment of a tile, that half reduces and stores between G and G + 1;
    // the lagging half has its last 16 MFMAs there and, in gemm_i8_kernel, arrives at G + 1 right behind them, so that ITS epilogue runs between G + 1
    // and G + 2 -- beside 16 MFMAs of the leading half, which then waits at G + 2: the two epilogues are serialised and both are exposed.  Here the
    // lagging half arrives at G + 1 only behind its epilogue and the next tile's accumulator initialisation: both halves reduce and store between the same
    // two barriers, and from G + 1 on the anti-phase is the old one.  Every wave executes the same barriers as before, one of them later: the epilogue
    // touches no LDS, the half's reads of the tile's last K-step are complete before its last MFMAs (the ring's WAR rule holds as it is), and the
    // producers only wait longer at G + 1, the next tile's first panels already in flight.  tests/test_gemm_sbs_barrier_model.py replays both orders.
    static_assert(EPI == EPI_MOD && !KBAR && FUSE == 0 && !SMALLK && !OZ2_I8_KR, "side-by-side epilogues: the residue launch of the ping-pong schedule, one phase per tile");
#endif
    for (int vb = blockIdx.x; vb < total; vb += G) {
        const TileMap tmap = OZ2_I8_MAP_TILE(vb);
        const PlaneRef pref = (FUSE || EPI == EPI_MAX) ? PlaneRef{0, 0} : plane_ref(args, tmap.plane);  // (the bound GEMM looks its plane up at the epilogue: one value less across its K loop)
        const PlaneConsts pcon = (FUSE || EPI == EPI_MAX) ? PlaneConsts{} : plane_consts(args, pref);  // fetched here: the latency passes behind the K loop
        for (int pl = 0; pl < planes_per_tile; ++pl) {
        v4i acc[8][4];
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                acc[i][j] = v4i{EPI == EPI_MAX ? 0 : args.acc0, EPI == EPI_MAX ? 0 : args.acc0, EPI == EPI_MAX ? 0 : args.acc0, EPI == EPI_MAX ? 0 : args.acc0};
#if OZ2_I8_SBS
        if (wm == 1 && vb != (int)blockIdx.x) {  // the previous tile's last barrier: behind its epilogue and this initialisation
#pragma unroll
            for (int i = 0; i < 8; ++i)  // (opaque uses: the v_mov_b32 are not sunk behind the barrier)
#pragma unroll
                for (int j = 0; j < 4; ++j) asm volatile("" : "+v"(acc[i][j]));
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_sched_barrier(0);
        }
#endif

        int kt = 0;  // phases: see the K-step-barrier branch
        const int nph = (EPI == EPI_MAX && args.kt_mid > 0) ? 2 : 1;
        for (int ph = 0; ph < nph; ++ph) {
        const int kt_end = (EPI == EPI_MAX && ph + 1 < nph) ? args.kt_mid : OZ2_I8_KSTEPS(tmap);
#define OZ2_I8_PP_DEFER 0
#if OZ2_I8_SBS
        for (; kt < kt_end - wm; ++kt) {  // the lagging half's last K-step of the tile is peeled: a tile has K-steps (kp >= 256)
#else
        for (; kt < kt_end; ++kt) {
#endif
#include "oz2_gemm_i8_pp_kstep.inc"
        }
#undef OZ2_I8_PP_DEFER
#if OZ2_I8_SBS
        if (wm == 1) {  // ... without the barrier behind its last MFMA segment
#define OZ2_I8_PP_DEFER 1
#include "oz2_gemm_i8_pp_kstep.inc"
#undef OZ2_I8_PP_DEFER
        }
#endif
#if OZ2_HOOK_SKIP_EPILOGUE
        (void)tmap;  // laboratory probe: no epilogue; the accumulators stay live
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) asm volatile("" ::"v"(acc[i][j]));
#else
        // every reload still pending on some path is waited for HERE (the previous tile's stores retired a whole K loop ago: free), so that the waitcnt
        // pass has no reason to put a vmcnt wait into the K loop (it did, in the K-step-barrier kernels until round 4 and in the bound GEMM after a
        // register-allocation change: tests/test_kernel_resources.py)
#if OZ2_HOOK_SKIP_EPILOGUE_HALF
        if ((OZ2_HOOK_SKIP_EPILOGUE_HALF >> wm) & 1) {  // laboratory probe: no epilogue on this half
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) asm volatile("" ::"v"(acc[i][j]));
        } else
#endif
        {
        __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
#if OZ2_I8_SBS
        // the epilogue's lane id is recomputed behind an opaque asm, as in the K-step-barrier branch: with the peeled K-step a lane-derived value of the
        // epilogue was otherwise kept in scratch across the K loop (8 bytes)
        int lane_e;
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane_e));
        i8_epilogue<EPI, NoHook, (int)SMALLK>(acc, args, pref, pcon, tmap.tm * BM + wm * 128, tmap.tn * BN + wn * 64, lane_e);
#else
        if constexpr (FUSE != 0) i8_epilogue<EPI, NoHook, -1>(acc, args, PlaneRef{0, pl}, tmap.tm * BM + wm * 128, tmap.tn * BN + wn * 64, lane);
        else if constexpr (EPI == EPI_MAX) i8_epilogue<EPI, NoHook, 0>(acc, args, plane_ref(args, tmap.plane), PlaneConsts{}, tmap.tm * BM + wm * 128, tmap.tn * BN + wn * 64, lane);
        else i8_epilogue<EPI, NoHook, (int)SMALLK>(acc, args, pref, pcon, tmap.tm * BM + wm * 128, tmap.tn * BN + wn * 64, lane);
#endif
        }
#endif
        }  // phase
        }
#ifdef OZ2_LAB_FUSED_CRT
        if constexpr (FUSE != 0) i8_crt_tail<std::conditional_t<FUSE == 2, float, double>>(args, tmap.tm * BM + wm * 128, tmap.tn * BN + wn * 64, lane);
#endif
    }
#if OZ2_I8_SBS
    if (wm == 1 && (int)blockIdx.x < total) __builtin_amdgcn_s_barrier();  // the last tile's last barrier
#endif
    if (wm == 0) __builtin_amdgcn_s_barrier();
    }
}
#undef OZ2_I8_MAP_TILE
#undef OZ2_I8_KSTEPS
