// One K-step of a consumer wave in the ping-pong schedule: the body of the K loop of oz2_gemm_i8_kernel.inc (which provides smem, sA, a_base, b_base, q, sw, acc).
// A file of its own because gemm_i8_sbs_kernel runs it twice: inside the K loop, and once more with OZ2_I8_PP_DEFER 1 as the lagging half's LAST K-step
// of a tile, which leaves out the barrier behind its last MFMA segment (the half takes it behind the epilogue) -- peeled, so that the K loop itself carries
// no test for it: a scalar compare and branch in front of every K-step's last barrier, on the hand-over path, measured 1.3 % of the launch at k = 8192
// (profiles/r10_sbs_epilogue_ab.txt).  Every other kernel includes it once with OZ2_I8_PP_DEFER 0: the text it always compiled.
            const char* curA = smem + sA * TILE_BYTES + a_base;
            const char* curB = smem + (sA == 4 ? 0 : sA + 1) * TILE_BYTES + b_base;
            sA = sA + 2 >= 5 ? sA - 3 : sA + 2;
#pragma unroll
            for (int ks2 = 0; ks2 < 2; ++ks2) {
                const int coff = (((ks2 << 2) | q) ^ sw) << 4;
                v4i bf[4];
#pragma unroll
                for (int ah = 0; ah < 2; ++ah) {
                    v4i af[4];
                    if (ah == 0) {
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            bf[j] = *(const v4i*)(curB + j * 16 * BK + coff);
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        af[i] = *(const v4i*)(curA + (ah * 4 + i) * 16 * BK + coff);
                    // Only the K-step's LAST load segment completes its reads BEFORE the barrier: that is the barrier the ring's WAR rule counts on
                    // (LDS operations of a wave complete in order, so its wait covers every read of the K-step).  The other three segments arrive at
                    // the barrier as soon as their reads are ISSUED and wait behind it: a wave's LDS latency no longer delays the hand-over of all
                    // twelve (+0.4 / +0.5 % at k = 6144 / 8192, planes bit-identical: profiles/archive/r04e_late_wait_ab.txt)
                    if (ks2 == 1 && ah == 1) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    __builtin_amdgcn_sched_barrier(0);
                    __builtin_amdgcn_s_barrier();
                    __builtin_amdgcn_sched_barrier(0);
                    if (!(ks2 == 1 && ah == 1)) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    __builtin_amdgcn_sched_barrier(0);
                    __builtin_amdgcn_s_setprio(1);
                    // serpentine order over the 4 x 4 fragment pairs: consecutive MFMAs share an operand register also across the row change
                    // (B fragment 3, 3, 0, 0 ...): +0.5 ... 0.65 % at k >= 8192, interleaved (profiles/archive/r04_gemm_ab_serpentine_kbar.txt)
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int jj = 0; jj < 4; ++jj) {
                            const int j = (i & 1) ? 3 - jj : jj;
                            acc[ah * 4 + i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(af[i], bf[j], acc[ah * 4 + i][j], 0, 0, 0);
                        }
                    __builtin_amdgcn_s_setprio(0);
                    __builtin_amdgcn_sched_barrier(0);
#if OZ2_I8_PP_DEFER
                    if (!(ks2 == 1 && ah == 1))  // (the lagging half's last barrier of the tile: behind its epilogue)
#endif
                    __builtin_amdgcn_s_barrier();
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
