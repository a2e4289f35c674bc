// Prologue of the producer (LDS-DMA) waves of gemm_i8_kernel, shared by the kernel body and by the out-of-line CRT producer
// (i8_producer_crt): included inside a function that provides args, smem, lane, wave, KT1, total, G, planes_per_tile and FUSE.
// Defines the PRODUCER_* macros (undefined again by oz2_gemm_i8_producer_undef.inc).
        // Wave pw issues DMA instructions Q = 16 pw .. 16 pw + 15 of every K-tile (1 KiB = 8 rows x 128 B each; 4096 16-byte
        // LDS slots per stage: slot s <-> operand (s >= 2048: B), row (s & 2047) >> 3, physical chunk s & 7 holding logical
        // chunk (s & 7) ^ ((row >> 1) & 7)), i.e. waves 0,1 fetch A and waves 2,3 fetch B.  Per tile: a wave-uniform base
        // pointer per K segment and 16 per-lane byte offsets (row * kp + chunk, B rows clamped to the rows that exist), so
        // the K loop issues global_load_lds with SGPR base + VGPR offset and no address arithmetic.
        const int pw = wave - 8;
        const bool isB = pw >= 2;
        unsigned doff[16];
        const int8_t *g0, *g1, *g2;
        auto uniform = [](const int8_t* ptr) {
            const unsigned long long v = (unsigned long long)ptr;
            const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
            return (const int8_t*)(((unsigned long long)hi << 32) | lo);
        };
#ifndef OZ2_PRODUCER_MAP_TILE  // (the laboratory kernel that reads its arguments from the kernel-argument address space keeps the division form)
#define OZ2_PRODUCER_MAP_TILE(vb_) map_tile<EPI != EPI_MAX>((vb_), total, args.map)
#endif
// Hooks of the K-ranged kernel (gemm_i8_kr_kernel defines them, oz2_gemm_i8_kernel.inc): the range [kfirst, kend) of the tile whose panels are fetched next
// is taken where the tile is set, kin enters a tile at kfirst and PRODUCER_ADVANCE leaves it at kend.  Empty everywhere else: a tile runs [0, KT1).
#ifndef OZ2_PRODUCER_KEND
#define OZ2_PRODUCER_KR_DECL() do {} while (0)
#define OZ2_PRODUCER_KR_SET(tmap_) do {} while (0)
#define OZ2_PRODUCER_KR_ENTER() do {} while (0)
#define OZ2_PRODUCER_KEND KT1
#endif
#define PRODUCER_SET_TILE(vb_)                                                                                               \
    do {                                                                                                                     \
        const TileMap tmap_ = OZ2_PRODUCER_MAP_TILE(vb_);                                                      \
        const PlaneRef pr_ = plane_ref(args, tmap_.plane);                                                                   \
        const size_t off_ = pr_.boff + (isB ? (size_t)pr_.tt * args.strideB + (size_t)tmap_.tn * BN * args.kp                \
                                            : (size_t)pr_.tt * args.strideA + (size_t)tmap_.tm * BM * args.kp);              \
        g0 = uniform((isB ? args.B[0] : args.A[0]) + off_);                                                                  \
        g1 = uniform((isB ? args.B[1] : args.A[1]) + off_);                                                                  \
        g2 = uniform((isB ? args.B[2] : args.A[2]) + off_);                                                                  \
        const int nvalid_ = isB ? ((args.n - tmap_.tn * BN) < BN ? (args.n - tmap_.tn * BN) : BN) : BM;                       \
        _Pragma("unroll") for (int q = 0; q < 16; ++q) {                                                                     \
            const int pp_ = (((pw & 1) * 16 + q) * 64 + lane);                                                               \
            int row_ = pp_ >> 3;                                                                                             \
            const int c_ = (pp_ & 7) ^ ((row_ >> 1) & 7);                                                                    \
            row_ = row_ < nvalid_ ? row_ : nvalid_ - 1;                                                                      \
            doff[q] = (unsigned)row_ * (unsigned)args.kp + c_ * 16;                                                          \
        }                                                                                                                    \
        OZ2_PRODUCER_KR_SET(tmap_);                                                                                          \
    } while (0)
#define PRODUCER_DMA(src_, q_, stage_)                                                                                       \
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)((src_) + doff[q_]),                     \
                                     (__attribute__((address_space(3))) void*)((stage_) + (pw * 16 + (q_)) * 1024), 16, 0, 0)  /* cache-policy bits of the LDS-DMA: sc0 / sc1 measured neutral, nt 10 % slower */

        // 2.5-stage ring of operand panels (5 x 32 KiB = all 160 KiB of LDS): panel h = 2 g + isB lives in slot h % 5.  The slot of
        // A(g') held B(g'-3) and the slot of B(g') held A(g'-2), so during K-step g the A producers may fetch A(g+2) and the B
        // producers B(g+1): 96 KiB in flight per CU instead of 64 -- the 2-stage version was bound by the DMA round trip
        // (64 KiB per ~1.5 us of L2-miss latency = 43 GB/s per CU against the 60 GB/s a full-speed K-step consumes).
        int vb_next = blockIdx.x;  // tile of the panel to fetch next
        int pl_next = 0;           // FUSE: its residue plane
        bool more = true;
        OZ2_PRODUCER_KR_DECL();
        PRODUCER_SET_TILE(vb_next);
        int seg = 0, kin = 0;      // its segment / K-step inside the segment (no divisions in the loop)
        OZ2_PRODUCER_KR_ENTER();
        int hs = isB ? 1 : 0;      // its slot
#define PRODUCER_BEGIN()                                                                                                     \
    do {                                                                                                                     \
        fsrc = (seg == 0 ? g0 : seg == 1 ? g1 : g2) + (size_t)OZ2_HOOK_KSTEP(kin) * BK;                                      \
        fdst = smem + hs * TILE_BYTES - (isB ? TILE_BYTES : 0);   /* PRODUCER_DMA adds pw * 16 KiB */                         \
    } while (0)
#define PRODUCER_ADVANCE()                                                                                                   \
    do {                                                                                                                     \
        hs = hs + 2 >= 5 ? hs - 3 : hs + 2;                                                                                  \
        if (++kin == OZ2_PRODUCER_KEND) {                                                                                    \
            kin = 0;                                                                                                         \
            if (++seg == args.nseg) {                                                                                        \
                seg = 0;                                                                                                     \
                if (FUSE && ++pl_next < planes_per_tile) { /* same tile, next residue plane: the lane offsets stay */        \
                    const size_t st_ = isB ? args.strideB : args.strideA;                                                    \
                    g0 = uniform(g0 + st_), g1 = uniform(g1 + st_), g2 = uniform(g2 + st_);                                  \
                } else {                                                                                                     \
                    pl_next = 0;                                                                                             \
                    vb_next += G;                                                                                            \
                    more = vb_next < total;                                                                                  \
                    if (more) PRODUCER_SET_TILE(vb_next);                                                                    \
                    OZ2_PRODUCER_KR_ENTER();                                                                                 \
                }                                                                                                            \
            }                                                                                                                \
        }                                                                                                                    \
    } while (0)
#define PRODUCER_FETCH()                                                                                                     \
    do {                                                                                                                     \
        PRODUCER_BEGIN();                                                                                                    \
        _Pragma("unroll") for (int q = 0; q < 16; ++q) PRODUCER_DMA(fsrc, q, fdst);                                          \
        PRODUCER_ADVANCE();                                                                                                  \
    } while (0)
        const int8_t* fsrc = g0;
        char* fdst = smem;
        PRODUCER_FETCH();  // panel 0
        bool ahead = false;
        if (!isB && more) {
            PRODUCER_FETCH();  // A(1)
            ahead = true;
        }
        if (ahead) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
