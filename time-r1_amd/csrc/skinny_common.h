// What the decode-row ("skinny", M <= 64) GEMM kernels share: the bf16 family (gemm_skinny.hip) and its fp8 twin (gemm_w8.hip).
// Device side: the output-tile index, the wave's K slice, the x-into-LDS copy of the register-fragment kernels, the rmsnorm / SwiGLU fragment helpers and the
// cross-block split-K fixup.  Host side: which K have an LDS-streamed form and how much dynamic LDS those forms take.  The k-loops stay in the kernels.
#pragma once
#include "tr1_common.h"

// cache policy bits of the weight-stream DMA loads of the decode kernels (0 = default, 2 = nt: read-once weights leave L2 first)
#ifndef TR1_W_AUX
#define TR1_W_AUX 2
#endif

// Launch of the single-pass decode-regime kernel (gemm_skinny.hip); tr1_gemm_nt_bf16 (gemm.hip) routes M <= 64 here.
void launch_skinny(const void* A, const void* B, void* C, const void* bias, const void* residual, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb,
                   int64_t ldc, int64_t ldr, int out_f32, int ksplit, hipStream_t s);

TR1_DEV float silu_f32(float x) { return x / (1.f + __expf(-x)); }
// x' = bf16(x * w) of one MFMA fragment (the rmsnorm weight folded into the operand) while ss accumulates sum x^2
TR1_DEV bf16x8_t scale_frag_sumsq(bf16x8_t x, bf16x8_t w, float& ss) {
    const u32x4_t xu = __builtin_bit_cast(u32x4_t, x), wu = __builtin_bit_cast(u32x4_t, w);
    u32x4_t o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float a = bflo(xu[e]), b = bfhi(xu[e]);
        ss = fmaf(a, a, fmaf(b, b, ss));
        o[e] = pack2bf(a * bflo(wu[e]), b * bfhi(wu[e]));
    }
    return __builtin_bit_cast(bf16x8_t, o);
}

// Element i of a block's output tile [column group c][row group mg][16 rows mm][16 columns nn] (MG row groups): the order of the reduction buffers, of the
// parked split-K tiles and of the epilogue loops.
// Declares c, mg, mm, nn; the row of x / of the output is mg * 16 + mm.  (A macro: as an inlined helper or a returned struct the same four expressions came out
// of hipcc with two to three more VGPRs in the MG = 2 rmsnorm kernels of both families; -Rpass-analysis=kernel-resource-usage before changing its form.)
#define SKINNY_TILE_IDX(MG_, i_) const int c = (i_) / ((MG_) * 256), mg = ((i_) >> 8) % (MG_), mm = ((i_) >> 4) & 15, nn = (i_) & 15

// In-block split-K: wave `wave` of WAVES takes the k-steps [s0, s1) of the block's nsteps, counted from the block's first (an empty range where there are
// more waves than steps).
template <int WAVES>
TR1_DEV void skinny_wave_kslice(int64_t nsteps, int wave, int64_t& s0, int64_t& s1) {
    const int64_t s_per = (nsteps + WAVES - 1) / WAVES;
    s0 = wave * s_per;
    s1 = s0 + s_per; if (s1 > nsteps) s1 = nsteps;
}

// XLDS forms of the register-fragment bf16 kernels: the block copies its 16 activation rows ONCE into LDS by DMA, image [K/64 segments][16 rows][128 bytes]
// with chunk c of row r at c ^ keyA(r) (applied on the source address), 1 KiB (8 rows) per instruction, the instructions dealt round-robin to the waves.
// Issued from inline asm (tr1_dma16): after the builtin hipcc would put vmcnt(0) in front of every LDS read, draining the weight stream.  The callers' counted
// s_waitcnt vmcnt(8) / vmcnt(12) rely on these being the OLDEST vector-memory operations of the wave: call it before the first weight load.
// (A macro over the kernel's X, M, K, ldx, xs_base, lane, wave: as an inlined function hipcc rotated the loop and reordered the prologue around it.)
#define SKINNY_X_TO_LDS(WAVES_)                                                                                                         \
    do {                                                                                                                                \
        const int r8 = lane >> 3;                                                                                                       \
        const int n_inst = (int)(K >> 5);                                     /* 1 KiB per instruction */                               \
        for (int i = __builtin_amdgcn_readfirstlane(wave); i < n_inst; i += (WAVES_)) {                                                 \
            const int r = (i & 1) * 8 + r8;                                                                                             \
            const unsigned off = (unsigned)((r < M ? r : M - 1) * (int)ldx + (i >> 1) * 64 + (((lane & 7) ^ keyA(r)) << 3)) * 2u;       \
            const unsigned dst = xs_base + (unsigned)i * 1024u;                                                                         \
            tr1_dma16(off, X, dst);                                                                                                     \
        }                                                                                                                               \
    } while (0)

// ---- cross-block split-K with in-kernel fixup ---------------------------------------------------------------------------------------------------------------
// Block (x, y) of a (column groups, K slabs) grid has its waves' fp32 partial tiles in LDS (TILE_ floats per wave, THREADS_ threads, MG_ row groups; RED_ = the
// element (c, mg, mm, nn) of wave w).  Every block sums its waves in wave order, parks the tile in L2-resident scratch and takes a ticket; the block that draws the last
// ticket of its column group sums the gridDim.y tiles in SLAB ORDER - deterministic, whichever block arrives last - runs STORE_ on each sum (the kernel's own
// epilogue: a statement over i, c, mg, mm, nn and the float v - bias, residual, row scale, bounds, output type) and re-arms the counter for the next launch (ordered by
// the kernel boundary).  Every other block runs NOT_LAST_ (a return).
//   * The tiles are written and read with device-scope (write-through / L2-bypassing) accesses, so they are visible across XCDs (per-XCD L2) without flushing
//     the caches: s_waitcnt vmcnt(0) means the stores are acknowledged at device scope before the ticket is drawn.  A full agent-scope fence there would write
//     back and invalidate the whole L2 and evict x for every other block (measured: 38 -> 55 us on the 7B down projection).
//   * The last block keeps every slab load in flight before the first add (4 slabs, the usual case: ((t0 + t1) + t2) + t3; up to 16: the same left-to-right
//     sum).  As a rolled loop each device-scope load waited for the one before it: 8 300 cycles for the last-arriving block (block timeline in DESIGN.md).
//   * PARKED_ / TICKETED_: statements after the tile is parked / after the ticket is drawn (block-timeline stamps; empty otherwise).
// UPTO16_: the launcher may split K 5 .. 16 ways (bf16: skinny_fix_cfg); false compiles the in-flight 16-slab form out (fp8: always 4 slabs).
// fix_ws: [gridDim.y][gridDim.x][TILE_] floats; fix_cnt: one counter per column group, zero before the first launch; TICKET_: an int lvalue in LDS.
// A macro, and with the rolled loop for more than 16 slabs that no launcher can reach (skinny_fix_cfg caps the split at 16, the fp8 form fixes 4): as an inlined
// helper with callables, and equally with that loop deleted from the kernels' own text, hipcc allocated the bf16 fixup kernels differently (VGPRs +-1 to +4, other SGPR
// spill counts).  This text compiles to the register, spill, LDS and occupancy figures the kernels had with their own copies.
#define SKINNY_SPLITK_FIXUP(TILE_, THREADS_, MG_, UPTO16_, RED_, TICKET_, PARKED_, TICKETED_, NOT_LAST_, STORE_) \
    do { \
        float* mine__ = fix_ws + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * (TILE_); \
        for (int i = threadIdx.x; i < (TILE_); i += (THREADS_)) { \
            SKINNY_TILE_IDX(MG_, i); \
            float v = 0.f; \
            _Pragma("unroll") for (int w = 0; w < (THREADS_) / 64; ++w) v += RED_; \
            __hip_atomic_store(mine__ + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); \
        } \
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); \
        __syncthreads(); \
        PARKED_; \
        if (threadIdx.x == 0) TICKET_ = __hip_atomic_fetch_add(&fix_cnt[blockIdx.x], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); \
        __syncthreads(); \
        TICKETED_; \
        if (TICKET_ != (int)gridDim.y - 1) { NOT_LAST_; } \
        for (int i = threadIdx.x; i < (TILE_); i += (THREADS_)) { \
            SKINNY_TILE_IDX(MG_, i); \
            float v = 0.f; \
            if (gridDim.y == 4) { \
                float t[4]; \
                _Pragma("unroll") for (int ks = 0; ks < 4; ++ks) \
                    t[ks] = __hip_atomic_load(fix_ws + ((int64_t)ks * gridDim.x + blockIdx.x) * (TILE_) + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); \
                v = ((t[0] + t[1]) + t[2]) + t[3]; \
            } else if ((UPTO16_) && gridDim.y <= 16) { \
                float t[16]; \
                _Pragma("unroll") for (int ks = 0; ks < 16; ++ks) \
                    t[ks] = ks < (int)gridDim.y ? __hip_atomic_load(fix_ws + ((int64_t)ks * gridDim.x + blockIdx.x) * (TILE_) + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.f; \
                v = t[0]; \
                _Pragma("unroll") for (int ks = 1; ks < 16; ++ks) if (ks < (int)gridDim.y) v += t[ks]; \
            } else { \
                for (int ks = 0; ks < (int)gridDim.y; ++ks) \
                    v += __hip_atomic_load(fix_ws + ((int64_t)ks * gridDim.x + blockIdx.x) * (TILE_) + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); \
            } \
            STORE_; \
        } \
        if (threadIdx.x == 0) fix_cnt[blockIdx.x] = 0; \
    } while (0)

// ---- launch side: the LDS-streamed forms ----------------------------------------------------------------------------------------------------------------------
// norm_glu_lds_kernel / norm_glu_lds_f8_kernel give each wave a 512-wide K slice: they exist for K = 512 * NST, NST = 7 / 4 / 3 (hidden 3584 / 2048 / 1536).
inline bool skinny_lds_stream_k(int64_t K) { return K % 512 == 0 && (K / 512 == 7 || K / 512 == 4 || K / 512 == 3); }
// Dynamic LDS of norm_glu_lds_kernel<NST, ring, nred, mg>: the 8 waves' rings of 4 KiB stages + nred reduction buffers of 8 x mg x (gate | up) 16 x 17 floats +
// the sums of squares + the waves' norm-weight KiB (+ one 2 KiB x stage per wave where the x staging leaves ring slot 0 to the first weight stage: XSLOT0).
constexpr size_t norm_glu_lds_bytes(int ring, int nred, int mg, bool x_stage) {
    return 8 * ring * 4096 + (nred * 8 * mg * 2 * 16 * 17 + 8 * mg * 16) * sizeof(float) + 8192 + (x_stage ? 16384 : 0);
}
// Dynamic LDS of norm_glu_lds_f8_kernel<nw, ring>: the same image for nw waves, + one 4 KiB x stage and the norm-weight KiB per wave.  The launcher raises
// the limit to the 7-wave form's size: one limit for the three.
constexpr size_t norm_glu_lds_f8_bytes(int nw, int ring) {
    return (size_t)nw * ring * 4096 + (2 * nw * 2 * 16 * 17 + nw * 16) * sizeof(float) + (size_t)nw * (4096 + 1024);
}
