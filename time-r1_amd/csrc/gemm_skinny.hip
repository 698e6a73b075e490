// bf16 decode-row ("skinny") GEMMs for gfx950 (CDNA4): out[M,N] = act(x)[M,K] * W[N,K]^T for M <= 64 rows (one new token per rollout row), every launch
// HBM-bound on streaming W once.  Four kernels: gemm_skinny_kernel (register-fragment stream; optional cross-block split-K), norm_gemm_skinny_kernel (rmsnorm
// folded in; SwiGLU or RoPE + KV-append epilogues), norm_glu_lds_kernel and gemm_skinny_lds_fix_kernel (weights by DMA through per-wave LDS rings).  What they
// share with each other and with the fp8 twins of gemm_w8.hip is in skinny_common.h; the training GEMMs are in gemm.hip.
#include "skinny_common.h"
#include <stdlib.h>

#define BK 64      // k-step of every kernel here (one 128-byte row run of bf16)

// ------------------------------------------------------------------------------------------------------------------
// Skinny GEMM for the decode regime (M <= 64 rows, one new token per rollout row): out[M,N] = x[M,K] * W[N,K]^T.
// HBM-bound weight streaming: every W element is read exactly once, straight from global memory into the MFMA A
// fragment (no LDS: the operand is not shared between waves).  A block owns 16 output columns; its 4 waves split K
// and the partial 16x16 tiles are reduced through LDS.  Each lane fetches 32 contiguous bytes of one W row per
// step, so a 16-lane group covers one full 128-byte line per row; the k-order inside the MFMA is permuted the same
// way for x (any k permutation is legal as long as A and B agree).
// ------------------------------------------------------------------------------------------------------------------
// Optional block-timeline probe (tools/probe_skinny.hip compiles this file with -DTR1_PROBE): wall_clock64() at block entry, after
// the k loop and at block exit, 4 slots per block.  Not compiled into the library.
// The stamp probes of the other kernels here (tools/build_probe_lib.py, TR1_HIP_LIB=tools/_probe_lib.so) share one mechanism: TR1_STAMP_PROBE defines the device
// pointer and its extern "C" setter, a kernel keeps six s_memtime stamps in registers (TR1_STAMPS, TR1_STAMP) and writes them once, at its very end, to row
// `row` (8 slots) of the buffer from the lanes that satisfy `who` (TR1_STAMP_DUMP).  Each family below names its symbol, who dumps and which row.
#ifdef TR1_PROBE
__device__ unsigned long long* tr1_probe = nullptr;
#define TR1_PROBE_AT(slot) do { if (tr1_probe && threadIdx.x == 0) tr1_probe[(size_t)(blockIdx.y * gridDim.x + blockIdx.x) * 4 + (slot)] = wall_clock64(); } while (0)
#define TR1_STAMP_PROBE(sym, setter) __device__ unsigned long long* sym = nullptr; \
    extern "C" int setter(void* ptr) { return (int)hipMemcpyToSymbol(HIP_SYMBOL(sym), &ptr, sizeof(ptr)); }
#define TR1_STAMPS unsigned long long stamps_[6] = {0, 0, 0, 0, 0, 0}
#define TR1_STAMP(on, i) do { if (on) stamps_[i] = __builtin_amdgcn_s_memtime(); } while (0)
#define TR1_STAMP_DUMP(sym, who, row) do { if (sym && (who)) { \
    _Pragma("unroll") for (int i_ = 0; i_ < 6; ++i_) sym[(int64_t)(row) * 8 + i_] = stamps_[i_]; } } while (0)
#else
#define TR1_PROBE_AT(slot) do { } while (0)
#define TR1_STAMP_PROBE(sym, setter)
#define TR1_STAMPS do { } while (0)
#define TR1_STAMP(on, i) do { } while (0)
#define TR1_STAMP_DUMP(sym, who, row) do { } while (0)
#endif

// NCOL: 16-column groups per wave.  The x (activation) fragment is loaded once per k-step and reused for NCOL weight fragments, so
// the L2 traffic for x drops from 1x to 1/NCOL of the weight stream (matters at M = 16, where x is as large as a block's W slab).
// MG: 16-row groups of x (M <= 16*MG): every weight fragment fetched from HBM feeds MG MFMAs, so batching more rollout rows into one
// decode step (G = 16, or several prompts of a gradient-accumulation window) keeps the single pass over the weights.
// XLDS (round 3; MG = 1, no cross-block split-K): x reaches the MFMA through ONE DMA copy into LDS per block instead of per-wave vector loads - see the
// note at norm_gemm_skinny_kernel (the L1 tag pipe looks up 64 pieces per 1 KiB load in the operand layout; at NCOL = 1 half of the loads were x).
template <int WAVES, int UNROLL, int NCOL, int MG, bool XLDS = false>
__global__ __launch_bounds__(WAVES * 64) void gemm_skinny_kernel(const bf16_t* __restrict__ X, const bf16_t* __restrict__ W, bf16_t* __restrict__ C,
                                                                 float* __restrict__ Cf32, const bf16_t* __restrict__ bias,
                                                                 const bf16_t* __restrict__ residual, int M, int64_t N, int64_t K, int64_t ldx,
                                                                 int64_t ldw, int64_t ldc, int64_t ldr, float* __restrict__ fix_ws,
                                                                 int* __restrict__ fix_cnt) {
    __shared__ __attribute__((aligned(16))) float red[WAVES][NCOL][MG][16][17];
    __shared__ int s_ticket;
    extern __shared__ __attribute__((aligned(1024))) char sk_xs[];             // XLDS: [K/64 segments][16 rows][128 bytes]
    static_assert(!XLDS || MG == 1, "the LDS copy of x holds 16 rows");
    TR1_PROBE_AT(0);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int u = lane & 15, g = lane >> 4;
    const int64_t n0 = (int64_t)blockIdx.x * 16 * NCOL;
    // lane (u,g) takes k = g*8.. and 32+g*8.. of every 64-element step: a 16-lane group reads 64 contiguous bytes of a W row per load
    const bf16_t* wp[NCOL];
#pragma unroll
    for (int c = 0; c < NCOL; ++c) {
        int64_t wrow = n0 + c * 16 + u; if (wrow >= N) wrow = N - 1;
        wp[c] = W + wrow * ldw + g * 8;
    }
    // rows >= M of the MFMA B operand are padding: they re-read row M-1 (unconditional loads keep the k loop branch-free, so the
    // compiler can count the loads in flight instead of draining them with vmcnt(0)); their output columns are never stored
    const bf16_t* xp[MG];
#pragma unroll
    for (int mg = 0; mg < MG; ++mg) xp[mg] = X + (int64_t)(mg * 16 + u < M ? mg * 16 + u : (M - 1)) * ldx + g * 8;
    // gridDim.y > 1: cross-block split-K - block (x, y) covers k-steps [kb, ke); the partial tiles are merged by the in-kernel fixup below
    const int64_t nsteps_all = K / 64;
    const int64_t per_split = (nsteps_all + gridDim.y - 1) / gridDim.y;
    const int64_t kb = (int64_t)blockIdx.y * per_split;
    int64_t ke = kb + per_split; if (ke > nsteps_all) ke = nsteps_all;
    const int64_t nsteps = ke > kb ? ke - kb : 0;       // (skinny_wave_kslice with the slab's first step added: written out, the helper form reorders this kernel's prologue)
    const int64_t s_per = (nsteps + WAVES - 1) / WAVES;
    const int64_t s0 = kb + wave * s_per;
    int64_t s1 = s0 + s_per; if (s1 > ke) s1 = ke;
    f32x4_t acc[NCOL][MG][2];
#pragma unroll
    for (int c = 0; c < NCOL; ++c)
#pragma unroll
        for (int mg = 0; mg < MG; ++mg) { acc[c][mg][0] = (f32x4_t){0.f, 0.f, 0.f, 0.f}; acc[c][mg][1] = (f32x4_t){0.f, 0.f, 0.f, 0.f}; }
    const unsigned xs_base = (unsigned)(uintptr_t)(__attribute__((address_space(3))) void*)sk_xs;
    if (XLDS) SKINNY_X_TO_LDS(WAVES);
    const unsigned xs_lane = xs_base + (unsigned)(u * 128);
    const int xs_key = keyA(u);
    // Rotating software pipeline over UNROLL k-step buffers: a buffer is refilled (next k-step, UNROLL ahead) right after its MFMAs are
    // issued.  Measured neutral against the batch form (issue UNROLL steps, drain, repeat): hipcc still drains the queue once per trip
    // (s_waitcnt vmcnt(1)/vmcnt(0) at the loop header), and the N sweep of tools/probe_skinny.hip shows the kernel already at
    // t = 7 us + bytes / 5.4-5.8 TB/s, i.e. within ~15 % of what this access pattern streams at any size.
    bf16x8_t wa[UNROLL][NCOL][2], xa[UNROLL][MG][2];
#define SK_LOAD(q, st)                                                                                   \
    do {                                                                                                 \
        const int64_t k__ = (st) * 64;                                                                   \
        _Pragma("unroll") for (int c = 0; c < NCOL; ++c) {                                               \
            wa[q][c][0] = *reinterpret_cast<const bf16x8_t*>(wp[c] + k__);                               \
            wa[q][c][1] = *reinterpret_cast<const bf16x8_t*>(wp[c] + k__ + 32);                          \
        }                                                                                                \
        if (!XLDS) { _Pragma("unroll") for (int mg = 0; mg < MG; ++mg) {                                 \
            xa[q][mg][0] = *reinterpret_cast<const bf16x8_t*>(xp[mg] + k__);                             \
            xa[q][mg][1] = *reinterpret_cast<const bf16x8_t*>(xp[mg] + k__ + 32);                        \
        } }                                                                                              \
    } while (0)
#define SK_MFMA(q, st)                                                                                                        \
    do {                                                                                                                      \
        if (XLDS) {                                                                                                           \
            typedef const __attribute__((address_space(3))) bf16x8_t* xs_ptr_t;                                               \
            const unsigned xa__ = xs_lane + (unsigned)(st) * 2048u;                                                           \
            xa[q][0][0] = *(xs_ptr_t)(uintptr_t)(xa__ + (unsigned)(((0 + g) ^ xs_key) << 4));                                 \
            xa[q][0][1] = *(xs_ptr_t)(uintptr_t)(xa__ + (unsigned)(((4 + g) ^ xs_key) << 4));                                 \
        }                                                                                                                     \
        _Pragma("unroll") for (int c = 0; c < NCOL; ++c)                                                                      \
            _Pragma("unroll") for (int mg = 0; mg < MG; ++mg) {                                                               \
                acc[c][mg][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa[q][c][0], xa[q][mg][0], acc[c][mg][0], 0, 0, 0);   \
                acc[c][mg][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa[q][c][1], xa[q][mg][1], acc[c][mg][1], 0, 0, 0);   \
            }                                                                                                                 \
    } while (0)
    int64_t s = s0;
#pragma unroll
    for (int q = 0; q < UNROLL; ++q)
        if (s0 + q < s1) SK_LOAD(q, s0 + q);
    if (XLDS) {       // the x copy has landed for this wave when only the UNROLL * 2 NCOL younger register loads are still in flight
        static_assert(!XLDS || UNROLL * 2 * NCOL == 8, "vmcnt below is written for 8 register loads in the prologue");
        asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    }
    for (; s + 2 * UNROLL <= s1; s += UNROLL) {          // steady state: branch-free
#pragma unroll
        for (int q = 0; q < UNROLL; ++q) { SK_MFMA(q, s + q); SK_LOAD(q, s + q + UNROLL); }
    }
#pragma unroll
    for (int q = 0; q < UNROLL; ++q)
        if (s + q < s1) { SK_MFMA(q, s + q); if (s + q + UNROLL < s1) SK_LOAD(q, s + q + UNROLL); }
    s += UNROLL;
#pragma unroll
    for (int q = 0; q < UNROLL; ++q)
        if (s + q < s1) SK_MFMA(q, s + q);
#undef SK_LOAD
#undef SK_MFMA
    // D[row = n index (g*4+r)][col = m (u)]
#pragma unroll
    for (int c = 0; c < NCOL; ++c)
#pragma unroll
        for (int mg = 0; mg < MG; ++mg)
#pragma unroll
            for (int r = 0; r < 4; ++r) red[wave][c][mg][u][g * 4 + r] = acc[c][mg][0][r] + acc[c][mg][1][r];
    TR1_PROBE_AT(1);
    __syncthreads();
    TR1_PROBE_AT(2);
    constexpr int TILE = NCOL * MG * 256;
    if (fix_cnt) {      // cross-block split-K (gridDim.y slabs): the partial tiles are merged by the last-arriving block
        SKINNY_SPLITK_FIXUP(TILE, WAVES * 64, MG, true, red[w][c][mg][mm][nn], s_ticket, , , return, {
            const int m = mg * 16 + mm;
            const int64_t n = n0 + c * 16 + nn;
            if (m < M && n < N) {
                if (bias) v += bf2f(bias[n]);
                if (residual) v += bf2f(residual[(int64_t)m * ldr + n]);
                if (Cf32) Cf32[(int64_t)m * ldc + n] = v;
                else C[(int64_t)m * ldc + n] = f2bf(v);
            }
        });
        return;
    }
    for (int i = threadIdx.x; i < TILE; i += WAVES * 64) {   // (column group, row group, m, n)
        SKINNY_TILE_IDX(MG, i);
        const int m = mg * 16 + mm;
        const int64_t n = n0 + c * 16 + nn;
        if (m < M && n < N) {
            float v = 0.f;
#pragma unroll
            for (int w = 0; w < WAVES; ++w) v += red[w][c][mg][mm][nn];
            if (bias) v += bf2f(bias[n]);
            if (residual) v += bf2f(residual[(int64_t)m * ldr + n]);
            if (Cf32) Cf32[(int64_t)m * ldc + n] = v;
            else C[(int64_t)m * ldc + n] = f2bf(v);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------
// Decode-step fusion: out = rmsnorm(x; lnw) @ W^T with the normalisation folded into the GEMM (every block streams all of x anyway):
//   prologue  x'[m,k] = bf16(x[m,k] * lnw[k]) feeds the MFMA while sum_k x^2 is accumulated per row; the epilogue scales row m by
//             rstd[m] = rsqrt(mean x^2 + eps)  (rmsnorm is linear after the row scale, so the GEMM commutes with it)
//   GLU       the block's two column groups are gate rows n0.. and up rows up_off+n0.. of W; the epilogue writes
//             silu(gate) * up (Qwen2MLP TF:459-466), so the [M, 2I] intermediate never reaches HBM.
// Saves the separate rmsnorm / swiglu launches of a decode layer (each ~6-7 us of pure launch + fill/drain at M <= 64 rows).
// ------------------------------------------------------------------------------------------------------------------
// block timeline of the fused QKV launch (tools/bench_qkv32.py PROBE=1 against tools/_probe_lib.so): s_memtime at entry / first loads issued / stream
// consumed / partials reduced (after the barrier) / epilogue stored, for waves 0 and WAVES-1 of every block
TR1_STAMP_PROBE(tr1_qkv_probe, probe_qkv_set_ptr)
#define QKV_STAMP(i) TR1_STAMP(QKV, i)
#define QKV_DUMP() TR1_STAMP_DUMP(tr1_qkv_probe, QKV && lane == 0 && (wave == 0 || wave == WAVES - 1), (int64_t)blockIdx.x * 2 + (wave ? 1 : 0))
// QKV: the block's two column groups are columns (d, d + hd/2) of one head and the epilogue is qkv_epilogue_store (RoPE + cache append).
// XLDS (round 3, MG = 1): the activation rows do not travel through the vector-memory path at all.  In the MFMA operand layout a wave load touches 16
// rows x 64 bytes = 64 separate (line, 16-byte) pieces, and the L1 tag pipe looks them up one per cycle: a 1 KiB load instruction costs ~64 cycles
// (measured 38-54 GB/s per CU in this kernel, block timeline in DESIGN.md), and half of this kernel's load instructions were x and lnw.  With XLDS the
// block copies x ONCE into LDS by DMA (8 rows x 128 bytes per instruction = 8 lines; 16 rows x K, swizzled on the source address like every other
// tile here) and reads its fragments with ds_read_b128; only the weights stay on the register path.  Same values, same order of operations.
template <int WAVES, int UNROLL, int MG, bool GLU, int NCOL = 2, bool QKV = false, bool XLDS = false>
__global__ __launch_bounds__(WAVES * 64) void norm_gemm_skinny_kernel(const bf16_t* __restrict__ X, const bf16_t* __restrict__ lnw,
                                                                      const bf16_t* __restrict__ W, bf16_t* __restrict__ C,
                                                                      const bf16_t* __restrict__ bias, int M, int64_t N, int64_t K, int64_t ldx,
                                                                      int64_t ldw, int64_t ldc, float eps, int64_t up_off, QkvEpi qe = QkvEpi{}) {
    static_assert(!GLU || NCOL % 2 == 0, "GLU pairs NCOL/2 gate column groups with NCOL/2 up column groups");
    static_assert(!QKV || (NCOL == 2 && !GLU), "QKV pairs the two rotate-half column groups of a head");
    static_assert(!XLDS || MG == 1, "the LDS copy of x holds 16 rows");
    extern __shared__ __attribute__((aligned(1024))) char ng_xs[];             // XLDS: [K/64 segments][16 rows][128 bytes]
    __shared__ __attribute__((aligned(16))) float red[WAVES][NCOL][MG][16][17];
    __shared__ float ssred[WAVES][MG][16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    TR1_STAMPS;
    QKV_STAMP(0);
    const int u = lane & 15, g = lane >> 4;
    const int qkv_gph = QKV ? qe.hd >> 5 : 1;                                   // 16-column group pairs per head
    const int qkv_h = QKV ? (int)blockIdx.x / qkv_gph : 0, qkv_j = QKV ? (int)blockIdx.x % qkv_gph : 0;
    constexpr int OG = GLU ? NCOL / 2 : (QKV ? 1 : NCOL);                       // output column groups per block
    const int64_t n0 = QKV ? (int64_t)qkv_h * qe.hd + qkv_j * 16 : (int64_t)blockIdx.x * (16 * OG);
    const bf16_t* wp[NCOL];
#pragma unroll
    for (int c = 0; c < NCOL; ++c) {
        int64_t wrow = QKV ? n0 + c * (qe.hd >> 1) + u : (GLU ? n0 + (c % OG) * 16 + u : n0 + c * 16 + u);
        if (wrow >= N) wrow = N - 1;
        if (GLU && c >= OG) wrow += up_off;
        wp[c] = W + wrow * ldw + g * 8;
    }
    const bf16_t* xp[MG];      // rows >= M re-read row M-1 (see gemm_skinny_kernel); their outputs are never stored
#pragma unroll
    for (int mg = 0; mg < MG; ++mg) xp[mg] = X + (int64_t)(mg * 16 + u < M ? mg * 16 + u : (M - 1)) * ldx + g * 8;
    const bf16_t* lp = lnw + g * 8;
    int64_t s0, s1;
    skinny_wave_kslice<WAVES>(K / 64, wave, s0, s1);
    constexpr int NA = (GLU && NCOL >= 4) ? 1 : 2;      // accumulators per tile: the wide GLU forms have enough independent tiles to hide the MFMA latency
    f32x4_t acc[NCOL][MG][NA];
    float ss[MG];
#pragma unroll
    for (int mg = 0; mg < MG; ++mg) {
        ss[mg] = 0.f;
#pragma unroll
        for (int c = 0; c < NCOL; ++c) { acc[c][mg][0] = (f32x4_t){0.f, 0.f, 0.f, 0.f}; acc[c][mg][NA - 1] = (f32x4_t){0.f, 0.f, 0.f, 0.f}; }
    }
    const unsigned xs_base = (unsigned)(uintptr_t)(__attribute__((address_space(3))) void*)ng_xs;
    if (XLDS) SKINNY_X_TO_LDS(WAVES);
    const unsigned xs_lane = xs_base + (unsigned)(u * 128);
    const int xs_key = keyA(u);
    // rotating software pipeline over UNROLL k-step buffers (see gemm_skinny_kernel)
    bf16x8_t wa[UNROLL][NCOL][2], xa[UNROLL][MG][2], la[UNROLL][2];
#define NG_LOAD(q, st)                                                                                   \
    do {                                                                                                 \
        const int64_t k__ = (st) * 64;                                                                   \
        _Pragma("unroll") for (int c = 0; c < NCOL; ++c) {                                               \
            wa[q][c][0] = *reinterpret_cast<const bf16x8_t*>(wp[c] + k__);                               \
            wa[q][c][1] = *reinterpret_cast<const bf16x8_t*>(wp[c] + k__ + 32);                          \
        }                                                                                                \
        if (!XLDS) { _Pragma("unroll") for (int mg = 0; mg < MG; ++mg) {                                 \
            xa[q][mg][0] = *reinterpret_cast<const bf16x8_t*>(xp[mg] + k__);                             \
            xa[q][mg][1] = *reinterpret_cast<const bf16x8_t*>(xp[mg] + k__ + 32);                        \
        } }                                                                                              \
        la[q][0] = *reinterpret_cast<const bf16x8_t*>(lp + k__);                                         \
        la[q][1] = *reinterpret_cast<const bf16x8_t*>(lp + k__ + 32);                                    \
    } while (0)
#define NG_MFMA(q, st)                                                                                                        \
    do {                                                                                                                      \
        if (XLDS) {                                                                                                           \
            typedef const __attribute__((address_space(3))) bf16x8_t* xs_ptr_t;                                               \
            const unsigned xa__ = xs_lane + (unsigned)(st) * 2048u;                                                           \
            xa[q][0][0] = *(xs_ptr_t)(uintptr_t)(xa__ + (unsigned)(((0 + g) ^ xs_key) << 4));                                 \
            xa[q][0][1] = *(xs_ptr_t)(uintptr_t)(xa__ + (unsigned)(((4 + g) ^ xs_key) << 4));                                 \
        }                                                                                                                     \
        _Pragma("unroll") for (int mg = 0; mg < MG; ++mg) {                                                                   \
            const bf16x8_t x0__ = scale_frag_sumsq(xa[q][mg][0], la[q][0], ss[mg]);                                           \
            const bf16x8_t x1__ = scale_frag_sumsq(xa[q][mg][1], la[q][1], ss[mg]);                                           \
            _Pragma("unroll") for (int c = 0; c < NCOL; ++c) {                                                                \
                acc[c][mg][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa[q][c][0], x0__, acc[c][mg][0], 0, 0, 0);           \
                acc[c][mg][NA - 1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa[q][c][1], x1__, acc[c][mg][NA - 1], 0, 0, 0); \
            }                                                                                                                 \
        }                                                                                                                     \
    } while (0)
    int64_t s = s0;
#pragma unroll
    for (int q = 0; q < UNROLL; ++q)
        if (s0 + q < s1) NG_LOAD(q, s0 + q);
    QKV_STAMP(1);
    if (XLDS) {       // the x copy has landed for this wave when only the UNROLL * (2 NCOL + 2) younger register loads are still in flight
        static_assert(!XLDS || UNROLL * (2 * NCOL + 2) == 12, "vmcnt below is written for 12 register loads in the prologue");
        asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    }
    for (; s + 2 * UNROLL <= s1; s += UNROLL) {
#pragma unroll
        for (int q = 0; q < UNROLL; ++q) { NG_MFMA(q, s + q); NG_LOAD(q, s + q + UNROLL); }
    }
#pragma unroll
    for (int q = 0; q < UNROLL; ++q)
        if (s + q < s1) { NG_MFMA(q, s + q); if (s + q + UNROLL < s1) NG_LOAD(q, s + q + UNROLL); }
    s += UNROLL;
#pragma unroll
    for (int q = 0; q < UNROLL; ++q)
        if (s + q < s1) NG_MFMA(q, s + q);
#undef NG_LOAD
#undef NG_MFMA
    QKV_STAMP(2);
#pragma unroll
    for (int mg = 0; mg < MG; ++mg) {     // lanes u, u+16, u+32, u+48 hold disjoint k chunks of row u
        float v = ss[mg];
        v += __shfl_xor(v, 16, 64);
        v += __shfl_xor(v, 32, 64);
        if (g == 0) ssred[wave][mg][u] = v;
#pragma unroll
        for (int c = 0; c < NCOL; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) red[wave][c][mg][u][g * 4 + r] = NA == 2 ? acc[c][mg][0][r] + acc[c][mg][1][r] : acc[c][mg][0][r];
    }
    __syncthreads();
    QKV_STAMP(3);
    const float inv_k = 1.f / (float)K;
    for (int i = threadIdx.x; i < OG * MG * 256; i += WAVES * 64) {   // (column group, row group, m, n)
        SKINNY_TILE_IDX(MG, i);
        const int m = mg * 16 + mm;
        const int64_t n = n0 + c * 16 + nn;
        if (m < M && n < N) {
            float sq = 0.f, v = 0.f, v2 = 0.f;
#pragma unroll
            for (int w = 0; w < WAVES; ++w) { sq += ssred[w][mg][mm]; v += red[w][c][mg][mm][nn]; if (GLU || QKV) v2 += red[w][GLU ? c + OG : 1][mg][mm][nn]; }
            const float rstd = rsqrtf(sq * inv_k + eps);
            v = __fmul_rn(v, rstd);          // explicitly rounded (no fma contraction): the fused-QKV and two-kernel paths agree bit for bit
            if (QKV) {      // same rounding points as projection -> bf16 qkv buffer -> decode_qkv_post
                const int64_t nb = n + (qe.hd >> 1);
                float vb = __fmul_rn(v2, rstd);
                if (bias) { v = __fadd_rn(v, bf2f(bias[n])); vb = __fadd_rn(vb, bf2f(bias[nb])); }
                qkv_epilogue_store(qe, m, qkv_h, qkv_j * 16 + nn, bf2f(f2bf(v)), bf2f(f2bf(vb)));
            } else if (GLU) {      // same rounding points as the unfused path: gate/up rounded to bf16, silu rounded, product rounded
                const float gt = bf2f(f2bf(v)), up = bf2f(f2bf(v2 * rstd));
                C[(int64_t)m * ldc + n] = f2bf(bf2f(f2bf(silu_f32(gt))) * up);
            } else {
                if (bias) v = __fadd_rn(v, bf2f(bias[n]));
                C[(int64_t)m * ldc + n] = f2bf(v);
            }
        }
    }
    QKV_STAMP(4);
    QKV_DUMP();
}

// ------------------------------------------------------------------------------------------------------------------
// LDS-streamed form of the fused rmsnorm + gate/up + SwiGLU decode GEMM (M <= 16 rows).
// The register-fragment stream of norm_gemm_skinny_kernel reads 64-byte pieces of 16 weight rows per wave instruction and tops out at
// ~4.8 TB/s (a pure load kernel with that shape: 5.5 TB/s; with row-contiguous requests: 6.1 TB/s, tools/probe_stream.hip).  Here the
// weights go HBM -> LDS with global_load_lds in full 128-byte row runs (8 rows per wave instruction), each wave keeps its OWN ring of
// stages in LDS and reads the MFMA fragments back with ds_read_b128, so nothing but the issuing wave's counted vmcnt orders a stage
// (no barrier in the stream).  Consequences used below:
//   * a block is PERSISTENT over a contiguous range of column-group pairs (16 gate rows + 16 up rows), so the activation fragments
//     x' = bf16(x * lnw) of the wave's k-slice (K/8 columns) are built ONCE and stay in registers, and sum x^2 is reduced once per block;
//   * after the last stage of a pair the eight waves drop their partial tiles in LDS, meet at ONE raw barrier (the DMA of the next pair
//     stays in flight) and 256 threads finish one output each, with the rounding points of norm_gemm_skinny_kernel's GLU epilogue.  The
//     epilogue's global stores share vmcnt with the DMA; that is safe for the counted waits: loads retire in order among themselves, so
//     "at most 4(R-1) operations outstanding" still implies that the stage being consumed has landed - outstanding stores can only make
//     a wait longer, never shorter.
// LDS image of a stage: [gate 16 rows | up 16 rows] x 128 bytes (64 k); row r keeps its logical 16-byte chunk c at position c ^ keyA(r)
// (applied on the SOURCE address of the DMA): the 16-row fragment reads are conflict-free.
// ------------------------------------------------------------------------------------------------------------------
// QKV (round 3): the same stream for the fused rmsnorm + q/k/v projection + M-RoPE + KV append at <= 16 rows.  One block per column-group pair
// (16 columns d of a head and their rotate-half partners d + hd/2: `up_off` = hd/2 weight rows), no persistence (144 pairs at 7B), epilogue and
// rounding points of norm_gemm_skinny_kernel's QKV form - same k-slices per wave, same two accumulators per tile, same wave-order reduction, so the
// result is bit-identical to it.  What changes is the path of the weights: full 128-byte row runs by DMA (8 tag look-ups per KiB) instead of
// 64-byte pieces of 16 rows per wave load (64 look-ups per KiB: the L1 tag pipe held the register-fragment kernel at ~40 GB/s per CU).
TR1_STAMP_PROBE(tr1_glu_probe, probe_glu_set_ptr)      // waves 0 and 7 of every block (tools/bench_glu32.py)
#define GLU_STAMP(i) TR1_STAMP(true, i)
#define GLU_DUMP() TR1_STAMP_DUMP(tr1_glu_probe, lane == 0 && (wave == 0 || wave == 7), (int64_t)blockIdx.x * 2 + (wave ? 1 : 0))
// MODE 0: gate/up + SwiGLU.  MODE 1: fused QKV (above).  MODE 2 (round 3): plain projection C = rmsnorm(x) W^T for a wide N (the lm_head): the block's two
// row groups are output columns n and n + N/2 (`up_off` = N/2 weight rows apart), both stored as they are.
template <int NST, int R, int NRED = 2, int MG = 1, int MODE = 0>
__global__ __launch_bounds__(512) void norm_glu_lds_kernel(const bf16_t* __restrict__ X, const bf16_t* __restrict__ lnw, const bf16_t* __restrict__ W,
                                                           bf16_t* __restrict__ C, int M, int64_t N, int64_t K, int64_t ldx, int64_t ldw,
                                                           int64_t ldc, float eps, int64_t up_off, const bf16_t* __restrict__ bias = nullptr,
                                                           QkvEpi qe = QkvEpi{}, int c_frag = 0) {
    // c_frag (MODE 0, MG = 1; round 6): the SwiGLU output leaves FRAGMENT-MAJOR - element (m, n) at (n / 32) * 512 + m * 32 + n % 32, the layout
    // tr1_gemm_oproj_frag reads (one contiguous KiB per MFMA operand fragment) - for the all-stages-in-flight down projection of the 2B shapes
    constexpr bool QKV = MODE == 1, PLAIN = MODE == 2;
    constexpr int STAGE = 4096;                                            // bytes per stage: gate 2 KiB + up 2 KiB
    constexpr int REDW = MG * 2 * 16 * 17;                                 // floats of one wave's partial: MG row groups x (gate | up)
    // red[2][8][REDW] f32 | ssq[8][16] | [8 waves][R stages][4 KiB].  The rings come LAST: a DMA destination is passed as (slot - stage offset)
    // because the instruction's immediate offset is added to the LDS address too, and that pointer must not fall below the LDS base.
    extern __shared__ __attribute__((aligned(16))) char glu_lds[];
    float* red = reinterpret_cast<float*>(glu_lds);
    float* ssq = red + NRED * 8 * REDW;                                   // [8 waves][MG][16]
    char* rings = glu_lds + (NRED * 8 * REDW + 8 * MG * 16) * sizeof(float);
    static_assert((NRED * 8 * REDW + 8 * MG * 16) * sizeof(float) >= 6 * 128 && ((NRED * 8 * REDW + 8 * MG * 16) * sizeof(float)) % 16 == 0, "ring base");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, u = lane & 15, g = lane >> 4;
    TR1_STAMPS;
    GLU_STAMP(0);
    const int64_t NP = QKV ? (int64_t)gridDim.x : (PLAIN ? up_off / 16 : (N + 15) / 16);
    const int64_t p0 = NP * blockIdx.x / gridDim.x, p1 = NP * (blockIdx.x + 1) / gridDim.x;
    const int qkv_gph = QKV ? qe.hd >> 5 : 1;                               // column-group pairs per head
    const int qkv_h = QKV ? (int)blockIdx.x / qkv_gph : 0, qkv_j = QKV ? (int)blockIdx.x % qkv_gph : 0;
    const int64_t row_base = QKV ? (int64_t)qkv_h * qe.hd + qkv_j * 16 : p0 * 16;      // first weight row of the block's first pair
    const int npair = (int)(p1 - p0);
    const int64_t kb = (int64_t)wave * (K / 8);
    // ---- DMA lane map: instruction j covers rows 8j .. 8j+7; lane -> row 8j + (lane >> 3), physical chunk lane & 7, logical chunk ^ keyA(row).
    // Four per-lane source pointers (gate / up rows of the pair being ISSUED) advance by 16 rows per pair; the stage inside the pair is an
    // immediate offset of the DMA instruction, so issuing a stage costs no vector ALU work.
    char* ring = rings + wave * R * STAGE;
    const int total = npair * NST;
    const bf16_t* pg[2]; const bf16_t* pu[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int r = 8 * j + (lane >> 3);
        pg[j] = W + (row_base + r) * ldw + kb + (((lane & 7) ^ keyA(r)) << 3);
        pu[j] = pg[j] + up_off * ldw;
    }
    const int64_t pair_step = 16 * ldw;
    int islot = 0;                                       // ring slot of the next item to issue (wave-uniform)
#define GLU_ISSUE(ST) do {                                                                                               \
        char* dst__ = ring + islot * STAGE - (ST) * 128;   /* the instruction offset is added to the LDS address as well */  \
        _Pragma("unroll") for (int j = 0; j < 2; ++j) {                                                                  \
            __builtin_amdgcn_global_load_lds((gptr_t)pg[j], (lptr_t)(dst__ + j * 1024), 16, (ST) * 128, TR1_W_AUX);              \
            __builtin_amdgcn_global_load_lds((gptr_t)pu[j], (lptr_t)(dst__ + 2048 + j * 1024), 16, (ST) * 128, TR1_W_AUX);       \
        }                                                                                                                \
        islot = (islot + 1 == R) ? 0 : islot + 1;                                                                        \
    } while (0)
#define GLU_ISSUE_ST(ST) do { switch (ST) { case 0: GLU_ISSUE(0); break; case 1: GLU_ISSUE(1); break; case 2: GLU_ISSUE(2); break; case 3: GLU_ISSUE(3); break; \
                                           case 4: GLU_ISSUE(4); break; case 5: GLU_ISSUE(5); break; default: GLU_ISSUE(6); break; } } while (0)
#define GLU_NEXT_PAIR() do { _Pragma("unroll") for (int j = 0; j < 2; ++j) { pg[j] += pair_step; pu[j] += pair_step; } } while (0)
    static_assert(NST <= 7, "stage offsets are enumerated up to 7");
    constexpr bool XDMA = (MG <= 2) && (2 * R + NRED >= NST);   // round 3: this wave's x slice goes through its own (still empty) ring first (MG = 2: one 16-row group after the other)
#define GLU_PROLOGUE(I0, I1) do {                                                                                \
        _Pragma("unroll") for (int i = (I0); i < (I1); ++i) {    /* prologue: items 0 .. R-2 */                  \
            if (i < total) {                                                                                     \
                if (i > 0 && i % NST == 0) GLU_NEXT_PAIR();                                                      \
                GLU_ISSUE_ST(i % NST);                                                                           \
            }                                                                                                    \
        } } while (0)
    // x staging that leaves ring slot 0 to the FIRST weight stage (requested together with the x copy): slots 1 .. R-1, the reduction slices and one
    // extra 2 KiB per wave behind the norm-weight area
    constexpr bool XSLOT0 = XDMA && MG == 1 && (2 * (R - 1) + NRED + 1 >= NST) && R >= 3;
    if (!XDMA) GLU_PROLOGUE(0, R - 1);
    GLU_STAMP(1);
    // ---- x' fragments of this wave's k-slice (once per block) and the row sums of squares - built AFTER the first weight stages were
    // issued, so the HBM stream starts at kernel entry instead of waiting for this L2 round trip
    bf16x8_t xr[MG][NST * 2];
    if (XDMA) {
        // The round-2 form loaded x and lnw with per-wave vector loads AFTER issuing the first weight stages: 28 loads per lane in four dependent
        // batches, each load touching 16 rows x 64 bytes (64 L1 tag look-ups per KiB) - 15 400 of the launch's 98 000 cycles, with only two weight stages
        // in flight meanwhile (block timeline).  Here the wave's x slice (16 rows x K/8 columns = NST stages of 2 KiB) is copied by DMA into
        // its own ring (and, past 2R stages, its reduction slices - all unused so far), read back as fragments, and only then does the weight
        // stream start: one L2 round trip instead of four, 8 tag look-ups per KiB.  Same fragments in the same order -> same sum of squares.
        // the wave's slice of the norm weight as well: ONE DMA instruction (1 KiB = 512 columns from kb on; lanes past the end of lnw re-read its
        // last 16 bytes) into a private KiB behind the rings instead of 2 NST vector loads per lane
        char* lnw_lds = rings + 8 * R * STAGE + wave * 1024;
        {
            int64_t col = kb + lane * 8;
            if (col + 8 > K) col = K - 8;
            __builtin_amdgcn_global_load_lds((gptr_t)(lnw + col), (lptr_t)lnw_lds, 16, 0, 0);
        }
        char* const x_extra = rings + 8 * R * STAGE + 8 * 1024 + wave * 2048;
        auto x_stage = [&](int st) -> char* {
            if (!XSLOT0) return st < 2 * R ? ring + st * 2048 : reinterpret_cast<char*>(red + ((st - 2 * R) * 8 + wave) * REDW);
            if (st < 2 * (R - 1)) return ring + STAGE + st * 2048;
            if (st - 2 * (R - 1) < NRED) return reinterpret_cast<char*>(red + ((st - 2 * (R - 1)) * 8 + wave) * REDW);
            return x_extra;
        };
#pragma unroll
        for (int mg = 0; mg < MG; ++mg) {
        float ss = 0.f;
#pragma unroll
        for (int st = 0; st < NST; ++st) {
            char* dst = x_stage(st);
#pragma unroll
            for (int jx = 0; jx < 2; ++jx) {
                const int r = mg * 16 + 8 * jx + (lane >> 3);
                const bf16_t* src = X + (int64_t)(r < M ? r : M - 1) * ldx + kb + st * 64 + (((lane & 7) ^ keyA(r & 15)) << 3);
                __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(dst + jx * 1024), 16, 0, 0);
            }
        }
        if (XSLOT0) {
            GLU_PROLOGUE(0, 1);                                           // the first weight stage travels while x' is built
            asm volatile("s_waitcnt vmcnt(4)" ::: "memory");              // everything but that stage's four DMA instructions has landed
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
#pragma unroll
        for (int i = 0; i < NST * 2; ++i) {
            const int st = i >> 1, ks = i & 1;
            const char* sbx = x_stage(st);
            const bf16x8_t xv = *reinterpret_cast<const bf16x8_t*>(sbx + u * 128 + (((ks * 4 + g) ^ keyA(u)) << 4));
            const bf16x8_t lvi = *reinterpret_cast<const bf16x8_t*>(lnw_lds + (i * 32 + g * 8) * 2);
            u32x4_t f = __builtin_bit_cast(u32x4_t, scale_frag_sumsq(xv, lvi, ss));
            asm volatile("" : "+v"(f));
            xr[mg][i] = __builtin_bit_cast(bf16x8_t, f);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");              // the ring is free again: next row group / start (continue) the weight stream
        float v = ss;
        v += __shfl_xor(v, 16, 64);
        v += __shfl_xor(v, 32, 64);
        if (g == 0) ssq[(wave * MG + mg) * 16 + u] = v;
        }
        if (XSLOT0) GLU_PROLOGUE(1, R - 1); else GLU_PROLOGUE(0, R - 1);
    } else
    {
        float ss[MG];
        const bf16_t* xp[MG];
#pragma unroll
        for (int mg = 0; mg < MG; ++mg) { ss[mg] = 0.f; xp[mg] = X + (int64_t)(mg * 16 + u < M ? mg * 16 + u : M - 1) * ldx + kb + g * 8; }
        const bf16_t* lp = lnw + kb + g * 8;
#pragma unroll
        for (int i0 = 0; i0 < NST * 2; i0 += 4) {        // four k-halves at a time: the loads of ALL fragments in flight at once would not fit the
#pragma unroll                                           // register file next to xr at MG = 2 (scheduling fence below)
            for (int i = i0; i < i0 + 4 && i < NST * 2; ++i) {
                const bf16x8_t lv = *reinterpret_cast<const bf16x8_t*>(lp + i * 32);
#pragma unroll
                for (int mg = 0; mg < MG; ++mg) {
                    const bf16x8_t xv = *reinterpret_cast<const bf16x8_t*>(xp[mg] + i * 32);
                    u32x4_t f = __builtin_bit_cast(u32x4_t, scale_frag_sumsq(xv, lv, ss[mg]));
                    asm volatile("" : "+v"(f));          // pin the PACKED fragment here: left alone, the compiler keeps the unpacked f32 products
                    xr[mg][i] = __builtin_bit_cast(bf16x8_t, f);     // live into the main loop (2x the registers) and spills at MG = 2
                }
            }
            if (MG > 1) __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int mg = 0; mg < MG; ++mg) {
            float v = ss[mg];
            v += __shfl_xor(v, 16, 64);
            v += __shfl_xor(v, 32, 64);
            if (g == 0) ssq[(wave * MG + mg) * 16 + u] = v;
        }
    }
    GLU_STAMP(2);
    TR1_BARRIER();                                       // the eight waves' sum-of-squares partials are in LDS (the prologue DMA is in flight)
    GLU_STAMP(3);
    float rstd;
    {
        float sq = 0.f;
#pragma unroll
        for (int w = 0; w < 8; ++w) sq += ssq[(w * MG + (MG > 1 ? (threadIdx.x >> 8) : 0)) * 16 + ((threadIdx.x >> 4) & 15)];
        rstd = rsqrtf(sq * (1.f / (float)K) + eps);
    }
    const int rd_off = u * 128;
    const int kA = keyA(u);
    int cslot = 0;                                       // ring slot of the item being consumed
    for (int pi = 0; pi < npair; ++pi) {
        f32x4_t ag[MG][2], au[MG][2];
#pragma unroll
        for (int mg = 0; mg < MG; ++mg) ag[mg][0] = ag[mg][1] = au[mg][0] = au[mg][1] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int st = 0; st < NST; ++st) {
            const int item = pi * NST + st;
            if (item + R - 1 < total) {
                if ((st + R - 1) % NST == 0) GLU_NEXT_PAIR();           // the issue stream enters the next pair here (compile-time position)
                GLU_ISSUE_ST((st + R - 1) % NST);
            }
            const int rem = total - 1 - item;              // items issued after this one and still allowed in flight
            if (rem >= R - 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 * (R - 1)) : "memory");
            else if (rem == 2 && R > 3) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
            else if (rem == 1 && R > 2) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const char* sb = ring + cslot * STAGE + rd_off;
            cslot = (cslot + 1 == R) ? 0 : cslot + 1;
            bf16x8_t wg[2], wu[2];
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const int off = ((ks * 4 + g) ^ kA) << 4;
                wg[ks] = *reinterpret_cast<const bf16x8_t*>(sb + off);
                wu[ks] = *reinterpret_cast<const bf16x8_t*>(sb + 2048 + off);
            }
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int mg = 0; mg < MG; ++mg) {
                    ag[mg][ks] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wg[ks], xr[mg][st * 2 + ks], ag[mg][ks], 0, 0, 0);
                    au[mg][ks] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wu[ks], xr[mg][st * 2 + ks], au[mg][ks], 0, 0, 0);
                }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");          // this stage's reads have returned before its slot can be refilled
        }
        float* rw = red + ((NRED == 2 ? (pi & 1) : 0) * 8 + wave) * REDW;
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int mg = 0; mg < MG; ++mg) {
                rw[mg * 544 + u * 17 + g * 4 + r] = ag[mg][0][r] + ag[mg][1][r];
                rw[mg * 544 + 16 * 17 + u * 17 + g * 4 + r] = au[mg][0][r] + au[mg][1][r];
            }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        TR1_BARRIER();                                                  // partial tiles are visible; the DMA of the next pair stays in flight
        if (threadIdx.x < 256 * MG) {
            const int mgi = MG > 1 ? (threadIdx.x >> 8) : 0, mm = (threadIdx.x >> 4) & 15, nn = threadIdx.x & 15;
            const float* rb = red + (NRED == 2 ? (pi & 1) : 0) * 8 * REDW + mgi * 544;
            float v = 0.f, v2 = 0.f;
#pragma unroll
            for (int w = 0; w < 8; ++w) { v += rb[w * REDW + mm * 17 + nn]; v2 += rb[w * REDW + 16 * 17 + mm * 17 + nn]; }
            v = __fmul_rn(v, rstd);
            if (QKV) {      // rounding points of norm_gemm_skinny_kernel's QKV epilogue (projection -> bf16 -> RoPE / cache append)
                const int64_t n = row_base + nn, nb = n + (qe.hd >> 1);
                float vb = __fmul_rn(v2, rstd);
                if (bias) { v = __fadd_rn(v, bf2f(bias[n])); vb = __fadd_rn(vb, bf2f(bias[nb])); }
                if (mgi * 16 + mm < M && n < N) qkv_epilogue_store(qe, mgi * 16 + mm, qkv_h, qkv_j * 16 + nn, bf2f(f2bf(v)), bf2f(f2bf(vb)));
            } else if (PLAIN) {
                const int64_t n = (p0 + pi) * 16 + nn;
                float vb = __fmul_rn(v2, rstd);
                if (bias) { v = __fadd_rn(v, bf2f(bias[n])); vb = __fadd_rn(vb, bf2f(bias[n + up_off])); }
                const int mrow = mgi * 16 + mm;
                if (mrow < M && n < up_off) { C[(int64_t)mrow * ldc + n] = f2bf(v); if (n + up_off < N) C[(int64_t)mrow * ldc + n + up_off] = f2bf(vb); }
            } else {
            const float gt = bf2f(f2bf(v)), up = bf2f(f2bf(v2 * rstd));
            const int64_t n = (p0 + pi) * 16 + nn;
            if (mgi * 16 + mm < M && n < N) C[c_frag ? (n >> 5) * 512 + mm * 32 + (n & 31) : (int64_t)(mgi * 16 + mm) * ldc + n] = f2bf(bf2f(f2bf(silu_f32(gt))) * up);
            }
        }
        if (NRED == 1) TR1_BARRIER();                                   // single reduction buffer: everybody has read it before the next pair writes
        if (pi == 0) GLU_STAMP(4);
    }
    GLU_STAMP(5);
    GLU_DUMP();
#undef GLU_ISSUE
#undef GLU_ISSUE_ST
#undef GLU_NEXT_PAIR
}

// 1 when tr1_norm_gemm_skinny(..., glu = 2) can write the SwiGLU output fragment-major (the LDS-streamed <= 16-row form; N % 32: whole 32-column fragments)
extern "C" int tr1_norm_gemm_glu_frag_ok(int64_t M, int64_t N, int64_t K) {
    return M >= 1 && M <= 16 && skinny_lds_stream_k(K) && N % 32 == 0;
}

// The LDS-streamed decode forms (norm_glu_lds_kernel) exist for K = 512 * NST, NST = 7 / 4 / 3 (hidden 3584 / 2048 / 1536): the run-time stage count becomes the
// template argument here.  One LDS size per form, so the cap is dyn itself.
template <int RING, int NRED, int MG, int MODE>
static void launch_norm_glu_lds(int64_t nst, unsigned grid, size_t dyn, hipStream_t s, const void* x, const void* lnw, const void* W, void* out, int64_t M, int64_t N,
                                int64_t K, int64_t ldx, int64_t ldw, int64_t ldc, float eps, int64_t up_off, const void* bias, const QkvEpi& qe, int c_frag) {
    tr1_dispatch<7, 4, 3>((int)nst, [&](auto NST) {
        tr1_launch<norm_glu_lds_kernel<decltype(NST)::value, RING, NRED, MG, MODE>>(dim3(grid), dim3(512), dyn, (int)dyn, s, (const bf16_t*)x, (const bf16_t*)lnw,
                                                                                  (const bf16_t*)W, (bf16_t*)out, (int)M, N, K, ldx, ldw, ldc, eps, up_off,
                                                                                  (const bf16_t*)bias, qe, c_frag);
    });
}

extern "C" int tr1_norm_gemm_skinny(const void* x, const void* lnw, const void* W, const void* bias, void* out, int64_t M, int64_t N, int64_t K,
                                    int64_t ldx, int64_t ldw, int64_t ldc, float eps, int glu, void* stream) {
    TR1_CHECK_ARG(glu >= 0 && glu <= 2, "norm_gemm_skinny: glu must be 0, 1 or 2 (packed gate/up weights: tr1_norm_glu_pk)");
    TR1_CHECK_ARG(K % BK == 0 && K >= BK, "norm_gemm_skinny: K must be a positive multiple of 64");
    TR1_CHECK_ARG(M >= 1 && M <= 64, "norm_gemm_skinny: 1 <= M <= 64 (decode rows)");
    TR1_CHECK_ARG(N % 8 == 0 && ldx % 8 == 0 && ldw % 8 == 0 && ldc % 8 == 0, "norm_gemm_skinny: N%8, ldx%8, ldw%8, ldc%8 required");
    TR1_CHECK_ARG(!glu || !bias, "norm_gemm_skinny: the GLU form takes no bias");
    hipStream_t s = (hipStream_t)stream;
    // N = output columns (glu: the intermediate size I; W then has 2*I rows, gate rows first)
#define NG(WV, UN, MGR, GL)                                                                                                          \
    hipLaunchKernelGGL((norm_gemm_skinny_kernel<WV, UN, MGR, GL>), dim3((unsigned)((N + (GL ? 16 : 32) - 1) / (GL ? 16 : 32))),      \
                       dim3(WV * 64), 0, s, (const bf16_t*)x, (const bf16_t*)lnw, (const bf16_t*)W, (bf16_t*)out, (const bf16_t*)bias, \
                       (int)M, N, K, ldx, ldw, ldc, eps, N)
    // gate/up + SwiGLU at <= 16 rows: UNROLL 2 keeps the kernel at 128 VGPRs = 4 blocks per CU (1024 slots for 1184 blocks); measured 59.2 vs 60.9 us
    const int64_t nst = K / 512;                     // 64-wide stages per wave (8 waves split K)
    constexpr int RING = 3;
    // LDS of the two row-group forms: <= 16 rows = ring of 3 + double reduction buffer + the waves' norm-weight KiB + one x stage each (a ring of 4 with a single
    // buffer and a second barrier per pair measured the same); 17 .. 32 rows = two row groups per wave against the SAME LDS stage, single reduction buffer
    constexpr size_t dyn1 = norm_glu_lds_bytes(RING, 2, 1, true), dyn2 = norm_glu_lds_bytes(RING, 1, 2, false);
    const bool lds_k = skinny_lds_stream_k(K);
    if (!glu && M > 16 && M <= 32 && N >= 65536 && N % 32 == 0 && lds_k) {
        // 17 .. 32 rows (config 4): two row groups per wave against the same LDS stage, single reduction buffer
        const int64_t NPh = N / 32, n_cu = tr1_cu_count();
        launch_norm_glu_lds<RING, 1, 2, 2>(nst, (unsigned)(NPh < n_cu ? NPh : n_cu), dyn2, s, x, lnw, W, out, M, N, K, ldx, ldw, ldc, eps, N / 2, bias, QkvEpi{}, 0);
        TR1_LAUNCH_CHECK();
    }
    if (!glu && M <= 16 && N >= 65536 && N % 32 == 0 && lds_k) {
        // wide plain projection (the lm_head) through the LDS stream: 256 persistent blocks x 8 waves, column pairs (n, n + N/2)
        const int64_t NPh = N / 32, n_cu = tr1_cu_count();
        launch_norm_glu_lds<RING, 2, 1, 2>(nst, (unsigned)(NPh < n_cu ? NPh : n_cu), dyn1, s, x, lnw, W, out, M, N, K, ldx, ldw, ldc, eps, N / 2, bias, QkvEpi{}, 0);
        TR1_LAUNCH_CHECK();
    }
    TR1_CHECK_ARG(glu != 2 || tr1_norm_gemm_glu_frag_ok(M, N, K), "norm_gemm_skinny: glu = 2 (fragment-major SwiGLU output) needs M <= 16 and the LDS-streamed form (tr1_norm_gemm_glu_frag_ok)");
    if (glu && M <= 32 && lds_k && N % 16 == 0) {   // hidden 3584 / 2048 / 1536
        // 17..32 rows (config 4 decodes 2 x 16 rollouts, 132 KB of LDS): 77.4 -> 52.8 us at 32 x 18944 x 3584 (5.1 TB/s of weights) over the register-fragment form.
        const int64_t NP = N / 16, n_cu = tr1_cu_count();
        const unsigned grid = (unsigned)(NP < n_cu ? NP : n_cu);
        if (M <= 16) launch_norm_glu_lds<RING, 2, 1, 0>(nst, grid, dyn1, s, x, lnw, W, out, M, N, K, ldx, ldw, ldc, eps, N, nullptr, QkvEpi{}, glu == 2 ? 1 : 0);
        else launch_norm_glu_lds<RING, 1, 2, 0>(nst, grid, dyn2, s, x, lnw, W, out, M, N, K, ldx, ldw, ldc, eps, N, nullptr, QkvEpi{}, 0);
    }
    else if (glu) { if (M <= 16) NG(4, 2, 1, true); else if (M <= 32) NG(4, 2, 2, true); else NG(4, 2, 4, true); }
    else if (N >= 100000 && M <= 32) {      // lm_head: 4 column groups per block halve the re-reads of x (228 -> ~195 us at M = 16)
#define NG4(UN, MGR)                                                                                                                 \
    hipLaunchKernelGGL((norm_gemm_skinny_kernel<4, UN, MGR, false, 4>), dim3((unsigned)((N + 63) / 64)), dim3(256), 0, s, (const bf16_t*)x,    \
                       (const bf16_t*)lnw, (const bf16_t*)W, (bf16_t*)out, (const bf16_t*)bias, (int)M, N, K, ldx, ldw, ldc, eps, N)
        if (M <= 16) NG4(2, 1); else NG4(2, 2);
#undef NG4
    }
    else     { if (M <= 16) NG(8, 2, 1, false); else if (M <= 32) NG(8, 2, 2, false); else NG(4, 2, 4, false); }   // 8 waves: see tr1_norm_gemm_qkv
#undef NG
    TR1_LAUNCH_CHECK();
}

extern "C" int tr1_norm_gemm_qkv(const void* x, const void* lnw, const void* Wqkv, const void* bias, const void* cosb, const void* sinb, void* q_out,
                                 int64_t ld_q, void* kcache, int64_t k_ld, void* vtcache, int64_t vt_ld, const void* slots, int64_t M, int64_t n_heads,
                                 int64_t n_kv, int64_t head_dim, int64_t K, int64_t ldx, int64_t ldw, float eps, void* stream) {
    TR1_CHECK_ARG(K % BK == 0 && K >= BK, "norm_gemm_qkv: K must be a positive multiple of 64");
    TR1_CHECK_ARG(M >= 1 && M <= 64, "norm_gemm_qkv: 1 <= M <= 64 (decode rows)");
    TR1_CHECK_ARG(head_dim % 32 == 0 && ldx % 8 == 0 && ldw % 8 == 0, "norm_gemm_qkv: head_dim % 32, ldx % 8, ldw % 8 required");
    const int64_t heads = n_heads + 2 * n_kv, N = heads * head_dim;
    QkvEpi qe{(const float*)cosb, (const float*)sinb, (bf16_t*)q_out, ld_q, (bf16_t*)kcache, k_ld, (bf16_t*)vtcache, vt_ld, (const int*)slots,
              (int)n_heads, (int)n_kv, (int)head_dim};
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)(heads * (head_dim / 32)));
    // M <= 16: only heads * hd/32 = 144 blocks (7B) for 256 CUs, so 8 waves per block split K and double the loads in flight per CU
    // (tools/microbench.py fused: 15.8 -> 13.5 us); 17 .. 32 rows likewise 8 waves x UNROLL 2, the same form as tr1_norm_gemm_skinny so the two stay
    // bit-identical (fused QKV at 32 rows: 19.7 -> 18.4 us)
#define NGQ(WV, UN, MGR)                                                                                                              \
    hipLaunchKernelGGL((norm_gemm_skinny_kernel<WV, UN, MGR, false, 2, true>), grid, dim3(WV * 64), 0, s, (const bf16_t*)x, (const bf16_t*)lnw, \
                       (const bf16_t*)Wqkv, (bf16_t*)nullptr, (const bf16_t*)bias, (int)M, N, K, ldx, ldw, (int64_t)0, eps, (int64_t)0, qe)
    // Weights by DMA through per-wave LDS rings (norm_glu_lds_kernel, QKV mode; bit-identical).  Before the x slice was staged by DMA as well the
    // decode step measured 3 547 us with it against 3 472 us for the register-fragment form with x in LDS; with the staged x it is 3 277 against
    // 3 325 us.  Other shapes take the register-fragment kernel (x through LDS where it fits).
    const int64_t nst = K / 512;
    if (M > 16 && M <= 32 && skinny_lds_stream_k(K)) {      // 17 .. 32 rows (config 4): two row groups per wave, ring of 3
        constexpr int RING2 = 3;
        constexpr size_t dyn = norm_glu_lds_bytes(RING2, 1, 2, false);
        launch_norm_glu_lds<RING2, 1, 2, 1>(nst, grid.x, dyn, s, x, lnw, Wqkv, nullptr, M, N, K, ldx, ldw, 0, eps, head_dim / 2, bias, qe, 0);
        TR1_LAUNCH_CHECK();
    }
    if (M <= 16 && skinny_lds_stream_k(K)) {
        constexpr int RING = 4;
        constexpr size_t dyn = norm_glu_lds_bytes(RING, 1, 1, false);      // (ring of 4: the x staging fits without the extra stage area... see XSLOT0)
        launch_norm_glu_lds<RING, 1, 1, 1>(nst, grid.x, dyn, s, x, lnw, Wqkv, nullptr, M, N, K, ldx, ldw, 0, eps, head_dim / 2, bias, qe, 0);
        TR1_LAUNCH_CHECK();
    }
    if (M <= 16 && K / 64 / 8 >= 2 && K * 32 <= 120 * 1024 && (int64_t)M * ldx * 2 < 0x7fffffffLL)
        tr1_launch<norm_gemm_skinny_kernel<8, 2, 1, false, 2, true, true>>(grid, dim3(512), (size_t)(K * 32), 120 * 1024, s, (const bf16_t*)x, (const bf16_t*)lnw,
                                                                           (const bf16_t*)Wqkv, (bf16_t*)nullptr, (const bf16_t*)bias, (int)M, N, K, ldx, ldw, (int64_t)0, eps,
                                                                           (int64_t)0, qe);
    else if (M <= 16) NGQ(8, 2, 1); else if (M <= 32) NGQ(8, 2, 2); else NGQ(4, 2, 4);
#undef NGQ
    TR1_LAUNCH_CHECK();
}

// Launch of the decode-regime kernel (single pass over K; the split-K + fixup form is launched by tr1_gemm_skinny_fixup).
void launch_skinny(const void* A, const void* B, void* C, const void* bias, const void* residual, int64_t M, int64_t N, int64_t K,
                   int64_t lda, int64_t ldb, int64_t ldc, int64_t ldr, int out_f32, int ksplit, hipStream_t s) {
#define SK(WV, UN, NC, MGR)                                                                                                          \
    hipLaunchKernelGGL((gemm_skinny_kernel<WV, UN, NC, MGR>), dim3((unsigned)((N + 16 * NC - 1) / (16 * NC)), (unsigned)ksplit),    \
                       dim3(WV * 64), 0, s, (const bf16_t*)A, (const bf16_t*)B, out_f32 ? nullptr : (bf16_t*)C,                     \
                       out_f32 ? (float*)C : nullptr, (const bf16_t*)bias, (const bf16_t*)residual, (int)M, N, K, lda, ldb, ldc, ldr,   \
                       (float*)nullptr, (int*)nullptr)
    // choices measured on MI355X with tools/microbench.py skinny (non-temporal loads hurt; 8-way in-block split-K pays for long K)
    // (A/B on MI355X, M = 16: gate_up 37888x3584 67.6 -> 56.8 us with NCOL 2; lm_head 152064x3584 247 -> 188 us with NCOL 4;
    //  the 3584x18944 down projection has too few column groups for NCOL > 1 and wants split-K instead)
    const int ncol = N >= 100000 ? 4 : (N >= 4096 && ksplit == 1 ? 2 : 1);
    const bool longk = K / ksplit >= 8192;
    if (M <= 16) {
        if (longk) { if (ncol >= 2 && N >= 16384) SK(8, 2, 2, 1); else SK(8, 4, 1, 1); }
        else if (ncol == 4) SK(4, 2, 4, 1);
        else if (ncol == 2) SK(4, 4, 2, 1);
        else {
            if (ksplit == 1 && K / 64 / 4 >= 4 && K * 32 <= 120 * 1024 && (int64_t)M * lda * 2 < 0x7fffffffLL) {
                tr1_launch<gemm_skinny_kernel<4, 4, 1, 1, true>>(dim3((unsigned)((N + 15) / 16), 1u), dim3(256), (size_t)(K * 32), 120 * 1024, s, (const bf16_t*)A,
                                                                 (const bf16_t*)B, out_f32 ? nullptr : (bf16_t*)C, out_f32 ? (float*)C : nullptr, (const bf16_t*)bias,
                                                                 (const bf16_t*)residual, (int)M, N, K, lda, ldb, ldc, ldr, (float*)nullptr, (int*)nullptr);
            } else SK(4, 4, 1, 1);
        }
    } else if (M <= 32) {       // LDS reduce buffer: WAVES * NCOL * MG * 1088 B <= 64 KB
        if (longk) { if (ncol >= 2 && N >= 16384) SK(8, 2, 2, 2); else SK(8, 2, 1, 2); }
        else if (ncol == 4) SK(4, 2, 4, 2);
        else if (ncol == 2) SK(4, 2, 2, 2);
        else SK(4, 4, 1, 2);
    } else {
        if (longk) SK(8, 2, 1, 4);
        else if (ncol >= 2) SK(4, 2, 2, 4);
        else SK(4, 2, 1, 4);
    }
#undef SK
}

// ------------------------------------------------------------------------------------------------------------------
// LDS-streamed form of the split-K + fixup decode projection (down_proj at M <= 16: N = 3584 columns, K = 18944).
// Same decomposition, workspace and ticket protocol as gemm_skinny_kernel<4, 2, 4, 1> launched by tr1_gemm_skinny_fixup (a block owns 64
// output columns and one of `gridDim.y` K-slabs; the last-arriving slab sums the tiles in slab order), but the 64 x 64 weight stages and
// the 16 x 64 activation stages travel HBM/L2 -> LDS as full 128-byte row runs (global_load_lds), each wave has its own two-slot ring and
// takes the slab's 64-wide stages round-robin, so the only ordering in the stream is the issuing wave's counted vmcnt.
// ------------------------------------------------------------------------------------------------------------------
// NWI = weight DMA instructions (8 rows each) per stage: 8 = 64-column blocks; 7 = 56-column blocks (round 3): 3584 columns are then 64 groups, and
// 64 x 4 K-slabs fill all 256 CUs (56 x 4 = 224 left 32 of them idle).  The MFMAs still run on four 16-row weight tiles - rows 56..63 of a stage are
// never written and only feed the eight output columns that are not stored - so every stored value is the same sum in the same order as with NWI = 8.
TR1_STAMP_PROBE(tr1_down_probe, probe_down_set_ptr)      // thread 0 of every block (tools/mall_probe2.py)
#define DOWN_STAMP(i) TR1_STAMP(true, i)
#define DOWN_DUMP() TR1_STAMP_DUMP(tr1_down_probe, threadIdx.x == 0, (int64_t)blockIdx.y * gridDim.x + blockIdx.x)
template <int WAVES, int MG = 1, int NWI = 8>
__global__ __launch_bounds__(WAVES * 64) void gemm_skinny_lds_fix_kernel(const bf16_t* __restrict__ X, const bf16_t* __restrict__ W, bf16_t* __restrict__ C,
                                                                         const bf16_t* __restrict__ bias, const bf16_t* __restrict__ residual, int M,
                                                                         int64_t N, int64_t K, int64_t ldx, int64_t ldw, int64_t ldc, int64_t ldr,
                                                                         float* __restrict__ fix_ws, int* __restrict__ fix_cnt) {
    constexpr int NC = 4, XOFF = NWI * 1024, STAGE = XOFF + MG * 2048;      // NWI * 8 weight rows + 16*MG activation rows, 128 bytes each (56-column stages: the MFMA's
                                                                            // weight rows 56..63 read into the activation area - they feed output columns that are never stored)
    constexpr int TILE = NC * MG * 256;
    extern __shared__ __attribute__((aligned(16))) char sk_lds[];           // [WAVES][2][STAGE]; afterwards red[WAVES][NC][MG][16][17] f32; ticket at the end
    int* s_ticket = reinterpret_cast<int*>(sk_lds + WAVES * 2 * STAGE);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, u = lane & 15, g = lane >> 4;
    TR1_STAMPS;
    DOWN_STAMP(0);
    constexpr int COLS = NWI * 8;                                           // output columns a block owns
    const int64_t n0 = (int64_t)blockIdx.x * COLS;
    const int64_t kslab = K / gridDim.y, k0 = (int64_t)blockIdx.y * kslab;
    const int nst = (int)(kslab / 64);
    const int n_my = wave < nst ? (nst - wave + WAVES - 1) / WAVES : 0;       // stages wave, wave + WAVES, ...
    char* ring = sk_lds + wave * 2 * STAGE;
    // DMA lane map (8 rows x 128 bytes per instruction): lane -> row 8j + (lane >> 3), physical chunk lane & 7, logical chunk ^ keyA(row)
    const bf16_t* pw[NWI]; const bf16_t* px[2 * MG];
#pragma unroll
    for (int j = 0; j < NWI; ++j) {
        const int r = 8 * j + (lane >> 3);
        int64_t row = n0 + r; if (row >= N) row = N - 1;
        pw[j] = W + row * ldw + k0 + (int64_t)wave * 64 + (((lane & 7) ^ keyA(r)) << 3);
    }
#pragma unroll
    for (int j = 0; j < 2 * MG; ++j) {
        const int r = 8 * j + (lane >> 3);
        px[j] = X + (int64_t)(r < M ? r : M - 1) * ldx + k0 + (int64_t)wave * 64 + (((lane & 7) ^ keyA(r)) << 3);
    }
#define SKL_ISSUE(SLOT) do {                                                                                              \
        char* dst__ = ring + (SLOT) * STAGE;                                                                              \
        _Pragma("unroll") for (int j = 0; j < NWI; ++j) { __builtin_amdgcn_global_load_lds((gptr_t)pw[j], (lptr_t)(dst__ + j * 1024), 16, 0, TR1_W_AUX); pw[j] += WAVES * 64; } \
        _Pragma("unroll") for (int j = 0; j < 2 * MG; ++j) { __builtin_amdgcn_global_load_lds((gptr_t)px[j], (lptr_t)(dst__ + XOFF + j * 1024), 16, 0, 0); px[j] += WAVES * 64; } \
    } while (0)
    f32x4_t acc[NC][MG][2];
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int mg = 0; mg < MG; ++mg) acc[c][mg][0] = acc[c][mg][1] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    const int rd_w = u * 128, kA = keyA(u);
#define SKL_CONSUME(SLOT) do {                                                                                            \
        const char* sb__ = ring + (SLOT) * STAGE;                                                                         \
        bf16x8_t xf__[MG][2], wf__[NC][2];                                                                                \
        _Pragma("unroll") for (int ks = 0; ks < 2; ++ks) {                                                                \
            const int off__ = ((ks * 4 + g) ^ kA) << 4;                                                                   \
            _Pragma("unroll") for (int mg = 0; mg < MG; ++mg) xf__[mg][ks] = *reinterpret_cast<const bf16x8_t*>(sb__ + XOFF + mg * 2048 + rd_w + off__); \
            _Pragma("unroll") for (int c = 0; c < NC; ++c) wf__[c][ks] = *reinterpret_cast<const bf16x8_t*>(sb__ + c * 2048 + rd_w + off__); \
        }                                                                                                                 \
        _Pragma("unroll") for (int ks = 0; ks < 2; ++ks)                                                                  \
        _Pragma("unroll") for (int c = 0; c < NC; ++c)                                                                    \
        _Pragma("unroll") for (int mg = 0; mg < MG; ++mg)                                                                 \
            acc[c][mg][ks] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf__[c][ks], xf__[mg][ks], acc[c][mg][ks], 0, 0, 0); \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                                                \
    } while (0)
    if (n_my > 0) SKL_ISSUE(0);
    for (int i = 0; i < n_my; i += 2) {
        if (i + 1 < n_my) { SKL_ISSUE(1); asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NWI + 2 * MG) : "memory"); } else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        SKL_CONSUME(0);
        if (i + 1 < n_my) {
            if (i + 2 < n_my) { SKL_ISSUE(0); asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NWI + 2 * MG) : "memory"); } else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            SKL_CONSUME(1);
        }
    }
#undef SKL_ISSUE
#undef SKL_CONSUME
    DOWN_STAMP(1);
    TR1_BARRIER();
    DOWN_STAMP(2);                                                          // every wave is done with its ring: the space becomes the reduction buffer
    float* red = reinterpret_cast<float*>(sk_lds);                          // [WAVES][NC][MG][16][17]
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int mg = 0; mg < MG; ++mg)
#pragma unroll
            for (int r = 0; r < 4; ++r) red[(((wave * NC + c) * MG + mg) * 16 + u) * 17 + g * 4 + r] = acc[c][mg][0][r] + acc[c][mg][1][r];
    __syncthreads();
    // ---- cross-block fixup: park the tile, draw a ticket, the last slab sums in slab order
    SKINNY_SPLITK_FIXUP(TILE, WAVES * 64, MG, true, red[(((w * NC + c) * MG + mg) * 16 + mm) * 17 + nn], *s_ticket, DOWN_STAMP(3), DOWN_STAMP(4), DOWN_DUMP(); return, {
        const int m = mg * 16 + mm;
        const int64_t n = n0 + c * 16 + nn;
        if (m < M && n < N && c * 16 + nn < COLS) {
            if (bias) v += bf2f(bias[n]);
            if (residual) v += bf2f(residual[(int64_t)m * ldr + n]);
            C[(int64_t)m * ldc + n] = f2bf(v);
        }
    });
    DOWN_STAMP(5);
    DOWN_DUMP();
}

// ---- narrow-N decode projections (o_proj, down_proj): cross-block split-K with in-kernel fixup -----------------------------------
// N/16 column groups cannot fill 256 CUs and every block re-reads all of x from L2; 4 k-slabs x wider column groups (NCOL 2-4) cut
// the x traffic and put ~4x more blocks in flight.  Measured at M = 16 (tools/microbench.py splitk): down 3584x18944 38.5 -> 29 us.
static int skinny_fix_cfg(int64_t M, int64_t N, int64_t K, int* ncol, int* mg) {
    *mg = M <= 16 ? 1 : (M <= 32 ? 2 : 4);
    *ncol = (K >= 8192 && *mg <= 2) ? 4 : 2;
    int ks = K >= 2048 ? 4 : 1;
    // Few column groups (a narrow output over a long K - the Qwen2-VL-2B down projection: 1536 / 64 = 24 groups x 4 slabs = 96 blocks on 256 CUs, 2.1 TB/s): as
    // many K slabs (<= 16, whole 64-k stages each) as still give at most one block per CU - 24 x 10 = 240 blocks there.
    const int64_t groups = (N + 16 * *ncol - 1) / (16 * *ncol);
    if (ks == 4 && *mg == 1 && groups * 4 < 192)
        for (int cand = 5; cand <= 16; ++cand)
            if (K % ((int64_t)cand * 64) == 0 && groups * cand <= 256) ks = cand;
    return ks;
}

// 56-column blocks for the LDS-streamed <= 16-row form when that is what fills the chip: N % 56 == 0 and N/56 x ks <= 256 < more blocks than N/64 x ks
// (7B down projection: 64 x 4 = 256 blocks instead of 56 x 4 = 224).
static bool skinny_fix_cols56(int64_t N, int ks, int ncol, int mg) {
    return mg <= 2 && ncol == 4 && ks > 1 && N % 56 == 0 && (N / 56) * ks <= 256 && (N / 56) > (N + 63) / 64;
}

extern "C" int64_t tr1_gemm_skinny_fixup_workspace_floats(int64_t M, int64_t N, int64_t K) {
    // fp32 tiles [ksplit][column groups][NCOL*MG*256] followed by one int32 ticket counter per column group (zero-initialised ONCE by
    // the caller; the kernel re-arms them)
    int ncol, mg;
    const int ks = skinny_fix_cfg(M, N, K, &ncol, &mg);
    int64_t groups = (N + 16 * ncol - 1) / (16 * ncol);
    if (skinny_fix_cols56(N, ks, ncol, mg)) groups = N / 56;
    return ks * groups * ncol * mg * 256 + groups;
}

extern "C" int tr1_gemm_skinny_fixup(const void* A, const void* B, void* C, const void* bias, const void* residual, int64_t M, int64_t N, int64_t K,
                                     int64_t lda, int64_t ldb, int64_t ldc, int64_t ldr, void* ws_f32, int64_t ws_floats, void* stream) {
    TR1_CHECK_ARG(K % BK == 0 && K >= 256, "gemm_skinny_fixup: K must be a multiple of 64 and >= 256");
    TR1_CHECK_ARG(M >= 1 && M <= 64, "gemm_skinny_fixup: 1 <= M <= 64 (decode rows)");
    TR1_CHECK_ARG(N % 8 == 0 && lda % 8 == 0 && ldb % 8 == 0 && ldc % 8 == 0 && (!residual || ldr % 8 == 0), "gemm_skinny_fixup: N%8, ld%8 required");
    int ncol, mg;
    const int ks = skinny_fix_cfg(M, N, K, &ncol, &mg);
    TR1_CHECK_ARG(ks <= 16, "gemm_skinny_fixup: at most 16 K slabs (the fixup sums them fully in flight)");
    const bool c56 = (K / ks) % 64 == 0 && skinny_fix_cols56(N, ks, ncol, mg);
    const int64_t groups = c56 ? N / 56 : (N + 16 * ncol - 1) / (16 * ncol);
    TR1_CHECK_ARG(ws_f32 && ws_floats >= ks * groups * ncol * mg * 256 + groups, "gemm_skinny_fixup: workspace too small");
    float* tiles = (float*)ws_f32;
    int* cnt = (int*)(tiles + ks * groups * ncol * mg * 256);
    hipStream_t s = (hipStream_t)stream;
#define SKF(WV, UN, NC, MGR)                                                                                                         \
    hipLaunchKernelGGL((gemm_skinny_kernel<WV, UN, NC, MGR>), dim3((unsigned)groups, (unsigned)ks), dim3(WV * 64), 0, s,            \
                       (const bf16_t*)A, (const bf16_t*)B, (bf16_t*)C, (float*)nullptr, (const bf16_t*)bias, (const bf16_t*)residual, \
                       (int)M, N, K, lda, ldb, ldc, ldr, tiles, ks > 1 ? cnt : (int*)nullptr)
    // the LDS-streamed forms (WV waves, MGR row groups, NWI * 8 weight rows per stage; one LDS size each)
#define SKL(WV, MGR, NWI, DYN)                                                                                                                \
    tr1_launch<gemm_skinny_lds_fix_kernel<WV, MGR, NWI>>(dim3((unsigned)groups, (unsigned)ks), dim3(WV * 64), DYN, DYN, s, (const bf16_t*)A, (const bf16_t*)B, \
                                                         (bf16_t*)C, (const bf16_t*)bias, (const bf16_t*)residual, (int)M, N, K, lda, ldb, ldc, ldr, tiles, cnt)
    if (c56 && mg == 2) SKL(7, 2, 7, 7 * 2 * (7 * 1024 + 2 * 2048) + 16);       // round 5, 17 .. 32 rows: 56-column blocks as well (256 blocks), whose 11 KiB stages leave room for a seventh wave
    else if (mg == 2 && ncol == 4 && ks > 1 && (K / ks) % 64 == 0 && N % 64 == 0) SKL(6, 2, 8, 6 * 2 * 12288 + 16);       // 17 .. 32 rows: 12 KiB stages, 6 waves
    else if (c56) SKL(7, 1, 7, 7 * 2 * (7 * 1024 + 2048) + 16);
    else if (mg == 1 && ncol == 4 && ks > 1 && (K / ks) % 64 == 0 && N % 64 == 0) SKL(7, 1, 8, 7 * 2 * 10240 + 16);       // <= 16 rows: 10 KiB stages, 7 waves
    else if (mg == 1) { if (ncol == 4) SKF(4, 2, 4, 1); else SKF(4, 4, 2, 1); }
    else if (mg == 2) { if (ncol == 4) SKF(4, 2, 4, 2); else SKF(4, 2, 2, 2); }
    else SKF(4, 2, 2, 4);
#undef SKL
#undef SKF
    TR1_LAUNCH_CHECK();
}
