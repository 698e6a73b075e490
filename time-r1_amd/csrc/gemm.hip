// bf16 GEMM for gfx950 (CDNA4): C[M,N] = A[M,K] * B[N,K]^T (+ bias[N]) (+ residual[M,N]), fp32 accumulate on MFMA.
//
// This is the projection workhorse behind every Linear in the GRPO path (reference call sites: the cuBLAS GEMMs under
// transformers/models/qwen2_vl/modeling_qwen2_vl.py:501-504 (q/k/v/o), :459-466 (MLP), :251-274 (patch embed as GEMM),
// :277-290 (patch merger), :1323 (lm_head)).  Both operands are K-contiguous ("NT"), which is what nn.Linear stores.
//
// Design (MI355X-first, see /opt/skills/guides/cdna_hip_programming.md section 5):
//   * 128x128x64 block tile, 256 threads = 4 waves (2x2), each wave owns 64x64 = 4x4 v_mfma_f32_16x16x32_bf16 tiles.
//   * operands go HBM -> LDS directly with global_load_lds_dwordx4 (no VGPR round trip), two LDS buffers,
//     one __syncthreads per K-tile (the barrier's vmcnt(0) retires the DMA issued one iteration earlier).
//   * the LDS image is lane-linear per DMA instruction, so the bank-conflict swizzle is applied on the SOURCE
//     address (which 16-byte chunk of the 128-byte row a lane fetches) and mirrored on the ds_read_b128 side.
//   * the MFMA is issued with the weight tile as the A operand and the activation tile as the B operand, with the
//     16 weight rows of tile j permuted so that every lane ends up owning 16 CONTIGUOUS output columns of one output
//     row: the epilogue is two 16-byte bf16 stores (or four fp32 ones) per row, no LDS transpose.
//   * 1-D grid with an XCD-aware, M-grouped tile order so the 32 blocks resident on one XCD share B panels in its L2.
// The decode-row ("skinny") family, M <= 64, lives in gemm_skinny.hip; tr1_gemm_nt_bf16 routes small M to its launch_skinny.
#include "skinny_common.h"      // launch_skinny (tr1_common.h comes with it: gptr_t / lptr_t, keyA, TR1_BARRIER)
#include <stdlib.h>

#define BM 128
#define BN 128
#define BK 64
#define TILE_BYTES (BM * BK * 2)  // 16 KiB per operand per buffer

TR1_DEV bf16x8_t zero_frag8() { u32x4_t w = {0, 0, 0, 0}; return __builtin_bit_cast(bf16x8_t, w); }
TR1_DEV int keyB(int row) { return (((row >> 4) & 3) << 1) | ((row >> 1) & 1); }

// Stage one 128x64 bf16 tile: 16 wave-instructions of 1 KiB, 4 per wave. Rows beyond `rows_valid` are clamped
// (their products land in rows/cols that are never stored).
template <bool IS_B>
TR1_DEV void stage_tile(const bf16_t* __restrict__ g, int64_t ld, int64_t row0, int64_t rows_valid, int64_t k0, char* lds_tile,
                        int wave, int lane) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int inst = wave * 4 + i;
        const int row = inst * 8 + (lane >> 3);
        const int phys = lane & 7;
        const int logical = phys ^ (IS_B ? keyB(row) : keyA(row));
        int64_t grow = row0 + row;
        if (grow >= rows_valid) grow = rows_valid - 1;
        const bf16_t* src = g + grow * ld + k0 + logical * 8;
        __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(lds_tile + inst * 1024), 16, 0, 0);
    }
}

template <bool OUT_F32, bool ACCUM>
__global__ __launch_bounds__(256, 2) void gemm_nt_kernel(const bf16_t* __restrict__ A, const bf16_t* __restrict__ B, void* __restrict__ Cv,
                                                         const bf16_t* __restrict__ bias, const bf16_t* __restrict__ residual,
                                                         int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc,
                                                         int64_t ldr, int tiles_m, int tiles_n) {
    __shared__ __attribute__((aligned(16))) char smem[4 * TILE_BYTES];  // [buf][A|B]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;

    // ---- XCD-aware tile order: block b runs on XCD b%8; give each XCD a contiguous run of the grouped order.
    const int nwg = tiles_m * tiles_n;
    int wgid;
    {
        const int b = blockIdx.x, xcd = b & 7, q = nwg >> 3, r = nwg & 7;
        wgid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (b >> 3);
    }
    const int GROUP_M = 8;
    const int group = wgid / (GROUP_M * tiles_n);
    const int first_m = group * GROUP_M;
    const int gsz = min(tiles_m - first_m, GROUP_M);
    const int in_group = wgid - group * GROUP_M * tiles_n;
    const int tm = first_m + in_group % gsz;
    const int tn = in_group / gsz;
    const int64_t m0 = (int64_t)tm * BM, n0 = (int64_t)tn * BN;

    f32x4_t acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

    const int nk = (int)(K / BK);
    stage_tile<false>(A, lda, m0, M, 0, smem, wave, lane);
    stage_tile<true>(B, ldb, n0, N, 0, smem + TILE_BYTES, wave, lane);

    const int u = lane & 15, g = lane >> 4;
    for (int kt = 0; kt < nk; ++kt) {
        __syncthreads();  // retires this wave's DMA for tile kt (vmcnt(0)) and orders it against every reader
        char* curA = smem + (kt & 1) * 2 * TILE_BYTES;
        char* curB = curA + TILE_BYTES;
        if (kt + 1 < nk) {
            char* nxtA = smem + ((kt + 1) & 1) * 2 * TILE_BYTES;
            stage_tile<false>(A, lda, m0, M, (int64_t)(kt + 1) * BK, nxtA, wave, lane);
            stage_tile<true>(B, ldb, n0, N, (int64_t)(kt + 1) * BK, nxtA + TILE_BYTES, wave, lane);
        }
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8_t xa[4], wb[4];
            const int chunk = ks * 4 + g;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = wm * 64 + i * 16 + u;
                xa[i] = *reinterpret_cast<const bf16x8_t*>(curA + row * 128 + ((chunk ^ keyA(row)) << 4));
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int row = wn * 64 + (u >> 2) * 16 + j * 4 + (u & 3);
                wb[j] = *reinterpret_cast<const bf16x8_t*>(curB + row * 128 + ((chunk ^ keyB(row)) << 4));
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wb[j], xa[i], acc[i][j], 0, 0, 0);
        }
    }

    // ---- epilogue: lane owns, for each i, row m = m0 + wm*64 + i*16 + u and columns n0 + wn*64 + g*16 + [0,16)
    const int64_t nbase = n0 + wn * 64 + g * 16;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t m = m0 + wm * 64 + i * 16 + u;
        if (m >= M) continue;
#pragma unroll
        for (int h = 0; h < 2; ++h) {  // two 8-column halves
            const int64_t n = nbase + h * 8;
            if (n + 8 > N) continue;
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = acc[i][h * 2 + (e >> 2)][e & 3];
            if (bias) {
                const u32x4_t bv = *reinterpret_cast<const u32x4_t*>(bias + n);
#pragma unroll
                for (int e = 0; e < 4; ++e) { v[2 * e] += bflo(bv[e]); v[2 * e + 1] += bfhi(bv[e]); }
            }
            if (residual) {
                const u32x4_t rv = *reinterpret_cast<const u32x4_t*>(residual + m * ldr + n);
#pragma unroll
                for (int e = 0; e < 4; ++e) { v[2 * e] += bflo(rv[e]); v[2 * e + 1] += bfhi(rv[e]); }
            }
            if (OUT_F32) {
                float* cp = reinterpret_cast<float*>(Cv) + m * ldc + n;
                f32x4_t o0 = {v[0], v[1], v[2], v[3]}, o1 = {v[4], v[5], v[6], v[7]};
                if (ACCUM) {
                    const f32x4_t p0 = *reinterpret_cast<const f32x4_t*>(cp), p1 = *reinterpret_cast<const f32x4_t*>(cp + 4);
                    o0 += p0; o1 += p1;
                }
                *reinterpret_cast<f32x4_t*>(cp) = o0;
                *reinterpret_cast<f32x4_t*>(cp + 4) = o1;
            } else {
                bf16_t* cp = reinterpret_cast<bf16_t*>(Cv) + m * ldc + n;
                u32x4_t o;
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = pack2bf(v[2 * e], v[2 * e + 1]);
                *reinterpret_cast<u32x4_t*>(cp) = o;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------
// 256x256x64 variant for large outputs: 512 threads = 8 waves (2 x 4), each wave owns 128x64 = 8x4 MFMA tiles, so every
// ds_read_b128 feeds more MFMAs (12 fragment reads per 32 MFMAs instead of 16) and the HBM/L2 traffic per FLOP halves.
// Same staging / swizzle / epilogue scheme as gemm_nt_kernel; 128 KiB of LDS (two buffers), one block per CU.
// ------------------------------------------------------------------------------------------------------------------
#define BN2 256
#define TILE2_BYTES (BN2 * BK * 2)  // 32 KiB: the B operand tile (and the A tile of the 256-row form)

// RT = 16-row MFMA tiles per wave along M: 7 / 8 / 9 / 10 -> 224 / 256 / 288 / 320 x 256 block.  The 288-row form exists for the M = 5074 (P + G*C)
// GEMMs with N = 3584: 18 x 14 = 252 blocks fill the 256 CUs in ONE round at 98 % padding efficiency, where 256 x 256 needs two rounds
// (280 blocks) and 128 x 128 three (1120 blocks on 512 slots).
// Epilogue of the phased 8-wave forms THROUGH LDS.  Stored straight from the accumulator layout, an instruction writes 64 separate
// 16-byte pieces (16 rows x 4 pieces at 64-byte stride for fp32): every 128-byte line is visited by 4-8 instructions, and the fp32
// read-modify-write of a weight gradient ran at 2.3 TB/s (904 against 1297 TFLOP/s for the same shape with bf16 output).  Here each wave
// parks CH of its 16-row accumulator tiles in its own slice of the (now dead) operand buffers - 256-byte rows, 16-byte chunks XOR-swizzled
// with the row so both directions are bank-conflict free - and reads them back row-contiguous: an instruction then covers 4 full fp32 rows
// (8 bf16 rows) of the wave's 64 columns, i.e. only whole lines.  Values and rounding are unchanged.
// EPI = 1 ("lm_head -> log-prob / entropy"): nothing is stored to C.  The wave's 64 columns of a row are rounded to bf16 (the logits the
// reference materialises are bf16) and reduced to the online-softmax triple (max, sum e^(x-max), sum x e^(x-max)); lane c8 = 0 of a row writes it to
// part[row][ncol0 / 64] (Cv = float4 partials, ldc = column blocks per row, +1 slot per row for the target's logit), and the lane that holds
// column targets[row] writes that logit to slot ldc - 1.  `bias` carries the int32 targets.  The [R, V] logits never exist in HBM.
template <bool OUT_F32, bool ACCUM, int RT, int EPI = 0>
TR1_DEV void store_acc256_lds(const f32x4_t (&acc)[RT][4], char* __restrict__ wave_lds, void* __restrict__ Cv, const bf16_t* __restrict__ bias,
                              const bf16_t* __restrict__ residual, int64_t M, int64_t N, int64_t ldc, int64_t ldr, int64_t mrow0, int64_t ncol0,
                              int lane, float* __restrict__ sumsq_slot = nullptr, bf16_t* __restrict__ wire16 = nullptr, int64_t ldw16 = 0) {
    // wire16 (fp32 output only): the value stored is ALSO written, rounded to bf16, at the same (row, column) of a second matrix - the gradient exchange's
    // wire-format copy of a weight gradient, taken from the epilogue that produces the final fp32 value instead of a 6-byte-per-parameter staging pass
    constexpr int CH = (RT % 2 == 0) ? 4 : 3;                             // 16-row tiles per pass: 8 waves x CH x 4 KiB fit the operand buffers
    const int u = lane & 15, g = lane >> 4;
    float ssq = 0.f;                                                      // fp32 output only: sum of squares of what this wave stores (gradient norm)
#pragma unroll
    for (int i0 = 0; i0 < RT; i0 += CH) {
        const int cnt = RT - i0 < CH ? RT - i0 : CH;
#pragma unroll
        for (int ii = 0; ii < CH; ++ii) {
            if (ii < cnt) {
                const int row = ii * 16 + u;
#pragma unroll
                for (int j = 0; j < 4; ++j) *reinterpret_cast<f32x4_t*>(wave_lds + row * 256 + (((g * 4 + j) ^ u) << 4)) = acc[i0 + ii][j];
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (OUT_F32) {
            const int c = lane & 15;
            const int64_t n = ncol0 + c * 4;
#pragma unroll
            for (int r4 = 0; r4 < CH * 4; ++r4) {
                if (r4 < cnt * 4) {
                    const int rr = r4 * 4 + (lane >> 4);
                    f32x4_t v = *reinterpret_cast<const f32x4_t*>(wave_lds + rr * 256 + ((c ^ (rr & 15)) << 4));
                    const int64_t m = mrow0 + i0 * 16 + rr;
                    if (m < M && n + 4 <= N) {
                        if (bias) { const u32x2_t bv = *reinterpret_cast<const u32x2_t*>(bias + n); v[0] += bflo(bv[0]); v[1] += bfhi(bv[0]); v[2] += bflo(bv[1]); v[3] += bfhi(bv[1]); }
                        if (residual) {
                            const u32x2_t rv = *reinterpret_cast<const u32x2_t*>(residual + m * ldr + n);
                            v[0] += bflo(rv[0]); v[1] += bfhi(rv[0]); v[2] += bflo(rv[1]); v[3] += bfhi(rv[1]);
                        }
                        float* cp = reinterpret_cast<float*>(Cv) + m * ldc + n;
                        if (ACCUM) v += *reinterpret_cast<const f32x4_t*>(cp);
                        *reinterpret_cast<f32x4_t*>(cp) = v;      // (non-temporal C stores measured: -0.55 us per round of tiles in a probe, nothing in the step)
                        if (wire16) *reinterpret_cast<u32x2_t*>(wire16 + m * ldw16 + n) = (u32x2_t){pack2bf(v[0], v[1]), pack2bf(v[2], v[3])};
                        ssq += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
                    }
                }
            }
        } else {
            const int c8 = lane & 7;
            const int64_t n = ncol0 + c8 * 8;
            u32x4_t bv = {0, 0, 0, 0};
            if (EPI != 1 && bias && n + 8 <= N) bv = *reinterpret_cast<const u32x4_t*>(bias + n);      // (EPI 1: `bias` carries the int32 targets)
#pragma unroll
            for (int r8 = 0; r8 < CH * 2; ++r8) {
                if (r8 < cnt * 2) {
                    const int rr = r8 * 8 + (lane >> 3);
                    const f32x4_t v0 = *reinterpret_cast<const f32x4_t*>(wave_lds + rr * 256 + (((2 * c8) ^ (rr & 15)) << 4));
                    const f32x4_t v1 = *reinterpret_cast<const f32x4_t*>(wave_lds + rr * 256 + (((2 * c8 + 1) ^ (rr & 15)) << 4));
                    float v[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
                    const int64_t m = mrow0 + i0 * 16 + rr;
                    if (EPI == 1) {
                        const bool ok = m < M && n + 8 <= N;
                        const int tg = m < M ? reinterpret_cast<const int*>(bias)[m] : -1;
                        float mx = -INFINITY;
#pragma unroll
                        for (int e = 0; e < 8; ++e) { v[e] = ok ? bf2f(f2bf(v[e])) : -INFINITY; mx = fmaxf(mx, v[e]); }
                        mx = fmaxf(mx, __shfl_xor(mx, 1, 64)); mx = fmaxf(mx, __shfl_xor(mx, 2, 64)); mx = fmaxf(mx, __shfl_xor(mx, 4, 64));
                        const float ms = (mx == -INFINITY) ? 0.f : mx;
                        float se = 0.f, te = 0.f;
#pragma unroll
                        for (int e = 0; e < 8; ++e) {
                            const float ex = __expf(v[e] - ms);               // exp(-inf) = 0 for masked columns
                            se += ex; te += (v[e] == -INFINITY) ? 0.f : v[e] * ex;
                        }
                        se += __shfl_xor(se, 1, 64); se += __shfl_xor(se, 2, 64); se += __shfl_xor(se, 4, 64);
                        te += __shfl_xor(te, 1, 64); te += __shfl_xor(te, 2, 64); te += __shfl_xor(te, 4, 64);
                        if (m < M) {
                            f32x4_t* prow = reinterpret_cast<f32x4_t*>(Cv) + m * ldc;
                            if (c8 == 0 && ncol0 < N) prow[ncol0 >> 6] = (f32x4_t){mx, se, te, 0.f};   // a wave's 64-column slice past N (N % 256 != 0) has no slot:
                            //                                                                            slot N/64 is the target logit, N/64 + 1 the next row
                            if (ok && tg >= n && tg < n + 8) reinterpret_cast<float*>(prow + (ldc - 1))[0] = v[tg - n];
                        }
                        continue;
                    }
                    if (m < M && n + 8 <= N) {
                        if (bias) {
#pragma unroll
                            for (int e = 0; e < 4; ++e) { v[2 * e] += bflo(bv[e]); v[2 * e + 1] += bfhi(bv[e]); }
                        }
                        if (residual) {
                            const u32x4_t rv = *reinterpret_cast<const u32x4_t*>(residual + m * ldr + n);
#pragma unroll
                            for (int e = 0; e < 4; ++e) { v[2 * e] += bflo(rv[e]); v[2 * e + 1] += bfhi(rv[e]); }
                        }
                        if (EPI == 5) {      // QuickGELU (Qwen2-VL vision MLP, TF:300-301) on the bf16-rounded projection, as act_kernel<1> after the GEMM
#pragma unroll
                            for (int e = 0; e < 8; ++e) { const float x = bf2f(f2bf(v[e])); v[e] = x / (1.f + __expf(-1.702f * x)); }
                        }
                        u32x4_t o;
#pragma unroll
                        for (int e = 0; e < 4; ++e) o[e] = pack2bf(v[2 * e], v[2 * e + 1]);
                        *reinterpret_cast<u32x4_t*>(reinterpret_cast<bf16_t*>(Cv) + m * ldc + n) = o;
                    }
                }
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                 // the next pass overwrites the slice
    }
    if (OUT_F32 && sumsq_slot) {      // the FINAL value of every gradient element passes through this epilogue in the window's last micro-step: its
#pragma unroll                        // squared norm costs a few FMAs here instead of a 30 GB read of the arena (sumsq_kernel) before AdamW
        for (int o = 32; o >= 1; o >>= 1) ssq += __shfl_xor(ssq, o, 64);
        if (lane == 0) *sumsq_slot = ssq;
    }
}

TR1_DEV float epi_silu(float x) { return x / (1.f + __expf(-x)); }

// ------------------------------------------------------------------------------------------------------------------
// Phased ("ping-pong") form of the 8-wave kernel (the 256-column tiles described above).  The K loop is cut into 4 phases per 64-wide
// K-tile and the two wave groups (wm = 0 / 1: the two waves
// that share a SIMD) run one barrier apart, so while one wave of a SIMD issues its MFMAs the other one reads its next fragments
// from LDS and issues the HBM->LDS DMA for the tiles ahead - the matrix pipe never waits for LDS.
//   phase q of tile t:  [ds_read the A fragments of M-quarter q (phase 0: also all B fragments);  issue this phase's DMA rounds;
//                        s_waitcnt lgkmcnt(0)]  s_barrier  [MFMA quarter q x all 4 N fragments x 2 k-steps]  s_barrier
//   DMA schedule (one "round" = 8 KiB = 64 rows, one global_load_lds per thread; every wave issues the same number of rounds so
//   the counted vmcnt below means the same thing in every wave):
//       phases 0, 1 of tile t: the A rounds of tile t+1   (that buffer's A region was last read in phase 3 of tile t-1)
//       phases 2, 3 of tile t: the 4 B rounds of tile t+2 (tile t's B region is only read in phase 0)
//   phase 3 waits vmcnt(4) (the B rounds of t+2 stay in flight) BEFORE its first barrier; tile t+1 is first read one phase later.
//   Every ds_read is retired (lgkmcnt(0)) before the barrier that ends its load section, so a region may be restaged from the next
//   barrier interval on.  A tiles whose row count is not a multiple of 64 send the surplus half round to a 4 KiB junk area.
// ------------------------------------------------------------------------------------------------------------------

// K-major ("NN") B operand: B is [K, N] row-major (the weight itself in dX = dY * W).  A round stages 16 k-rows x 256 columns (512 bytes
// per row, two rows per wave instruction); row r keeps its logical 16-byte chunk c at position c ^ keyKM(r), and the MFMA fragments are read
// back TRANSPOSED with ds_read_b64_tr_b16 (a 16-lane group reads a 4 x 16 block, each lane supplying an 8-byte address and receiving one
// column), so no W^T copy is ever built.  With 512-byte rows eight k-rows of a half-wave share their banks; the key spreads them over the
// four translates a 16-byte-granular swizzle can reach (2-way conflicts on these reads, 8 of the 24 fragment reads of a tile).
TR1_DEV int keyKM(int krow) { return (krow & 1) | ((krow & 2) << 2); }
TR1_DEV void stage_round_km(const bf16_t* __restrict__ g, int64_t ld, int64_t n0, int64_t n_valid, int64_t k0, int64_t k_valid, char* lds_region,
                            int round, int wave, int lane) {
    const int inst = round * 8 + wave;                                   // 2 k-rows (1 KiB) per wave-instruction
    const int krow = inst * 2 + (lane >> 5);
    const int logical = (lane & 31) ^ keyKM(krow);
    int64_t col = n0 + logical * 8;
    if (col + 8 > n_valid) col = n_valid - 8;                            // columns past N: any valid chunk (their outputs are never stored)
    int64_t kr = k0 + krow;
    if (kr >= k_valid) kr = k_valid - 1;                                 // k rows past the operand (weight gradient: the token count is not a multiple
    //                                                                      of 64): re-read the last row - the A side carries zeros there
    __builtin_amdgcn_global_load_lds((gptr_t)(g + kr * ld + col), (lptr_t)(lds_region + inst * 1024), 16, 0, 0);
}

// Fused-epilogue forms of the phased NT kernel (EPI template argument of gemm_nt8p_kernel); extra operands travel in GemmEpi.
//   EPI 2 "gate/up + SwiGLU" (training / prefill / reference forward; TF:459-466 act_fn(gate_proj(x)) * up_proj(x)): B = [2I, K] (gate rows then up
//         rows).  A block's 256 B-tile rows are 4 x (32 gate rows | the 32 up rows of the SAME intermediate columns), so every wave holds both
//         halves of 32 columns and the epilogue writes a = silu(g) * u [M, I] (C) and, when the backward needs it, gu (ep.p0) from the same tile.
//   EPI 3 "down-projection dgrad + SwiGLU backward" (K-major form): C = dgu [M, 2I] = [da * u * silu'(g) | da * silu(g)] with gu read in the epilogue.
//   EPI 4 "q/k/v projection + bias + M-RoPE" (TF:501-504, :212-222): rotating tiles (q and k heads of 128) hold per wave 32 columns d and their
//         rotate-half partners d + 64; q goes to C, k to ep.p0 (the K cache rows), v (plain tiles) to ep.p1.
// All three round exactly where the unfused path rounds (GEMM output to bf16 first), so results are bit-identical to GEMM + elementwise kernel.
struct GemmEpi {
    void* p0; void* p1; const float* f0; const float* f1;
    int64_t ld0, ld1;
    int i0, i1;
};

// B-tile row (0..255) -> row of the stored weight for the fused forms; -1 = past the operand (clamped by the caller)
template <int EPI>
TR1_DEV int64_t epi_brow(int row, int64_t n0, int64_t N, const GemmEpi& ep) {
    if (EPI == 2) {
        const int64_t col = (n0 >> 1) + (row >> 6) * 32 + (row & 31);        // intermediate column
        const int64_t I = ep.i0;
        return ((row >> 5) & 1) * I + (col < I ? col : I - 1);
    }
    if (EPI == 4) {
        if (n0 < (int64_t)ep.i0 + ep.i1) return n0 + (row >> 7) * 128 + ((row >> 6) & 1) * 32 + ((row >> 5) & 1) * 64 + (row & 31);
        const int64_t r = n0 + row;
        return r < N ? r : N - 1;
    }
    if (EPI == 7) {          // vision q|k|v: ep.i0 = pairs per section (n_heads * half), ep.i1 = half (40); a tile = 128 consecutive pairs of one section
        const int tps = ep.i0 >> 7, tile = (int)(n0 >> 8);
        const int sec = tile / tps, pair = (tile - sec * tps) * 128 + (row >> 6) * 32 + (row & 31);
        const int head = pair / ep.i1, d = pair - head * ep.i1;
        return (int64_t)sec * 2 * ep.i0 + head * 2 * ep.i1 + d + ((row >> 5) & 1) * ep.i1;
    }
    const int64_t r = n0 + row;
    return r < N ? r : N - 1;
}

template <bool IS_B, int REGION_ROWS, int EPI = 0>
TR1_DEV void stage_round(const bf16_t* __restrict__ g, int64_t ld, int64_t row0, int64_t rows_valid, int64_t k0, char* lds_region,
                         char* junk, int round, int wave, int lane, const GemmEpi* ep = nullptr) {
    const int inst = round * 8 + wave;                                   // 8 rows (1 KiB) per wave-instruction
    int row = inst * 8 + (lane >> 3);
    char* dst = lds_region + inst * 1024;
    if (REGION_ROWS % 64 != 0 && inst * 8 >= REGION_ROWS) { dst = junk + (wave & 3) * 1024; row = REGION_ROWS - 8 + (lane >> 3); }   // wave-uniform
    const int logical = (lane & 7) ^ (IS_B ? keyB(row) : keyA(row));
    int64_t grow;
    if (IS_B && (EPI == 2 || EPI == 4 || EPI == 7)) grow = epi_brow<EPI>(row, row0, rows_valid, *ep);
    else { grow = row0 + row; if (grow >= rows_valid) grow = rows_valid - 1; }
    __builtin_amdgcn_global_load_lds((gptr_t)(g + grow * ld + k0 + logical * 8), (lptr_t)dst, 16, 0, 0);
}


template <int RT, int EPI>
TR1_DEV void store_acc256_pairs(const f32x4_t (&acc)[RT][4], char* __restrict__ wave_lds, void* __restrict__ Cv, const bf16_t* __restrict__ bias,
                                int64_t M, int64_t N, int64_t ldc, int64_t mrow0, int64_t n0, int wn, int lane, const GemmEpi& ep) {
    constexpr int CH = (RT % 2 == 0) ? 4 : 3;
    const int u = lane & 15, g = lane >> 4;
    const int c4 = lane & 3, q = (lane >> 2) & 3;
    const int rr16 = (q & 1) + (q >> 1) * 8 + 2 * (lane >> 4);
    // column bookkeeping of this lane's 8 pair columns
    int64_t col_a;              // EPI 2: intermediate column; EPI 4: column inside q (or k) of the "a" half (d < 64)
    bf16_t *dst_a, *dst_b, *dst_ga = nullptr, *dst_gb = nullptr;
    int64_t ld_o, ld_g = 0;
    bool col_ok;
    u32x4_t ba = {0, 0, 0, 0}, bb = {0, 0, 0, 0};
    int dcs = 0;                // EPI 4: index of the lane's first column into a row of the cos / sin tables
    if (EPI == 2) {
        const int64_t I = ep.i0;
        col_a = (n0 >> 1) + wn * 32 + c4 * 8;
        col_ok = col_a + 8 <= I;
        if (bias && col_ok) { ba = *reinterpret_cast<const u32x4_t*>(bias + col_a); bb = *reinterpret_cast<const u32x4_t*>(bias + I + col_a); }
        dst_a = reinterpret_cast<bf16_t*>(Cv) + col_a; dst_b = nullptr; ld_o = ldc;
        if (ep.p0) { dst_ga = reinterpret_cast<bf16_t*>(ep.p0) + col_a; dst_gb = dst_ga + I; ld_g = ep.ld0; }
    } else if (EPI == 7) {
        // Qwen2-VL / 2.5-VL vision attention (TF:225-248 apply_rotary_pos_emb_vision, head dim 80): section = q | k | v, the lane's 8 pair columns d0..d0+7
        // (< 40) of one head and their partners d0 + 40.  Outputs go to 128-wide PADDED heads: d -> head*128 + d, d + 40 -> head*128 + 48 + d (64 + d when half > 48), so the head-dim-128
        // attention kernels (32x32x16 MFMA, K / V row-major) take the tower; the pad columns are zero-filled once by the caller.
        const int tps = ep.i0 >> 7, tile = (int)(n0 >> 8);
        const int sec = tile / tps, pair0 = (tile - sec * tps) * 128 + wn * 32 + c4 * 8;
        const int head = pair0 / ep.i1, d0 = pair0 - head * ep.i1;
        const int64_t ncol = (int64_t)sec * 2 * ep.i0 + head * 2 * ep.i1 + d0;
        col_ok = true;
        dcs = sec < 2 ? d0 : -1;                                        // -1: v, no rotation
        if (bias) { ba = *reinterpret_cast<const u32x4_t*>(bias + ncol); bb = *reinterpret_cast<const u32x4_t*>(bias + ncol + ep.i1); }
        if (sec == 0) { dst_a = reinterpret_cast<bf16_t*>(Cv); ld_o = ldc; }
        else if (sec == 1) { dst_a = reinterpret_cast<bf16_t*>(ep.p0); ld_o = ep.ld0; }
        else { dst_a = reinterpret_cast<bf16_t*>(ep.p1); ld_o = ep.ld1; }
        dst_a += head * 128 + d0;
        dst_b = dst_a + (ep.i1 <= 48 ? 48 : 64);       // round 6: halves of <= 48 features sit 48 apart - the head's live features then end at 96 (tr1_attn_fwd_rows_live96)
        col_a = ncol;
    } else {
        const int d = (wn & 1) * 32 + c4 * 8;
        const int64_t ncol = n0 + (wn >> 1) * 128 + d;                  // column of the fused q|k|v projection
        col_ok = true;
        dcs = d;
        if (bias) { ba = *reinterpret_cast<const u32x4_t*>(bias + ncol); bb = *reinterpret_cast<const u32x4_t*>(bias + ncol + 64); }
        if (n0 < ep.i0) { dst_a = reinterpret_cast<bf16_t*>(Cv) + ncol; ld_o = ldc; }
        else { dst_a = reinterpret_cast<bf16_t*>(ep.p0) + (ncol - ep.i0); ld_o = ep.ld0; }
        dst_b = dst_a + 64;
        col_a = ncol;
    }
#pragma unroll
    for (int i0 = 0; i0 < RT; i0 += CH) {
        const int cnt = RT - i0 < CH ? RT - i0 : CH;
#pragma unroll
        for (int ii = 0; ii < CH; ++ii) {
            if (ii < cnt) {
                const int row = ii * 16 + u;
#pragma unroll
                for (int j = 0; j < 4; ++j) *reinterpret_cast<f32x4_t*>(wave_lds + row * 256 + (((g * 4 + j) ^ u) << 4)) = acc[i0 + ii][j];
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int r16 = 0; r16 < CH; ++r16) {
            if (r16 < cnt) {
                const int rr = r16 * 16 + rr16;
                const char* rowp = wave_lds + rr * 256;
                const f32x4_t a0 = *reinterpret_cast<const f32x4_t*>(rowp + (((2 * c4) ^ rr16) << 4));
                const f32x4_t a1 = *reinterpret_cast<const f32x4_t*>(rowp + (((2 * c4 + 1) ^ rr16) << 4));
                const f32x4_t b0 = *reinterpret_cast<const f32x4_t*>(rowp + (((8 + 2 * c4) ^ rr16) << 4));
                const f32x4_t b1 = *reinterpret_cast<const f32x4_t*>(rowp + (((9 + 2 * c4) ^ rr16) << 4));
                float va[8] = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
                float vb[8] = {b0[0], b0[1], b0[2], b0[3], b1[0], b1[1], b1[2], b1[3]};
                const int64_t m = mrow0 + i0 * 16 + rr;
                if (m < M && col_ok) {
                    u32x4_t oa, ob;
                    if (EPI == 2) {
                        u32x4_t pg, pu;
                        if (bias) {
#pragma unroll
                            for (int e = 0; e < 4; ++e) { va[2 * e] += bflo(ba[e]); va[2 * e + 1] += bfhi(ba[e]); vb[2 * e] += bflo(bb[e]); vb[2 * e + 1] += bfhi(bb[e]); }
                        }
#pragma unroll
                        for (int e = 0; e < 4; ++e) { pg[e] = pack2bf(va[2 * e], va[2 * e + 1]); pu[e] = pack2bf(vb[2 * e], vb[2 * e + 1]); }
                        if (dst_ga) {
                            *reinterpret_cast<u32x4_t*>(dst_ga + m * ld_g) = pg;
                            *reinterpret_cast<u32x4_t*>(dst_gb + m * ld_g) = pu;
                        }
#pragma unroll
                        for (int e = 0; e < 4; ++e) {        // as swiglu_fwd_kernel: on the bf16-rounded gate / up, silu rounded to bf16 before the product
                            const float x0 = bf2f(f2bf(epi_silu(bflo(pg[e])))) * bflo(pu[e]);
                            const float x1 = bf2f(f2bf(epi_silu(bfhi(pg[e])))) * bfhi(pu[e]);
                            oa[e] = pack2bf(x0, x1);
                        }
                        *reinterpret_cast<u32x4_t*>(dst_a + m * ld_o) = oa;
                    } else {
                        const int rs = EPI == 7 ? ep.i1 : 64, dc = dcs < 0 ? 0 : dcs;
                        const float* cp = ep.f0 + m * rs + dc;
                        const float* sp = ep.f1 + m * rs + dc;
                        f32x4_t c0 = *reinterpret_cast<const f32x4_t*>(cp), c1 = *reinterpret_cast<const f32x4_t*>(cp + 4);
                        f32x4_t s0 = *reinterpret_cast<const f32x4_t*>(sp), s1 = *reinterpret_cast<const f32x4_t*>(sp + 4);
                        if (EPI == 7 && dcs < 0) { c0 = c1 = (f32x4_t){1.f, 1.f, 1.f, 1.f}; s0 = s1 = (f32x4_t){0.f, 0.f, 0.f, 0.f}; }    // v: x * 1 - y * 0 = x exactly
                        const float cc[8] = {c0[0], c0[1], c0[2], c0[3], c1[0], c1[1], c1[2], c1[3]};
                        const float ss[8] = {s0[0], s0[1], s0[2], s0[3], s1[0], s1[1], s1[2], s1[3]};
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            va[2 * e] += bflo(ba[e]); va[2 * e + 1] += bfhi(ba[e]); vb[2 * e] += bflo(bb[e]); vb[2 * e + 1] += bfhi(bb[e]);
                        }
#pragma unroll
                        for (int e = 0; e < 8; ++e) { va[e] = bf2f(f2bf(va[e])); vb[e] = bf2f(f2bf(vb[e])); }      // the projection output as the unfused path stores it
#pragma unroll
                        for (int e = 0; e < 4; ++e) {        // as rope_apply_kernel (forward)
                            oa[e] = pack2bf(va[2 * e] * cc[2 * e] - vb[2 * e] * ss[2 * e], va[2 * e + 1] * cc[2 * e + 1] - vb[2 * e + 1] * ss[2 * e + 1]);
                            ob[e] = pack2bf(vb[2 * e] * cc[2 * e] + va[2 * e] * ss[2 * e], vb[2 * e + 1] * cc[2 * e + 1] + va[2 * e + 1] * ss[2 * e + 1]);
                        }
                        *reinterpret_cast<u32x4_t*>(dst_a + m * ld_o) = oa;
                        *reinterpret_cast<u32x4_t*>(dst_b + m * ld_o) = ob;
                    }
                }
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
}

// EPI 3: the wave's 64 columns of da (K-major dgrad of the down projection) -> dgu columns n (gate half) and I + n (up half), as swiglu_bwd_kernel
template <int RT>
TR1_DEV void store_acc256_glubwd(const f32x4_t (&acc)[RT][4], char* __restrict__ wave_lds, void* __restrict__ Cv, int64_t M, int64_t N, int64_t ldc,
                                 int64_t mrow0, int64_t ncol0, int lane, const GemmEpi& ep) {
    constexpr int CH = (RT % 2 == 0) ? 4 : 3;
    const int u = lane & 15, g = lane >> 4;
    const int c8 = lane & 7;
    const int64_t n = ncol0 + c8 * 8, I = ep.i0;
    const bf16_t* gu = reinterpret_cast<const bf16_t*>(ep.p0);
    bf16_t* dguT = reinterpret_cast<bf16_t*>(ep.p1);          // optional second output: dgu^T [2I, ep.ld1] (ep.ld1 = tokens rounded up to 64, columns >= M zero)
    if (dguT && mrow0 + RT * 16 >= M && mrow0 + RT * 16 < ep.ld1 && ((mrow0 + RT * 16) % (RT * 32)) == 0) {
        // the tile rows end (a multiple of 32) short of the padded width (a multiple of 64): the lower wave row of the last row tile zero-fills the 32 columns left
        const int64_t mz = mrow0 + RT * 16;
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            const int idx = it * 64 + lane, col = idx >> 2, ch = idx & 3, part = col >> 6, ncol = col & 63;
            if (ncol0 + ncol < N && mz + ch * 8 < ep.ld1)
                *reinterpret_cast<u32x4_t*>(dguT + ((int64_t)part * I + ncol0 + ncol) * ep.ld1 + mz + ch * 8) = u32x4_t{0, 0, 0, 0};
        }
    }
#pragma unroll
    for (int i0 = 0; i0 < RT; i0 += CH) {
        const int cnt = RT - i0 < CH ? RT - i0 : CH;
#pragma unroll
        for (int ii = 0; ii < CH; ++ii) {
            if (ii < cnt) {
                const int row = ii * 16 + u;
#pragma unroll
                for (int j = 0; j < 4; ++j) *reinterpret_cast<f32x4_t*>(wave_lds + row * 256 + (((g * 4 + j) ^ u) << 4)) = acc[i0 + ii][j];
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int r8 = 0; r8 < CH * 2; ++r8) {
            if (r8 < cnt * 2) {
                const int rr = r8 * 8 + (lane >> 3);
                const f32x4_t v0 = *reinterpret_cast<const f32x4_t*>(wave_lds + rr * 256 + (((2 * c8) ^ (rr & 15)) << 4));
                const f32x4_t v1 = *reinterpret_cast<const f32x4_t*>(wave_lds + rr * 256 + (((2 * c8 + 1) ^ (rr & 15)) << 4));
                const float v[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
                if (dguT) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // (both reads of every lane have returned before the row is rewritten below)
                const int64_t m = mrow0 + i0 * 16 + rr;
                u32x4_t og = {0, 0, 0, 0}, ou = {0, 0, 0, 0};
                if (m < M && n + 8 <= N) {
                    const u32x4_t gg = *reinterpret_cast<const u32x4_t*>(gu + m * ep.ld0 + n);
                    const u32x4_t uu = *reinterpret_cast<const u32x4_t*>(gu + m * ep.ld0 + I + n);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float gv[2] = {bflo(gg[e]), bfhi(gg[e])}, uv[2] = {bflo(uu[e]), bfhi(uu[e])};
                        const float dv[2] = {bf2f(f2bf(v[2 * e])), bf2f(f2bf(v[2 * e + 1]))};      // da as the unfused dgrad stores it
                        float rg[2], ru[2];
#pragma unroll
                        for (int k = 0; k < 2; ++k) {
                            const float sg = 1.f / (1.f + __expf(-gv[k]));
                            const float si = gv[k] * sg;
                            rg[k] = dv[k] * uv[k] * (sg * (1.f + gv[k] * (1.f - sg)));
                            ru[k] = dv[k] * si;
                        }
                        og[e] = pack2bf(rg[0], rg[1]); ou[e] = pack2bf(ru[0], ru[1]);
                    }
                    bf16_t* cp = reinterpret_cast<bf16_t*>(Cv) + m * ldc + n;
                    *reinterpret_cast<u32x4_t*>(cp) = og;
                    *reinterpret_cast<u32x4_t*>(cp + I) = ou;
                }
                if (dguT) {
                    // the row's fp32 values have been read (its 8 lanes cover all 16 chunks, LDS operations of a wave retire in order): its 256 bytes now
                    // hold the bf16 results (zeros for rows >= M: the transposed copy is zero-padded), gate chunk c8 at ((row & 1) << 3 | c8 ^ (row / 8 % 8)), up in
                    // the other half - conflict-free for these row writes (two rows per quarter wave use opposite halves) and for the column reads below
                    const int k3 = (rr >> 3) & 7, hb = rr & 1;
                    *reinterpret_cast<u32x4_t*>(wave_lds + rr * 256 + (((hb << 3) | (c8 ^ k3)) << 4)) = og;
                    *reinterpret_cast<u32x4_t*>(wave_lds + rr * 256 + ((((hb ^ 1) << 3) | (c8 ^ k3)) << 4)) = ou;
                }
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (dguT) {
            // transposed read-back: lane -> (column, 8-row chunk); the 8 lanes of a column write 128 contiguous bytes of dgu^T (8 row chunks = 64 rows)
            const int rc = lane & 7;
            const int64_t mchunk = mrow0 + i0 * 16 + rc * 8;
            if (rc < cnt * 2 && mchunk < ep.ld1) {
#pragma unroll
                for (int it = 0; it < 16; ++it) {
                    const int part = it >> 3, ncol = (it & 7) * 8 + (lane >> 3);
                    if (ncol0 + ncol < N) {
                        unsigned short t[8];
#pragma unroll
                        for (int e = 0; e < 8; ++e) {
                            const int row = rc * 8 + e;
                            t[e] = *reinterpret_cast<const unsigned short*>(wave_lds + row * 256 + ((((part ^ (row & 1)) << 3) | ((ncol >> 3) ^ rc)) << 4) + (ncol & 7) * 2);
                        }
                        const u32x4_t w = {t[0] | ((unsigned)t[1] << 16), t[2] | ((unsigned)t[3] << 16), t[4] | ((unsigned)t[5] << 16), t[6] | ((unsigned)t[7] << 16)};
                        *reinterpret_cast<u32x4_t*>(dguT + ((int64_t)part * I + ncol0 + ncol) * ep.ld1 + mchunk) = w;
                    }
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
    }
}

template <bool OUT_F32, bool ACCUM, int RT, bool BKM = false, int EPI = 0>
__global__ __launch_bounds__(512) void gemm_nt8p_kernel(const bf16_t* __restrict__ A, const bf16_t* __restrict__ B, void* __restrict__ Cv,
                                                        const bf16_t* __restrict__ bias, const bf16_t* __restrict__ residual,
                                                        int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc,
                                                        int64_t ldr, int tiles_m, int tiles_n, const GemmEpi ep) {
    constexpr int BMX = RT * 32;
    constexpr int A_BYTES = BMX * BK * 2, BUF_BYTES = A_BYTES + TILE2_BYTES;
    constexpr int AR = (BMX + 63) / 64;                // A rounds per K-tile; phases 0 / 1 issue AR0 / AR1 of them
    constexpr int AR0 = (AR + 1) / 2;
    constexpr int Q0 = 0, Q1 = (RT + 3) / 4, Q2 = Q1 + (RT + 2) / 4, Q3 = Q2 + (RT + 1) / 4, Q4 = RT;   // M-quarters (m-tile ranges)
    constexpr int QMAX = Q1 - Q0;
    extern __shared__ __attribute__((aligned(16))) char smem2[];  // [buf][A | B] + junk
    char* const junk = smem2 + 2 * BUF_BYTES;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 2, wn = wave & 3;
    const int nwg = tiles_m * tiles_n;
    int wgid;
    {
        int b = blockIdx.x;
        if (EPI == 6) {                                  // S-way split-K (S = ep.i0): the grid holds every tile S times; copy kz reduces its share of the
            const int kz = b / nwg;                      // K tiles into its own fp32 plane of C (summed by splitk_reduce_kernel in a fixed order)
            b -= kz * nwg;
            const int nk_all = (int)(K / BK), q = nk_all / ep.i0, r = nk_all - q * ep.i0;
            const int64_t k0 = (int64_t)(kz * q + (kz < r ? kz : r)) * BK;
            K = (int64_t)(q + (kz < r ? 1 : 0)) * BK;
            A += k0;
            B += BKM ? k0 * ldb : k0;
            Cv = reinterpret_cast<float*>(Cv) + (int64_t)kz * ep.ld0;
        }
        const int xcd = b & 7, q = nwg >> 3, r = nwg & 7;
        wgid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (b >> 3);
    }
    const int GROUP_M = 4;
    const int group = wgid / (GROUP_M * tiles_n);
    const int first_m = group * GROUP_M;
    const int gsz = min(tiles_m - first_m, GROUP_M);
    const int in_group = wgid - group * GROUP_M * tiles_n;
    const int tm = first_m + in_group % gsz;
    const int tn = in_group / gsz;
    const int64_t m0 = (int64_t)tm * BMX, n0 = (int64_t)tn * BN2;

    f32x4_t acc[RT][4];
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

    const int nk = (int)(K / BK);
    const int u = lane & 15, g = lane >> 4;
    // per-lane LDS byte offsets of the fragment reads (k-step 1 = k-step 0 with chunk bit 2 flipped: offset ^ 64)
    const int a_off = (wm * (RT * 16) + u) * 128 + ((g ^ ((u >> 1) & 7)) << 4);
    const int b_off = (wn * 64 + (u >> 2) * 16 + (u & 3)) * 128 + ((g ^ (((u >> 2) << 1) | ((u >> 1) & 1))) << 4);
    // BKM fragment j of k step ks: lane L of a 16-lane group supplies row (L >> 2) of a 4-row block, 8 bytes at columns wn*64 + (L & 3)*16 + j*4.
    // Lane group g takes the blocks of k rows g*8 .. +3 and g*8 + 4 .. +7, i.e. the standard k order of the MFMA, so the A side is unchanged.
    const int bkm_row = g * 8 + (u >> 2);                                   // + ks*32 (+4 for the second half)
    const int bkm_key = keyKM(bkm_row);                                     // depends on the row's low two bits only
    const int64_t bkm_kvalid = (BKM && ldr > 0) ? ldr : K;                  // K-major B: `ldr` carries the number of valid k rows of B (no residual in this form)

#define STAGE_A(t, r) stage_round<false, BMX>(A, lda, m0, M, (int64_t)(t) * BK, smem2 + ((t) & 1) * BUF_BYTES, junk, (r), wave, lane)
#define STAGE_B(t, r) do { if (BKM) stage_round_km(B, ldb, n0, N, (int64_t)(t) * BK, bkm_kvalid, smem2 + ((t) & 1) * BUF_BYTES + A_BYTES, (r), wave, lane); \
                           else stage_round<true, BN2, EPI>(B, ldb, n0, N, (int64_t)(t) * BK, smem2 + ((t) & 1) * BUF_BYTES + A_BYTES, junk, (r), wave, lane, &ep); } while (0)
    // prologue: tile 0 complete, B of tile 1 in flight
#pragma unroll
    for (int r = 0; r < 4; ++r) STAGE_B(0, r);
#pragma unroll
    for (int r = 0; r < AR; ++r) STAGE_A(0, r);
    if (nk > 1) {
#pragma unroll
        for (int r = 0; r < 4; ++r) STAGE_B(1, r);
        asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    TR1_BARRIER();
    if (wm == 1) TR1_BARRIER();                        // the second wave group runs one barrier interval behind the first

    bf16x8_t bf[4][2], af[QMAX][2];
#define LOAD_A(QA, QB) do {                                                                                    \
        _Pragma("unroll") for (int i = (QA); i < (QB); ++i) {                                                  \
            af[i - (QA)][0] = *reinterpret_cast<const bf16x8_t*>(curA + a_off + i * 2048);                     \
            af[i - (QA)][1] = *reinterpret_cast<const bf16x8_t*>(curA + (a_off ^ 64) + i * 2048);              \
        } } while (0)
#define COMPUTE(QA, QB) do {                                                                                   \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                                     \
        TR1_BARRIER();                                                                                         \
        __builtin_amdgcn_s_setprio(1);                                                                         \
        _Pragma("unroll") for (int ks = 0; ks < 2; ++ks)                                                       \
        _Pragma("unroll") for (int i = (QA); i < (QB); ++i)                                                    \
        _Pragma("unroll") for (int j = 0; j < 4; ++j)                                                          \
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf[j][ks], af[i - (QA)][ks], acc[i][j], 0, 0, 0); \
        __builtin_amdgcn_s_setprio(0);                                                                         \
        TR1_BARRIER();                                                                                         \
    } while (0)

    for (int t = 0; t < nk; ++t) {
        const char* curA = smem2 + (t & 1) * BUF_BYTES;
        const char* curB = curA + A_BYTES;
        // ---- phase 0: all B fragments + A quarter 0; A rounds [0, AR0) of tile t+1
        if (BKM) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    const int lc = wn * 8 + (u & 3) * 2 + (j >> 1);                                    // logical 16-byte chunk of the piece
                    const char* pb = curB + (ks * 32 + bkm_row) * 512 + ((lc ^ bkm_key) << 4) + (j & 1) * 8;
                    const u32x2_t h0 = tr1_lds_read_tr16(pb), h1 = tr1_lds_read_tr16(pb + 4 * 512);    // rows +4: same key (low two bits unchanged)
                    u32x4_t w = {h0[0], h0[1], h1[0], h1[1]};
                    bf[j][ks] = __builtin_bit_cast(bf16x8_t, w);
                }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                bf[j][0] = *reinterpret_cast<const bf16x8_t*>(curB + b_off + j * 512);
                bf[j][1] = *reinterpret_cast<const bf16x8_t*>(curB + (b_off ^ 64) + j * 512);
            }
        }
        LOAD_A(Q0, Q1);
        if (t + 1 < nk) {
#pragma unroll
            for (int r = 0; r < AR0; ++r) STAGE_A(t + 1, r);
        }
        COMPUTE(Q0, Q1);
        // ---- phase 1: A quarter 1; the remaining A rounds of tile t+1
        LOAD_A(Q1, Q2);
        if (t + 1 < nk) {
#pragma unroll
            for (int r = AR0; r < AR; ++r) STAGE_A(t + 1, r);
        }
        COMPUTE(Q1, Q2);
        // ---- phase 2: A quarter 2; B rounds 0, 1 of tile t+2 (tile t's B region is free: read in phase 0 only)
        LOAD_A(Q2, Q3);
        if (t + 2 < nk) { STAGE_B(t + 2, 0); STAGE_B(t + 2, 1); }
        COMPUTE(Q2, Q3);
        // ---- phase 3: A quarter 3; B rounds 2, 3 of tile t+2; tile t+1 must have landed before the next barrier
        LOAD_A(Q3, Q4);
        if (t + 2 < nk) {
            STAGE_B(t + 2, 2); STAGE_B(t + 2, 3);
            asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        COMPUTE(Q3, Q4);
    }
    if (wm == 0) TR1_BARRIER();
#undef LOAD_A
#undef COMPUTE
#undef STAGE_A
#undef STAGE_B
#ifdef TR1_PROBE_NO_EPI      // measurement build (tools/build_variant.py noepi -DTR1_PROBE_NO_EPI=1): the tile ends here, nothing is stored - what the epilogue costs
    if (K > 0) return;
#endif
    // every wave is past its last LDS read (the realignment barrier above): the operand buffers become 8 private staging slices
    if (EPI == 2 || EPI == 7 || (EPI == 4 && n0 < (int64_t)ep.i0 + ep.i1))
        store_acc256_pairs<RT, EPI>(acc, smem2 + wave * (((RT % 2 == 0) ? 4 : 3) * 4096), Cv, bias, M, N, ldc, m0 + wm * (RT * 16), n0, wn, lane, ep);
    else if (EPI == 4)       // V tile: bias only, into its own buffer
        store_acc256_lds<false, false, RT, 0>(acc, smem2 + wave * (((RT % 2 == 0) ? 4 : 3) * 4096), ep.p1, bias + ep.i0 + ep.i1, nullptr, M, N - ep.i0 - ep.i1,
                                              ep.ld1, 0, m0 + wm * (RT * 16), n0 - ep.i0 - ep.i1 + wn * 64, lane);
    else if (EPI == 6)
        store_acc256_lds<true, false, RT, 0>(acc, smem2 + wave * (((RT % 2 == 0) ? 4 : 3) * 4096), Cv, nullptr, nullptr, M, N, ldc, 0, m0 + wm * (RT * 16), n0 + wn * 64, lane);
    else if (EPI == 3)
        store_acc256_glubwd<RT>(acc, smem2 + wave * (((RT % 2 == 0) ? 4 : 3) * 4096), Cv, M, N, ldc, m0 + wm * (RT * 16), n0 + wn * 64, lane, ep);
    else
    store_acc256_lds<OUT_F32, ACCUM, RT, EPI>(acc, smem2 + wave * (((RT % 2 == 0) ? 4 : 3) * 4096), Cv, bias, residual, M, N, ldc, ldr,
                                              m0 + wm * (RT * 16), n0 + wn * 64, lane,
                                              (OUT_F32 && EPI == 0 && ep.p0) ? reinterpret_cast<float*>(ep.p0) + (int64_t)blockIdx.x * 8 + wave : nullptr,
                                              (OUT_F32 && EPI == 0 && ep.p0) ? reinterpret_cast<bf16_t*>(ep.p1) : nullptr, ep.ld1);
}

// ---- tile height and launch of the phased 8-wave GEMM (gemm_nt8p_kernel: 224 / 256 / 288 / 320 rows x 256 columns, one block per CU) ------------------
// Cost of a tile height: CU-rounds x block area / relative efficiency of the structure (tile-count quantisation).
// Intrinsic efficiency of the heights relative to 256 x 256 (more A-fragment reuse per B fragment with taller tiles), measured on M = 37888, N = 3584,
// K = 5120 and 8192^3 after removing tile-count quantisation (tools/microbench.py gemm, tile forced):
static const double NT8P_EFF[4] = {0.94, 1.0, 1.025, 1.03};      // 224, 256, 288, 320 rows
static double nt8p_cost(int64_t M, int64_t n_tiles, int64_t rows, double eff) {
    const int64_t t = ((M + rows - 1) / rows) * n_tiles;
    return (double)((t + 255) / 256) * 256.0 * (double)(rows * BN2) / eff;
}
// RT (rows / 32) of the cheapest height for M rows x n_tiles column tiles; among equals the one tried first wins: first = 256 tries 256, 224, 288, 320,
// first = 224 tries 224, 256, 288, 320.  224 is the NT dispatch (tr1_gemm_nt_bf16) and the NT weight gradient (tr1_wgrad_f32_sumsq), whose results are
// bit-identical because they pick alike; every other form starts at 256.
static int nt8p_pick_rt(int64_t M, int64_t n_tiles, int first) {
    int rt = first / 32; double best = nt8p_cost(M, n_tiles, first, NT8P_EFF[rt - 7]);
    for (int r = 7; r <= 10; ++r) { const double c = nt8p_cost(M, n_tiles, r * 32, NT8P_EFF[r - 7]); if (c < best) { best = c; rt = r; } }
    return rt;
}
// what a launch needs of the height: row tiles and dynamic LDS (two buffers of an A tile + a B tile, + the 4 KiB junk page)
struct Nt8pTile {
    int rt; int64_t t2m; size_t dyn;
    Nt8pTile(int rt_, int64_t M) : rt(rt_), t2m((M + rt_ * 32 - 1) / (rt_ * 32)), dyn(2 * ((size_t)rt_ * 32 * BK * 2 + TILE2_BYTES) + 4096) {}
};
// the one place where the run-time height becomes the kernel's template argument; the four heights share the 320-row form's LDS limit
template <bool OUT_F32, bool ACCUM, bool BKM, int EPI>
static void launch_nt8p(const Nt8pTile& t, int64_t t2n, int64_t blocks, hipStream_t s, const void* A, const void* B, void* C, const void* bias, const void* residual,
                        int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc, int64_t ldr, const GemmEpi& ep) {
    constexpr int LDS_CAP = (int)(2 * (320 * BK * 2 + TILE2_BYTES)) + 4096;
    tr1_dispatch<7, 9, 10, 8>(t.rt, [&](auto R) {
        tr1_launch<gemm_nt8p_kernel<OUT_F32, ACCUM, decltype(R)::value, BKM, EPI>>(dim3((unsigned)blocks), dim3(512), t.dyn, LDS_CAP, s, (const bf16_t*)A, (const bf16_t*)B, C,
                                                                                 (const bf16_t*)bias, (const bf16_t*)residual, M, N, K, lda, ldb, ldc, ldr, (int)t.t2m,
                                                                                 (int)t2n, ep);
    });
}

extern "C" int tr1_gemm_nt_bf16(const void* A, const void* B, void* C, const void* bias, const void* residual, int64_t M, int64_t N,
                                int64_t K, int64_t lda, int64_t ldb, int64_t ldc, int64_t ldr, int out_f32, int accumulate, void* stream) {
    TR1_CHECK_ARG(K % BK == 0, "gemm_nt: K must be a multiple of 64 (pad the operands)");
    TR1_CHECK_ARG(N % 8 == 0 && lda % 8 == 0 && ldb % 8 == 0 && ldc % 4 == 0, "gemm_nt: N%8, lda%8, ldb%8, ldc%4 required");
    TR1_CHECK_ARG(!accumulate || out_f32, "gemm_nt: accumulate requires fp32 output");
    TR1_CHECK_ARG(!residual || ldr % 8 == 0, "gemm_nt: ldr%8 required");
    TR1_CHECK_ARG(out_f32 || ldc % 8 == 0, "gemm_nt: ldc%8 required for bf16 output");
    if (M == 0 || N == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    if (M <= 64 && !accumulate && K >= 256) {
        launch_skinny(A, B, C, bias, residual, M, N, K, lda, ldb, ldc, ldr, out_f32, 1, s);
        TR1_LAUNCH_CHECK();
    }
    const int tiles_m = (int)((M + BM - 1) / BM), tiles_n = (int)((N + BN - 1) / BN);
    if (M >= 512 && N >= 256) {
        // the cheapest 8-wave height against the 128 x 128 form, which runs 2 blocks per CU (512 slots) at 0.80 of the 256 x 256 rate per CU: the 8-wave
        // tile only where it is strictly cheaper
        const int64_t t128 = (int64_t)tiles_m * tiles_n, t2n = (N + BN2 - 1) / BN2;
        const double cost128 = (double)((t128 + 511) / 512) * 512.0 * (double)(BM * BN) / 0.80;
        const Nt8pTile t(nt8p_pick_rt(M, t2n, 224), M);
        if (nt8p_cost(M, t2n, t.rt * 32, NT8P_EFF[t.rt - 7]) < cost128) {
            auto go = [&](auto OF, auto AC) {
                launch_nt8p<decltype(OF)::value, decltype(AC)::value, false, 0>(t, t2n, t.t2m * t2n, s, A, B, C, bias, residual, M, N, K, lda, ldb, ldc, ldr, GemmEpi{});
            };
            if (!out_f32) go(std::false_type{}, std::false_type{}); else if (accumulate) go(std::true_type{}, std::true_type{}); else go(std::true_type{}, std::false_type{});
            TR1_LAUNCH_CHECK();
        }
    }
    dim3 grid((unsigned)(tiles_m * tiles_n));
#define LAUNCH(OF, AC)                                                                                                              \
    hipLaunchKernelGGL((gemm_nt_kernel<OF, AC>), grid, dim3(256), 0, s, (const bf16_t*)A, (const bf16_t*)B, C, (const bf16_t*)bias, \
                       (const bf16_t*)residual, M, N, K, lda, ldb, ldc, ldr, tiles_m, tiles_n)
    if (out_f32) { if (accumulate) LAUNCH(true, true); else LAUNCH(true, false); }
    else LAUNCH(false, false);
#undef LAUNCH
    TR1_LAUNCH_CHECK();
}

// C[M,N] = A[M,K] * B[K,N]  ("NN": B is K-major - the dgrad dX = dY * W reads the weight as stored, no W^T copy).  Phased 8-wave forms only
// (M >= 512, N >= 256): B tiles are staged as 16 k-rows x 256 columns per round and read back transposed (ds_read_b64_tr_b16).  bf16 output.
extern "C" int tr1_gemm_nn_bf16(const void* A, const void* B, void* C, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc,
                                void* stream) {
    TR1_CHECK_ARG(K % BK == 0, "gemm_nn: K must be a multiple of 64");
    TR1_CHECK_ARG(N % 8 == 0 && lda % 8 == 0 && ldb % 8 == 0 && ldc % 8 == 0, "gemm_nn: N%8, lda%8, ldb%8, ldc%8 required");
    TR1_CHECK_ARG(M >= 512 && N >= 256, "gemm_nn: M >= 512 and N >= 256 required (smaller problems: transpose B and use gemm_nt)");
    const int64_t t2n = (N + BN2 - 1) / BN2;
    const Nt8pTile t(nt8p_pick_rt(M, t2n, 256), M);
    launch_nt8p<false, false, true, 0>(t, t2n, t.t2m * t2n, (hipStream_t)stream, A, B, C, nullptr, nullptr, M, N, K, lda, ldb, ldc, 0, GemmEpi{});
    TR1_LAUNCH_CHECK();
}

// C[M,N] (fp32) (+)= A[M,K] * B[K,N] with B K-major and only its first `b_rows` k rows valid: the WEIGHT GRADIENT dW[n,k] += sum_t dY^T[n,t] X[t,k]
// with A = dY^T (the transposed copy, zero-padded to a multiple of 64 tokens) and B = X AS STORED - no X^T copy (the 18944-column SwiGLU
// output of the down projection was the largest transpose of the backward).  Same kernel, tiles and accumulation order as tr1_gemm_nn_bf16.
extern "C" int tr1_gemm_nn_acc_f32(const void* A, const void* B, void* C, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc,
                                   int accumulate, int64_t b_rows, void* stream) {
    TR1_CHECK_ARG(K % BK == 0, "gemm_nn_acc: K must be a multiple of 64");
    TR1_CHECK_ARG(N % 8 == 0 && lda % 8 == 0 && ldb % 8 == 0 && ldc % 4 == 0, "gemm_nn_acc: N%8, lda%8, ldb%8, ldc%4 required");
    TR1_CHECK_ARG(M >= 512 && N >= 256, "gemm_nn_acc: M >= 512 and N >= 256 required");
    TR1_CHECK_ARG(b_rows >= 1 && b_rows <= K, "gemm_nn_acc: 1 <= b_rows <= K");
    hipStream_t s = (hipStream_t)stream;
    const int64_t t2n = (N + BN2 - 1) / BN2;
    const Nt8pTile t(nt8p_pick_rt(M, t2n, 256), M);
    if (accumulate) launch_nt8p<true, true, true, 0>(t, t2n, t.t2m * t2n, s, A, B, C, nullptr, nullptr, M, N, K, lda, ldb, ldc, b_rows, GemmEpi{});
    else launch_nt8p<true, false, true, 0>(t, t2n, t.t2m * t2n, s, A, B, C, nullptr, nullptr, M, N, K, lda, ldb, ldc, b_rows, GemmEpi{});
    TR1_LAUNCH_CHECK();
}

// Weight gradient C[M, N] fp32 (+)= A B^T (b_kmajor = 0: B = X^T [N, K]) or A B (b_kmajor = 1: B = X as stored [K, N], its first b_rows rows valid), on the
// phased 8-wave kernel, which ALSO leaves the sum of squares of every value it stored in sumsq_partials (one float per wave: 8 x blocks; *n_partials receives
// the count) - in the last micro-step of an accumulation window that is the squared norm of the final gradient, so the optimizer's grad-norm pass does not
// have to read these matrices again.  Same kernel, k order and (for shapes the NT dispatch gives to the 8-wave tiles) tile choice as tr1_gemm_nt_bf16(out_f32) / tr1_gemm_nn_acc_f32: bit-identical C.
extern "C" int tr1_wgrad_f32_sumsq(const void* A, const void* B, void* C, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc, int accumulate,
                                   int b_kmajor, int64_t b_rows, void* sumsq_partials, int64_t partials_capacity, int64_t* n_partials, void* wire_bf16, int64_t ld_wire,
                                   void* stream) {
    TR1_CHECK_ARG(K % BK == 0 && N % 8 == 0 && lda % 8 == 0 && ldb % 8 == 0 && ldc % 4 == 0, "wgrad_f32_sumsq: K%64, N%8, lda%8, ldb%8, ldc%4 required");
    TR1_CHECK_ARG(M >= 512 && N >= 256, "wgrad_f32_sumsq: M >= 512 and N >= 256 required (smaller gradients: plain GEMM + tr1_sumsq_accum)");
    TR1_CHECK_ARG(!b_kmajor || (b_rows >= 1 && b_rows <= K), "wgrad_f32_sumsq: 1 <= b_rows <= K");
    TR1_CHECK_ARG(sumsq_partials && n_partials, "wgrad_f32_sumsq: partials buffer required");
    hipStream_t s = (hipStream_t)stream;
    const int64_t t2n = (N + BN2 - 1) / BN2;
    const Nt8pTile t(nt8p_pick_rt(M, t2n, b_kmajor ? 256 : 224), M);      // each operand form picks like its plain GEMM (tr1_gemm_nn_acc_f32 / the NT dispatch): bit-identical C
    const int64_t blocks = t.t2m * t2n;
    TR1_CHECK_ARG(blocks * 8 <= partials_capacity, "wgrad_f32_sumsq: partials buffer too small (8 floats per 256-column tile block)");
    TR1_CHECK_ARG(!wire_bf16 || ld_wire % 4 == 0, "wgrad_f32_sumsq: ld_wire % 4 required");
    GemmEpi ep{}; ep.p0 = sumsq_partials; ep.p1 = wire_bf16; ep.ld1 = ld_wire;
    auto go = [&](auto AC, auto KM) {
        launch_nt8p<true, decltype(AC)::value, decltype(KM)::value, 0>(t, t2n, blocks, s, A, B, C, nullptr, nullptr, M, N, K, lda, ldb, ldc, b_kmajor ? b_rows : 0, ep);
    };
    if (b_kmajor) { if (accumulate) go(std::true_type{}, std::true_type{}); else go(std::false_type{}, std::true_type{}); }
    else { if (accumulate) go(std::true_type{}, std::false_type{}); else go(std::false_type{}, std::false_type{}); }
    *n_partials = blocks * 8;
    TR1_LAUNCH_CHECK();
}

// ---- fused-epilogue training GEMMs (EPI 2 / 3 / 4 of gemm_nt8p_kernel) ----------------------------------------------------------------
// a[M, I] = silu(x Wg^T) * (x Wu^T) with Wgu = [2I, K] (gate rows, then up rows); gu_out (optional) receives the projection itself [M, 2I] for the backward.
// Bit-identical to tr1_gemm_nt_bf16 + tr1_swiglu_fwd.
extern "C" int tr1_gemm_glu_bf16(const void* x, const void* Wgu, const void* bias, void* a_out, void* gu_out, int64_t M, int64_t I, int64_t K, int64_t ldx,
                                 int64_t ldw, int64_t lda, int64_t ldgu, void* stream) {
    TR1_CHECK_ARG(K % BK == 0 && I % 8 == 0 && ldx % 8 == 0 && ldw % 8 == 0 && lda % 8 == 0 && (!gu_out || ldgu % 8 == 0), "gemm_glu: K%64, I%8, ld%8 required");
    TR1_CHECK_ARG(I < (1 << 30), "gemm_glu: I too large");
    if (M == 0 || I == 0) return 0;
    const int64_t t2n = (I + 127) / 128;
    const Nt8pTile t(nt8p_pick_rt(M, t2n, 256), M);
    GemmEpi ep{}; ep.p0 = gu_out; ep.ld0 = ldgu; ep.i0 = (int)I;
    launch_nt8p<false, false, false, 2>(t, t2n, t.t2m * t2n, (hipStream_t)stream, x, Wgu, a_out, bias, nullptr, M, 2 * I, K, ldx, ldw, lda, 0, ep);
    TR1_LAUNCH_CHECK();
}

// y[M, N] = quick_gelu(x W^T + bias) (Qwen2-VL vision MLP fc1 + activation, TF:300-301).  Bit-identical to tr1_gemm_nt_bf16 (bias) + tr1_quickgelu_fwd.
extern "C" int tr1_gemm_bias_quickgelu_bf16(const void* x, const void* W, const void* bias, void* y, int64_t M, int64_t N, int64_t K, int64_t ldx, int64_t ldw,
                                            int64_t ldy, void* stream) {
    TR1_CHECK_ARG(K % BK == 0 && N % 8 == 0 && ldx % 8 == 0 && ldw % 8 == 0 && ldy % 8 == 0, "gemm_bias_quickgelu: K%64, N%8, ld%8 required");
    if (M == 0 || N == 0) return 0;
    const int64_t t2n = (N + BN2 - 1) / BN2;
    const Nt8pTile t(nt8p_pick_rt(M, t2n, 256), M);
    launch_nt8p<false, false, false, 5>(t, t2n, t.t2m * t2n, (hipStream_t)stream, x, W, y, bias, nullptr, M, N, K, ldx, ldw, ldy, 0, GemmEpi{});
    TR1_LAUNCH_CHECK();
}

// Fused q|k|v projection + bias + M-RoPE for head dim 128: q_out[M, n_heads*128] and k_out[M, n_kv*128] rotated (cos / sin fp32 [M, 64]), v_out[M, n_kv*128]
// plain.  Bit-identical to tr1_gemm_nt_bf16 (bias) + tr1_rope_apply on the q and k columns.  n_heads and n_kv must be even (whole 256-column tiles).
extern "C" int tr1_gemm_qkv_rope_bf16(const void* x, const void* Wqkv, const void* bias, const void* cosb, const void* sinb, void* q_out, int64_t ldq,
                                      void* k_out, int64_t ldk, void* v_out, int64_t ldv, int64_t M, int64_t n_heads, int64_t n_kv, int64_t head_dim,
                                      int64_t K, int64_t ldx, int64_t ldw, void* stream) {
    TR1_CHECK_ARG(head_dim == 128 && n_heads % 2 == 0 && n_kv % 2 == 0, "gemm_qkv_rope: head_dim 128 and even head counts required");
    TR1_CHECK_ARG(K % BK == 0 && ldx % 8 == 0 && ldw % 8 == 0 && ldq % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0, "gemm_qkv_rope: K%64, ld%8 required");
    if (M == 0) return 0;
    const int64_t N = (n_heads + 2 * n_kv) * 128, t2n = N / 256;
    const Nt8pTile t(nt8p_pick_rt(M, t2n, 256), M);
    GemmEpi ep{}; ep.p0 = k_out; ep.ld0 = ldk; ep.p1 = v_out; ep.ld1 = ldv; ep.f0 = (const float*)cosb; ep.f1 = (const float*)sinb;
    ep.i0 = (int)(n_heads * 128); ep.i1 = (int)(n_kv * 128);
    launch_nt8p<false, false, false, 4>(t, t2n, t.t2m * t2n, (hipStream_t)stream, x, Wqkv, q_out, bias, nullptr, M, N, K, ldx, ldw, ldq, 0, ep);
    TR1_LAUNCH_CHECK();
}

// Vision-tower attention input (Qwen2-VL / Qwen2.5-VL blocks, head dim 2 * half = 80): fused q|k|v projection + bias + 2-D rotary embedding (cos / sin fp32
// [M, half]), written as 128-wide zero-PADDED heads q128 / k128 / v128 [M, n_heads * 128] (feature d < half at d, d + half at 64 + d; the caller zero-fills
// the buffers once).  Values bit-identical to tr1_gemm_nt_bf16 (bias) + tr1_rope_apply on q and k.  n_heads * half must be a multiple of 128.
extern "C" int tr1_gemm_qkv_rope_vit_bf16(const void* x, const void* Wqkv, const void* bias, const void* cosb, const void* sinb, void* q128, int64_t ldq,
                                          void* k128, int64_t ldk, void* v128, int64_t ldv, int64_t M, int64_t n_heads, int64_t half, int64_t K,
                                          int64_t ldx, int64_t ldw, void* stream) {
    TR1_CHECK_ARG(half % 8 == 0 && half <= 64 && (n_heads * half) % 128 == 0, "gemm_qkv_rope_vit: half % 8 == 0, half <= 64, n_heads * half % 128 == 0 required");
    TR1_CHECK_ARG(K % BK == 0 && ldx % 8 == 0 && ldw % 8 == 0 && ldq % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0, "gemm_qkv_rope_vit: K%64, ld%8 required");
    if (M == 0) return 0;
    const int64_t pairs = n_heads * half, N = 6 * pairs, t2n = N / 256;
    const Nt8pTile t(nt8p_pick_rt(M, t2n, 256), M);
    GemmEpi ep{}; ep.p0 = k128; ep.ld0 = ldk; ep.p1 = v128; ep.ld1 = ldv; ep.f0 = (const float*)cosb; ep.f1 = (const float*)sinb;
    ep.i0 = (int)pairs; ep.i1 = (int)half;
    launch_nt8p<false, false, false, 7>(t, t2n, t.t2m * t2n, (hipStream_t)stream, x, Wqkv, q128, bias, nullptr, M, N, K, ldx, ldw, ldq, 0, ep);
    TR1_LAUNCH_CHECK();
}

// dgu[M, 2I] = SwiGLU backward of da = dh[M, H] * Wd[H, I] (Wd = the down projection as stored, K-major operand), with gu[M, 2I] the saved projection.
// Bit-identical to tr1_gemm_nn_bf16 + tr1_swiglu_bwd; da never exists in HBM.
extern "C" int tr1_gemm_nn_glubwd_bf16(const void* dh, const void* Wd, const void* gu, void* dgu, int64_t M, int64_t I, int64_t H, int64_t lda, int64_t ldb,
                                       int64_t ldgu, int64_t lddgu, void* dgu_t, int64_t ld_t, void* stream) {
    TR1_CHECK_ARG(!dgu_t || (ld_t % 64 == 0 && ld_t >= M && ld_t < M + 64), "gemm_nn_glubwd: dgu^T needs ld_t = tokens rounded up to 64");
    TR1_CHECK_ARG(H % BK == 0 && I % 8 == 0 && lda % 8 == 0 && ldb % 8 == 0 && ldgu % 8 == 0 && lddgu % 8 == 0, "gemm_nn_glubwd: H%64, I%8, ld%8 required");
    TR1_CHECK_ARG(M >= 512 && I >= 256, "gemm_nn_glubwd: M >= 512 and I >= 256 required");
    const int64_t t2n = (I + BN2 - 1) / BN2;
    const Nt8pTile t(nt8p_pick_rt(M, t2n, 256), M);
    GemmEpi ep{}; ep.p0 = const_cast<void*>(gu); ep.ld0 = ldgu; ep.i0 = (int)I; ep.p1 = dgu_t; ep.ld1 = ld_t;
    launch_nt8p<false, false, true, 3>(t, t2n, t.t2m * t2n, (hipStream_t)stream, dh, Wd, dgu, nullptr, nullptr, M, I, H, lda, ldb, lddgu, 0, ep);
    TR1_LAUNCH_CHECK();
}

// C[M, N] (bf16) = A B^T or A B (+bias)(+residual) with a deterministic S-way split over K: thin outputs over a long K leave most CUs idle in the plain
// forms - the continuation forward's down projection (1600 x 3584 x 18944: 98 tiles of 256 x 256 for 256 CUs, 838 TFLOP/s), its o projection, and the
// lm_head's data gradient (1600 x 3584 over K = 152064, which used to pay a 2.2 GB transpose of the lm_head weight in front of a 128 x 128-tile GEMM).
// All S shares of the reduction run as blocks of ONE launch into fp32 planes of ws_f32, a second launch adds the planes in a fixed order.  (RT, S) by the
// cost model below: rounds of 256 blocks x tile rows x k tiles per share.  b_kmajor: B = [K, N] as stored (the weight itself in a dgrad).
// K must hold at least two k tiles (K >= 2 * 64) and S never exceeds the number of k tiles: every share owns at least one tile.  (A share of no tiles
// would still run the kernel's prologue, which stages tile 0 of its share - 128 bytes past the end of every row of A and B.)
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const float* __restrict__ planes, int S, int64_t plane, const bf16_t* __restrict__ bias,
                                                            const bf16_t* __restrict__ residual, int64_t ldr, bf16_t* __restrict__ C, int64_t ldc, int64_t M, int64_t N) {
    const int64_t nch = N >> 3, total = M * nch;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t m = i / nch, n = (i - m * nch) * 8;
        const float* p = planes + m * N + n;
        f32x4_t a0 = *reinterpret_cast<const f32x4_t*>(p), a1 = *reinterpret_cast<const f32x4_t*>(p + 4);
        for (int z = 1; z < S; ++z) {
            a0 += *reinterpret_cast<const f32x4_t*>(p + z * plane); a1 += *reinterpret_cast<const f32x4_t*>(p + z * plane + 4);
        }
        float v[8] = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
        if (bias) {
            const u32x4_t bv = *reinterpret_cast<const u32x4_t*>(bias + n);
#pragma unroll
            for (int e = 0; e < 4; ++e) { v[2 * e] += bflo(bv[e]); v[2 * e + 1] += bfhi(bv[e]); }
        }
        if (residual) {
            const u32x4_t rv = *reinterpret_cast<const u32x4_t*>(residual + m * ldr + n);
#pragma unroll
            for (int e = 0; e < 4; ++e) { v[2 * e] += bflo(rv[e]); v[2 * e + 1] += bfhi(rv[e]); }
        }
        u32x4_t o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = pack2bf(v[2 * e], v[2 * e + 1]);
        *reinterpret_cast<u32x4_t*>(C + m * ldc + n) = o;
    }
}
// (RT, S) for a split-K launch: minimise rounds(256 blocks) x tile rows x k tiles per share / efficiency, plus the partial planes' traffic
static void splitk_pick(int64_t M, int64_t N, int64_t K, int max_s, int* rt_out, int* s_out) {
    const int64_t t2n = (N + BN2 - 1) / BN2, nk = K / BK;
    double best = 1e300; int brt = 8, bs = 1;
    for (int r = 7; r <= 10; ++r)
        for (int S = 1; S <= max_s && S <= nk; ++S) {
            const int64_t tiles = ((M + r * 32 - 1) / (r * 32)) * t2n, blocks = tiles * S;
            const double rounds = (double)((blocks + 255) / 256), kshare = (double)((nk + S - 1) / S);
            // block time ~ rows x k tiles; a plane costs one fp32 write + read of M x N per share, priced against the GEMM's per-CU rate (~25 k-tile rows per 4 KB)
            const double c = rounds * (r * 32) * kshare / NT8P_EFF[r - 7] + (S > 1 ? 0.02 * S * (double)(M * N) / 256.0 / 64.0 : 0.0);
            if (c < best) { best = c; brt = r; bs = S; }
        }
    *rt_out = brt; *s_out = bs;
}
extern "C" int64_t tr1_gemm_splitk_max_splits(void) { return 8; }
extern "C" int tr1_gemm_splitk_bf16(const void* A, const void* B, void* C, const void* bias, const void* residual, int64_t M, int64_t N, int64_t K,
                                    int64_t lda, int64_t ldb, int64_t ldc, int64_t ldr, int b_kmajor, void* ws_f32, int64_t ws_floats, void* stream) {
    TR1_CHECK_ARG(K % BK == 0 && N % 8 == 0 && lda % 8 == 0 && ldb % 8 == 0 && ldc % 8 == 0 && (!residual || ldr % 8 == 0), "gemm_splitk: K%64, N%8, ld%8 required");
    TR1_CHECK_ARG(ws_f32 && ws_floats >= 2 * M * N, "gemm_splitk: workspace of at least 2*M*N floats required (8*M*N for every split count)");
    TR1_CHECK_ARG(K >= 2 * BK, "gemm_splitk: K >= 128 required (two k tiles: one per share of the smallest split)");
    if (M == 0 || N == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    int rt, S;
    const int64_t max_s = ws_floats / (M * N);
    splitk_pick(M, N, K, (int)(max_s < 8 ? max_s : 8), &rt, &S);
    if (S < 2) S = 2;        // (the caller asked for the split form: thin outputs; S = 1 would be the plain GEMM); K >= 2 * BK above keeps S <= nk
    TR1_CHECK_ARG(S <= K / BK, "gemm_splitk: more shares than k tiles");
    const int64_t t2n = (N + BN2 - 1) / BN2;
    const Nt8pTile t(rt, M);
    GemmEpi ep{}; ep.ld0 = M * N; ep.i0 = S;
    if (b_kmajor) launch_nt8p<true, false, true, 6>(t, t2n, S * t.t2m * t2n, s, A, B, ws_f32, nullptr, nullptr, M, N, K, lda, ldb, N, 0, ep);
    else launch_nt8p<true, false, false, 6>(t, t2n, S * t.t2m * t2n, s, A, B, ws_f32, nullptr, nullptr, M, N, K, lda, ldb, N, 0, ep);
    hipLaunchKernelGGL(splitk_reduce_kernel, dim3(tr1_grid_1d(M * N / 8, 256, 2048)), dim3(256), 0, s, (const float*)ws_f32, S, M * N,
                       (const bf16_t*)bias, (const bf16_t*)residual, ldr, (bf16_t*)C, ldc, M, N);
    TR1_LAUNCH_CHECK();
}

// ---- lm_head -> (log-prob of the target, entropy, LSE) without materialised logits --------------------------------------------------
// ref: _get_per_token_logps (src/time_r1/rl/timer1_trainer.py:449-481) computes logits [G, L, V], log_softmax, gather and entropy; here the
// GEMM epilogue reduces every 64-column slice of a row to (max, sum e, sum x e) and this kernel merges the V / 64 slices of a row.
__global__ __launch_bounds__(256) void lse_combine_kernel(const f32x4_t* __restrict__ part, int64_t ncb, float* __restrict__ logp, float* __restrict__ ent,
                                                          float* __restrict__ lse_out) {
    __shared__ float red[16];
    const int64_t row = blockIdx.x;
    const f32x4_t* pr = part + row * (ncb + 1);
    float mx = -INFINITY;
    for (int64_t i = threadIdx.x; i < ncb; i += 256) mx = fmaxf(mx, pr[i][0]);
    mx = block_max(mx, red);
    __syncthreads();
    float se = 0.f, te = 0.f;
    for (int64_t i = threadIdx.x; i < ncb; i += 256) {
        const f32x4_t v = pr[i];
        const float w = (v[0] == -INFINITY) ? 0.f : __expf(v[0] - mx);
        se += v[1] * w; te += v[2] * w;
    }
    se = block_sum(se, red);
    __syncthreads();
    te = block_sum(te, red);
    if (threadIdx.x == 0) {
        const float l = mx + logf(se);
        const float xt = reinterpret_cast<const float*>(pr + ncb)[0];
        lse_out[row] = l; logp[row] = xt - l; ent[row] = l - te / se;
    }
}

extern "C" int64_t tr1_lmhead_lse_workspace_floats(int64_t M, int64_t N) { return M * ((N + 63) / 64 + 1) * 4; }

// hn [M, K] bf16 (final-norm output of the prediction rows), W [N, K] bf16 (lm_head), targets int32 [M]  ->  logp, entropy, lse fp32 [M].
extern "C" int tr1_lmhead_lse_fwd(const void* hn, const void* W, const void* targets, void* part_ws, int64_t ws_floats, void* logp, void* ent,
                                  void* lse, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, void* stream) {
    TR1_CHECK_ARG(K % BK == 0 && N % 64 == 0 && lda % 8 == 0 && ldb % 8 == 0, "lmhead_lse: K % 64, N % 64, lda % 8, ldb % 8 required");
    TR1_CHECK_ARG(part_ws && ws_floats >= tr1_lmhead_lse_workspace_floats(M, N), "lmhead_lse: workspace too small");
    if (M == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const int64_t ncb = N / 64;
    const int64_t t2n = (N + BN2 - 1) / BN2;
    const Nt8pTile t(nt8p_pick_rt(M, t2n, 256), M);
    // EPI 1: `bias` carries the int32 targets, C the float4 partials with ldc = column blocks per row + the target's slot
    launch_nt8p<false, false, false, 1>(t, t2n, t.t2m * t2n, s, hn, W, part_ws, targets, nullptr, M, N, K, lda, ldb, ncb + 1, 0, GemmEpi{});
    hipLaunchKernelGGL(lse_combine_kernel, dim3((unsigned)M), dim3(256), 0, s, (const f32x4_t*)part_ws, ncb, (float*)logp, (float*)ent, (float*)lse);
    TR1_LAUNCH_CHECK();
}
