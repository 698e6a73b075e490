// LoRA (peft_config): the two kernels of the merged-adapter design.
//   tr1_lora_merge : W = bf16_rne(W0 + s * Bt^T A) for one targeted projection (or a row slice of the fused qkv / gate-up matrix), from the frozen base copy
//                    and the fp32 adapter masters - run after every optimizer step, never as a delta.
//   tr1_lora_wgrad : G[r, Wd] (+)= scale * thin[M, r]^T wide[M, Wd], the rank-r weight gradients dBt = s u^T dY and dA = s v^T x that replace the full-size
//                    weight-gradient GEMMs; both operands are read as stored (the reduction runs over their rows), once.
// ref: peft.tuners.lora.Linear (merge: weight + scaling * B @ A; forward: result + lora_B(lora_A(x)) * scaling), reached from the reference through
// get_peft_config(model_args) (src/time_r1/main.py) and GRPOTrainer's peft_config argument (src/time_r1/rl/timer1_trainer.py:290-293).
#include "tr1_common.h"
#include "../../include/timer1_hip.h"

// ------------------------------------------------------------------------------------------------------------------ merge
// Arithmetic, pinned (no fma contraction, as ref_mix / adamw_step_sr16): acc = 0; for j ascending: acc = fadd(acc, fmul(Bt[j, o], A[j, i]));
// y = fadd(w0, fmul(s, acc)); W = bf16_rne(y).  An fp32 torch loop over j reproduces it bit for bit.
TR1_DEV float lora_mac(float acc, float b, float a) {
#pragma clang fp contract(off)
    const float t = b * a;
    return acc + t;
}
TR1_DEV float lora_out(float w0, float s, float acc) {
#pragma clang fp contract(off)
    const float t = s * acc;
    return w0 + t;
}
// A block owns 64 rows (o) x 128 columns (i): thread (ty, tx) of 16 x 16 computes rows 4 ty .. 4 ty + 3 x columns 8 tx .. 8 tx + 7, so one rank step costs it
// three 16-byte LDS reads for 64 arithmetic instructions.  LDS: the A tile as [j][half][tx] float4 (a half-wave's 16-byte reads are contiguous) and the Bt tile
// as [j][64] floats; r * 768 bytes (48 KiB at r = 64).  HBM: 4 B per element of W (W0 read, W written, 16 bytes per thread and row) + the adapter tiles.
constexpr int LM_ROWS = 64, LM_COLS = 128;
__global__ __launch_bounds__(256) void lora_merge_kernel(bf16_t* __restrict__ W, int64_t ldw, const bf16_t* __restrict__ W0, int64_t ldw0, const float* __restrict__ A,
                                                         const float* __restrict__ Bt, int64_t out, int64_t in, int r, float s) {
    extern __shared__ __attribute__((aligned(16))) char lm_lds[];
    f32x4_t* a_s = reinterpret_cast<f32x4_t*>(lm_lds);                      // [r][2][16]
    float* bt_s = reinterpret_cast<float*>(lm_lds + (size_t)r * LM_COLS * 4);      // [r][64]
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int64_t i0 = (int64_t)blockIdx.x * LM_COLS, o0 = (int64_t)blockIdx.y * LM_ROWS;
    for (int idx = tid; idx < r * 32; idx += 256) {
        const int j = idx >> 5, c4 = idx & 31;
        const int64_t col = i0 + c4 * 4;
        f32x4_t v = {0.f, 0.f, 0.f, 0.f};
        if (col + 4 <= in) v = *reinterpret_cast<const f32x4_t*>(A + (int64_t)j * in + col);
        a_s[(j * 2 + (c4 & 1)) * 16 + (c4 >> 1)] = v;
    }
    for (int idx = tid; idx < r * LM_ROWS; idx += 256) {
        const int j = idx >> 6, oo = idx & 63;
        bt_s[idx] = (o0 + oo < out) ? Bt[(int64_t)j * out + o0 + oo] : 0.f;
    }
    __syncthreads();
    float acc[4][8];
#pragma unroll
    for (int rr = 0; rr < 4; ++rr)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[rr][e] = 0.f;
#pragma unroll 2
    for (int j = 0; j < r; ++j) {
        const f32x4_t a0 = a_s[(j * 2) * 16 + tx], a1 = a_s[(j * 2 + 1) * 16 + tx];
        const f32x4_t b = *reinterpret_cast<const f32x4_t*>(bt_s + j * LM_ROWS + ty * 4);
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                acc[rr][e] = lora_mac(acc[rr][e], b[rr], a0[e]);
                acc[rr][4 + e] = lora_mac(acc[rr][4 + e], b[rr], a1[e]);
            }
        }
    }
    const int64_t col = i0 + tx * 8;
    if (col + 8 > in) return;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        const int64_t o = o0 + ty * 4 + rr;
        if (o >= out) break;
        const u32x4_t w0 = *reinterpret_cast<const u32x4_t*>(W0 + o * ldw0 + col);
        u32x4_t y;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            y[e] = pack2bf(lora_out(bflo(w0[e]), s, acc[rr][2 * e]), lora_out(bfhi(w0[e]), s, acc[rr][2 * e + 1]));
        *reinterpret_cast<u32x4_t*>(W + o * ldw + col) = y;
    }
}

extern "C" int tr1_lora_merge(void* W_bf16, int64_t ldw, const void* W0_bf16, int64_t ldw0, const void* A_f32, const void* Bt_f32, int64_t out, int64_t in, int64_t r,
                              float s, void* stream) {
    TR1_CHECK_ARG(out >= 0 && in >= 0 && (r == 16 || r == 32 || r == 64), "lora_merge: r must be 16, 32 or 64 (rank 8 is stored as 16 rows, the upper 8 zero)");
    if (out == 0 || in == 0) return 0;
    TR1_CHECK_ARG(W_bf16 && W0_bf16 && A_f32 && Bt_f32 && W_bf16 != W0_bf16, "lora_merge: null pointer, or W aliases W0 (the merge reads the base copy)");
    TR1_CHECK_ARG(in % 8 == 0 && ldw % 8 == 0 && ldw0 % 8 == 0 && ldw >= in && ldw0 >= in, "lora_merge: in, ldw, ldw0 must be multiples of 8 and ld >= in");
    TR1_CHECK_ARG((((uintptr_t)W_bf16 | (uintptr_t)W0_bf16 | (uintptr_t)A_f32) & 15) == 0 && ((uintptr_t)Bt_f32 & 3) == 0, "lora_merge: W, W0, A must be 16-byte aligned");
    const dim3 grid((unsigned)((in + LM_COLS - 1) / LM_COLS), (unsigned)((out + LM_ROWS - 1) / LM_ROWS));
    TR1_CHECK_ARG((out + LM_ROWS - 1) / LM_ROWS <= 65535, "lora_merge: more than 65535 x 64 rows");
    const size_t lds = (size_t)r * (LM_COLS + LM_ROWS) * 4;
    hipLaunchKernelGGL(lora_merge_kernel, grid, dim3(256), lds, (hipStream_t)stream, (bf16_t*)W_bf16, ldw, (const bf16_t*)W0_bf16, ldw0, (const float*)A_f32,
                       (const float*)Bt_f32, out, in, (int)r, s);
    TR1_LAUNCH_CHECK();
}

// ------------------------------------------------------------------------------------------------------------------ rank-r weight gradient
// G[i, n] (+)= scale * sum_m thin[m, i] wide[m, n].  D = A B on the 16x16x32 bf16 MFMA with A = thin^T and B = wide: BOTH operands are K-major here (k = the row
// m of either array), so a block stages [128 rows][r] of thin and [128 rows][64 columns] of wide row-major in LDS and every fragment is a transposing read
// (ds_read_b64_tr_b16, as the K-major GEMM's B operand, gemm.hip): lane (g, t) of a wave takes rows 8 g + t / 4 and + 4 of a 32-row step for both operands, so
// the two fragments pair the same k whatever order the hardware numbers them in.  Wave w of the 4 owns columns 16 w .. 16 w + 15 of the block's 64, all r rows.
// The split over M is a fixed function of (M, Wd): TR1_LORA_WGRAD_MCHUNK-row chunks dealt to S splits so that about TR1_LORA_WGRAD_BLOCKS blocks exist (see
// lora_wgrad_splits); S = 1 stores G directly, S > 1 leaves fp32 planes in ws that a second launch adds in ascending order: same inputs, same bits.
// Rows past a split's end and columns past Wd are staged as zeros (never read past either operand); their outputs are not stored.
TR1_DEV bf16x8_t lora_frag(const char* p, int stride) {
    const u32x2_t lo = tr1_lds_read_tr16(p), hi = tr1_lds_read_tr16(p + 4 * stride);
    const u32x4_t w = {lo[0], lo[1], hi[0], hi[1]};
    return __builtin_bit_cast(bf16x8_t, w);
}
constexpr int LW_COLS = 64, LW_KSTEP = 128, LW_WSTRIDE = LW_COLS * 2 + 16;      // bytes per staged row of wide (16 bytes of padding)
static_assert(TR1_LORA_WGRAD_MCHUNK % LW_KSTEP == 0 && TR1_LORA_WGRAD_COLS == LW_COLS, "include/timer1_hip.h states the split geometry of tr1_lora_wgrad");

template <int R>
__global__ __launch_bounds__(256) void lora_wgrad_kernel(float* __restrict__ G, int64_t ldg, float* __restrict__ planes, const bf16_t* __restrict__ thin, int64_t ldt,
                                                         const bf16_t* __restrict__ wide, int64_t ldw, int64_t M, int64_t Wd, int64_t rows_per_split, float scale,
                                                         int accumulate) {
    constexpr int TSTRIDE = R * 2 + 16, TN = R / 16, TCH = R / 8;
    __shared__ __attribute__((aligned(16))) char w_s[LW_KSTEP * LW_WSTRIDE];
    __shared__ __attribute__((aligned(16))) char t_s[LW_KSTEP * TSTRIDE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t n0 = (int64_t)blockIdx.x * LW_COLS;
    const int64_t m_begin = (int64_t)blockIdx.y * rows_per_split;
    const int64_t m_end = (m_begin + rows_per_split < M) ? m_begin + rows_per_split : M;
    f32x4_t acc[TN];
#pragma unroll
    for (int i = 0; i < TN; ++i) acc[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    u32x4_t wreg[4], treg[TN];
    auto load = [&](int64_t m0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = tid + 256 * i;
            const int64_t m = m0 + (c >> 3), col = n0 + (c & 7) * 8;
            wreg[i] = u32x4_t{0u, 0u, 0u, 0u};
            if (m < m_end && col < Wd) wreg[i] = *reinterpret_cast<const u32x4_t*>(wide + m * ldw + col);
        }
#pragma unroll
        for (int i = 0; i < TN; ++i) {
            const int c = tid + 256 * i;
            const int64_t m = m0 + c / TCH;
            treg[i] = u32x4_t{0u, 0u, 0u, 0u};
            if (m < m_end) treg[i] = *reinterpret_cast<const u32x4_t*>(thin + m * ldt + (c % TCH) * 8);
        }
    };
    const int g = lane >> 4, t = lane & 15;
    load(m_begin);
    for (int64_t m0 = m_begin; m0 < m_end; m0 += LW_KSTEP) {       // block-uniform trip count: every lane of every wave stays active (the transposing reads need that)
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = tid + 256 * i;
            *reinterpret_cast<u32x4_t*>(w_s + (c >> 3) * LW_WSTRIDE + (c & 7) * 16) = wreg[i];
        }
#pragma unroll
        for (int i = 0; i < TN; ++i) {
            const int c = tid + 256 * i;
            *reinterpret_cast<u32x4_t*>(t_s + (c / TCH) * TSTRIDE + (c % TCH) * 16) = treg[i];
        }
        __syncthreads();
        if (m0 + LW_KSTEP < m_end) load(m0 + LW_KSTEP);            // the next step's rows travel while this one is multiplied
#pragma unroll
        for (int ks = 0; ks < LW_KSTEP / 32; ++ks) {
            const int row = ks * 32 + 8 * g + (t >> 2);
            const bf16x8_t bf = lora_frag(w_s + row * LW_WSTRIDE + (wave * 16 + 4 * (t & 3)) * 2, LW_WSTRIDE);
#pragma unroll
            for (int rt = 0; rt < TN; ++rt) {
                const bf16x8_t af = lora_frag(t_s + row * TSTRIDE + (rt * 16 + 4 * (t & 3)) * 2, TSTRIDE);
                acc[rt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bf, acc[rt], 0, 0, 0);
            }
        }
    }
    const int64_t n = n0 + wave * 16 + t;
    if (n >= Wd) return;
#pragma unroll
    for (int rt = 0; rt < TN; ++rt)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int i = rt * 16 + g * 4 + e;
            if (planes) {
                planes[((int64_t)blockIdx.y * R + i) * Wd + n] = acc[rt][e];
            } else {
                float* p = G + (int64_t)i * ldg + n;
                const float v = scale * acc[rt][e];
                *p = accumulate ? *p + v : v;
            }
        }
}
// G[i, n] (+)= scale * (plane 0 + plane 1 + ... + plane S - 1)[i, n], planes added in ascending order
__global__ __launch_bounds__(256) void lora_wgrad_reduce_kernel(float* __restrict__ G, int64_t ldg, const float* __restrict__ planes, int S, int64_t r, int64_t Wd,
                                                                float scale, int accumulate) {
    const int64_t total = r * Wd;
    for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        float sum = planes[idx];
        for (int z = 1; z < S; ++z) sum += planes[z * total + idx];
        const int64_t i = idx / Wd, n = idx - i * Wd;
        float* p = G + i * ldg + n;
        const float v = scale * sum;
        *p = accumulate ? *p + v : v;
    }
}
// (splits, rows per split) of an [M, Wd] problem: whole chunks of TR1_LORA_WGRAD_MCHUNK rows, as many splits as bring the launch to about
// TR1_LORA_WGRAD_BLOCKS blocks and no more than there are chunks.  HipOps.lora_wgrad_splits is the same arithmetic (it sizes the workspace).
static void lora_wgrad_splits(int64_t M, int64_t Wd, int64_t* S, int64_t* rows) {
    const int64_t ntile = (Wd + LW_COLS - 1) / LW_COLS, nchunk = (M + TR1_LORA_WGRAD_MCHUNK - 1) / TR1_LORA_WGRAD_MCHUNK;
    int64_t want = TR1_LORA_WGRAD_BLOCKS / ntile;
    if (want < 1) want = 1;
    if (want > nchunk) want = nchunk;
    const int64_t per = (nchunk + want - 1) / want;
    *S = (nchunk + per - 1) / per;
    *rows = per * TR1_LORA_WGRAD_MCHUNK;
}

extern "C" int tr1_lora_wgrad(void* G_f32, int64_t ldg, const void* thin_bf16, int64_t ldt, const void* wide_bf16, int64_t ldw, int64_t M, int64_t Wd, int64_t r,
                              float scale, int accumulate, void* ws_f32, int64_t ws_floats, void* stream) {
    TR1_CHECK_ARG(M >= 1 && Wd >= 8 && (r == 16 || r == 32 || r == 64), "lora_wgrad: M >= 1, Wd >= 8 and r in {16, 32, 64} required");
    TR1_CHECK_ARG(G_f32 && thin_bf16 && wide_bf16, "lora_wgrad: null pointer");
    TR1_CHECK_ARG(Wd % 8 == 0 && ldw % 8 == 0 && ldt % 8 == 0 && ldw >= Wd && ldt >= r && ldg >= Wd, "lora_wgrad: Wd, ldw, ldt must be multiples of 8; ld >= width");
    TR1_CHECK_ARG((((uintptr_t)thin_bf16 | (uintptr_t)wide_bf16) & 15) == 0 && ((uintptr_t)G_f32 & 3) == 0, "lora_wgrad: thin and wide must be 16-byte aligned");
    int64_t S, rows;
    lora_wgrad_splits(M, Wd, &S, &rows);
    TR1_CHECK_ARG(S <= 65535, "lora_wgrad: too many splits");
    float* planes = nullptr;
    if (S > 1) {
        TR1_CHECK_ARG(ws_f32 && ws_floats >= S * r * Wd, "lora_wgrad: workspace too small (splits x r x Wd floats)");
        planes = (float*)ws_f32;
    }
    const dim3 grid((unsigned)((Wd + LW_COLS - 1) / LW_COLS), (unsigned)S);
    hipStream_t s = (hipStream_t)stream;
#define LORA_WGRAD_LAUNCH(R)                                                                                                                       \
    hipLaunchKernelGGL(lora_wgrad_kernel<R>, grid, dim3(256), 0, s, (float*)G_f32, ldg, planes, (const bf16_t*)thin_bf16, ldt, (const bf16_t*)wide_bf16, ldw, M, Wd, \
                       rows, scale, accumulate)
    if (r == 16) LORA_WGRAD_LAUNCH(16);
    else if (r == 32) LORA_WGRAD_LAUNCH(32);
    else LORA_WGRAD_LAUNCH(64);
#undef LORA_WGRAD_LAUNCH
    if (S > 1)
        hipLaunchKernelGGL(lora_wgrad_reduce_kernel, dim3(tr1_grid_1d(r * Wd, 256, 1024)), dim3(256), 0, s, (float*)G_f32, ldg, (const float*)planes, (int)S, r, Wd, scale,
                           accumulate);
    TR1_LAUNCH_CHECK();
}
