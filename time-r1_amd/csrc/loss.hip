// Vocabulary-side kernels of the GRPO step for gfx950: per-token log-prob + entropy over the lm_head logits (forward and
// backward) and the GRPO loss/gradient on [G, C] token grids.  (The rollout sampler lives in sampler.hip.)
//
// Reference semantics:
//   logp / entropy : src/time_r1/rl/timer1_trainer.py:458-481  (log_softmax, gather, H = -sum p log p)
//   KL (k3)        : :635-639        loss (both branches): :713-737
#include "tr1_common.h"
#include "../../include/timer1_hip.h"

// ---------------------------------------------------------------------------------------------------------------------
// One 256-thread block per row; single pass, online (max, sum exp, sum exp*x).  logits bf16 [R, V] with row stride ld.
// ---------------------------------------------------------------------------------------------------------------------
struct OnlineSE { float m, z, s; };  // running max, sum e^(x-m), sum e^(x-m)*x
TR1_DEV void ose_add(OnlineSE& a, float x) {
    if (x > a.m) { const float f = __expf(a.m - x); a.z = a.z * f + 1.f; a.s = a.s * f + x; a.m = x; }
    else { const float e = __expf(x - a.m); a.z += e; a.s += e * x; }
}
TR1_DEV void ose_merge(OnlineSE& a, const OnlineSE& b) {
    const float m = fmaxf(a.m, b.m);
    if (m == -INFINITY) return;
    const float fa = __expf(a.m - m), fb = __expf(b.m - m);
    a.z = a.z * fa + b.z * fb; a.s = a.s * fa + b.s * fb; a.m = m;
}

__global__ __launch_bounds__(256) void logp_entropy_fwd_kernel(const bf16_t* __restrict__ logits, int64_t ld, const int* __restrict__ targets,
                                                               float* __restrict__ logp, float* __restrict__ entropy, float* __restrict__ lse_out,
                                                               int V) {
    __shared__ float sm[3][4];
    const int r = blockIdx.x;
    const bf16_t* row = logits + (int64_t)r * ld;
    OnlineSE a = {-INFINITY, 0.f, 0.f};
    const int nch = V >> 3;
    for (int c = threadIdx.x; c < nch; c += 256) {
        const u32x4_t p = *reinterpret_cast<const u32x4_t*>(row + c * 8);
#pragma unroll
        for (int j = 0; j < 4; ++j) { ose_add(a, bflo(p[j])); ose_add(a, bfhi(p[j])); }
    }
    for (int i = nch * 8 + threadIdx.x; i < V; i += 256) ose_add(a, bf2f(row[i]));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        OnlineSE b = {__shfl_xor(a.m, o, 64), __shfl_xor(a.z, o, 64), __shfl_xor(a.s, o, 64)};
        ose_merge(a, b);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { sm[0][wave] = a.m; sm[1][wave] = a.z; sm[2][wave] = a.s; }
    __syncthreads();
    if (threadIdx.x == 0) {
        OnlineSE t = {sm[0][0], sm[1][0], sm[2][0]};
        for (int w = 1; w < 4; ++w) { OnlineSE b = {sm[0][w], sm[1][w], sm[2][w]}; ose_merge(t, b); }
        const float lse = t.m + __logf(t.z);
        const int tg = targets[r];
        logp[r] = bf2f(row[tg]) - lse;
        if (entropy) entropy[r] = lse - t.s / t.z;   // H = lse - E_p[x]
        if (lse_out) lse_out[r] = lse;
    }
}

// dlogits[r, v] = dlogp[r] * (1[v == target] - exp(x - lse))     (bf16 out, same shape/stride as logits; may alias logits)
__global__ void logp_bwd_kernel(const bf16_t* __restrict__ logits, int64_t ld, const int* __restrict__ targets, const float* __restrict__ lse,
                                const float* __restrict__ dlogp, bf16_t* __restrict__ dlogits, int64_t ld_out, int V) {
    const int r = blockIdx.y;
    const float g = dlogp[r], ls = lse[r];
    const int tg = targets[r];
    const bf16_t* row = logits + (int64_t)r * ld;
    bf16_t* orow = dlogits + (int64_t)r * ld_out;
    const int nch = V >> 3;
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < nch; c += gridDim.x * blockDim.x) {
        const u32x4_t p = *reinterpret_cast<const u32x4_t*>(row + c * 8);
        u32x4_t o;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int v0 = c * 8 + 2 * j;
            const float a = g * ((v0 == tg ? 1.f : 0.f) - __expf(bflo(p[j]) - ls));
            const float b = g * ((v0 + 1 == tg ? 1.f : 0.f) - __expf(bfhi(p[j]) - ls));
            o[j] = pack2bf(a, b);
        }
        *reinterpret_cast<u32x4_t*>(orow + c * 8) = o;
    }
}

// The same pass with a gradient arriving at the entropy as well (an entropy term in the loss: verl's entropy_coeff).  H = -sum_v p log p, so
// d H / d x_v = -p_v (log p_v + H) and
//   dlogits[r, v] = dlogp[r] * (1[v == target] - p) - dent[r] * p * ((x - lse[r]) + ent[r]),     p = exp(x - lse[r])
// lse and ent are the forward's outputs as they are (in the chunked backward they come from the fused lm_head and the logits from a second GEMM).  Grid, loads,
// stores and aliasing as logp_bwd_kernel; a row with dent[r] == 0 runs that kernel's expression, so it gives that kernel's values.
__global__ void logp_entropy_bwd_kernel(const bf16_t* __restrict__ logits, int64_t ld, const int* __restrict__ targets, const float* __restrict__ lse,
                                        const float* __restrict__ ent, const float* __restrict__ dlogp, const float* __restrict__ dent,
                                        bf16_t* __restrict__ dlogits, int64_t ld_out, int V) {
    const int r = blockIdx.y;
    const float g = dlogp[r], de = dent[r], ls = lse[r], H = ent[r];
    const int tg = targets[r];
    const bf16_t* row = logits + (int64_t)r * ld;
    bf16_t* orow = dlogits + (int64_t)r * ld_out;
    const int nch = V >> 3;
    const bool plain = de == 0.f;       // uniform over the block
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < nch; c += gridDim.x * blockDim.x) {
        const u32x4_t p = *reinterpret_cast<const u32x4_t*>(row + c * 8);
        u32x4_t o;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int v0 = c * 8 + 2 * j;
            const float la = bflo(p[j]) - ls, lb = bfhi(p[j]) - ls;
            const float pa = __expf(la), pb = __expf(lb);
            float a = g * ((v0 == tg ? 1.f : 0.f) - pa);
            float b = g * ((v0 + 1 == tg ? 1.f : 0.f) - pb);
            if (!plain) { a -= de * pa * (la + H); b -= de * pb * (lb + H); }
            o[j] = pack2bf(a, b);
        }
        *reinterpret_cast<u32x4_t*>(orow + c * 8) = o;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Top-entropy token selection (trl.GRPOConfig.top_entropy_quantile, get_high_entropy_mask): over the live positions (mask != 0) of ent[N], thr = the quantile of
// order q = 1 - rho with linear interpolation between the order statistics around pos = q (n - 1), as torch.quantile defines it; weight[i] = 1 where the position is
// live and ent[i] >= thr (ties kept), else 0; stats3 = {thr, number kept, n}.  n == 0: all zeros.  One 1024-thread block (N = G * C, a few tens of thousands at most):
//   1. n = number of live positions
//   2. radix select of the floor(pos)-th smallest value on an order-preserving 32-bit key (the sampler's bfkey for fp32; -0 is keyed as +0, so the order is the
//      floats' own), most significant byte first, one 256-bin LDS histogram per pass; the ceil(pos)-th is the same value when its ties reach that far, else the
//      smallest key above it (one more pass)
//   3. thr in fp64 with torch's lerp, the comparison in fp64, the count of kept positions
// Masked positions are never read.  Integer LDS atomics only (a histogram's counts do not depend on the order of arrival): same inputs, same bits.  No workspace.
// rho arrives as a float, so pos is known to (n - 1) 2^-23 only: a pos that close to an integer IS that integer (thr = an order statistic, and its ties are kept).
// ---------------------------------------------------------------------------------------------------------------------
TR1_DEV unsigned f32key(float x) {
    if (x == 0.f) x = 0.f;
    const unsigned u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
TR1_DEV float f32key_value(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
// by the block's first 256 threads (one bin each, ascending): the bin b with (count in bins < b) <= k < (count in bins <= b), and that first count.  k < the histogram's total.
TR1_DEV void eq_find_bin(const unsigned* hist, unsigned k, unsigned* scr, unsigned* bin_out, unsigned* below_out) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    unsigned val = 0u, incl = 0u;
    if (tid < 256) {
        val = hist[tid];
        incl = val;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const unsigned t = __shfl_up(incl, d, 64); if (lane >= d) incl += t; }
        if (lane == 63) scr[w] = incl;
    }
    __syncthreads();
    if (tid < 256) {
        unsigned off = 0u;
        for (int j = 0; j < w; ++j) off += scr[j];
        incl += off;
        const unsigned excl = incl - val;
        if (excl <= k && k < incl) { *bin_out = (unsigned)tid; *below_out = excl; }      // exactly one thread
    }
    __syncthreads();
}
__global__ __launch_bounds__(1024) void entropy_quantile_weight_kernel(const float* __restrict__ ent, const int* __restrict__ mask, float* __restrict__ weight,
                                                                       float* __restrict__ stats3, int N, float rho) {
    __shared__ unsigned hist[256], scr[4];
    __shared__ unsigned s_n, s_bin, s_below, s_min, s_kept;
    const int tid = threadIdx.x;
    if (tid == 0) { s_n = 0u; s_min = 0xffffffffu; s_kept = 0u; }
    __syncthreads();
    // ---- 1. live positions
    unsigned c = 0u;
    for (int i = tid; i < N; i += 1024) c += (mask[i] != 0) ? 1u : 0u;
    if (c) atomicAdd(&s_n, c);
    __syncthreads();
    const unsigned n = s_n;
    if (n == 0u) {
        for (int i = tid; i < N; i += 1024) weight[i] = 0.f;
        if (tid == 0) { stats3[0] = 0.f; stats3[1] = 0.f; stats3[2] = 0.f; }
        return;
    }
    // ---- 2. the two order statistics around pos (ascending ranks, from 0)
    double pos = (1.0 - (double)rho) * (double)(n - 1u);
    const double near = rint(pos);
    if (fabs(pos - near) <= (double)(n - 1u) * 0x1p-23) pos = near;
    const unsigned k_lo = (unsigned)floor(pos), k_hi = (unsigned)ceil(pos);
    const double frac = pos - (double)k_lo;
    unsigned prefix = 0u, pmask = 0u, k = k_lo, cnt_eq = 0u;
    for (int shift = 24; shift >= 0; shift -= 8) {
        if (tid < 256) hist[tid] = 0u;
        __syncthreads();
        for (int i = tid; i < N; i += 1024) {
            if (mask[i] == 0) continue;
            const unsigned key = f32key(ent[i]);
            if ((key & pmask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        eq_find_bin(hist, k, scr, &s_bin, &s_below);
        k -= s_below; prefix |= s_bin << shift; pmask |= 0xffu << shift;
        cnt_eq = hist[s_bin];
        __syncthreads();      // every thread has read the bin before the next pass clears the histogram
    }
    const unsigned key_lo = prefix;
    unsigned key_hi = key_lo;
    if (k_hi != k_lo && k + 1u >= cnt_eq) {      // k = rank of the floor statistic among its ties: the next rank leaves them
        unsigned mn = 0xffffffffu;
        for (int i = tid; i < N; i += 1024) {
            if (mask[i] == 0) continue;
            const unsigned key = f32key(ent[i]);
            if (key > key_lo) mn = min(mn, key);
        }
        if (mn != 0xffffffffu) atomicMin(&s_min, mn);
        __syncthreads();
        key_hi = s_min;
    }
    // ---- 3. threshold (torch's lerp), weights, count
    const double v_lo = (double)f32key_value(key_lo), v_hi = (double)f32key_value(key_hi);
    const double thr = frac < 0.5 ? v_lo + frac * (v_hi - v_lo) : v_hi - (v_hi - v_lo) * (1.0 - frac);
    unsigned kept = 0u;
    for (int i = tid; i < N; i += 1024) {
        float w = 0.f;
        if (mask[i] != 0 && (double)ent[i] >= thr) { w = 1.f; ++kept; }
        weight[i] = w;
    }
    if (kept) atomicAdd(&s_kept, kept);
    __syncthreads();
    if (tid == 0) { stats3[0] = (float)thr; stats3[1] = (float)s_kept; stats3[2] = (float)n; }
}

// ---------------------------------------------------------------------------------------------------------------------
// GRPO loss + d loss / d logp on the [G, C] grid (one block; G*C is a few thousand elements).
//   mode 1 (use_grpo): l = -(rho*A - beta*kl), loss = mean_g( sum_t l*m / sum_t m )
//   mode 0 (clip)    : l = -min(rho*A, clamp(rho,1-el,1+eh)*A) + beta*kl, loss = sum l*m / sum m
// rho = exp(logp - logp.detach()) == 1 in value; its gradient wrt logp is 1 (and the min/clamp pair passes the full
// gradient at rho == 1), so dl/dlogp = -A + beta*(1 - exp(ref - logp)).
// out[0] = loss, out[1] = mean_g(masked-mean kl), out[2] = sum of mask; row_len[g] = sum_t m.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void grpo_loss_kernel(const float* __restrict__ logp, const float* __restrict__ ref_logp,
                                                        const int* __restrict__ mask, const float* __restrict__ adv, float* __restrict__ dlogp,
                                                        float* __restrict__ out, float* __restrict__ row_len, float* __restrict__ row_kl, int G,
                                                        int C, float beta, int use_grpo, float grad_scale) {
    __shared__ float red[16];
    __shared__ float s_len[64], s_l[64], s_kl[64];
    float tot_mask = 0.f;
    for (int g = 0; g < G; ++g) {
        float len = 0.f, sl = 0.f, skl = 0.f;
        for (int t = threadIdx.x; t < C; t += blockDim.x) {
            const int i = g * C + t;
            const float m = (float)mask[i];
            float kl = 0.f;
            if (ref_logp) { const float d = ref_logp[i] - logp[i]; kl = __expf(d) - d - 1.f; }
            const float l = -adv[g] + beta * kl;
            len += m; sl += l * m; skl += kl * m;
        }
        len = block_sum(len, red); sl = block_sum(sl, red); skl = block_sum(skl, red);
        if (threadIdx.x == 0) { s_len[g] = len; s_l[g] = sl; s_kl[g] = skl; row_len[g] = len; if (row_kl) row_kl[g] = skl; }
        tot_mask += len;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < G * C; i += blockDim.x) {
        const int g = i / C;
        const float m = (float)mask[i];
        float dkl = 0.f;
        if (ref_logp) dkl = 1.f - __expf(ref_logp[i] - logp[i]);
        const float w = use_grpo ? (m / s_len[g] / (float)G) : (m / tot_mask);
        dlogp[i] = (m > 0.f) ? (-adv[g] + beta * dkl) * w * grad_scale : 0.f;
    }
    if (threadIdx.x == 0) {
        float loss = 0.f, klm = 0.f, num = 0.f;
        for (int g = 0; g < G; ++g) {
            if (use_grpo) loss += s_l[g] / s_len[g] / (float)G; else num += s_l[g];
            klm += s_kl[g] / s_len[g] / (float)G;
        }
        if (!use_grpo) loss = num / tot_mask;
        out[0] = loss; out[1] = klm; out[2] = tot_mask;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// GRPO loss + d loss / d logp against an OLD policy (several updates per rollout): the clipped loss of timer1_trainer.py:713-737 with a choice of normaliser, a
// token- or sequence-level importance coefficient and an upper cap on it (trl.GRPOConfig loss_type / importance_sampling_level / delta on top of epsilon_low /
// epsilon_high).  ONE kernel behind two entry points:
//   tr1_grpo_policy_loss : every argument is the caller's; clip = 1, count_floor = 1
//   tr1_grpo_loss_ratio  : norm_mode = use_grpo ? 0 : 1, seq_level = 0, delta = 0, clip = !use_grpo, count_floor = 0
// One 256-thread block per completion row.  (1) It counts the live tokens its normaliser needs - its row, and for the token mean the whole grid: integers, so every
// block gets the same exact number - and at sequence level sums the row's log-ratios and weights in fp64.  (2) One pass over the row writes dlogp and accumulates the
// row's partials.  (3) The partials go to ws (release fence), a ticket counter names the last block to finish (acquire fence), and that block alone folds the G rows -
// one row per lane, the fixed tree of wave_sum - into out8.  No floating-point atomics: same inputs, same bits.  Masked positions are never read.  Per live token
//   d = logp - old_logp (0 when old_logp is null)     kl = exp(ref - logp) - (ref - logp) - 1 (0 when ref_logp is null)     w = tok_weight or 1 (a constant)
//   c = exp(d)                                  (seq_level 0)        c = s_g = exp(sum_t d m / max(len_g, f)), one value per row          (seq_level 1)
//   a = min(min(c, delta) A, clamp(c, 1-el, 1+eh) A)   (delta <= 0: no cap;  clip = 0: a = c A)         l = -w a + beta kl         loss = sum n l
//   n = 1 / (max(len_g, f) G)  (norm_mode 0, row mean)   1 / max(tot, f)  (1, token mean)   1 / (G C)  (2, fixed length);  len_g = sum_t m, tot = sum m
// f = count_floor: at 1 a row (or a grid) without a live token gives zeros, at 0 the counts divide as they are and it gives NaN, as the ratio entry point's PyTorch
// reference does.  g(c) = 0 where (A > 0, c > 1+eh), (A < 0, c < 1-el) or (delta on, A < 0, c > delta), 1 elsewhere (delta > 1+eh is the caller's contract); with
// clip = 0 nothing is clamped, g = 1 everywhere, and low / high are only counted against el / eh.
//   token level    : dlogp = gs n (-w (c A) g(c) + beta (1 - exp(ref - logp))), both products rounded
//   sequence level : d s_g / d logp_t = s_g / max(len_g, f) on every live token, so dlogp = gs n (-A s_g g(s_g) (sum_t w m) / max(len_g, f) + beta (1 - exp(ref - logp)))
// out8 = {loss, mean_g masked-mean kl, sum mask, low / high / either clip fraction (tokens, so a clipped sequence counts with all of its), masked mean of
// c - 1 - log c, largest c};  ws = [ticket, pad to 16 words, G x 8 row partials], the TR1_GRPO_*_WS_WORDS of both entry points, zero before the first call, left zero.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int GLR_HEAD = 16, GLR_ROW = 8, GLR_MAX_G = 64;
constexpr int GLR_WS_WORDS = GLR_HEAD + GLR_ROW * GLR_MAX_G;
TR1_DEV double block_sum_f64(double v, double* red4) {      // 256 threads, fixed tree; every thread gets the sum
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red4[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red4[0] + red4[1]) + (red4[2] + red4[3]);
}
__global__ __launch_bounds__(256) void grpo_policy_loss_kernel(const float* __restrict__ logp, const float* __restrict__ old_logp, const float* __restrict__ ref_logp,
                                                               const float* __restrict__ tok_weight, const int* __restrict__ mask, const float* __restrict__ adv,
                                                               float* __restrict__ dlogp, float* __restrict__ out, float* __restrict__ row_len, float* __restrict__ row_kl,
                                                               float* ws, int G, int C, float beta, int norm_mode, int seq_level, float eps_low, float eps_high,
                                                               float delta, int clip, float count_floor, float grad_scale) {
    __shared__ float red[16];
    __shared__ double red4[4];
    __shared__ float part[GLR_ROW][4];
    __shared__ int s_last;
    const int g = blockIdx.x, tid = threadIdx.x;
    const int64_t row0 = (int64_t)g * C;
    const int* mrow = mask + row0;
    // ---- 1. live-token counts; at sequence level the row's sum of log-ratios and of weights
    float cnt_row = 0.f, cnt_all = 0.f;
    double sd = 0.0, sw = 0.0;
    for (int t = tid; t < C; t += 256) {
        if (mrow[t] == 0) continue;
        cnt_row += 1.f;
        if (seq_level) {
            if (old_logp) sd += (double)logp[row0 + t] - (double)old_logp[row0 + t];
            sw += tok_weight ? (double)tok_weight[row0 + t] : 1.0;
        }
    }
    cnt_row = block_sum(cnt_row, red);
    if (seq_level) { sd = block_sum_f64(sd, red4); sw = block_sum_f64(sw, red4); }
    if (norm_mode == 1) {
        const int64_t n = (int64_t)G * C;
        int c = 0;
        if ((reinterpret_cast<uintptr_t>(mask) & 15) == 0) {
            const int64_t n4 = n >> 2;
            const int4* m4 = reinterpret_cast<const int4*>(mask);
            for (int64_t i = tid; i < n4; i += 256) { const int4 v = m4[i]; c += (v.x != 0) + (v.y != 0) + (v.z != 0) + (v.w != 0); }
            for (int64_t i = (n4 << 2) + tid; i < n; i += 256) c += (mask[i] != 0);
        } else {
            for (int64_t i = tid; i < n; i += 256) c += (mask[i] != 0);
        }
        cnt_all = block_sum((float)c, red);      // per-thread counts and their sum stay below 2^24: exact in fp32
    }
    const float len_f = fmaxf(cnt_row, count_floor);
    const float norm = norm_mode == 0 ? 1.f / (len_f * (float)G) : norm_mode == 1 ? 1.f / fmaxf(cnt_all, count_floor) : 1.f / ((float)G * (float)C);
    // ---- 2. the row
    const float A = adv[g], lo = 1.f - eps_low, hi = 1.f + eps_high;
    const bool cap = clip && delta > 0.f;
    float s_g = 1.f, k3_g = 0.f, seq_term = 0.f;
    if (seq_level) {
        const double dbar = sd / (double)len_f;
        s_g = (float)exp(dbar);
        k3_g = (float)(expm1(dbar) - dbar);
        const bool stuck = clip && (((A > 0.f) && (s_g > hi)) || ((A < 0.f) && (s_g < lo)) || (cap && (A < 0.f) && (s_g > delta)));
        seq_term = stuck ? 0.f : -A * s_g * (float)(sw / (double)len_f);      // the mean weight is exactly 1 without tok_weight: the token-level bits at s_g = 1
    }
    float s_l = 0.f, s_kl = 0.f, n_low = 0.f, n_high = 0.f, n_any = 0.f, s_k3 = 0.f, mx = 0.f;
    for (int t = tid; t < C; t += 256) {
        const int64_t i = row0 + t;
        float dl = 0.f;
        if (mrow[t] != 0) {
            const float lp = logp[i];
            float c = s_g, k3 = k3_g;
            if (!seq_level) {
                const float d = old_logp ? lp - old_logp[i] : 0.f;
                c = expf(d); k3 = expm1f(d) - d;
            }
            const float w = tok_weight ? tok_weight[i] : 1.f;
            float kl = 0.f, dkl = 0.f;
            if (ref_logp) { const float r = ref_logp[i] - lp; const float e = __expf(r); kl = e - r - 1.f; dkl = 1.f - e; }
            const bool low = (A < 0.f) && (c < lo), high = (A > 0.f) && (c > hi);
            float term = c * A, dterm = c * A;
            if (clip) {
                term = fminf((cap ? fminf(c, delta) : c) * A, fminf(fmaxf(c, lo), hi) * A);
                if (low || high || (cap && (A < 0.f) && (c > delta))) dterm = 0.f;
            }
            s_l += -w * term + beta * kl;
            s_kl += kl;
            n_low += low ? 1.f : 0.f; n_high += high ? 1.f : 0.f; n_any += (low || high) ? 1.f : 0.f;
            s_k3 += k3;
            mx = fmaxf(mx, c);
            // roundings pinned to what each form compiled to while there were two kernels (the ratio kernel rounded both products, the sequence level fused beta dkl)
            dl = (seq_level ? __fmaf_rn(beta, dkl, seq_term) : __fmul_rn(beta, dkl) - __fmul_rn(w, dterm)) * norm * grad_scale;
        }
        dlogp[i] = dl;
    }
    {
        float v[GLR_ROW] = {cnt_row, s_l, s_kl, n_low, n_high, n_any, s_k3, 0.f};
#pragma unroll
        for (int k = 0; k < GLR_ROW - 1; ++k) v[k] = (k == 0) ? v[k] : wave_sum(v[k]);
        v[GLR_ROW - 1] = wave_max(mx);
        if ((tid & 63) == 0) {
#pragma unroll
            for (int k = 0; k < GLR_ROW; ++k) part[k][tid >> 6] = v[k];
        }
    }
    __syncthreads();
    unsigned* ticket = reinterpret_cast<unsigned*>(ws);
    float* rows = ws + GLR_HEAD;
    if (tid < GLR_ROW) {
        const float a = part[tid][0], b = part[tid][1], c = part[tid][2], d = part[tid][3];
        const float r = (tid == 0) ? a : (tid == GLR_ROW - 1) ? fmaxf(fmaxf(a, b), fmaxf(c, d)) : ((a + b) + (c + d));
        rows[g * GLR_ROW + tid] = r;
        if (tid == 0) row_len[g] = r;
        if (tid == 2 && row_kl) row_kl[g] = r;
    }
    // publish: the writers' stores have left the wave, ONE agent-scope release, then the ticket (the counter form of the in-launch hand-off; the explicit
    // waits stay beside the fences).  The block that draws ticket G - 1 has every row's partials behind its one agent-scope acquire, on whichever XCDs they ran.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned prev = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = (prev == (unsigned)(G - 1));
        if (s_last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
    }
    __syncthreads();
    if (!s_last || tid >= 64) return;
    // ---- 3. the last block: lane = row, fixed-order fold
    const volatile float* vr = rows;
    const bool on = tid < G;
    float p[GLR_ROW];
#pragma unroll
    for (int k = 0; k < GLR_ROW; ++k) p[k] = on ? vr[tid * GLR_ROW + k] : 0.f;
    const float tot = wave_sum(p[0]), tot_f = fmaxf(tot, count_floor), plen = fmaxf(p[0], count_floor);
    const float per_row_l = on ? p[1] / plen / (float)G : 0.f, per_row_kl = on ? p[2] / plen / (float)G : 0.f;      // (an idle lane would be 0 / 0 at floor 0)
    const float sum_l = wave_sum(p[1]), row_mean_l = wave_sum(per_row_l);
    const float loss = norm_mode == 0 ? row_mean_l : norm_mode == 1 ? sum_l / tot_f : sum_l / ((float)G * (float)C);
    const float klm = wave_sum(per_row_kl);
    const float f_low = wave_sum(p[3]) / tot_f, f_high = wave_sum(p[4]) / tot_f, f_any = wave_sum(p[5]) / tot_f;
    const float k3 = wave_sum(p[6]) / tot_f;
    const float rmax = wave_max(p[7]);
    if (tid == 0) {
        out[0] = loss; out[1] = klm; out[2] = tot; out[3] = f_low; out[4] = f_high; out[5] = f_any; out[6] = k3; out[7] = rmax;
        *ticket = 0u;         // zero again for the next call
    }
}

extern "C" int tr1_logp_entropy_fwd(const void* logits, int64_t ld, const void* targets, void* logp, void* entropy, void* lse, int64_t R,
                                    int64_t V, void* stream) {
    TR1_CHECK_ARG(ld % 8 == 0, "logp_entropy: ld must be a multiple of 8");
    if (R == 0) return 0;
    hipLaunchKernelGGL(logp_entropy_fwd_kernel, dim3((unsigned)R), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)logits, ld,
                       (const int*)targets, (float*)logp, (float*)entropy, (float*)lse, (int)V);
    TR1_LAUNCH_CHECK();
}
extern "C" int tr1_logp_bwd(const void* logits, int64_t ld, const void* targets, const void* lse, const void* dlogp, void* dlogits,
                            int64_t ld_out, int64_t R, int64_t V, void* stream) {
    TR1_CHECK_ARG(ld % 8 == 0 && ld_out % 8 == 0 && V % 8 == 0, "logp_bwd: ld and V must be multiples of 8");
    if (R == 0) return 0;
    dim3 grid((unsigned)tr1_grid_1d(V / 8, 256, 64), (unsigned)R);
    hipLaunchKernelGGL(logp_bwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)logits, ld, (const int*)targets,
                       (const float*)lse, (const float*)dlogp, (bf16_t*)dlogits, ld_out, (int)V);
    TR1_LAUNCH_CHECK();
}
extern "C" int tr1_logp_entropy_bwd(const void* logits, int64_t ld, const void* targets, const void* lse, const void* ent, const void* dlogp,
                                    const void* dent, void* dlogits, int64_t ld_out, int64_t R, int64_t V, void* stream) {
    if (!dent) return tr1_logp_bwd(logits, ld, targets, lse, dlogp, dlogits, ld_out, R, V, stream);      // no entropy gradient: the kernel that always ran
    TR1_CHECK_ARG(ld % 8 == 0 && ld_out % 8 == 0 && V % 8 == 0, "logp_entropy_bwd: ld and V must be multiples of 8");
    TR1_CHECK_ARG(ent, "logp_entropy_bwd: dent needs the forward's entropy");
    if (R == 0) return 0;
    dim3 grid((unsigned)tr1_grid_1d(V / 8, 256, 64), (unsigned)R);
    hipLaunchKernelGGL(logp_entropy_bwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)logits, ld, (const int*)targets,
                       (const float*)lse, (const float*)ent, (const float*)dlogp, (const float*)dent, (bf16_t*)dlogits, ld_out, (int)V);
    TR1_LAUNCH_CHECK();
}
extern "C" int tr1_entropy_quantile_weight(const void* ent, const void* mask, void* weight, void* stats3, int64_t N, float rho, void* stream) {
    TR1_CHECK_ARG(N >= 1 && N <= TR1_ENTROPY_QUANTILE_MAX_N, "entropy_quantile_weight: need 1 <= N <= 2^20 (one block walks the grid)");
    TR1_CHECK_ARG(rho > 0.f && rho <= 1.f, "entropy_quantile_weight: rho must be in (0, 1]");
    TR1_CHECK_ARG(ent && mask && weight && stats3, "entropy_quantile_weight: null argument");
    hipLaunchKernelGGL(entropy_quantile_weight_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, (const float*)ent, (const int*)mask, (float*)weight,
                       (float*)stats3, (int)N, rho);
    TR1_LAUNCH_CHECK();
}
extern "C" int tr1_grpo_loss(const void* logp, const void* ref_logp, const void* mask, const void* adv, void* dlogp, void* out3,
                             void* row_len, void* row_kl, int64_t G, int64_t C, float beta, int use_grpo, float grad_scale, void* stream) {
    TR1_CHECK_ARG(G >= 1 && G <= 64, "grpo_loss: G must be in [1, 64]");
    hipLaunchKernelGGL(grpo_loss_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)logp, (const float*)ref_logp,
                       (const int*)mask, (const float*)adv, (float*)dlogp, (float*)out3, (float*)row_len, (float*)row_kl, (int)G, (int)C, beta,
                       use_grpo, grad_scale);
    TR1_LAUNCH_CHECK();
}
static_assert(GLR_WS_WORDS == TR1_GRPO_LOSS_RATIO_WS_WORDS, "include/timer1_hip.h states the workspace size of tr1_grpo_loss_ratio");
extern "C" int tr1_grpo_loss_ratio(const void* logp, const void* old_logp, const void* ref_logp, const void* tok_weight, const void* mask,
                                   const void* adv, void* dlogp, void* out8, void* row_len, void* row_kl, void* ws, int64_t G, int64_t C, float beta,
                                   int use_grpo, float eps_low, float eps_high, float grad_scale, void* stream) {
    TR1_CHECK_ARG(G >= 1 && G <= GLR_MAX_G, "grpo_loss_ratio: G must be in [1, 64]");
    TR1_CHECK_ARG(C >= 1 && G * C < ((int64_t)1 << 24), "grpo_loss_ratio: need 1 <= C and G * C < 2^24");
    TR1_CHECK_ARG(logp && old_logp && mask && adv && dlogp && out8 && row_len && ws, "grpo_loss_ratio: null argument");
    hipLaunchKernelGGL(grpo_policy_loss_kernel, dim3((unsigned)G), dim3(256), 0, (hipStream_t)stream, (const float*)logp, (const float*)old_logp, (const float*)ref_logp,
                       (const float*)tok_weight, (const int*)mask, (const float*)adv, (float*)dlogp, (float*)out8, (float*)row_len, (float*)row_kl, (float*)ws, (int)G, (int)C,
                       beta, /*norm_mode*/ use_grpo ? 0 : 1, /*seq_level*/ 0, eps_low, eps_high, /*delta*/ 0.f, /*clip*/ use_grpo ? 0 : 1, /*count_floor*/ 0.f, grad_scale);
    TR1_LAUNCH_CHECK();
}
static_assert(GLR_WS_WORDS == TR1_GRPO_POLICY_LOSS_WS_WORDS, "include/timer1_hip.h states the workspace size of tr1_grpo_policy_loss");
extern "C" int tr1_grpo_policy_loss(const void* logp, const void* old_logp, const void* ref_logp, const void* tok_weight, const void* mask,
                                    const void* adv, void* dlogp, void* out8, void* row_len, void* row_kl, void* ws, int64_t G, int64_t C, float beta,
                                    int norm_mode, int seq_level, float eps_low, float eps_high, float delta, float grad_scale, void* stream) {
    TR1_CHECK_ARG(G >= 1 && G <= GLR_MAX_G, "grpo_policy_loss: G must be in [1, 64]");
    TR1_CHECK_ARG(C >= 1 && G * C < ((int64_t)1 << 24), "grpo_policy_loss: need 1 <= C and G * C < 2^24");
    TR1_CHECK_ARG(logp && mask && adv && dlogp && out8 && row_len && ws, "grpo_policy_loss: null argument");
    TR1_CHECK_ARG(norm_mode >= 0 && norm_mode <= 2 && (seq_level == 0 || seq_level == 1),
                  "grpo_policy_loss: norm_mode is 0 (row mean), 1 (token mean) or 2 (fixed length), seq_level 0 or 1");
    hipLaunchKernelGGL(grpo_policy_loss_kernel, dim3((unsigned)G), dim3(256), 0, (hipStream_t)stream, (const float*)logp, (const float*)old_logp, (const float*)ref_logp,
                       (const float*)tok_weight, (const int*)mask, (const float*)adv, (float*)dlogp, (float*)out8, (float*)row_len, (float*)row_kl, (float*)ws, (int)G, (int)C,
                       beta, norm_mode, seq_level, eps_low, eps_high, delta, /*clip*/ 1, /*count_floor*/ 1.f, grad_scale);
    TR1_LAUNCH_CHECK();
}
