// Fused AdamW over ONE flat parameter arena (fp32 master / m / v / grad, bf16 working copy) + global grad-norm clip.
// Replaces DeepSpeed's FusedAdam / DeepSpeedCPUAdam on the reference path (scripts/zero3.json:13-21, zero3_offload.json:24-31);
// update rule = torch.optim.AdamW (decoupled weight decay, bias correction), HF defaults lr/betas/eps, max_grad_norm 1.0.
// HBM-bound: 16 B read (g, p, m, v) + 14 B written (p, m, v, bf16 copy) [+4 B when the gradient is zeroed in place] per parameter.
// With bf16 moments (tr1_adamw_step_sr16, stochastic rounding): 12 B read + 10 B written.
#include "tr1_common.h"

// every array is streamed exactly once per step (258 GB for the 7B arena): nt loads/stores keep it from turning over L2 / the memory-side cache
#ifndef TR1_OPT_NT
#define TR1_OPT_NT 1
#endif
#if TR1_OPT_NT
#define OPT_LD(ptr) __builtin_nontemporal_load(ptr)
#define OPT_ST(val, ptr) __builtin_nontemporal_store(val, ptr)
#else
#define OPT_LD(ptr) (*(ptr))
#define OPT_ST(val, ptr) (*(ptr) = (val))
#endif

__global__ __launch_bounds__(256) void sumsq_kernel(const float* __restrict__ g, int64_t n, float* __restrict__ part) {
    __shared__ float red[16];
    float s = 0.f;
    const int64_t n4 = n >> 2;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        const f32x4_t v = OPT_LD(reinterpret_cast<const f32x4_t*>(g) + i);
        s += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
    }
    if (blockIdx.x == 0) for (int64_t i = n4 * 4 + threadIdx.x; i < n; i += blockDim.x) s += g[i] * g[i];
    s = block_sum(s, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;        // per-block partial: partials_sum_kernel adds them in a fixed order (reproducible norm)
}

// the same sum over a bf16 array (data-parallel runs: the all-reduced gradient stays in its bf16 wire buffer and is consumed from there)
__global__ __launch_bounds__(256) void sumsq_bf16_kernel(const bf16_t* __restrict__ g, int64_t n, float* __restrict__ part) {
    __shared__ float red[16];
    float s = 0.f;
    const int64_t n8 = n >> 3;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n8; i += (int64_t)gridDim.x * blockDim.x) {
        const u32x4_t v = OPT_LD(reinterpret_cast<const u32x4_t*>(g) + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) { const float a = bflo(v[e]), b = bfhi(v[e]); s += a * a + b * b; }
    }
    if (blockIdx.x == 0) for (int64_t i = n8 * 8 + threadIdx.x; i < n; i += blockDim.x) { const float a = bf2f(g[i]); s += a * a; }
    s = block_sum(s, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// sumsq: device scalar with sum of squared grads (already multiplied by nothing); clip coefficient derived in-kernel so the
// step needs no host round trip:  coef = grad_mult * min(1, max_norm / (grad_mult*sqrt(sumsq) + 1e-6)).
// G16: the gradient is read from a bf16 array `g16` (the all-reduced wire buffer); `g` (fp32 accumulator) is then only zeroed, never read.
template <bool G16>
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v, float* __restrict__ g,
                                                    bf16_t* __restrict__ p16, int64_t n, float lr, float beta1, float beta2, float eps,
                                                    float wd, float bc1, float bc2_sqrt, const float* __restrict__ sumsq, float max_norm,
                                                    float grad_mult, int zero_grad, const bf16_t* __restrict__ g16) {
    float coef = grad_mult;
    if (sumsq && max_norm > 0.f) {
        const float norm = sqrtf(*sumsq) * grad_mult;
        coef = grad_mult * fminf(1.f, max_norm / (norm + 1e-6f));
    }
    const int64_t n4 = n >> 2;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        f32x4_t pv = OPT_LD(reinterpret_cast<f32x4_t*>(p) + i), mv = OPT_LD(reinterpret_cast<f32x4_t*>(m) + i), vv = OPT_LD(reinterpret_cast<f32x4_t*>(v) + i);
        f32x4_t gv;
        if (G16) { const u32x2_t w = OPT_LD(reinterpret_cast<const u32x2_t*>(g16) + i); gv = (f32x4_t){bflo(w[0]), bfhi(w[0]), bflo(w[1]), bfhi(w[1])}; }
        else gv = OPT_LD(reinterpret_cast<f32x4_t*>(g) + i);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float gg = gv[j] * coef;
            pv[j] *= (1.f - lr * wd);
            mv[j] = beta1 * mv[j] + (1.f - beta1) * gg;
            vv[j] = beta2 * vv[j] + (1.f - beta2) * gg * gg;
            const float denom = sqrtf(vv[j]) / bc2_sqrt + eps;
            pv[j] -= (lr / bc1) * (mv[j] / denom);
        }
        OPT_ST(pv, reinterpret_cast<f32x4_t*>(p) + i); OPT_ST(mv, reinterpret_cast<f32x4_t*>(m) + i); OPT_ST(vv, reinterpret_cast<f32x4_t*>(v) + i);
        const u32x2_t w = {pack2bf(pv[0], pv[1]), pack2bf(pv[2], pv[3])};
        OPT_ST(w, reinterpret_cast<u32x2_t*>(p16) + i);
        if (zero_grad) OPT_ST(((f32x4_t){0.f, 0.f, 0.f, 0.f}), reinterpret_cast<f32x4_t*>(g) + i);
    }
    if (blockIdx.x == 0) {
        for (int64_t i = n4 * 4 + threadIdx.x; i < n; i += blockDim.x) {
            const float gg = (G16 ? bf2f(g16[i]) : g[i]) * coef;
            float pv = p[i] * (1.f - lr * wd);
            const float mv = beta1 * m[i] + (1.f - beta1) * gg, vv = beta2 * v[i] + (1.f - beta2) * gg * gg;
            pv -= (lr / bc1) * (mv / (sqrtf(vv) / bc2_sqrt + eps));
            p[i] = pv; m[i] = mv; v[i] = vv; p16[i] = f2bf(pv);
            if (zero_grad) g[i] = 0.f;
        }
    }
}

// ws_f32: >= 2048 floats of scratch for the per-block partials (no float atomics: the same gradient gives the same norm on every run)
extern "C" int tr1_sumsq_accum(const void* g, int64_t n, void* out_scalar, void* ws_f32, int64_t ws_floats, void* stream) {
    if (n == 0) return 0;
    const int nb = tr1_grid_1d(n / 4 + 1, 256, 2048);
    TR1_CHECK_ARG(ws_f32 && ws_floats >= nb, "sumsq_accum: workspace too small");
    hipLaunchKernelGGL(sumsq_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, (const float*)g, n, (float*)ws_f32);
    hipLaunchKernelGGL(partials_sum_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)ws_f32, (int64_t)nb, (float*)out_scalar);
    TR1_LAUNCH_CHECK();
}

extern "C" int tr1_adamw_step(void* p_f32, void* m_f32, void* v_f32, void* g_f32, void* p_bf16, int64_t n, float lr, float beta1, float beta2,
                              float eps, float weight_decay, int64_t step, const void* sumsq_scalar, float max_norm, float grad_mult,
                              int zero_grad, void* stream) {
    TR1_CHECK_ARG(step >= 1, "adamw: step counts from 1");
    if (n == 0) return 0;
    const float bc1 = (float)(1.0 - pow((double)beta1, (double)step));
    const float bc2_sqrt = (float)sqrt(1.0 - pow((double)beta2, (double)step));
    hipLaunchKernelGGL(adamw_kernel<false>, dim3(tr1_grid_1d(n / 4 + 1, 256, 4096)), dim3(256), 0, (hipStream_t)stream, (float*)p_f32, (float*)m_f32,
                       (float*)v_f32, (float*)g_f32, (bf16_t*)p_bf16, n, lr, beta1, beta2, eps, weight_decay, bc1, bc2_sqrt,
                       (const float*)sumsq_scalar, max_norm, grad_mult, zero_grad, (const bf16_t*)nullptr);
    TR1_LAUNCH_CHECK();
}

// Data-parallel form: the gradient SUM over ranks is read from the bf16 wire buffer `g_bf16` (no bf16 -> fp32 copy-back pass); the fp32
// accumulator `g_f32` is only zeroed (zero_grad) for the next window.
extern "C" int tr1_adamw_step_g16(void* p_f32, void* m_f32, void* v_f32, void* g_f32, const void* g_bf16, void* p_bf16, int64_t n, float lr, float beta1,
                                  float beta2, float eps, float weight_decay, int64_t step, const void* sumsq_scalar, float max_norm, float grad_mult,
                                  int zero_grad, void* stream) {
    TR1_CHECK_ARG(step >= 1 && g_bf16, "adamw_g16: step counts from 1, bf16 gradient required");
    if (n == 0) return 0;
    const float bc1 = (float)(1.0 - pow((double)beta1, (double)step));
    const float bc2_sqrt = (float)sqrt(1.0 - pow((double)beta2, (double)step));
    hipLaunchKernelGGL(adamw_kernel<true>, dim3(tr1_grid_1d(n / 4 + 1, 256, 4096)), dim3(256), 0, (hipStream_t)stream, (float*)p_f32, (float*)m_f32,
                       (float*)v_f32, (float*)g_f32, (bf16_t*)p_bf16, n, lr, beta1, beta2, eps, weight_decay, bc1, bc2_sqrt,
                       (const float*)sumsq_scalar, max_norm, grad_mult, zero_grad, (const bf16_t*)g_bf16);
    TR1_LAUNCH_CHECK();
}

// ---- AdamW with bf16 moments (GRPOConfig.optimizer_state_dtype="bf16"): m and v are stored in bf16, rounded STOCHASTICALLY (nearest-even freezes them: at beta2 =
// 0.999 a decaying v = 1.0 rounds back to 1.0 for ever).  HBM: 12 B read (g, p, m16, v16) + 10 B written (p, m16, v16, bf16 copy) [+4 B zeroing] per parameter.
// The master update of a step is the fp32-state kernel's from the same inputs: p' and p16 come from the UNROUNDED fp32 m', v'; only what is stored is rounded.
// Rounding of fp32 bits b with 16 random bits r: s = min((b & 0x7fffffff) + r, 0x7f7fffff), result = sign | s, upper half.  A value bf16 holds is unchanged, zero
// stays zero, v stays >= 0, a finite value stays finite, and the mean over r is the value.  inf / NaN take the nearest-even conversion.
TR1_DEV unsigned bf_sr(float f, unsigned r16) {
    const unsigned b = __float_as_uint(f), mag = b & 0x7fffffffu;
    const unsigned s = min(mag + r16, 0x7f7fffffu);
    return mag >= 0x7f800000u ? (unsigned)f2bf(f) : ((b & 0x80000000u) | s) >> 16;      // a select, not a branch: the conversion has no side effect
}
// sumsq -> coef -> gg -> m', v' with every operation rounded once (no fma contraction), so a host fp32 emulation reproduces the stored moments bit for bit:
// the random bits decide at a fixed threshold, and one ulp of fp32 moves a value across it.
TR1_DEV float sr16_coef(const float* __restrict__ sumsq, float max_norm, float grad_mult) {
#pragma clang fp contract(off)
    if (!(sumsq && max_norm > 0.f)) return grad_mult;
    const float norm = sqrtf(*sumsq) * grad_mult;
    const float den = norm + 1e-6f;
    return grad_mult * fminf(1.f, max_norm / den);
}
TR1_DEV void sr16_moments(float g, float coef, float beta1, float beta2, float m, float v, float& mn, float& vn) {
#pragma clang fp contract(off)
    const float gg = g * coef;
    const float m1 = beta1 * m, m2 = (1.f - beta1) * gg;
    mn = m1 + m2;
    const float v1 = beta2 * v, v2 = (1.f - beta2) * gg, v3 = v2 * gg;
    vn = v1 + v3;
}
#define SR16_STREAM 0x53523136u     // "SR16": the last Philox counter word (the sampler's is 0)
#define SR16_GRID_CAP 4096          // blocks of 256 lanes x 8 elements: one grid trip covers 2^23 elements (7B arena: 30.6 / 29.8 / 29.5 ms at 1024 / 2048 / 4096)
// Random bits of the GLOBAL element e = index_base + i: Philox block e / 4, word e % 4; its low half rounds m, its high half v.  A lane's 8 elements lie in 2
// blocks when index_base is a multiple of 4 and in 3 otherwise: SH = index_base % 4 is a template argument, so the words are picked without indexed registers.
template <bool G16, int SH>
__global__ __launch_bounds__(256) void adamw_sr16_kernel(float* __restrict__ p, bf16_t* __restrict__ m, bf16_t* __restrict__ v, float* __restrict__ g,
                                                         bf16_t* __restrict__ p16, int64_t n, float lr, float beta1, float beta2, float eps, float wd, float bc1,
                                                         float bc2_sqrt, const float* __restrict__ sumsq, float max_norm, float grad_mult, int zero_grad,
                                                         const bf16_t* __restrict__ g16, uint64_t seed, uint64_t index_base, unsigned step_lo) {
    const float coef = sr16_coef(sumsq, max_norm, grad_mult);
    const unsigned k0 = (unsigned)(seed & 0xffffffffu), k1 = (unsigned)(seed >> 32);
    const int64_t n8 = n >> 3;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n8; i += (int64_t)gridDim.x * blockDim.x) {
        f32x4_t pv[2] = {OPT_LD(reinterpret_cast<f32x4_t*>(p) + 2 * i), OPT_LD(reinterpret_cast<f32x4_t*>(p) + 2 * i + 1)};
        const u32x4_t mw = OPT_LD(reinterpret_cast<u32x4_t*>(m) + i), vw = OPT_LD(reinterpret_cast<u32x4_t*>(v) + i);
        f32x4_t gv[2];
        if (G16) {
            const u32x4_t w = OPT_LD(reinterpret_cast<const u32x4_t*>(g16) + i);
            gv[0] = (f32x4_t){bflo(w[0]), bfhi(w[0]), bflo(w[1]), bfhi(w[1])}; gv[1] = (f32x4_t){bflo(w[2]), bfhi(w[2]), bflo(w[3]), bfhi(w[3])};
        } else { gv[0] = OPT_LD(reinterpret_cast<f32x4_t*>(g) + 2 * i); gv[1] = OPT_LD(reinterpret_cast<f32x4_t*>(g) + 2 * i + 1); }
        constexpr int NB = SH ? 3 : 2;
        unsigned R[4 * NB];
        const uint64_t q = (index_base + 8 * (uint64_t)i) >> 2;
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            unsigned c[4] = {(unsigned)((q + b) & 0xffffffffu), (unsigned)((q + b) >> 32), step_lo, SR16_STREAM};
            philox4x32_10(c, k0, k1);
            R[4 * b] = c[0]; R[4 * b + 1] = c[1]; R[4 * b + 2] = c[2]; R[4 * b + 3] = c[3];
        }
        unsigned mh[8], vh[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float m0 = (j & 1) ? bfhi(mw[j >> 1]) : bflo(mw[j >> 1]), v0 = (j & 1) ? bfhi(vw[j >> 1]) : bflo(vw[j >> 1]);
            float mn, vn;
            sr16_moments(gv[j >> 2][j & 3], coef, beta1, beta2, m0, v0, mn, vn);
            float pj = pv[j >> 2][j & 3];
            pj *= (1.f - lr * wd);
            const float denom = sqrtf(vn) / bc2_sqrt + eps;
            pj -= (lr / bc1) * (mn / denom);
            pv[j >> 2][j & 3] = pj;
            const unsigned r = R[SH + j];
            mh[j] = bf_sr(mn, r & 0xffffu); vh[j] = bf_sr(vn, r >> 16);
        }
        OPT_ST(pv[0], reinterpret_cast<f32x4_t*>(p) + 2 * i); OPT_ST(pv[1], reinterpret_cast<f32x4_t*>(p) + 2 * i + 1);
        const u32x4_t mo = {mh[0] | (mh[1] << 16), mh[2] | (mh[3] << 16), mh[4] | (mh[5] << 16), mh[6] | (mh[7] << 16)};
        const u32x4_t vo = {vh[0] | (vh[1] << 16), vh[2] | (vh[3] << 16), vh[4] | (vh[5] << 16), vh[6] | (vh[7] << 16)};
        OPT_ST(mo, reinterpret_cast<u32x4_t*>(m) + i); OPT_ST(vo, reinterpret_cast<u32x4_t*>(v) + i);
        const u32x4_t w = {pack2bf(pv[0][0], pv[0][1]), pack2bf(pv[0][2], pv[0][3]), pack2bf(pv[1][0], pv[1][1]), pack2bf(pv[1][2], pv[1][3])};
        OPT_ST(w, reinterpret_cast<u32x4_t*>(p16) + i);
        if (zero_grad) {
            OPT_ST(((f32x4_t){0.f, 0.f, 0.f, 0.f}), reinterpret_cast<f32x4_t*>(g) + 2 * i); OPT_ST(((f32x4_t){0.f, 0.f, 0.f, 0.f}), reinterpret_cast<f32x4_t*>(g) + 2 * i + 1);
        }
    }
    if (blockIdx.x == 0) {
        for (int64_t i = n8 * 8 + threadIdx.x; i < n; i += blockDim.x) {
            float mn, vn;
            sr16_moments(G16 ? bf2f(g16[i]) : g[i], coef, beta1, beta2, bf2f(m[i]), bf2f(v[i]), mn, vn);
            float pj = p[i] * (1.f - lr * wd);
            pj -= (lr / bc1) * (mn / (sqrtf(vn) / bc2_sqrt + eps));
            const uint64_t e = index_base + (uint64_t)i;
            unsigned c[4] = {(unsigned)((e >> 2) & 0xffffffffu), (unsigned)(e >> 34), step_lo, SR16_STREAM};
            philox4x32_10(c, k0, k1);
            const unsigned w = (unsigned)(e & 3), r = w == 0 ? c[0] : w == 1 ? c[1] : w == 2 ? c[2] : c[3];
            p[i] = pj; m[i] = (bf16_t)bf_sr(mn, r & 0xffffu); v[i] = (bf16_t)bf_sr(vn, r >> 16); p16[i] = f2bf(pj);
            if (zero_grad) g[i] = 0.f;
        }
    }
}

// bf16 moments, stochastic rounding keyed by (seed, step, index_base + i): index_base is the offset of element 0 in the whole arena, so a range split into several
// calls or sharded over ranks gets the same bits.  g_bf16 (nullable): the wire-buffer form, g_f32 is then only zeroed.
extern "C" int tr1_adamw_step_sr16(void* p_f32, void* m_bf16, void* v_bf16, void* g_f32, const void* g_bf16, void* p_bf16, int64_t n, float lr, float beta1,
                                   float beta2, float eps, float weight_decay, int64_t step, const void* sumsq_scalar, float max_norm, float grad_mult,
                                   int zero_grad, uint64_t seed, int64_t index_base, void* stream) {
    TR1_CHECK_ARG(step >= 1 && index_base >= 0 && n >= 0, "adamw_sr16: step counts from 1, index_base and n are not negative");
    if (n == 0) return 0;
    const float bc1 = (float)(1.0 - pow((double)beta1, (double)step));
    const float bc2_sqrt = (float)sqrt(1.0 - pow((double)beta2, (double)step));
    const dim3 grid(tr1_grid_1d(n / 8 + 1, 256, SR16_GRID_CAP));
    tr1_dispatch<0, 1, 2, 3>((int)(index_base & 3), [&](auto sh) {
        constexpr int SH = decltype(sh)::value;
        auto go = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, grid, dim3(256), 0, (hipStream_t)stream, (float*)p_f32, (bf16_t*)m_bf16, (bf16_t*)v_bf16, (float*)g_f32, (bf16_t*)p_bf16, n, lr,
                               beta1, beta2, eps, weight_decay, bc1, bc2_sqrt, (const float*)sumsq_scalar, max_norm, grad_mult, zero_grad, (const bf16_t*)g_bf16,
                               seed, (uint64_t)index_base, (unsigned)((uint64_t)step & 0xffffffffu));
        };
        if (g_bf16) go(adamw_sr16_kernel<true, SH>); else go(adamw_sr16_kernel<false, SH>);
    });
    TR1_LAUNCH_CHECK();
}

extern "C" int tr1_sumsq_accum_bf16(const void* g_bf16, int64_t n, void* out_scalar, void* ws_f32, int64_t ws_floats, void* stream) {
    if (n == 0) return 0;
    const int nb = tr1_grid_1d(n / 8 + 1, 256, 2048);
    TR1_CHECK_ARG(ws_f32 && ws_floats >= nb, "sumsq_accum_bf16: workspace too small");
    hipLaunchKernelGGL(sumsq_bf16_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)g_bf16, n, (float*)ws_f32);
    hipLaunchKernelGGL(partials_sum_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)ws_f32, (int64_t)nb, (float*)out_scalar);
    TR1_LAUNCH_CHECK();
}

// g[base + l * stride + r] = 0 for l < count and r in the (at most 8) half-open ranges rel[2i], rel[2i+1]: the SMALL per-layer tensors of the gradient arena
// (norm weights, biases, padding).  The weight-gradient GEMMs OVERWRITE the large matrices on the first micro-step of every accumulation window, so the
// optimizer no longer zeroes those (4 of its 34 bytes per parameter); what still accumulates from zero is cleared by this launch (a few KB per layer).
struct ZeroRanges { int64_t a[8], b[8]; int n; };
__global__ __launch_bounds__(256) void zero_periodic_kernel(float* __restrict__ g, int64_t base, int64_t stride, ZeroRanges zr) {
    float* gl = g + base + (int64_t)blockIdx.y * stride;
    for (int r = 0; r < zr.n; ++r)
        for (int64_t i = zr.a[r] + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < zr.b[r]; i += (int64_t)gridDim.x * blockDim.x) gl[i] = 0.f;
}
extern "C" int tr1_zero_ranges_periodic(void* g_f32, int64_t base, int64_t stride, int64_t count, const int64_t* rel_ranges, int64_t n_ranges, void* stream) {
    TR1_CHECK_ARG(n_ranges >= 0 && n_ranges <= 8 && (n_ranges == 0 || rel_ranges), "zero_ranges_periodic: at most 8 ranges");
    if (count <= 0 || n_ranges == 0) return 0;
    ZeroRanges zr; zr.n = (int)n_ranges;
    int64_t longest = 1;
    for (int i = 0; i < zr.n; ++i) {
        zr.a[i] = rel_ranges[2 * i]; zr.b[i] = rel_ranges[2 * i + 1];
        TR1_CHECK_ARG(zr.a[i] >= 0 && zr.b[i] >= zr.a[i] && zr.b[i] <= stride, "zero_ranges_periodic: range outside the period");
        if (zr.b[i] - zr.a[i] > longest) longest = zr.b[i] - zr.a[i];
    }
    const unsigned gx = (unsigned)((longest + 255) / 256 < 64 ? (longest + 255) / 256 : 64);
    hipLaunchKernelGGL(zero_periodic_kernel, dim3(gx, (unsigned)count), dim3(256), 0, (hipStream_t)stream, (float*)g_f32, base, stride, zr);
    TR1_LAUNCH_CHECK();
}

// out += sum of partials[0 .. n) in a FIXED order (one block: thread t adds partials[t], partials[t + 1024], ...; then the block tree) - the per-wave sums of
// squares the weight-gradient epilogues left (tr1_wgrad_f32_sumsq)
// two fixed-order levels (a single 1024-thread block took 0.33 ms for the 7B step's 720 k partials): level 1 - block b sums its contiguous share and leaves
// the result in scratch[b]; level 2 - one wave-sized block adds the <= 256 block sums to `out`
__global__ __launch_bounds__(256) void sumsq_partials_kernel(const float* __restrict__ part, int64_t n, float* __restrict__ scratch) {
    __shared__ float red[16];
    const int64_t per = (n + gridDim.x - 1) / gridDim.x, a = (int64_t)blockIdx.x * per, b = a + per < n ? a + per : n;
    float s = 0.f;
    for (int64_t i = a + threadIdx.x; i < b; i += 256) s += part[i];
    s = block_sum(s, red);
    if (threadIdx.x == 0) scratch[blockIdx.x] = s;
}
__global__ __launch_bounds__(256) void sumsq_partials_final_kernel(const float* __restrict__ scratch, int nb, float* __restrict__ out) {
    __shared__ float red[16];
    float s = threadIdx.x < nb ? scratch[threadIdx.x] : 0.f;
    s = block_sum(s, red);
    if (threadIdx.x == 0) atomicAdd(out, s);
}
// partials_f32 must have room for 256 more floats behind its n entries (scratch of the first level)
extern "C" int tr1_sumsq_partials_accum(const void* partials_f32, int64_t n, void* out_scalar, void* stream) {
    if (n == 0) return 0;
    const int nb = (int)(n < 256 * 256 ? (n + 255) / 256 : 256);
    float* scratch = (float*)partials_f32 + n;
    hipLaunchKernelGGL(sumsq_partials_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, (const float*)partials_f32, n, scratch);
    hipLaunchKernelGGL(sumsq_partials_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)scratch, nb, (float*)out_scalar);
    TR1_LAUNCH_CHECK();
}

// out += sum of g[base + l * stride + r]^2 over l < count and r in the (<= 8) half-open ranges: the SMALL per-layer gradient tensors next to the large matrices
// whose squared norm came out of the weight-gradient epilogues
__global__ __launch_bounds__(256) void sumsq_periodic_kernel(const float* __restrict__ g, int64_t base, int64_t stride, ZeroRanges zr, float* __restrict__ part) {
    __shared__ float red[16];
    const float* gl = g + base + (int64_t)blockIdx.y * stride;
    float s = 0.f;
    for (int r = 0; r < zr.n; ++r)
        for (int64_t i = zr.a[r] + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < zr.b[r]; i += (int64_t)gridDim.x * blockDim.x) { const float v = gl[i]; s += v * v; }
    s = block_sum(s, red);
    if (threadIdx.x == 0) part[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
}
extern "C" int tr1_sumsq_ranges_periodic(const void* g_f32, int64_t base, int64_t stride, int64_t count, const int64_t* rel_ranges, int64_t n_ranges, void* out_scalar,
                                         void* ws_f32, int64_t ws_floats, void* stream) {
    TR1_CHECK_ARG(n_ranges >= 0 && n_ranges <= 8 && (n_ranges == 0 || rel_ranges) && out_scalar, "sumsq_ranges_periodic: at most 8 ranges");
    if (count <= 0 || n_ranges == 0) return 0;
    ZeroRanges zr; zr.n = (int)n_ranges;
    int64_t longest = 1;
    for (int i = 0; i < zr.n; ++i) {
        zr.a[i] = rel_ranges[2 * i]; zr.b[i] = rel_ranges[2 * i + 1];
        TR1_CHECK_ARG(zr.a[i] >= 0 && zr.b[i] >= zr.a[i] && zr.b[i] <= stride, "sumsq_ranges_periodic: range outside the period");
        if (zr.b[i] - zr.a[i] > longest) longest = zr.b[i] - zr.a[i];
    }
    const unsigned gx = (unsigned)((longest + 255) / 256 < 64 ? (longest + 255) / 256 : 64);
    TR1_CHECK_ARG(ws_f32 && ws_floats >= (int64_t)gx * count, "sumsq_ranges_periodic: workspace too small (64 floats per period)");
    hipLaunchKernelGGL(sumsq_periodic_kernel, dim3(gx, (unsigned)count), dim3(256), 0, (hipStream_t)stream, (const float*)g_f32, base, stride, zr, (float*)ws_f32);
    hipLaunchKernelGGL(partials_sum_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)ws_f32, (int64_t)gx * count, (float*)out_scalar);
    TR1_LAUNCH_CHECK();
}

// Reference-policy sync (trl.GRPOConfig.sync_ref_model, the TR-DPO rule): ref = (1 - alpha) ref + alpha policy, in place on the bf16 reference arena.
// Three fp32 roundings, pinned (no fma contraction: ref_mix), then ONE rounding to bf16: ref[i] = bf16_rne(fadd(fmul(keep, ref[i]), fmul(alpha, policy[i]))),
// keep = 1 - alpha rounded once on the host.  Two products, so a pair of opposite sign near the largest bf16 does not overflow where the mix is finite.
// The same pass leaves sum (policy - ref)^2 and sum ref^2 of the values BEFORE the mix as per-block partials (part[b] and part[gridDim.x + b]): the
// weight-space distance costs no traffic of its own.  HBM-bound: 4 B read + 2 B written per element, every array streamed once.
// (__fmul_rn / __fadd_rn are plain * and + to this compiler and were contracted into v_pk_fma_f32 here; the pragma takes the contract flag off these three operations)
TR1_DEV float ref_mix(float keep, float alpha, float r, float p) {
#pragma clang fp contract(off)
    const float t1 = keep * r, t2 = alpha * p;
    return t1 + t2;
}
__global__ __launch_bounds__(256) void ref_mixup_kernel(bf16_t* __restrict__ ref, const bf16_t* __restrict__ pol, int64_t n, float alpha, float keep,
                                                        float* __restrict__ part) {
    __shared__ float red[16];
    float sd = 0.f, sr = 0.f;
    const int64_t n8 = n >> 3;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n8; i += (int64_t)gridDim.x * blockDim.x) {
        const u32x4_t rv = OPT_LD(reinterpret_cast<const u32x4_t*>(ref) + i), pv = OPT_LD(reinterpret_cast<const u32x4_t*>(pol) + i);
        u32x4_t o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float ra = bflo(rv[e]), rb = bfhi(rv[e]), pa = bflo(pv[e]), pb = bfhi(pv[e]);
            const float da = pa - ra, db = pb - rb;
            sd += da * da + db * db;
            sr += ra * ra + rb * rb;
            o[e] = pack2bf(ref_mix(keep, alpha, ra, pa), ref_mix(keep, alpha, rb, pb));
        }
        OPT_ST(o, reinterpret_cast<u32x4_t*>(ref) + i);
    }
    if (blockIdx.x == 0) {
        for (int64_t i = n8 * 8 + threadIdx.x; i < n; i += blockDim.x) {
            const float r = bf2f(ref[i]), p = bf2f(pol[i]), d = p - r;
            sd += d * d;
            sr += r * r;
            ref[i] = f2bf(ref_mix(keep, alpha, r, p));
        }
    }
    sd = block_sum(sd, red);
    sr = block_sum(sr, red);
    if (threadIdx.x == 0) { part[blockIdx.x] = sd; part[gridDim.x + blockIdx.x] = sr; }
}
// sums[0] = sum of part[0 .. nb), sums[1] = sum of part[nb .. 2 nb), each in the fixed order of partials_sum_kernel; written, not accumulated (nb = 0: both 0)
__global__ __launch_bounds__(256) void ref_mixup_sums_kernel(const float* __restrict__ part, int nb, float* __restrict__ sums) {
    __shared__ float red[16];
    float sd = 0.f, sr = 0.f;
    for (int i = threadIdx.x; i < nb; i += 256) { sd += part[i]; sr += part[nb + i]; }
    sd = block_sum(sd, red);
    sr = block_sum(sr, red);
    if (threadIdx.x == 0) { sums[0] = sd; sums[1] = sr; }
}
// ws_f32: >= 4096 floats (two partials per block, at most 2048 blocks).  No float atomics: the same inputs give the same two sums on every run.
extern "C" int tr1_ref_mixup(void* ref_bf16, const void* policy_bf16, int64_t n, float alpha, void* sums_f32, void* ws_f32, int64_t ws_floats, void* stream) {
    TR1_CHECK_ARG(n >= 0 && sums_f32 && (n == 0 || (ref_bf16 && policy_bf16 && ref_bf16 != policy_bf16)), "ref_mixup: null or aliased pointer");
    TR1_CHECK_ARG(alpha >= 0.f && alpha <= 1.f, "ref_mixup: alpha must be in [0, 1]");
    TR1_CHECK_ARG((((uintptr_t)ref_bf16 | (uintptr_t)policy_bf16) & 15) == 0, "ref_mixup: both arrays must be 16-byte aligned");
    const int nb = n ? tr1_grid_1d(n / 8 + 1, 256, 2048) : 0;
    TR1_CHECK_ARG(nb == 0 || (ws_f32 && ws_floats >= 2 * (int64_t)nb), "ref_mixup: workspace too small");
    if (nb)
        hipLaunchKernelGGL(ref_mixup_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, (bf16_t*)ref_bf16, (const bf16_t*)policy_bf16, n, alpha, 1.0f - alpha,
                           (float*)ws_f32);
    hipLaunchKernelGGL(ref_mixup_sums_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)ws_f32, nb, (float*)sums_f32);
    TR1_LAUNCH_CHECK();
}
