// Shared device/host helpers for the timer1 HIP library (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <type_traits>

typedef unsigned short bf16_t;  // raw bfloat16 bits

typedef __attribute__((ext_vector_type(8))) short bf16x8_t;   // MFMA A/B fragment (8 bf16, 4 VGPRs)
typedef __attribute__((ext_vector_type(4))) float f32x4_t;    // MFMA 16x16 C/D fragment
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_t;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2_t;

#define TR1_DEV __device__ __forceinline__

TR1_DEV float bf2f(bf16_t h) { return __uint_as_float(((unsigned)h) << 16); }

// round-to-nearest-even via the gfx950 hardware conversion (v_cvt_pk_bf16_f32; the compiler selects it for __bf16 casts),
// same rounding as torch's float->bfloat16 cast
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_native_t;
TR1_DEV bf16_t f2bf(float f) { const __bf16 b = (__bf16)f; return __builtin_bit_cast(bf16_t, b); }
TR1_DEV unsigned pack2bf(float lo, float hi) {
    const bf16x2_native_t v = {(__bf16)lo, (__bf16)hi};
    return __builtin_bit_cast(unsigned, v);
}
TR1_DEV float bflo(unsigned w) { return __uint_as_float(w << 16); }
TR1_DEV float bfhi(unsigned w) { return __uint_as_float(w & 0xffff0000u); }

// ---- cross-lane exchanges without the LDS (round 6).  __shfl_xor lowers to ds_bpermute_b32: an LDS round trip plus an lgkmcnt(0) wait that also drains every LDS read
// in flight; a 6-step wave reduction is six DEPENDENT round trips (~500 cycles in the latency-bound decode kernels).  gfx950 exchanges the halves (v_permlane32_swap)
// and the odd / even 16-lane rows (v_permlane16_swap) of a wave in the vector unit, and DPP row rotations cover the steps inside a row.  The reductions below take
// the SAME partners in the SAME order as the xor butterfly 32, 16, 8, 4, 2, 1 they replace: after step k the values have period k inside a row, so the lane that a
// rotation by k/2 reads holds exactly what lane ^ (k/2) holds - and a + b, max(a, b) do not care which side the partner is on: bit-identical results.
// (Assembly for the swaps: the builtin's second result is mis-assigned by this hipcc; the leading nops are the VALU-write -> permlane-read wait states.)
TR1_DEV void tr1_halves32(float x, float& a, float& b) { a = x; b = x; asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b)); }   // a = lane & 31 of the lower half, b = of the upper half
TR1_DEV void tr1_halves16(float x, float& a, float& b) { a = x; b = x; asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b)); }   // a = the even row of each row pair, b = the odd row
template <int N> TR1_DEV float tr1_row_ror(float x) { return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x120 + N, 0xf, 0xf, false)); }
TR1_DEV float tr1_sum_xor32(float v) { float a, b; tr1_halves32(v, a, b); return a + b; }      // == v + __shfl_xor(v, 32, 64)
TR1_DEV float tr1_sum_xor16(float v) { float a, b; tr1_halves16(v, a, b); return a + b; }      // == v + __shfl_xor(v, 16, 64)
TR1_DEV float wave_sum(float v) {
    v = tr1_sum_xor32(v); v = tr1_sum_xor16(v);
    v += tr1_row_ror<8>(v); v += tr1_row_ror<4>(v); v += tr1_row_ror<2>(v); v += tr1_row_ror<1>(v);
    return v;
}
TR1_DEV float wave_max(float v) {
    float a, b;
    tr1_halves32(v, a, b); v = fmaxf(a, b);
    tr1_halves16(v, a, b); v = fmaxf(a, b);
    v = fmaxf(v, tr1_row_ror<8>(v)); v = fmaxf(v, tr1_row_ror<4>(v)); v = fmaxf(v, tr1_row_ror<2>(v)); v = fmaxf(v, tr1_row_ror<1>(v));
    return v;
}
// (value, index) pairs through the same exchanges: the larger value wins, equal values keep the LOWER index (torch.argmax made deterministic).  The index
// travels as raw bits (the swaps and rotations move registers, no float arithmetic touches it).  Every lane ends with the wave's pair.
TR1_DEV void tr1_argmax_pick(float& v, int& i, float pv, int pi) { if (pv > v || (pv == v && pi < i)) { v = pv; i = pi; } }
TR1_DEV void wave_argmax(float& v, int& i) {
    float a, b, ia, ib;
    tr1_halves32(v, a, b); tr1_halves32(__int_as_float(i), ia, ib); v = a; i = __float_as_int(ia); tr1_argmax_pick(v, i, b, __float_as_int(ib));
    tr1_halves16(v, a, b); tr1_halves16(__int_as_float(i), ia, ib); v = a; i = __float_as_int(ia); tr1_argmax_pick(v, i, b, __float_as_int(ib));
    tr1_argmax_pick(v, i, tr1_row_ror<8>(v), __float_as_int(tr1_row_ror<8>(__int_as_float(i))));
    tr1_argmax_pick(v, i, tr1_row_ror<4>(v), __float_as_int(tr1_row_ror<4>(__int_as_float(i))));
    tr1_argmax_pick(v, i, tr1_row_ror<2>(v), __float_as_int(tr1_row_ror<2>(__int_as_float(i))));
    tr1_argmax_pick(v, i, tr1_row_ror<1>(v), __float_as_int(tr1_row_ror<1>(__int_as_float(i))));
}

// block-wide sum for blockDim.x <= 1024 (multiple of 64); red must hold >= 16 floats
TR1_DEV float block_sum(float v, float* red) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    __syncthreads();
    if (lane == 0) red[wid] = v;
    __syncthreads();
    float t = (lane < nw) ? red[lane] : 0.f;
    t = wave_sum(t);
    return t;
}
TR1_DEV float block_max(float v, float* red) {
    v = wave_max(v);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    __syncthreads();
    if (lane == 0) red[wid] = v;
    __syncthreads();
    float t = (lane < nw) ? red[lane] : -INFINITY;
    t = wave_max(t);
    return t;
}

// ---- Philox4x32-10 (Salmon et al. 2011): the one counter-based generator of the library.  The sampler keys it by (seed; row, step, 0, 0), the bf16-moment AdamW by
// (seed; element / 4 low, element / 4 high, step, 0x53523136): the last counter word keeps the two streams apart.
TR1_DEV void philox4x32_10(unsigned c[4], unsigned k0, unsigned k1) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const unsigned long long p0 = 0xD2511F53ull * c[0], p1 = 0xCD9E8D57ull * c[2];      // one 32 x 32 -> 64 multiply each (v_mad_u64_u32), not a high and a low one
        const unsigned h0 = (unsigned)(p0 >> 32), l0 = (unsigned)p0, h1 = (unsigned)(p1 >> 32), l1 = (unsigned)p1;
        const unsigned n0 = h1 ^ c[1] ^ k0, n1 = l1, n2 = h0 ^ c[3] ^ k1, n3 = l0;
        c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}

// ---- what every kernel with a DMA-staged 128-byte-row LDS image shares (GEMMs, decode projections) ----
typedef const __attribute__((address_space(1))) void* gptr_t;      // operand types of __builtin_amdgcn_global_load_lds
typedef __attribute__((address_space(3))) void* lptr_t;
// Transposing LDS read (ds_read_b64_tr_b16): a 16-lane group reads a 4 x 16 block of 16-bit elements, each lane supplying an 8-byte address and receiving one column.
typedef __attribute__((ext_vector_type(4))) short tr1_s16x4_t;
TR1_DEV u32x2_t tr1_lds_read_tr16(const char* p) {
    const tr1_s16x4_t v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) tr1_s16x4_t*)(p));
    return __builtin_bit_cast(u32x2_t, v);
}
TR1_DEV int keyA(int row) { return (row >> 1) & 7; }               // row r keeps its logical 16-byte chunk c at position c ^ keyA(r): conflict-free 16-row fragment reads
// raw s_barrier pinned against the scheduler (no vmcnt(0) / lgkmcnt(0) drain as __syncthreads has: DMA stays in flight across it)
#define TR1_PIN() do { asm volatile("" ::: "memory"); __builtin_amdgcn_sched_barrier(0); } while (0)
#define TR1_BARRIER() do { TR1_PIN(); __builtin_amdgcn_s_barrier(); TR1_PIN(); } while (0)

// ---- LDS DMA (global -> LDS without a register round trip): each lane's 16 (tr1_dma16) / 4 (tr1_dma4) bytes at sbase + voff land at LDS byte address
// lds_addr (wave-uniform, it travels in m0) + lane * 16 / 4.  The instructions are written in assembly: for the builtin, hipcc tracks the asynchronous LDS
// write and puts an s_waitcnt vmcnt(0) in front of the next LDS read it cannot prove disjoint (all of them: one dynamic LDS array) - the "prefetch" then
// completes before the first operand read of the tile, i.e. nothing is prefetched (and a weight stream in flight is drained).  Landing is ordered by the
// caller's hand-counted vmcnt wait + barrier.
TR1_DEV void tr1_dma16(unsigned voff, const void* sbase, unsigned lds_addr) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" ::"s"(lds_addr), "v"(voff), "s"(sbase) : "memory", "m0");
}
TR1_DEV void tr1_dma4(unsigned voff, const void* sbase, unsigned lds_addr) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dword %1, %2" ::"s"(lds_addr), "v"(voff), "s"(sbase) : "memory", "m0");
}

// ---- host side error plumbing (C ABI returns int; message via tr1_last_error) ----
extern "C" void tr1_set_error_(const char* msg);

#define TR1_CHECK_ARG(cond, msg)                                  \
    do {                                                          \
        if (!(cond)) {                                            \
            tr1_set_error_(msg);                                  \
            return 1000;                                          \
        }                                                         \
    } while (0)

#define TR1_LAUNCH_CHECK()                                        \
    do {                                                          \
        hipError_t e__ = hipGetLastError();                       \
        if (e__ != hipSuccess) {                                  \
            tr1_set_error_(hipGetErrorString(e__));               \
            return (int)e__;                                      \
        }                                                         \
        return 0;                                                 \
    } while (0)

// ---- per-device host state.  A process normally drives ONE GPU, but tools and tests may touch more: the CU count and a kernel's raised
// dynamic-LDS limit belong to a device, so both are kept per device (ordinals 0..15).
inline int tr1_device() { int dev = 0; return (hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 16) ? dev : 0; }
inline int tr1_cu_count() {
    static int cached[16] = {0};
    const int dev = tr1_device();
    if (!cached[dev]) {
        hipDeviceProp_t pr;
        const int cus = (hipGetDeviceProperties(&pr, dev) == hipSuccess) ? pr.multiProcessorCount : 0;
        cached[dev] = cus > 0 ? cus : 256;
    }
    return cached[dev];
}
// once per device: tr1_launch keeps one per kernel
struct Tr1PerDevice {
    bool done[16] = {};
    bool first() { const int d = tr1_device(); if (done[d]) return false; return done[d] = true; }
};
// Every launch that may need more than 64 KiB of dynamic LDS: tr1_launch<kernel>(grid, block, dyn, lds_cap, stream, kernel arguments...).  lds_cap is the most
// the kernel is ever launched with (dyn itself where there is one size); above 64 KiB the kernel's limit is raised to it on the kernel's first launch on each
// device - the template holds one Tr1PerDevice per kernel, so a kernel that is launched is a kernel that was raised.  A failed raise surfaces at the launch
// (TR1_LAUNCH_CHECK).  The kernel is a function pointer here: its default arguments do not apply, pass every argument.
template <auto Kernel, class... A>
inline void tr1_launch(dim3 grid, dim3 block, size_t dyn, int lds_cap, hipStream_t s, A... args) {
    static Tr1PerDevice raised;
    if (lds_cap > 64 * 1024 && raised.first())
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds_cap);
    hipLaunchKernelGGL(Kernel, grid, block, dyn, s, args...);
}
// f(std::integral_constant<int, V>{}) for the V of the list that equals v (the last of the list where none does): a run-time tile height or stage count
// becomes a template argument in one place
template <int V0, int... Vs, class F>
inline void tr1_dispatch(int v, F f) {
    if constexpr (sizeof...(Vs) == 0) f(std::integral_constant<int, V0>{});
    else if (v == V0) f(std::integral_constant<int, V0>{});
    else tr1_dispatch<Vs...>(v, f);
}

// dw[c] += sum_b part[b][c] (the fixed-order second level of every per-block column reduction: norm weights, bias gradients), b in ascending order inside each of 16 row groups, groups combined in a fixed order.  64 columns per block.
static __global__ __launch_bounds__(1024) void norm_dw_reduce_kernel(const float* __restrict__ part, float* __restrict__ dw, int nblk, int cols) {
    __shared__ float red[16][64];
    const int cl = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cl;
    const int per = (nblk + 15) / 16, b0 = rg * per, b1 = min(nblk, b0 + per);
    float s = 0.f;
    if (c < cols) {
#pragma unroll 8
        for (int b = b0; b < b1; ++b) s += part[(size_t)b * cols + c];
    }
    red[rg][cl] = s;
    __syncthreads();
    if (rg == 0 && c < cols) {
        float t = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) t += red[i][cl];
        dw[c] += t;
    }
}

// out[0] += sum of part[0 .. n) in a fixed order (one block of 256: thread t adds part[t], part[t + 256], ...; then the block tree) - the second level
// of the per-block squared-norm partials
static __global__ __launch_bounds__(256) void partials_sum_kernel(const float* __restrict__ part, int64_t n, float* __restrict__ out) {
    __shared__ float red[16];
    float s = 0.f;
    for (int64_t i = threadIdx.x; i < n; i += 256) s += part[i];
    s = block_sum(s, red);
    if (threadIdx.x == 0) out[0] += s;
}

static inline int tr1_grid_1d(int64_t work_items, int per_block, int cap = 8192) {
    int64_t g = (work_items + per_block - 1) / per_block;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (int)g;
}

// ---- decode: q/k/v projection epilogue (shared by the bf16 and fp8 decode GEMMs) ---------------------------------------------------
// The fused QKV kernels give each block the column pair (d, d + hd/2) of one head, so rotate-half RoPE closes inside the block and the
// results go straight to their consumers: roped q -> q_out, roped k -> K cache row slots[m], v -> V^T cache column slots[m]
// (= tr1_decode_qkv_post folded into the projection; reference: Qwen2VLAttention.forward TF:521-556 + DynamicCache.update).
struct QkvEpi {
    const float* cosb; const float* sinb;            // [R, hd/2] fp32 tables of the rows' positions
    bf16_t* q_out; int64_t ld_q;
    bf16_t* kcache; int64_t k_ld;
    bf16_t* vtcache; int64_t vt_ld;
    const int* slots;
    int n_heads, n_kv, hd;
};
// rotate-half pair with explicitly rounded products (no fma contraction): the fused and the two-kernel decode paths must agree bit for bit
TR1_DEV void rope_pair(float a, float b, float c, float s, float& oa, float& ob) {
    oa = __fsub_rn(__fmul_rn(a, c), __fmul_rn(b, s));
    ob = __fadd_rn(__fmul_rn(b, c), __fmul_rn(a, s));
}
// vA / vB: projection outputs (bias included) of row m at columns h*hd + d and h*hd + hd/2 + d, already rounded to bf16 like the unfused path
TR1_DEV void qkv_epilogue_store(const QkvEpi& e, int m, int h, int d, float vA, float vB) {
    const int half = e.hd >> 1;
    if (h < e.n_heads + e.n_kv) {
        const float c = e.cosb[(int64_t)m * half + d], s = e.sinb[(int64_t)m * half + d];
        float fa, fb;
        rope_pair(vA, vB, c, s, fa, fb);
        const bf16_t oa = f2bf(fa), ob = f2bf(fb);
        bf16_t* dst = (h < e.n_heads) ? (e.q_out + (int64_t)m * e.ld_q + (int64_t)h * e.hd + d)
                                      : (e.kcache + (int64_t)e.slots[m] * e.k_ld + (int64_t)(h - e.n_heads) * e.hd + d);
        dst[0] = oa; dst[half] = ob;
    } else {
        bf16_t* col = e.vtcache + ((int64_t)(h - e.n_heads - e.n_kv) * e.hd + d) * e.vt_ld + e.slots[m];
        col[0] = f2bf(vA); col[(int64_t)half * e.vt_ld] = f2bf(vB);
    }
}
