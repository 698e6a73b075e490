// Losslessly packed 12-bit bf16 weights for the decode gate/up GEMM (gfx950): the packer and the packed twin of norm_glu_lds_kernel<NST, R, 2, 1, 0>
// (gemm_skinny.hip).  The gate/up launch is HBM-bound on streaming its [2I, K] weight once per decode step; the weights are constant over the ~200 steps of a
// rollout window, so they are re-encoded once per weight version into 75 % of the bytes and the twin streams that image.  The encoding is exact: the twin
// rebuilds the very bf16x8 MFMA operands the bf16 kernel reads, in the same order, so the stored bits are the same.
//
// Format.  A STAGE is what one wave consumes per step of its stream: 16 gate rows + 16 up rows of one column-group pair x 64 k = 2048 bf16 values.  Within a stage
// the values of exponent >> 1 (the low 7 bits of a bf16's HIGH byte) span a few binades below the stage's largest, so the high byte becomes a 4-bit code,
// sign << 3 | (exponent >> 1) - base, a window of 8 values of exponent >> 1 (16 binades).  base = max(0, the stage's largest exponent >> 1, minus 7) where that
// leaves at most PK_P values outside; otherwise the start (0 .. 120) of the window that covers most of the stage's values, among equals the highest: an outlier
// weight or an Inf then costs a patch of its own instead of pushing the small values out.  The LOW byte
// ((exponent & 1) << 7 | mantissa) is kept verbatim.  A value outside the window (zeros and denormals, Inf / NaN, rare tiny or huge values) gets code 0 and an
// entry (position, bf16 bits) in the stage's patch list, which overrides the element exactly; more than PK_P patches in any stage make the MATRIX not
// representable (the flag word), and decode keeps the bf16 kernel for it.
//   record (3072 bytes, one per stage, in the order the twin walks them: ((pair * 8 + wave) * NST + stage)): the LDS image itself, lane-major for the consumer -
//     plane A [64 lanes][16 B]: low bytes of the lane's two gate operands (k-half 0: elements 0..7, k-half 1: elements 0..7)
//     plane B [64 lanes][16 B]: the same for the up rows
//     plane C [64 lanes][16 B]: one code dword per operand (gate 0, gate 1, up 0, up 1); byte b = code(element b) | code(element b + 4) << 4
//     where lane = g * 16 + u holds row u, k = khalf * 32 + g * 8 + element: the operand layout of v_mfma_f32_16x16x32_bf16.  Three contiguous 1 KiB DMA
//     instructions per stage (the bf16 image: four), three conflict-free ds_read_b128 per lane (four).
//   tail (16 dwords per stage, a parallel array): base * 0x01010101, patch count, PK_P entries position << 16 | bits in ascending position;
//     position = (operand * 64 + lane) * 8 + element.  It travels by a FOURTH DMA instruction (16 lanes x 4 bytes) into the stage's ring slot rather than by scalar
//     loads: the stage keeps the four vector-memory operations the hand-counted vmcnt waits of the bf16 kernel assume, base and count arrive with the data they
//     describe, and no load with a register destination sits in the stream (hipcc drains the DMA queue in front of the first use of one).
#include "skinny_common.h"
#include "../../include/timer1_hip.h"

namespace {
constexpr int PK_REC = 3072;                 // bytes of a record
constexpr int PK_TAIL_DW = 16;               // dwords of a tail
// Patch capacity.  Per-stage patch counts over 14.7 M values (7168 stages): N(0, 0.02) mean 0.16 / max 3, U(-0.03, 0.03) 0.03 / 2, Student-t(3) 1.2 / 13 (18
// under the maximum alone).  14 is what a 64-byte tail (one HBM burst, 2 % of the record) holds next to base and count, and it clears the heaviest-tailed of the three.
constexpr int PK_P = PK_TAIL_DW - 2;
constexpr int PK_SLOT = PK_REC + PK_TAIL_DW * 4;      // ring slot: record + tail
constexpr int PK_RING = 4;                   // 3 stages (9 KiB + tails) of each wave in flight: what the bf16 kernel's ring of 3 x 4 KiB keeps (8 KiB), in the same LDS
constexpr int PK_REDW = 2 * 16 * 17;         // floats of one wave's partial (gate | up)

// x staging (2 KiB per 64-k stage of the wave's slice): ring slots 1 .. R-1 first (slot 0 takes the first weight stage meanwhile), then the two reduction
// slices, then a private area behind the norm-weight KiB
constexpr int pk_x_in_ring(int ring) { return (ring - 1) * PK_SLOT / 2048; }
constexpr int pk_x_extra(int nst, int ring) { return nst - pk_x_in_ring(ring) - 2 > 0 ? nst - pk_x_in_ring(ring) - 2 : 0; }
constexpr size_t pk_lds_bytes(int ring) {
    return (size_t)8 * ring * PK_SLOT + (2 * 8 * PK_REDW + 8 * 16) * sizeof(float) + 8 * 1024 + (size_t)8 * pk_x_extra(7, ring) * 2048;
}
static_assert(pk_lds_bytes(PK_RING) <= 160 * 1024, "LDS of the packed gate/up kernel");

// eight codes + eight low bytes -> the bf16x8 operand.  he / ho: the high bytes of elements 0..3 / 4..7 (sign | base + offset; base + 7 <= 127: no carry between bytes)
TR1_DEV bf16x8_t pk_unpack(unsigned l0, unsigned l1, unsigned c, unsigned base4) {
    const unsigned he = (((c << 4) & 0x80808080u) | ((c & 0x07070707u) + base4));
    const unsigned ho = ((c & 0x80808080u) | (((c >> 4) & 0x07070707u) + base4));
    u32x4_t o;
    o[0] = __builtin_amdgcn_perm(he, l0, 0x05010400u);
    o[1] = __builtin_amdgcn_perm(he, l0, 0x07030602u);
    o[2] = __builtin_amdgcn_perm(ho, l1, 0x05010400u);
    o[3] = __builtin_amdgcn_perm(ho, l1, 0x07030602u);
    return __builtin_bit_cast(bf16x8_t, o);
}
}  // namespace

// Same structure as norm_glu_lds_kernel<NST, R, 2, 1, 0> (see the notes there): persistent blocks over contiguous ranges of column-group pairs, x' fragments and
// sum x^2 once per block, one ring per wave ordered by that wave's counted vmcnt alone, wave-order reduction, the SwiGLU epilogue with its rounding points.  The
// weight path differs: a stage is 3 + 1 DMA instructions, and the operands are unpacked in registers.
template <int NST, int R>
__global__ __launch_bounds__(512) void norm_glu_lds_pk_kernel(const bf16_t* __restrict__ X, const bf16_t* __restrict__ lnw, const char* __restrict__ rec,
                                                              const unsigned* __restrict__ tails, bf16_t* __restrict__ C, int M, int64_t N, int64_t K,
                                                              int64_t ldx, int64_t ldc, float eps, int c_frag) {
    constexpr int REDW = PK_REDW, SLOT = PK_SLOT;
    constexpr int NXR = pk_x_in_ring(R), NXE = pk_x_extra(NST, R);
    static_assert(R >= 3 && R <= 4 && NXR + 2 + NXE >= NST, "x staging");
    // red[2][8][REDW] f32 | ssq[8][16] | [8 waves][R slots] | norm-weight KiB per wave | x stages
    extern __shared__ __attribute__((aligned(16))) char pk_lds[];
    float* red = reinterpret_cast<float*>(pk_lds);
    float* ssq = red + 2 * 8 * REDW;
    char* rings = pk_lds + (2 * 8 * REDW + 8 * 16) * sizeof(float);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, u = lane & 15, g = lane >> 4;
    const int64_t NP = N / 16;
    const int64_t p0 = NP * blockIdx.x / gridDim.x, p1 = NP * (blockIdx.x + 1) / gridDim.x;
    const int npair = (int)(p1 - p0);
    const int64_t kb = (int64_t)wave * (K / 8);
    char* ring = rings + wave * R * SLOT;
    const int total = npair * NST;
    // per-lane source pointers of the stage being ISSUED: the records (and tails) of a wave's NST stages of a pair are contiguous, the next pair's lie 8 NST further
    const char* prec = rec + ((p0 * 8 + wave) * NST) * (int64_t)PK_REC + lane * 16;
    const unsigned* ptail = tails + ((p0 * 8 + wave) * NST) * (int64_t)PK_TAIL_DW + (lane & 15);
    int islot = 0;
    // the three record instructions share one LDS base: the instruction offset is added to the LDS address as well as to the source
#define PK_ISSUE() do {                                                                                                   \
        char* dst__ = ring + islot * SLOT;                                                                                \
        __builtin_amdgcn_global_load_lds((gptr_t)prec, (lptr_t)dst__, 16, 0, TR1_W_AUX);                                  \
        __builtin_amdgcn_global_load_lds((gptr_t)prec, (lptr_t)dst__, 16, 1024, TR1_W_AUX);                               \
        __builtin_amdgcn_global_load_lds((gptr_t)prec, (lptr_t)dst__, 16, 2048, TR1_W_AUX);                               \
        if (lane < 16) __builtin_amdgcn_global_load_lds((gptr_t)ptail, (lptr_t)(dst__ + PK_REC), 4, 0, TR1_W_AUX);        \
        prec += PK_REC; ptail += PK_TAIL_DW;                                                                              \
        islot = (islot + 1 == R) ? 0 : islot + 1;                                                                         \
    } while (0)
#define PK_NEXT_PAIR() do { prec += (int64_t)7 * NST * PK_REC; ptail += (int64_t)7 * NST * PK_TAIL_DW; } while (0)
#define PK_PROLOGUE(I0, I1) do {                                                                                 \
        _Pragma("unroll") for (int i = (I0); i < (I1); ++i) {    /* prologue: items 0 .. R-2 */                  \
            if (i < total) {                                                                                     \
                if (i > 0 && i % NST == 0) PK_NEXT_PAIR();                                                       \
                PK_ISSUE();                                                                                      \
            }                                                                                                    \
        } } while (0)
    // ---- x' fragments of this wave's k-slice (once per block) and the row sums of squares: the slice goes by DMA through the still empty ring, the same
    // fragments in the same order as the bf16 kernel -> the same sum of squares
    bf16x8_t xr[NST * 2];
    {
        char* lnw_lds = rings + 8 * R * SLOT + wave * 1024;
        {
            int64_t col = kb + lane * 8;
            if (col + 8 > K) col = K - 8;
            __builtin_amdgcn_global_load_lds((gptr_t)(lnw + col), (lptr_t)lnw_lds, 16, 0, 0);
        }
        char* const x_extra = rings + 8 * R * SLOT + 8 * 1024 + wave * (NXE * 2048);
        auto x_stage = [&](int st) -> char* {
            if (st < NXR) return ring + SLOT + st * 2048;
            if (st - NXR < 2) return reinterpret_cast<char*>(red + ((st - NXR) * 8 + wave) * REDW);
            return x_extra + (st - NXR - 2) * 2048;
        };
        float ss = 0.f;
#pragma unroll
        for (int st = 0; st < NST; ++st) {
            char* dst = x_stage(st);
#pragma unroll
            for (int jx = 0; jx < 2; ++jx) {
                const int r = 8 * jx + (lane >> 3);
                const bf16_t* src = X + (int64_t)(r < M ? r : M - 1) * ldx + kb + st * 64 + (((lane & 7) ^ keyA(r & 15)) << 3);
                __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(dst + jx * 1024), 16, 0, 0);
            }
        }
        PK_PROLOGUE(0, 1);                                            // the first weight stage travels while x' is built
        if (total > 0) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");   // everything but that stage's four DMA instructions has landed
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
        for (int i = 0; i < NST * 2; ++i) {
            const int st = i >> 1, ks = i & 1;
            const char* sbx = x_stage(st);
            const bf16x8_t xv = *reinterpret_cast<const bf16x8_t*>(sbx + u * 128 + (((ks * 4 + g) ^ keyA(u)) << 4));
            const bf16x8_t lvi = *reinterpret_cast<const bf16x8_t*>(lnw_lds + (i * 32 + g * 8) * 2);
            u32x4_t f = __builtin_bit_cast(u32x4_t, scale_frag_sumsq(xv, lvi, ss));
            asm volatile("" : "+v"(f));
            xr[i] = __builtin_bit_cast(bf16x8_t, f);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");              // the ring is free again: continue the weight stream
        float v = ss;
        v += __shfl_xor(v, 16, 64);
        v += __shfl_xor(v, 32, 64);
        if (g == 0) ssq[wave * 16 + u] = v;
        PK_PROLOGUE(1, R - 1);
    }
    TR1_BARRIER();                                       // the eight waves' sum-of-squares partials are in LDS (the prologue DMA is in flight)
    float rstd;
    {
        float sq = 0.f;
#pragma unroll
        for (int w = 0; w < 8; ++w) sq += ssq[w * 16 + ((threadIdx.x >> 4) & 15)];
        rstd = rsqrtf(sq * (1.f / (float)K) + eps);
    }
    const int rd_off = lane * 16;
    int cslot = 0;                                       // ring slot of the item being consumed
    for (int pi = 0; pi < npair; ++pi) {
        f32x4_t ag[2], au[2];
        ag[0] = ag[1] = au[0] = au[1] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int st = 0; st < NST; ++st) {
            const int item = pi * NST + st;
            if (item + R - 1 < total) {
                if ((st + R - 1) % NST == 0) PK_NEXT_PAIR();           // the issue stream enters the next pair here (compile-time position)
                PK_ISSUE();
            }
            const int rem = total - 1 - item;              // items issued after this one and still allowed in flight
            if (rem >= R - 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 * (R - 1)) : "memory");
            else if (rem == 2 && R > 3) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
            else if (rem == 1 && R > 2) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const char* slot = ring + cslot * SLOT;
            cslot = (cslot + 1 == R) ? 0 : cslot + 1;
            const u32x4_t la = *reinterpret_cast<const u32x4_t*>(slot + rd_off);
            const u32x4_t lb = *reinterpret_cast<const u32x4_t*>(slot + 1024 + rd_off);
            const u32x4_t cc = *reinterpret_cast<const u32x4_t*>(slot + 2048 + rd_off);
            const u32x2_t hd = *reinterpret_cast<const u32x2_t*>(slot + PK_REC);      // base x4, patch count (the same address in every lane: a broadcast)
            u32x4_t w4[4];                                  // gate k-half 0, gate 1, up 0, up 1
            w4[0] = __builtin_bit_cast(u32x4_t, pk_unpack(la[0], la[1], cc[0], hd[0]));
            w4[1] = __builtin_bit_cast(u32x4_t, pk_unpack(la[2], la[3], cc[1], hd[0]));
            w4[2] = __builtin_bit_cast(u32x4_t, pk_unpack(lb[0], lb[1], cc[2], hd[0]));
            w4[3] = __builtin_bit_cast(u32x4_t, pk_unpack(lb[2], lb[3], cc[3], hd[0]));
            const int npatch = __builtin_amdgcn_readfirstlane((int)hd[1]);
            if (npatch != 0) {                              // wave-uniform and rare: the owning lane overrides the element with the stored bits
                for (int i = 0; i < npatch; ++i) {
                    const unsigned e = *reinterpret_cast<const unsigned*>(slot + PK_REC + 8 + i * 4);
                    const int pos = (int)(e >> 16);
                    const bool mine = ((pos >> 3) & 63) == lane;
                    const int dw = ((pos >> 9) << 2) | ((pos >> 1) & 3);
                    const unsigned keep = (pos & 1) ? 0x0000ffffu : 0xffff0000u, put = (pos & 1) ? (e << 16) : (e & 0xffffu);
#pragma unroll
                    for (int q = 0; q < 16; ++q)
                        if (mine && dw == q) w4[q >> 2][q & 3] = (w4[q >> 2][q & 3] & keep) | put;
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) asm volatile("" : "+v"(w4[q]));
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                ag[ks] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, w4[ks]), xr[st * 2 + ks], ag[ks], 0, 0, 0);
                au[ks] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, w4[2 + ks]), xr[st * 2 + ks], au[ks], 0, 0, 0);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");          // this stage's reads have returned before its slot can be refilled
        }
        float* rw = red + ((pi & 1) * 8 + wave) * REDW;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            rw[u * 17 + g * 4 + r] = ag[0][r] + ag[1][r];
            rw[16 * 17 + u * 17 + g * 4 + r] = au[0][r] + au[1][r];
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        TR1_BARRIER();                                                  // partial tiles are visible; the DMA of the next pair stays in flight
        if (threadIdx.x < 256) {
            const int mm = (threadIdx.x >> 4) & 15, nn = threadIdx.x & 15;
            const float* rb = red + (pi & 1) * 8 * REDW;
            float v = 0.f, v2 = 0.f;
#pragma unroll
            for (int w = 0; w < 8; ++w) { v += rb[w * REDW + mm * 17 + nn]; v2 += rb[w * REDW + 16 * 17 + mm * 17 + nn]; }
            v = __fmul_rn(v, rstd);
            const float gt = bf2f(f2bf(v)), up = bf2f(f2bf(v2 * rstd));
            const int64_t n = (p0 + pi) * 16 + nn;
            if (mm < M && n < N) C[c_frag ? (n >> 5) * 512 + mm * 32 + (n & 31) : (int64_t)mm * ldc + n] = f2bf(bf2f(f2bf(silu_f32(gt))) * up);
        }
    }
#undef PK_ISSUE
#undef PK_NEXT_PAIR
#undef PK_PROLOGUE
}

// ---- packer: one block per stage (256 threads = 4 operands x 64 lanes, eight values each); the record and its tail are assembled in LDS and leave in 16-byte
// vector stores.  Patches are listed in ascending position (a fixed order: the image is a function of the weights alone).
template <int NST>
__global__ __launch_bounds__(256) void pack_bf16_glu_kernel(const bf16_t* __restrict__ W, int64_t I, int64_t K, int64_t ldw, char* __restrict__ rec,
                                                            unsigned* __restrict__ tails, int* __restrict__ flag) {
    __shared__ __attribute__((aligned(16))) unsigned img[(PK_REC + PK_TAIL_DW * 4) / 4];
    __shared__ int s_hist[128], s_max, s_best, s_total[2];
    __shared__ unsigned char s_cnt[256];
    const int t = threadIdx.x, op = t >> 6, lane = t & 63, u = lane & 15, g = lane >> 4;
    const int64_t r = blockIdx.x;
    const int st = (int)(r % NST), wv = (int)((r / NST) & 7);
    const int64_t p = r / (8 * NST);
    if (t < 128) s_hist[t] = 0;
    if (t == 0) { s_max = 0; s_best = 0; s_total[0] = 0; s_total[1] = 0; }
    if (t < PK_TAIL_DW) img[PK_REC / 4 + t] = 0;
    const int64_t row = ((op >> 1) ? I : 0) + p * 16 + u, k = (int64_t)wv * (K / 8) + st * 64 + (op & 1) * 32 + g * 8;
    const u32x4_t v = *reinterpret_cast<const u32x4_t*>(W + row * ldw + k);
    unsigned h[8];
    int mx = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        h[e] = (e & 1) ? v[e >> 1] >> 16 : v[e >> 1] & 0xffffu;
        mx = max(mx, (int)((h[e] >> 8) & 0x7f));
    }
    mx = (int)wave_max((float)mx);
    __syncthreads();
    if (lane == 0) atomicMax(&s_max, mx);
    __syncthreads();
    unsigned code, lo0 = 0, lo1 = 0, pmask;
#pragma unroll
    for (int e = 0; e < 8; ++e)
        if (e < 4) lo0 |= (h[e] & 0xffu) << (e * 8); else lo1 |= (h[e] & 0xffu) << ((e - 4) * 8);
    auto encode = [&](int base) {
        code = 0; pmask = 0;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int off = (int)((h[e] >> 8) & 0x7f) - base;
            const bool in = off >= 0 && off <= 7;
            const unsigned nib = in ? ((h[e] >> 15) << 3 | (unsigned)off) : 0u;
            code |= nib << ((e & 3) * 8 + (e >> 2) * 4);
            if (!in) pmask |= 1u << e;
        }
    };
    // the window under the stage's largest value where that leaves at most PK_P patches (nearly every stage of real weights: no histogram needed) ...
    int base = s_max > 7 ? s_max - 7 : 0;
    encode(base);
    if (pmask) atomicAdd(&s_total[0], __popc(pmask));
    __syncthreads();
    int total = s_total[0];
    if (total > PK_P) {                                   // ... else the window of 8 that covers most values, among equals the highest (block-uniform branch)
        // histogram of exponent >> 1 over the stage.  A wave's values sit in a handful of bins: one LDS add per distinct bin of the wave, not one per value
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int bin = (h[e] >> 8) & 0x7f;
            bool todo = true;
            for (unsigned long long m = __ballot(todo); m; m = __ballot(todo)) {
                const int b = __builtin_amdgcn_readlane(bin, __ffsll((long long)m) - 1);
                const unsigned long long same = __ballot(todo && bin == b);
                if (bin == b) { if (todo && lane == __ffsll((long long)same) - 1) atomicAdd(&s_hist[b], __popcll(same)); todo = false; }
            }
        }
        __syncthreads();
        if (t <= 120) {
            int cov = 0;
#pragma unroll
            for (int j = 0; j < 8; ++j) cov += s_hist[t + j];
            atomicMax(&s_best, cov * 128 + t);
        }
        __syncthreads();
        base = s_best & 127;
        encode(base);
        if (pmask) atomicAdd(&s_total[1], __popc(pmask));
        __syncthreads();
        total = s_total[1];
    }
    const int mine = __popc(pmask);
    img[(op >> 1) * 256 + lane * 4 + (op & 1) * 2] = lo0;
    img[(op >> 1) * 256 + lane * 4 + (op & 1) * 2 + 1] = lo1;
    img[512 + lane * 4 + op] = code;
    if (total != 0) {
        s_cnt[t] = (unsigned char)mine;
        __syncthreads();
        if (mine) {
            int at = 0;
            for (int i = 0; i < t; ++i) at += s_cnt[i];
#pragma unroll
            for (int e = 0; e < 8; ++e)
                if (pmask >> e & 1) { if (at < PK_P) img[PK_REC / 4 + 2 + at] = (unsigned)(t * 8 + e) << 16 | h[e]; ++at; }
        }
        if (t == 0) { img[PK_REC / 4 + 1] = (unsigned)(total < PK_P ? total : PK_P); if (total > PK_P) *flag = 1; }
    }
    if (t == 0) img[PK_REC / 4] = (unsigned)base * 0x01010101u;
    __syncthreads();
    const u32x4_t* src = reinterpret_cast<const u32x4_t*>(img);
    if (t < PK_REC / 16) reinterpret_cast<u32x4_t*>(rec + r * PK_REC)[t] = src[t];
    else if (t < PK_REC / 16 + PK_TAIL_DW / 4) reinterpret_cast<u32x4_t*>(tails + r * PK_TAIL_DW)[t - PK_REC / 16] = src[t];
}

// ---- host side: the four entry points of the packed path (include/timer1_hip.h); the decode driver calls tr1_norm_glu_pk per layer.  The packed IMAGE of a
// [2I, K] weight is one buffer: pk_stages(I, K) records of 3072 bytes, then as many tails of 64 bytes, then 16 bytes whose first int is the flag (1: some stage
// needs more than PK_P patches - the matrix is not representable, keep the bf16 kernel).
static int64_t pk_stages(int64_t I, int64_t K) { return (I / 16) * 8 * (K / 512); }

// <= 16 rows, whole column-group pairs, K = 512 * {7, 4, 3}
extern "C" int tr1_glu_pk_ok(int64_t M, int64_t I, int64_t K) { return M >= 1 && M <= 16 && I >= 16 && I % 16 == 0 && skinny_lds_stream_k(K); }

extern "C" int64_t tr1_glu_pk_image_bytes(int64_t I, int64_t K) { return pk_stages(I, K) * (PK_REC + PK_TAIL_DW * 4) + 16; }

extern "C" int tr1_pack_bf16_glu(const void* W, int64_t I, int64_t K, int64_t ldw, void* image, void* stream) {
    TR1_CHECK_ARG(tr1_glu_pk_ok(1, I, K), "pack_bf16_glu: I % 16 == 0 and K = 512 * {7, 4, 3} required");
    TR1_CHECK_ARG(W && image && ldw % 8 == 0 && ldw >= K, "pack_bf16_glu: null argument or ldw % 8");
    TR1_CHECK_ARG(((uintptr_t)W | (uintptr_t)image) % 16 == 0, "pack_bf16_glu: 16-byte aligned buffers required");
    hipStream_t s = (hipStream_t)stream;
    const int64_t nrec = pk_stages(I, K);
    char* rec = (char*)image;
    unsigned* tails = (unsigned*)(rec + nrec * PK_REC);
    int* flag = (int*)(rec + nrec * (PK_REC + PK_TAIL_DW * 4));
    if (hipMemsetAsync(flag, 0, 16, s) != hipSuccess) { tr1_set_error_("pack_bf16_glu: memset failed"); return 1001; }
    tr1_dispatch<7, 4, 3>((int)(K / 512), [&](auto NST) {
        hipLaunchKernelGGL((pack_bf16_glu_kernel<decltype(NST)::value>), dim3((unsigned)nrec), dim3(256), 0, s, (const bf16_t*)W, I, K, ldw, rec, tails, flag);
    });
    TR1_LAUNCH_CHECK();
}

// out = silu(gate) * up of rmsnorm(x; lnw) against the packed image (flag 0): the bits the bf16 launch stores.  frag: fragment-major output (tr1_norm_gemm_glu_frag_ok)
extern "C" int tr1_norm_glu_pk(const void* x, const void* lnw, const void* image, void* out, int64_t M, int64_t I, int64_t K, int64_t ldx, int64_t ldc, float eps,
                               int frag, void* stream) {
    TR1_CHECK_ARG(tr1_glu_pk_ok(M, I, K), "norm_glu_pk: M <= 16, I % 16 == 0, K = 512 * {7, 4, 3} required");
    TR1_CHECK_ARG(x && lnw && image && out && ldx % 8 == 0 && ldc % 8 == 0, "norm_glu_pk: null argument or ldx % 8, ldc % 8");
    TR1_CHECK_ARG(!frag || I % 32 == 0, "norm_glu_pk: fragment-major output needs I % 32 == 0");
    const int64_t NP = I / 16, n_cu = tr1_cu_count(), nrec = pk_stages(I, K);
    const unsigned grid = (unsigned)(NP < n_cu ? NP : n_cu);
    constexpr size_t dyn = pk_lds_bytes(PK_RING);
    const char* rec = (const char*)image;
    tr1_dispatch<7, 4, 3>((int)(K / 512), [&](auto NST) {
        tr1_launch<norm_glu_lds_pk_kernel<decltype(NST)::value, PK_RING>>(dim3(grid), dim3(512), dyn, (int)dyn, (hipStream_t)stream, (const bf16_t*)x,
                                                                         (const bf16_t*)lnw, rec, (const unsigned*)(rec + nrec * PK_REC), (bf16_t*)out, (int)M, I, K,
                                                                         ldx, ldc, eps, frag ? 1 : 0);
    });
    TR1_LAUNCH_CHECK();
}
