// Rollout sampler for gfx950: repetition penalty, temperature + top-k + top-p + min-p, an inverse-CDF draw keyed by Philox, and greedy decoding - the kernels
// that turn one decode step's lm_head logits into one token per row, with their C entry points.
// Reference semantics: HF generate(do_sample, temperature, top_k, top_p, min_p, repetition_penalty); greedy = generate(do_sample=False).
#include "tr1_common.h"
#include "../../include/timer1_hip.h"

// ---------------------------------------------------------------------------------------------------------------------
// Sampler: one 1024-thread block per rollout row. x = logits / temperature; keep the top_k largest (ties with the k-th
// value kept, as HF's TopKLogitsWarper does); softmax over the kept set; inverse-CDF draw in vocabulary order with a
// Philox4x32-10 uniform keyed by (seed, row, step).  top_k <= 0 disables the filter.
// ---------------------------------------------------------------------------------------------------------------------
// 16-bit order-preserving key of a bf16 logit (temperature > 0 does not change the order, so top-k is selected on raw logits)
TR1_DEV unsigned bfkey(bf16_t b) { return (b & 0x8000u) ? ((~(unsigned)b) & 0xffffu) : ((unsigned)b | 0x8000u); }
// +0.0 and -0.0 compare equal as floats, so a k-th value of +0.0 ties with every -0.0 (HF's warper keeps both); -0.0 holds the next lower key
TR1_DEV unsigned samp_zero_tie(unsigned thr) { return thr == 0x8000u ? 0x7fffu : thr; }
TR1_DEV float key_logit(unsigned k) { const unsigned b = (k & 0x8000u) ? (k & 0x7fffu) : ((~k) & 0xffffu); return bf2f((bf16_t)b); }

// Multi-block sampler.  The vocabulary row (152k bf16 logits, L2 resident) is cut into SAMP_S slices, one 256-thread block each:
//   1. hist_hi   : 256-bin histogram of the key's high byte (+ row max)           -> finds the byte holding the k-th largest logit
//   2. hist_lo   : histogram of the low byte among logits in that high-byte bin    -> exact k-th largest 16-bit key = threshold
//   3. slice_sum : sum exp((x - max)/T) over kept logits per slice
//   4. pick      : Philox uniform, locate the slice and the token by an inverse-CDF walk in vocabulary order
// Workspace per row (uint32 words): hist_hi[256] | hist_lo[256] | misc[8] (0: max key) | slice sums[SAMP_S] (float)
#define SAMP_S 32
#define SAMP_WS_WORDS (256 + 256 + 8 + SAMP_S)
// top-p / min-p extension per row: mass_hi[256] | mass_lo[256] (64-bit fixed point, 2 words each) | misc[8] (0: final threshold key)
#define SAMP_EXT_WORDS (512 + 512 + 8)

struct SampleArgs {
    const bf16_t* logits; int64_t ld; int V; float inv_temp; int top_k; unsigned long long seed; int group_rows; unsigned long long seed_stride; const int* step_ptr; int* tokens; int64_t tok_ld;
    int* finished; int eos_id, pad_id, stop_at_eos; float* u_out; unsigned* ws;
    int* next_ids;      // optional [rows]: the drawn token once more, where the next decode step's embedding gather reads it (no copy kernel in between)
    int ws_clean;       // the caller zero-filled ws once: the fused pick kernel re-zeroes what the histogram kernels dirtied (no memset per call)
    int* done_count;    // optional [1]: += 1 when a row's finished flag goes 0 -> 1 (the early-stop poll of a sampled rollout reads it); NULL = off
};
// The launches of the top-p / min-p path carry three more arguments; without those filters the kernels receive SampleArgs and run the code they always ran.
struct SampleArgsF : SampleArgs {
    unsigned* ext;      // SAMP_EXT_WORDS per row behind the rows' SAMP_WS_WORDS blocks; word 1024 = the final threshold key
    float top_p, min_p;
};

TR1_DEV bool samp_row_done(const SampleArgs& a, int r) { return a.finished && a.stop_at_eos && a.finished[r]; }
// The one lane that wrote the row's token: EOS raises finished[r]; done_count counts the 0 -> 1 transition only (a second EOS of a row that runs on with
// stop_at_eos = 0 finds the flag set; rows skipped as done never get here).  finished[r] is written by this lane alone, so the read needs no atomic.
TR1_DEV void samp_mark_eos(const SampleArgs& a, int r, int tok) {
    if (!a.finished || tok != a.eos_id) return;
    if (a.done_count && !a.finished[r]) atomicAdd(a.done_count, 1);
    a.finished[r] = 1;
}

// threshold search over a 256-bin histogram: largest bin b with (count of keys in bins > b) < need <= (count in bins >= b)
TR1_DEV void samp_find_bin(const unsigned* hist, int need, int& bin, int& rem) {
    int acc = 0; int b = 255;
    for (; b > 0; --b) { if (acc + (int)hist[b] >= need) break; acc += (int)hist[b]; }
    bin = b; rem = need - acc;
}

// The same search by the first 256 threads of a block (one bin each, from the top): a suffix scan replaces the up-to-255 dependent reads of the
// serial walk (12 us of a 26 us launch).  hist: 256 bins in LDS; scr: 8 unsigned of LDS scratch; result in *bin_out / *rem_out (LDS).
TR1_DEV void samp_find_bin_par(const unsigned* hist, int need, unsigned* scr, int* bin_out, int* rem_out) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    unsigned val = 0u, incl = 0u;
    if (tid < 256) {
        val = hist[255 - tid];
        incl = val;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const unsigned t = __shfl_up(incl, d, 64); if (lane >= d) incl += t; }
        if (lane == 63) scr[w] = incl;
    }
    if (tid == 0) { *bin_out = 0; *rem_out = -1; }
    __syncthreads();
    if (tid < 256) {
        unsigned off = 0u;
        for (int j = 0; j < w; ++j) off += scr[j];
        incl += off;
        const unsigned excl = incl - val;
        if (tid < 255 && (int)incl >= need && (int)excl < need) { *bin_out = 255 - tid; *rem_out = need - (int)excl; }   // exactly one thread
        if (tid == 254) scr[4] = incl;                                            // count in bins 255 .. 1 (fallback: bin 0)
    }
    __syncthreads();
    if (tid == 0 && *rem_out < 0) *rem_out = need - (int)scr[4];
    __syncthreads();
}

__global__ __launch_bounds__(256) void samp_hist_hi_kernel(SampleArgs a) {
    __shared__ unsigned h[256];
    __shared__ unsigned smax;
    const int r = blockIdx.y;
    if (samp_row_done(a, r)) return;
    h[threadIdx.x] = 0u; if (threadIdx.x == 0) smax = 0u;
    __syncthreads();
    const bf16_t* row = a.logits + (int64_t)r * a.ld;
    const int per = (a.V + SAMP_S - 1) / SAMP_S, i0 = blockIdx.x * per, i1 = min(a.V, i0 + per);
    unsigned mx = 0u;
    for (int i = i0 + threadIdx.x; i < i1; i += 256) { const unsigned k = bfkey(row[i]); mx = max(mx, k); atomicAdd(&h[k >> 8], 1u); }
    atomicMax(&smax, mx);
    __syncthreads();
    unsigned* ws = a.ws + (int64_t)r * SAMP_WS_WORDS;
    if (h[threadIdx.x]) atomicAdd(&ws[threadIdx.x], h[threadIdx.x]);
    if (threadIdx.x == 0) atomicMax(&ws[512], smax);
}

__global__ __launch_bounds__(256) void samp_hist_lo_kernel(SampleArgs a) {
    __shared__ unsigned h[256];
    __shared__ int sbin;
    const int r = blockIdx.y;
    if (samp_row_done(a, r)) return;
    unsigned* ws = a.ws + (int64_t)r * SAMP_WS_WORDS;
    __shared__ unsigned hh[256], scr[8];
    __shared__ int srem;
    h[threadIdx.x] = 0u;
    hh[threadIdx.x] = ws[threadIdx.x];
    __syncthreads();
    samp_find_bin_par(hh, a.top_k, scr, &sbin, &srem);
    const unsigned bin = (unsigned)sbin;
    const bf16_t* row = a.logits + (int64_t)r * a.ld;
    const int per = (a.V + SAMP_S - 1) / SAMP_S, i0 = blockIdx.x * per, i1 = min(a.V, i0 + per);
    for (int i = i0 + threadIdx.x; i < i1; i += 256) { const unsigned k = bfkey(row[i]); if ((k >> 8) == bin) atomicAdd(&h[k & 255u], 1u); }
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(&ws[256 + threadIdx.x], h[threadIdx.x]);
}

// EXT (top-p / min-p): samp_filter_thr_kernel has folded all three filters into one key, word 1024 of the row's extension block
template <bool EXT> TR1_DEV unsigned samp_threshold(const SampleArgs& a, const unsigned* ws, const unsigned* ext, int r) {   // 16-bit key of the k-th largest logit (0 = keep all)
    if (EXT) return ext[(int64_t)r * SAMP_EXT_WORDS + 1024];
    if (a.top_k <= 0 || a.top_k >= a.V) return 0u;
    int bin, rem, lo, rem2;
    samp_find_bin(ws, a.top_k, bin, rem);
    samp_find_bin(ws + 256, rem, lo, rem2);
    return samp_zero_tie(((unsigned)bin << 8) | (unsigned)lo);
}

template <bool EXT> TR1_DEV void samp_slice_sum_body(const SampleArgs& a, unsigned* ext) {
    __shared__ float red[16];
    __shared__ unsigned sthr;
    const int r = blockIdx.y;
    if (samp_row_done(a, r)) return;
    unsigned* ws = a.ws + (int64_t)r * SAMP_WS_WORDS;
    if (threadIdx.x == 0) sthr = samp_threshold<EXT>(a, ws, ext, r);
    __syncthreads();
    const unsigned thr = sthr;
    const float mx = key_logit(ws[512]);
    const bf16_t* row = a.logits + (int64_t)r * a.ld;
    const int per = (a.V + SAMP_S - 1) / SAMP_S, i0 = blockIdx.x * per, i1 = min(a.V, i0 + per);
    float acc = 0.f;
    for (int i = i0 + threadIdx.x; i < i1; i += 256) { const bf16_t b = row[i]; if (bfkey(b) >= thr) acc += __expf((bf2f(b) - mx) * a.inv_temp); }
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) reinterpret_cast<float*>(ws + 520)[blockIdx.x] = acc;
}
__global__ __launch_bounds__(256) void samp_slice_sum_kernel(SampleArgs a) { samp_slice_sum_body<false>(a, nullptr); }
__global__ __launch_bounds__(256) void samp_slice_sum_ext_kernel(SampleArgsF a) { samp_slice_sum_body<true>(a, a.ext); }

template <bool EXT> TR1_DEV void samp_pick_body(const SampleArgs& a, unsigned* ext) {
    __shared__ float part[256];
    __shared__ unsigned sthr; __shared__ int sslice; __shared__ float sbase, starget;
    const int r = blockIdx.x, tid = threadIdx.x;
    const int step = a.step_ptr ? *a.step_ptr : 0;
    int* tok_out = a.tokens + (int64_t)r * a.tok_ld + step;
    if (samp_row_done(a, r)) { if (tid == 0) { *tok_out = a.pad_id; if (a.next_ids) a.next_ids[r] = a.pad_id; } return; }
    unsigned* ws = a.ws + (int64_t)r * SAMP_WS_WORDS;
    const float* sums = reinterpret_cast<const float*>(ws + 520);
    if (tid == 0) {
        sthr = samp_threshold<EXT>(a, ws, ext, r);
        float Z = 0.f;
        for (int i = 0; i < SAMP_S; ++i) Z += sums[i];
        // several prompts in one launch: rows [b*group_rows, (b+1)*group_rows) use seed + b*seed_stride and their row index inside the group,
        // i.e. exactly the stream a separate launch per prompt would draw
        const int grp = a.group_rows > 0 ? r / a.group_rows : 0;
        const unsigned long long sd = a.seed + (unsigned long long)grp * a.seed_stride;
        unsigned c[4] = {(unsigned)(a.group_rows > 0 ? r % a.group_rows : r), (unsigned)step, 0u, 0u};
        philox4x32_10(c, (unsigned)(sd & 0xffffffffu), (unsigned)(sd >> 32));
        const float uu = ((float)(c[0] >> 8) + 0.5f) * (1.0f / 16777216.0f);
        if (a.u_out) a.u_out[r] = uu;
        const float target = uu * Z;
        float acc = 0.f; int sl = 0;
        for (; sl < SAMP_S - 1; ++sl) { if (acc + sums[sl] >= target) break; acc += sums[sl]; }
        sslice = sl; sbase = acc; starget = target;
    }
    __syncthreads();
    const unsigned thr = sthr;
    const float mx = key_logit(ws[512]);
    const bf16_t* row = a.logits + (int64_t)r * a.ld;
    const int per = (a.V + SAMP_S - 1) / SAMP_S, i0 = sslice * per, i1 = min(a.V, i0 + per);
    const int tper = (per + 255) / 256, j0 = i0 + tid * tper, j1 = min(i1, j0 + tper);   // contiguous run per thread: vocabulary order
    float acc = 0.f;
    for (int i = j0; i < j1; ++i) { const bf16_t b = row[i]; if (bfkey(b) >= thr) acc += __expf((bf2f(b) - mx) * a.inv_temp); }
    part[tid] = acc;
    __syncthreads();
    if (tid == 0) {
        float c = sbase; int t = 0;
        for (; t < 255; ++t) { if (c + part[t] >= starget) break; c += part[t]; }
        int tok = -1, last_kept = -1;
        const int k0 = i0 + t * tper, k1 = min(i1, k0 + tper);
        for (int i = k0; i < k1; ++i) {
            const bf16_t b = row[i];
            if (bfkey(b) >= thr) { last_kept = i; c += __expf((bf2f(b) - mx) * a.inv_temp); if (c >= starget) { tok = i; break; } }
        }
        if (tok < 0) {   // rounding slack: fall back to the last kept token at or before this point
            if (last_kept >= 0) tok = last_kept;
            else { for (int i = min(k1, a.V) - 1; i >= 0; --i) { if (bfkey(row[i]) >= thr) { tok = i; break; } } }
            if (tok < 0) { for (int i = 0; i < a.V; ++i) { if (bfkey(row[i]) >= thr) { tok = i; break; } } }
        }
        *tok_out = tok;
        if (a.next_ids) a.next_ids[r] = tok;
        samp_mark_eos(a, r, tok);
    }
}
__global__ __launch_bounds__(256) void samp_pick_kernel(SampleArgs a) { samp_pick_body<false>(a, nullptr); }
__global__ __launch_bounds__(256) void samp_pick_ext_kernel(SampleArgsF a) { samp_pick_body<true>(a, a.ext); }

// slice_sum + pick in ONE launch, one 1024-thread block per row (the separate pair cost 15 + 33 us per decode step, most of it the serial
// walks of thread 0).  The 16 waves own contiguous segments of the row; a wave reads its segment coalesced (64 lanes x 16 bytes per
// iteration) and keeps the per-iteration wave sums, so the inverse-CDF walk in vocabulary order is a three-level search (segment ->
// iteration -> lane) with one lane finally walking 8 logits.  Needs V % 8 == 0, ld % 8 == 0 and V <= SAMP_FUSED_MAXV.
#define SAMP_MAXIT 20
#define SAMP_FUSED_MAXV (16 * 64 * SAMP_MAXIT * 8)
template <bool EXT> TR1_DEV void samp_sum_pick_body(const SampleArgs& a, unsigned* ext) {
    __shared__ float wsum[16];
    __shared__ unsigned sthr; __shared__ int sseg; __shared__ float sbase, starget;
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int step = a.step_ptr ? *a.step_ptr : 0;
    int* tok_out = a.tokens + (int64_t)r * a.tok_ld + step;
    if (samp_row_done(a, r)) { if (tid == 0) { *tok_out = a.pad_id; if (a.next_ids) a.next_ids[r] = a.pad_id; } return; }
    unsigned* ws = a.ws + (int64_t)r * SAMP_WS_WORDS;
    __shared__ unsigned shist[512];                 // both histograms staged once: the threshold search of thread 0 then walks LDS, not global memory
    __shared__ unsigned scr[8];
    __shared__ int sbin, srem, slo, srem2;
    if (tid < 512) shist[tid] = ws[tid];
    __syncthreads();
    if (EXT) { if (tid == 0) sthr = ext[(int64_t)r * SAMP_EXT_WORDS + 1024]; __syncthreads(); }
    else if (a.top_k <= 0 || a.top_k >= a.V) { if (tid == 0) sthr = 0u; __syncthreads(); }
    else {
        samp_find_bin_par(shist, a.top_k, scr, &sbin, &srem);
        samp_find_bin_par(shist + 256, srem, scr, &slo, &srem2);
        if (tid == 0) sthr = samp_zero_tie(((unsigned)sbin << 8) | (unsigned)slo);
        __syncthreads();
    }
    const unsigned thr = sthr;
    const float mx = key_logit(ws[512]);
    const bf16_t* row = a.logits + (int64_t)r * a.ld;
    const int nch = a.V >> 3, seg = (nch + 15) >> 4, c0 = wave * seg, c1 = min(nch, c0 + seg);
    const int nit = (seg + 63) >> 6;
    // all loads of the segment are issued up front (clamped addresses, no branches around them): one L2 round trip instead of one per iteration
    u32x4_t vals[SAMP_MAXIT];
#pragma unroll
    for (int it = 0; it < SAMP_MAXIT; ++it) {
        int ch = c0 + it * 64 + lane; if (ch > nch - 1) ch = nch - 1;
        vals[it] = *reinterpret_cast<const u32x4_t*>(row + (int64_t)ch * 8);
    }
    float lsum[SAMP_MAXIT], itsum[SAMP_MAXIT];
    float wtot = 0.f;
    // Chunk-level reject for top-k: the two 16-bit keys of every dword are formed with 32-bit ops (key = b ^ (sign ? 0xffff : 0x8000)) and the
    // chunk's largest key is compared with the threshold key - one test per 8 logits instead of 8 key transforms + 8 divergent branches (one
    // CU handles the whole row, so this loop is instruction-issue bound); only the ~k chunks that hold a kept logit take the exact path.
    const bool filt = thr != 0u;
#pragma unroll
    for (int it = 0; it < SAMP_MAXIT; ++it) {
        const int ch = c0 + it * 64 + lane;
        const bool okc = it < nit && ch < c1;
        bool any = okc;
        if (filt) {
            unsigned mk = 0u;
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                const unsigned w = vals[it][d];
                const unsigned neg = (w >> 15) & 0x00010001u;                 // 1 in each half that holds a negative value
                const unsigned kw = w ^ (((neg << 15) - neg) | 0x80008000u);  // negative half: ^ 0xffff, positive half: ^ 0x8000
                mk = max(mk, max(kw >> 16, kw & 0xffffu));
            }
            any = okc & (mk >= thr);
        }
        float sacc = 0.f;
        if (any) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {        // vocabulary order inside the chunk
                const bf16_t b = (bf16_t)((e & 1) ? (vals[it][e >> 1] >> 16) : (vals[it][e >> 1] & 0xffffu));
                if (bfkey(b) >= thr) sacc += __expf((bf2f(b) - mx) * a.inv_temp);
            }
        }
        lsum[it] = sacc;
        itsum[it] = wave_sum(sacc);
        wtot += itsum[it];
    }
    if (lane == 0) wsum[wave] = wtot;
    __syncthreads();
    if (a.ws_clean && tid < SAMP_WS_WORDS) ws[tid] = 0u;        // every thread has read the histograms and the row max: leave the row's workspace zero for the next call
    if (EXT && a.ws_clean && tid == 0) ext[(int64_t)r * SAMP_EXT_WORDS + 1024] = 0u;      // (the threshold key was read before the barrier above)
    if (tid == 0) {
        float Z = 0.f;
        for (int w = 0; w < 16; ++w) Z += wsum[w];
        const int grp = a.group_rows > 0 ? r / a.group_rows : 0;
        const unsigned long long sd = a.seed + (unsigned long long)grp * a.seed_stride;
        unsigned c[4] = {(unsigned)(a.group_rows > 0 ? r % a.group_rows : r), (unsigned)step, 0u, 0u};
        philox4x32_10(c, (unsigned)(sd & 0xffffffffu), (unsigned)(sd >> 32));
        const float uu = ((float)(c[0] >> 8) + 0.5f) * (1.0f / 16777216.0f);
        if (a.u_out) a.u_out[r] = uu;
        const float target = uu * Z;
        const int nv = (nch + seg - 1) / seg;        // non-empty segments (small vocabularies leave the last waves without chunks)
        float acc = 0.f; int sg = 0;
        for (; sg < nv - 1; ++sg) { if (acc + wsum[sg] >= target) break; acc += wsum[sg]; }
        sseg = sg; sbase = acc; starget = target;
    }
    __syncthreads();
    if (wave != sseg) return;
    const float target = starget;
    float c = sbase;
    int it = 0;
    float sl = lsum[0];
#pragma unroll
    for (int j = 0; j < SAMP_MAXIT - 1; ++j) {      // wave-uniform walk over the iteration sums; `sl` follows the selected iteration
        if (it == j && j + 1 < nit && !(c + itsum[j] >= target)) { c += itsum[j]; it = j + 1; sl = lsum[j + 1]; }
    }
    float incl = sl;                                // inclusive scan over the lanes (vocabulary order inside the iteration)
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const float t = __shfl_up(incl, d, 64); if (lane >= d) incl += t; }
    const float excl = incl - sl;
    const int last_ch = min(c1, c0 + (it + 1) * 64) - 1;                 // last valid chunk of this iteration
    const unsigned long long hit = __ballot(c + incl >= target && c0 + it * 64 + lane <= last_ch);
    const int L = hit ? (__ffsll((long long)hit) - 1) : (last_ch - (c0 + it * 64));
    if (lane != L) return;
    const int ch = c0 + it * 64 + L;
    float cc = c + excl;
    int tok = -1, last_kept = -1;
    for (int i = ch * 8; i < ch * 8 + 8; ++i) {
        const bf16_t b = row[i];
        if (bfkey(b) >= thr) { last_kept = i; cc += __expf((bf2f(b) - mx) * a.inv_temp); if (cc >= target) { tok = i; break; } }
    }
    if (tok < 0) {   // rounding slack: fall back to the last kept token at or before this point
        if (last_kept >= 0) tok = last_kept;
        else { for (int i = ch * 8 + 7; i >= 0; --i) { if (bfkey(row[i]) >= thr) { tok = i; break; } } }
        if (tok < 0) { for (int i = 0; i < a.V; ++i) { if (bfkey(row[i]) >= thr) { tok = i; break; } } }
    }
    *tok_out = tok;
    if (a.next_ids) a.next_ids[r] = tok;
    samp_mark_eos(a, r, tok);
}
__global__ __launch_bounds__(1024) void samp_sum_pick_kernel(SampleArgs a) { samp_sum_pick_body<false>(a, nullptr); }
__global__ __launch_bounds__(1024) void samp_sum_pick_ext_kernel(SampleArgsF a) { samp_sum_pick_body<true>(a, a.ext); }

// ---- top-p / min-p: two more filters, folded with top-k into ONE threshold key --------------------------------------------------------------------
// Order of HF generate: temperature, top-k, top-p, min-p.  K = the set top-k keeps (ties with the k-th value included; everything when top-k is off).
//   top-p : masses softmax(x/T) over K; a value class v (all tokens of one logit value) is kept iff the mass of the tokens of K with x > v is < top_p.
//           Equal logits stand or fall together (the rule top-k uses), the row maximum always stays; on rows without ties this is TopPLogitsWarper.
//   min-p : keep x iff exp((x - max)/T) >= min_p - a ratio to the maximum, independent of the normalisation, so it intersects with the other two.
// Each filter is "key >= some 16-bit key", so the kept set is key >= max of the three keys and the inverse-CDF kernels above run unchanged.
// The masses that decide the top-p boundary are 64-bit fixed point (exp(..) * 2^40, truncated, integer atomics): the sums do not depend on the order
// of the atomics, so the same row gives the same key on every run.  Z >= 2^40 (the maximum has mass 2^40), Z < 2^58 for any V < 2^18, and the
// truncation is below V * 2^-40 of the mass.  Two levels like the count histograms: mass per high byte of the key over K, then per low byte inside
// the bin that holds the boundary.  The float expression of a mass is the one the sum passes use.
#define SAMP_MASS_SCALE 1099511627776.0f      // 2^40
typedef unsigned long long samp_u64;
TR1_DEV samp_u64 samp_mass(bf16_t b, float mx, float inv_temp) { return (samp_u64)(__expf((bf2f(b) - mx) * inv_temp) * SAMP_MASS_SCALE); }

// top-k threshold key by a 256-thread block (the search of samp_sum_pick_kernel): shist 512, scr 8, si 4 words of LDS.  Block-uniform result.
TR1_DEV unsigned samp_topk_thr_par(const SampleArgs& a, const unsigned* ws, unsigned* shist, unsigned* scr, int* si) {
    if (a.top_k <= 0 || a.top_k >= a.V) return 0u;
    shist[threadIdx.x] = ws[threadIdx.x]; shist[256 + threadIdx.x] = ws[256 + threadIdx.x];
    __syncthreads();
    samp_find_bin_par(shist, a.top_k, scr, &si[0], &si[1]);
    samp_find_bin_par(shist + 256, si[1], scr, &si[2], &si[3]);
    return samp_zero_tie(((unsigned)si[0] << 8) | (unsigned)si[2]);
}

// Boundary search over a 256-bin mass histogram by a 256-thread block, bins taken from the top: the LOWEST bin b with
// (base + mass in bins > b) < top_p * Z.  Z = Zin, or the histogram's total when Zin == 0.  The condition holds for the top bin (the caller's
// base satisfies it) and, once false, stays false, so exactly one thread writes.  The chosen bin is never empty: an empty bin has the same mass
// above it as the bin below.  The comparison is in fp64 on integers: deterministic.
TR1_DEV void samp_mass_find_par(const samp_u64* hist, samp_u64 base, samp_u64 Zin, float top_p, samp_u64* scr, int* bin_out, samp_u64* above_out,
                                samp_u64* tot_out) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const samp_u64 val = hist[255 - tid];
    samp_u64 incl = val;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const samp_u64 t = __shfl_up(incl, d, 64); if (lane >= d) incl += t; }
    if (lane == 63) scr[w] = incl;
    if (tid == 0) { *bin_out = 255; *above_out = base; }      // (only a row of NaNs leaves it at that)
    __syncthreads();
    samp_u64 off = base;
    for (int j = 0; j < w; ++j) off += scr[j];
    incl += off;
    const samp_u64 excl = incl - val, tot = base + scr[0] + scr[1] + scr[2] + scr[3];
    const double lim = (double)top_p * (double)(Zin ? Zin : tot);
    if ((double)excl < lim && (tid == 255 || !((double)incl < lim))) { *bin_out = 255 - tid; *above_out = excl; }
    if (tid == 0) *tot_out = tot;
    __syncthreads();
}

__global__ __launch_bounds__(256) void samp_mass_hi_kernel(SampleArgsF a) {
    __shared__ samp_u64 h[256];
    __shared__ unsigned shist[512], scr[8];
    __shared__ int si[4];
    const int r = blockIdx.y;
    if (samp_row_done(a, r)) return;
    const unsigned* ws = a.ws + (int64_t)r * SAMP_WS_WORDS;
    h[threadIdx.x] = 0ull;
    const unsigned thr = samp_topk_thr_par(a, ws, shist, scr, si);
    __syncthreads();
    const float mx = key_logit(ws[512]);
    const bf16_t* row = a.logits + (int64_t)r * a.ld;
    const int per = (a.V + SAMP_S - 1) / SAMP_S, i0 = blockIdx.x * per, i1 = min(a.V, i0 + per);
    for (int i = i0 + threadIdx.x; i < i1; i += 256) {
        const bf16_t b = row[i]; const unsigned k = bfkey(b);
        if (k >= thr) { const samp_u64 m = samp_mass(b, mx, a.inv_temp); if (m) atomicAdd(&h[k >> 8], m); }
    }
    __syncthreads();
    samp_u64* mh = reinterpret_cast<samp_u64*>(a.ext + (int64_t)r * SAMP_EXT_WORDS);
    if (h[threadIdx.x]) atomicAdd(&mh[threadIdx.x], h[threadIdx.x]);
}

__global__ __launch_bounds__(256) void samp_mass_lo_kernel(SampleArgsF a) {
    __shared__ samp_u64 h[256], smh[256], scr64[4], sabove, stot;
    __shared__ unsigned shist[512], scr[8];
    __shared__ int si[4], sbin;
    const int r = blockIdx.y;
    if (samp_row_done(a, r)) return;
    const unsigned* ws = a.ws + (int64_t)r * SAMP_WS_WORDS;
    samp_u64* mh = reinterpret_cast<samp_u64*>(a.ext + (int64_t)r * SAMP_EXT_WORDS);
    h[threadIdx.x] = 0ull;
    smh[threadIdx.x] = mh[threadIdx.x];
    const unsigned thr = samp_topk_thr_par(a, ws, shist, scr, si);
    __syncthreads();
    samp_mass_find_par(smh, 0ull, 0ull, a.top_p, scr64, &sbin, &sabove, &stot);
    const unsigned bin = (unsigned)sbin;
    const float mx = key_logit(ws[512]);
    const bf16_t* row = a.logits + (int64_t)r * a.ld;
    const int per = (a.V + SAMP_S - 1) / SAMP_S, i0 = blockIdx.x * per, i1 = min(a.V, i0 + per);
    for (int i = i0 + threadIdx.x; i < i1; i += 256) {
        const bf16_t b = row[i]; const unsigned k = bfkey(b);
        if ((k >> 8) == bin && k >= thr) { const samp_u64 m = samp_mass(b, mx, a.inv_temp); if (m) atomicAdd(&h[k & 255u], m); }
    }
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(&mh[256 + threadIdx.x], h[threadIdx.x]);
}

// One 256-thread block per row: the three keys and their maximum.  Leaves the mass histograms zero for the next call (the ws_zeroed contract).
__global__ __launch_bounds__(256) void samp_filter_thr_kernel(SampleArgsF a) {
    __shared__ samp_u64 smh[256], scr64[4], sabove, stot, sabove2, stot2;
    __shared__ unsigned shist[512], scr[8], smin;
    __shared__ int si[4], sbin, slo;
    const int r = blockIdx.x, tid = threadIdx.x;
    if (samp_row_done(a, r)) return;
    const unsigned* ws = a.ws + (int64_t)r * SAMP_WS_WORDS;
    unsigned* ext = a.ext + (int64_t)r * SAMP_EXT_WORDS;
    samp_u64* mh = reinterpret_cast<samp_u64*>(ext);
    const unsigned thr_k = samp_topk_thr_par(a, ws, shist, scr, si);
    const unsigned maxkey = ws[512];
    const float mx = key_logit(maxkey);
    unsigned thr_p = 0u;
    if (a.top_p < 1.f) {
        smh[tid] = mh[tid];
        __syncthreads();
        samp_mass_find_par(smh, 0ull, 0ull, a.top_p, scr64, &sbin, &sabove, &stot);
        smh[tid] = mh[256 + tid];
        __syncthreads();
        samp_mass_find_par(smh, sabove, stot, a.top_p, scr64, &slo, &sabove2, &stot2);
        thr_p = ((unsigned)sbin << 8) | (unsigned)slo;
        if (a.ws_clean) { mh[tid] = 0ull; mh[256 + tid] = 0ull; }
    }
    unsigned thr_m = 0u;
    if (a.min_p > 0.f) {
        // smallest key whose mass ratio to the maximum reaches min_p: the ratio grows with the key, so first the lowest high byte whose TOP key passes,
        // then the lowest low byte inside it.  Keys above the row maximum do not occur in the row: they count as passing.
        if (tid == 0) smin = 255u;
        __syncthreads();
        unsigned k = ((unsigned)tid << 8) | 255u;
        if (k > maxkey || __expf((key_logit(k) - mx) * a.inv_temp) >= a.min_p) atomicMin(&smin, (unsigned)tid);
        __syncthreads();
        const unsigned hb = smin;
        __syncthreads();
        if (tid == 0) smin = 255u;
        __syncthreads();
        k = (hb << 8) | (unsigned)tid;
        if (k > maxkey || __expf((key_logit(k) - mx) * a.inv_temp) >= a.min_p) atomicMin(&smin, (unsigned)tid);
        __syncthreads();
        thr_m = (hb << 8) | smin;
    }
    if (tid == 0) ext[1024] = samp_zero_tie(max(thr_k, max(thr_p, thr_m)));
}

// ---- repetition penalty (RepetitionPenaltyLogitsProcessor): a seen token's logit x becomes x * penalty if x < 0, else x / penalty -------------------
// fp32 with an IEEE division, then ONE rounding to nearest-even bf16 (the sampler's domain stays bf16; HF keeps fp32 here).  seen: one bit per token,
// [rows, seen_ld] words.  The result goes to a separate buffer: the raw logits are still read afterwards (Rollout.track_logp).  ld may be 0: one
// prefill row shown to several rows.
struct PenaltyArgs { const bf16_t* logits; int64_t ld; bf16_t* out; int64_t out_ld; const unsigned* seen; int64_t seen_ld; int V; float penalty; };
TR1_DEV bf16_t samp_penalize(bf16_t b, float penalty) { const float x = bf2f(b); return f2bf(x < 0.f ? x * penalty : __fdiv_rn(x, penalty)); }

// 8 logits per thread: one 16-byte load, one byte of the bitmap, one 16-byte store; chunks without a seen token are copied untouched
__global__ __launch_bounds__(256) void penalize_vec_kernel(PenaltyArgs a) {
    const int ch = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y;
    if (ch >= (a.V >> 3)) return;
    u32x4_t v = *reinterpret_cast<const u32x4_t*>(a.logits + (int64_t)r * a.ld + (int64_t)ch * 8);
    const unsigned bits = (a.seen[(int64_t)r * a.seen_ld + (ch >> 2)] >> ((ch & 3) * 8)) & 0xffu;
    if (bits) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            if (bits & (1u << e)) {
                const unsigned w = v[e >> 1];
                v[e >> 1] = (e & 1) ? ((w & 0xffffu) | ((unsigned)samp_penalize((bf16_t)(w >> 16), a.penalty) << 16))
                                    : ((w & 0xffff0000u) | (unsigned)samp_penalize((bf16_t)(w & 0xffffu), a.penalty));
            }
        }
    }
    *reinterpret_cast<u32x4_t*>(a.out + (int64_t)r * a.out_ld + (int64_t)ch * 8) = v;
}
__global__ __launch_bounds__(256) void penalize_scalar_kernel(PenaltyArgs a) {      // any V, any ld, any 2-byte-aligned pointer
    const int i = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y;
    if (i >= a.V) return;
    const bf16_t b = a.logits[(int64_t)r * a.ld + i];
    const bool seen = (a.seen[(int64_t)r * a.seen_ld + (i >> 5)] >> (i & 31)) & 1u;
    a.out[(int64_t)r * a.out_ld + i] = seen ? samp_penalize(b, a.penalty) : b;
}

// every id of a list (a prompt) into each of `rows` bitmap rows; ids outside [0, V) are ignored
__global__ __launch_bounds__(256) void mark_ids_kernel(const int* __restrict__ ids, int64_t n, unsigned* seen, int64_t seen_ld, int rows, int V) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int id = ids[i];
    if (id < 0 || id >= V) return;
    for (int r = 0; r < rows; ++r) atomicOr(&seen[(int64_t)r * seen_ld + (id >> 5)], 1u << (id & 31));
}
// the token each row has just drawn (toks[r * tok_ld + *step_ptr]); rows with finished[r] != 0 hold a pad token (or the EOS that ended them): skipped
__global__ __launch_bounds__(256) void mark_drawn_kernel(const int* __restrict__ toks, int64_t tok_ld, const int* step_ptr, const int* finished,
                                                         unsigned* seen, int64_t seen_ld, int rows, int V) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= rows || (finished && finished[r])) return;
    const int id = toks[(int64_t)r * tok_ld + (step_ptr ? *step_ptr : 0)];
    if (id < 0 || id >= V) return;
    atomicOr(&seen[(int64_t)r * seen_ld + (id >> 5)], 1u << (id & 31));
}

// ---- greedy decoding: token = lowest index among the row's maxima, ONE launch per decode step (no workspace, no memset) ------------------------
// One 1024-thread block per row.  The row is split into a scalar head (up to the first 16-byte boundary), a body of 8-logit chunks read with
// 16-byte loads (thread t takes chunks t, t + 1024, ..., GREEDY_UNROLL loads in flight) and a scalar tail, so any V >= 1,
// any ld >= V and any 2-byte-aligned pointer work.  The step's logits were just written by the lm_head launch: this is an L2 / MALL read.
#define GREEDY_UNROLL 4
struct GreedyArgs {
    const bf16_t* logits; int64_t ld; int V; const int* step_ptr; int* tokens; int64_t tok_ld; int* finished; int eos_id, pad_id; int* next_ids; int* done_count;
};
__global__ __launch_bounds__(1024) void greedy_tokens_kernel(GreedyArgs a) {
    __shared__ float sv[16];
    __shared__ int si[16];
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int step = a.step_ptr ? *a.step_ptr : 0;
    int* tok_out = a.tokens + (int64_t)r * a.tok_ld + step;
    if (a.finished[r]) { if (tid == 0) { *tok_out = a.pad_id; if (a.next_ids) a.next_ids[r] = a.pad_id; } return; }      // block-uniform: finished[r] is only written after the barrier below
    const bf16_t* row = a.logits + (int64_t)r * a.ld;
    const int head = min(a.V, (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(row) & 15u)) & 15u) >> 1));
    const int nch = (a.V - head) >> 3, tail0 = head + nch * 8;
    float v = -INFINITY; int idx = 0x7fffffff;
    if (tid < head) tr1_argmax_pick(v, idx, bf2f(row[tid]), tid);
    if (nch > 0) {
        const u32x4_t* body = reinterpret_cast<const u32x4_t*>(row + head);
        for (int c0 = tid; c0 < nch; c0 += 1024 * GREEDY_UNROLL) {
            u32x4_t w[GREEDY_UNROLL];
#pragma unroll
            for (int u = 0; u < GREEDY_UNROLL; ++u) w[u] = body[min(c0 + u * 1024, nch - 1)];      // clamped: a repeated chunk only offers real (value, index) pairs again
#pragma unroll
            for (int u = 0; u < GREEDY_UNROLL; ++u) {
                const int base = head + min(c0 + u * 1024, nch - 1) * 8;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float x = (e & 1) ? bfhi(w[u][e >> 1]) : bflo(w[u][e >> 1]);
                    tr1_argmax_pick(v, idx, x, base + e);
                }
            }
        }
    }
    if (tid < a.V - tail0) tr1_argmax_pick(v, idx, bf2f(row[tail0 + tid]), tail0 + tid);
    wave_argmax(v, idx);
    if (lane == 0) { sv[wave] = v; si[wave] = idx; }
    __syncthreads();
    if (wave != 0) return;
    v = lane < 16 ? sv[lane] : -INFINITY; idx = lane < 16 ? si[lane] : 0x7fffffff;
    wave_argmax(v, idx);
    if (lane != 0) return;
    const int tok = (idx >= 0 && idx < a.V) ? idx : 0;      // (a row of NaNs compares false everywhere: stay inside the vocabulary)
    *tok_out = tok;
    if (a.next_ids) a.next_ids[r] = tok;
    if (tok == a.eos_id) { a.finished[r] = 1; if (a.done_count) atomicAdd(a.done_count, 1); }
}

extern "C" int tr1_greedy_tokens_step(const void* logits, int64_t ld, int64_t rows, int64_t V, const void* step_ptr, void* tokens, int64_t tok_ld,
                                      void* finished, int64_t eos_id, int64_t pad_id, void* next_ids, void* done_count, void* stream) {
    TR1_CHECK_ARG(logits && tokens && finished, "greedy: logits, tokens and finished must not be null");
    TR1_CHECK_ARG(V >= 1 && V < (1ll << 31) - 8 && ld >= V && rows >= 0 && tok_ld >= 1, "greedy: need 1 <= V < 2^31 - 8, ld >= V, tok_ld >= 1");
    TR1_CHECK_ARG((reinterpret_cast<uintptr_t>(logits) & 1) == 0, "greedy: logits must be 2-byte aligned");
    if (rows == 0) return 0;
    GreedyArgs a;
    a.logits = (const bf16_t*)logits; a.ld = ld; a.V = (int)V; a.step_ptr = (const int*)step_ptr; a.tokens = (int*)tokens; a.tok_ld = tok_ld;
    a.finished = (int*)finished; a.eos_id = (int)eos_id; a.pad_id = (int)pad_id; a.next_ids = (int*)next_ids; a.done_count = (int*)done_count;
    hipLaunchKernelGGL(greedy_tokens_kernel, dim3((unsigned)rows), dim3(1024), 0, (hipStream_t)stream, a);
    TR1_LAUNCH_CHECK();
}

extern "C" int64_t tr1_sample_workspace_words(int64_t rows) { return rows * SAMP_WS_WORDS; }

static int sample_tokens_impl(const void* logits, int64_t ld, int64_t rows, int64_t V, float temperature, int64_t top_k, float top_p, float min_p,
                                 uint64_t seed, int64_t group_rows, uint64_t seed_stride, const void* step_ptr, void* tokens, int64_t tok_ld,
                                 void* finished, int64_t eos_id, int64_t pad_id, int stop_at_eos, void* u_out, void* ws_u32, int64_t ws_words,
                                 void* next_ids, int ws_zeroed, bool filtered, void* done_count, void* stream) {
    TR1_CHECK_ARG(temperature > 0.f, "sample: temperature must be > 0");
    TR1_CHECK_ARG(!done_count || finished, "sample: done_count counts the rows whose finished flag rises: finished must not be null");
    const int64_t row_words = filtered ? SAMP_WS_WORDS + SAMP_EXT_WORDS : SAMP_WS_WORDS;
    TR1_CHECK_ARG(ws_u32 && ws_words >= rows * row_words, "sample: workspace too small (tr1_sample_workspace_words / tr1_sample_filtered_workspace_words)");
    TR1_CHECK_ARG(!filtered || (top_p > 0.f && top_p <= 1.f && min_p >= 0.f && min_p <= 1.f), "sample: need 0 < top_p <= 1 and 0 <= min_p <= 1");
    TR1_CHECK_ARG(!filtered || (reinterpret_cast<uintptr_t>(ws_u32) & 7) == 0, "sample: the filtered workspace must be 8-byte aligned");
    TR1_CHECK_ARG(!filtered || (V >= 1 && V < (1ll << 31) - 8), "sample: need 1 <= V < 2^31 - 8");
    if (rows == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    SampleArgsF a;
    a.logits = (const bf16_t*)logits; a.ld = ld; a.V = (int)V; a.inv_temp = 1.0f / temperature; a.top_k = (int)top_k; a.seed = seed; a.group_rows = (int)group_rows; a.seed_stride = seed_stride;
    a.step_ptr = (const int*)step_ptr; a.tokens = (int*)tokens; a.tok_ld = tok_ld; a.finished = (int*)finished; a.eos_id = (int)eos_id;
    a.pad_id = (int)pad_id; a.stop_at_eos = stop_at_eos; a.u_out = (float*)u_out; a.ws = (unsigned*)ws_u32;
    a.next_ids = (int*)next_ids; a.done_count = (int*)done_count;
    // top_p = 1 and min_p = 0 keep everything: exactly the launches of the unfiltered entry points
    const bool use_p = filtered && top_p < 1.f, use_m = filtered && min_p > 0.f;
    a.ext = (use_p || use_m) ? (unsigned*)ws_u32 + rows * SAMP_WS_WORDS : nullptr;
    a.top_p = use_p ? top_p : 1.f; a.min_p = use_m ? min_p : 0.f;
    const bool fused = V % 8 == 0 && ld % 8 == 0 && V <= SAMP_FUSED_MAXV && (reinterpret_cast<uintptr_t>(logits) & 15) == 0;
    a.ws_clean = (ws_zeroed && fused) ? 1 : 0;
    const size_t ws_bytes = (size_t)rows * (a.ext ? SAMP_WS_WORDS + SAMP_EXT_WORDS : SAMP_WS_WORDS) * 4;
    if (!a.ws_clean) hipMemsetAsync(ws_u32, 0, ws_bytes, s);
    dim3 grid(SAMP_S, (unsigned)rows);
    const SampleArgs& a0 = a;      // what the kernels shared with the unfiltered path receive
    hipLaunchKernelGGL(samp_hist_hi_kernel, grid, dim3(256), 0, s, a0);     // also yields the row max (needed without top-k too)
    if (top_k > 0 && top_k < V) hipLaunchKernelGGL(samp_hist_lo_kernel, grid, dim3(256), 0, s, a0);
    if (use_p) {
        hipLaunchKernelGGL(samp_mass_hi_kernel, grid, dim3(256), 0, s, a);
        hipLaunchKernelGGL(samp_mass_lo_kernel, grid, dim3(256), 0, s, a);
    }
    if (a.ext) hipLaunchKernelGGL(samp_filter_thr_kernel, dim3((unsigned)rows), dim3(256), 0, s, a);
    if (fused) {
        if (a.ext) hipLaunchKernelGGL(samp_sum_pick_ext_kernel, dim3((unsigned)rows), dim3(1024), 0, s, a);
        else hipLaunchKernelGGL(samp_sum_pick_kernel, dim3((unsigned)rows), dim3(1024), 0, s, a0);
    } else {
        if (a.ext) {
            hipLaunchKernelGGL(samp_slice_sum_ext_kernel, grid, dim3(256), 0, s, a);
            hipLaunchKernelGGL(samp_pick_ext_kernel, dim3((unsigned)rows), dim3(256), 0, s, a);
        } else {
            hipLaunchKernelGGL(samp_slice_sum_kernel, grid, dim3(256), 0, s, a0);
            hipLaunchKernelGGL(samp_pick_kernel, dim3((unsigned)rows), dim3(256), 0, s, a0);
        }
        if (ws_zeroed) hipMemsetAsync(ws_u32, 0, ws_bytes, s);      // keep the caller's "zero between calls" contract on this path too
    }
    TR1_LAUNCH_CHECK();
}

// done_count (the last argument of the four sampling entry points; int32 [1], may be NULL = off, needs finished): the lane that writes a row's token adds 1
// with an ordinary atomicAdd when finished[row] goes 0 -> 1 - once per row, as tr1_greedy_tokens_step counts - so the early stop of a sampled rollout
// (Rollout.early_stop) polls one word.  It stands behind `stream`: a caller of the earlier declaration that passes NULL there is a caller of this one.
extern "C" int tr1_sample_tokens(const void* logits, int64_t ld, int64_t rows, int64_t V, float temperature, int64_t top_k,
                                 uint64_t seed, int64_t group_rows, uint64_t seed_stride, const void* step_ptr, void* tokens, int64_t tok_ld,
                                 void* finished, int64_t eos_id, int64_t pad_id, int stop_at_eos, void* u_out, void* ws_u32, int64_t ws_words,
                                 void* stream, void* done_count) {
    return sample_tokens_impl(logits, ld, rows, V, temperature, top_k, 1.f, 0.f, seed, group_rows, seed_stride, step_ptr, tokens, tok_ld, finished, eos_id, pad_id,
                              stop_at_eos, u_out, ws_u32, ws_words, nullptr, 0, false, done_count, stream);
}

// The decode loop's form: next_ids[row] (optional) receives the drawn token as well - the buffer the next step's embedding gather reads, so no copy
// kernel runs between two steps - and ws_zeroed != 0 promises a workspace that was zero-filled ONCE and is only ever used through this entry point:
// the pick kernel then re-zeroes what the histogram kernels dirtied instead of a memset in front of every call.
extern "C" int tr1_sample_tokens_step(const void* logits, int64_t ld, int64_t rows, int64_t V, float temperature, int64_t top_k,
                                      uint64_t seed, int64_t group_rows, uint64_t seed_stride, const void* step_ptr, void* tokens, int64_t tok_ld,
                                      void* finished, int64_t eos_id, int64_t pad_id, int stop_at_eos, void* u_out, void* ws_u32, int64_t ws_words,
                                      void* next_ids, int ws_zeroed, void* stream, void* done_count) {
    return sample_tokens_impl(logits, ld, rows, V, temperature, top_k, 1.f, 0.f, seed, group_rows, seed_stride, step_ptr, tokens, tok_ld, finished, eos_id, pad_id,
                              stop_at_eos, u_out, ws_u32, ws_words, next_ids, ws_zeroed, false, done_count, stream);
}

// ---- sampler with top-p and min-p (HF TopPLogitsWarper / MinPLogitsWarper behind temperature and top-k; vLLM SamplingParams(top_p, min_p)) -----------
// Same arguments as tr1_sample_tokens / tr1_sample_tokens_step plus the two filters, and a larger workspace (tr1_sample_filtered_workspace_words).
// top_p = 1 and min_p = 0 run exactly the launches of the unfiltered entry points and give the same tokens.
extern "C" int64_t tr1_sample_filtered_workspace_words(int64_t rows) { return rows * (SAMP_WS_WORDS + SAMP_EXT_WORDS); }

extern "C" int tr1_sample_tokens_filtered(const void* logits, int64_t ld, int64_t rows, int64_t V, float temperature, int64_t top_k, float top_p, float min_p,
                                          uint64_t seed, int64_t group_rows, uint64_t seed_stride, const void* step_ptr, void* tokens, int64_t tok_ld,
                                          void* finished, int64_t eos_id, int64_t pad_id, int stop_at_eos, void* u_out, void* ws_u32, int64_t ws_words,
                                          void* stream, void* done_count) {
    return sample_tokens_impl(logits, ld, rows, V, temperature, top_k, top_p, min_p, seed, group_rows, seed_stride, step_ptr, tokens, tok_ld, finished, eos_id,
                              pad_id, stop_at_eos, u_out, ws_u32, ws_words, nullptr, 0, true, done_count, stream);
}

extern "C" int tr1_sample_tokens_filtered_step(const void* logits, int64_t ld, int64_t rows, int64_t V, float temperature, int64_t top_k, float top_p,
                                               float min_p, uint64_t seed, int64_t group_rows, uint64_t seed_stride, const void* step_ptr, void* tokens,
                                               int64_t tok_ld, void* finished, int64_t eos_id, int64_t pad_id, int stop_at_eos, void* u_out, void* ws_u32,
                                               int64_t ws_words, void* next_ids, int ws_zeroed, void* stream, void* done_count) {
    return sample_tokens_impl(logits, ld, rows, V, temperature, top_k, top_p, min_p, seed, group_rows, seed_stride, step_ptr, tokens, tok_ld, finished, eos_id,
                              pad_id, stop_at_eos, u_out, ws_u32, ws_words, next_ids, ws_zeroed, true, done_count, stream);
}

extern "C" int tr1_penalize_logits(const void* logits, int64_t ld, void* out, int64_t out_ld, const void* seen, int64_t seen_ld, int64_t rows, int64_t V,
                                   float penalty, void* stream) {
    TR1_CHECK_ARG(logits && out && seen && logits != out, "penalize: logits, out and seen must not be null, and out must not be logits");
    TR1_CHECK_ARG(penalty > 0.f, "penalize: penalty must be > 0");
    TR1_CHECK_ARG(V >= 1 && V < (1ll << 31) - 8 && rows >= 0 && rows < 65536 && (ld == 0 || ld >= V) && out_ld >= V && seen_ld >= (V + 31) / 32,
                  "penalize: need 1 <= V < 2^31 - 8, rows < 65536, ld == 0 or ld >= V, out_ld >= V, seen_ld >= ceil(V / 32)");
    if (rows == 0) return 0;
    PenaltyArgs a;
    a.logits = (const bf16_t*)logits; a.ld = ld; a.out = (bf16_t*)out; a.out_ld = out_ld; a.seen = (const unsigned*)seen; a.seen_ld = seen_ld; a.V = (int)V;
    a.penalty = penalty;
    const bool vec = V % 8 == 0 && ld % 8 == 0 && out_ld % 8 == 0 && ((reinterpret_cast<uintptr_t>(logits) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
    if (vec) hipLaunchKernelGGL(penalize_vec_kernel, dim3((unsigned)((V / 8 + 255) / 256), (unsigned)rows), dim3(256), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(penalize_scalar_kernel, dim3((unsigned)((V + 255) / 256), (unsigned)rows), dim3(256), 0, (hipStream_t)stream, a);
    TR1_LAUNCH_CHECK();
}

extern "C" int tr1_mark_seen_ids(const void* ids, int64_t n, void* seen, int64_t seen_ld, int64_t rows, int64_t V, void* stream) {
    TR1_CHECK_ARG(seen && (ids || n == 0) && n >= 0 && n < (1ll << 31), "mark_seen_ids: null pointer or bad count");
    TR1_CHECK_ARG(V >= 1 && V < (1ll << 31) - 8 && rows >= 0 && seen_ld >= (V + 31) / 32, "mark_seen_ids: need V >= 1 and seen_ld >= ceil(V / 32)");
    if (rows == 0 || n == 0) return 0;
    hipLaunchKernelGGL(mark_ids_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const int*)ids, n, (unsigned*)seen, seen_ld,
                       (int)rows, (int)V);
    TR1_LAUNCH_CHECK();
}

extern "C" int tr1_mark_seen_drawn(const void* tokens, int64_t tok_ld, const void* step_ptr, const void* finished, void* seen, int64_t seen_ld, int64_t rows,
                                   int64_t V, void* stream) {
    TR1_CHECK_ARG(seen && tokens && tok_ld >= 1, "mark_seen_drawn: null pointer or tok_ld < 1");
    TR1_CHECK_ARG(V >= 1 && V < (1ll << 31) - 8 && rows >= 0 && rows < (1ll << 31) && seen_ld >= (V + 31) / 32, "mark_seen_drawn: need V >= 1 and seen_ld >= ceil(V / 32)");
    if (rows == 0) return 0;
    hipLaunchKernelGGL(mark_drawn_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const int*)tokens, tok_ld,
                       (const int*)step_ptr, (const int*)finished, (unsigned*)seen, seen_ld, (int)rows, (int)V);
    TR1_LAUNCH_CHECK();
}
