/*
 * timer1_hip.h - C ABI of libtimer1_hip.so: the MI355X (gfx950) kernels behind the Time-R1 GRPO rollout-and-update path.
 *
 * The reference (xiaomi-research/time-r1) has no native code of its own; its hot path reaches native kernels only through
 * third-party wheels (torch/cuBLAS/flash-attn/DeepSpeed).  Every entry point below names the reference call site whose native
 * work it replaces ("ref:" = path under the reference repo, "TF:" = transformers/models/qwen2_vl/modeling_qwen2_vl.py).
 *
 * Conventions
 *   - plain pointers and sizes only; all pointers are DEVICE pointers unless stated; bf16 = raw uint16 bfloat16 bits;
 *   - `stream` is a hipStream_t (pass 0 for the null stream); every call is asynchronous on that stream;
 *   - return value 0 = success, otherwise a hipError_t or 1000 (argument check failed); tr1_last_error() returns the message;
 *   - the library never allocates device memory: workspaces are caller-provided.
 *
 * This header is parsed by time-r1_amd/hip.py to build the ctypes signatures, so keep one declaration per statement and
 * only the types: void*, const void*, char*, int64_t*, const int64_t*, int64_t, uint64_t, int, float.
 */
#ifndef TIMER1_HIP_H
#define TIMER1_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---- plumbing ------------------------------------------------------------------------------------------------------ */
int tr1_version(void);
const char* tr1_last_error(void);
int tr1_device_info(int device, char* arch, int64_t arch_len, int64_t* n_cu, int64_t* hbm_bytes);
/* Measurement helper (bench.py `peak_probe`, SURVEY 8d roofline): reads `bytes` of device memory once with row-contiguous 1 KiB wave requests;
 * timed by the caller, it gives the practical HBM read ceiling of the box that the decode GEMMs' `roofline.frac_of_measured` is read against. */
int tr1_probe_hbm_read(const void* buf, int64_t bytes, void* sink_u32, void* stream);

/* ---- GEMM: C[M,N] = A[M,K] * B[N,K]^T (+bias[N]) (+residual[M,N]); bf16 in, fp32 accumulate on MFMA ------------------- */
/* ref: every nn.Linear on the path - TF:501-504 (q/k/v/o), TF:459-466 (MLP), TF:251-274 (patch embed), TF:277-290 (merger),
 * TF:1323 (lm_head); called from src/time_r1/rl/timer1_trainer.py:452-457 (logprob forward) and :569-573 (generate).
 * K % 64 == 0 (pad), N % 8 == 0.  out_f32: C is fp32; accumulate (fp32 only): C += result (weight-gradient accumulation).
 * M <= 16 dispatches the HBM-streaming skinny kernel used by rollout decode. */
int tr1_gemm_nt_bf16(const void* A, const void* B, void* C, const void* bias, const void* residual, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc, int64_t ldr, int out_f32, int accumulate, void* stream);
/* The same product (b_kmajor = 0: B = [N, K]; 1: B = [K, N] as stored, e.g. the weight itself in a dgrad) for THIN outputs over a long K - the continuation
 * forward's down / o projections (1600 x 3584 x 18944 / 3584), the lm_head's data gradient (1600 x 3584 over K = 152064): the K tiles are dealt to S <= 8 shares
 * that run as blocks of ONE launch into fp32 planes of ws_f32 (>= 2*M*N floats; 8*M*N lets the cost model pick any S), a second launch adds the planes in a
 * fixed order (+bias, +residual): deterministic split-K.  K % 64 == 0 and K >= 128 (at least two k tiles: S >= 2 and every share owns at least one tile,
 * S <= K / 64; a smaller K is rejected before any launch); bf16 output. */
int tr1_gemm_splitk_bf16(const void* A, const void* B, void* C, const void* bias, const void* residual, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc, int64_t ldr, int b_kmajor, void* ws_f32, int64_t ws_floats, void* stream);
int64_t tr1_gemm_splitk_max_splits(void);
/* C[M,N] = A[M,K] * B[K,N], B K-major ("NN").  The dgrad of a Linear (dX = dY * W; reference: autograd of F.linear under accelerator.backward,
 * TF trainer.py:1952-1961) reads the weight as stored instead of a transposed copy.  Needs M >= 512, N >= 256, K % 64 == 0; bf16 in / out. */
int tr1_gemm_nn_bf16(const void* A, const void* B, void* C, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc, void* stream);
/* Fused-epilogue training GEMMs ("fuse SiLU*up", "M-RoPE fused into QKV epilogue"): each is bit-identical to the GEMM followed by the elementwise
 * kernel it absorbs (the GEMM output is rounded to bf16 exactly where the unfused path stores it).
 * tr1_gemm_glu_bf16: a[M, I] = silu(x Wg^T) * (x Wu^T), Wgu = [2I, K] gate rows then up rows (TF:459-466 Qwen2MLP, reached from
 *   src/time_r1/rl/timer1_trainer.py:452-457); gu_out (NULL = not needed) receives the projection [M, 2I] the backward reads. */
int tr1_gemm_glu_bf16(const void* x, const void* Wgu, const void* bias, void* a_out, void* gu_out, int64_t M, int64_t I, int64_t K, int64_t ldx, int64_t ldw, int64_t lda, int64_t ldgu, void* stream);
/* y = quick_gelu(x W^T + bias): the Qwen2-VL vision MLP's fc1 + activation in one launch (TF:300-301 VisionMlp); bias (optional) of tr1_gemm_glu_bf16 is the
 * [2I] gate|up bias of the Qwen2.5-VL vision MLP (modeling_qwen2_5_vl.py:85-96). */
int tr1_gemm_bias_quickgelu_bf16(const void* x, const void* W, const void* bias, void* y, int64_t M, int64_t N, int64_t K, int64_t ldx, int64_t ldw, int64_t ldy, void* stream);
/* tr1_gemm_qkv_rope_bf16: fused q|k|v projection + bias + multimodal rotary embedding for head dim 128 (TF:501-504 q/k/v_proj, TF:212-222
 *   apply_multimodal_rotary_pos_emb): q_out / k_out rotated with cos / sin fp32 [M, 64], v_out plain; k_out may point into the KV cache rows. */
int tr1_gemm_qkv_rope_bf16(const void* x, const void* Wqkv, const void* bias, const void* cosb, const void* sinb, void* q_out, int64_t ldq, void* k_out, int64_t ldk, void* v_out, int64_t ldv, int64_t M, int64_t n_heads, int64_t n_kv, int64_t head_dim, int64_t K, int64_t ldx, int64_t ldw, void* stream);
/* tr1_gemm_qkv_rope_vit_bf16: the vision blocks' q|k|v projection + bias + 2-D rotary embedding (TF:225-248 apply_rotary_pos_emb_vision inside VisionAttention
 *   TF:322-360; Qwen2.5-VL modeling_qwen2_5_vl.py:160-230) for head dim 2 * half = 80, written as 128-wide zero-padded heads (d < half at column d, d + half at
 *   48 + d when half <= 48 - 64 + d otherwise; the caller zero-fills q128 / k128 / v128 once) so that the head-dim-128 attention kernel runs the tower
 *   (tr1_attn_fwd_rows_live96 when half <= 48: every head's live features end at 96).  cos / sin fp32 [M, half]. */
int tr1_gemm_qkv_rope_vit_bf16(const void* x, const void* Wqkv, const void* bias, const void* cosb, const void* sinb, void* q128, int64_t ldq, void* k128, int64_t ldk, void* v128, int64_t ldv, int64_t M, int64_t n_heads, int64_t half, int64_t K, int64_t ldx, int64_t ldw, void* stream);
/* tr1_gemm_nn_glubwd_bf16: dgu[M, 2I] = SwiGLU backward of da = dh[M, H] Wd[H, I] (the down projection as stored) with the saved gu[M, 2I]; da is never
 *   written (autograd of TF:459-466 under accelerator.backward, src/time_r1/rl/timer1_trainer.py:709-737).  dgu_t (optional): the same values once more as
 *   dgu^T [2I, ld_t] (ld_t = M rounded up to 64, columns >= M zero) - the operand of the gate/up weight gradient, written from the epilogue's LDS staging
 *   instead of by a separate transpose pass over the 384 MB of dgu. */
int tr1_gemm_nn_glubwd_bf16(const void* dh, const void* Wd, const void* gu, void* dgu, int64_t M, int64_t I, int64_t H, int64_t lda, int64_t ldb, int64_t ldgu, int64_t lddgu, void* dgu_t, int64_t ld_t, void* stream);
/* Weight gradient without the X^T copy: C[M,N] fp32 (+)= A[M,K] B[K,N], B K-major with only its first b_rows rows valid (A = dY^T zero-padded to
 * K = tokens rounded up to 64, B = the saved activation as stored).  ref: autograd of nn.Linear inside HF Trainer.training_step (TF trainer.py:1892-1961). */
int tr1_gemm_nn_acc_f32(const void* A, const void* B, void* C_f32, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc, int accumulate, int64_t b_rows, void* stream);
/* Decode-step fusion (M <= 64 rows): out = rmsnorm(x; lnw, eps) @ W[N,K]^T (+ bias), the norm folded into the GEMM's operand load
 * (ref: input_layernorm -> q/k/v_proj TF:559-580 and post_attention_layernorm -> gate/up_proj TF:600-610 inside generate).
 * glu != 0: W is [2N, K] (gate rows, then up rows) and out[M, N] = silu(gate) * up (Qwen2MLP TF:459-466) - no [M, 2N] intermediate.
 * glu == 2 (M <= 16, tr1_norm_gemm_glu_frag_ok): the same values leave FRAGMENT-MAJOR - element (m, n) at (n / 32) * 512 + m * 32 + n % 32 of `out`
 * (16 x N bf16) - the operand layout of tr1_gemm_oproj_frag, which then runs the down projection with its whole weight slice in flight (2B shapes).
 * glu is 0, 1 or 2; anything else is an argument error. */
int tr1_norm_gemm_glu_frag_ok(int64_t M, int64_t N, int64_t K);
int tr1_norm_gemm_skinny(const void* x, const void* lnw, const void* W, const void* bias, void* out, int64_t M, int64_t N, int64_t K, int64_t ldx, int64_t ldw, int64_t ldc, float eps, int glu, void* stream);
/* Losslessly packed 12-bit gate/up weights (csrc/gemm_pk.hip; same call site as tr1_norm_gemm_skinny(glu = 1 / 2): post_attention_layernorm -> gate/up_proj TF:600-610,
 * Qwen2MLP TF:459-466 inside generate): a 4-bit sign + exponent code against a per-stage base, the low byte verbatim, an exact patch list for the rest.
 * The IMAGE of W[2I, K] (gate rows, then up rows) is one buffer of tr1_glu_pk_image_bytes(I, K) bytes: S = (I / 16) * 8 * (K / 512) stages as S records of 3072 bytes,
 * S tails of 64 bytes, then 16 bytes whose first int is the flag.
 * tr1_glu_pk_ok: 1 where the shape is covered - 1 <= M <= 16 rows, I >= 16, I % 16 == 0, K = 512 * {7, 4, 3}.
 * tr1_pack_bf16_glu: W[2I, K] (ldw) -> image; flag = 1 when some stage needs more than 14 patches: the matrix is then NOT representable and the caller keeps
 *   tr1_norm_gemm_skinny(glu = 1 / 2).
 * tr1_norm_glu_pk: out[M, I] = silu(gate) * up of rmsnorm(x; lnw, eps) against an image with flag 0 - the bits tr1_norm_gemm_skinny(glu = 1) stores, 0.77x the bytes
 *   streamed; frag != 0 (I % 32 == 0): the fragment-major output of glu = 2. */
int tr1_glu_pk_ok(int64_t M, int64_t I, int64_t K);
int64_t tr1_glu_pk_image_bytes(int64_t I, int64_t K);
int tr1_pack_bf16_glu(const void* W, int64_t I, int64_t K, int64_t ldw, void* image, void* stream);
int tr1_norm_glu_pk(const void* x, const void* lnw, const void* image, void* out, int64_t M, int64_t I, int64_t K, int64_t ldx, int64_t ldc, float eps, int frag, void* stream);
/* Decode rows: input_layernorm -> fused q/k/v projection -> M-RoPE -> KV-cache append in ONE launch (tr1_norm_gemm_skinny + tr1_decode_qkv_post):
 * roped q -> q_out[M, n_heads*hd]; roped k -> kcache[slots[m], :]; v -> vtcache[:, slots[m]].  Wqkv: [(n_heads + 2 n_kv)*hd, K] (q | k | v rows).
 * ref: Qwen2VLAttention.forward TF:521-556 + DynamicCache.update inside generate (timer1_trainer.py:568-573).  head_dim % 32 == 0. */
int tr1_norm_gemm_qkv(const void* x, const void* lnw, const void* Wqkv, const void* bias, const void* cosb, const void* sinb, void* q_out, int64_t ld_q, void* kcache, int64_t k_ld, void* vtcache, int64_t vt_ld, const void* slots, int64_t M, int64_t n_heads, int64_t n_kv, int64_t head_dim, int64_t K, int64_t ldx, int64_t ldw, float eps, void* stream);
/* Narrow decode projections (o_proj / down_proj at M <= 64 rows): C = A B^T (+bias)(+residual) with cross-block split-K and an in-kernel
 * fixup (the last block of a column group sums the fp32 partial tiles).  ws_f32: tr1_gemm_skinny_fixup_workspace_floats() floats whose
 * trailing ticket counters must be ZERO before the first call (the kernel re-arms them).  Same call sites as tr1_gemm_nt_bf16 in generate. */
int tr1_gemm_skinny_fixup(const void* A, const void* B, void* C, const void* bias, const void* residual, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc, int64_t ldr, void* ws_f32, int64_t ws_floats, void* stream);
int64_t tr1_gemm_skinny_fixup_workspace_floats(int64_t M, int64_t N, int64_t K);
/* out[c, r] = in[r, c]; columns [R, ld_out) of out are zero-filled (feeds the NT GEMM for dgrad / wgrad). */
int tr1_transpose_bf16(const void* in, int64_t ld_in, void* out, int64_t ld_out, int64_t R, int64_t C, void* stream);
/* The same transpose with colsum_f32[c] += sum_r in[r, c]: the bias gradient of a Linear (reference: autograd of F.linear, q/k/v_proj bias TF:501-504) taken
 * from the pass that builds dY^T for its weight gradient. */
int tr1_transpose_colsum_bf16(const void* in, int64_t ld_in, void* out, int64_t ld_out, int64_t R, int64_t C, void* colsum_f32, void* ws_f32, int64_t ws_floats, void* stream);

/* ---- normalisation ------------------------------------------------------------------------------------------------- */
/* ref: Qwen2RMSNorm TF:96-110 (fp32 math, cast to bf16 BEFORE the weight multiply).  If residual != NULL the kernel first forms
 * xsum = bf16(x + residual) (the decoder's residual add, TF:559-624), writes it, and normalises xsum.  rstd (fp32[rows]) optional. */
int tr1_rmsnorm_fwd(const void* x, const void* residual, const void* w, void* y, void* xsum, void* rstd, int64_t rows, int64_t cols, float eps, void* stream);
/* dx = rmsnorm'(dy) (+ dres if given);  dw_f32[c] += sum_r dy*xhat   (autograd of the above; ref: accelerator.backward, TF trainer.py:1952-1961).
 * dw_f32 may be NULL (no weight gradient); otherwise ws_f32 holds tr1_rmsnorm_bwd_workspace_floats() floats of per-block partial rows that a
 * second kernel adds in a fixed order (no atomics: the gradient is reproducible). */
int tr1_rmsnorm_bwd(const void* dy, const void* x, const void* w, const void* rstd, const void* dres, void* dx, void* dw_f32, void* ws_f32, int64_t ws_floats, int64_t rows, int64_t cols, void* stream);
int64_t tr1_rmsnorm_bwd_workspace_floats(int64_t rows, int64_t cols);
/* ref: nn.LayerNorm(eps=1e-6) in VisionBlock TF:425-449 and PatchMerger.ln_q TF:277-290 */
int tr1_layernorm_fwd(const void* x, const void* w, const void* b, void* y, void* mean, void* rstd, int64_t rows, int64_t cols, float eps, void* stream);
int tr1_layernorm_bwd(const void* dy, const void* x, const void* w, const void* mean, const void* rstd, void* dx, void* dw_f32, void* db_f32, void* ws_f32, int64_t ws_floats, int64_t rows, int64_t cols, void* stream);

/* ---- activations / elementwise ---------------------------------------------------------------------------------------- */
/* ref: Qwen2MLP TF:459-466: out = silu(gate) * up with gu = [gate | up] along the feature axis */
int tr1_swiglu_fwd(const void* gu, void* out, int64_t rows, int64_t inter, void* stream);
int tr1_swiglu_bwd(const void* dout, const void* gu, void* dgu, int64_t rows, int64_t inter, void* stream);
/* ref: PatchMerger GELU(erf) TF:277-290; VisionMlp quick_gelu TF:293-301 */
int tr1_gelu_fwd(const void* x, void* y, int64_t n, void* stream);
int tr1_gelu_bwd(const void* x, const void* dy, void* dx, int64_t n, void* stream);
int tr1_quickgelu_fwd(const void* x, void* y, int64_t n, void* stream);
/* ref: VisionMlp quick_gelu TF:293-301 backward (fix_vit=False trains the blocks, timer1_trainer.py:267-288): dx = dy (s + 1.702 x s (1 - s)),
 * s = sigmoid(1.702 x), fp32 math on bf16 inputs, rounded once */
int tr1_quickgelu_bwd(const void* x, const void* dy, void* dx, int64_t n, void* stream);
int tr1_add_bf16(const void* a, const void* b, void* y, int64_t n, void* stream);
int tr1_cast_f32_to_bf16(const void* x, void* y, int64_t n, void* stream);
int tr1_cast_bf16_to_f32(const void* x, void* y, int64_t n, void* stream);
int tr1_colsum_accum(const void* dy, void* dbias_f32, int64_t rows, int64_t cols, void* ws_f32, int64_t ws_floats, void* stream);
int64_t tr1_colsum_workspace_floats(int64_t rows, int64_t cols);

/* ---- rotary embeddings ------------------------------------------------------------------------------------------------ */
/* ref: Qwen2VLRotaryEmbedding TF:117-169 + apply_multimodal_rotary_pos_emb TF:180-222.  pos3: int32 [3, T] (t,h,w) from
 * get_rope_index TF:914-1016; cos/sin: fp32 [T, head_dim/2]; sections (sec_t, sec_h, sec_w) = mrope_section. */
int tr1_mrope_table(const void* pos3, void* cosb, void* sinb, int64_t T, int64_t head_dim, int64_t sec_t, int64_t sec_h, int64_t sec_w, float theta, int round_bf16, void* stream);
/* ref: VisionRotaryEmbedding + apply_rotary_pos_emb_vision TF:225-248; hw: int32 [N, 2] patch (h, w) ids in merge-block order */
int tr1_vision_rope_table(const void* hw, void* cosb, void* sinb, int64_t N, int64_t head_dim, float theta, void* stream);
/* rotate-half RoPE on n_heads heads stored inside rows of `in` (row stride ld_in); backward != 0 applies the adjoint rotation */
int tr1_rope_apply(const void* in, int64_t ld_in, void* out, int64_t ld_out, const void* cosb, const void* sinb, int64_t T, int64_t n_heads, int64_t head_dim, int backward, void* stream);
/* ref: VisionAttention TF:379-396 (q / k / v split of the fused qkv, apply_rotary_pos_emb_vision TF:225-248), backward of the tower's 128-wide padded
 * heads (fix_vit=False, timer1_trainer.py:267-288): [T, n_heads*128] with feature d < half at h*128 + d and its partner at h*128 + hoff + d ->
 * [T, n_heads*2*half] (row stride ld_out, may be a column view); rotate != 0 applies the adjoint rotation (cos / sin fp32 [T, half]).
 * Bit-identical to compacting + tr1_rope_apply(backward=1). */
int tr1_vit_heads_unpad(const void* in, int64_t ld_in, void* out, int64_t ld_out, const void* cosb, const void* sinb, int64_t T, int64_t n_heads, int64_t half, int64_t hoff, int rotate, void* stream);

/* ---- embedding / scatter ---------------------------------------------------------------------------------------------- */
/* ref: embed_tokens TF:1160 and the masked_scatter of video embeddings TF:1170-1176 */
int tr1_gather_rows(const void* table, const void* ids, void* out, int64_t T, int64_t cols, void* stream);
int tr1_scatter_rows(const void* src, const void* idx, void* dst, int64_t T, int64_t cols, void* stream);
int tr1_embed_bwd(const void* dout, const void* ids, void* dtable_f32, int64_t T, int64_t cols, void* stream);

/* ---- attention -------------------------------------------------------------------------------------------------------- */
/* Two-interval masked flash attention: key kv is visible to query token t iff kv < pre[t] or lo[t] <= kv <= hi[t].
 * ref: flash_attn_varlen_func / SDPA via TF:379-396 (ViT, cu_seqlens segments) and TF:521-556 (LLM causal GQA); the shared-prefix
 * form replaces the G-times replicated prompt of timer1_trainer.py:594-599.  Q/O: [T, n_heads*head_dim]; K: [slots, n_kv*head_dim];
 * VT: [n_kv*head_dim, vt_ld] (slot-contiguous).  lse (optional): fp32 [n_heads, T].  nsplit > 1 = split-KV (decode) with a
 * caller workspace of n_batch * tr1_attn_fwd_workspace_floats() floats.  n_batch > 1 runs n_batch independent problems in one launch:
 * problem b uses Q/O/mask rows [b*T, (b+1)*T) and cache slots starting at b*kv_batch_slots (decode over several prompts' caches). */
int tr1_attn_fwd(const void* Q, int64_t q_ld, const void* K, int64_t k_ld, const void* VT, int64_t vt_ld, void* O, int64_t o_ld, void* lse, const void* pre, const void* lo, const void* hi, int64_t T, int64_t n_heads, int64_t n_kv, int64_t n_slots, int64_t head_dim, float scale, int64_t nsplit, void* ws_f32, int64_t ws_floats, int64_t n_batch, int64_t kv_batch_slots, void* stream);
int64_t tr1_attn_fwd_workspace_floats(int64_t T, int64_t n_heads, int64_t n_kv, int64_t head_dim, int64_t nsplit);
/* The same attention (nsplit = 1, one problem, head_dim = 128) with K AND V row-major ([n_slots, n_kv*128], any leading dims % 8 == 0): the
 * 32x32x16-MFMA kernel of round 3 transposes V in its LDS reads, so the LLM's training / prefill / reference-policy forwards (TF:521-556 via
 * timer1_trainer.py:452-457, attn_implementation=flash_attention_2 in scripts/posttrain/train_rl.sh:33) need no V^T copy.  Same results as
 * tr1_attn_fwd up to the order of the fp32 accumulation.  From 3 072 key slots on the launch takes the 64-rows-per-wave kernel of round 6
 * (csrc/attn_fwd64.hip: one wave per SIMD, the softmax of tile t in the MFMA gaps of tiles t-1 / t+1) - bit-identical O and LSE; the
 * environment variable TR1_FWD64 = 1 / 0, read per call, forces / forbids it. */
int tr1_attn_fwd_rows(const void* Q, int64_t q_ld, const void* K, int64_t k_ld, const void* V, int64_t v_ld, void* O, int64_t o_ld, void* lse, const void* pre, const void* lo, const void* hi, int64_t T, int64_t n_heads, int64_t n_kv, int64_t n_slots, int64_t head_dim, float scale, void* stream);
/* tr1_attn_fwd_rows for 128-wide heads whose features 96..127 are ZERO in Q, K and V (the vision towers' head dim 80 in the padded layout of
 * tr1_gemm_qkv_rope_vit_bf16): 12 + 12 instead of 16 + 16 MFMAs per wave and key tile; O columns 96..127 of every head are not written (the caller keeps them
 * zero).  ref: VisionAttention.forward TF:379-396 / Qwen2.5-VL's windowed form, frozen towers (src/time_r1/rl/timer1_trainer.py:264-269). */
int tr1_attn_fwd_rows_live96(const void* Q, int64_t q_ld, const void* K, int64_t k_ld, const void* V, int64_t v_ld, void* O, int64_t o_ld, void* lse, const void* pre, const void* lo, const void* hi, int64_t T, int64_t n_heads, int64_t n_kv, int64_t n_slots, int64_t head_dim, float scale, void* stream);
/* Split-KV decode over the layers of ONE decode step (same pre/lo/hi in every layer of model.generate's step, timer1_trainer.py:568-573): the
 * launch with plan_mode 1 publishes each query tile's relevant-tile list in `plan` (int32[tr1_attn_plan_ints()]), launches with plan_mode 2 start
 * from it instead of reducing the masks again; plan_mode 0 (plan may be NULL) is tr1_attn_fwd.  Results are bit-identical in all three modes. */
int tr1_attn_fwd_planned(const void* Q, int64_t q_ld, const void* K, int64_t k_ld, const void* VT, int64_t vt_ld, void* O, int64_t o_ld, void* lse, const void* pre, const void* lo, const void* hi, int64_t T, int64_t n_heads, int64_t n_kv, int64_t n_slots, int64_t head_dim, float scale, int64_t nsplit, void* ws_f32, int64_t ws_floats, int64_t n_batch, int64_t kv_batch_slots, void* plan, int plan_mode, void* stream);
/* tr1_attn_fwd_planned whose merged rows leave FRAGMENT-MAJOR for tr1_gemm_oproj_frag: Ofrag holds ceil(n_batch * T / 16) * 16 x n_heads * 128 bf16, element (row m,
 * feature k) at ((m / 16) * (n_heads * 4) + k / 32) * 512 + (m % 16) * 32 + k % 32 (the 16 rows x 64 bytes of an MFMA operand fragment are one contiguous KiB).
 * Split-KV launches (nsplit > 1) at head dim 128.  ref: attention half of Qwen2VLAttention.forward inside model.generate (TF:521-552). */
int tr1_attn_fwd_planned_frag(const void* Q, int64_t q_ld, const void* K, int64_t k_ld, const void* VT, int64_t vt_ld, void* Ofrag, const void* pre, const void* lo, const void* hi, int64_t T, int64_t n_heads, int64_t n_kv, int64_t n_slots, int64_t head_dim, float scale, int64_t nsplit, void* ws_f32, int64_t ws_floats, int64_t n_batch, int64_t kv_batch_slots, void* plan, int plan_mode, void* stream);
/* Decode rows (M <= 32): C[M, N] = X @ W[N, K]^T (+ residual) with X fragment-major (layout above, K = n_heads * 128 <= 3584): every block keeps its whole
 * weight slice in flight (HBM -> LDS DMA) and owns its columns over the whole K - no split-K fixup (csrc/oproj.hip).  tr1_gemm_oproj_frag_ok: shape covered?
 * Round 6: also K <= 9216 at M <= 16 when a block's columns (N / 256 rounded up to a divisor of N, <= 8) fit 152 KB of LDS over the whole K - the
 * Qwen2-VL-2B down projection (1536 x 8960: 6 columns x 256 blocks), fed by tr1_norm_gemm_skinny(glu = 2).
 * ref: o_proj of Qwen2VLAttention.forward (TF:553-556) and down_proj of Qwen2MLP.forward (TF:459-466) inside model.generate
 * (src/time_r1/rl/timer1_trainer.py:568-578). */
int tr1_gemm_oproj_frag(const void* Xfrag, const void* W, const void* residual, void* C, int64_t M, int64_t N, int64_t K, int64_t ldw, int64_t ldr, int64_t ldc, void* stream);
int tr1_gemm_oproj_frag_ok(int64_t M, int64_t N, int64_t K);
int64_t tr1_attn_plan_ints(int64_t T, int64_t n_heads, int64_t n_kv, int64_t n_batch);
/* Backward of the above (recompute based): needs K, V row-major.  KT / kt_ld are kept for ABI stability and ignored (may be NULL / 0): the dQ
 * kernel reads its K^T fragments from the K rows with ds_read_b64_tr_b16.  QT / dOT (tr1_pack_transpose copies) only for head dims padded to
 * 32 or 96 (may be NULL for 64 / 128: the 8-wave dK/dV kernel transposes in its LDS reads the same way).
 * delta: fp32 [2*n_heads, T] scratch (delta, then the log2-scaled LSE); qmeta_ws: int32 [8*ceil(T*group/64)] scratch; ws_f32: tr1_attn_bwd_workspace_floats() floats (fp32 dK/dV
 * partials of the query-split dK/dV kernel).  Writes dQ [T, n_heads*hd], dK, dV [slots, n_kv*hd]. */
int tr1_attn_bwd(const void* Q, int64_t q_ld, const void* K, int64_t k_ld, const void* V, int64_t v_ld, const void* KT, int64_t kt_ld, const void* QT, int64_t qt_ld, const void* dOT, int64_t dot_ld, const void* O, int64_t o_ld, const void* dO, int64_t do_ld, const void* lse, void* delta, void* dQ, int64_t dq_ld, void* dK, int64_t dk_ld, void* dV, int64_t dv_ld, const void* pre, const void* lo, const void* hi, void* qmeta_ws, void* ws_f32, int64_t ws_floats, int64_t T, int64_t n_heads, int64_t n_kv, int64_t n_slots, int64_t head_dim, float scale, void* stream);
/* The same backward with the M-RoPE backward (TF:212-222 transposed) folded in: dQ / dK come back with respect to the UN-rotated projections, rotated in
 * the dQ kernel's epilogue and in the dK / dV partial-sum kernel (head dim 128; other shapes run tr1_rope_apply in place).  cos / sin fp32 [T, d/2], n_slots == T. */
int tr1_attn_bwd_rope(const void* Q, int64_t q_ld, const void* K, int64_t k_ld, const void* V, int64_t v_ld, const void* KT, int64_t kt_ld, const void* QT, int64_t qt_ld, const void* dOT, int64_t dot_ld, const void* O, int64_t o_ld, const void* dO, int64_t do_ld, const void* lse, void* delta, void* dQ, int64_t dq_ld, void* dK, int64_t dk_ld, void* dV, int64_t dv_ld, const void* pre, const void* lo, const void* hi, void* qmeta_ws, void* ws_f32, int64_t ws_floats, int64_t T, int64_t n_heads, int64_t n_kv, int64_t n_slots, int64_t head_dim, float scale, const void* rope_cos, const void* rope_sin, void* stream);
int64_t tr1_attn_bwd_workspace_floats(int64_t T, int64_t n_heads, int64_t n_kv, int64_t n_slots, int64_t head_dim);
/* out[(kvh*hd + d) * ld_out + col] = in[t*ld_in + (kvh*group + hq)*hd + d], col = t*group + hq (or slots[t] when slots != NULL, group 1);
 * without slots, columns [T*group, zero_cols) are zero-filled */
int tr1_pack_transpose(const void* in, int64_t ld_in, void* out, int64_t ld_out, const void* slots, int64_t T, int64_t n_heads, int64_t n_kv, int64_t head_dim, int64_t zero_cols, void* stream);
/* Decode-step post-projection in one launch: M-RoPE on q and k of the new tokens, k -> kcache[slots[r]], v -> vtcache[:, slots[r]]
 * (ref: Qwen2VLAttention.forward TF:521-556 with a DynamicCache update inside generate, timer1_trainer.py:568-573) */
int tr1_decode_qkv_post(const void* qkv, int64_t ld, const void* cosb, const void* sinb, void* q_out, int64_t ld_q, void* kcache, int64_t k_ld, void* vtcache, int64_t vt_ld, const void* slots, int64_t R, int64_t n_heads, int64_t n_kv, int64_t head_dim, void* stream);
/* KV-cache append: dst[slots[t], :] = src[t, :] */
int tr1_scatter_slots(const void* src, int64_t ld_src, void* dst, int64_t ld_dst, const void* slots, int64_t T, int64_t cols, void* stream);

/* ---- fp8 weight storage for the rollout (BASELINE config "fp8 weights") --------------------------------------------------------------- */
/* Per-row symmetric quantisation to OCP fp8 e4m3: scale[n] = amax_n / 448 (1 for a zero row), q = rne(w * 448 / amax_n).  Run once per
 * optimizer step on the decoder matrices; only the SAMPLING policy of generate (timer1_trainer.py:568-573) reads the fp8 copy. */
int tr1_quantize_fp8_rows(const void* w_bf16, int64_t ldw, void* q_fp8, int64_t ldq, void* scale_f32, int64_t N, int64_t K, void* stream);
/* Decode rows (M <= 64) against fp8 weights, dequantised to bf16 in registers (W8A16): out = act(x) W^T * scale (+bias)(+residual).
 * lnw != NULL folds rmsnorm(x; lnw, eps) into the operand load; glu != 0: W_fp8 is [2N, K] (gate rows then up rows), out = silu(gate)*up.
 * Same call sites as tr1_gemm_nt_bf16 / tr1_norm_gemm_skinny inside generate.  K % 128 == 0. */
int tr1_gemm_skinny_w8(const void* x, const void* lnw, const void* W_fp8, const void* wscale, const void* bias, const void* residual, void* out, int64_t M, int64_t N, int64_t K, int64_t ldx, int64_t ldw, int64_t ldc, int64_t ldr, float eps, int glu, void* stream);
/* W8A8, the "CDNA4 fp8 MFMA" form (BASELINE.json configs[4]): same arguments and call sites, but the fp8 weight codes feed
 * v_mfma_scale_f32_16x16x128_f8f6f4 directly and the activations (after the optional rmsnorm weight) are quantised in the operand load to
 * e4m3 with one power-of-two (E8M0) scale per row and per 32 consecutive k (OCP microscaling); weight row scale in the epilogue. */
int tr1_gemm_skinny_w8a8(const void* x, const void* lnw, const void* W_fp8, const void* wscale, const void* bias, const void* residual, void* out, int64_t M, int64_t N, int64_t K, int64_t ldx, int64_t ldw, int64_t ldc, int64_t ldr, float eps, int glu, void* stream);
/* W8A8 split-K + in-kernel fixup form (decode down projection, M <= 16, K % 512 == 0, N % 64 == 0); workspace as tr1_gemm_skinny_fixup. */
int tr1_gemm_skinny_fixup_w8a8(const void* x, const void* W_fp8, const void* wscale, void* out, const void* bias, const void* residual, int64_t M, int64_t N, int64_t K, int64_t ldx, int64_t ldw, int64_t ldc, int64_t ldr, void* ws_f32, int64_t ws_floats, void* stream);

/* ---- native decode-step driver ------------------------------------------------------------------------------------------------ */
/* One call enqueues a whole rollout decode step for R <= 64 rows: embed gather -> n_layers x {norm+qkv, rope + KV append, split-KV attention,
 * o_proj + residual, norm + gate/up + SwiGLU, down_proj + residual} -> final norm + lm_head -> logits[R, vocab] (bf16).
 * ref: per-token body of model.generate (timer1_trainer.py:568-573; Qwen2VLDecoderLayer TF:559-624, norm TF:839, lm_head TF:1323).
 * layer_ptrs: HOST array of 14 * n_layers DEVICE pointers, per layer {ln1, qkv.w, qkv.b, o.w, ln2, gu.w, down.w, K cache [B*s_cap, kv_dim], V^T cache [kv_dim, B*s_cap],
 * qkv.scale, o.scale, gu.scale, down.scale, gu.pk}; a slot the step does not use is NULL.  dims: HOST int64[13] {n_layers, hidden, n_heads, n_kv, head_dim,
 * intermediate, vocab, rows, n_batch, s_cap, nsplit, fp8_mask, mode}.
 * mode 0: bf16 weights; the scale slots, lm_head_scale and fp8_mask are unused (fp8_mask must be 0).  gu.pk: the packed 12-bit image of gu.w (tr1_pack_bf16_glu, flag 0) -
 *   the layer's gate/up launch is then tr1_norm_glu_pk, the same logits bit for bit - or NULL for a layer that keeps the bf16 gate/up launch.
 * mode 1 (W8A16, tr1_gemm_skinny_w8) / 2 (W8A8, every fp8 projection through tr1_gemm_skinny_w8a8, the fp8 MFMA): fp8 weights of tr1_quantize_fp8_rows with their
 *   fp32 row scales in the scale slots, lm_head / lm_head_scale likewise; embedding, norms, biases, KV cache stay bf16; gu.pk must be NULL.
 *   fp8_mask (bits 0..4 only): bit 0 qkv, 1 o, 2 gate/up, 3 down, 4 lm_head (31 = all).  A CLEAR bit keeps that matrix of the sampling policy in bf16: its weight slot
 *   (or `lm_head`) then holds the bf16 weight and the bf16 decode kernel runs - the mixed-precision policies of the config-5 drift study.  lm_head_scale may be NULL
 *   unless bit 4 is set.
 * ids int32[R]; cosb/sinb fp32 [R, head_dim/2]; slots int32[R] (absolute cache slot of each row's new token);
 * pre/lo/hi int32[R] (two-interval mask, cache-local per batch entry); work: device scratch of tr1_decode_step_workspace_bytes(dims),
 * ZERO-FILLED once by the caller before the first step (it holds self re-arming split-K ticket counters); the size depends on dims[0..10] alone. */
int tr1_decode_step(const void* layer_ptrs, const int64_t* dims, const void* embed, const void* final_norm, const void* lm_head, const void* lm_head_scale, const void* ids, const void* cosb, const void* sinb, const void* slots, const void* pre, const void* lo, const void* hi, void* work, int64_t work_bytes, void* logits, float eps, float scale, void* stream);
int64_t tr1_decode_step_workspace_bytes(const int64_t* dims);
/* Measurement helpers (bench.py `roofline`): between begin and end every tr1_decode_step call records a pair of HIP events on its
 * stream around each projection GEMM it launches (families 0 qkv, 1 o, 2 gate/up, 3 down, 4 lm_head).  end() synchronises those events and
 * writes, per family, the summed and the minimum launch duration in ms and the number of launches (host arrays of 5).  Not thread-safe. */
int tr1_decode_profile_begin(void);
int tr1_decode_profile_end(double* ms_by_family, double* min_ms_by_family, int64_t* launches_by_family);

/* ---- video preprocessing (SURVEY 8f "next" row 1) ------------------------------------------------------------------------ */
/* ref: torchvision resize(BICUBIC, antialias) at src/utils/vision_process.py:467-472 + Qwen2VLVideoProcessor rescale/normalize/patchify
 * (transformers video_processing_qwen2_vl.py:236-274).  frames: uint8 [T_in,3,H,W] on the device; out: bf16 [N_v, ld_out] patch rows (caller
 * zero-fills the K padding); ymin/wy, xmin/wx: per-output first tap + normalised weights [Ho,taps_y], [Wo,taps_x] (vision_process.aa_filter). */
int tr1_video_preprocess(const void* frames_u8, void* out_bf16, int64_t ld_out, const void* ymin, const void* wy, int64_t taps_y, const void* xmin, const void* wx, int64_t taps_x, int64_t T_in, int64_t T_out, int64_t H, int64_t W, int64_t Ho, int64_t Wo, float mean0, float mean1, float mean2, float std0, float std1, float std2, int64_t patch, int64_t temporal_patch, int64_t merge, void* stream);

/* ---- vocabulary side -------------------------------------------------------------------------------------------------- */
/* ref: src/time_r1/rl/timer1_trainer.py:458-481 (_get_per_token_logps: log_softmax, gather, entropy) */
int tr1_logp_entropy_fwd(const void* logits, int64_t ld, const void* targets, void* logp, void* entropy, void* lse, int64_t R, int64_t V, void* stream);
/* lm_head fused with the log-softmax statistics: hn [M,K] x W [N,K]^T is reduced in the GEMM epilogue to per-64-column (max, sum e, sum x e) and merged
 * per row - the [M, N] logits of _get_per_token_logps (timer1_trainer.py:449-481) never reach HBM.  part_ws: tr1_lmhead_lse_workspace_floats(M, N) floats. */
int tr1_lmhead_lse_fwd(const void* hn, const void* W, const void* targets, void* part_ws, int64_t ws_floats, void* logp, void* ent, void* lse, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, void* stream);
int64_t tr1_lmhead_lse_workspace_floats(int64_t M, int64_t N);
int tr1_logp_bwd(const void* logits, int64_t ld, const void* targets, const void* lse, const void* dlogp, void* dlogits, int64_t ld_out, int64_t R, int64_t V, void* stream);
/* tr1_logp_bwd with a gradient at the entropy too: dlogits[r, v] = dlogp[r] (1[v == t_r] - p) - dent[r] p ((x - lse[r]) + ent[r]), p = exp(x - lse[r])
 * (d H / d x_v = -p_v (log p_v + H)).  ref: src/time_r1/rl/timer1_trainer.py:473-481 computes this entropy under no_grad, a logged number; here it can carry a
 * loss term - the entropy bonus of verl's actor.entropy_coeff (GRPOConfig.entropy_coef) - and it feeds the token selection of trl.GRPOConfig.top_entropy_quantile
 * below.  lse, ent: the forward's outputs as they are (fp32 [R]); dlogp, dent fp32 [R]; dlogits bf16 with its own ld_out, may alias logits; ld, ld_out, V multiples
 * of 8.  dent NULL: tr1_logp_bwd itself, bit for bit; rows with dent[r] == 0 give its values, rows with dlogp[r] == dent[r] == 0 are exactly 0. */
int tr1_logp_entropy_bwd(const void* logits, int64_t ld, const void* targets, const void* lse, const void* ent, const void* dlogp, const void* dent /*may be null*/, void* dlogits, int64_t ld_out, int64_t R, int64_t V, void* stream);
/* trl.GRPOConfig.top_entropy_quantile (trl GRPOTrainer.get_high_entropy_mask) for one micro-step, without a host synchronisation: over the live positions
 * (mask != 0, int32) of ent (fp32 [N], the entropy of timer1_trainer.py:473-481 on the [G, C] grid) thr = the quantile of order 1 - rho, linearly interpolated between
 * the order statistics as torch.quantile does; weight[i] (fp32) = 1 where the position is live and ent[i] >= thr (ties kept), else 0 - the tok_weight of the loss
 * kernels below; stats3 = {thr, number kept, n live}.  n = 0: zeros.  0 < rho <= 1; N <= TR1_ENTROPY_QUANTILE_MAX_N (one block).  Masked positions are never read.
 * No workspace, no floating-point atomics: bit-identical from call to call. */
#define TR1_ENTROPY_QUANTILE_MAX_N 1048576
int tr1_entropy_quantile_weight(const void* ent, const void* mask, void* weight, void* stats3, int64_t N, float rho, void* stream);
/* ref: timer1_trainer.py:635-639 (k3 KL), :713-737 (both loss branches).  out3 = {loss, mean masked kl, sum mask}. */
int tr1_grpo_loss(const void* logp, const void* ref_logp, const void* mask, const void* adv, void* dlogp, void* out3, void* row_len, void* row_kl, int64_t G, int64_t C, float beta, int use_grpo, float grad_scale, void* stream);
/* ref: timer1_trainer.py:730-737 (the PPO-clip branch written out: coef_1 = exp(logp - old_logp), coef_2 = clamp(coef_1, 1 - eps_low, 1 + eps_high)) for
 * the 2nd .. num_iterations-th update on one rollout, where old_logp is the policy that was current when the completions were drawn; :635-639 (k3 KL).
 * tok_weight (may be null = 1): constant per-token weight on the advantage term.  out8 = {loss, mean masked kl, sum mask, low / high / either clip
 * fraction, masked mean of rho - 1 - log rho, max rho}.  One block per row, row partials in ws (TR1_GRPO_LOSS_RATIO_WS_WORDS 4-byte words, zero before the
 * first call; every call leaves it zero), folded in a fixed order: no floating-point atomics, bit-identical from call to call.  Masked positions are never read. */
#define TR1_GRPO_LOSS_RATIO_WS_WORDS 528
int tr1_grpo_loss_ratio(const void* logp, const void* old_logp, const void* ref_logp /*may be null*/, const void* tok_weight /*may be null*/, const void* mask, const void* adv, void* dlogp, void* out8, void* row_len, void* row_kl, void* ws, int64_t G, int64_t C, float beta, int use_grpo, float eps_low, float eps_high, float grad_scale, void* stream);
/* ref: timer1_trainer.py:713-737 (both loss branches), extended by the trl.GRPOConfig options loss_type ("grpo" / "bnpo" / "dr_grpo": norm_mode 0 = mean over
 * each row then over rows, 1 = mean over all live tokens, 2 = sum / (G * C)), importance_sampling_level (seq_level 0 = per-token ratio exp(logp - old_logp),
 * 1 = one ratio per row, exp of the row's mean log-ratio) and delta (upper cap on the ratio in the unclipped term; <= 0 = off) on top of epsilon_low /
 * epsilon_high.  old_logp may be null (the old policy is the policy), ref_logp and tok_weight as in tr1_grpo_loss_ratio, and so are the outputs, with the
 * coefficient in use for rho.  Every division by a token count uses max(count, 1): a row without a live token contributes 0 and nothing is non-finite.
 * One block per row, ws of TR1_GRPO_POLICY_LOSS_WS_WORDS 4-byte words (zero before the first call; every call leaves it zero), no floating-point atomics. */
#define TR1_GRPO_POLICY_LOSS_WS_WORDS 528
int tr1_grpo_policy_loss(const void* logp, const void* old_logp /*may be null*/, const void* ref_logp /*may be null*/, const void* tok_weight /*may be null*/, const void* mask, const void* adv, void* dlogp, void* out8, void* row_len, void* row_kl, void* ws, int64_t G, int64_t C, float beta, int norm_mode, int seq_level, float eps_low, float eps_high, float delta, float grad_scale, void* stream);
/* ref: model.generate(do_sample=True, temperature, top_k) at timer1_trainer.py:568-573.  tokens[row*tok_ld + *step_ptr] = draw.
 * group_rows > 0: rows [b*group_rows, (b+1)*group_rows) belong to prompt b and draw from the stream (seed + b*seed_stride, row % group_rows, step),
 * so several prompts sampled in one launch get exactly the tokens of one launch per prompt.
 * done_count (last argument of the four tr1_sample_tokens* entry points; int32 [1], null = off, needs finished): a rollout that ends when every row has drawn
 * its EOS (ref: scripts/finetune/run_activitynet.sh sets --max_completion_length 1024 for answers of one or two hundred tokens).  The lane that writes a row's
 * token adds 1 with an ordinary atomicAdd when finished[row] goes 0 -> 1: once per row; a second EOS of a row that runs on (stop_at_eos = 0) and rows skipped
 * as finished do not count - tr1_greedy_tokens_step keeps the same counter - so the host polls one word instead of summing the flags.  It is declared behind
 * `stream` so that the argument list of the earlier declaration is a prefix of this one. */
int tr1_sample_tokens(const void* logits, int64_t ld, int64_t rows, int64_t V, float temperature, int64_t top_k, uint64_t seed, int64_t group_rows, uint64_t seed_stride, const void* step_ptr, void* tokens, int64_t tok_ld, void* finished, int64_t eos_id, int64_t pad_id, int stop_at_eos, void* u_out, void* ws_u32, int64_t ws_words, void* stream, void* done_count /*may be null*/);
/* The decode loop's form (model.generate's per-token sampling, timer1_trainer.py:568-573): next_ids[row] (optional) receives the drawn token as well - the
 * buffer the next step's embedding gather reads - and ws_zeroed != 0 promises a workspace zero-filled ONCE and only used through this entry point (the pick
 * kernel re-zeroes it), so neither a copy kernel nor a memset runs between two decode steps. */
int tr1_sample_tokens_step(const void* logits, int64_t ld, int64_t rows, int64_t V, float temperature, int64_t top_k, uint64_t seed, int64_t group_rows, uint64_t seed_stride, const void* step_ptr, void* tokens, int64_t tok_ld, void* finished, int64_t eos_id, int64_t pad_id, int stop_at_eos, void* u_out, void* ws_u32, int64_t ws_words, void* next_ids, int ws_zeroed, void* stream, void* done_count /*may be null*/);
int64_t tr1_sample_workspace_words(int64_t rows);
/* TF: TopPLogitsWarper and MinPLogitsWarper behind TemperatureLogitsWarper and TopKLogitsWarper (transformers generation/logits_process.py; the order of
 * GenerationMixin._get_logits_processor), and SamplingParams(top_p=...) of ref: src/vllm_inference/vllm_infer.py:106-111.  The arguments of tr1_sample_tokens /
 * tr1_sample_tokens_step plus 0 < top_p <= 1 (1 = off) and 0 <= min_p <= 1 (0 = off); workspace: tr1_sample_filtered_workspace_words(rows) words, 8-byte aligned.
 * top-p keeps a logit value iff the softmax(x/T) mass (over the top-k set) of the strictly larger logits is < top_p: equal logits stand or fall together
 * (deterministic where the warper's unstable sort is not; identical on rows without ties), the maximum always stays.  min-p keeps x iff
 * exp((x - max)/T) >= min_p.  The kept set is the intersection of the three; the draw is the inverse CDF of tr1_sample_tokens with the same Philox stream.
 * With top_p = 1 and min_p = 0 the launches and the tokens are those of tr1_sample_tokens / tr1_sample_tokens_step. */
int tr1_sample_tokens_filtered(const void* logits, int64_t ld, int64_t rows, int64_t V, float temperature, int64_t top_k, float top_p, float min_p, uint64_t seed, int64_t group_rows, uint64_t seed_stride, const void* step_ptr, void* tokens, int64_t tok_ld, void* finished, int64_t eos_id, int64_t pad_id, int stop_at_eos, void* u_out, void* ws_u32, int64_t ws_words, void* stream, void* done_count /*may be null*/);
int tr1_sample_tokens_filtered_step(const void* logits, int64_t ld, int64_t rows, int64_t V, float temperature, int64_t top_k, float top_p, float min_p, uint64_t seed, int64_t group_rows, uint64_t seed_stride, const void* step_ptr, void* tokens, int64_t tok_ld, void* finished, int64_t eos_id, int64_t pad_id, int stop_at_eos, void* u_out, void* ws_u32, int64_t ws_words, void* next_ids, int ws_zeroed, void* stream, void* done_count /*may be null*/);
int64_t tr1_sample_filtered_workspace_words(int64_t rows);
/* TF: RepetitionPenaltyLogitsProcessor (transformers generation/logits_process.py), SamplingParams(repetition_penalty=...) of ref:
 * src/vllm_inference/vllm_infer.py:106-111.  out[r, v] = logits[r, v] where bit v of seen[r] is clear, else x * penalty (x < 0) or x / penalty, computed in
 * fp32 with an IEEE division and rounded ONCE to nearest-even bf16 (the warper keeps fp32; the sampler's domain here is bf16).  seen: uint32 [rows, seen_ld],
 * bit (v & 31) of word v >> 5.  ld may be 0 (one row shown to all).  out must not alias logits. */
int tr1_penalize_logits(const void* logits, int64_t ld, void* out, int64_t out_ld, const void* seen, int64_t seen_ld, int64_t rows, int64_t V, float penalty, void* stream);
/* The seen sets of the penalty (TF: RepetitionPenaltyLogitsProcessor gathers over input_ids = prompt + generated tokens): ids[n] (a prompt) into each of `rows`
 * bitmap rows; and the token every row has just drawn, tokens[r*tok_ld + *step_ptr] (step_ptr null: offset 0), except rows with finished[r] != 0 (finished may
 * be null), whose token is padding.  Ids outside [0, V) are ignored.  Marking twice changes nothing. */
int tr1_mark_seen_ids(const void* ids, int64_t n, void* seen, int64_t seen_ld, int64_t rows, int64_t V, void* stream);
int tr1_mark_seen_drawn(const void* tokens, int64_t tok_ld, const void* step_ptr, const void* finished, void* seen, int64_t seen_ld, int64_t rows, int64_t V, void* stream);
/* ref: the greedy SamplingParams(temperature=0) of the evaluation / filtering decoder, src/vllm_inference/vllm_infer.py:80-113.  bf16 logits [rows, V], row
 * stride ld >= V, any V >= 1, any 2-byte-aligned pointer.  Row r with finished[r] != 0: pad_id goes to tokens[r*tok_ld + *step_ptr] and next_ids[r], no logit
 * is read.  Otherwise the token is the LOWEST index among the entries equal to the row maximum (compared as floats); it goes to tokens and next_ids, and when it
 * equals eos_id, finished[r] = 1 and *done_count += 1 (int32 on the device, zeroed by the caller once per generate call).  next_ids and done_count may be null.
 * One launch, no workspace, no memset. */
int tr1_greedy_tokens_step(const void* logits, int64_t ld, int64_t rows, int64_t V, const void* step_ptr, void* tokens, int64_t tok_ld, void* finished, int64_t eos_id, int64_t pad_id, void* next_ids, void* done_count, void* stream);

/* ---- optimizer -------------------------------------------------------------------------------------------------------- */
/* ref: DeepSpeed FusedAdam / DeepSpeedCPUAdam selected by scripts/zero3.json:13-21 and zero3_offload.json:24-31 (AdamW, clip 1.0) */
int tr1_sumsq_accum(const void* g, int64_t n, void* out_scalar, void* ws_f32, int64_t ws_floats, void* stream);
int tr1_adamw_step(void* p_f32, void* m_f32, void* v_f32, void* g_f32, void* p_bf16, int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay, int64_t step, const void* sumsq_scalar, float max_norm, float grad_mult, int zero_grad, void* stream);
/* Data-parallel forms: the all-reduced gradient is consumed from its bf16 wire buffer (no copy back into the fp32 accumulator, which is only
 * zeroed).  ref: DeepSpeed's bf16 gradient all-reduce + FusedAdam (scripts/zero3.json:13-33). */
int tr1_adamw_step_g16(void* p_f32, void* m_f32, void* v_f32, void* g_f32, const void* g_bf16, void* p_bf16, int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay, int64_t step, const void* sumsq_scalar, float max_norm, float grad_mult, int zero_grad, void* stream);
/* AdamW with bf16 moments (GRPOConfig.optimizer_state_dtype = "bf16"): m and v are read as bf16 and widened exactly; coef, gg, m', v', denom and p' are
 * tr1_adamw_step's expressions in fp32; p' and p_bf16 = bf16_rne(p') come from the UNROUNDED m', v' (the master update of a step is the fp32-state kernel's);
 * then m', v' are stored rounded stochastically.  The chain sumsq -> coef -> gg -> m', v' runs without fma contraction, each operation rounded once:
 * m' = b1*m + (1-b1)*gg, v' = b2*v + ((1-b2)*gg)*gg, coef = grad_mult * fminf(1, max_norm / (sqrtf(sumsq)*grad_mult + 1e-6f)) - a host fp32 emulation gives the
 * same bits.  Rounding of fp32 bits b with a 16-bit r: mag = b & 0x7fffffff; mag >= 0x7f800000 (inf / NaN) -> nearest-even; else s = min(mag + r, 0x7f7fffff)
 * and the result is ((b & 0x80000000) | s) >> 16.  Random bits of the GLOBAL element e = index_base + i: Philox4x32-10, key (seed & 0xffffffff, seed >> 32),
 * counter ((e >> 2) & 0xffffffff, (e >> 2) >> 32, step & 0xffffffff, 0x53523136), output word e & 3: its low 16 bits round m, its high 16 bits v.  index_base
 * (>= 0, any value) is the offset of element 0 in the whole arena: splitting a range into several calls or sharding it over ranks changes no bit.
 * g_bf16 (nullable): the gradient is read from this bf16 array (the wire buffer) and g_f32 is only zeroed.  Never synchronises; n == 0 is a no-op; step >= 1;
 * views may start at any element. */
int tr1_adamw_step_sr16(void* p_f32, void* m_bf16, void* v_bf16, void* g_f32, const void* g_bf16, void* p_bf16, int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay, int64_t step, const void* sumsq_scalar, float max_norm, float grad_mult, int zero_grad, uint64_t seed, int64_t index_base, void* stream);
/* Gradient norm without re-reading the large gradient matrices (ref: torch.nn.utils.clip_grad_norm_ inside HF Trainer.training_step, TF trainer.py:1785 /
 * DeepSpeed gradient_clipping, scripts/zero3.json:35).  tr1_wgrad_f32_sumsq is the weight-gradient GEMM (NT or K-major B form, bit-identical C) whose epilogue
 * also leaves one sum of squares per wave of what it stored - in the LAST micro-step of an accumulation window that is the final gradient; *n_partials (HOST)
 * receives the number of floats written.  tr1_sumsq_partials_accum adds them to the norm scalar in a fixed order (two levels; the buffer must have room for 256 more floats behind its n entries); tr1_sumsq_ranges_periodic adds the small
 * per-layer tensors (same range description as tr1_zero_ranges_periodic).  wire_bf16 (optional, [M, N] bf16, leading dimension ld_wire): the stored value rounded to bf16 as well - the data-parallel gradient exchange's wire copy (dist.GradSync / ShardSync) without its staging pass. */
int tr1_wgrad_f32_sumsq(const void* A, const void* B, void* C_f32, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc, int accumulate, int b_kmajor, int64_t b_rows, void* sumsq_partials, int64_t partials_capacity, int64_t* n_partials, void* wire_bf16, int64_t ld_wire, void* stream);
int tr1_sumsq_partials_accum(const void* partials_f32, int64_t n, void* out_scalar, void* stream);
int tr1_sumsq_ranges_periodic(const void* g_f32, int64_t base, int64_t stride, int64_t count, const int64_t* rel_ranges, int64_t n_ranges, void* out_scalar, void* ws_f32, int64_t ws_floats, void* stream);
/* g[base + l*stride + r] = 0 for l < count, r in the <= 8 half-open ranges (rel_ranges = HOST array of 2*n_ranges offsets inside one period): clears the small
 * per-layer gradient tensors when the optimizer leaves the large matrices un-zeroed (their weight-gradient GEMMs overwrite them on the first micro-step of the
 * next accumulation window).  ref: optimizer.zero_grad() in HF Trainer.training_step / DeepSpeed engine.step (scripts/zero3.json). */
int tr1_zero_ranges_periodic(void* g_f32, int64_t base, int64_t stride, int64_t count, const int64_t* rel_ranges, int64_t n_ranges, void* stream);
int tr1_sumsq_accum_bf16(const void* g_bf16, int64_t n, void* out_scalar, void* ws_f32, int64_t ws_floats, void* stream);
/* Reference-policy sync: trl.GRPOConfig.sync_ref_model / ref_model_mixup_alpha (trl's SyncRefModelCallback, the TR-DPO rule); the reference re-anchors its
 * frozen policy (timer1_trainer.py:295-307) only by starting a new process per epoch.  In place on ref: ref[i] = bf16_rne(fadd(fmul(1 - alpha, ref[i]),
 * fmul(alpha, policy[i]))) with three separately rounded fp32 operations (1 - alpha rounded once on the host) and ONE rounding to bf16, where trl's bf16
 * mul_ then add_ round twice.  alpha in [0, 1]; for finite data alpha = 0 returns ref and alpha = 1 returns policy (a zero comes out as +0 where the other
 * term is a zero of the opposite sign, as in IEEE addition).  sums_f32[0] = sum (policy - ref)^2 and sums_f32[1] = sum ref^2 of the values BEFORE the mix
 * (fp32, per-block partials added in a fixed order: the same inputs give the same bits); written, not accumulated; n = 0 writes two zeros.
 * Both arrays 16-byte aligned and distinct, any n.  ws_f32: >= 4096 floats of scratch. */
int tr1_ref_mixup(void* ref_bf16, const void* policy_bf16, int64_t n, float alpha, void* sums_f32, void* ws_f32, int64_t ws_floats, void* stream);

/* ---- LoRA (peft_config; csrc/lora.hip) -----------------------------------------------------------------------------------------
 * ref: GRPOTrainer's peft_config (timer1_trainer.py:290-293, get_peft_config in main.py) -> peft.tuners.lora.Linear.  The adapters are kept MERGED: the policy's
 * weight is W = bf16_rne(W0 + s Bt^T A), rebuilt from the frozen base copy W0 and the fp32 adapter masters after every optimizer step.
 * tr1_lora_merge: W [out, in] bf16 (leading dimension ldw; a row slice of the fused q|k|v or gate|up matrix is a pointer offset), W0 likewise (ldw0), A fp32
 * [r, in] and Bt fp32 [r, out] contiguous, r in {16, 32, 64}.  Arithmetic, each operation rounded to fp32 on its own (no fma): acc = 0; for j ascending:
 * acc = fadd(acc, fmul(Bt[j, o], A[j, i])); W[o, i] = bf16_rne(fadd(W0[o, i], fmul(s, acc))).  in, ldw, ldw0 multiples of 8; W, W0, A 16-byte aligned; W != W0.
 * tr1_lora_wgrad: G [r, Wd] fp32 (ldg) (+)= scale * thin^T wide with thin bf16 [M, r] (ldt) and wide bf16 [M, Wd] (ldw; a column slice is a pointer offset), both
 * read as stored, once (bf16 MFMA, fp32 accumulate).  The rows are dealt to S splits of whole TR1_LORA_WGRAD_MCHUNK-row chunks, S the largest count that keeps
 * S * ceil(Wd / TR1_LORA_WGRAD_COLS) at or below TR1_LORA_WGRAD_BLOCKS (at least 1, at most the number of chunks) - a function of (M, Wd) alone; S > 1 goes
 * through S fp32 planes of r * Wd floats in ws_f32, added in ascending order: the same inputs give the same bits.  Wd, ldt, ldw multiples of 8; thin and wide
 * 16-byte aligned. */
#define TR1_LORA_WGRAD_MCHUNK 256
#define TR1_LORA_WGRAD_COLS 64
#define TR1_LORA_WGRAD_BLOCKS 1024
int tr1_lora_merge(void* W_bf16, int64_t ldw, const void* W0_bf16, int64_t ldw0, const void* A_f32, const void* Bt_f32, int64_t out, int64_t in, int64_t r, float s, void* stream);
int tr1_lora_wgrad(void* G_f32, int64_t ldg, const void* thin_bf16, int64_t ldt, const void* wide_bf16, int64_t ldw, int64_t M, int64_t Wd, int64_t r, float scale, int accumulate, void* ws_f32, int64_t ws_floats, void* stream);

/* ---- Collectives (rccl_{init, allreduce, reduce_scatter, allgather}) ------------------------------------------------------------------
 * There is ONE exchange path: time-r1_amd/dist.py drives RCCL through torch.distributed's "nccl" backend (which IS librccl on ROCm): per-segment
 * all-reduce (GradSync) or reduce-scatter + all-gather (ShardSync) of the bf16 wire arena, overlapped with the backward.  The round-4/5
 * tr1_rccl_* entry points duplicated that binding without a caller in the product and were removed in round 6; a native host links librccl directly
 * (ncclCommInitRank / ncclAllReduce / ncclReduceScatter / ncclAllGather on the stream it hands to the tr1_* kernels) - see INTEGRATION.md 2c. */

#ifdef __cplusplus
}
#endif
#endif
