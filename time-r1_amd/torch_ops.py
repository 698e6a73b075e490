"""PyTorch-ROCm custom ops over the C ABI: `torch.ops.timer1.*` (SURVEY.md 8b "op-level" seam).

Every op is registered with the dispatcher through `torch.library.custom_op` (schema, CUDA/HIP kernel, fake/meta kernel, autograd
formula that itself calls the matching `*_bwd` op), so the kernels compose with autograd, `torch.library.opcheck` and tracing, and can be
dropped into the REFERENCE's own HF model (`Qwen2_5_VLForConditionalGeneration`, reference src/time_r1/rl/timer1_trainer.py:244-262)
without this repo's engine:

    import time_r1_amd.torch_ops as T
    T.patch_hf_model(model)                      # Qwen2RMSNorm.forward -> timer1::rmsnorm, SwiGLU -> timer1::swiglu (+ optional nn.Linear -> timer1::linear)
    model = Qwen2_5_VLForConditionalGeneration.from_pretrained(path, attn_implementation="timer1_hip")      # after T.register_hf_attention()

Device contract: the implementations are HIP only (`device_types="cuda"`); a CPU tensor raises NotImplementedError from the dispatcher -
there is no fallback.  Kernels are launched on torch's CURRENT stream of the tensor's device; nothing is retained past the call.
Activations are bf16, statistics / gradients of parameters fp32 (cast to the parameter dtype by the wrappers).
"""
import inspect
from typing import Optional, Tuple

import torch
from torch import Tensor

from .ops import GRPO_LEVELS, LOSS_TYPE_NORM, HipOps

BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32
_OPS = {}


def _ops(t: Tensor) -> HipOps:
    d = t.device
    if d.type != "cuda":
        raise NotImplementedError("timer1 ops are HIP-only (got a %s tensor); there is no CPU fallback" % d.type)
    o = _OPS.get(d.index)
    if o is None:
        o = _OPS[d.index] = HipOps("cuda:%d" % (d.index if d.index is not None else torch.cuda.current_device()))
    return o


def _rows(x: Tensor) -> Tensor:
    return x.reshape(-1, x.shape[-1]).contiguous()


_op = lambda name, **k: torch.library.custom_op("timer1::" + name, mutates_args=k.pop("mutates_args", ()), device_types="cuda", **k)  # noqa: E731


# ===================================================================================================================== RMSNorm
# Qwen2RMSNorm (transformers modeling_qwen2_vl.py:96-110): y = w * (x * rsqrt(mean(x^2) + eps)).to(dtype)
@_op("rmsnorm_fwd")
def rmsnorm_fwd(x: Tensor, w: Tensor, eps: float) -> Tuple[Tensor, Tensor]:
    y, rstd, _ = _ops(x).rmsnorm_fwd(x, w, eps)
    return y, rstd


@rmsnorm_fwd.register_fake
def _(x, w, eps):
    return torch.empty_like(x), x.new_empty(x.shape[0], dtype=F32)


@_op("rmsnorm_bwd")
def rmsnorm_bwd(dy: Tensor, x: Tensor, w: Tensor, rstd: Tensor) -> Tuple[Tensor, Tensor]:
    dw = torch.zeros(w.numel(), dtype=F32, device=x.device)
    dx = _ops(x).rmsnorm_bwd(dy, x, w, rstd, dw=dw)
    return dx, dw


@rmsnorm_bwd.register_fake
def _(dy, x, w, rstd):
    return torch.empty_like(x), w.new_empty(w.numel(), dtype=F32)


def _rms_setup(ctx, inputs, output):
    x, w, _ = inputs
    ctx.save_for_backward(x, w, output[1])


def _rms_backward(ctx, dy, _drstd):
    x, w, rstd = ctx.saved_tensors
    dx, dw = torch.ops.timer1.rmsnorm_bwd(dy.contiguous(), x, w, rstd)
    return dx, dw.to(w.dtype), None


rmsnorm_fwd.register_autograd(_rms_backward, setup_context=_rms_setup)


def rmsnorm(x: Tensor, w: Tensor, eps: float = 1e-6) -> Tensor:
    """Any leading shape; last dim = hidden.  Differentiable in x and w."""
    y, _ = torch.ops.timer1.rmsnorm_fwd(_rows(x), w.contiguous(), float(eps))
    return y.view(x.shape)


# ====================================================================================================================== SwiGLU
# Qwen2MLP (modeling_qwen2_vl.py:459-466): down(silu(gate(x)) * up(x)); here on the fused [rows, 2I] = [gate | up] projection output
@_op("swiglu_fwd")
def swiglu_fwd(gu: Tensor) -> Tensor:
    return _ops(gu).swiglu_fwd(gu)


@swiglu_fwd.register_fake
def _(gu):
    return gu.new_empty(gu.shape[0], gu.shape[1] // 2)


@_op("swiglu_bwd")
def swiglu_bwd(da: Tensor, gu: Tensor) -> Tensor:
    return _ops(gu).swiglu_bwd(da, gu)


@swiglu_bwd.register_fake
def _(da, gu):
    return torch.empty_like(gu)


swiglu_fwd.register_autograd(lambda ctx, da: torch.ops.timer1.swiglu_bwd(da.contiguous(), ctx.saved_tensors[0]),
                             setup_context=lambda ctx, inputs, output: ctx.save_for_backward(inputs[0]))


def swiglu(gate_up: Tensor) -> Tensor:
    a = torch.ops.timer1.swiglu_fwd(_rows(gate_up))
    return a.view(*gate_up.shape[:-1], gate_up.shape[-1] // 2)


# ====================================================================================================================== Linear
# bf16 MFMA GEMM (LDS-staged 128x128 / 256x256 tiles): y = x W^T (+ b); dgrad reads W as stored (K-major "NN" form), wgrad accumulates in fp32
@_op("linear_fwd")
def linear_fwd(x: Tensor, w: Tensor, bias: Optional[Tensor]) -> Tensor:
    return _ops(x).gemm_nt(x, w, bias=bias)


@linear_fwd.register_fake
def _(x, w, bias):
    return x.new_empty(x.shape[0], w.shape[0])


@_op("linear_bwd")
def linear_bwd(dy: Tensor, x: Tensor, w: Tensor, need_bias: bool) -> Tuple[Tensor, Tensor, Tensor]:
    o = _ops(x)
    dx = o.gemm_nn(dy, w)
    dw = o.gemm_nt(o.transpose(dy), o.transpose(x), out_f32=True)
    db = torch.zeros(w.shape[0] if need_bias else 0, dtype=F32, device=x.device)
    if need_bias:
        o.colsum_accum(dy, db)
    return dx, dw, db


@linear_bwd.register_fake
def _(dy, x, w, need_bias):
    return torch.empty_like(x), w.new_empty(w.shape, dtype=F32), w.new_empty(w.shape[0] if need_bias else 0, dtype=F32)


def _lin_setup(ctx, inputs, output):
    x, w, b = inputs
    ctx.save_for_backward(x, w)
    ctx.has_bias = b is not None
    ctx.b_dtype = b.dtype if b is not None else None


def _lin_backward(ctx, dy):
    x, w = ctx.saved_tensors
    dx, dw, db = torch.ops.timer1.linear_bwd(dy.contiguous(), x, w, ctx.has_bias)
    return dx, dw.to(w.dtype), (db.to(ctx.b_dtype) if ctx.has_bias else None)


linear_fwd.register_autograd(_lin_backward, setup_context=_lin_setup)


def linear(x: Tensor, w: Tensor, bias: Optional[Tensor] = None) -> Tensor:
    """x [..., K] @ w[N, K]^T; K must be a multiple of 64 (the kernels' K tile)."""
    y = torch.ops.timer1.linear_fwd(_rows(x), w.contiguous(), bias)
    return y.view(*x.shape[:-1], w.shape[0])


# ===================================================================================================================== rotary
# rotate-half RoPE with per-token cos/sin tables [T, hd/2] fp32 (M-RoPE tables come from mrope_table; vision tables from vision_rope_table)
@_op("rope_fwd")
def rope_fwd(x: Tensor, cos: Tensor, sin: Tensor, n_heads: int, head_dim: int, backward: bool) -> Tensor:
    return _ops(x).rope_apply(x, n_heads, head_dim, cos, sin, backward=backward)


@rope_fwd.register_fake
def _(x, cos, sin, n_heads, head_dim, backward):
    return x.new_empty(x.shape[0], n_heads * head_dim)


def _rope_setup(ctx, inputs, output):
    _, cos, sin, ctx.nh, ctx.hd, ctx.bwd = inputs
    ctx.save_for_backward(cos, sin)


def _rope_backward(ctx, dy):        # the rotation is orthogonal: its gradient is the inverse rotation
    cos, sin = ctx.saved_tensors
    return torch.ops.timer1.rope_fwd(dy.contiguous(), cos, sin, ctx.nh, ctx.hd, not ctx.bwd), None, None, None, None, None


rope_fwd.register_autograd(_rope_backward, setup_context=_rope_setup)


def rope(x: Tensor, cos: Tensor, sin: Tensor, n_heads: int, head_dim: int) -> Tensor:
    """x [T, n_heads*head_dim] bf16; cos/sin [T, head_dim/2] fp32."""
    return torch.ops.timer1.rope_fwd(x.contiguous(), cos.contiguous(), sin.contiguous(), n_heads, head_dim, False)


@_op("mrope_table")
def mrope_table(pos3: Tensor, head_dim: int, s0: int, s1: int, s2: int, theta: float) -> Tuple[Tensor, Tensor]:
    return _ops(pos3).mrope_table(pos3, head_dim, (s0, s1, s2), theta)


@mrope_table.register_fake
def _(pos3, head_dim, s0, s1, s2, theta):
    T = pos3.shape[1]
    return pos3.new_empty(T, head_dim // 2, dtype=F32), pos3.new_empty(T, head_dim // 2, dtype=F32)


# =================================================================================================================== attention
# Two-interval mask per query row t: keys kv < pre[t] or lo[t] <= kv <= hi[t].  Causal: pre = 0, lo = 0, hi = t.  Varlen (cu_seqlens):
# lo = segment start, hi = segment end - 1.  Shared-prefix GRPO packing: pre = P for completion rows.  GQA by n_heads / n_kv.
@_op("attn_fwd")
def attn_fwd(q: Tensor, k: Tensor, v: Tensor, pre: Tensor, lo: Tensor, hi: Tensor, n_heads: int, n_kv: int, head_dim: int, scale: float) -> Tuple[Tensor, Tensor]:
    o = _ops(q)
    vt = o.pack_transpose(v, n_kv, n_kv, head_dim)
    out, lse = o.attn_fwd(q, k, vt, pre, lo, hi, n_heads, n_kv, k.shape[0], head_dim, scale, need_lse=True)
    return out, lse


@attn_fwd.register_fake
def _(q, k, v, pre, lo, hi, n_heads, n_kv, head_dim, scale):
    return q.new_empty(q.shape[0], n_heads * head_dim), q.new_empty(n_heads, q.shape[0], dtype=F32)


@_op("attn_bwd")
def attn_bwd(do: Tensor, q: Tensor, k: Tensor, v: Tensor, out: Tensor, lse: Tensor, pre: Tensor, lo: Tensor, hi: Tensor, n_heads: int, n_kv: int,
             head_dim: int, scale: float) -> Tuple[Tensor, Tensor, Tensor]:
    return _ops(q).attn_bwd(q, k, v, out, do, lse, pre, lo, hi, n_heads, n_kv, k.shape[0], head_dim, scale)


@attn_bwd.register_fake
def _(do, q, k, v, out, lse, pre, lo, hi, n_heads, n_kv, head_dim, scale):
    return torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)


def _attn_setup(ctx, inputs, output):
    q, k, v, pre, lo, hi, nh, nkv, hd, scale = inputs
    ctx.save_for_backward(q, k, v, output[0], output[1], pre, lo, hi)
    ctx.cfg = (nh, nkv, hd, scale)


def _attn_backward(ctx, do, _dlse):
    q, k, v, out, lse, pre, lo, hi = ctx.saved_tensors
    dq, dk, dv = torch.ops.timer1.attn_bwd(do.contiguous(), q, k, v, out, lse, pre, lo, hi, *ctx.cfg)
    return dq, dk, dv, None, None, None, None, None, None, None


attn_fwd.register_autograd(_attn_backward, setup_context=_attn_setup)


def attention(q: Tensor, k: Tensor, v: Tensor, pre: Tensor, lo: Tensor, hi: Tensor, n_heads: int, n_kv: int, head_dim: int, scale: Optional[float] = None) -> Tensor:
    """q [T, n_heads*hd], k / v [S, n_kv*hd] (S == T for self-attention over one packed sequence), masks int32 [T]."""
    scale = head_dim ** -0.5 if scale is None else scale
    return torch.ops.timer1.attn_fwd(q.contiguous(), k.contiguous(), v.contiguous(), pre, lo, hi, n_heads, n_kv, head_dim, float(scale))[0]


def causal_masks(T: int, device) -> Tuple[Tensor, Tensor, Tensor]:
    z = torch.zeros(T, dtype=I32, device=device)
    return z, z, torch.arange(T, dtype=I32, device=device)


def varlen_masks(cu_seqlens: Tensor, causal: bool = False) -> Tuple[Tensor, Tensor, Tensor]:
    """flash-attn style cu_seqlens [n+1] -> (pre, lo, hi) for non-causal (ViT) or causal segments."""
    cu = cu_seqlens.to(torch.long)
    T = int(cu[-1])
    idx = torch.arange(T, device=cu.device)
    seg = torch.searchsorted(cu[1:], idx, right=True)
    lo = cu[seg]
    hi = idx if causal else cu[seg + 1] - 1
    return torch.zeros(T, dtype=I32, device=cu.device), lo.to(I32), hi.to(I32)


# ========================================================================================================== vocabulary / loss side
@_op("logp_entropy_fwd")
def logp_entropy_fwd(logits: Tensor, targets: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    return _ops(logits).logp_entropy_fwd(logits, targets)


@logp_entropy_fwd.register_fake
def _(logits, targets):
    R = logits.shape[0]
    return logits.new_empty(R, dtype=F32), logits.new_empty(R, dtype=F32), logits.new_empty(R, dtype=F32)


@_op("logp_bwd")
def logp_bwd(logits: Tensor, targets: Tensor, lse: Tensor, dlogp: Tensor) -> Tensor:
    return _ops(logits).logp_bwd(logits, targets, lse, dlogp, inplace=False)


@logp_bwd.register_fake
def _(logits, targets, lse, dlogp):
    return torch.empty_like(logits)


@_op("logp_entropy_bwd")
def logp_entropy_bwd(logits: Tensor, targets: Tensor, lse: Tensor, ent: Tensor, dlogp: Tensor, dent: Tensor) -> Tensor:
    return _ops(logits).logp_entropy_bwd(logits, targets, lse, ent, dlogp, dent, inplace=False)


@logp_entropy_bwd.register_fake
def _(logits, targets, lse, ent, dlogp, dent):
    return torch.empty_like(logits)


def _lp_setup(ctx, inputs, output):
    ctx.set_materialize_grads(False)                   # an output the graph never uses arrives as None in the backward, not as zeros
    ctx.save_for_backward(inputs[0], inputs[1], output[2], output[1])


def _lp_backward(ctx, dlogp, dent, _dlse):
    logits, targets, lse, ent = ctx.saved_tensors
    if dent is None:                                   # the entropy is only a logged metric (reference :473-481 computes it under no_grad): logp_bwd, as ever
        if dlogp is None:
            return None, None
        return torch.ops.timer1.logp_bwd(logits, targets, lse, dlogp.contiguous().float()), None
    dlogp = torch.zeros_like(lse) if dlogp is None else dlogp.contiguous().float()
    return torch.ops.timer1.logp_entropy_bwd(logits, targets, lse, ent, dlogp, dent.contiguous().float()), None


logp_entropy_fwd.register_autograd(_lp_backward, setup_context=_lp_setup)


def logp_entropy(logits: Tensor, targets: Tensor) -> Tuple[Tensor, Tensor]:
    """Per-row log-softmax gathered at `targets` + entropy of the row distribution, one pass over [R, V] bf16 logits
    (reference timer1_trainer.py:458-481).  Differentiable in logits through both outputs: a loss that uses the entropy (an entropy bonus) runs
    timer1::logp_entropy_bwd, one that uses logp alone runs timer1::logp_bwd."""
    lp, ent, _ = torch.ops.timer1.logp_entropy_fwd(logits.contiguous(), targets.to(I32).contiguous())
    return lp, ent


@_op("entropy_quantile_weight")
def entropy_quantile_weight_op(ent: Tensor, mask: Tensor, rho: float) -> Tuple[Tensor, Tensor]:
    return _ops(ent).entropy_quantile_weight(ent, mask, rho)


@entropy_quantile_weight_op.register_fake
def _(ent, mask, rho):
    return torch.empty_like(ent), ent.new_empty(3)


def entropy_quantile_weight(entropy: Tensor, completion_mask: Tensor, top_entropy_quantile: float) -> Tuple[Tensor, Tensor]:
    """-> (weight, stats).  trl.GRPOConfig.top_entropy_quantile: weight is 1 on the live tokens whose entropy is at or above the (1 - top_entropy_quantile) quantile
    of the live entropies and 0 elsewhere - the tok_weight of grpo_loss_ratio / grpo_policy_loss.  stats = [threshold, tokens kept, live tokens].  No gradient."""
    return torch.ops.timer1.entropy_quantile_weight(entropy.detach().float().contiguous(), completion_mask.to(I32).contiguous(), float(top_entropy_quantile))


@_op("lmhead_logp_entropy")
def lmhead_logp_entropy(hn: Tensor, w: Tensor, targets: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """(logp[target], entropy, lse) of softmax(hn @ w^T) per row with the statistics reduced in the GEMM epilogue: no [R, V] logits in HBM
    (forward only - the no-grad reference-policy log-probs of timer1_trainer.py:613-632)."""
    r = _ops(hn).lmhead_lse(hn, w, targets)
    if r is None:
        raise RuntimeError("lmhead_logp_entropy: needs V % 64 == 0, K % 64 == 0, V >= 256 and row-major operands")
    return r


@lmhead_logp_entropy.register_fake
def _(hn, w, targets):
    R = hn.shape[0]
    return hn.new_empty(R, dtype=F32), hn.new_empty(R, dtype=F32), hn.new_empty(R, dtype=F32)


def _grpo_op(name, n_out):
    """_op for the three GRPO loss ops, which share everything but their arguments: -> (out [n_out], dlogp [G, C], row_len [G]); the kernel has already written
    d loss / d logp, so the backward is dlogp * d out[0] for logp and None for every other argument."""
    def deco(fn):
        op = _op(name)(fn)
        n_in = len(inspect.signature(fn).parameters)
        op.register_fake(lambda logp, *a, **k: (logp.new_empty(n_out), torch.empty_like(logp), logp.new_empty(logp.shape[0])))
        op.register_autograd(lambda ctx, dout, _d1, _d2: (ctx.saved_tensors[0] * dout[0],) + (None,) * (n_in - 1),
                             setup_context=lambda ctx, inputs, output: ctx.save_for_backward(output[1]))
        return op
    return deco


def _grpo_call(op, logp, old_logp, ref_logp, tok_weight, completion_mask, advantages, beta, *mode):
    """The public wrappers' side of grpo_loss_ratio / grpo_policy_loss: constants detached and made fp32, grad_scale 1 -> (loss, mean k3-KL, stats)."""
    const = lambda t: None if t is None else t.detach().float().contiguous()  # noqa: E731
    out8, _, _ = op(logp.contiguous(), const(old_logp), ref_logp, const(tok_weight), completion_mask.to(I32).contiguous(), advantages.float().contiguous(),
                    float(beta), *mode, 1.0)
    return out8[0], out8[1], out8[3:]


@_grpo_op("grpo_loss", 3)
def grpo_loss_op(logp: Tensor, ref_logp: Optional[Tensor], mask: Tensor, adv: Tensor, beta: float, use_grpo: bool, grad_scale: float) -> Tuple[Tensor, Tensor, Tensor]:
    dlogp, out3, row_len, _ = _ops(logp).grpo_loss(logp, ref_logp, mask, adv, beta, use_grpo, grad_scale)
    return out3, dlogp, row_len


def grpo_loss(logp: Tensor, ref_logp: Optional[Tensor], completion_mask: Tensor, advantages: Tensor, beta: float, use_grpo: bool) -> Tuple[Tensor, Tensor]:
    """-> (loss, mean k3-KL).  logp fp32 [G, C]; the loss algebra of reference timer1_trainer.py:635-737 (k3 KL, both loss branches) in one
    kernel that also produces dL/dlogp, which the autograd formula hands back."""
    out3, _, _ = torch.ops.timer1.grpo_loss(logp.contiguous(), ref_logp, completion_mask.to(I32).contiguous(), advantages.float().contiguous(),
                                            float(beta), bool(use_grpo), 1.0)
    return out3[0], out3[1]


@_grpo_op("grpo_loss_ratio", 8)
def grpo_loss_ratio_op(logp: Tensor, old_logp: Tensor, ref_logp: Optional[Tensor], tok_weight: Optional[Tensor], mask: Tensor, adv: Tensor, beta: float,
                       use_grpo: bool, eps_low: float, eps_high: float, grad_scale: float) -> Tuple[Tensor, Tensor, Tensor]:
    dlogp, out8, row_len, _ = _ops(logp).grpo_loss_ratio(logp, old_logp, ref_logp, mask, adv, beta, use_grpo, eps_low, eps_high, grad_scale, tok_weight=tok_weight)
    return out8, dlogp, row_len


def grpo_loss_ratio(logp: Tensor, old_logp: Tensor, ref_logp: Optional[Tensor], completion_mask: Tensor, advantages: Tensor, beta: float, use_grpo: bool,
                    epsilon_low: float = 0.2, epsilon_high: Optional[float] = None, tok_weight: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Tensor]:
    """-> (loss, mean k3-KL, stats).  The loss of reference timer1_trainer.py:730-737 against the log-probs `old_logp` of the policy that drew the completions
    (a later one of several updates on one rollout): rho = exp(logp - old_logp), clipped to [1 - epsilon_low, 1 + epsilon_high] on the side the advantage's
    sign makes matter.  stats = [low, high, either clip fraction, masked mean of rho - 1 - log rho, max rho].  Differentiable in logp only."""
    eh = epsilon_low if epsilon_high is None else epsilon_high
    return _grpo_call(torch.ops.timer1.grpo_loss_ratio, logp, old_logp, ref_logp, tok_weight, completion_mask, advantages, beta, bool(use_grpo),
                      float(epsilon_low), float(eh))


@_grpo_op("grpo_policy_loss", 8)
def grpo_policy_loss_op(logp: Tensor, old_logp: Optional[Tensor], ref_logp: Optional[Tensor], tok_weight: Optional[Tensor], mask: Tensor, adv: Tensor,
                        beta: float, norm_mode: int, seq_level: int, eps_low: float, eps_high: float, delta: float, grad_scale: float) -> Tuple[Tensor, Tensor, Tensor]:
    dlogp, out8, row_len, _ = _ops(logp).grpo_policy_loss(logp, old_logp, ref_logp, mask, adv, beta, norm_mode, seq_level, eps_low, eps_high, delta, grad_scale,
                                                          tok_weight=tok_weight)
    return out8, dlogp, row_len


def grpo_policy_loss(logp: Tensor, old_logp: Optional[Tensor], ref_logp: Optional[Tensor], completion_mask: Tensor, advantages: Tensor, beta: float,
                     loss_type: str = "grpo", importance_sampling_level: str = "token", epsilon_low: float = 0.2, epsilon_high: Optional[float] = None,
                     delta: Optional[float] = None, tok_weight: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Tensor]:
    """-> (loss, mean k3-KL, stats).  The clipped GRPO loss with trl.GRPOConfig's loss_type ("grpo": mean over each completion, then over completions; "bnpo":
    mean over all live tokens; "dr_grpo": sum over G * C), importance_sampling_level ("token" | "sequence": one ratio per completion, the exp of its mean
    log-ratio) and delta (upper cap on the ratio in the unclipped term).  old_logp None: the old policy is the policy.  Completions without a live token
    contribute 0.  stats as grpo_loss_ratio's, with the coefficient in use for rho.  Differentiable in logp only."""
    eh = epsilon_low if epsilon_high is None else epsilon_high
    return _grpo_call(torch.ops.timer1.grpo_policy_loss, logp, old_logp, ref_logp, tok_weight, completion_mask, advantages, beta, LOSS_TYPE_NORM[loss_type],
                      GRPO_LEVELS[importance_sampling_level], float(epsilon_low), float(eh), float(delta) if delta else 0.0)


# ============================================================================================================ sampler / optimizer / video
@_op("sample_tokens", mutates_args=("tokens", "finished"))
def sample_tokens(logits: Tensor, temperature: float, top_k: int, seed: int, step: Tensor, tokens: Tensor, finished: Tensor, eos_id: int, pad_id: int,
                  stop_at_eos: bool) -> None:
    _ops(logits).sample_tokens(logits, temperature, top_k, seed, step, tokens, finished, eos_id, pad_id, stop_at_eos)


@_op("sample_tokens_filtered", mutates_args=("tokens", "finished"))
def sample_tokens_filtered(logits: Tensor, temperature: float, top_k: int, top_p: float, min_p: float, seed: int, step: Tensor, tokens: Tensor,
                           finished: Tensor, eos_id: int, pad_id: int, stop_at_eos: bool) -> None:
    """sample_tokens with the nucleus (top_p) and min-p filters behind top-k: TopPLogitsWarper / MinPLogitsWarper, equal logits kept or dropped together."""
    _ops(logits).sample_tokens(logits, temperature, top_k, seed, step, tokens, finished, eos_id, pad_id, stop_at_eos, top_p=top_p, min_p=min_p)


@_op("penalize_logits")
def penalize_logits(logits: Tensor, seen: Tensor, penalty: float) -> Tensor:
    """RepetitionPenaltyLogitsProcessor on bf16 logits [rows, V] with a seen bitmap int32 [rows, ceil(V / 32)]; fp32 arithmetic, one rounding to bf16."""
    return _ops(logits).penalize_logits(logits, seen, penalty)


@penalize_logits.register_fake
def _(logits, seen, penalty):
    return logits.new_empty(logits.shape)


@_op("mark_seen_ids", mutates_args=("seen",))
def mark_seen_ids(seen: Tensor, vocab_size: int, ids: Tensor) -> None:
    _ops(seen).mark_seen(seen, vocab_size, ids=ids)


@_op("mark_seen_drawn", mutates_args=("seen",))
def mark_seen_drawn(seen: Tensor, vocab_size: int, tokens: Tensor, step: Optional[Tensor], finished: Optional[Tensor]) -> None:
    _ops(seen).mark_seen(seen, vocab_size, tokens=tokens, step_dev=step, finished=finished)


@_op("adamw_step", mutates_args=("p32", "m", "v", "g", "p16"))
def adamw_step(p32: Tensor, m: Tensor, v: Tensor, g: Tensor, p16: Tensor, lr: float, beta1: float, beta2: float, eps: float, weight_decay: float, step: int,
               max_norm: float, grad_mult: float) -> Tensor:
    """Global-norm clip + AdamW on flat fp32 master / m / v / grad, bf16 working copy refreshed, grad zeroed.  Returns the pre-clip norm."""
    o = _ops(p32)
    ss = torch.zeros(1, dtype=F32, device=p32.device)
    o.sumsq_accum(g, ss)
    o.adamw_step(p32, m, v, g, p16, lr, beta1, beta2, eps, weight_decay, step, sumsq=ss, max_norm=max_norm, grad_mult=grad_mult, zero_grad=True)
    return ss.sqrt() * grad_mult


@adamw_step.register_fake
def _(p32, m, v, g, p16, lr, beta1, beta2, eps, weight_decay, step, max_norm, grad_mult):
    return p32.new_empty(1)


@_op("adamw_step_sr16", mutates_args=("p32", "m", "v", "g", "p16"))
def adamw_step_sr16(p32: Tensor, m: Tensor, v: Tensor, g: Tensor, p16: Tensor, lr: float, beta1: float, beta2: float, eps: float, weight_decay: float, step: int,
                    max_norm: float, grad_mult: float, seed: int, index_base: int) -> Tensor:
    """adamw_step with bf16 moments m / v rounded stochastically; the random bits are keyed by (seed, step, index_base + element).  Returns the pre-clip norm."""
    o = _ops(p32)
    ss = torch.zeros(1, dtype=F32, device=p32.device)
    o.sumsq_accum(g, ss)
    o.adamw_step_sr16(p32, m, v, g, p16, lr, beta1, beta2, eps, weight_decay, step, seed, index_base, sumsq=ss, max_norm=max_norm, grad_mult=grad_mult, zero_grad=True)
    return ss.sqrt() * grad_mult


@adamw_step_sr16.register_fake
def _(p32, m, v, g, p16, lr, beta1, beta2, eps, weight_decay, step, max_norm, grad_mult, seed, index_base):
    return p32.new_empty(1)


@_op("ref_mixup", mutates_args=("ref",))
def ref_mixup(ref: Tensor, policy: Tensor, alpha: float) -> Tensor:
    """trl.GRPOConfig.sync_ref_model's update: ref = (1 - alpha) ref + alpha policy in place on flat bf16 weights (fp32 arithmetic, one rounding to bf16).
    Returns fp32 [2]: sum (policy - ref)^2 and sum ref^2 of the values before the mix."""
    return _ops(ref).ref_mixup(ref, policy, alpha)


@ref_mixup.register_fake
def _(ref, policy, alpha):
    return ref.new_empty(2, dtype=F32)


@_op("lora_merge", mutates_args=("w",))
def lora_merge(w: Tensor, w0: Tensor, a: Tensor, bt: Tensor, s: float) -> None:
    """peft's merged LoRA weight from the frozen base copy: w[out, in] = bf16_rne(w0 + s * bt^T a) with fp32 adapters a [r, in], bt [r, out] (lora_B stored
    transposed), r in {16, 32, 64}; fp32 arithmetic in a pinned order, one rounding to bf16.  w / w0 may be row slices of a fused matrix."""
    _ops(w).lora_merge(w, w0, a, bt, s)


@lora_merge.register_fake
def _(w, w0, a, bt, s):
    return None


@_op("lora_wgrad", mutates_args=("g",))
def lora_wgrad(g: Tensor, thin: Tensor, wide: Tensor, scale: float, accumulate: bool) -> None:
    """g[r, Wd] fp32 (+)= scale * thin[M, r]^T @ wide[M, Wd] (bf16 operands as stored; wide may be a column slice): the rank-r weight gradients of a LoRA
    adapter.  The same inputs give the same bits."""
    _ops(g).lora_wgrad(g, thin, wide, scale, accumulate)


@lora_wgrad.register_fake
def _(g, thin, wide, scale, accumulate):
    return None


@_op("video_preprocess")
def video_preprocess(frames_u8: Tensor, out_h: int, out_w: int, k_pad: int) -> Tensor:
    """uint8 [T,3,H,W] -> bf16 [N_v, k_pad] normalised patches in the HF video processor's layout (resize + rescale + normalise + patchify)."""
    return _ops(frames_u8).video_preprocess(frames_u8, (out_h, out_w), k_pad)[0]


@video_preprocess.register_fake
def _(frames_u8, out_h, out_w, k_pad):
    T = (frames_u8.shape[0] + 1) // 2
    return frames_u8.new_empty(T * (out_h // 14) * (out_w // 14), k_pad, dtype=BF16)


# ================================================================================== packed 12-bit bf16 gate/up weights: the format in plain torch
# The definition of csrc/gemm_pk.hip's format that runs on a CPU (see the note at the head of that file): any device, integer tensor ops only.  A stage = 16 gate + 16 up rows
# of a column-group pair x 64 k, stage index (pair * 8 + wave) * NST + s; inside a stage the value of operand op (gate k-half 0 / 1, up 0 / 1), lane
# g * 16 + u, element e is W[(op >> 1) * I + pair * 16 + u, wave * K / 8 + s * 64 + (op & 1) * 32 + g * 8 + e].
PK_REC, PK_TAIL_DW, PK_P = 3072, 16, 14


def _pk_stages(w: Tensor) -> Tensor:
    """bf16 [2I, K] -> int32 bit patterns [stages, 4 operands, 64 lanes, 8 elements]."""
    I, K = w.shape[0] // 2, w.shape[1]
    nst = K // 512
    assert w.dtype == BF16 and w.shape[0] == 2 * I and I % 16 == 0 and K == 512 * nst and nst in (7, 4, 3)
    b = w.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF
    v = b.view(2, I // 16, 16, 8, nst, 2, 4, 8)                     # up, pair, u, wave, s, khalf, g, e
    return v.permute(1, 3, 4, 0, 5, 6, 2, 7).reshape(-1, 4, 64, 8)  # pair, wave, s | up, khalf | g, u | e


def pack_bf16_glu_ref(w: Tensor) -> Tuple[Tensor, Tensor, bool]:
    """-> (records uint8 [stages, 3072], tails int32 [stages, 16], representable).  Byte for byte the records and tails of the image HipOps.pack_bf16_glu writes."""
    v = _pk_stages(w)
    n = v.shape[0]
    e7 = (v >> 8) & 0x7F
    flat = e7.reshape(n, 2048)
    base = (flat.amax(dim=1) - 7).clamp_(min=0)                                            # the window under the stage's largest value ...
    over = (((flat < base[:, None]) | (flat > base[:, None] + 7)).sum(dim=1) > PK_P).nonzero(as_tuple=True)[0]
    if over.numel():                                                                       # ... unless that leaves more than PK_P values outside: the fullest window
        hist = torch.zeros(over.numel(), 129, dtype=torch.int64, device=w.device)
        hist[:, 1:].scatter_add_(1, flat[over].to(torch.int64), torch.ones(over.numel(), 2048, dtype=torch.int64, device=w.device))
        cs = hist.cumsum(dim=1)
        cover = cs[:, 8:] - cs[:, :121]                                                    # values inside the window [b, b + 7], b = 0 .. 120
        base[over] = (cover * 128 + torch.arange(121, device=w.device)).argmax(dim=1).to(base.dtype)      # among equals the highest
    off = e7 - base.view(n, 1, 1, 1)
    inw = (off >= 0) & (off <= 7)
    nib = torch.where(inw, ((v >> 15) << 3) | off, torch.zeros_like(off))
    lo = (v & 0xFF).view(n, 2, 2, 64, 8).permute(0, 1, 3, 2, 4).reshape(n, 2048)            # planes A | B: [up][lane][khalf][e]
    code = (nib[..., :4] | (nib[..., 4:] << 4)).permute(0, 2, 1, 3).reshape(n, 1024)        # plane C: [lane][op][byte]
    rec = torch.cat([lo, code], dim=1).to(torch.uint8)
    miss = ~inw.reshape(n, 2048)
    cnt = miss.sum(dim=1)
    tails = torch.zeros(n, PK_TAIL_DW, dtype=torch.int64, device=w.device)
    tails[:, 0] = base * 0x01010101
    tails[:, 1] = cnt.clamp(max=PK_P)
    r, pos = miss.nonzero(as_tuple=True)                                                   # row-major: ascending position inside each stage
    k = (miss.cumsum(dim=1) - 1)[r, pos]
    keep = k < PK_P
    tails[r[keep], 2 + k[keep]] = (pos[keep] << 16) | v.reshape(n, 2048)[r[keep], pos[keep]].to(torch.int64)
    tails = torch.where(tails >= 2 ** 31, tails - 2 ** 32, tails).to(torch.int32)
    return rec, tails, bool((cnt <= PK_P).all())


def unpack_bf16_glu_ref(rec: Tensor, tails: Tensor, I: int, K: int) -> Tensor:
    """The bf16 [2I, K] weight the packed gate/up kernel multiplies by: codes against the stage base, then the patches."""
    n, nst = rec.shape[0], K // 512
    r = rec.to(torch.int32)
    t = tails.to(torch.int64) & 0xFFFFFFFF
    lo = r[:, :2048].view(n, 2, 64, 2, 8).permute(0, 1, 3, 2, 4).reshape(n, 4, 64, 8)
    c = r[:, 2048:].view(n, 64, 4, 4).permute(0, 2, 1, 3)                                  # [op][lane][byte]
    nib = torch.cat([c & 0xF, c >> 4], dim=3)
    base = (t[:, 0] & 0x7F).to(torch.int32).view(n, 1, 1, 1)
    v = (((nib >> 3) << 15) | (((nib & 7) + base) << 8) | lo).reshape(n, 2048)
    for i in range(PK_P):
        has = (t[:, 1] > i).nonzero(as_tuple=True)[0]
        if has.numel():
            e = t[has, 2 + i]
            v[has, e >> 16] = (e & 0xFFFF).to(torch.int32)
    v = v.view(I // 16, 8, nst, 2, 2, 4, 16, 8).permute(3, 0, 6, 1, 2, 4, 5, 7).reshape(2 * I, K)
    return torch.where(v >= 2 ** 15, v - 2 ** 16, v).to(torch.int16).view(BF16)


OP_NAMES = ["rmsnorm_fwd", "rmsnorm_bwd", "swiglu_fwd", "swiglu_bwd", "linear_fwd", "linear_bwd", "rope_fwd", "mrope_table", "attn_fwd", "attn_bwd",
            "logp_entropy_fwd", "logp_bwd", "logp_entropy_bwd", "entropy_quantile_weight", "lmhead_logp_entropy", "grpo_loss", "grpo_loss_ratio", "grpo_policy_loss", "sample_tokens", "sample_tokens_filtered", "penalize_logits", "mark_seen_ids",
            "mark_seen_drawn", "adamw_step", "adamw_step_sr16", "ref_mixup", "lora_merge", "lora_wgrad", "video_preprocess"]


# ================================================================================================ dropping the ops into an HF model
class TimeR1RMSNorm(torch.nn.Module):
    """Drop-in for Qwen2RMSNorm / Qwen2_5_VLRMSNorm (same parameter name `weight`, same `variance_epsilon`)."""

    def __init__(self, hidden_size, eps=1e-6, weight=None):
        super().__init__()
        self.weight = weight if weight is not None else torch.nn.Parameter(torch.ones(hidden_size))
        self.variance_epsilon = eps

    def forward(self, hidden_states):
        return rmsnorm(hidden_states, self.weight, self.variance_epsilon)


def hf_attention_forward(module, query, key, value, attention_mask=None, dropout=0.0, scaling=None, is_causal=None, **kwargs):
    """transformers AttentionInterface signature: q [B, H, T, D], k / v [B, Hkv, S, D] -> ([B, T, H, D], None).
    Honours what transformers passes: `is_causal` (decoder: True; the Qwen2-VL / Qwen2.5-VL VISION blocks route through the same function
    with is_causal=False and flash-style `cu_seq_lens_q` -> bidirectional attention inside each frame / window), S > T (`generate` with a
    KV cache: the T new queries are the last T of the S keys, causal among themselves) and refuses what it cannot express (a padding /
    arbitrary additive mask) instead of silently ignoring it.  Reference call site: timer1_trainer.py:452-457 (logprob forward)."""
    B, Hq, T, D = query.shape
    Hkv, S = key.shape[1], key.shape[2]
    if S < T:
        raise NotImplementedError("timer1_hip attention: fewer keys (%d) than queries (%d)" % (S, T))
    causal = is_causal if is_causal is not None else bool(getattr(module, "is_causal", True))
    if attention_mask is not None:
        # transformers builds the plain causal triangle for sdpa-like backends, as an additive float mask (0 = keep) or as a bool mask
        # (True = keep); anything else (left padding, sliding windows, packed documents) cannot be expressed by one (pre, lo, hi) interval per
        # query here.  An explicit mask REPLACES is_causal in transformers' sdpa path, so an all-keep mask over T > 1 queries means bidirectional
        # attention even when the module is causal: it is honoured as such (it equals the triangle only for T == 1).
        keep = attention_mask if attention_mask.dtype == torch.bool else (attention_mask == 0)
        keep = keep.expand(B, -1, T, S).reshape(-1, T, S) if keep.dim() == 4 else keep.reshape(-1, T, S)
        tri = torch.ones(T, S, dtype=torch.bool, device=query.device).tril(S - T) if causal else torch.ones(T, S, dtype=torch.bool, device=query.device)
        full = bool((keep == tri).all())
        if not full and bool(keep.all()):
            full, causal = True, False
    else:
        full = True
    if not full:
        raise NotImplementedError("timer1_hip attention: a non-trivial attention_mask (padding / sliding window) was passed; use "
                                  "attn_implementation='sdpa' for padded batches")
    cu = kwargs.get("cu_seq_lens_q", kwargs.get("cu_seqlens"))
    if cu is not None and S == T:
        pre, lo, hi = varlen_masks(cu.to(query.device), causal=causal)
    elif causal:
        z = torch.zeros(T, dtype=I32, device=query.device)
        pre, lo, hi = z, z, torch.arange(S - T, S, dtype=I32, device=query.device)       # query t sees keys 0 .. (S - T) + t
    else:
        z = torch.zeros(T, dtype=I32, device=query.device)
        pre, lo, hi = z, z, torch.full((T,), S - 1, dtype=I32, device=query.device)
    outs = []
    for b in range(B):
        q2 = query[b].transpose(0, 1).reshape(T, Hq * D)
        k2 = key[b].transpose(0, 1).reshape(S, Hkv * D)
        v2 = value[b].transpose(0, 1).reshape(S, Hkv * D)
        outs.append(attention(q2, k2, v2, pre, lo, hi, Hq, Hkv, D, scaling).view(T, Hq, D))
    return torch.stack(outs, 0), None


def register_hf_attention(name="timer1_hip"):
    """After this, `attn_implementation="timer1_hip"` selects the HIP attention inside any transformers model."""
    from transformers import AttentionInterface
    AttentionInterface.register(name, hf_attention_forward)
    return name


def _is_silu(act):
    name = getattr(act, "__name__", type(act).__name__).lower()
    return "silu" in name and "quick" not in name


def patch_hf_model(model, rmsnorm_modules=True, swiglu_mlp=True, linears=False):
    """Swap the hot modules of an HF Qwen2-VL / Qwen2.5-VL model (bf16, on a HIP device) for the timer1 ops, in place.
    rmsnorm_modules: every *RMSNorm module's forward.  swiglu_mlp: MLPs with gate_proj / up_proj / down_proj compute act(gate)*up through
    timer1::swiglu.  linears: also route nn.Linear layers whose in_features % 64 == 0 through timer1::linear (MFMA GEMM + own dgrad / wgrad)."""
    import types
    n = dict(rmsnorm=0, mlp=0, linear=0)
    for mod in model.modules():
        cls = type(mod).__name__
        if rmsnorm_modules and cls.endswith("RMSNorm") and hasattr(mod, "weight"):
            eps = getattr(mod, "variance_epsilon", getattr(mod, "eps", 1e-6))
            mod.forward = types.MethodType(lambda self, x, _eps=eps: rmsnorm(x, self.weight, _eps), mod)
            n["rmsnorm"] += 1
        elif swiglu_mlp and all(hasattr(mod, a) for a in ("gate_proj", "up_proj", "down_proj")) and _is_silu(getattr(mod, "act_fn", None)):
            def mlp_forward(self, x):
                gu = torch.cat([self.gate_proj(x), self.up_proj(x)], dim=-1)
                return self.down_proj(swiglu(gu))
            mod.forward = types.MethodType(mlp_forward, mod)
            n["mlp"] += 1
        if linears and isinstance(mod, torch.nn.Linear) and mod.in_features % 64 == 0 and mod.out_features % 8 == 0:
            mod.forward = types.MethodType(lambda self, x: linear(x, self.weight, self.bias), mod)
            n["linear"] += 1
    return n
