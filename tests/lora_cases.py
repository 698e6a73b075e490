"""Cases and references for LoRA (time-r1_amd/lora.py, csrc/lora.hip; the CPU stand-ins are RefOps.lora_merge / lora_wgrad).
Shared by tests/test_lora_ref.py (CPU) and tests/test_lora_gpu.py (the HIP kernels and the HIP trainer on the same cases).

The merge, per element of a targeted matrix, with s = fp32(scale):

    acc = 0;  for j ascending: acc = fadd(acc, fmul(Bt[j, o], A[j, i]));   W[o, i] = bf16_rne(fadd(W0[o, i], fmul(s, acc)))

`merge_composite` (oracle.ref_ops) is that text in torch, one fp32 op at a time: the kernel must match it bit for bit.  `merge64` is the fp64 value.

What the composite may differ from RNE(fp64 value) by: the r products round once each (2^-24 |p_j|), the r - 1 non-trivial additions of the chain round once each
(at most 2^-24 sum |p|), s * acc rounds once and the last addition once - together at most 2^-24 ((r + 1) |s| sum_j |p_j| + |y|) <= (r + 3) 2^-24 c |y| with
c = (|w0| + |s| sum_j |Bt A|) / |y| the cancellation of the element.  Only a value within that relative distance of a bf16 tie may round the other way.

The rank-r weight gradient G = scale * thin^T wide sums M exact products of bf16 pairs (16 significant bits: exact in fp32) in some order: at most M - 1 roundings
of partial sums, one for the scale, one for the accumulation into G - (M + 2) 2^-23 scale sum_m |thin wide| per element covers any order and an accumulator
that truncates (2^-23 per step) instead of rounding to nearest.
"""
import math

import torch

import optim_cases as oc
from oracle.ref_ops import merge_acc, merge_composite  # noqa: F401  (the kernel's contract; RefOps.lora_merge is built from them)

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64

MERGE_SHAPES = ((8, 8), (24, 72), (64, 128), (130, 264))           # (out, in): one thread's chunk, a partial tile, exactly one tile, more than one block both ways
MERGE_RANKS = (16, 32, 64)
MERGE_SCALES = (0.0, 0.25, 2.0, 0.25 * math.sqrt(2.0))
WGRAD_WIDTHS = (8, 136, 264)
WGRAD_RANKS = (16, 32, 64)
WGRAD_SCALES = (1.0, 2.0, 0.17)


def f32(x):
    return oc.f32(x)


# ---------------------------------------------------------------------------------------------------------------------- merge
MAX_CANCELLATION = 64.0


def merge_data(out, in_, r, seed=0, big=False):
    """-> (W0 bf16 [out, in], A fp32 [r, in], Bt fp32 [r, out]).  W0 ~ N(0, 0.02) as the synthetic weights, A as peft draws it, Bt ~ N(0, 0.02) (big: 0.5, the
    adapter term then dominates the sum, which is where a fused multiply-add shows).  An element that would cancel beyond MAX_CANCELLATION at one of
    MERGE_SCALES gets a base weight of the adapter term's sign and at least a quarter of sum_j |Bt A| (then c <= 1 + 4 s <= 9 at every scale) - under unbounded
    cancellation no fixed number of bf16 ulps holds for any fp32 formula, as in ref_sync_cases.  With c <= 64 the fp32 chain is off by at most
    67 * 64 * 2^-24 = 2.6e-4 relative, below a quarter of a bf16 ulp."""
    g = torch.Generator().manual_seed(7000 + 131 * out + in_ + 17 * r + seed)
    w0 = (torch.randn(out, in_, generator=g) * 0.02).to(BF16)
    a = ((torch.rand(r, in_, generator=g) * 2 - 1) / math.sqrt(in_)).to(F32)
    bt = (torch.randn(r, out, generator=g) * (0.5 if big else 0.02)).to(F32)
    p = torch.einsum("jo,ji->oji", bt.double(), a.double())
    d, dabs = p.sum(1), p.abs().sum(1)
    bad = torch.zeros_like(d, dtype=torch.bool)
    for s in MERGE_SCALES:
        sf = float(f32(s))
        bad |= (w0.double().abs() + sf * dabs) > MAX_CANCELLATION * (w0.double() + sf * d).abs()
    fixed = torch.copysign(torch.maximum(w0.double().abs(), 0.25 * dabs), d).to(BF16)
    return torch.where(bad, fixed, w0), a, bt


def merge_fused_variant(w0, a, bt, s):
    """What a kernel computes whose compiler contracted each step into a fused multiply-add: acc = fma(Bt, A, acc), y = fma(s, acc, w0).  A product of two fp32
    values is exact in fp64 and its sum with an fp32 value is there to far below an fp32 rounding, so rounding the fp64 result once to fp32 is the fma."""
    acc = torch.zeros(bt.shape[1], a.shape[1], dtype=F32)
    for j in range(a.shape[0]):
        acc = (acc.double() + bt[j].double()[:, None] * a[j].double()[None, :]).to(F32)
    return (w0.double() + float(f32(s)) * acc.double()).to(F32).to(w0.dtype)


def merge64(w0, a, bt, s):
    """-> (fp64 value, cancellation c per element)."""
    p = torch.einsum("jo,ji->oji", bt.double(), a.double())          # [out, r, in]
    y = w0.double() + float(f32(s)) * p.sum(1)
    mag = w0.double().abs() + abs(float(f32(s))) * p.abs().sum(1)
    c = torch.where(y != 0, mag / y.abs().clamp(min=1e-300), torch.ones_like(y))
    return y, c


MERGE_DATA = ((False, 0), (True, 0), (True, 1))          # (big, seed) of every data set the kernel is run on per (shape, rank)


def merge_cases():
    for out, in_ in MERGE_SHAPES:
        for r in MERGE_RANKS:
            for s in MERGE_SCALES:
                yield out, in_, r, s


# ---------------------------------------------------------------------------------------------------------------------- rank-r weight gradient
def wgrad_data(M, Wd, r, scale=1.0, seed=0):
    """-> (thin bf16 [M, r], wide bf16 [M, Wd], G0 fp32 [r, Wd]): values of mixed magnitude and sign.  G0, the value accumulated onto, is what an earlier call of
    the same kind leaves: at most half of scale sum_m |thin wide| per element, either sign - so |G0 + result| <= 1.5 of that sum and the one rounding of the
    accumulation is inside the (M + 2) of the bound."""
    g = torch.Generator().manual_seed(9000 + 7 * M + 3 * Wd + r + seed)
    thin = (torch.randn(M, r, generator=g) * torch.pow(2.0, torch.randint(-3, 3, (M, 1), generator=g).float())).to(BF16)
    wide = (torch.randn(M, Wd, generator=g) * torch.pow(2.0, torch.randint(-4, 2, (M, 1), generator=g).float())).to(BF16)
    mag = float(f32(scale)) * (thin.double().abs().t() @ wide.double().abs())
    g0 = (0.5 * mag * torch.rand(r, Wd, generator=g).double() * (torch.randint(0, 2, (r, Wd), generator=g).double() * 2 - 1)).to(F32)
    return thin, wide, g0


def wgrad64(thin, wide, scale, g0=None):
    """-> (fp64 result, the bound (M + 2) 2^-23 scale sum_m |thin wide| per element)."""
    t, w = thin.double(), wide.double()
    sc_ = float(f32(scale))
    prod = sc_ * (t.t() @ w)
    bound = (thin.shape[0] + 2) * 2.0 ** -23 * sc_ * (t.abs().t() @ w.abs())
    if g0 is not None:
        prod = prod + g0.double()
    return prod, bound


# ---------------------------------------------------------------------------------------------------------------------- engine: adapter gradients against fp64 autograd
class UnmergedWeight:
    """Stands in for a fused weight matrix in oracle.ref_model's `x @ W[name].t()`: the UNMERGED form x W0^T + s (x A^T) B per adapted row slice
    (parts = [(first row, rows, A [r, in], Bt [r, rows])]), differentiable in A and Bt."""

    def __init__(self, w0, parts, s):
        self.w0, self.parts, self.s = w0, parts, s

    def t(self):
        return self

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        x, me = args
        assert func in (torch.Tensor.matmul, torch.matmul, torch.Tensor.__matmul__), func
        y = x @ me.w0.t()
        pieces, pos = [], 0
        for r0, rows, a, bt in sorted(me.parts, key=lambda p: p[0]):
            if r0 > pos:
                pieces.append(torch.zeros(*x.shape[:-1], r0 - pos, dtype=y.dtype))
            pieces.append(me.s * ((x @ a.t()) @ bt))
            pos = r0 + rows
        if pos < me.w0.shape[0]:
            pieces.append(torch.zeros(*x.shape[:-1], me.w0.shape[0] - pos, dtype=y.dtype))
        return y + torch.cat(pieces, -1)


def engine_adapter_grads(ops, targets, r, recompute, reuse_prefill, variant="qwen2_vl", shape=(70, 4, 24), beta=0.04, scale_alpha=32, grad_scale=0.5, seed=5):
    """One micro-step of the LoRA engine (prepare -> [rollout] -> forward_logps -> loss_backward, the completions forced) with Bt set to random values (with
    peft's Bt = 0 every dA is identically zero).  -> (adapters, {arena name: (engine gradient, fp64 autograd gradient of the unmerged form)})."""
    import recompute_cases as rcc
    from oracle import ref_model as RM
    from time_r1_amd.grpo import GRPOCore
    from time_r1_amd.lora import LoraAdapters, LoraSpec
    from time_r1_amd.model import Engine
    from time_r1_amd.params import ModelParams
    from time_r1_amd.positions import PackedLayout
    P, G, C = shape
    cfg = rcc.CONFIGS[variant]()
    pol = ModelParams(cfg, ops, seed=1, optimizer_state=False, with_grad=False)
    spec = LoraSpec(r=r, lora_alpha=scale_alpha, target_modules=targets)
    eng = Engine(cfg, ops, pol, activation_recompute=recompute)
    lora = eng.lora = LoraAdapters(pol, spec, seed=3)
    a = lora.train
    g = torch.Generator().manual_seed(seed)
    for i in range(cfg.text.n_layers):
        for m, _, _, out, _ in lora.slices:
            bt = a.view(a.master, lora.name(i, m, "Bt"))
            bt[:r].copy_(torch.randn(r, out, generator=g) * 0.05)
    a.w16.copy_(a.master)
    lora.merge()
    core = GRPOCore(eng, lora.base, G, C, beta=beta, use_grpo=False, seed=3, rope_index_mode="hf4", reuse_prefill=reuse_prefill)
    ids, pix, g3 = rcc.prompt_for(cfg, P)
    toks, mask, adv = rcc.forced_inputs(G, C)
    st = core.prepare(ids, pix, g3)
    if reuse_prefill:
        core.rollout(st)
    else:
        st.layout = PackedLayout(st.P, G, C)
    st.completion_ids = ops.tensor(toks.numpy(), torch.int32)
    core.forward_logps(st)
    a.grad.zero_()
    core.loss_backward(st, ops.tensor(mask.numpy(), torch.int32), ops.tensor(adv.numpy(), F32), grad_scale)
    # ---- the same loss in fp64 on the unmerged form, autograd through oracle/ref_model.py
    W = {}
    for arena in (lora.base, pol.frozen):
        for name in arena.names():
            W[name] = arena.w(name).detach().cpu().double().clone()
    Wref = dict(W)
    leaves = {}
    t = cfg.text
    for i in range(t.n_layers):
        for mat, parts in lora.by_matrix.items():
            ps = []
            for m, _, r0, out, _ in parts:
                A = a.view(a.master, lora.name(i, m, "A")).detach().cpu().double().clone().requires_grad_(True)
                Bt = a.view(a.master, lora.name(i, m, "Bt")).detach().cpu().double().clone().requires_grad_(True)
                leaves[lora.name(i, m, "A")], leaves[lora.name(i, m, "Bt")] = A, Bt
                ps.append((r0, out, A, Bt))
            key = "l%d.%s.w" % (i, mat)
            W[key] = UnmergedWeight(W[key], ps, spec.scale)
    full = torch.cat([torch.as_tensor(ids)[None].repeat(G, 1), toks.long()], 1)
    pix64 = torch.as_tensor(pix).double()

    def logps(Wx):
        vid = RM.vision_tower(Wx, cfg, pix64, g3)
        lp, _ = RM.per_token_logps(RM.llm_logits(Wx, cfg, full, vid, g3, "hf4"), full)
        return lp[:, P - 1:]
    logp = logps(W)
    m64, A64 = mask.double(), adv.double()[:, None]
    ratio = torch.exp(logp - logp.detach())
    l = -torch.min(ratio * A64, torch.clamp(ratio, 0.8, 1.2) * A64)
    if beta != 0.0:
        with torch.no_grad():
            ref_logp = logps(Wref)
        l = l + beta * (torch.exp(ref_logp - logp) - (ref_logp - logp) - 1)
    loss = grad_scale * (l * m64).sum() / m64.sum()
    loss.backward()
    return lora, {n: (a.g(n).detach().cpu().clone(), leaf.grad) for n, leaf in leaves.items()}


# ---------------------------------------------------------------------------------------------------------------------- the tiny trainer
def tiny_lora_trainer(ops, fx, out_dir, peft, mu=1, ga=1, n_rows=3, save_steps=0, cls=None, pol=None, **over):
    """ratio_cases.tiny_trainer with a peft_config (None: the full-parameter trainer on the same rows).  The reference policy is left as the trainer made it:
    under LoRA it is the base copy the merge reads."""
    from helpers import golden_params
    from oracle.text import FakeProcessor
    from ratio_cases import varied_reward
    from time_r1_amd.trainer import TimeR1_Trainer, GRPOConfig
    cfg, pol0, _ = golden_params(ops, fx)
    pol = pol if pol is not None else pol0          # pol: the caller's ModelParams (e.g. weights shared between two backends)
    over = {**dict(beta=fx["beta"], learning_rate=1e-3), **over}
    args = GRPOConfig(output_dir=str(out_dir), num_generations=fx["G"], max_completion_length=fx["C"], use_grpo=fx["use_grpo"], rope_index_mode="hf5",
                      gradient_accumulation_steps=ga, temperature=1.0, logging_steps=1, num_iterations=mu, num_train_epochs=1,
                      save_strategy="steps" if save_steps else "no", save_steps=save_steps or 500, disable_log_print=True, **over)
    tr = (cls or TimeR1_Trainer)(pol, [varied_reward], [], args=args, processing_class=FakeProcessor(cfg), ops=ops, peft_config=peft)
    rows = []
    for i in range(n_rows):
        r = dict(fx["row"])
        r["problem"] = "event %d" % i
        r["video_frames"] = torch.randint(0, 256, (4, 3, 56, 84), generator=torch.Generator().manual_seed(100 + i), dtype=torch.uint8).float()
        rows.append(r)
    tr.train_dataset = rows
    return tr


ALL_LINEAR = dict(r=16, lora_alpha=32, target_modules="all-linear")
QV = dict(r=8, lora_alpha=16, target_modules=["q_proj", "v_proj"])


def run_snapshots(tr, ckpt=None, callbacks=()):
    """train() -> per optimizer step (on_step_end): merged weights, base copy, adapter masters as CPU clones; plus the step-0 log-probs of the first micro-step."""
    snaps, first = [], {}
    o_lb = tr.core.loss_backward

    def lb(st, *a, **k):
        if "logp" not in first:
            first.update(logp=st.logp.detach().clone().cpu(), ref_logp=None if st.ref_logp is None else st.ref_logp.detach().clone().cpu())
        return o_lb(st, *a, **k)
    tr.core.loss_backward = lb

    class CB:
        def on_step_end(self, args, state, control, **kw):
            s = dict(step=state.global_step, w=tr.params.train.w16.detach().clone().cpu())
            if tr.lora is not None:
                s.update(base=tr.lora.base.w16.detach().clone().cpu(), master=tr.lora.train.master.detach().clone().cpu())
            snaps.append(s)
    tr.callbacks = [CB()] + list(callbacks)
    tr.train(resume_from_checkpoint=ckpt)
    return snaps, first


def targeted_mask(tr):
    """Boolean mask over params.train.w16: True on the rows of the targeted projections of every layer."""
    a = tr.params.train
    mask = torch.zeros(a.numel, dtype=torch.bool)
    for i in range(tr.cfg.text.n_layers):
        for _, mat, r0, out, in_ in tr.lora.slices:
            off, shape = a.offsets["l%d.%s.w" % (i, mat)]
            mask[off + r0 * in_: off + (r0 + out) * in_] = True
    return mask
