"""LoRA for the decoder (TimeR1_Trainer's peft_config, reference timer1_trainer.py:264-293 / main.py get_peft_config): rank-r adapters kept MERGED.

For a targeted projection with frozen base weight W0 [out, in] the policy's weight is

    W = bf16_rne(W0 + s * Bt^T A),      A [r, in], Bt [r, out] (peft's lora_B stored transposed), s = lora_alpha / r (/ sqrt(r) with use_rslora)

and lives where the weight lives in full-parameter training (ModelParams.train.w16): every forward, the decode kernels, the fp8 rollout copies and the
exports read it without knowing about adapters.  The backward keeps the data gradient dX = dY W (the merged weight) and replaces the full-size weight
gradient by two rank-r products per target: with u = x A^T and v = dY Bt^T (ops.gemm_nt, N = r), dBt += s u^T dY and dA += s v^T x (ops.lora_wgrad).
The merge is recomputed from W0 and the fp32 adapter masters after every optimizer step (ops.lora_merge), never applied as a delta.  DESIGN.md section 7r.

The adapters live in one more params.Arena (one segment per decoder layer, fp32 master / grad, moments in fp32 or bf16), so AdamWFlat, the clipping norm, the
data-parallel exchange and the optimizer checkpoints serve them unchanged: `LoraAdapters.train` is that arena, which is all AdamWFlat asks of its `params`.
"""
import math

import torch

from .params import Arena

TARGET_MODULES = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")
RANKS = (8, 16, 32, 64)
_SHORT = {"q_proj": "q", "k_proj": "k", "v_proj": "v", "o_proj": "o", "gate_proj": "gate", "up_proj": "up", "down_proj": "down"}
_HF_PARENT = {"q_proj": "self_attn", "k_proj": "self_attn", "v_proj": "self_attn", "o_proj": "self_attn", "gate_proj": "mlp", "up_proj": "mlp", "down_proj": "mlp"}
ADAPTER_KEY = "base_model.model.model.language_model.layers.%d.%s.%s.lora_%s.weight"


def _field(cfg, name, default):
    if isinstance(cfg, dict):
        return cfg.get(name, default)
    return getattr(cfg, name, default)


class LoraSpec:
    """What the engine needs of a peft LoraConfig.  Built from any object or dict with peft's field names (peft itself is not imported)."""

    def __init__(self, r=8, lora_alpha=8, target_modules=None, lora_dropout=0.0, bias="none", use_rslora=False, use_dora=False, init_lora_weights=True):
        if isinstance(r, bool) or not isinstance(r, int) or r not in RANKS:
            raise ValueError("LoRA rank r must be one of %s, got %r" % (RANKS, r))
        if target_modules is None:
            raise ValueError("LoRA needs target_modules: a non-empty subset of %s, or \"all-linear\"" % (TARGET_MODULES,))
        if isinstance(target_modules, str):
            mods = TARGET_MODULES if target_modules == "all-linear" else (target_modules,)
        else:
            mods = tuple(target_modules)
            if "all-linear" in mods:
                mods = TARGET_MODULES if len(mods) == 1 else mods
        bad = [m for m in mods if m not in TARGET_MODULES]
        if bad or not mods:
            raise ValueError("LoRA target_modules must be a non-empty subset of %s or \"all-linear\" (decoder projections only; the vision tower is never "
                             "adapted), got %r" % (TARGET_MODULES, target_modules))
        if float(lora_dropout or 0.0) != 0.0:
            raise NotImplementedError("lora_dropout = %r: the merged-adapter design has no dropout (use 0)" % (lora_dropout,))
        if bias != "none":
            raise NotImplementedError("LoRA bias = %r: biases are frozen (use \"none\")" % (bias,))
        if use_dora:
            raise NotImplementedError("use_dora: DoRA is not implemented")
        if init_lora_weights not in (True, None):
            raise NotImplementedError("init_lora_weights = %r: only peft's default initialisation (A uniform, B zero) is implemented" % (init_lora_weights,))
        self.r, self.lora_alpha, self.use_rslora = int(r), float(lora_alpha), bool(use_rslora)
        self.targets = tuple(m for m in TARGET_MODULES if m in mods)          # canonical order, duplicates dropped
        self.r_store = max(self.r, 16)          # r = 8 is stored as 16 rows, rows 8..15 zero: their gradients are zero, so AdamW leaves them zero (exact)
        self.scale = self.lora_alpha / (math.sqrt(self.r) if self.use_rslora else self.r)

    @classmethod
    def from_config(cls, cfg):
        if isinstance(cfg, cls):
            return cfg
        pt = _field(cfg, "peft_type", None)
        if pt is not None and str(getattr(pt, "value", pt)).upper() != "LORA":
            raise NotImplementedError("peft_type %r: only LoRA is implemented" % (pt,))
        tm = _field(cfg, "target_modules", None)
        if isinstance(tm, (set, frozenset)):
            tm = sorted(tm)
        return cls(r=_field(cfg, "r", 8), lora_alpha=_field(cfg, "lora_alpha", 8), target_modules=tm, lora_dropout=_field(cfg, "lora_dropout", 0.0),
                   bias=_field(cfg, "bias", "none"), use_rslora=_field(cfg, "use_rslora", False), use_dora=_field(cfg, "use_dora", False),
                   init_lora_weights=_field(cfg, "init_lora_weights", True))

    def adapter_config(self, base_model_name_or_path=None):
        """adapter_config.json in peft's field names."""
        return dict(peft_type="LORA", task_type="CAUSAL_LM", r=self.r, lora_alpha=self.lora_alpha, target_modules=list(self.targets), lora_dropout=0.0, bias="none",
                    use_rslora=self.use_rslora, use_dora=False, init_lora_weights=True, fan_in_fan_out=False, inference_mode=True, modules_to_save=None,
                    base_model_name_or_path=base_model_name_or_path)


def check_backend(ops):
    missing = [n for n in ("lora_merge", "lora_wgrad") if not hasattr(ops, n)]
    if missing:
        raise NotImplementedError("peft_config (LoRA): the %s op backend has no %s" % (type(ops).__name__, " / ".join(missing)))


class LoraAdapters:
    """The adapters of one model: their arena (`train`), the frozen base copy W0 (`base`: also the reference policy), the merge and the gradient calls."""

    def __init__(self, params, spec: LoraSpec, seed=0, moment_dtype=torch.float32):
        check_backend(params.ops)
        self.params, self.ops, self.cfg, self.spec = params, params.ops, params.cfg, spec
        t = self.cfg.text
        rs = spec.r_store
        # (module, fused matrix, first row, rows = out, in) per target, in TARGET_MODULES order
        dims = {"q_proj": ("qkv", 0, t.q_dim, t.hidden), "k_proj": ("qkv", t.q_dim, t.kv_dim, t.hidden), "v_proj": ("qkv", t.q_dim + t.kv_dim, t.kv_dim, t.hidden),
                "o_proj": ("o", 0, t.hidden, t.q_dim), "gate_proj": ("gu", 0, t.intermediate, t.hidden), "up_proj": ("gu", t.intermediate, t.intermediate, t.hidden),
                "down_proj": ("down", 0, t.hidden, t.intermediate)}
        self.slices = [(m,) + dims[m] for m in spec.targets]
        self.by_matrix = {}
        for s in self.slices:
            self.by_matrix.setdefault(s[1], []).append(s)
        specs = []
        for i in range(t.n_layers):
            for m, _, _, out, in_ in self.slices:
                specs += [("l%d.%s.A" % (i, _SHORT[m]), (rs, in_)), ("l%d.%s.Bt" % (i, _SHORT[m]), (rs, out))]
        self.train = Arena(self.ops, specs, with_optimizer_state=True, moment_dtype=moment_dtype)
        self.base = params.train.clone_weights_only()      # W0, taken before the first merge
        self.init_adapters(seed)
        self.merge()                                       # Bt = 0: the merged weights equal W0

    def name(self, i, module, which):
        return "l%d.%s.%s" % (i, _SHORT[module], which)

    def init_adapters(self, seed):
        """peft's default: A ~ U(-1/sqrt(in), 1/sqrt(in)) (kaiming_uniform_(a = sqrt(5))), B = 0.  Drawn on the host by name from `seed`, so every rank of a
        data-parallel run holds the same adapters."""
        a = self.train
        g = torch.Generator().manual_seed(int(seed) + 0x10A4)
        a.master.zero_()
        r = self.spec.r
        for i in range(self.cfg.text.n_layers):
            for m, _, _, out, in_ in self.slices:
                bound = 1.0 / math.sqrt(in_)
                w = (torch.rand(r, in_, generator=g) * 2.0 - 1.0) * bound
                a.view(a.master, self.name(i, m, "A"))[:r].copy_(w)
        a.w16.copy_(a.master)

    def numel(self):
        """Trainable adapter parameters (unpadded)."""
        return self.cfg.text.n_layers * sum(self.spec.r * (out + in_) for _, _, _, out, in_ in self.slices)

    # ---------------------------------------------------------------------------------------------------------------- merge
    def merge(self, layers=None):
        """params.train.w16 <- bf16_rne(W0 + s Bt^T A) for every targeted matrix (of `layers`, default all), from the fp32 masters; bumps the arena's version
        so copies derived from the old weights (W^T caches, fp8 rollout weights) are rebuilt."""
        a, tr, base, s = self.train, self.params.train, self.base, self.spec.scale
        for i in (range(self.cfg.text.n_layers) if layers is None else layers):
            for m, mat, r0, out, _ in self.slices:
                key = "l%d.%s.w" % (i, mat)
                self.ops.lora_merge(tr.w(key)[r0:r0 + out], base.w(key)[r0:r0 + out], a.view(a.master, self.name(i, m, "A")), a.view(a.master, self.name(i, m, "Bt")), s)
        tr.version = getattr(tr, "version", 0) + 1

    # ---------------------------------------------------------------------------------------------------------------- gradients
    def wgrad(self, i, mat, dy, x):
        """The adapter gradients of the targets inside matrix `mat` ("qkv" | "o" | "gu" | "down") of layer i, where the full-parameter backward runs the weight
        gradient dW = dy^T x: dy [M, rows of the matrix], x [M, in].  Accumulates into the adapter arena's grad (AdamW zeroes it); main stream."""
        ops, a, s = self.ops, self.train, self.spec.scale
        for m, _, r0, out, _ in self.by_matrix.get(mat, ()):
            A16, Bt16 = a.w(self.name(i, m, "A")), a.w(self.name(i, m, "Bt"))
            dys = dy if (r0 == 0 and out == dy.shape[1]) else dy[:, r0:r0 + out]
            u = ops.gemm_nt(x, A16)                  # [M, r]
            v = ops.gemm_nt(dys, Bt16)               # [M, r]
            ops.lora_wgrad(a.g(self.name(i, m, "Bt")), u, dys, s, accumulate=True)
            ops.lora_wgrad(a.g(self.name(i, m, "A")), v, x, s, accumulate=True)

    # ---------------------------------------------------------------------------------------------------------------- export
    def export_adapter(self, base_model_name_or_path=None):
        """-> (tensors of adapter_model.safetensors, adapter_config.json dict) in peft's layout: lora_A.weight [r, in], lora_B.weight [out, r], fp32, the
        padding rows of r = 8 dropped."""
        a, r = self.train, self.spec.r
        sd = {}
        for i in range(self.cfg.text.n_layers):
            for m, _, _, _, _ in self.slices:
                sd[ADAPTER_KEY % (i, _HF_PARENT[m], m, "A")] = a.view(a.master, self.name(i, m, "A"))[:r].detach().float().cpu().contiguous().clone()
                sd[ADAPTER_KEY % (i, _HF_PARENT[m], m, "B")] = a.view(a.master, self.name(i, m, "Bt"))[:r].detach().float().cpu().t().contiguous().clone()
        return sd, self.spec.adapter_config(base_model_name_or_path)
