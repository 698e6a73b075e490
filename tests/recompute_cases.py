"""Cases and the micro-step harness for activation_recompute="mlp" (Engine.RECOMPUTED), shared by tests/test_recompute_ref.py (the oracle
op backend on the CPU) and tests/test_recompute_gpu.py (HipOps).

The property under test is equality by construction: the backward rebuilds xn / xn2 / gu / a with the forward's own launches over the forward's own row ranges,
so every gradient of the "mlp" run is the "none" run's bit for bit.  Nothing here has a tolerance.

Shapes (P prompt rows, G completions of C tokens, M = P + G C packed rows), each the smallest that takes its path:
  tail                P = 70, C = 24: 166 rows, P - 1 >= 0.4 M, so the last layer runs rows >= P - 1 only (a one-row prompt piece after a prefill + continuation)
  no-tail             P = 20, C = 24: 116 rows, every row runs the last layer
  short-continuation  P = 70, C = 12: the continuation's 48 rows sit below gemm_glu's 64-row switch while the whole sequence (118 rows) sits above it
"""
import torch

from time_r1_amd.config import tiny_test, tiny_test_25
from time_r1_amd.grpo import GRPOCore
from time_r1_amd.model import Engine
from time_r1_amd.params import ModelParams
from time_r1_amd.positions import PackedLayout
from time_r1_amd.synthetic import synthetic_prompt

I32 = torch.int32
SHAPES = {"tail": (70, 4, 24), "no-tail": (20, 4, 24), "short-continuation": (70, 4, 12)}
CONFIGS = {"qwen2_vl": tiny_test, "qwen2_5_vl": tiny_test_25}
RECOMPUTED = ("xn", "xn2", "gu", "a")


def prompt_for(cfg, P, grid=None):
    """A synthetic prompt of exactly P rows: text, <|vision_start|>, the video tokens of `grid` (patches), <|vision_end|>, text."""
    grid = grid or ((4, 6, 8) if P >= 60 else (2, 4, 4))
    rest = P - 2 - grid[0] * grid[1] * grid[2] // cfg.vision.merge_unit
    assert rest >= 2, (P, grid)
    ids, pix, g = synthetic_prompt(cfg, grid, rest // 2, rest - rest // 2, seed=2, text_vocab=400)
    assert len(ids) == P
    return ids, pix, g


def forced_inputs(G, C, seed=9):
    """Completions (the forced tokens both modes see), a ragged mask and advantages."""
    g = torch.Generator().manual_seed(seed)
    toks = torch.randint(2, 400, (G, C), generator=g).to(I32)
    lens = torch.randint(max(1, C // 2), C + 1, (G,), generator=g)
    lens[0] = C
    mask = (torch.arange(C)[None, :] < lens[:, None]).to(I32)
    adv = torch.randn(G, generator=g)
    return toks, mask, adv


def bits(t):
    t = t.detach().contiguous().cpu()
    return t.view(torch.int16) if t.element_size() == 2 else t.view(I32)


def build(ops, mode, variant="qwen2_vl", G=4, C=24, beta=0.0, fix_vit=True, reuse_prefill=True, entropy_coef=0.0, n_layers=2, through="core"):
    """-> (cfg, policy params, engine, core).  through: which constructor is handed the mode ("core": GRPOCore(activation_recompute=), "engine": Engine(...))."""
    cfg = CONFIGS[variant](n_layers=n_layers)
    pol = ModelParams(cfg, ops, seed=1, train_vit=not fix_vit)
    ref = ModelParams(cfg, ops, seed=2, optimizer_state=False, train_vit=not fix_vit).train if beta != 0.0 else None
    kw = {} if mode is None else {"activation_recompute": mode}
    eng = Engine(cfg, ops, pol, **(kw if through == "engine" else {}))
    core = GRPOCore(eng, ref, G, C, beta=beta, use_grpo=False, seed=3, rope_index_mode="hf4", reuse_prefill=reuse_prefill, entropy_coef=entropy_coef,
                    **(kw if through == "core" else {}))
    return cfg, pol, eng, core


def micro_steps(ops, shape, mode, variant="qwen2_vl", beta=0.0, fix_vit=True, reuse_prefill=True, replay=False, entropy_coef=0.0, steps=1, n_layers=2,
                through="core", on_ctx=None, grid=None, before_step=None, keep=None):
    """`steps` consecutive micro-steps (prepare -> [rollout] -> forward_logps -> loss_backward) on one engine, the completions forced; with replay, each is followed by
    one replayed update (forward_logps(replay=True) on moved weights, the ratio loss against the first pass's log-probs).
    reuse_prefill: the rollout runs (its prefill is the prompt half of the policy forward) and its tokens are then replaced by the forced ones; otherwise no
    rollout runs at all and the full-sequence path takes the update.
    before_step(eng): called right before each step's forward_logps; on_ctx(eng, st): right after every forward_logps; keep: a dict that receives the engine.
    -> list of dict(grad, out, row_len, logp[, replay_grad, replay_out]) per step, everything on the host."""
    P, G, C = shape
    cfg, pol, eng, core = build(ops, mode, variant, G, C, beta, fix_vit, reuse_prefill, entropy_coef, n_layers, through)
    if keep is not None:
        keep["eng"] = eng
    tr = pol.train
    ids, pix, g3 = prompt_for(cfg, P, grid)
    res = []
    for step in range(steps):
        toks, mask, adv = forced_inputs(G, C, seed=9 + step)
        st = core.prepare(ids, pix, g3)
        if reuse_prefill:
            core.rollout(st)
        else:
            st.layout = PackedLayout(st.P, G, C)
        st.completion_ids = ops.tensor(toks.numpy(), I32)
        if before_step is not None:
            before_step(eng)
        core.forward_logps(st)
        if on_ctx is not None:
            on_ctx(eng, st)
        old = st.logp.clone()
        tr.grad.zero_()
        mask_d, adv_d = ops.tensor(mask.numpy(), I32), ops.tensor(adv.numpy(), torch.float32)
        out, row_len = core.loss_backward(st, mask_d, adv_d, 0.5, keep_pixels=replay)
        r = dict(grad=tr.grad.detach().clone().cpu(), out=out.detach().clone().cpu(), row_len=row_len.detach().clone().cpu(), logp=old.detach().clone().cpu())
        if replay:
            tr.w16.copy_((tr.w16.float() * 1.01).to(tr.w16.dtype))         # the weights have moved, as after an optimizer step (the same move in both modes)
            core.forward_logps(st, replay=True)
            if on_ctx is not None:
                on_ctx(eng, st)
            tr.grad.zero_()
            out, _ = core.loss_backward(st, mask_d, adv_d, 0.5, old_logp=old, eps=(0.2, 0.28))
            r.update(replay_grad=tr.grad.detach().clone().cpu(), replay_out=out.detach().clone().cpu())
        res.append(r)
    return res


def assert_equal_runs(a, b, what):
    """Every recorded tensor of two runs, bit for bit."""
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert set(x) == set(y)
        assert float(x["grad"].abs().max()) > 0, (what, "the step must have a gradient")
        for k in x:
            assert x[k].shape == y[k].shape and torch.equal(bits(x[k]), bits(y[k])), (what, "step %d" % i, k, float((x[k].float() - y[k].float()).abs().max()))


class Spy:
    """Wraps an op backend: records (name, row count of the first tensor argument) of every op call, in order."""

    def __init__(self, ops):
        object.__setattr__(self, "_ops", ops)
        object.__setattr__(self, "calls", [])

    def __getattr__(self, name):
        v = getattr(self._ops, name)
        if not callable(v) or name.startswith("_") or name in ("empty", "zeros", "tensor"):
            return v

        def f(*a, **k):
            rows = next((int(x.shape[0]) for x in a if torch.is_tensor(x) and x.dim() >= 1), None)
            self.calls.append((name, rows))
            return v(*a, **k)
        return f

    def __setattr__(self, name, value):
        setattr(self._ops, name, value)
