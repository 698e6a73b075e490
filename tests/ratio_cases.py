"""Cases and fp64 reference for the GRPO loss against an OLD policy (tr1_grpo_loss_ratio, csrc/loss.hip; its fp32 CPU stand-in is
oracle.ref_ops.RefOps.grpo_loss_ratio), and the tiny-trainer scenario for several updates per rollout (GRPOConfig.num_iterations).  Shared by tests/test_policy_reuse_ref.py (CPU) and
tests/test_policy_reuse_gpu.py (the HIP kernel and the HIP trainer on the same cases).

The loss, per live token (mask != 0), with rho = exp(logp - old_logp), kl = exp(ref - logp) - (ref - logp) - 1, w = tok_weight or 1 (a constant):
  use_grpo : l = -(w rho A - beta kl),                                         loss = mean_g( sum_t l m / sum_t m )
  clip     : l = -w min(rho A, clamp(rho, 1 - eps_low, 1 + eps_high) A) + beta kl,  loss = sum l m / sum m
The reference below is that text in fp64, differentiated by autograd (it extends vocab_cases.ref_grpo, which fixes rho = 1).

The clip decision is a step function of rho, so a token within 1e-3 of a clip boundary is MOVED (old_logp shifted by 0.01), never left out: every
token of every case is compared.  Masked positions hold old_logp = -300 against logp = -80: the ratio there is inf in fp32, and no output may see it.
"""
import torch

import vocab_cases as vc

EPS_PAIRS = ((0.2, 0.2), (0.2, 0.28))
MAX_DELTA = 0.6
NEAR = 1e-3


def _near_boundary(logp, old, live, eps):
    rho = torch.exp(logp.double() - old.double())
    return live & (((rho - (1 - eps[0])).abs() < NEAR) | ((rho - (1 + eps[1])).abs() < NEAR))


def ratio_case(G, C, eps, seed=0):
    """-> dict(logp, old_logp, ref_logp, tok_weight fp32 [G, C], mask int32 [G, C], adv fp32 [G], moved = number of tokens shifted off a clip boundary).
    logp / ref_logp / mask / adv are vocab_cases.grpo_case's; logp - old_logp is uniform in +-0.6 with ~10 % exact zeros; tok_weight uniform in [0, 2]."""
    logp, ref, mask, adv = vc.grpo_case(G, C, seed)
    g = torch.Generator().manual_seed(9001 + seed + 131 * G + C)
    delta = (torch.rand(G, C, generator=g) * 2 - 1) * MAX_DELTA
    delta[torch.rand(G, C, generator=g) < 0.1] = 0.0
    live = mask.bool()
    old = logp - delta
    old[delta == 0] = logp[delta == 0]
    near = _near_boundary(logp, old, live, eps)
    moved = int(near.sum())
    old = torch.where(near, old - 0.01, old)                 # rho grows by ~1 %: ten times the exclusion width away from the boundary it sat on
    assert not _near_boundary(logp, old, live, eps).any()
    old = torch.where(live, old, torch.full_like(old, -300.0))
    tokw = torch.rand(G, C, generator=g) * 2
    return dict(logp=logp, old_logp=old, ref_logp=ref, tok_weight=tokw, mask=mask, adv=adv, moved=moved)


def ref_grpo_ratio(logp, old_logp, ref_logp, tok_weight, mask, adv, beta, use_grpo, eps_low, eps_high, grad_scale):
    """fp64 + autograd -> (dlogp = grad_scale * d loss / d logp, out8, row_len, row_kl).  out8 = [loss, mean_g masked-mean kl, sum mask, low / high / either
    clip fraction (clip_ratio_metrics: flag * mask summed over sum mask), masked mean of rho - 1 - log rho, largest rho over the live tokens]."""
    lp = logp.double().clone().requires_grad_(True)
    live = mask.bool()
    m = mask.double()
    A = adv.double()[:, None]
    zero = torch.zeros_like(lp)
    d = torch.where(live, lp - old_logp.double(), zero)      # selection: a masked position holds anything
    rho = torch.exp(d)
    kl = torch.zeros_like(lp)
    if ref_logp is not None:
        r = torch.where(live, ref_logp.double() - lp, zero)
        kl = torch.exp(r) - r - 1
    w = tok_weight.double() if tok_weight is not None else torch.ones_like(lp)
    if use_grpo:
        per_tok = -(w * rho * A - beta * kl) if beta != 0.0 else -(w * rho * A)
        loss = ((per_tok * m).sum(1) / m.sum(1)).mean()
    else:
        per_tok = -w * torch.min(rho * A, torch.clamp(rho, 1 - eps_low, 1 + eps_high) * A)
        if beta != 0.0:
            per_tok = per_tok + beta * kl
        loss = (per_tok * m).sum() / m.sum()
    (grad,) = torch.autograd.grad(loss, lp)
    rho, kl, d = rho.detach(), kl.detach(), d.detach()
    lens, tot = m.sum(1), m.sum()
    is_low = (rho < 1 - eps_low) & (A < 0)
    is_high = (rho > 1 + eps_high) & (A > 0)
    out8 = torch.stack([loss.detach(), ((kl * m).sum(1) / lens).mean(), tot, (is_low * m).sum() / tot, (is_high * m).sum() / tot,
                        ((is_low | is_high) * m).sum() / tot, ((rho - 1 - d) * m).sum() / tot, rho[live].max()])
    return grad * grad_scale, out8, lens, (kl * m).sum(1)


# ------------------------------------------------------------------------------------------------------ several updates per rollout: the tiny trainer
def varied_reward(prompts, completions, **kw):
    """A reward that differs inside a group (the tiny random model never writes a well-formed answer, so the project's rewards are all zero there)."""
    return [float(sum(map(ord, c)) % 7) / 6.0 for c in completions]


def tiny_trainer(ops, fx, out_dir, mu, ga=2, epochs=1, save_steps=0, n_rows=4, **over):
    from helpers import golden_params
    from oracle.text import FakeProcessor
    from time_r1_amd.trainer import TimeR1_Trainer, GRPOConfig
    cfg, pol, ref = golden_params(ops, fx)
    args = GRPOConfig(output_dir=str(out_dir), num_generations=fx["G"], max_completion_length=fx["C"], beta=fx["beta"], use_grpo=fx["use_grpo"],
                      rope_index_mode="hf5", gradient_accumulation_steps=ga, temperature=1.0, logging_steps=1, num_iterations=mu, num_train_epochs=epochs,
                      save_strategy="steps" if save_steps else "no", save_steps=save_steps or 500, learning_rate=1e-4, disable_log_print=True, **over)
    tr = TimeR1_Trainer(pol, [varied_reward], [], args=args, processing_class=FakeProcessor(cfg), ops=ops)
    if fx["beta"] != 0:
        tr.ref_model.w16.copy_(ref.relayout(tr.params.train_vit).train.w16.to(tr.ref_model.w16.device))
    rows = []
    for i in range(n_rows):
        r = dict(fx["row"])
        r["problem"] = "event %d" % i
        r["video_frames"] = torch.randint(0, 256, (4, 3, 56, 84), generator=torch.Generator().manual_seed(100 + i), dtype=torch.uint8).float()
        rows.append(r)
    tr.train_dataset = rows
    return tr


def run_recorded(tr, ckpt=None):
    """train() with spies -> dict(masters after every optimizer step, rollouts, reference-policy head forwards, the log-probs each loss call saw, generated
    tokens at every log)."""
    rec = dict(masters=[], rollouts=0, ref_forwards=0, first_logp=[], replay_old=[], tokens_at_log=[])
    core, eng = tr.core, tr.engine
    o_many, o_one, o_head, o_lb = core.rollout_many, core.rollout, eng.head_fwd, core.loss_backward

    def many(states):
        rec["rollouts"] += 1
        return o_many(states)

    def one(st):
        rec["rollouts"] += 1
        return o_one(st)

    def head(arena, *a, **k):
        rec["ref_forwards"] += int(arena is tr.ref_model)
        return o_head(arena, *a, **k)

    def lb(st, *a, **k):
        if k.get("old_logp") is None:
            rec["first_logp"].append(st.logp.detach().clone().cpu())
        else:
            rec["replay_old"].append(k["old_logp"].detach().clone().cpu())
        return o_lb(st, *a, **k)
    core.rollout_many, core.rollout, eng.head_fwd, core.loss_backward = many, one, head, lb

    class CB:
        def on_step_end(self, args, state, control, **kw):
            rec["masters"].append(tr.params.train.master.detach().clone().cpu())

        def on_log(self, args, state, control, logs=None, **kw):
            rec["tokens_at_log"].append(tr.generated_tokens)
    tr.callbacks = [CB()]
    tr.train(resume_from_checkpoint=ckpt)
    return rec


ROLLOUT_KEYS = ("reward", "reward_std", "completion_length", "rollout_logp_drift")
REPLAY_KEYS = ("clip_ratio/low_mean", "clip_ratio/low_min", "clip_ratio/high_mean", "clip_ratio/high_max", "clip_ratio/region_mean", "policy_kl_old")


def check_reuse_scenario(ops, tmp_path, atol_step1, **over):
    """GA = 2, 4 rows, one epoch: mu = 2 makes 2 rollouts and 4 optimizer steps; mu = 1 on the same rows makes 2.  Returns the mu = 2 trainer and record."""
    import math
    from helpers import load_case
    fx = load_case("clip_beta")
    tr2 = tiny_trainer(ops, fx, tmp_path / "mu2", mu=2, save_steps=2, **over)
    r2 = run_recorded(tr2)
    tr1 = tiny_trainer(ops, fx, tmp_path / "mu1", mu=1, **over)
    r1 = run_recorded(tr1)
    assert tr2.state.global_step == 4 and tr2.state.max_steps == 4 and abs(tr2.state.epoch - 1.0) < 1e-9
    assert tr1.state.global_step == 2
    assert r2["rollouts"] == 2 and r1["rollouts"] == 2                      # one batched rollout per loader window, whatever mu
    # one reference-policy forward per micro-step of a FIRST pass (2 windows x GA 2 = 4, the count of the mu = 1 run on the same rows); the 4 replayed
    # micro-steps add none - with a reference forward in every replay it would be 8
    assert r2["ref_forwards"] == 4 and r1["ref_forwards"] == 4
    assert len(r2["masters"]) == 4 and len(r1["masters"]) == 2
    # old policy: what each replay was handed is what the first pass of the same micro-step computed
    assert len(r2["first_logp"]) == 4 and len(r2["replay_old"]) == 4
    for w in range(2):
        for i in range(2):
            assert torch.equal(r2["replay_old"][2 * w + i], r2["first_logp"][2 * w + i])
    assert not r1["replay_old"]
    # tokens are counted once per rollout
    assert r2["tokens_at_log"][1] == r2["tokens_at_log"][0] > 0 and r2["tokens_at_log"][3] == r2["tokens_at_log"][2] > r2["tokens_at_log"][1]
    assert r2["tokens_at_log"][0] == r1["tokens_at_log"][0]
    logs2, logs1 = tr2.state.log_history, tr1.state.log_history
    assert len(logs2) == 4 and len(logs1) == 2
    for step in (1, 3):             # replay steps
        for k in REPLAY_KEYS + ("loss", "kl", "generation_entropy", "grad_norm"):
            assert k in logs2[step] and math.isfinite(logs2[step][k]), (step, k, logs2[step].get(k))
        assert not [k for k in logs2[step] if k in ROLLOUT_KEYS or k.startswith("rewards/") or k.startswith("metrics/") or k == "rollout_tokens_per_sec"], logs2[step]
        assert logs2[step]["grad_norm"] > 0
    metric_keys = lambda l: {k for k in l if not k.startswith("perf/") and k not in ("samples_per_sec", "rollout_tokens_per_sec")}
    assert metric_keys(logs2[0]) == metric_keys(logs1[0]) == metric_keys(logs1[1])
    assert not [k for k in logs1[0] if k in REPLAY_KEYS]
    # step 1 is the code that runs at mu = 1, at the same learning rate (the schedule starts at the base rate whatever its horizon)
    a, b = r2["masters"][0], r1["masters"][0]
    assert torch.allclose(a, b, atol=atol_step1, rtol=0), float((a - b).abs().max())
    a, b = r2["masters"][1], r1["masters"][1]
    assert float((a - b).abs().max()) > 1e-6, "the second step of mu = 2 replays window 1; at mu = 1 it trains on window 2"
    return fx, tr2, r2


def check_resume(ops, tmp_path, fx, tr2, atol, **over):
    """checkpoint-2 of the 4-step mu = 2 run (written after the first rollout's LAST update), resumed in a fresh trainer: skips window 1, reaches step 4 on the same weights."""
    import json
    import os
    d = tmp_path / "mu2" / "checkpoint-2"
    assert os.path.exists(d / "model.safetensors") and not os.path.exists(tmp_path / "mu2" / "checkpoint-1") and not os.path.exists(tmp_path / "mu2" / "checkpoint-3")
    assert json.load(open(d / "trainer_state.json"))["global_step"] == 2
    tr = tiny_trainer(ops, fx, tmp_path / "resumed", mu=2, **over)
    rec = run_recorded(tr, ckpt=str(d))
    assert tr.state.global_step == 4 and rec["rollouts"] == 1 and len(rec["masters"]) == 2
    a, b = tr.params.train.master.cpu(), tr2.params.train.master.cpu()
    assert torch.allclose(a, b, atol=atol, rtol=0), float((a - b).abs().max())


def first_pass_and_replay_grads(ops, out_dir, fix_vit=True):
    """One micro-step, then its replay on UNCHANGED weights: rho = 1 everywhere, so the replay path (merger / tower re-run on the kept features / pixels,
    full-sequence decoder forward in place of prefill + continuation, ratio kernel, backward) must reproduce the first pass's gradient.
    -> (first-pass gradient, replay gradient, the replay's metrics)."""
    from helpers import load_case
    tr = tiny_trainer(ops, load_case("clip_beta"), out_dir, mu=2, ga=1, n_rows=1, fix_vit=fix_vit)
    tr._reuse = []
    tr.accumulation_window([[tr.train_dataset[0]]])
    recs, tr._reuse = tr._reuse, None
    g = tr.params.train.grad
    g1 = g.detach().clone().cpu()
    g.zero_()
    tr._replay_window(recs, more=False)
    g2 = g.detach().clone().cpu()
    assert recs[0]["st"].pixels is None          # dropped after the last replay (kept until then only when the tower trains)
    return g1, g2, {k: v[-1] for k, v in tr.flush_metrics().items()}
