"""Cases and fp64 references for the two entropy options of the GRPO objective (GRPOConfig.entropy_coef, GRPOConfig.top_entropy_quantile):
tr1_logp_entropy_bwd and tr1_entropy_quantile_weight (csrc/loss.hip; the fp32 CPU stand-ins are RefOps' methods of the same names).  Shared by
tests/test_entropy_objective_ref.py (CPU) and tests/test_entropy_objective_gpu.py (the HIP kernels, the head, GRPOCore and the trainer on the same cases).

  H = -sum_v p log p,  d H / d x_v = -p_v (log p_v + H)
  dlogits[r, v] = dlogp[r] (1[v == t_r] - p) - dent[r] p ((x - lse[r]) + H[r]),   p = exp(x - lse[r])
  top_entropy_quantile = rho: thr = quantile of order 1 - rho of the live entropies (torch.quantile, linear interpolation), weight = live and H >= thr
"""
import torch

import vocab_cases as vc

RHOS = (0.2, 0.5, 0.8, 1.0)
QUANTILE_SHAPES = ((1, 1), (1, 7), (8, 200), (3, 257), (16, 1024))
NEAR_THR = 1e-6             # a live token this close to the fp64 threshold, and not equal to it, may fall on either side ...
MAX_LEFT_OUT = 2            # ... at most this many per case
TOL_THR = 1e-5


def ref_dlogits_ent(logits, targets, dlogp, dent, stats=None):
    """fp64 dlogits with a gradient at the entropy; `stats` = vc.ref_stats(logits, targets) if already known."""
    _, H, lse = vc.ref_stats(logits, targets) if stats is None else stats
    d = vc.ref_dlogits(logits, targets, dlogp, lse)
    lp = logits.double() - lse[:, None]
    d -= dent.double()[:, None] * lp.exp() * (lp + H[:, None])
    return d


def bwd_dent(R, seed):
    """Upstream gradient of the entropy, both signs; rows r % 7 == 2 are exactly 0.  With vc.bwd_dlogp (rows r % 5 == 3 zero) the pairs (dlogp = 0, dent != 0) at
    r = 3, (dlogp != 0, dent = 0) at r = 2 and (0, 0) at r = 23 all occur from R = 24 on."""
    g = torch.Generator().manual_seed(seed + 11)
    d = torch.randn(R, generator=g) * 0.5
    d[d == 0] = 0.25
    d[torch.arange(R) % 7 == 2] = 0.0
    return d


def ref_quantile_weight(ent, mask, rho):
    """fp64 torch.quantile over the live values, then >=  ->  (weight fp32 shaped like ent, thr, kept, n).  Masked positions are never looked at."""
    live = mask != 0
    vals = ent[live].double()
    n = int(vals.numel())
    if n == 0:
        return torch.zeros(ent.shape, dtype=torch.float32), 0.0, 0, 0
    thr = torch.quantile(vals, 1.0 - rho)
    w = torch.zeros(ent.shape, dtype=torch.float32)
    w[live] = (vals >= thr).float()
    return w, float(thr), int(w.sum()), n


def quantile_masks(G, C):
    """name -> mask int32 [G, C]: vc.grpo_case's (a row of length 1, a row with holes, prefixes, a full row), the same with row 1 and the last row fully masked
    (G > 1), and an all-masked grid."""
    mask = vc.grpo_case(G, C)[2]
    out = {"case": mask, "none": torch.zeros_like(mask)}
    if G > 1:
        m2 = mask.clone()
        m2[1] = 0
        m2[G - 1] = 0
        out["empty"] = m2
    return out


def quantile_entropies(mask, kind, seed=0):
    """fp32 [G, C], NaN at masked positions.  "uniform": uniform in [0, 5).  "zeros": half of the live values exactly 0.0, a few at -1e-7 (lse - s / z rounds
    below zero on a one-hot row) and -0.0, the rest uniform."""
    G, C = mask.shape
    g = torch.Generator().manual_seed(7001 + seed + 131 * G + C)
    e = torch.rand(G, C, generator=g) * 5
    if kind == "zeros":
        u = torch.rand(G, C, generator=g)
        e[u < 0.5] = 0.0
        e[u < 0.06] = -1e-7
        e[u < 0.03] = -0.0
    else:
        assert kind == "uniform"
    return torch.where(mask != 0, e, torch.full_like(e, float("nan")))


def compare_quantile(got_w, got_stats, ent, mask, rho, what):
    """The selection against the fp64 reference -> number of tokens left out of the comparison (near the threshold and not equal to it)."""
    ref_w, thr, kept, n = ref_quantile_weight(ent, mask, rho)
    w, st = got_w.detach().float().cpu(), got_stats.detach().double().cpu()
    assert torch.isfinite(w).all() and torch.isfinite(st).all(), what
    assert bool(((w == 0) | (w == 1)).all()) and bool((w[mask == 0] == 0).all()), what
    live = mask != 0
    near = (live & ((ent.double() - thr).abs() <= NEAR_THR) & (ent.double() != thr)) if n else torch.zeros_like(live)      # NaN (masked) compares false
    left = int((near & (w != ref_w)).sum())
    assert left <= MAX_LEFT_OUT, (what, left)
    assert torch.equal(w[~near], ref_w[~near]), (what, int((w != ref_w).sum()), left)
    assert float(st[2]) == n and abs(float(st[0]) - thr) <= TOL_THR and abs(float(st[1]) - kept) <= left and float(st[1]) == float(w.sum()), (what, st, thr, kept, n)
    if rho == 1.0:
        assert torch.equal(w, live.float()), what
    return left


# ------------------------------------------------------------------------------------------------------ the tiny trainer with the two options
def first_step(ops, case, out_dir, **over):
    """lfc.first_step_masters on any golden fixture: one optimizer step (GA = 2, two rows) -> (masters, the step's log)."""
    import ratio_cases as rc
    from helpers import load_case
    tr = rc.tiny_trainer(ops, load_case(case), out_dir, mu=1, n_rows=2, **over)
    rec = rc.run_recorded(tr)
    assert tr.state.global_step == 1 and len(rec["masters"]) == 1
    return rec["masters"][0], tr.state.log_history[0]


def _bits(t):
    return t.contiguous().view(torch.int32)


def check_defaults_are_the_parent_run(ops, tmp_path, plain_ops=None):
    """entropy_coef = 0 and top_entropy_quantile = 1, implicit or explicit (None = 1), reach the masters of a run that names neither, bit for bit; plain_ops (a
    backend WITHOUT the two ops) runs the defaults too: no new code runs."""
    for case in ("clip_beta", "grpo_beta"):
        base, log0 = first_step(ops, case, tmp_path / (case + "-base"))
        for name, over in (("explicit", dict(entropy_coef=0.0, top_entropy_quantile=1.0)), ("none", dict(top_entropy_quantile=None))):
            got, log = first_step(ops, case, tmp_path / (case + "-" + name), **over)
            assert torch.equal(_bits(got), _bits(base)), (case, name, float((got - base).abs().max()))
            assert log["loss"] == log0["loss"] and set(log) == set(log0)
        if plain_ops is not None:
            assert not hasattr(plain_ops, "logp_entropy_bwd") and not hasattr(plain_ops, "entropy_quantile_weight")
            got, _ = first_step(plain_ops, case, tmp_path / (case + "-plain"))
            assert torch.equal(_bits(got), _bits(base)), case


def check_entropy_bonus_in_the_logged_loss(ops, tmp_path):
    """use_grpo: the bonus's normaliser is the row mean, which is generation_entropy's own mean, and the first step's rollout does not depend on the coefficient:
    loss(c) = loss(0) - c * generation_entropy.  1e-5: fp32 sums of O(1) terms (1e-7 each) and the log's rounding of `loss` to 6 decimals."""
    base, log0 = first_step(ops, "grpo_beta", tmp_path / "c0")
    H = log0["generation_entropy"]
    assert H > 0.1, H
    for c in (0.01, -0.01):
        got, log = first_step(ops, "grpo_beta", tmp_path / ("c%g" % c), entropy_coef=c)
        assert set(log) == set(log0), "no new log keys"
        assert log["generation_entropy"] == H and log["reward"] == log0["reward"]
        err = abs(log["loss"] - (log0["loss"] - c * H))
        print("entropy_coef %g: loss %.6f, expected %.6f - %g * %.6f, error %.3g" % (c, log["loss"], log0["loss"], c, H, err))
        assert err <= 1e-5, (c, log["loss"], log0["loss"], H)
        assert float((got - base).abs().max()) > 1e-6, "the bonus must reach the weights"


def check_top_entropy_quantile_changes_the_step(ops, tmp_path):
    for case in ("clip_beta", "grpo_beta"):
        base, log0 = first_step(ops, case, tmp_path / (case + "-all"))
        got, log = first_step(ops, case, tmp_path / (case + "-top"), top_entropy_quantile=0.2)
        assert set(log) == set(log0) and log["generation_entropy"] == log0["generation_entropy"]
        assert float((got - base).abs().max()) > 1e-6, case


def check_two_iterations_with_both_options(ops, tmp_path):
    import math
    import ratio_cases as rc
    from helpers import load_case
    for over in (dict(), dict(loss_type="dr_grpo", importance_sampling_level="sequence", delta=1.5)):
        tr = rc.tiny_trainer(ops, load_case("clip_beta"), tmp_path / ("mu2-%d" % len(over)), mu=2, ga=2, n_rows=2, entropy_coef=0.01, top_entropy_quantile=0.5, **over)
        rec = rc.run_recorded(tr)
        assert tr.state.global_step == 2 and rec["rollouts"] == 1 and len(rec["replay_old"]) == 2
        for log in tr.state.log_history:
            for k in ("loss", "kl", "generation_entropy", "grad_norm"):
                assert k in log and math.isfinite(log[k]), (k, log.get(k))
        assert float((rec["masters"][1] - rec["masters"][0]).abs().max()) > 0


def check_all_truncated_leaves_the_weights_alone(ops, tmp_path):
    """lfc.check_all_truncated_leaves_the_weights_alone with both options on: every mask row is zero, so no token is selected, the bonus's normaliser is 0 everywhere
    and the update is a finite no-op."""
    import math
    import ratio_cases as rc
    from helpers import load_case
    tr = rc.tiny_trainer(ops, load_case("clip_beta"), tmp_path / "trunc", mu=1, mask_truncated_completions=True, entropy_coef=0.01, top_entropy_quantile=0.5)
    tr.processing_class.eos_token_id = -7
    before = tr.params.train.master.detach().clone().cpu()
    rec = rc.run_recorded(tr)
    assert tr.state.global_step == 2 and len(rec["masters"]) == 2
    for m in rec["masters"]:
        assert torch.equal(_bits(m), _bits(before))
    for log in tr.state.log_history:
        assert log["completions/clipped_ratio"] == 1.0 and log["loss"] == 0.0
        for k, v in log.items():
            assert not isinstance(v, float) or math.isfinite(v), (k, v)
