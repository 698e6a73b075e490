"""Cases and fp64 reference for the GRPO objective family (tr1_grpo_policy_loss, csrc/loss.hip; its fp32 CPU stand-in is
oracle.ref_ops.RefOps.grpo_policy_loss): the clipped loss with a choice of
normaliser (GRPOConfig.loss_type), a token- or sequence-level importance coefficient (importance_sampling_level) and an upper cap on it (delta), and with
rows that hold no live token (mask_truncated_completions).  Shared by tests/test_loss_family_ref.py (CPU) and tests/test_loss_family_gpu.py.

Per live token, with d = logp - old_logp (0 when there is no old policy), kl = exp(ref - logp) - (ref - logp) - 1, w = tok_weight or 1 (a constant):
  c = exp(d)                       (level 0, token)          c = s_g = exp(sum_t d m / max(len_g, 1))          (level 1, sequence)
  a = min(min(c, delta) A, clamp(c, 1 - eps_low, 1 + eps_high) A)        (delta <= 0: no inner min)
  l = -w a + beta kl,  loss = sum n l,  n = m / (max(len_g, 1) G) | m / max(tot, 1) | m / (G C)        (norm 0 row mean | 1 token mean | 2 fixed length)
The reference below is that text in fp64 with torch.min / torch.clamp, differentiated by autograd.

The clip decisions are step functions of c, so whatever sits within ratio_cases.NEAR of a boundary (1 - eps_low, 1 + eps_high, delta) is MOVED - a token at
token level, a whole row at sequence level - never left out.  The rows cycle through five regimes of (sign of A, s_g), see REGIMES.
"""
import torch

import ratio_cases as rc
import vocab_cases as vc
from oracle.ref_ops import grpo_modes

DELTA = 1.5
NORMS = (0, 1, 2)
LEVELS = (0, 1)
EMPTY_SHAPES = ((8, 200), (3, 257))
REGIMES = ("unclipped", "low", "high", "capped", "below")
# row g is built for regime g % 5: the target of its s_g as a multiple of a boundary (>= 10 % away from every boundary, 100 x NEAR) and the sign of A
#   unclipped: s inside the range, A as drawn      low: A < 0, s < 1 - eps_low      high: A > 0, s > 1 + eps_high
#   capped: A < 0, s > delta                       below: A > 0, s < 1 - eps_low (the unclipped side is the smaller one: the gradient flows)
_TARGET = {"unclipped": lambda lo, hi: 1.05, "low": lambda lo, hi: 0.8 * lo, "high": lambda lo, hi: 1.1 * hi, "capped": lambda lo, hi: 1.15 * DELTA,
           "below": lambda lo, hi: 0.8 * lo}
_SIGN = {"unclipped": 0, "low": -1, "high": 1, "capped": -1, "below": 1}


def _bounds(eps):
    return (1 - eps[0], 1 + eps[1], DELTA)


def _row_coef(logp, old, live):
    d = torch.where(live, logp.double() - old.double(), torch.zeros_like(logp, dtype=torch.float64))
    return torch.exp(d.sum(1) / live.sum(1).clamp(min=1))


def _near_tokens(logp, old, live, eps):
    rho = torch.exp(logp.double() - old.double())
    return live & torch.stack([(rho - b).abs() < rc.NEAR for b in _bounds(eps)]).any(0)


def _near_rows(logp, old, live, eps):
    s = _row_coef(logp, old, live)
    return live.any(1) & torch.stack([(s - b).abs() < rc.NEAR for b in _bounds(eps)]).any(0)


def row_regimes(case, eps, delta=DELTA):
    """The regime each row is in at sequence level, from the inputs alone (None for a row without a live token)."""
    live = case["mask"].bool()
    s = _row_coef(case["logp"], case["old_logp"], live)
    out = []
    for g in range(live.shape[0]):
        A, sg = float(case["adv"][g]), float(s[g])
        if not bool(live[g].any()):
            out.append(None)
        elif A < 0 and sg > delta:
            out.append("capped")
        elif A < 0 and sg < 1 - eps[0]:
            out.append("low")
        elif A > 0 and sg > 1 + eps[1]:
            out.append("high")
        elif A > 0 and sg < 1 - eps[0]:
            out.append("below")
        elif 1 - eps[0] < sg < 1 + eps[1]:
            out.append("unclipped")
        else:
            out.append("other")
    return out


_CACHE = {}


def family_case(G, C, eps, seed=0):
    """-> dict(logp, old_logp, ref_logp, tok_weight fp32 [G, C], mask int32 [G, C], adv fp32 [G], moved, empty).  ratio_cases.ratio_case plus, per row, a shift of
    logp - old_logp that puts the row's s_g on the target of regime g % 5 and the sign of adv that the regime names; then every token and every row within
    NEAR of 1 - eps_low, 1 + eps_high or DELTA is moved by 0.01 in the log-ratio.  moved counts both.  `empty`: the same case with row 1 and the last row
    fully masked (old_logp = -300 there, like every masked position).  Built once per (G, C, eps, seed) and shared: treat it as read-only."""
    key = (G, C, eps, seed)
    if key in _CACHE:
        return _CACHE[key]
    c = rc.ratio_case(G, C, eps, seed)
    logp, mask = c["logp"], c["mask"]
    live = mask.bool()
    old = torch.where(live, c["old_logp"], logp)
    lo, hi, _ = _bounds(eps)
    adv = c["adv"].clone()
    s = _row_coef(logp, old, live)
    for g in range(G):
        name = REGIMES[g % 5]
        shift = float(torch.log(torch.tensor(_TARGET[name](lo, hi), dtype=torch.float64)) - torch.log(s[g]))
        old[g] = old[g] - shift                      # d grows by shift on the whole row: s_g lands on the target
        if _SIGN[name]:
            adv[g] = _SIGN[name] * adv[g].abs().clamp(min=0.1)
    moved = 0
    for _ in range(8):
        near_t = _near_tokens(logp, old, live, eps)
        old = torch.where(near_t, old - 0.01, old)
        near_r = _near_rows(logp, old, live, eps)
        old = torch.where(near_r[:, None] & live, old - 0.01, old)
        moved += int(near_t.sum()) + int(near_r.sum())
        if not near_t.any() and not near_r.any():
            break
    assert not _near_tokens(logp, old, live, eps).any() and not _near_rows(logp, old, live, eps).any()
    dead = torch.full_like(old, -300.0)
    out = dict(logp=logp, old_logp=torch.where(live, old, dead), ref_logp=c["ref_logp"], tok_weight=c["tok_weight"], mask=mask, adv=adv, moved=moved)
    m2 = mask.clone()
    m2[min(1, G - 1)] = 0
    m2[G - 1] = 0
    out["empty"] = dict(out, mask=m2, old_logp=torch.where(m2.bool(), old, dead))
    _CACHE[key] = out
    return out


def ref_policy_loss(logp, old_logp, ref_logp, tok_weight, mask, adv, beta, norm, level, eps_low, eps_high, delta, grad_scale):
    """fp64 + autograd -> (dlogp = grad_scale * d loss / d logp, out8, row_len, row_kl).  out8 = [loss, mean_g(sum_t kl m / max(len_g, 1)), sum mask, low / high /
    either clip fraction over max(sum mask, 1), masked mean of c - 1 - log c, largest c over the live tokens (0 when there is none)]."""
    norm, level = grpo_modes(norm, level)
    G, C = logp.shape
    lp = logp.double().clone().requires_grad_(True)
    live = mask.bool()
    m = mask.bool().double()
    A = adv.double()[:, None]
    zero = torch.zeros_like(lp)
    lens, tot = m.sum(1), m.sum()
    len1, tot1 = lens.clamp(min=1), tot.clamp(min=1)
    d = torch.where(live, lp - (old_logp.double() if old_logp is not None else lp.detach()), zero)      # selection: a masked position holds anything
    logc = ((d * m).sum(1) / len1)[:, None].expand(G, C) if level == 1 else d
    c = torch.exp(logc)
    kl = zero
    if ref_logp is not None:
        r = torch.where(live, ref_logp.double() - lp, zero)
        kl = torch.exp(r) - r - 1
    w = tok_weight.double() if tok_weight is not None else torch.ones_like(lp)
    capped = torch.min(c, torch.full_like(c, delta)) if delta and delta > 0 else c
    per_tok = -w * torch.min(capped * A, torch.clamp(c, 1 - eps_low, 1 + eps_high) * A) + beta * kl
    n = (m / (len1[:, None] * G), m / tot1, m / float(G * C))[norm]
    loss = (n * per_tok).sum()
    (grad,) = torch.autograd.grad(loss, lp, allow_unused=True)
    grad = torch.zeros_like(lp) if grad is None else grad
    c, kl, logc = c.detach(), kl.detach(), logc.detach()
    is_low = (c < 1 - eps_low) & (A < 0)
    is_high = (c > 1 + eps_high) & (A > 0)
    out8 = torch.stack([loss.detach(), ((kl * m).sum(1) / len1).mean(), tot, (is_low * m).sum() / tot1, (is_high * m).sum() / tot1,
                        ((is_low | is_high) * m).sum() / tot1, ((c - 1 - logc) * m).sum() / tot1, torch.where(live, c, zero).max()])
    return grad * grad_scale, out8, lens, (kl * m).sum(1)


def settings():
    """(norm, level, delta, beta, with tok_weight) over the whole product."""
    import itertools
    return list(itertools.product(NORMS, LEVELS, (0.0, DELTA), (0.0, 0.04), (False, True)))


def compare(got, ref, dead, what):
    """The four outputs of one call against the reference: finite, within TOL_GRPO, clip fractions within 1e-6, dlogp zero at dead positions -> worst share."""
    worst = 0.0
    for name, a, b in zip(("dlogp", "out8", "row_len", "row_kl"), got, ref):
        assert torch.isfinite(a).all(), (name, what)
        r = vc.worst(a, b, vc.TOL_GRPO)[0]
        worst = max(worst, r)
    assert torch.allclose(got[1][3:6].double().cpu(), ref[1][3:6], atol=1e-6, rtol=0), (what, got[1][3:6], ref[1][3:6])
    assert bool((got[0].cpu()[dead] == 0).all()), what
    return worst


# tiny-trainer equalities: the bound on the masters after one optimizer step between two runs whose gradients differ in summation order only.  A reordered
# sum moves a gradient element by ~1e-7 of its terms; the first AdamW step lr * g / (|g| + eps) turns a relative change r of g into at most lr * r / 4, and
# only elements whose terms cancel down to |g| ~ eps move further, by lr * dg / eps: percent of lr.  2 % of the fixture's lr = 1e-4 is the bound the suite
# holds such differences to (test_policy_reuse_gpu.py, test_configs_gpu.py); a wrong normaliser or sign moves every element by lr, fifty times as far.
STEP1_ATOL = 2e-6


def first_step_masters(ops, out_dir, **over):
    """One optimizer step (GA = 2, two rows) of the tiny trainer on the clip_beta fixture -> (masters, the step's log)."""
    from helpers import load_case
    tr = rc.tiny_trainer(ops, load_case("clip_beta"), out_dir, mu=1, n_rows=2, **over)
    rec = rc.run_recorded(tr)
    assert tr.state.global_step == 1 and len(rec["masters"]) == 1
    return rec["masters"][0], tr.state.log_history[0]


def check_first_step_equals_legacy(ops, tmp_path, atol):
    """loss_type="bnpo" is the legacy clip branch's normaliser, and at one update per rollout (c = 1 everywhere) a sequence-level ratio changes neither the loss
    nor its gradient: both reach the legacy run's masters.  -> the two logs of the runs on the general path."""
    base, log0 = first_step_masters(ops, tmp_path / "legacy")
    assert "policy_kl_old" not in log0
    logs = []
    for name, over in (("bnpo", dict(loss_type="bnpo")), ("sequence", dict(importance_sampling_level="sequence"))):
        got, log = first_step_masters(ops, tmp_path / name, **over)
        diff = float((got - base).abs().max())
        print("%s: largest master difference to the legacy run %.3g" % (name, diff))
        assert diff <= atol, (name, diff)
        for k in rc.REPLAY_KEYS:
            assert k in log, (name, k)
        assert log["clip_ratio/region_mean"] == 0.0 and abs(log["policy_kl_old"]) < 1e-9
        logs.append(log)
    return logs


def check_all_truncated_leaves_the_weights_alone(ops, tmp_path):
    """An EOS id that never occurs: every completion is truncated, every mask row is zero, and an update must be a no-op - not NaN."""
    import math
    from helpers import load_case
    tr = rc.tiny_trainer(ops, load_case("clip_beta"), tmp_path / "trunc", mu=1, mask_truncated_completions=True)
    tr.processing_class.eos_token_id = -7
    before = tr.params.train.master.detach().clone().cpu()
    rec = rc.run_recorded(tr)
    assert tr.state.global_step == 2 and len(rec["masters"]) == 2
    for m in rec["masters"]:
        assert torch.equal(m.view(torch.int32), before.view(torch.int32))
    for log in tr.state.log_history:
        assert log["completions/clipped_ratio"] == 1.0 and log["completion_length"] == tr.max_completion_length
        for k, v in log.items():
            assert not isinstance(v, float) or math.isfinite(v), (k, v)
    return tr
