"""The GRPO objective family (GRPOConfig.loss_type / importance_sampling_level / delta / scale_rewards / mask_truncated_completions), CPU side: the fp64
reference of tests/loss_family_cases.py against its fp32 stand-in and against the references it must coincide with, the conditions on the cases, config
validation, the host-side pieces, and the trainer on the oracle op backend (RefOps).  tests/test_loss_family_gpu.py runs the HIP kernel and the HIP
trainer against the same references."""
import math

import numpy as np
import pytest
import torch

import loss_family_cases as fc
import ratio_cases as rc
import vocab_cases as vc
from oracle.ref_ops import RefOps
from test_policy_reuse_ref import STANDIN_SHARE
from time_r1_amd.grpo import eos_mask, group_advantages, policy_objective, truncation_mask
from time_r1_amd.trainer import GRPOConfig


def _args(c, with_w):
    return c["logp"], c["old_logp"], c["ref_logp"], (c["tok_weight"] if with_w else None), c["mask"], c["adv"]


@pytest.mark.parametrize("G,C", vc.GRPO_SHAPES)
def test_fp32_standin_against_fp64_reference(G, C):
    worst, moved = 0.0, 0
    for eps in rc.EPS_PAIRS:
        c = fc.family_case(G, C, eps)
        moved += c["moved"]
        for cc in (c, c["empty"]) if (G, C) in fc.EMPTY_SHAPES else (c,):
            dead = cc["mask"] == 0
            for norm, level, delta, beta, with_w in fc.settings():
                logp, old, ref_lp, w, mask, adv = _args(cc, with_w)
                ref = fc.ref_policy_loss(logp, old, ref_lp, w, mask, adv, beta, norm, level, eps[0], eps[1], delta, 0.5)
                got = RefOps().grpo_policy_loss(logp, old, ref_lp, mask, adv, beta, norm, level, eps[0], eps[1], delta, 0.5, tok_weight=w)
                worst = max(worst, fc.compare(got, ref, dead, (eps, norm, level, delta, beta, with_w)))
    print("G=%d C=%d: worst share of TOL_GRPO %.4f, %d boundary tokens / rows moved" % (G, C, worst, moved))
    assert worst <= STANDIN_SHARE, worst


def test_every_regime_occurs_at_sequence_level():
    """A condition on the INPUTS: over the shapes with G >= 8 the rows cover unclipped / low-clipped / high-clipped / delta-capped / positive-below-range, and no
    row sits anywhere else."""
    for eps in rc.EPS_PAIRS:
        seen = set()
        for G, C in vc.GRPO_SHAPES:
            reg = fc.row_regimes(fc.family_case(G, C, eps), eps)
            assert "other" not in reg and None not in reg, (G, C, reg)
            if G >= 8:
                seen |= set(reg)
                assert set(reg) == set(fc.REGIMES), (G, C, reg)
        assert seen == set(fc.REGIMES)
    for G, C in fc.EMPTY_SHAPES:
        e = fc.family_case(G, C, rc.EPS_PAIRS[0])["empty"]
        lens = e["mask"].sum(1)
        assert int(lens[1]) == 0 and int(lens[G - 1]) == 0 and int(lens[0]) > 0


@pytest.mark.parametrize("G,C", vc.GRPO_SHAPES)
def test_token_mean_at_token_level_without_a_cap_is_the_ratio_reference(G, C):
    for eps in rc.EPS_PAIRS:
        c = fc.family_case(G, C, eps)
        for beta, with_w in ((0.0, False), (0.04, True)):
            logp, old, ref_lp, w, mask, adv = _args(c, with_w)
            a = fc.ref_policy_loss(logp, old, ref_lp, w, mask, adv, beta, "token", "token", eps[0], eps[1], 0.0, 0.5)
            b = rc.ref_grpo_ratio(logp, old, ref_lp, w, mask, adv, beta, False, eps[0], eps[1], 0.5)
            for x, y in zip(a, b):
                assert torch.allclose(x, y, atol=1e-14, rtol=1e-12)


@pytest.mark.parametrize("G,C", vc.GRPO_SHAPES)
def test_sequence_level_on_the_policy_itself_is_token_level(G, C):
    """old_logp == logp, no tok_weight: s_g = 1 and d s_g / d logp_t = 1 / len_g on each of the len_g live tokens - the token-level gradient, in all three norms."""
    c = fc.family_case(G, C, rc.EPS_PAIRS[1])
    logp, _, ref_lp, _, mask, adv = _args(c, False)
    for norm in fc.NORMS:
        for old in (logp.clone(), None):
            a = fc.ref_policy_loss(logp, old, ref_lp, None, mask, adv, 0.04, norm, 1, 0.2, 0.28, fc.DELTA, 1.0)
            b = fc.ref_policy_loss(logp, old, ref_lp, None, mask, adv, 0.04, norm, 0, 0.2, 0.28, fc.DELTA, 1.0)
            assert torch.allclose(a[0], b[0], atol=1e-15, rtol=1e-12) and torch.allclose(a[1], b[1], atol=1e-14, rtol=1e-12)
            assert float(a[1][7]) == 1.0 and bool((a[1][3:7] == 0).all())


def test_empty_rows_and_an_empty_grid_give_zeros_not_nan():
    for G, C in fc.EMPTY_SHAPES:
        e = fc.family_case(G, C, rc.EPS_PAIRS[0])["empty"]
        none = dict(e, mask=torch.zeros_like(e["mask"]))
        for norm, level, delta, beta, with_w in fc.settings():
            for fn in ("ref", "fp32"):
                for cc in (e, none):
                    logp, old, ref_lp, w, mask, adv = _args(cc, with_w)
                    if fn == "ref":
                        out = fc.ref_policy_loss(logp, old, ref_lp, w, mask, adv, beta, norm, level, 0.2, 0.2, delta, 1.0)
                    else:
                        out = RefOps().grpo_policy_loss(logp, old, ref_lp, mask, adv, beta, norm, level, 0.2, 0.2, delta, 1.0, tok_weight=w)
                    assert all(torch.isfinite(t).all() for t in out)
                    assert bool((out[0][mask == 0] == 0).all())
                    assert float(out[2][1]) == 0 and float(out[3][1]) == 0 and float(out[2][G - 1]) == 0 and float(out[3][G - 1]) == 0
                    if cc is none:
                        assert bool((out[0] == 0).all()) and bool((out[1] == 0).all()), out[1]


def test_config_validation():
    bad = (dict(loss_type="dapo"), dict(loss_type="ppo"), dict(loss_type="grpo", use_grpo=True), dict(importance_sampling_level="group"),
           dict(delta=1.2), dict(delta=1.1, epsilon_low=0.1), dict(delta=1.25, epsilon_high=0.28), dict(delta=-1.0), dict(use_grpo=True, delta=2.0),
           dict(use_grpo=True, importance_sampling_level="sequence"))
    for kw in bad:
        with pytest.raises(ValueError):
            GRPOConfig(**kw)
    with pytest.raises(ValueError, match="out of scope"):
        GRPOConfig(loss_type="dapo")
    with pytest.raises(ValueError, match="loss_type.*use_grpo"):
        GRPOConfig(loss_type="bnpo", use_grpo=True)
    c = GRPOConfig()
    assert (c.loss_type, c.importance_sampling_level, c.delta, c.scale_rewards, c.mask_truncated_completions) == (None, "token", None, True, False)
    c = GRPOConfig(loss_type="dr_grpo", importance_sampling_level="sequence", delta="1.5", epsilon_high=0.28, scale_rewards=False, mask_truncated_completions=True)
    assert c.delta == 1.5 and c.scale_rewards is False and c.mask_truncated_completions is True
    assert GRPOConfig(delta=1.15, epsilon_low=0.1).delta == 1.15            # epsilon_high None: the bound is 1 + epsilon_low
    GRPOConfig(use_grpo=True, mask_truncated_completions=True, scale_rewards=False)


def test_routing_of_the_settings_to_the_kernel_arguments():
    assert policy_objective() is None and policy_objective(use_grpo=True) is None
    assert policy_objective(loss_type="grpo", epsilon_low=0.1, epsilon_high=0.3) == dict(norm=0, level=0, eps_low=0.1, eps_high=0.3, delta=0.0)
    assert policy_objective(loss_type="bnpo")["norm"] == 1 and policy_objective(loss_type="dr_grpo")["norm"] == 2
    assert policy_objective(importance_sampling_level="sequence") == dict(norm=1, level=1, eps_low=0.2, eps_high=0.2, delta=0.0)
    assert policy_objective(delta=1.5)["delta"] == 1.5 and policy_objective(mask_truncated_completions=True)["norm"] == 1
    o = policy_objective(use_grpo=True, mask_truncated_completions=True)
    # no clip: the range is [0, 3e38], which no fp32 ratio leaves - the clipped loss with this range IS the unclipped one
    assert o["norm"] == 0 and 1 - o["eps_low"] == 0.0 and 1 + o["eps_high"] > 1e38 and math.isfinite(o["eps_high"])
    c = fc.family_case(8, 200, (0.2, 0.2))
    logp, old, ref_lp, w, mask, adv = _args(c, True)
    a = fc.ref_policy_loss(logp, old, ref_lp, w, mask, adv, 0.04, o["norm"], o["level"], o["eps_low"], o["eps_high"], o["delta"], 1.0)
    b = rc.ref_grpo_ratio(logp, old, ref_lp, w, mask, adv, 0.04, True, 0.2, 0.2, 1.0)
    assert torch.allclose(a[0], b[0], atol=1e-15, rtol=1e-12) and torch.allclose(a[1][:3], b[1][:3], atol=1e-14, rtol=1e-12)


def test_group_advantages_without_the_division_by_std():
    g = torch.Generator().manual_seed(0)
    rpf = torch.rand(16, 2, generator=g)
    rpf[8:] = rpf[8:9] + 1e-4 * torch.rand(8, 2, generator=g)       # a near-constant group: the case scale_rewards=False exists for
    r0, a0, s0 = group_advantages(rpf, 8)
    r1, a1, s1 = group_advantages(rpf, 8, scale=True)
    r2, a2, s2 = group_advantages(rpf, 8, scale=False)
    assert torch.equal(a0, a1) and torch.equal(r0, r2) and torch.equal(s0, s2)
    mean = r2.view(2, 8).mean(1).repeat_interleave(8)
    assert torch.equal(a2, r2 - mean)
    assert torch.allclose(a0, a2 / (s0 + 1e-4))
    assert float(a0[8:].abs().max()) > 100 * float(a2[8:].abs().max())


def test_truncation_mask_on_hand_written_grids():
    eos, C = 9, 5
    ids = np.array([[9, 1, 2, 3, 4],        # EOS at 0: one live token, not truncated
                    [1, 2, 3, 4, 9],        # EOS at C - 1: all live, not truncated
                    [1, 2, 3, 4, 5],        # no EOS: truncated
                    [1, 9, 9, 2, 3]])       # EOS in the middle
    m = eos_mask(ids, eos)
    assert m.tolist() == [[1, 0, 0, 0, 0], [1, 1, 1, 1, 1], [1, 1, 1, 1, 1], [1, 1, 0, 0, 0]]
    m2, trunc = truncation_mask(ids, eos, m)
    assert trunc.tolist() == [False, False, True, False]
    assert m2.dtype == np.int32 and m2.tolist() == [[1, 0, 0, 0, 0], [1, 1, 1, 1, 1], [0, 0, 0, 0, 0], [1, 1, 0, 0, 0]]
    assert m.sum(1).tolist() == [1, 5, 5, 2]         # the caller's lengths (completion_length) are taken before the rows are zeroed


def test_the_five_settings_parse_from_the_command_line(monkeypatch):
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import train_grpo
    seen = {}

    class Stop(Exception):
        pass

    def trainer(model=None, reward_funcs=None, metric_funcs=None, args=None, **kw):
        seen["args"] = args
        raise Stop()
    monkeypatch.setattr(train_grpo, "init_from_env", lambda *a, **k: None)
    monkeypatch.setattr(train_grpo, "load_json_dataset_tg", lambda *a, **k: [])
    monkeypatch.setattr(train_grpo, "TimeR1_Trainer", trainer)
    base = ["train_grpo.py", "--model_name_or_path", "m", "--train_data_path", "d"]
    monkeypatch.setattr(sys, "argv", base + ["--loss_type", "dr_grpo", "--importance_sampling_level", "sequence", "--delta", "1.5", "--scale_rewards", "false",
                                             "--mask_truncated_completions", "true"])
    with pytest.raises(Stop):
        train_grpo.main()
    a = seen["args"]
    assert (a.loss_type, a.importance_sampling_level, a.delta, a.scale_rewards, a.mask_truncated_completions) == ("dr_grpo", "sequence", 1.5, False, True)
    monkeypatch.setattr(sys, "argv", base)
    with pytest.raises(Stop):
        train_grpo.main()
    a = seen["args"]
    assert (a.loss_type, a.importance_sampling_level, a.delta, a.scale_rewards, a.mask_truncated_completions) == (None, "token", None, True, False)
    monkeypatch.setattr(sys, "argv", base + ["--loss_type", "dapo"])
    with pytest.raises(ValueError, match="dapo"):
        train_grpo.main()


def test_torch_op_is_registered_with_a_fake_kernel_and_no_cpu_fallback():
    import time_r1_amd.torch_ops as T
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert "grpo_policy_loss" in T.OP_NAMES
    assert str(torch.ops.timer1.grpo_policy_loss.default._schema).startswith("timer1::grpo_policy_loss")
    with FakeTensorMode():
        lp = torch.empty(8, 200, device="cuda")
        m = torch.empty(8, 200, dtype=torch.int32, device="cuda")
        out8, dlogp, row_len = torch.ops.timer1.grpo_policy_loss(lp, None, None, None, m, torch.empty(8, device="cuda"), 0.0, 2, 1, 0.2, 0.2, 1.5, 1.0)
        assert out8.shape == (8,) and dlogp.shape == (8, 200) and row_len.shape == (8,)
        loss, kl, stats = T.grpo_policy_loss(lp, lp, lp, m, torch.empty(8, device="cuda"), 0.04, "dr_grpo", "sequence", 0.2, 0.28, delta=1.5, tok_weight=lp)
        assert loss.shape == () and kl.shape == () and stats.shape == (5,)
    c = fc.family_case(3, 257, (0.2, 0.2))
    with pytest.raises(NotImplementedError):
        T.grpo_policy_loss(c["logp"], c["old_logp"], c["ref_logp"], c["mask"], c["adv"], 0.04)
    with pytest.raises(KeyError):
        T.grpo_policy_loss(c["logp"], c["old_logp"], c["ref_logp"], c["mask"], c["adv"], 0.04, loss_type="dapo")


def test_bnpo_and_the_sequence_level_reach_the_legacy_first_step(tmp_path):
    fc.check_first_step_equals_legacy(RefOps(), tmp_path, fc.STEP1_ATOL)


def test_all_truncated_completions_leave_the_weights_bit_unchanged(tmp_path):
    fc.check_all_truncated_leaves_the_weights_alone(RefOps(), tmp_path)


def test_use_grpo_with_the_truncation_mask_takes_the_general_path(tmp_path):
    from helpers import load_case
    ops = RefOps()
    calls = []
    orig = ops.grpo_policy_loss
    ops.grpo_policy_loss = lambda *a, **k: (calls.append(a[6:11]), orig(*a, **k))[1]
    tr = rc.tiny_trainer(ops, load_case("grpo_beta"), tmp_path, mu=1, ga=1, n_rows=1, mask_truncated_completions=True)
    rc.run_recorded(tr)
    assert len(calls) == 1 and calls[0][0] == 0 and calls[0][1] == 0 and calls[0][2] == 1.0 and calls[0][3] > 1e38, calls
    assert "completions/clipped_ratio" in tr.state.log_history[0]
    with pytest.raises(ValueError, match="use_grpo"):
        rc.tiny_trainer(ops, load_case("grpo_beta"), tmp_path, mu=2, mask_truncated_completions=True)


def test_two_updates_at_sequence_level_with_a_cap_log_finite_replay_keys(tmp_path):
    from helpers import load_case
    tr = rc.tiny_trainer(RefOps(), load_case("clip_beta"), tmp_path, mu=2, ga=2, n_rows=2, importance_sampling_level="sequence", delta=1.5)
    rec = rc.run_recorded(tr)
    assert tr.state.global_step == 2 and rec["rollouts"] == 1 and len(rec["replay_old"]) == 2
    logs = tr.state.log_history
    for step in (0, 1):
        for k in rc.REPLAY_KEYS + ("loss", "kl", "generation_entropy", "grad_norm"):
            assert k in logs[step] and math.isfinite(logs[step][k]), (step, k, logs[step].get(k))
    assert logs[0]["policy_kl_old"] == 0.0 and logs[1]["policy_kl_old"] > 0       # the policy has left the one that drew the completions
    assert "reward" in logs[0] and "reward" not in logs[1] and "completions/clipped_ratio" not in logs[0]
    assert float((rec["masters"][1] - rec["masters"][0]).abs().max()) > 0
