"""Several clipped policy updates per rollout (GRPOConfig.num_iterations), CPU side: the fp64 reference of the ratio loss against vocab_cases.ref_grpo and
against its fp32 stand-in, config validation, and the trainer's step arithmetic / replay path / resume on the oracle op backend (RefOps).
tests/test_policy_reuse_gpu.py runs the HIP kernel and the HIP trainer against the same references."""
import itertools

import pytest
import torch

import ratio_cases as rc
import vocab_cases as vc
from helpers import load_case
from oracle.ref_ops import RefOps
from time_r1_amd.trainer import GRPOConfig

STANDIN_SHARE = 0.25            # the fp32 stand-in must sit within this share of TOL_GRPO of the fp64 reference


@pytest.mark.parametrize("G,C", vc.GRPO_SHAPES)
def test_fp32_standin_against_fp64_reference(G, C):
    worst, moved = 0.0, 0
    for eps, beta, use_grpo, with_w, gs in itertools.product(rc.EPS_PAIRS, (0.0, 0.04), (False, True), (False, True), (1.0, 0.5)):
        c = rc.ratio_case(G, C, eps)
        moved += c["moved"]
        w = c["tok_weight"] if with_w else None
        ref = rc.ref_grpo_ratio(c["logp"], c["old_logp"], c["ref_logp"], w, c["mask"], c["adv"], beta, use_grpo, eps[0], eps[1], gs)
        got = RefOps().grpo_loss_ratio(c["logp"], c["old_logp"], c["ref_logp"], c["mask"], c["adv"], beta, use_grpo, eps[0], eps[1], gs, tok_weight=w)
        for a, b in zip(got, ref):
            assert torch.isfinite(a).all()
            worst = max(worst, vc.worst(a, b, vc.TOL_GRPO)[0])
        assert torch.allclose(got[1][3:6].double(), ref[1][3:6], atol=1e-6, rtol=0)
        assert bool((got[0][c["mask"] == 0] == 0).all())
    print("G=%d C=%d: worst share of TOL_GRPO %.4f, %d boundary tokens moved" % (G, C, worst, moved))
    assert worst <= STANDIN_SHARE, worst


@pytest.mark.parametrize("G,C", vc.GRPO_SHAPES)
@pytest.mark.parametrize("use_grpo", [False, True])
def test_reference_with_the_old_policy_equal_to_the_policy_is_ref_grpo(G, C, use_grpo):
    logp, ref, mask, adv = vc.grpo_case(G, C)
    for beta, gs in ((0.0, 1.0), (0.04, 0.5)):
        a = rc.ref_grpo_ratio(logp, logp.clone(), ref, None, mask, adv, beta, use_grpo, 0.2, 0.2, gs)
        b = vc.ref_grpo(logp, ref, mask, adv, beta, use_grpo, gs)
        assert torch.allclose(a[0], b[0], atol=1e-14, rtol=1e-12)
        assert torch.allclose(a[1][:3], b[1], atol=1e-14, rtol=1e-12)
        assert torch.equal(a[2], b[2]) and torch.allclose(a[3], b[3], atol=1e-14, rtol=1e-12)
        assert bool((a[1][3:7] == 0).all()) and float(a[1][7]) == 1.0


def test_config_validation():
    for bad in (dict(num_iterations=0), dict(num_iterations=-1), dict(epsilon_low=0.0), dict(epsilon_low=1.0), dict(epsilon_low=-0.1), dict(epsilon_high=0.0),
                dict(epsilon_high=-0.2)):
        with pytest.raises(ValueError):
            GRPOConfig(**bad)
    c = GRPOConfig()
    assert c.num_iterations == 1 and c.epsilon_low == 0.2 and c.epsilon_high is None
    c = GRPOConfig(num_iterations=4, epsilon_low=0.1, epsilon_high="0.28")
    assert c.num_iterations == 4 and c.epsilon_high == 0.28


def test_trainer_rejects_unbounded_and_misaligned_settings(tmp_path):
    ops = RefOps()
    with pytest.raises(ValueError, match="use_grpo"):
        rc.tiny_trainer(ops, load_case("grpo_beta"), tmp_path, mu=2)                 # this fixture has use_grpo=True
    fx = load_case("clip_beta")
    with pytest.raises(ValueError, match="save_steps"):
        rc.tiny_trainer(ops, fx, tmp_path, mu=2, save_steps=3)
    tr = rc.tiny_trainer(ops, fx, tmp_path, mu=2, save_steps=4, epsilon_low=0.1, epsilon_high=0.3)
    assert (tr.num_iterations, tr.epsilon_low, tr.epsilon_high) == (2, 0.1, 0.3)
    tr = rc.tiny_trainer(ops, fx, tmp_path, mu=1, save_steps=3)
    assert (tr.num_iterations, tr.epsilon_low, tr.epsilon_high) == (1, 0.2, 0.2)
    tr.num_iterations = 2                       # settings changed after construction are checked again when train() starts
    with pytest.raises(ValueError, match="save_steps"):
        tr.train()


def test_two_updates_per_rollout_and_resume_on_the_oracle_backend(tmp_path):
    """GA = 2, 4 rows, num_iterations = 2: 2 rollouts, 4 optimizer steps; step 1 is the mu = 1 run's step 1, step 2 is not its step 2; the replays run no
    rollout and no reference-policy forward, are handed the first pass's log-probs, count no tokens twice, and log the clip / old-policy keys.
    (Reference-policy forwards are counted per micro-step: 4 first-pass micro-steps, 4 forwards - not 8.)  Then checkpoint-2 resumed to step 4."""
    ops = RefOps()
    fx, tr2, _ = rc.check_reuse_scenario(ops, tmp_path, atol_step1=0.0)
    rc.check_resume(ops, tmp_path, fx, tr2, atol=2e-6)


def test_three_updates_hand_every_replay_the_same_old_policy(tmp_path):
    ops = RefOps()
    tr = rc.tiny_trainer(ops, load_case("clip_beta"), tmp_path, mu=3, ga=1, n_rows=1)
    rec = rc.run_recorded(tr)
    assert tr.state.global_step == 3 and rec["rollouts"] == 1 and rec["ref_forwards"] == 1
    assert len(rec["first_logp"]) == 1 and len(rec["replay_old"]) == 2
    assert torch.equal(rec["replay_old"][0], rec["first_logp"][0]) and torch.equal(rec["replay_old"][1], rec["first_logp"][0])
    k = [l["policy_kl_old"] for l in tr.state.log_history[1:]]
    assert k[0] > 0 and k[1] > 0                # the policy has left the one that drew the completions


def test_torch_op_is_registered_with_a_fake_kernel_and_no_cpu_fallback():
    import time_r1_amd.torch_ops as T
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert "grpo_loss_ratio" in T.OP_NAMES
    assert str(torch.ops.timer1.grpo_loss_ratio.default._schema).startswith("timer1::grpo_loss_ratio")
    with FakeTensorMode():
        lp = torch.empty(8, 200, device="cuda")
        m = torch.empty(8, 200, dtype=torch.int32, device="cuda")
        out8, dlogp, row_len = torch.ops.timer1.grpo_loss_ratio(lp, lp, None, None, m, torch.empty(8, device="cuda"), 0.0, False, 0.2, 0.2, 1.0)
        assert out8.shape == (8,) and dlogp.shape == (8, 200) and row_len.shape == (8,)
        loss, kl, stats = T.grpo_loss_ratio(lp, lp, lp, m, torch.empty(8, device="cuda"), 0.04, False, 0.2, 0.28, tok_weight=lp)
        assert loss.shape == () and kl.shape == () and stats.shape == (5,)
    c = rc.ratio_case(3, 257, (0.2, 0.2))
    with pytest.raises(NotImplementedError):
        T.grpo_loss_ratio(c["logp"], c["old_logp"], c["ref_logp"], c["mask"], c["adv"], 0.04, False)


@pytest.mark.parametrize("fix_vit", [True, False])
def test_replay_on_unchanged_weights_reproduces_the_first_pass_gradient(tmp_path, fix_vit):
    """fp32 on the CPU: the two passes differ in summation order only (one decoder forward over P + G C rows against prefill + continuation), the bound the
    window tests of test_trainer_resume_and_windows.py use for the same kind of difference."""
    g1, g2, m = rc.first_pass_and_replay_grads(RefOps(), tmp_path, fix_vit)
    assert float(g1.abs().max()) > 0
    assert torch.allclose(g1, g2, atol=1e-6 * max(1.0, float(g1.abs().max())), rtol=1e-4), float((g1 - g2).abs().max())
    assert m["clip_ratio/region_mean"] == 0.0 and abs(m["policy_kl_old"]) < 1e-9


def test_two_updates_with_a_training_tower(tmp_path):
    tr = rc.tiny_trainer(RefOps(), load_case("clip_beta"), tmp_path, mu=2, ga=2, n_rows=2, fix_vit=False)
    a = tr.params.train
    lo, hi = a.offsets["patch.w"][0], a.master.numel()          # the tower's specs sit at the end of the trainable arena (params.arena_specs)
    rec = rc.run_recorded(tr)
    assert tr.state.global_step == 2 and rec["rollouts"] == 1
    assert float((rec["masters"][1][lo:hi] - rec["masters"][0][lo:hi]).abs().max()) > 0, "the replayed step must move the tower too"
    assert all(torch.isfinite(m).all() for m in rec["masters"])


def test_the_three_settings_parse_from_the_command_line(monkeypatch):
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
    monkeypatch.setattr(sys, "argv", ["train_grpo.py", "--num_iterations", "2", "--epsilon_low", "0.1", "--epsilon_high", "0.28", "--model_name_or_path", "m",
                                      "--train_data_path", "d"])
    with pytest.raises(Stop):
        train_grpo.main()
    a = seen["args"]
    assert (a.num_iterations, a.epsilon_low, a.epsilon_high) == (2, 0.1, 0.28)
    monkeypatch.setattr(sys, "argv", ["train_grpo.py", "--model_name_or_path", "m", "--train_data_path", "d"])
    with pytest.raises(Stop):
        train_grpo.main()
    a = seen["args"]
    assert (a.num_iterations, a.epsilon_low, a.epsilon_high) == (1, 0.2, None)
