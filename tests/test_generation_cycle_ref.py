"""GRPOConfig.steps_per_generation on the CPU: configuration rules, and the generation cycle's scenarios (tests/generation_cycle_cases.py) on the oracle op
backend.  tests/test_generation_cycle_gpu.py runs the same scenarios on HipOps."""
import re

import pytest
import torch

import generation_cycle_cases as gc
import ratio_cases as rc
from helpers import load_case
from oracle.ref_ops import RefOps
from time_r1_amd.trainer import GRPOConfig


# ---------------------------------------------------------------------------------------------------------------- 1. validation
def test_config_rules_name_their_values():
    assert GRPOConfig().steps_per_generation is None
    assert GRPOConfig(gradient_accumulation_steps=2, steps_per_generation=2).steps_per_generation == 2
    assert GRPOConfig(gradient_accumulation_steps=2, steps_per_generation="4").steps_per_generation == 4
    for bad in (0, -2, 1.5, "two", True):
        with pytest.raises(ValueError, match="steps_per_generation must be None or an integer >= 1, got " + re.escape(repr(bad))):
            GRPOConfig(steps_per_generation=bad)
    with pytest.raises(ValueError, match=r"steps_per_generation \(3\) must be a multiple of gradient_accumulation_steps \(2\)"):
        GRPOConfig(gradient_accumulation_steps=2, steps_per_generation=3)
    with pytest.raises(ValueError, match=r"steps_per_generation \(1\) .*gradient_accumulation_steps \(2\).*more than once per window is not offered"):
        GRPOConfig(gradient_accumulation_steps=2, steps_per_generation=1)
    with pytest.raises(ValueError, match=r"steps_per_generation = 4 with gradient_accumulation_steps = 2 .*use_grpo=True"):
        GRPOConfig(gradient_accumulation_steps=2, steps_per_generation=4, use_grpo=True)
    with pytest.raises(ValueError, match=r"steps_per_generation = 4 with gradient_accumulation_steps = 2 .*rollout_batching=True"):
        GRPOConfig(gradient_accumulation_steps=2, steps_per_generation=4, rollout_batching=False)
    with pytest.raises(ValueError, match=r"save_steps \(6\) must be a multiple of .* 2 x 2 = 4"):
        GRPOConfig(gradient_accumulation_steps=2, steps_per_generation=4, num_iterations=2, save_steps=6)
    with pytest.raises(ValueError, match=r"ref_model_sync_steps \(6\) must be a multiple of .* 2 x 2 = 4"):
        GRPOConfig(gradient_accumulation_steps=2, steps_per_generation=4, num_iterations=2, save_steps=4, sync_ref_model=True, ref_model_sync_steps=6)
    # neither cadence binds where it is not in force, and k = 1 binds nothing
    GRPOConfig(gradient_accumulation_steps=2, steps_per_generation=4, save_steps=3, save_strategy="no", ref_model_sync_steps=3)
    GRPOConfig(gradient_accumulation_steps=2, steps_per_generation=2, save_steps=3, use_grpo=True, rollout_batching=False)
    GRPOConfig(gradient_accumulation_steps=2, steps_per_generation=4, save_steps=4, sync_ref_model=True, ref_model_sync_steps=4)


def test_trainer_checks_again_at_construction_and_at_train(tmp_path):
    ops, fx = RefOps(), load_case("clip_beta")
    assert gc.cycle_trainer(ops, fx, tmp_path, k=None)._check_generation_args() == 1
    assert gc.cycle_trainer(ops, fx, tmp_path, k=1)._check_generation_args() == 1
    tr = gc.cycle_trainer(ops, fx, tmp_path, k=2)
    assert tr._check_generation_args() == 2
    tr.args.steps_per_generation = 3                      # args is mutable: construction passed, train() checks again
    with pytest.raises(ValueError, match=r"steps_per_generation \(3\) must be a multiple"):
        tr.train()
    tr = gc.cycle_trainer(ops, fx, tmp_path, k=2, mu=1, save_steps=2)
    tr.num_iterations = 2                                 # the trainer's own num_iterations is what the cadence is checked against
    with pytest.raises(ValueError, match=r"save_steps \(2\) must be a multiple of .* 2 x 2 = 4"):
        tr.train()
    with pytest.raises(ValueError, match="use_grpo=True"):
        args = rc.tiny_trainer(ops, fx, tmp_path, mu=1).args
        args.steps_per_generation, args.use_grpo = 4, True
        from time_r1_amd.trainer import generation_windows
        generation_windows(args)
    # an epoch of 2 rows is one window of GA = 2: shorter than a cycle of 2 windows
    tr = gc.cycle_trainer(ops, fx, tmp_path, k=2, n_rows=2)
    with pytest.raises(ValueError, match=r"steps_per_generation = 4 is 2 accumulation windows of 2 micro-steps, and an epoch holds 1"):
        tr.train()
    with pytest.raises(ValueError, match=r"generation_cycle got 1 window\(s\); steps_per_generation = 4 .* makes 2"):
        gc.cycle_trainer(ops, fx, tmp_path, k=2).generation_cycle([[]])


def test_flag_parses_from_the_command_line(monkeypatch):
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
    base = ["train_grpo.py", "--model_name_or_path", "m", "--train_data_path", "d", "--gradient_accumulation_steps", "2"]
    monkeypatch.setattr(sys, "argv", base + ["--steps_per_generation", "4"])
    with pytest.raises(Stop):
        train_grpo.main()
    assert seen["args"].steps_per_generation == 4
    monkeypatch.setattr(sys, "argv", base)
    with pytest.raises(Stop):
        train_grpo.main()
    assert seen["args"].steps_per_generation is None
    monkeypatch.setattr(sys, "argv", base + ["--steps_per_generation", "3"])
    with pytest.raises(ValueError, match="multiple of gradient_accumulation_steps"):
        train_grpo.main()


# ---------------------------------------------------------------------------------------------------------------- 2 .. 7 on the oracle backend
def test_steps_per_generation_equal_to_ga_is_none_bit_for_bit(tmp_path):
    gc.check_identity(RefOps(), tmp_path)


@pytest.mark.parametrize("fixture", gc.FIXTURES)
def test_one_rollout_two_windows_scored_before_the_first_step(tmp_path, fixture):
    gc.check_cycle_shape(RefOps(), tmp_path, fixture, exact_tokens=True)


def test_two_iterations_run_iteration_major_with_one_checkpoint(tmp_path):
    gc.check_iteration_major(RefOps(), tmp_path)


def test_deferred_window_reads_the_old_policy(tmp_path):
    gc.check_old_policy(RefOps(), tmp_path)


@pytest.mark.parametrize("fix_vit", [True, False])
def test_unmoved_weights_reproduce_the_on_policy_gradient(tmp_path, fix_vit):
    """The bounds of test_replay_on_unchanged_weights_reproduces_the_first_pass_gradient on HipOps (0.06, 1e-3), for the same comparison - a replay forward
    against a first-pass forward; fp32 on the CPU sits far inside them."""
    rel, log = gc.check_unmoved_weights(RefOps(), tmp_path, fix_vit)
    print("relative L2 distance of the deferred window's gradient: %.3g, policy_kl_old %.3g" % (rel, log["policy_kl_old"]))
    assert rel <= 0.06, rel
    assert log["clip_ratio/region_mean"] == 0.0 and log["policy_kl_old"] < 1e-3


def test_each_step_logs_its_own_windows_rollout_once(tmp_path):
    gc.check_metrics(RefOps(), tmp_path)


@pytest.mark.parametrize("trim", [False, True])
def test_resume_at_a_cycle_end(tmp_path, trim):
    gc.check_resume(RefOps(), tmp_path, atol=2e-6, **({"trim_completions": True} if trim else {}))


def test_stop_inside_a_cycle_ends_after_that_step(tmp_path):
    """max_steps = 1 with k = 2: the cycle's first optimizer step is the last; the scored window is dropped."""
    tr = gc.cycle_trainer(RefOps(), load_case("clip_beta"), tmp_path, max_steps=1)
    rec = gc.run_recorded(tr)
    assert tr.state.global_step == 1 and gc.names(rec["events"]).count("step") == 1
    assert gc.update_order(rec["events"]) == [(1, 1)]


def test_trailing_windows_of_an_epoch_are_dropped(tmp_path, capsys):
    """6 rows, GA = 2, k = 2, two epochs: 3 windows an epoch, one cycle, steps_per_epoch = 2; the third window fills no cycle and no cycle spans the epochs."""
    tr = gc.cycle_trainer(RefOps(), load_case("clip_beta"), tmp_path, n_rows=6, epochs=2)
    rec = gc.run_recorded(tr)
    assert tr.state.global_step == 4 and tr.state.max_steps == 4 and tr._steps_per_epoch == 2 and abs(tr.state.epoch - 2.0) < 1e-9
    assert [e for e in rec["events"] if e[0] == "rollout"] == [("rollout", 4)] * 2
    assert rec["sample_calls"] == 8
    assert "epoch 0: 1 trailing window(s) do not fill a generation cycle of 2" in capsys.readouterr().out


def test_scoring_form_saves_nothing_and_matches_the_replay_forward():
    """forward_logps(score=True) against forward_logps(replay=True) on the same weights: the same log-probs bit for bit, no saved context."""
    import numpy as np
    import recompute_cases as rcc
    from time_r1_amd.positions import PackedLayout
    ops = RefOps()
    cfg, pol, eng, core = rcc.build(ops, None, beta=0.04)
    ids, pix, g3 = rcc.prompt_for(cfg, 70)
    toks, _, _ = rcc.forced_inputs(4, 24)
    states = []
    for _ in range(2):
        st = core.prepare(ids, pix, g3)
        st.layout = PackedLayout(st.P, 4, 24)
        st.completion_ids = ops.tensor(toks.numpy(), torch.int32)
        states.append(st)
    a, b = states
    core.forward_logps(a, score=True)
    assert a.llm_ctx is None and a.head_ctx is None and a.merger_ctx is None and a.vid_embeds is None and a.ref_logp is not None
    core.forward_logps(b)
    core.forward_logps(b, replay=True)
    assert torch.equal(a.logp, b.logp) and torch.equal(a.entropy, b.entropy) and torch.equal(a.ref_logp, b.ref_logp)
    assert np.isfinite(a.logp.numpy()).all()
