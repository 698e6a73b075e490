"""GRPOConfig.steps_per_generation on the MI355X: the scenarios of tests/generation_cycle_cases.py on HipOps, and the couplings that exist only there - LoRA
and an fp8 sampling policy with its importance cap."""
import math

import pytest
import torch

import generation_cycle_cases as gc
from helpers import load_case

pytestmark = pytest.mark.gpu
GA = gc.GA


def test_steps_per_generation_equal_to_ga_is_none_bit_for_bit(hip_ops, tmp_path):
    gc.check_identity(hip_ops, tmp_path)


@pytest.mark.parametrize("fixture", gc.FIXTURES)
def test_one_rollout_two_windows_scored_before_the_first_step(hip_ops, tmp_path, fixture):
    gc.check_cycle_shape(hip_ops, tmp_path, fixture, exact_tokens=False)


def test_two_iterations_run_iteration_major_with_one_checkpoint(hip_ops, tmp_path):
    gc.check_iteration_major(hip_ops, tmp_path)


def test_deferred_window_reads_the_old_policy(hip_ops, tmp_path):
    gc.check_old_policy(hip_ops, tmp_path)


@pytest.mark.parametrize("fix_vit", [True, False])
def test_unmoved_weights_reproduce_the_on_policy_gradient(hip_ops, tmp_path, fix_vit):
    """The bounds of test_policy_reuse_gpu.py::test_replay_on_unchanged_weights_reproduces_the_first_pass_gradient, for the same comparison: a replay forward
    (against log-probs scored in the replay's launches) and a first-pass forward, both in bf16."""
    rel, log = gc.check_unmoved_weights(hip_ops, tmp_path, fix_vit)
    print("relative L2 distance of the deferred window's gradient: %.3g, policy_kl_old %.3g, region %.3g" % (rel, log["policy_kl_old"], log["clip_ratio/region_mean"]))
    assert rel <= 0.06, rel
    assert log["clip_ratio/region_mean"] == 0.0 and log["policy_kl_old"] < 1e-3


def test_each_step_logs_its_own_windows_rollout_once(hip_ops, tmp_path):
    gc.check_metrics(hip_ops, tmp_path)


@pytest.mark.parametrize("trim", [False, True])
def test_resume_at_a_cycle_end(hip_ops, tmp_path, trim):
    """atol 2e-6: the bound of the resume tests on HipOps (atomics ordering in the embedding gradient)."""
    gc.check_resume(hip_ops, tmp_path, atol=2e-6, **({"trim_completions": True} if trim else {}))


# ---------------------------------------------------------------------------------------------------------------- 8. couplings
def test_lora_merges_after_every_step_of_a_cycle(hip_ops, tmp_path):
    import lora_cases as lc
    tr = lc.tiny_lora_trainer(hip_ops, load_case("clip_beta"), tmp_path, lc.QV, ga=GA, n_rows=2 * GA, steps_per_generation=2 * GA)
    assert tr.lora is not None and tr.lora_spec.r == 8
    rec = gc.run_recorded(tr)
    ev = gc.names(rec["events"])
    assert tr.state.global_step == 2 and gc.update_order(rec["events"]) == [(1, 1), (2, 1)]
    steps = [i for i, n in enumerate(ev) if n == "step"]
    assert len(steps) == 2 and all(ev[i + 1] == "merge" for i in steps) and ev.count("merge") == 2
    assert all(math.isfinite(l["loss"]) and math.isfinite(l["grad_norm"]) for l in tr.state.log_history)
    assert float((rec["masters"][1] - rec["masters"][0]).abs().max()) > 0
    for p in range(GA, 2 * GA):
        assert torch.equal(rec["old"][p][0], rec["scored"][p])


def test_fp8_sampling_policy_caps_the_deferred_windows_importance_weight(hip_ops, tmp_path):
    tr = gc.cycle_trainer(hip_ops, load_case("clip_beta"), tmp_path, rollout_weight_dtype="fp8")
    cap = tr._is_cap
    assert cap is not None and tr.core.roll.track_logp
    scored_w = {}
    o_score = tr._step_score

    def score(ctx, deferred=False):
        st = ctx["st"]
        s = o_score(ctx, deferred=deferred)
        if deferred:      # the weight from the SCORED log-probs: min(exp(scored logp - sampling logp), cap)
            scored_w[id(st)] = (s["tokw"].detach().clone().cpu(), torch.exp(st.logp.float() - st.sample_logp.to(st.logp.device).float()).clamp(max=cap).cpu())
        return s
    tr._step_score = score
    rec = gc.run_recorded(tr)
    assert tr.state.global_step == 2 and len(scored_w) == GA
    for got, want in scored_w.values():
        assert torch.equal(got, want)
    seen = [w for p in range(GA, 2 * GA) for w in rec["tokw"][p]]
    assert len(seen) == GA
    for w, (got, _) in zip(seen, scored_w.values()):
        assert w is not None and w.dtype == torch.float32 and float(w.max()) <= cap and float(w.min()) > 0
        assert torch.equal(w, got)
    logs = tr.state.log_history
    assert all(math.isfinite(l["loss"]) and math.isfinite(l["grad_norm"]) for l in logs)
    assert "rollout_logp_drift" in logs[0] and "rollout_logp_drift" in logs[1]
