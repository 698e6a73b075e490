"""What the trainer logs against what its loss calls returned: the key set of every log line and the values of the device-side metrics, for a first pass and a
replay, with and without an objective.  Shared by tests/test_metric_record_ref.py (CPU) and tests/test_metric_record_gpu.py (HipOps on the same tiny model).

GRPOCore.loss_backward returns [loss, mean kl, sum mask] or, from the ratio / policy kernels, [loss, mean kl, sum mask, clip low, clip high, clip region, k3 to the
old policy, largest ratio].  A log line averages the micro-steps of its optimizer step, so with one rank
  kl = mean of slot 1, clip_ratio/low_mean | high_mean | region_mean = mean of slots 3 | 4 | 5, policy_kl_old = mean of slot 6,
  rollout_logp_drift = mean of sum(|logp - sample_logp| mask) / sum(mask)
over that step's calls.  These are the same fp32 numbers averaged on the host: rel. 1e-6.
"""
import pytest
import torch

import ratio_cases as rc

GA = 2
COMMON = {"loss", "grad_norm", "learning_rate", "epoch", "step", "generation_entropy", "kl"}
ROLLOUT = {"completion_length", "rewards/varied_reward", "reward", "reward_std"}
CLIP = {"clip_ratio/low_mean", "clip_ratio/low_min", "clip_ratio/high_mean", "clip_ratio/high_max", "clip_ratio/region_mean"}
DRIFT, KL_OLD = {"rollout_logp_drift"}, {"policy_kl_old"}
SLOT_OF = {"kl": 1, "clip_ratio/low_mean": 3, "clip_ratio/high_mean": 4, "clip_ratio/region_mean": 5, "policy_kl_old": 6}

# (fixture, num_iterations, settings, the key set of each log line)
SETTINGS = (
    ("clip_beta", 2, dict(log_rollout_drift=True), (COMMON | ROLLOUT | DRIFT, COMMON | CLIP | KL_OLD)),
    ("clip_beta", 2, dict(loss_type="dr_grpo", rollout_importance_cap=2.0), (COMMON | ROLLOUT | CLIP | KL_OLD | DRIFT, COMMON | CLIP | KL_OLD)),
    ("grpo_beta", 1, dict(), (COMMON | ROLLOUT,)),
)


def metric_keys(log):
    return {k for k in log if not k.startswith("perf/") and k not in ("samples_per_sec", "rollout_tokens_per_sec")}


def check_logged_values_are_the_loss_calls(ops, tmp_path):
    from helpers import load_case
    for n, (case, mu, over, want_keys) in enumerate(SETTINGS):
        tr = rc.tiny_trainer(ops, load_case(case), tmp_path / ("run%d" % n), mu=mu, ga=GA, n_rows=2, **over)
        calls, inner = [], tr.core.loss_backward

        def spy(st, mask, *a, **k):
            seen = dict(logp=st.logp.detach().float().cpu().clone(), mask=mask.detach().float().cpu().clone(),
                        sample_logp=None if st.sample_logp is None else st.sample_logp.detach().float().cpu().clone())
            out = inner(st, mask, *a, **k)
            seen["vec"] = out[0].detach().float().cpu().clone()
            calls.append(seen)
            return out
        tr.core.loss_backward = spy
        tr.train()
        logs = tr.state.log_history
        assert len(logs) == len(want_keys) == mu and len(calls) == GA * mu, (case, len(logs), len(calls))
        for step, (log, want) in enumerate(zip(logs, want_keys)):
            assert metric_keys(log) == want, (case, step, sorted(metric_keys(log) ^ want))
            mine = calls[GA * step:GA * (step + 1)]
            assert len({c["vec"].numel() for c in mine}) == 1 and mine[0]["vec"].numel() in (3, 8)
            for key, slot in SLOT_OF.items():
                if key in want:
                    exp = sum(float(c["vec"][slot]) for c in mine) / GA
                    print("OBS %s step %d %-24s logged %.9g, loss calls %.9g" % (case, step, key, log[key], exp))
                    assert log[key] == pytest.approx(exp, rel=1e-6), (case, step, key)
            if "rollout_logp_drift" in want:
                exp = sum(float(((c["logp"] - c["sample_logp"]).abs() * c["mask"]).sum() / c["mask"].sum().clamp(min=1)) for c in mine) / GA
                print("OBS %s step %d %-24s logged %.9g, loss calls %.9g" % (case, step, "rollout_logp_drift", log["rollout_logp_drift"], exp))
                assert log["rollout_logp_drift"] == pytest.approx(exp, rel=1e-6), (case, step)
