"""GRPOConfig.trim_completions on the CPU oracle backend: the trimmed update against a golden micro-step of the unmodified reference whose completions all
end early (tests/golden/gen_short_golden.py), option on = option off wherever a row has no EOS, the replayed updates of num_iterations > 1 on the trimmed
rows, the sampled rollout's early stop, and the option's plumbing."""
import sys

import numpy as np
import pytest
import torch

from helpers import frames_for, CASES, load_case, HF_GRAD_KEYS, pick_grad, grads_cleared
import trim_cases as tc
from test_trainer_host_logic import make_trainer

NEW_KEY = "completions/trimmed_length"


def _forced_row(fx):
    row = dict(fx["row"])
    row["_forced_completion_ids"] = fx["completion_ids"].numpy()
    return row


def _step(fx, **over):
    cfg, tr = make_trainer(fx, **over)
    tr._video_inputs = lambda ex: ([frames_for(fx)], [2.0])
    calls = tc.spy_rows(tr)
    loss = tr.compute_loss(tr.model, [_forced_row(fx)])
    return cfg, tr, calls, loss


def test_trimmed_update_matches_the_reference_golden():
    """The reference ran all 16 columns; the trimmed update runs 9 (first EOS at 8, 8, 5, 8) and must give its loss, metrics and gradients at the tolerances of
    test_trainer_host_logic.test_compute_loss_matches_reference_golden, and its decoded completions exactly - those come from the full [G, C] rows (decoding
    9 columns would change `reward` from 0.4847 to 0.8805)."""
    fx = load_case(tc.SHORT)
    G, C = fx["G"], fx["C"]
    assert tc.first_eos_lengths(fx["completion_ids"].numpy(), 1).tolist() == [9, 9, 6, 9] and C == 16
    cfg, tr, calls, loss = _step(fx, trim_completions=True)
    P = len(fx["prompt_ids"])
    assert calls and all(rows == P + G * 9 and row0 == 0 for _, rows, row0 in calls), calls      # policy and reference forward alike
    assert {c[0] for c in calls} == {True, False}
    assert abs(float(loss) - float(fx["loss"])) < 2e-5
    for k, v in fx["metrics"].items():
        assert abs(tr._metrics[k][0] - v[0]) < 5e-5, (k, tr._metrics[k], v)
    assert set(tr._metrics) == set(fx["metrics"]) | {NEW_KEY} and tr._metrics[NEW_KEY] == [9.0]
    assert tr.last_completions == fx["completions"]
    g = tr.params.train
    for hk, gold in fx["grads"].items():
        if hk in HF_GRAD_KEYS:
            mine = pick_grad(cfg, g.g, hk)
            assert torch.allclose(mine, gold, atol=2e-5 * max(1.0, gold.abs().max().item()), rtol=2e-3), hk
    for tok, gold in fx["embed_grad_rows"].items():
        assert torch.allclose(g.g("embed")[tok], gold, atol=2e-5 * max(1.0, gold.abs().max().item()), rtol=2e-3), tok
    # the same fixture with the option off: the current code on all 16 columns
    cfg0, tr0, calls0, loss0 = _step(fx)
    assert all(rows == P + G * C for _, rows, _ in calls0) and NEW_KEY not in tr0._metrics
    assert abs(float(loss0) - float(fx["loss"])) < 2e-5


@pytest.mark.parametrize("case", CASES)
def test_option_on_equals_option_off_when_a_row_has_no_eos(case):
    """Every case of helpers.CASES keeps a row without EOS: Ct = C, nothing is trimmed, every value is the option-off run's bit for bit."""
    fx = load_case(case)
    assert int(tc.first_eos_lengths(fx["completion_ids"].numpy(), 1).max()) == fx["C"]
    _, tr1, calls1, loss1 = _step(fx, trim_completions=True)
    _, tr0, calls0, loss0 = _step(fx)
    assert calls1 == calls0
    assert float(loss1) == float(loss0)
    m1, m0 = dict(tr1._metrics), dict(tr0._metrics)
    assert m1.pop(NEW_KEY) == [float(fx["C"])] and m1 == m0
    assert torch.equal(tr1.params.train.grad, tr0.params.train.grad)
    assert tr1.last_completions == tr0.last_completions


def test_replay_runs_on_the_trimmed_rows():
    """num_iterations = 2: first pass, one optimizer step, then the replay - with the option on it runs on P + 4 * 9 rows and gives the option-off replay's loss
    and gradients at the tolerances of the golden test."""
    fx = load_case(tc.SHORT)
    P, G = len(fx["prompt_ids"]), fx["G"]
    out = {}
    for on in (True, False):
        cfg, tr = make_trainer(fx, num_iterations=2, learning_rate=1e-3, disable_log_print=True, **({"trim_completions": True} if on else {}))
        tr._video_inputs = lambda ex: ([frames_for(fx)], [2.0])
        calls = tc.spy_rows(tr)
        tr._reuse = []
        first = tr.accumulation_window([[_forced_row(fx)]])
        recs, tr._reuse = tr._reuse, None
        tr._optimizer_step(None, save=False)
        assert grads_cleared(tr)
        n_first = len(calls)
        losses = tr._replay_window(recs, more=False)
        replay_calls = calls[n_first:]
        assert replay_calls == [(True, P + G * (9 if on else fx["C"]), 0)], replay_calls       # one policy forward, no reference forward
        out[on] = (float(first[0]), float(losses[0]), tc.named_grads(tr), dict(tr.flush_metrics()), tr.state.log_history[0])
        assert recs[0]["old_logp"].shape == (G, fx["C"]) and recs[0]["mask"].shape == (G, fx["C"])
    assert abs(out[True][0] - out[False][0]) < 2e-5 and abs(out[True][1] - out[False][1]) < 2e-5
    assert out[True][1] != out[True][0], "the replay runs on moved weights"
    for n, gold in out[False][2].items():
        assert float(gold.abs().max()) > 0, n
        assert torch.allclose(out[True][2][n], gold, atol=2e-5 * max(1.0, gold.abs().max().item()), rtol=2e-3), n
    m1, m0 = out[True][3], out[False][3]
    assert set(m1) == set(m0) and NEW_KEY not in m1, "the replay logs no rollout-side key"
    assert out[True][4][NEW_KEY] == 9.0 and NEW_KEY not in out[False][4], "the first pass's log carries the new key, with the option on only"
    for k in m0:
        assert np.allclose(m1[k], m0[k], atol=5e-5, rtol=0), (k, m1[k], m0[k])


def test_sampled_rollout_stops_early_and_keeps_the_tokens(ref_ops):
    """The op-by-op step on the oracle backend, whose sample_tokens has no done_count: the poller sums the finished flags."""
    r = tc.early_stop_scenario(ref_ops, G=4, C=32, poll_every=4, n_layers=2)
    print("sampled early stop (oracle backend): rows end at %s, %d of %d decode steps enqueued" % (r["ends"], r["n_early"], r["n_full"]))
    assert not r["counted"]


def test_option_sets_stop_at_eos_and_parses_from_the_command_line(monkeypatch):
    import os
    from time_r1_amd.trainer import GRPOConfig
    a = GRPOConfig(trim_completions=True)
    assert a.trim_completions is True and a.stop_at_eos is True
    a = GRPOConfig()
    assert a.trim_completions is False and a.stop_at_eos is False
    fx = load_case("clip_beta")
    _, tr = make_trainer(fx, trim_completions=True)
    assert tr.core.trim_completions and tr.core.roll.early_stop and tr.core.roll.stop_at_eos
    _, tr = make_trainer(fx)
    assert not tr.core.trim_completions and not tr.core.roll.early_stop and not tr.core.roll.stop_at_eos
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
    monkeypatch.setattr(sys, "argv", ["train_grpo.py", "--trim_completions", "true", "--model_name_or_path", "m", "--train_data_path", "d"])
    with pytest.raises(Stop):
        train_grpo.main()
    assert seen["args"].trim_completions is True and seen["args"].stop_at_eos is True
    monkeypatch.setattr(sys, "argv", ["train_grpo.py", "--model_name_or_path", "m", "--train_data_path", "d"])
    with pytest.raises(Stop):
        train_grpo.main()
    assert seen["args"].trim_completions is False and seen["args"].stop_at_eos is False


def test_work_accounting_follows_the_rows_and_steps_run():
    """_count_update reads the trimmed layout, _count_decode the steps enqueued; at full length both give the figures they always gave."""
    fx = load_case(tc.SHORT)
    _, tr1, _, _ = _step(fx, trim_completions=True)
    _, tr0, _, _ = _step(fx)
    f1, f0 = tr1.core.work["train_flops"], tr0.core.work["train_flops"]
    assert 0 < f1 < f0
    core = tr0.core
    core.work = dict.fromkeys(core.work, 0.0)
    core._count_decode([20, 30])
    full = core.work["decode_bytes"]
    core.work = dict.fromkeys(core.work, 0.0)
    core._count_decode([20, 30], steps=core.C - 1)
    assert core.work["decode_bytes"] == full
    core.work = dict.fromkeys(core.work, 0.0)
    core._count_decode([20, 30], steps=3)
    assert 0 < core.work["decode_bytes"] < full
