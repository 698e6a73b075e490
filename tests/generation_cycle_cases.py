"""Scenarios for GRPOConfig.steps_per_generation (one rollout for k = steps_per_generation / GA accumulation windows, TimeR1_Trainer.generation_cycle; DESIGN.md
section 7u), shared by tests/test_generation_cycle_ref.py (the oracle op backend on the CPU) and tests/test_generation_cycle_gpu.py (HipOps).

The tiny trainer is ratio_cases.tiny_trainer (tiny_test / tiny_test_25 golden weights, G = 4, C = 8, GA = 2, a reward that varies inside a group); k = 2 unless a
scenario says otherwise, so 4 dataset rows make one cycle and 8 make two.  `run_recorded` trains with spies and returns what happened, in order: every scenario
reads that record."""
import json
import math
import os

import torch

import ratio_cases as rc
import recompute_cases as rcc
from helpers import load_case

GA = 2
FIXTURES = ("clip_beta", "q25_clip_beta_ragged")          # tiny_test, tiny_test_25; both run the clipped branch (use_grpo=False)
ROLLOUT_KEYS = ("reward", "reward_std", "completion_length", "rewards/varied_reward")


def cycle_trainer(ops, fx, out_dir, k=2, mu=1, n_rows=None, save_steps=0, **over):
    """k windows of GA = 2 per rollout (k None: the option left at None); n_rows defaults to one cycle's."""
    spg = {} if k is None else {"steps_per_generation": k * GA}
    return rc.tiny_trainer(ops, fx, out_dir, mu=mu, ga=GA, n_rows=n_rows or (k or 1) * GA, save_steps=save_steps, **spg, **over)


def run_recorded(tr, ckpt=None):
    """train() with spies -> dict:
    events   in call order: ("rollout", states), ("first", p) / ("score", p) for _step_score of prompt p (not deferred / deferred), ("reward", ),
             ("update", p, iteration of that prompt, an old_logp was passed), ("step", ), ("merge", ), ("save", global step)
    scored   p -> clone of the log-probs a deferred score left (taken when _step_score returned); old[p] -> clones of the old_logp of each later update
    tokw     p -> the tok_weight of each update that had an old_logp;   grads: clone of the gradient arena at each optimizer.step
    rollout  p -> the host metric values of its rollout;   tokens: p -> completion ids [G, C] on the host;   masters: after each step;   saves (prompts are
    numbered in the order they are prepared, over the whole run)."""
    rec = dict(events=[], scored={}, old={}, tokw={}, grads=[], rollout={}, tokens={}, masters=[], tokens_at_log=[], sample_calls=None)
    ev, core, order, n_upd = rec["events"], tr.core, {}, {}
    o_prep, o_many, o_score, o_lb, o_step, o_save = tr._step_prepare, core.rollout_many, tr._step_score, core.loss_backward, tr.optimizer.step, tr._save_checkpoint

    def prep(inputs):
        c = o_prep(inputs)
        order[id(c["st"])] = len(order)
        rec.setdefault("keep", []).append(c["st"])         # (ids stay unique while the states live)
        return c

    def many(states, **kw):
        ev.append(("rollout", len(states)))
        return o_many(states, **kw)

    def score(ctx, deferred=False):
        s = o_score(ctx, deferred=deferred)
        p = order[id(ctx["st"])]
        ev.append(("score" if deferred else "first", p))
        if deferred:
            rec["scored"][p] = ctx["st"].logp.detach().clone().cpu()
        rec["rollout"][p] = s["rollout"]
        host = ctx["st"].completion_ids_host          # (None for forced completions)
        rec["tokens"][p] = ctx["st"].completion_ids.cpu().numpy() if host is None else host.copy()
        return s

    def lb(st, *a, **k):
        p = order[id(st)]
        n_upd[p] = n_upd.get(p, 0) + 1
        old = k.get("old_logp")
        ev.append(("update", p, n_upd[p], old is not None))
        if old is not None:
            rec["old"].setdefault(p, []).append(old.detach().clone().cpu())
            tw = k.get("tok_weight")
            rec["tokw"].setdefault(p, []).append(None if tw is None else tw.detach().clone().cpu())
        return o_lb(st, *a, **k)

    def step(*a, **k):
        ev.append(("step",))
        g = (tr.lora.train if tr.lora is not None else tr.params.train).grad
        rec["grads"].append(g.detach().clone().cpu())
        return o_step(*a, **k)

    def save():
        ev.append(("save", tr.state.global_step))
        return o_save()

    def reward(fn):
        def f(*a, **k):
            ev.append(("reward",))
            return fn(*a, **k)
        f.__name__ = fn.__name__
        return f
    tr._step_prepare, core.rollout_many, tr._step_score, core.loss_backward, tr.optimizer.step, tr._save_checkpoint = prep, many, score, lb, step, save
    tr.reward_funcs = [reward(f) for f in tr.reward_funcs]
    if tr.lora is not None:
        o_merge = tr.lora.merge

        def merge(*a, **k):
            ev.append(("merge",))
            return o_merge(*a, **k)
        tr.lora.merge = merge

    class CB:
        def on_step_end(self, args, state, control, **kw):
            rec["masters"].append((tr.lora.train if tr.lora is not None else tr.params.train).master.detach().clone().cpu())

        def on_log(self, args, state, control, logs=None, **kw):
            rec["tokens_at_log"].append(tr.generated_tokens)
    tr.callbacks = [CB()]
    tr.train(resume_from_checkpoint=ckpt)
    rec["sample_calls"] = core.roll.calls
    rec.pop("keep", None)
    return rec


def names(ev):
    return [e[0] for e in ev]


def update_order(ev):
    """-> the (window, iteration) of the updates, 1-based, each window's GA micro-steps collapsed into one entry."""
    out = []
    for e in ev:
        if e[0] == "update":
            w = (e[1] // GA + 1, e[2])
            if not out or out[-1] != w:
                out.append(w)
    return out


# ---------------------------------------------------------------------------------------------------------------- 2. identity
def metric_keys(log):
    return {k for k in log if not k.startswith("perf/") and k not in ("samples_per_sec", "rollout_tokens_per_sec")}


def check_identity(ops, tmp_path):
    """steps_per_generation = GA against None, two optimizer steps: losses, gradient norms, metric key sets, final bf16 weights and the op-call sequence."""
    fx = load_case("clip_beta")
    runs = {}
    for name, k in (("none", None), ("ga", 1)):
        spy = rcc.Spy(ops)
        tr = cycle_trainer(spy, fx, tmp_path / name, k=k, n_rows=2 * GA)
        assert tr.args.steps_per_generation == (None if k is None else GA)
        rec = run_recorded(tr)
        assert tr.state.global_step == 2
        runs[name] = dict(calls=list(spy.calls), logs=tr.state.log_history, w16=rcc.bits(tr.params.train.w16), events=rec["events"])
    a, b = runs["none"], runs["ga"]
    assert len(a["calls"]) > 100 and a["calls"] == b["calls"]
    assert a["events"] == b["events"] and "score" not in names(a["events"])
    assert torch.equal(a["w16"], b["w16"])
    for la, lb in zip(a["logs"], b["logs"]):
        assert metric_keys(la) == metric_keys(lb) and set(la) == set(lb)
        assert la["loss"] == lb["loss"] and la["grad_norm"] == lb["grad_norm"]
        assert not [k for k in la if "score" in k]


# ---------------------------------------------------------------------------------------------------------------- 3. shape of a cycle
def check_cycle_shape(ops, tmp_path, fixture, exact_tokens):
    """k = 2, mu = 1: one rollout of 2 GA states (2 GA of one with rollout_group_rows at one prompt's rows, the same sampling streams), GA first-pass updates and
    GA scoring passes before the first optimizer step, GA replay-form updates after it, no reward call after it."""
    fx = load_case(fixture)
    tr = cycle_trainer(ops, fx, tmp_path / "one")
    rec = run_recorded(tr)
    ev = rec["events"]
    assert [e for e in ev if e[0] == "rollout"] == [("rollout", 2 * GA)]
    assert tr.state.global_step == 2 and names(ev).count("step") == 2
    s1 = names(ev).index("step")
    head, tail = ev[:s1], ev[s1 + 1:]
    assert [e for e in head if e[0] == "update"] == [("update", p, 1, False) for p in range(GA)]
    assert [e for e in head if e[0] in ("first", "score")] == [("first", p) for p in range(GA)] + [("score", p) for p in range(GA, 2 * GA)]
    assert [e for e in tail if e[0] == "update"] == [("update", p, 1, True) for p in range(GA, 2 * GA)]
    assert "reward" not in names(tail) and names(head).count("reward") == 2 * GA
    assert "first" not in names(tail) and "score" not in names(tail) and "rollout" not in names(tail)
    assert update_order(ev) == [(1, 1), (2, 1)]
    assert "perf/ms_score" in tr.state.log_history[0]
    # the same cycle decoded one prompt at a time
    tr1 = cycle_trainer(ops, fx, tmp_path / "single")
    tr1.rollout_group_rows = tr1.num_generations
    rec1 = run_recorded(tr1)
    assert [e for e in rec1["events"] if e[0] == "rollout"] == [("rollout", 1)] * (2 * GA)
    assert rec1["sample_calls"] == rec["sample_calls"] == 2 * GA
    assert [e for e in rec1["events"] if e[0] != "rollout"] == [e for e in ev if e[0] != "rollout"]
    assert tr1.state.global_step == 2
    if exact_tokens:      # (a backend whose decode kernels change with the row count may round a logit differently; the streams are the same either way)
        for p in range(2 * GA):
            assert (rec1["tokens"][p] == rec["tokens"][p]).all(), p
        # window 1's prompts sat in two groups here: each saved prefill kept its own buffer set and its own K/V cache, so the updates are the same
        for a, b in zip(rec1["masters"], rec["masters"]):
            assert torch.equal(a, b)
    return tr, rec


def check_iteration_major(ops, tmp_path):
    """k = 2, mu = 2: updates in the order (1,1), (2,1), (1,2), (2,2), 4 optimizer steps, one checkpoint at save_steps = 4; the replays run nothing of a rollout."""
    fx = load_case("clip_beta")
    tr = cycle_trainer(ops, fx, tmp_path, mu=2, save_steps=4)
    rec = run_recorded(tr)
    ev = rec["events"]
    assert update_order(ev) == [(1, 1), (2, 1), (1, 2), (2, 2)]
    assert tr.state.global_step == 4 and names(ev).count("step") == 4
    assert [e for e in ev if e[0] == "save"] == [("save", 4)]
    assert sorted(d for d in os.listdir(tmp_path) if d.startswith("checkpoint-")) == ["checkpoint-4"]
    s1 = names(ev).index("step")
    assert not [e for e in ev[s1 + 1:] if e[0] in ("reward", "first", "score", "rollout")]
    # every later update of a window is handed the same old policy: window 1 its first pass's log-probs, window 2 the scored ones
    for p in range(GA, 2 * GA):
        assert len(rec["old"][p]) == 2 and all(torch.equal(o, rec["scored"][p]) for o in rec["old"][p])
    for p in range(GA):
        assert len(rec["old"][p]) == 1
    return tr, rec


# ---------------------------------------------------------------------------------------------------------------- 4. the old policy
def check_old_policy(ops, tmp_path):
    """learning_rate > 0: the deferred window's loss reads the log-probs scored BEFORE the first optimizer step, its policy_kl_old is > 0 (the policy has moved),
    the first window's is exactly 0 (loss_type="bnpo" - the clip branch's own normaliser - puts the key into every log)."""
    fx = load_case("clip_beta")
    tr = cycle_trainer(ops, fx, tmp_path, loss_type="bnpo")
    assert tr.args.learning_rate > 0
    rec = run_recorded(tr)
    assert float((rec["masters"][1] - rec["masters"][0]).abs().max()) > 0
    for p in range(GA, 2 * GA):
        assert len(rec["old"][p]) == 1 and torch.equal(rec["old"][p][0], rec["scored"][p]), p
    for p in range(GA):
        assert p not in rec["old"] and p not in rec["scored"]
    logs = tr.state.log_history
    assert logs[0]["policy_kl_old"] == 0.0
    assert logs[1]["policy_kl_old"] > 0.0
    return tr, rec


# ---------------------------------------------------------------------------------------------------------------- 5. unmoved weights
def check_unmoved_weights(ops, tmp_path, fix_vit):
    """Weights held still (learning rate 0: AdamW adds exactly nothing), one k = 2 cycle; then the second window's prompts with its completions forced, in a
    plain trainer on the same weights.  -> (relative L2 distance of the cycle's second-window gradient to the plain one, the second window's log)."""
    fx = load_case("clip_beta")
    tr = cycle_trainer(ops, fx, tmp_path / "cycle", fix_vit=fix_vit)
    tr.args.learning_rate = 0.0
    w0 = tr.params.train.w16.detach().clone()
    in_order = cycle_rows_in_loader_order(tr)
    rec = run_recorded(tr)
    assert torch.equal(tr.params.train.w16, w0) and tr.state.global_step == 2
    g_cycle = rec["grads"][1]
    plain = cycle_trainer(ops, fx, tmp_path / "plain", k=None, n_rows=2 * GA, fix_vit=fix_vit)
    plain.args.learning_rate = 0.0
    rows = []
    for p in range(GA, 2 * GA):
        r = dict(in_order[p])
        r["_forced_completion_ids"] = rec["tokens"][p]
        rows.append(r)
    plain.train_dataset = rows
    plain.get_train_dataloader = lambda: _InOrder(rows)
    rec_p = run_recorded(plain)
    assert plain.state.global_step == 1 and "rollout" not in names(rec_p["events"])
    g_plain = rec_p["grads"][0]
    assert float(g_plain.norm()) > 0
    return float((g_cycle - g_plain).norm() / g_plain.norm()), tr.state.log_history[1]


class _InOrder:
    """A loader that yields the rows in their order, one per batch (the cycle's second window, in the order the cycle saw it)."""

    def __init__(self, rows):
        self.rows = rows

    def __len__(self):
        return len(self.rows)

    def skip_epochs(self, k):
        pass

    def __iter__(self):
        return iter([[r] for r in self.rows])


def cycle_rows_in_loader_order(tr):
    """The dataset rows in the order the trainer's loader yields them in its first epoch."""
    return [b[0] for b in tr.get_train_dataloader()]


# ---------------------------------------------------------------------------------------------------------------- 6. metrics
def check_metrics(ops, tmp_path):
    """k = 2, mu = 2 with the drift metric on: the rollout's keys come with each window's FIRST update and carry that window's own values; never on iteration 2;
    every completion's tokens are counted once."""
    fx = load_case("clip_beta")
    tr = cycle_trainer(ops, fx, tmp_path, mu=2, log_rollout_drift=True)
    rec = run_recorded(tr)
    logs = tr.state.log_history
    assert len(logs) == 4
    for w in range(2):
        ro = [rec["rollout"][p] for p in range(w * GA, (w + 1) * GA)]
        log = logs[w]
        for k in ROLLOUT_KEYS + ("rollout_logp_drift",):
            assert k in log and math.isfinite(log[k]), (w, k)
        assert abs(log["reward"] - sum(float(r["reward"].mean()) for r in ro) / GA) < 1e-5
        assert abs(log["completion_length"] - sum(float(r["length"].mean()) for r in ro) / GA) < 1e-4
        assert abs(log["rewards/varied_reward"] - sum(float(r["rpf"].mean()) for r in ro) / GA) < 1e-5
    r0, r1 = (sum(float(rec["rollout"][p]["reward"].mean()) for p in range(w * GA, (w + 1) * GA)) / GA for w in range(2))
    assert abs(r0 - r1) > 1e-4, "the two windows' rewards must differ for this test to tell them apart"
    for log in logs[2:]:
        assert not [k for k in log if k in ROLLOUT_KEYS or k == "rollout_logp_drift" or k.startswith("rewards/") or k == "rollout_tokens_per_sec"], log
        assert "policy_kl_old" in log and "loss" in log
    total = sum(float(rec["rollout"][p]["length"].sum()) for p in range(2 * GA))
    first = sum(float(rec["rollout"][p]["length"].sum()) for p in range(GA))
    assert rec["tokens_at_log"] == [first, total, total, total]
    assert tr.generated_tokens == total
    return tr, rec


# ---------------------------------------------------------------------------------------------------------------- 7. resume
def check_resume(ops, tmp_path, atol, **over):
    """Two cycles (8 rows, 4 optimizer steps), checkpoints at the cycle ends; checkpoint-2 resumed in a fresh trainer decodes one cycle and reaches step 4 on the
    straight run's weights."""
    fx = load_case("clip_beta")
    tr = cycle_trainer(ops, fx, tmp_path / "straight", n_rows=4 * GA, save_steps=2, **over)
    rec = run_recorded(tr)
    assert tr.state.global_step == 4 and tr.state.max_steps == 4 and abs(tr.state.epoch - 1.0) < 1e-9
    assert [e for e in rec["events"] if e[0] == "save"] == [("save", 2), ("save", 4)]
    assert [e for e in rec["events"] if e[0] == "rollout"] == [("rollout", 2 * GA)] * 2
    d = tmp_path / "straight" / "checkpoint-2"
    assert json.load(open(d / "trainer_state.json"))["global_step"] == 2
    tr2 = cycle_trainer(ops, fx, tmp_path / "resumed", n_rows=4 * GA, **over)
    rec2 = run_recorded(tr2, ckpt=str(d))
    assert tr2.state.global_step == 4 and len(rec2["masters"]) == 2
    assert [e for e in rec2["events"] if e[0] == "rollout"] == [("rollout", 2 * GA)]
    assert rec2["sample_calls"] == rec["sample_calls"] == 4 * GA
    for p in range(2 * GA):      # the resumed run's prompts 0 .. 3 are the straight run's 4 .. 7
        assert (rec2["tokens"][p] == rec["tokens"][2 * GA + p]).all()
    a, b = tr2.params.train.master.cpu(), tr.params.train.master.cpu()
    assert torch.allclose(a, b, atol=atol, rtol=0), float((a - b).abs().max())
    return tr, rec
