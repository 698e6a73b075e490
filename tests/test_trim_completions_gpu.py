"""GRPOConfig.trim_completions on the MI355X: the sampler kernels' finished-row counter, the sampled rollout's early stop (native step and op-by-op step),
the trimmed update against the golden micro-step whose completions all end early, and a batched window whose update takes the saved-prefill continuation
path - option on against option off on the same tokens, both against the CPU oracle's fp32 values, and once with LoRA (step-0 KL exactly 0)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import frames_for, load_case, HF_GRAD_KEYS, pick_grad  # noqa: E402
import trim_cases as tc  # noqa: E402

I32 = torch.int32
NEW_KEY = "completions/trimmed_length"


# ------------------------------------------------------------------------------------------------------------------ 1. the counter
def _eos_logits(rows, V, eos, subset, seed):
    """bf16 [rows, V]: random logits; the EOS logit is 60 in the rows of `subset` (every other token's mass is below e^-50: the draw is EOS whatever the
    uniform) and -inf elsewhere (never drawn)."""
    x = torch.randn(rows, V, generator=torch.Generator().manual_seed(seed)).to(torch.bfloat16)
    x[:, eos] = float("-inf")
    x[sorted(subset), eos] = 60.0
    return x


@pytest.mark.parametrize("mode", ["plain", "step", "filtered", "filtered_step"])
@pytest.mark.parametrize("rows,V", [(1, 512), (5, 512), (16, 512), (64, 512), (5, 152064), (5, 515)])      # 515: the two-launch sum / pick pair
def test_sampler_counts_each_finished_row_once(hip_ops, rows, V, mode):
    ops = hip_ops
    eos, pad = V // 3, V + 5
    subset = {r for r in range(rows) if r % 3 == 0 or r == rows - 1}
    x = _eos_logits(rows, V, eos, subset, seed=rows + V).cuda()
    kw = dict(top_p=0.9, min_p=0.01) if mode.startswith("filtered") else {}
    want_fin = torch.tensor([int(r in subset) for r in range(rows)], dtype=I32)
    step0, step1 = (torch.tensor([s], dtype=I32, device="cuda") for s in (0, 1))

    def call(step, tokens, fin, stop, cnt):
        nxt = torch.full((rows,), -3, dtype=I32, device="cuda") if mode.endswith("step") else None
        ops.sample_tokens(x, 1.0, 50, 77, step, tokens, fin, eos, pad, stop, next_ids=nxt, done_count=cnt, **kw)
        return nxt
    for stop in (True, False):
        tokens = torch.full((rows, 3), -7, dtype=I32, device="cuda")
        fin = torch.zeros(rows, dtype=I32, device="cuda")
        cnt = torch.tensor([3], dtype=I32, device="cuda")
        nxt = call(step0, tokens, fin, stop, cnt)
        t = tokens.cpu()
        assert torch.equal(fin.cpu(), want_fin) and int(cnt) == 3 + len(subset), (int(cnt), len(subset))
        assert torch.equal(t[:, 0] == eos, want_fin.bool()) and bool((t[:, 1:] == -7).all())
        assert nxt is None or torch.equal(nxt.cpu(), t[:, 0])
        # the same tokens without the counter (the entry points the call stands for)
        tokens0 = torch.full((rows, 3), -7, dtype=I32, device="cuda")
        fin0 = torch.zeros(rows, dtype=I32, device="cuda")
        call(step0, tokens0, fin0, stop, None)
        assert torch.equal(tokens0.cpu(), t) and torch.equal(fin0.cpu(), want_fin)
        # a second call on the same logits: with stop_at_eos the finished rows are skipped (padding), without it they draw a second EOS - neither counts
        call(step1, tokens, fin, stop, cnt)
        t = tokens.cpu()
        assert int(cnt) == 3 + len(subset) and torch.equal(fin.cpu(), want_fin)
        assert torch.equal(t[:, 1] == (pad if stop else eos), want_fin.bool())
        assert not bool((t[~want_fin.bool(), 1] == eos).any())


# ------------------------------------------------------------------------------------------------------------------ 2. the early stop
@pytest.mark.parametrize("native", [True, False], ids=["native", "op-by-op"])
def test_sampled_early_stop_ends_the_loop_and_keeps_the_tokens(hip_ops, native):
    """test_greedy_decode_gpu.test_early_stop_ends_the_loop_and_keeps_the_tokens for greedy=False, top_k=1: 2 prompts x 4 rows, C = 64."""
    r = tc.early_stop_scenario(hip_ops, G=4, C=64, poll_every=4, native=native)
    print("sampled early stop (%s): rows end at %s, %d of %d decode steps enqueued" % ("native" if native else "op-by-op", r["ends"], r["n_early"], r["n_full"]))
    assert r["counted"], "the HIP sampler counts finished rows on the device"


# ------------------------------------------------------------------------------------------------------------------ 3. the golden
def test_trimmed_hip_trainer_vs_reference_golden(hip_ops):
    """The bounds of test_trainer_gpu.test_hip_trainer_vs_reference_golden on the fixture whose completions end at columns 8, 8, 5, 8 of 16."""
    fx = load_case(tc.SHORT)
    cfg, tr = tc.make_trainer(fx, hip_ops, trim_completions=True)
    frames = frames_for(fx)
    tr._video_inputs = lambda ex: ([frames], [2.0])
    calls = tc.spy_rows(tr)
    row = dict(fx["row"])
    row["_forced_completion_ids"] = fx["completion_ids"].numpy()
    loss = tr.compute_loss(tr.model, [row])
    P = len(fx["prompt_ids"])
    assert calls and all(rows == P + fx["G"] * 9 for _, rows, _ in calls), calls
    print("trimmed golden: loss %.6f (reference %.6f)" % (float(loss), float(fx["loss"])))
    assert abs(float(loss) - float(fx["loss"])) < 5e-3
    for k, v in fx["metrics"].items():
        tol = 5e-3 if k in ("kl",) else (0.05 if k == "generation_entropy" else 1e-6)
        print("  %s %.6f (reference %.6f)" % (k, tr._metrics[k][0], v[0]))
        assert abs(tr._metrics[k][0] - v[0]) <= tol, (k, tr._metrics[k], v)
    assert set(tr._metrics) == set(fx["metrics"]) | {NEW_KEY} and tr._metrics[NEW_KEY] == [9.0]
    assert tr.last_completions == fx["completions"]
    g = tr.params.train
    for hk, gold in fx["grads"].items():
        if hk in HF_GRAD_KEYS:
            mine = pick_grad(cfg, g.g, hk).float().cpu()
            rel = (mine - gold).norm() / gold.norm().clamp(min=1e-12)
            print("  grad %s relative L2 %.4f" % (hk, float(rel)))
            assert rel < 0.06, (hk, float(rel))


# ------------------------------------------------------------------------------------------------------------------ 4. the batched window
WINDOW_C = 32


def _window_rows(fx, base):
    rows = []
    for i in range(2):
        r = dict(fx["row"])
        r["problem"] = "event %d" % i
        r["video_frames"] = torch.randint(0, 256, (4, 3, 56, 84), generator=torch.Generator().manual_seed(base + i), dtype=torch.uint8).float()
        rows.append(r)
    return rows


def _window_trainer(fx, ops, eos, **over):
    cfg, tr = tc.make_trainer(fx, ops, ga=2, C=WINDOW_C, top_k=1, **over)
    tr._video_inputs = lambda ex: ([ex["video_frames"]], [2.0])
    tr.cfg.eos_token_id = tr.processing_class.eos_token_id = eos
    return cfg, tr


def _run_window(tr, rows):
    """-> dict(tokens per prompt, losses, metrics, named gradients, decoder calls, decode steps enqueued)."""
    toks, core = [], tr.core
    orig = core.rollout_many

    def many(states):
        out = orig(states)
        toks.extend(t.cpu().clone() for t in out)
        return out
    core.rollout_many = many
    calls = tc.spy_rows(tr)
    losses = [float(x) for x in tr.accumulation_window([[dict(r)] for r in rows])]
    return dict(tokens=toks, losses=losses, metrics={k: list(v) for k, v in tr._metrics.items()}, grads=tc.named_grads(tr), calls=calls,
                steps=core.roll.last_steps_run, arena=None if tr.lora is not None else tr.params.train.grad.detach().float().cpu().clone())


@functools.lru_cache(maxsize=None)
def _window_setup():
    """The EOS id of the window tests and the oracle's fp32 values, computed once.  The id comes from a rollout that stops nowhere (sampled, top_k = 1): the
    token that every row of both prompts holds within its first 24 columns and whose first occurrence comes latest; frame seeds are searched until there is one."""
    import time_r1_amd  # noqa: F401
    from time_r1_amd.ops import HipOps
    ops = HipOps("cuda:0")
    fx = load_case("clip_beta")
    for base in range(40, 60, 2):
        rows = _window_rows(fx, base)
        _, tr = _window_trainer(fx, ops, -1)
        states = [tr._step_prepare([dict(r)])["st"] for r in rows]
        tr.core.rollout_many(states)
        t = torch.cat([st.completion_ids.cpu() for st in states])
        # among the tokens every row holds within its first 24 columns, the one whose first occurrence comes latest: the longest live part that still trims
        firsts = {int(x): max(r.tolist().index(x) for r in t[:, :24]) for x in set(t[0, :24].tolist())
                  if x != tr.cfg.pad_token_id and all(x in r.tolist() for r in t[:, :24])}
        eos = max(firsts, key=lambda x: (firsts[x], -x)) if firsts else None
        if eos is not None:
            break
    assert eos is not None, "no frame seed whose rows share a token within their first columns"
    return fx, rows, eos


@functools.lru_cache(maxsize=None)
def _oracle_window(tokens_key):
    """The CPU oracle (fp32) on the GPU run's tokens, teacher-forced, option off."""
    from oracle.ref_ops import RefOps
    fx, rows, eos = _window_setup()
    tokens = [np.asarray(t, dtype=np.int32) for t in tokens_key]
    _, tr = _window_trainer(fx, RefOps(), eos, stop_at_eos=True)
    forced = []
    for r, t in zip(rows, tokens):
        r = dict(r)
        r["_forced_completion_ids"] = t
        forced.append(r)
    return _run_window(tr, forced)


def _check_against_oracle(name, run, gold, grads=True):
    for i, (a, b) in enumerate(zip(run["losses"], gold["losses"])):
        print("%s micro-step %d: loss %.6f (oracle %.6f)" % (name, i, a, b))
        assert abs(a - b) < 5e-3, (name, i, a, b)
    for k, v in gold["metrics"].items():
        tol = 5e-3 if k == "kl" else (0.05 if k == "generation_entropy" else 1e-6)
        for i, (a, b) in enumerate(zip(run["metrics"][k], v)):
            print("%s micro-step %d: %s %.6f (oracle %.6f)" % (name, i, k, a, b))
            assert abs(a - b) <= tol, (name, k, i, a, b)
    assert set(run["metrics"]) - {NEW_KEY} == set(gold["metrics"])
    if grads:
        for n, g in gold["grads"].items():
            rel = float((run["grads"][n] - g).norm() / g.norm().clamp(min=1e-12))
            print("%s: grad %s relative L2 to the oracle %.4f" % (name, n, rel))
            assert rel < 0.06, (name, n, rel)


def test_batched_window_on_the_continuation_path_on_against_off(hip_ops):
    fx, rows, eos = _window_setup()
    G, C = fx["G"], WINDOW_C
    _, tr_off = _window_trainer(fx, hip_ops, eos, stop_at_eos=True)
    off = _run_window(tr_off, rows)
    _, tr_on = _window_trainer(fx, hip_ops, eos, trim_completions=True)
    on = _run_window(tr_on, rows)
    assert len(on["tokens"]) == 2 and all(torch.equal(a, b) for a, b in zip(on["tokens"], off["tokens"])), "the early stop must not change a token"
    Ct = [min(C, max(8, int(tc.first_eos_lengths(t.numpy(), eos).max()))) for t in on["tokens"]]
    print("window: EOS id %d, trimmed lengths %s of %d, decode steps %d (on) / %d (off)" % (eos, Ct, C, on["steps"], off["steps"]))
    assert max(Ct) < C and on["metrics"][NEW_KEY] == [float(c) for c in Ct]
    assert off["steps"] == C - 1 and on["steps"] < C - 1
    # the update of prompt b: the policy's continuation over the saved prefill (row0 = P, G*Ct rows), the reference's one pass over P + G*Ct rows
    upd_on = [c for c in on["calls"] if c[2] > 0 or not c[0]]
    upd_off = [c for c in off["calls"] if c[2] > 0 or not c[0]]
    assert len(upd_on) == len(upd_off) == 4
    for b in range(2):
        (pol, rows_c, row0), (pol_r, rows_r, row0_r) = upd_on[2 * b], upd_on[2 * b + 1]
        assert pol and not pol_r and row0 > 0 and row0_r == 0
        assert rows_c == G * Ct[b] and rows_r == row0 + G * Ct[b], (upd_on, Ct)
        assert upd_off[2 * b][1] == G * C and upd_off[2 * b + 1][1] == row0 + G * C
    gold = _oracle_window(tuple(tuple(map(tuple, t.tolist())) for t in on["tokens"]))
    _check_against_oracle("option off", off, gold)
    _check_against_oracle("option on", on, gold)
    d = float((on["arena"] - off["arena"]).norm() / off["arena"].norm())
    print("window: gradient arena, option on against option off: relative L2 %.3e" % d)
    for k in off["metrics"]:
        print("window: %s on %s off %s" % (k, on["metrics"][k], off["metrics"][k]))


def test_batched_window_with_lora_keeps_step_zero_kl_exactly_zero(hip_ops):
    """peft_config r = 8 on q/v: the reference policy's forward repeats the policy's two launches (GRPOCore._ref_split_fwd) - on the trimmed rows too, with the
    prefill's own tail_from - so KL is exactly 0 before the adapters move."""
    fx, rows, eos = _window_setup()
    G, C = fx["G"], WINDOW_C
    _, tr = _window_trainer(fx, hip_ops, eos, trim_completions=True, peft=dict(r=8, lora_alpha=16, target_modules=["q_proj", "v_proj"]))
    run = _run_window(tr, rows)
    Ct = run["metrics"][NEW_KEY]
    print("LoRA window: trimmed lengths %s of %d, kl %s" % (Ct, C, run["metrics"]["kl"]))
    assert max(Ct) < C
    ref_cont = [c for c in run["calls"] if not c[0] and c[2] > 0]
    assert [c[1] for c in ref_cont] == [G * int(c) for c in Ct], "the reference's continuation runs on the trimmed rows"
    assert run["metrics"]["kl"] == [0.0, 0.0], run["metrics"]["kl"]
