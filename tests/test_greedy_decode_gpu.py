"""Batched greedy decoding with early stop on the MI355X: the one-launch argmax kernel against torch (exact), the batched evaluation against the CPU
oracle's logits, determinism (run to run, native step against op-by-op), the early stop, and many prompts x one row at full 7B width."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------------ 1. the kernel
def _planted_logits(rows, V, ld, off, shift, eos, seed):
    """-> (flat bf16 buffer on the host, view [rows, V] with row stride ld starting `off` elements in, finished flags).  Row r is of kind (r + shift) % 8:
    0 maximum duplicated at several indices, 1 maximum at index 0, 2 maximum at V - 1, 3 -inf everywhere except one entry, 4 finished on entry,
    5 maximum at eos, 6 -inf everywhere, 7 plain random (bf16 random rows have natural ties at the maximum as well)."""
    g = torch.Generator().manual_seed(seed)
    flat = torch.randn(off + rows * ld, generator=g).to(torch.bfloat16)
    x = flat.as_strided((rows, V), (ld, 1), off)
    finished = torch.zeros(rows, dtype=torch.int32)
    for r in range(rows):
        kind = (r + shift) % 8
        if kind == 0:
            idx = torch.randint(0, V, (5,), generator=g)
            x[r, idx] = 9.0
        elif kind == 1:
            x[r, 0] = 9.5
        elif kind == 2:
            x[r, V - 1] = 9.5
        elif kind == 3:
            keep = float(x[r, V // 2])
            x[r] = float("-inf")
            x[r, V // 2] = keep
        elif kind == 4:
            finished[r] = 1
            x[r] = float("nan")          # a finished row's logits are never looked at
        elif kind == 5:
            x[r, eos] = 11.0
        elif kind == 6:
            x[r] = float("-inf")
    return flat, x, finished


@pytest.mark.parametrize("rows,V,ld,off", [(1, 1, 8, 0), (3, 515, 520, 0), (16, 151936, 151936, 0), (64, 152064, 152064, 0), (5, 1031, 1040, 1),
                                           (6, 300, 301, 1), (4, 7, 7, 3), (9, 8, 8, 0), (8, 4099, 4104, 7)])
def test_greedy_kernel_equals_torch_argmax_lowest_index(hip_ops, rows, V, ld, off):
    ops = hip_ops
    eos, pad, step, ncol = V // 3, V + 5, 2, 5
    for shift in (range(8) if rows < 8 else (0,)):
        flat, x, fin0 = _planted_logits(rows, V, ld, off, shift, eos, seed=1000 * rows + shift)
        xf = x.float()
        want = (xf == xf.max(1, keepdim=True).values).int().argmax(1).to(torch.int32)       # lowest index among the maxima
        live = fin0 == 0
        want = torch.where(live, want, torch.full_like(want, pad))
        want_fin = (fin0.bool() | (live & (want == eos))).to(torch.int32)
        newly = int((live & (want == eos)).sum())
        d_flat = flat.cuda()
        d_x = d_flat.as_strided((rows, V), (ld, 1), off)
        assert d_x.data_ptr() % 16 == (2 * off) % 16
        step_dev = torch.tensor([step], dtype=torch.int32, device="cuda")
        for with_opt in (True, False):
            tokens = torch.full((rows, ncol), -7, dtype=torch.int32, device="cuda")
            fin = fin0.cuda()
            nxt = torch.full((rows,), -3, dtype=torch.int32, device="cuda") if with_opt else None
            cnt = torch.tensor([3], dtype=torch.int32, device="cuda") if with_opt else None
            ops.greedy_tokens(d_x, step_dev, tokens, fin, eos, pad, next_ids=nxt, done_count=cnt)
            torch.cuda.synchronize()
            t = tokens.cpu()
            assert torch.equal(t[:, step], want), (shift, t[:, step].tolist(), want.tolist())
            assert bool((t[:, [c for c in range(ncol) if c != step]] == -7).all()), "other token columns must stay untouched"
            assert torch.equal(fin.cpu(), want_fin)
            if with_opt:
                assert torch.equal(nxt.cpu(), want) and int(cnt) == 3 + newly
        assert torch.equal(d_flat.cpu().view(torch.int16), flat.view(torch.int16)), "logits are read only"


# ------------------------------------------------------------------------------------------------------------------ 2. against the oracle
def _eval_rows(fx, n):
    rows = []
    for i in range(n):
        r = dict(fx["row"])
        r["problem"] = "event %d" % i
        r["video_frames"] = torch.randint(0, 256, (4, 3, 56, 84), generator=torch.Generator().manual_seed(700 + i), dtype=torch.uint8).float()
        rows.append(r)
    return rows


def test_batched_greedy_evaluation_checked_against_oracle_logits(hip_ops, ref_ops):
    """evaluate_grounding(batch_size=4) on 5 rows (one full batch, one short batch), judged like the one-row path in test_configs_gpu.py: the HIP tokens are
    teacher-forced through the oracle engine; every token up to and including EOS has an oracle logit within 0.05 of its row's oracle maximum, everything
    after EOS is padding, text and IoU equal what the same tokens give on the oracle side.  Tokens need not equal the batch_size=1 run (the decode GEMMs
    pick kernel forms by row count); how many differ is printed."""
    from helpers import load_case
    from test_configs_gpu import _tiny_trainer
    from time_r1_amd import evaluate as E
    from time_r1_amd.grpo import GRPOCore
    from time_r1_amd.positions import PackedLayout
    C = 10
    fx = load_case("grpo_beta")
    cfg, tr = _tiny_trainer(hip_ops, fx, ga=1)
    rows = _eval_rows(fx, 5)
    tr._video_inputs = lambda ex: ([ex["video_frames"]], [2.0])
    seen, sizes = [], []
    orig = GRPOCore.rollout_many

    def spy(self, states):
        assert self.roll.greedy and self.G == 1
        toks = orig(self, states)
        sizes.append(len(states))
        seen.extend((st.prompt_ids_host.copy(), t.cpu().clone()) for st, t in zip(states, toks))
        return toks
    GRPOCore.rollout_many = spy
    try:
        metrics, records = E.evaluate_grounding(tr, rows, max_new_tokens=C, batch_size=4)
        n4 = len(seen)
        _, records1 = E.evaluate_grounding(tr, rows, max_new_tokens=C, batch_size=1)
    finally:
        GRPOCore.rollout_many = orig
    assert sizes[:2] == [4, 1] and n4 == 5 and len(records) == 5 and [r["index"] for r in records] == list(range(5))
    assert set(metrics) == {"mIoU", "R1@0.3", "R1@0.5", "R1@0.7", "avg"}
    differ = sum(int((a[1] != b[1]).sum()) for a, b in zip(seen[:5], seen[5:]))
    print("batched greedy evaluation: %d of %d tokens differ between batch_size=4 and batch_size=1" % (differ, 5 * C))
    cfg_r, tr_r = _tiny_trainer(ref_ops, fx, ga=1)
    core = GRPOCore(tr_r.engine, None, 1, C, beta=0.0, temperature=1.0, top_k=1, seed=0, rope_index_mode=tr.args.rope_index_mode, reuse_prefill=False)
    worst = 0.0
    for (ids, toks), row, rec in zip(seen[:5], rows, records):
        pi = tr_r.processing_class(text=["PROMPT"], videos=[row["video_frames"]], fps=[2.0])
        st = core.prepare(np.asarray(pi["input_ids"]).reshape(-1), pi["pixel_values_videos"], np.asarray(pi["video_grid_thw"]))
        assert np.array_equal(st.prompt_ids_host, ids)
        t = toks.clone()
        assert t.shape == (1, C)
        eos = (t[0] == cfg.eos_token_id).nonzero()
        n_valid = int(eos[0]) + 1 if len(eos) else C
        assert bool((t[0, n_valid:] == cfg.pad_token_id).all()), "positions after EOS must be padding"
        st.layout = PackedLayout(st.P, 1, C)
        st.completion_ids = t.clone()
        core.forward_logps(st)
        logits = st.head_ctx["logits"].float()            # pred-row order: the first-token row, then steps s >= 1
        for s in range(n_valid):
            row_l = logits[0] if s == 0 else logits[1 + (s - 1)]
            gap = float(row_l.max() - row_l[int(t[0, s])])
            worst = max(worst, gap)
            print("row %d step %d: oracle max - oracle logit of the HIP token = %.4f" % (rec["index"], s, gap))
            assert gap < 0.05, (rec["index"], s, gap)
        completion = tr_r.processing_class.batch_decode(t, skip_special_tokens=True)[0]
        assert completion == rec["completion"]
        assert rec["iou"] == E.compute_iou(E.extract_answer_span(completion), row["solution"])
    print("worst gap %.4f" % worst)


# ------------------------------------------------------------------------------------------------------------------ 3. determinism
def _tiny_engine(ops, inter=256):
    import time_r1_amd  # noqa: F401
    from time_r1_amd.config import tiny_test
    from time_r1_amd.params import ModelParams
    from time_r1_amd.model import Engine
    cfg = tiny_test(n_layers=3)
    cfg.text.intermediate = inter
    params = ModelParams(cfg, ops, seed=1)
    return cfg, Engine(cfg, ops, params)


def _greedy_core(eng, C, poll_every=8, native=True):
    from time_r1_amd.grpo import GRPOCore
    core = GRPOCore(eng, None, 1, C, beta=0.0, seed=5, rope_index_mode="hf4", reuse_prefill=False, greedy=True)
    core.roll.poll_every = poll_every
    core.roll.native_decode = native
    return core


def _prompt(cfg, core, seed, extra=0):
    from time_r1_amd.synthetic import synthetic_prompt
    return core.prepare(*synthetic_prompt(cfg, (4, 6, 8), 9, 7 + extra, seed=seed, text_vocab=400))


@pytest.mark.parametrize("B,inter", [(3, 256), (16, 8192)])      # 16 rows x intermediate 8192: the split-K fix-up down projection
def test_greedy_tokens_repeat_and_native_equals_op_by_op(hip_ops, B, inter):
    cfg, eng = _tiny_engine(hip_ops, inter)
    used = []
    orig = hip_ops.greedy_tokens

    def spy(*a, **k):
        used.append(1)
        return orig(*a, **k)
    hip_ops.greedy_tokens = spy
    outs = []
    try:
        for native in (True, True, False):
            core = _greedy_core(eng, 12, native=native)
            toks = core.rollout_many([_prompt(cfg, core, 2 + b, extra=b % 3) for b in range(B)])
            outs.append(torch.stack([t.cpu() for t in toks]))
    finally:
        del hip_ops.greedy_tokens
    assert len(used) >= 3 * B, "greedy mode must select tokens with the greedy kernel"
    assert torch.equal(outs[0], outs[1]), "the same batch twice"
    assert torch.equal(outs[0], outs[2]), "native decode step against the op-by-op loop"
    assert outs[0].shape == (B, 1, 12) and outs[0].min() >= 0 and outs[0].max() < cfg.text.vocab_size
    assert len({tuple(o.reshape(-1).tolist()) for o in outs[0]}) > 1, "different prompts should not all decode alike"


# ------------------------------------------------------------------------------------------------------------------ 4. early stop
def test_early_stop_ends_the_loop_and_keeps_the_tokens(hip_ops):
    C = 64
    cfg, eng = _tiny_engine(hip_ops)
    pad = cfg.pad_token_id

    def run(seeds, poll_every):
        core = _greedy_core(eng, C, poll_every=poll_every)
        toks = core.rollout_many([_prompt(cfg, core, sd) for sd in seeds])
        return torch.cat([t.cpu() for t in toks]), core.roll.last_steps_run
    old_eos = cfg.eos_token_id
    try:
        cfg.eos_token_id = -1          # no id ends a row: the plain greedy continuation
        base, n = run([2, 2, 2, 2], 0)
        assert n == C - 1
        assert bool((base[:, 3] == base[0, 3]).all()), "copies of one prompt decode alike"
        eos = int(base[0, 3])
        cfg.eos_token_id = eos
        full, n_full = run([2, 2, 2, 2], 0)
        early, n_early = run([2, 2, 2, 2], 4)
        ends = [int((r == eos).nonzero()[0]) for r in full]
        print("early stop: rows end at steps %s, decode steps enqueued %d (poll_every=4) against %d" % (ends, n_early, n_full))
        assert max(ends) <= 3 and n_full == C - 1
        assert n_early <= 3 + 2 * 4 + 1 and n_early < C - 1, n_early
        assert torch.equal(early, full)
        assert all(bool((r[e + 1:] == pad).all()) for r, e in zip(full, ends))
        # one row that never produces this id keeps the loop running to the end
        other = None
        for sd in range(20, 30):
            cfg.eos_token_id = -1
            probe, _ = run([2, 2, sd, 2], 0)
            cfg.eos_token_id = eos
            if eos not in probe[2].tolist():
                other = sd
                break
        assert other is not None, "no seeded prompt without the chosen id among 10"
        mixed, n_mixed = run([2, 2, other, 2], 4)
        assert n_mixed == C - 1
        assert torch.equal(mixed[2], probe[2]) and eos not in mixed[2].tolist()
        for r in (0, 1, 3):
            e = int((mixed[r] == eos).nonzero()[0])
            assert e <= 3 and bool((mixed[r, e + 1:] == pad).all())
    finally:
        cfg.eos_token_id = old_eos


# ------------------------------------------------------------------------------------------------------------------ 5. full width
def test_32_prompts_one_row_each_at_full_width(hip_ops):
    """qwen2-vl-7b widths with 2 decoder layers and a 2-block tower: 32 prompts of two lengths, one row each (tr1_decode_step with n_batch = 32), 8 decode
    steps.  Logits finite, tokens inside the vocabulary, and prompt 0 decodes the same when the other 31 prompts change places."""
    import time_r1_amd  # noqa: F401
    from time_r1_amd.config import PRESETS
    from time_r1_amd.params import ModelParams
    from time_r1_amd.model import Engine
    from time_r1_amd.synthetic import synthetic_prompt
    ops = hip_ops
    cfg = PRESETS["qwen2-vl-7b"]()
    cfg.text.n_layers = 2
    cfg.vision.depth = 2
    params = ModelParams(cfg, ops, init="none")
    params.init_random_device(0)
    eng = Engine(cfg, ops, params)
    B, C = 32, 9
    core = _greedy_core(eng, C, poll_every=0)
    sts = [core.prepare(*synthetic_prompt(cfg, (8, 14, 28), 64, 64 if b % 2 == 0 else 41, seed=b)) for b in range(B)]
    assert len({st.P for st in sts}) == 2
    finite = []
    orig = ops.greedy_tokens

    def spy(logits, *a, **k):
        finite.append(torch.isfinite(logits).all())
        return orig(logits, *a, **k)
    ops.greedy_tokens = spy
    try:
        a = torch.cat([t.cpu() for t in core.rollout_many(sts)])
        assert core.roll.last_steps_run == C - 1 and len(finite) == B + C - 1
        perm = [0] + [int(i) + 1 for i in torch.randperm(B - 1, generator=torch.Generator().manual_seed(3))]
        assert perm != list(range(B))
        b = torch.cat([t.cpu() for t in core.rollout_many([sts[i] for i in perm])])
    finally:
        del ops.greedy_tokens
    assert all(bool(f) for f in finite), "logits must be finite"
    assert a.shape == (B, C) and int(a.min()) >= 0 and int(a.max()) < cfg.text.vocab_size
    assert int(b.min()) >= 0 and int(b.max()) < cfg.text.vocab_size
    assert torch.equal(a[0], b[0]), (a[0].tolist(), b[0].tolist())
    same = sum(bool(torch.equal(a[i], b[j])) for j, i in enumerate(perm))
    print("full width, 32 prompts x 1 row: %d of 32 prompts decode identically after the permutation" % same)
