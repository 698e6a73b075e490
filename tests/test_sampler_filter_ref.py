"""CPU side of the sampler's top-p / min-p / repetition-penalty feature: the fp64 reference of tests/sampler_filter_cases.py against the transformers
warpers, and the host plumbing (GRPOConfig, Rollout on the oracle backend, generation_config.json)."""
import json
import os
import sys

import pytest
import torch

import sampler_filter_cases as fc
import vocab_cases as vc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import load_case, golden_params, frames_for, ref_ops_without  # noqa: E402
from oracle.ref_ops import RefOps  # noqa: E402
from oracle.text import FakeProcessor  # noqa: E402
from time_r1_amd import rewards as R  # noqa: E402
from time_r1_amd.trainer import TimeR1_Trainer, GRPOConfig, generation_config_dict  # noqa: E402

I32 = torch.int32


# ------------------------------------------------------------------------------------------------------------ reference vs transformers
@pytest.mark.parametrize("top_k,T,top_p,min_p", [(0, 1.0, 0.9, 0.0), (50, 0.7, 0.9, 0.0), (0, 1.0, 1.0, 0.05), (50, 1.0, 0.95, 0.02), (0, 0.7, 0.5, 0.0), (5, 1.3, 0.3, 0.4)])
def test_reference_kept_set_equals_hf_warpers(top_k, T, top_p, min_p):
    """Temperature -> TopK -> TopP -> MinP of transformers on 200 tie-free 64-token rows: the same kept set, row by row."""
    lp = pytest.importorskip("transformers.generation.logits_process")
    rows = fc.tie_free_rows(200, 64, seed=3)
    procs = [lp.TemperatureLogitsWarper(T)]
    if top_k:
        procs.append(lp.TopKLogitsWarper(top_k))
    if top_p < 1.0:
        procs.append(lp.TopPLogitsWarper(top_p))
    if min_p > 0.0:
        procs.append(lp.MinPLogitsWarper(min_p))
    scores = rows.double()
    for p in procs:
        scores = p(None, scores)
    hf_keep = torch.isfinite(scores)
    sizes = set()
    for r in range(rows.shape[0]):
        keep, cdf, margin = fc.ref_filter(rows[r], T, top_k, top_p, min_p)
        if margin > 1e-9:          # (fp64 on both sides; a row exactly on a boundary would be decided by the order of a sum)
            assert torch.equal(keep, hf_keep[r]), (r, int(keep.sum()), int(hf_keep[r].sum()))
        hf_p = torch.softmax(scores[r], 0)
        assert torch.allclose(torch.cumsum(hf_p, 0), cdf, atol=1e-12), "the CDF over the kept set is the softmax of the warped scores"
        sizes.add(int(keep.sum()))
    assert len(sizes) > 1


def test_reference_filters_off_equal_token_cdf():
    row = vc.sweep_rows(1, 4096, seed=5)[0]
    for top_k in (0, 50):
        keep, cdf, margin = fc.ref_filter(row, 0.9, top_k)
        keep0, cdf0 = vc.token_cdf(row, 0.9, top_k)
        assert torch.equal(keep, keep0) and torch.equal(cdf, cdf0) and margin == float("inf")


@pytest.mark.parametrize("V", [1001, vc.V_FULL])
def test_crafted_rows_have_the_kept_sets_they_name(V):
    for name, c in fc.crafted_filter_cases(V).items():
        keep, _, margin = fc.ref_filter(c["logits"][0], c["temperature"], c["top_k"], c["top_p"], c["min_p"])
        assert int(keep.sum()) == c["kept"], (name, int(keep.sum()))
        exact = name in ("top_p_1e-6", "min_p_1", "min_p_1_signed_zero_max")      # boundaries that are exact in every arithmetic: mass above = 0, ratio = 1
        assert exact or margin > 100 * vc.CDF_SLACK, (name, margin)


def test_sweep_rows_keep_their_distance_from_every_boundary():
    """No row of the GPU sweep may be left out of the kept-set check: all margins above CDF_SLACK; tiny and wide nuclei both occur."""
    sizes = []
    for cfg in fc.SWEEP_CONFIGS:
        _, refs, margins = fc.sweep_refs(cfg)
        assert min(margins) > vc.CDF_SLACK, (cfg, min(margins))
        sizes += [int(k.sum()) for k, _ in refs]
    assert min(sizes) <= 4 and max(sizes) >= 10000


def test_reference_penalty_equals_hf_processor():
    """RepetitionPenaltyLogitsProcessor on rows whose penalised values are exact in bf16 (multiples of 0.25 in [-8, 8], penalty 2): equal values."""
    lp = pytest.importorskip("transformers.generation.logits_process")
    g = torch.Generator().manual_seed(9)
    V, rows = 300, 6
    x = (torch.randint(-32, 33, (rows, V), generator=g).float() / 4).to(vc.BF16)
    ids = torch.stack([torch.randperm(V, generator=g)[:40] for _ in range(rows)])
    ids[:, 5] = ids[:, 4]                                                          # a repeated id is penalised once
    want = lp.RepetitionPenaltyLogitsProcessor(2.0)(ids, x.float().clone())
    got = fc.ref_penalize(x, [sorted(set(r.tolist())) for r in ids], 2.0)
    assert torch.equal(got.float(), want) and not torch.equal(got, x)
    bm = fc.seen_bitmap(rows, V, [r.tolist() for r in ids])
    assert [fc.bitmap_tokens(bm[r], V) for r in range(rows)] == [set(r.tolist()) for r in ids]


# ------------------------------------------------------------------------------------------------------------ host plumbing
def test_grpo_config_fields_and_ranges():
    a = GRPOConfig()
    assert (a.top_p, a.min_p, a.repetition_penalty) == (1.0, None, 1.0)
    a = GRPOConfig(top_p="0.9", min_p="0.05", repetition_penalty=1.05)          # the command line hands strings over for Optional fields
    assert (a.top_p, a.min_p, a.repetition_penalty) == (0.9, 0.05, 1.05)
    for bad in (dict(top_p=0.0), dict(top_p=1.5), dict(top_p=-0.1), dict(min_p=-0.1), dict(min_p=1.5), dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0)):
        with pytest.raises(ValueError):
            GRPOConfig(**bad)


def test_rollout_range_errors():
    from time_r1_amd.rollout import Rollout
    r = Rollout(None, 2, 4, top_p=0.9, min_p=None, repetition_penalty=1.1)
    assert (r.top_p, r.min_p, r.repetition_penalty) == (0.9, 0.0, 1.1)
    for bad in (dict(top_p=0.0), dict(top_p=1.01), dict(min_p=-1e-3), dict(min_p=1.01), dict(repetition_penalty=0.0), dict(repetition_penalty=float("inf"))):
        with pytest.raises(ValueError):
            Rollout(None, 2, 4, **bad)


class FilterRefOps(RefOps):
    """RefOps that records what the rollout asks of the sampler, the penalty and the seen bitmap."""

    def __init__(self):
        super().__init__()
        self.calls = []

    def sample_tokens(self, logits, temperature, top_k, seed, step_dev, tokens, finished, eos_id, pad_id, stop_at_eos, u_out=None, group_rows=0,
                      seed_stride=0, top_p=1.0, min_p=0.0):
        self.calls.append(("sample", int(step_dev.item()), top_p, min_p, logits.clone()))
        return super().sample_tokens(logits, temperature, top_k, seed, step_dev, tokens, finished, eos_id, pad_id, stop_at_eos, u_out, group_rows, seed_stride,
                                     top_p, min_p)

    def penalize_logits(self, logits, seen, penalty, out=None):
        sets = [sorted(fc.bitmap_tokens(seen[r], logits.shape[1])) for r in range(logits.shape[0])]
        self.calls.append(("penalize", penalty, logits.clone(), sets))
        assert out is not None and out.data_ptr() != logits.data_ptr(), "the penalised logits go to a buffer of their own"
        return super().penalize_logits(logits, seen, penalty, out=out)

    def mark_seen(self, seen, V, ids=None, tokens=None, step_dev=None, finished=None):
        if ids is not None:
            self.calls.append(("mark_ids", seen, ids.tolist()))
        else:
            col = tokens[:, int(step_dev.item())] if tokens.dim() == 2 else tokens
            self.calls.append(("mark_drawn", int(step_dev.item()) if step_dev is not None else None, col.tolist(), None if finished is None else finished.tolist()))
        return super().mark_seen(seen, V, ids=ids, tokens=tokens, step_dev=step_dev, finished=finished)


class RecordingRefOps(type(ref_ops_without("penalize_logits", "mark_seen"))):
    """An oracle backend from before the feature (sample_tokens without the new arguments, no penalize_logits / mark_seen) that records how sample_tokens is
    called."""

    def __init__(self):
        super().__init__()
        self.calls = []

    def sample_tokens(self, logits, temperature, top_k, seed, step_dev, tokens, finished, eos_id, pad_id, stop_at_eos, u_out=None, group_rows=0,
                      seed_stride=0):
        self.calls.append((float(temperature), int(top_k), int(seed), int(step_dev.item())))
        return super().sample_tokens(logits, temperature, top_k, seed, step_dev, tokens, finished, eos_id, pad_id, stop_at_eos, u_out, group_rows, seed_stride)


def _trainer(ops, **over):
    fx = load_case("clip_nobeta")
    cfg, pol, _ = golden_params(ops, fx)
    args = GRPOConfig(output_dir="/tmp/tr1_filter_test", num_generations=fx["G"], max_completion_length=fx["C"], beta=fx["beta"], use_grpo=fx["use_grpo"],
                      rope_index_mode="hf5", temperature=1.0, logging_steps=1, save_strategy="no", **over)
    tr = TimeR1_Trainer(pol, [R.iou_timestamp_reward_v2, R.format_reward], list(R.metric_funcs_registry.values()), args=args, train_dataset=None,
                        processing_class=FakeProcessor(cfg), ops=ops)
    tr._video_inputs = lambda ex: ([frames_for(fx)], [2.0])
    return fx, cfg, tr


def _core(tr, G, C, **kw):
    from time_r1_amd.grpo import GRPOCore
    return GRPOCore(tr.engine, None, G, C, beta=0.0, temperature=1.0, top_k=20, seed=11, rope_index_mode=tr.args.rope_index_mode, reuse_prefill=False, **kw)


def test_trainer_passes_the_fields_to_the_rollout():
    _, _, tr = _trainer(RefOps(), top_p=0.85, min_p=0.03, repetition_penalty=1.2)
    roll = tr.core.roll
    assert (roll.top_p, roll.min_p, roll.repetition_penalty) == (0.85, 0.03, 1.2)
    _, _, tr = _trainer(RefOps())
    assert (tr.core.roll.top_p, tr.core.roll.min_p, tr.core.roll.repetition_penalty) == (1.0, 0.0, 1.0)


def test_rollout_marks_prompt_and_drawn_tokens_and_skips_finished_rows():
    from time_r1_amd import evaluate as E
    ops = FilterRefOps()
    fx, cfg, tr = _trainer(ops)
    G, C, pen = 3, 7, 1.5
    row = dict(fx["row"])
    toks = {}
    for stop in (False, True):
        core = _core(tr, G, C, top_p=0.9, min_p=0.01, repetition_penalty=pen, stop_at_eos=stop)
        st = E._prepare_row(tr, core, row)
        prompt = set(st.prompt_ids.tolist())
        V = int(tr.engine.params.lm_head_w(tr.engine.params.train).shape[0])
        old = cfg.eos_token_id
        if stop:      # end row 0 at its third token
            cfg.eos_token_id = int(toks[False][0, 2])
        ops.calls = []
        try:
            t = toks[stop] = core.rollout(st).clone()
        finally:
            cfg.eos_token_id = old
        calls = ops.calls
        kinds = [c[0] for c in calls]
        assert kinds == ["mark_ids", "penalize", "sample", "mark_drawn"] + ["penalize", "sample", "mark_drawn"] * (C - 1)
        seen = calls[0][1]
        assert seen.shape == (G, (V + 31) // 32) and calls[0][2] == st.prompt_ids.tolist(), "the prompt's ids go into the prompt's G rows"
        assert calls[1][2].shape[0] == 1 and calls[1][3] == [sorted(v for v in prompt if v < V)], "the ONE prefill row is penalised, by the prompt's tokens"
        for s in range(C):
            p, smp, mk = calls[1 + 3 * s], calls[2 + 3 * s], calls[3 + 3 * s]
            assert smp[1] == s and smp[2:4] == (0.9, 0.01), "top_p / min_p reach every sampler call"
            want = fc.ref_penalize(p[2].to(vc.BF16), p[3], pen).float()
            assert torch.equal(smp[4].float(), want.expand(smp[4].shape[0], -1)), "step %d: the sampler reads the penalised logits" % s
            assert mk[1] == s and mk[2] == t[:, s].tolist(), "step %d: the column just drawn is marked" % s
            assert (mk[3] is None) == (not stop)
            if s > 0:      # every row is penalised by its prompt and its own earlier tokens (finished rows: up to their end)
                for r in range(G):
                    live = [int(x) for x in t[r, :s]]
                    if stop and int(toks[False][0, 2]) in live:
                        live = live[:live.index(int(toks[False][0, 2]))]
                    assert set(p[3][r]) == {v for v in prompt | set(live) if v < V}, (s, r)
        if stop:
            eos, pad = int(toks[False][0, 2]), cfg.pad_token_id
            assert torch.equal(t[0, :3], toks[False][0, :3]) and bool((t[0, 3:] == pad).all()), "row 0 ends at its third token and is padded"
            assert pad in prompt or pad not in fc.bitmap_tokens(seen[0], V), "padding of a finished row is never marked"
    assert not torch.equal(toks[False][0, 3:], toks[True][0, 3:])


def test_defaults_leave_the_backend_calls_as_they_were():
    from time_r1_amd import evaluate as E
    ops = RecordingRefOps()
    fx, _, tr = _trainer(ops)
    row = dict(fx["row"])
    out = []
    for kw in ({}, dict(top_p=1.0, min_p=0.0, repetition_penalty=1.0), dict(top_p=None, min_p=None, repetition_penalty=None)):
        core = _core(tr, 2, 5, **kw)
        ops.calls = []
        out.append((core.rollout(E._prepare_row(tr, core, row)).clone(), list(ops.calls)))
    assert len(out[0][1]) == 5 and all(torch.equal(out[0][0], t) and out[0][1] == c for t, c in out[1:])
    assert not hasattr(ops, "penalize_logits") and not hasattr(ops, "mark_seen")


@pytest.mark.parametrize("kw", [dict(top_p=0.9), dict(min_p=0.05), dict(repetition_penalty=1.1)], ids=["top_p", "min_p", "repetition_penalty"])
def test_non_default_on_a_backend_without_the_ops_raises(kw):
    from time_r1_amd import evaluate as E
    ops = RecordingRefOps()
    fx, _, tr = _trainer(ops)
    core = _core(tr, 2, 4, **kw)
    st = E._prepare_row(tr, core, dict(fx["row"]))
    with pytest.raises(NotImplementedError, match=list(kw)[0]):
        core.rollout(st)
    assert ops.calls == [], "refused before anything was sampled"


def test_greedy_mode_honours_the_penalty_and_ignores_the_filters():
    from time_r1_amd import evaluate as E
    ops = FilterRefOps()
    fx, _, tr = _trainer(ops)
    row = dict(fx["row"])
    core = _core(tr, 1, 6, greedy=True, top_p=0.5, min_p=0.5, repetition_penalty=1.0)
    plain = core.rollout(E._prepare_row(tr, core, row)).clone()
    assert all(c[0] == "sample" and c[2:4] == (1.0, 0.0) for c in ops.calls), "greedy: top_p / min_p are not passed on"
    ops.calls = []
    core = _core(tr, 1, 6, greedy=True, repetition_penalty=50.0)
    pen = core.rollout(E._prepare_row(tr, core, row)).clone()
    assert [c[0] for c in ops.calls][:4] == ["mark_ids", "penalize", "sample", "mark_drawn"]
    live = [int(x) for x in pen[0]]
    if core.cfg.eos_token_id in live:
        live = live[:live.index(core.cfg.eos_token_id) + 1]
    assert len(set(live)) == len(live), "with a huge penalty the argmax never repeats a token"
    assert plain.shape == pen.shape


def test_generation_config_keys_only_when_non_default(tmp_path):
    _, cfg, tr = _trainer(RefOps())
    tr.processing_class.save_pretrained = lambda d: None
    tr.save_model(str(tmp_path / "a"))
    gc = json.load(open(tmp_path / "a" / "generation_config.json"))
    assert set(gc) == {"eos_token_id", "pad_token_id", "do_sample", "temperature"}
    _, cfg, tr = _trainer(RefOps(), top_p=0.9, min_p=0.05, repetition_penalty=1.05)
    tr.processing_class.save_pretrained = lambda d: None
    tr.save_model(str(tmp_path / "b"))
    gc = json.load(open(tmp_path / "b" / "generation_config.json"))
    assert (gc["top_p"], gc["min_p"], gc["repetition_penalty"]) == (0.9, 0.05, 1.05) and gc["temperature"] == 1.0
    d = generation_config_dict(cfg, GRPOConfig(min_p=0.0, top_p=1.0, repetition_penalty=1.0))
    assert set(d) == {"eos_token_id", "pad_token_id", "do_sample", "temperature"}
    assert set(generation_config_dict(cfg, GRPOConfig(repetition_penalty=1.1))) == {"eos_token_id", "pad_token_id", "do_sample", "temperature", "repetition_penalty"}


def test_evaluate_accepts_a_repetition_penalty():
    from time_r1_amd import evaluate as E
    from time_r1_amd import data as D
    ops = FilterRefOps()
    fx, _, tr = _trainer(ops)
    ds = D.RowDataset([dict(fx["row"])])
    for bs in (None, 1):
        ops.calls = []
        E.evaluate_grounding(tr, ds, max_new_tokens=4, batch_size=bs, repetition_penalty=1.3)
        assert any(c[0] == "penalize" and c[1] == 1.3 for c in ops.calls), bs
        ops.calls = []
        E.evaluate_grounding(tr, ds, max_new_tokens=4, batch_size=bs)
        assert all(c[0] == "sample" for c in ops.calls), bs
