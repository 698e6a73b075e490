"""Shared pieces of the trim_completions tests (GRPOConfig.trim_completions: sampled rollouts that stop once every row has drawn its EOS, updates on the live
columns only): the tiny trainer, a spy on the decoder's row counts, and the early-stop scenario that tests/test_trim_completions_ref.py runs on the CPU
oracle backend and tests/test_trim_completions_gpu.py on the HIP path."""
import numpy as np
import torch

from helpers import golden_params, HF_GRAD_KEYS

SHORT = "clip_beta_short"          # tests/golden/gen_short_golden.py: C = 16, first EOS at columns 8, 8, 5, 8 -> Ct = 9
GRAD_NAMES = sorted({n for n, _ in HF_GRAD_KEYS.values()} | {"embed"})


def make_trainer(fx, ops, ga=1, peft=None, C=None, **over):
    """test_trainer_gpu._make with keyword overrides (and an optional peft_config, whose reference policy stays the base copy)."""
    import time_r1_amd  # noqa: F401
    from time_r1_amd.trainer import TimeR1_Trainer, GRPOConfig
    from time_r1_amd import rewards as R
    from oracle.text import FakeProcessor
    cfg, pol, ref = golden_params(ops, fx)
    args = GRPOConfig(output_dir="/tmp/tr1_trim", num_generations=fx["G"], max_completion_length=C or fx["C"], beta=fx["beta"], use_grpo=fx["use_grpo"],
                      rope_index_mode="hf5", gradient_accumulation_steps=ga, temperature=1.0, save_strategy="no", disable_log_print=True, **over)
    tr = TimeR1_Trainer(pol, [R.iou_timestamp_reward_v2, R.format_reward], [], args=args, processing_class=FakeProcessor(cfg), ops=ops, peft_config=peft)
    if fx["beta"] != 0 and peft is None:
        tr.ref_model.w16.copy_(ref.train.w16)
    return cfg, tr


def spy_rows(tr):
    """Record every decoder-stack call of the trainer's engine -> list of (arena is the trainable one, rows, row0)."""
    calls, eng = [], tr.engine
    orig = eng.llm_fwd

    def llm_fwd(arena, h, *a, **k):
        calls.append((arena is eng.params.train, int(h.shape[0]), int(k.get("row0", 0))))
        return orig(arena, h, *a, **k)
    eng.llm_fwd = llm_fwd
    return calls


def named_grads(tr):
    a = tr.lora.train if tr.lora is not None else tr.params.train
    names = a.names() if tr.lora is not None else GRAD_NAMES
    return {n: a.g(n).detach().float().cpu().clone() for n in names}


def first_eos_lengths(ids, eos):
    """numpy [G, C] -> per row (index of the first EOS + 1), C without one."""
    ids = np.asarray(ids)
    is_eos = ids == eos
    return np.where(is_eos.any(1), is_eos.argmax(1) + 1, ids.shape[1])


# ---------------------------------------------------------------------------------------------------------------- the early-stop scenario
def tiny_engine(ops, n_layers=3):
    import time_r1_amd  # noqa: F401
    from time_r1_amd.config import tiny_test
    from time_r1_amd.params import ModelParams
    from time_r1_amd.model import Engine
    cfg = tiny_test(n_layers=n_layers)
    return cfg, Engine(cfg, ops, ModelParams(cfg, ops, seed=1))


def early_stop_scenario(ops, G, C, poll_every, native=True, n_layers=3, prompt_seeds=range(2, 14), other_seeds=range(20, 40), last_end=5):
    """A top_k = 1 SAMPLED rollout (greedy=False) of 2 prompts x G rows with Rollout.early_stop against the same rollout run to the end.  The EOS id is taken
    from a run that stops nowhere: the first token that every row of two copies of one prompt holds within its first `last_end` + 1 columns - prompt seeds are
    searched until one has such a token (top_k = 1 keeps ties at the maximum, so the rows of a prompt need not decode alike).  Then a second prompt whose rows
    never hold that id (searched as well) keeps the loop running to the end.  -> dict of what the callers print / assert further."""
    from time_r1_amd.grpo import GRPOCore
    from time_r1_amd.rollout import Rollout
    from time_r1_amd.synthetic import synthetic_prompt
    cfg, eng = tiny_engine(ops, n_layers)
    pad, old_eos, bufs = cfg.pad_token_id, cfg.eos_token_id, []
    orig_buffers = Rollout._buffers

    def keep_buffers(self, *a, **k):
        bufs.append(orig_buffers(self, *a, **k))
        return bufs[-1]

    cache = {}

    def inputs(sd):      # one prompt per seed, whatever id ends a row at the time (synthetic_prompt avoids the EOS id in its text)
        if sd not in cache:
            now, cfg.eos_token_id = cfg.eos_token_id, -1
            cache[sd] = synthetic_prompt(cfg, (4, 6, 8), 9, 7, seed=sd, text_vocab=400)
            cfg.eos_token_id = now
        return cache[sd]

    def run(seeds, early, pe):
        core = GRPOCore(eng, None, G, C, beta=0.0, temperature=1.0, top_k=1, seed=5, rope_index_mode="hf4", stop_at_eos=True, reuse_prefill=False)
        core.roll.poll_every, core.roll.early_stop, core.roll.native_decode = pe, early, native
        toks = core.rollout_many([core.prepare(*inputs(sd)) for sd in seeds])
        return torch.cat([t.cpu() for t in toks]), core.roll.last_steps_run
    Rollout._buffers = keep_buffers
    try:
        eos = seed = None
        for sd in prompt_seeds:
            cfg.eos_token_id = -1          # no id ends a row
            base, n = run([sd, sd], False, 0)
            assert n == C - 1
            for t in base[0, 1:last_end + 1].tolist():
                if t != pad and all(t in r[:last_end + 1].tolist() for r in base):
                    eos, seed = int(t), sd
                    break
            if eos is not None:
                break
        assert eos is not None, "no prompt seed whose rows share a token within their first columns"
        cfg.eos_token_id = eos
        full, n_full = run([seed, seed], False, 0)
        assert n_full == C - 1 and bufs[-1].done_count is None, "without early_stop the sampled loop runs to the end and keeps no counter"
        early, n_early = run([seed, seed], True, poll_every)
        buf = bufs[-1]
        ends = [int((r == eos).nonzero()[0]) for r in full]
        assert max(ends) <= last_end
        assert torch.equal(early, full), "early stop must not change a token"
        assert all(bool((r[e + 1:] == pad).all()) for r, e in zip(full, ends)), "pads follow each EOS"
        assert n_early <= max(ends) + 2 * poll_every + 1 and n_early < C - 1, (n_early, ends)
        assert int(buf.finished.sum()) == 2 * G
        counted = buf.done_count is not None
        if counted:
            assert int(buf.done_count) == int(buf.finished.sum())
        # one prompt that never produces this id keeps the loop running to the end
        other = None
        for sd in other_seeds:
            cfg.eos_token_id = -1
            probe, _ = run([seed, sd], False, 0)
            cfg.eos_token_id = eos
            if eos not in probe[G:].reshape(-1).tolist():
                other = sd
                break
        assert other is not None, "no seeded prompt without the chosen id"
        mixed_full, _ = run([seed, other], False, 0)
        mixed, n_mixed = run([seed, other], True, poll_every)
        buf = bufs[-1]
        assert n_mixed == C - 1
        assert torch.equal(mixed, mixed_full) and torch.equal(mixed[G:], probe[G:]) and eos not in mixed[G:].reshape(-1).tolist()
        assert int(buf.finished.sum()) == G
        if counted:
            assert int(buf.done_count) == G
        return dict(eos=eos, ends=ends, n_early=n_early, n_full=n_full, counted=counted)
    finally:
        Rollout._buffers = orig_buffers
        cfg.eos_token_id = old_eos
