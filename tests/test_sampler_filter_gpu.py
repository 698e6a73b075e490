"""The sampler's top-p / min-p filters, the repetition penalty and the seen-token bitmap on the GPU, against the fp64 reference of
tests/sampler_filter_cases.py (pinned to the transformers warpers on the CPU by tests/test_sampler_filter_ref.py).

Every draw is judged exactly: the token lies in the reference's kept set and the Philox uniform (bit-equal to the host's) lies in the token's fp64 CDF
interval with the project's CDF_SLACK = 1e-4.  A kept set can only differ from the reference's when a row sits within the kernel's mass error of a
boundary: fp32 exp-argument rounding bounds that error near 4e-6, rows of the sweep keep a margin above CDF_SLACK (asserted), the crafted rows sit
percents away from theirs or exactly on a representable one (top_p = 1e-6, min_p = 1)."""
import pytest
import torch

import sampler_filter_cases as fc
import vocab_cases as vc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16, I32 = vc.BF16, vc.I32


def bits(t):
    return t.contiguous().view(torch.int16)


def step_t(s):
    return torch.tensor([s], dtype=I32, device=DEV)


def run_draws(hip_ops, logits_d, cfg, seeds, n_steps):
    """(seed, step) sweep of one configuration -> [(seed, step, tokens, u)]; the uniforms are checked against the host's Philox, bit for bit."""
    top_k, T, top_p, min_p = cfg
    rows = logits_d.shape[0]
    out = []
    for seed in seeds:
        tok = torch.full((rows, n_steps), -7, dtype=I32, device=DEV)
        us = []
        for step in range(n_steps):
            u = torch.zeros(rows, device=DEV)
            hip_ops.sample_tokens(logits_d, T, top_k, seed, step_t(step), tok, None, -1, 0, False, u_out=u, top_p=top_p, min_p=min_p)
            us.append(u)
        tok_c = tok.cpu()
        for step in range(n_steps):
            u_c = us[step].cpu().tolist()
            for r in range(rows):
                assert u_c[r] == vc.philox_u(seed, r, step), ("philox uniform", seed, step, r)
            out.append((seed, step, tok_c[:, step].tolist(), u_c))
    return out


def judge(draws, refs, what):
    worst, n = 0.0, 0
    for seed, step, toks, us in draws:
        for r, (t, u) in enumerate(zip(toks, us)):
            keep, cdf = refs[r]
            e = vc.draw_error(keep, cdf, t, u)
            assert e is None, (what, "seed %d step %d row %d" % (seed, step, r), e)
            worst = max(worst, (float(cdf[t - 1]) if t > 0 else 0.0) - u, u - float(cdf[t]))
            n += 1
    print("OBS %-70s %d draws, worst distance outside the CDF interval %.3e (slack %g)" % (what, n, worst, vc.CDF_SLACK))


# ------------------------------------------------------------------------------------------------------------ 1. sweep
@pytest.mark.parametrize("cfg", fc.SWEEP_CONFIGS, ids=["k%d-T%g-p%g-m%g" % c for c in fc.SWEEP_CONFIGS])
def test_filter_sweep_full_vocabulary(hip_ops, cfg):
    """16 rows x 8 steps x 3 seeds at V = 152064 per configuration; no row is left out (every margin is above CDF_SLACK)."""
    logits, refs, margins = fc.sweep_refs(cfg)
    assert min(margins) > vc.CDF_SLACK, "a sweep row sits on a filter boundary: change SWEEP_ROW_SEED, not the cap (%r)" % (margins,)
    draws = run_draws(hip_ops, logits.to(DEV), cfg, fc.SWEEP_SEEDS, fc.SWEEP_STEPS)
    assert sum(len(d[2]) for d in draws) == fc.SWEEP_ROWS * fc.SWEEP_STEPS * len(fc.SWEEP_SEEDS)
    judge(draws, refs, "filter sweep top_k=%d T=%g top_p=%g min_p=%g (kept %d .. %d)" % (cfg + (min(int(k.sum()) for k, _ in refs), max(int(k.sum()) for k, _ in refs))))


# ------------------------------------------------------------------------------------------------------------ 2. crafted rows
CRAFTED_V = (vc.V_FULL, vc.V_UNFUSED, 1001)
_CRAFTED = {V: fc.crafted_filter_cases(V) for V in CRAFTED_V}
CRAFTED_ROWS = 8      # the one row, drawn by 8 rows with their own uniforms: 8 x 4 steps x 4 seeds = 128 draws per case


@pytest.mark.parametrize("V", CRAFTED_V, ids=["fused-V152064", "unfused-V163848", "V1001"])
@pytest.mark.parametrize("name", sorted(_CRAFTED[1001]))
def test_filter_crafted(hip_ops, name, V):
    c = _CRAFTED[V][name]
    cfg = (c["top_k"], c["temperature"], c["top_p"], c["min_p"])
    keep, cdf, _ = fc.ref_filter(c["logits"][0], c["temperature"], c["top_k"], c["top_p"], c["min_p"])
    assert int(keep.sum()) == c["kept"]
    logits_d = c["logits"].to(DEV).expand(CRAFTED_ROWS, V).contiguous()
    draws = run_draws(hip_ops, logits_d, cfg, vc.CRAFTED_SEEDS, vc.CRAFTED_STEPS)
    judge(draws, [(keep, cdf)] * CRAFTED_ROWS, "filter crafted %s V=%d" % (name, V))
    drawn = set(t for d in draws for t in d[2])
    assert drawn == set(torch.nonzero(keep)[:, 0].tolist()), (name, V, "every kept token is drawn over 128 draws, nothing else", sorted(drawn))


# ------------------------------------------------------------------------------------------------------------ 3. defaults are the old path
def raw_filtered(hip_ops, logits, T, top_k, top_p, min_p, seed, step, tok, fin, eos, pad, stop, u, group_rows=0, seed_stride=0, next_ids=None, ws=None):
    """The new entry points called directly (HipOps.sample_tokens routes the defaults to the old ones)."""
    rows, V = logits.shape
    nws = int(hip_ops.L.raw("tr1_sample_filtered_workspace_words")(rows))
    ws = torch.zeros(nws, dtype=I32, device=DEV) if ws is None else ws
    head = (logits.data_ptr(), logits.stride(0), rows, V, float(T), int(top_k), float(top_p), float(min_p), int(seed) & (2 ** 64 - 1), int(group_rows),
            int(seed_stride), step.data_ptr(), tok.data_ptr(), tok.stride(0), 0 if fin is None else fin.data_ptr(), eos, pad, int(stop), u.data_ptr(),
            ws.data_ptr(), nws)
    if next_ids is None:
        hip_ops.L.call("tr1_sample_tokens_filtered", *head, hip_ops._s())
    else:
        hip_ops.L.call("tr1_sample_tokens_filtered_step", *head, next_ids.data_ptr(), 1, hip_ops._s())
    return ws


@pytest.mark.parametrize("V", [vc.V_FULL, 1001])
@pytest.mark.parametrize("top_k", [0, 50])
def test_defaults_equal_the_unfiltered_entry_points(hip_ops, V, top_k):
    """top_p = 1, min_p = 0 through the new entry points: tokens, finished flags and uniforms bit-identical to tr1_sample_tokens / _step, with grouped seeds
    and with rows that finish on the way (stop_at_eos)."""
    B, G, eos, pad, seed = 2, 4, 3, 1, 20240607
    rows, C = B * G, 8
    tok = [torch.full((rows, C), -7, dtype=I32, device=DEV) for _ in range(4)]
    fin = [torch.zeros(rows, dtype=I32, device=DEV) for _ in range(4)]
    nid = [torch.full((rows,), -7, dtype=I32, device=DEV) for _ in range(2)]
    ws_step = None
    for call in range(C):
        logits_d = vc.step_form_logits(call + 3, rows, V, eos).to(DEV)
        u = [torch.zeros(rows, device=DEV) for _ in range(4)]
        kw = dict(group_rows=G, seed_stride=7919)
        hip_ops.sample_tokens(logits_d, 0.9, top_k, seed, step_t(call), tok[0], fin[0], eos, pad, True, u_out=u[0], **kw)
        raw_filtered(hip_ops, logits_d, 0.9, top_k, 1.0, 0.0, seed, step_t(call), tok[1], fin[1], eos, pad, True, u[1], **kw)
        hip_ops.sample_tokens(logits_d, 0.9, top_k, seed, step_t(call), tok[2], fin[2], eos, pad, True, u_out=u[2], next_ids=nid[0], **kw)
        ws_step = raw_filtered(hip_ops, logits_d, 0.9, top_k, 1.0, 0.0, seed, step_t(call), tok[3], fin[3], eos, pad, True, u[3], next_ids=nid[1], ws=ws_step, **kw)
        assert not bool(ws_step.any()), "call %d left the step-form workspace dirty" % call
        for i in (1, 2, 3):
            assert torch.equal(tok[0], tok[i]) and torch.equal(fin[0], fin[i]) and torch.equal(u[0], u[i]), (call, i)
        assert torch.equal(nid[0], nid[1])
    f = fin[0].cpu()
    assert bool(f.any()) and (tok[0].cpu()[f.bool()] == pad).any(), "rows finished on the way and received padding"


# ------------------------------------------------------------------------------------------------------------ 4. step form, consecutive calls
@pytest.mark.parametrize("V", [vc.V_FULL, 1001])
def test_filter_step_form_over_consecutive_calls(hip_ops, V):
    """The step form with a workspace zeroed once: 12 decode calls with both filters on, rows finishing on the way, equal call by call to the one-shot form;
    the cached workspace is all zero after every call, and repeating a call gives the same tokens."""
    rows, eos, pad, seed, C = 8, 3, 1, 777, 12
    cfg = dict(top_p=0.9, min_p=0.02)
    tok_a = torch.full((rows, C), -7, dtype=I32, device=DEV)
    tok_b = tok_a.clone()
    fin_a = torch.zeros(rows, dtype=I32, device=DEV)
    fin_b = fin_a.clone()
    nid = torch.full((rows,), -7, dtype=I32, device=DEV)
    n_checked = 0
    for call in range(C):
        logits = vc.step_form_logits(call, rows, V, eos)
        logits_d = logits.to(DEV)
        was_done = fin_b.cpu().bool()
        u_a, u_b = torch.zeros(rows, device=DEV), torch.zeros(rows, device=DEV)
        tok_r, fin_r, nid_r = tok_b.clone(), fin_b.clone(), nid.clone()
        hip_ops.sample_tokens(logits_d, 1.0, 50, seed, step_t(call), tok_a, fin_a, eos, pad, True, u_out=u_a, **cfg)
        hip_ops.sample_tokens(logits_d, 1.0, 50, seed, step_t(call), tok_b, fin_b, eos, pad, True, u_out=u_b, next_ids=nid, **cfg)
        hip_ops.sample_tokens(logits_d, 1.0, 50, seed, step_t(call), tok_r, fin_r, eos, pad, True, next_ids=nid_r, **cfg)      # the same call once more
        assert not bool(hip_ops._ws[("sampler_step_filtered", rows)].any()), "call %d left the cached workspace dirty" % call
        assert torch.equal(tok_a, tok_b) and torch.equal(fin_a, fin_b) and torch.equal(u_a, u_b), "call %d: step form differs from the one-shot form" % call
        assert torch.equal(tok_r, tok_b) and torch.equal(fin_r, fin_b) and torch.equal(nid_r, nid), "call %d: two identical calls differ" % call
        assert torch.equal(nid, tok_b[:, call])
        t, f, u = tok_b[:, call].cpu(), fin_b.cpu().bool(), u_b.cpu()
        for r in range(rows):
            if was_done[r]:
                assert int(t[r]) == pad and int(nid[r]) == pad
                continue
            keep, cdf, margin = fc.ref_filter(logits[r], 1.0, 50, **cfg)
            assert float(u[r]) == vc.philox_u(seed, r, call)
            if margin > vc.CDF_SLACK:
                e = vc.draw_error(keep, cdf, int(t[r]), float(u[r]))
                assert e is None, (call, r, e)
                n_checked += 1
            assert bool(f[r]) == (int(t[r]) == eos)
    assert bool(fin_b.any()) and n_checked >= rows * C // 2
    print("OBS filter step form V=%d: %d live draws checked over %d calls" % (V, n_checked, C))


# ------------------------------------------------------------------------------------------------------------ 5. penalty and bitmap
def penalty_logits(rows, V, seed):
    x = vc.sweep_rows(rows, V, seed=seed).float()
    x[:, 0], x[:, V - 1], x[:, 64], x[:, 65], x[:, 66] = -3.3, 7.1, 0.0, -0.0, -1e-3
    return x.to(BF16)


@pytest.mark.parametrize("penalty", [1.05, 2.0])
@pytest.mark.parametrize("V", [1001, vc.V_FULL])
def test_penalize_logits_bit_exact(hip_ops, V, penalty):
    """Against torch on the CPU (fp32 ops, .to(bfloat16)), bit for bit: contiguous rows, rows of a wider tensor (strided, unaligned base), and one row shown
    to all (stride 0); seen sets: empty, one token, token 0, token V - 1, a whole 32-bit word."""
    seen_lists = fc.penalty_seen_sets(V)
    rows = len(seen_lists)
    seen_d = fc.seen_bitmap(rows, V, seen_lists).to(DEV)
    logits = penalty_logits(rows, V, seed=31)
    want = fc.ref_penalize(logits, seen_lists, penalty)
    assert not torch.equal(bits(want), bits(logits))
    got = hip_ops.penalize_logits(logits.to(DEV), seen_d, penalty)
    assert torch.equal(bits(got).cpu(), bits(want)), "contiguous rows"
    wide = torch.full((rows, vc.ceil8(V) + 16), 64.0, dtype=BF16)
    wide[:, 3:3 + V] = logits
    view = wide.to(DEV)[:, 3:3 + V]
    out_store = torch.full((rows, vc.ceil8(V) + 8), 5.0, dtype=BF16, device=DEV)
    got = hip_ops.penalize_logits(view, seen_d, penalty, out=out_store[:, :V])
    assert torch.equal(bits(got).cpu(), bits(want)), "strided rows"
    assert bool((out_store[:, V:] == 5.0).all()), "nothing is written past V"
    one = logits[1:2]
    got = hip_ops.penalize_logits(one.to(DEV).expand(rows, V), seen_d, penalty)
    assert torch.equal(bits(got).cpu(), bits(fc.ref_penalize(one.expand(rows, V).contiguous(), seen_lists, penalty))), "stride-0 row"
    assert torch.equal(bits(logits.to(DEV)[1:2]).cpu(), bits(one)), "the input is left alone"


@pytest.mark.parametrize("V", [1001, vc.V_FULL])
def test_mark_seen(hip_ops, V):
    """Ids of a list go into every row, drawn tokens into their own row, finished rows are skipped, ids outside the vocabulary ignored, twice = once."""
    rows, W = 4, (V + 31) // 32
    seen = torch.zeros(rows, W, dtype=I32, device=DEV)
    ids = [0, 31, 32, 63, V - 1, V // 2, V // 2, 5]
    hip_ops.mark_seen(seen, V, ids=torch.tensor(ids + [V, -1, 2 ** 30], dtype=I32, device=DEV))
    want = [set(ids) for _ in range(rows)]
    assert [fc.bitmap_tokens(seen[r].cpu(), V) for r in range(rows)] == want
    tokens = torch.tensor([[7, 9, 1], [V - 2, 11, 1], [64, 13, 1], [V, 15, 1]], dtype=I32, device=DEV)
    fin = torch.tensor([0, 0, 1, 0], dtype=I32, device=DEV)
    for _ in range(2):
        hip_ops.mark_seen(seen, V, tokens=tokens, step_dev=step_t(1), finished=fin)      # column 1; row 2 is finished
    for r, t in ((0, 9), (1, 11), (3, 15)):
        want[r].add(t)
    assert [fc.bitmap_tokens(seen[r].cpu(), V) for r in range(rows)] == want
    hip_ops.mark_seen(seen, V, tokens=tokens[:, 0].contiguous())                          # a [rows] vector (next_ids), nobody finished; row 3's id V is outside
    for r, t in ((0, 7), (1, V - 2), (2, 64)):
        want[r].add(t)
    assert [fc.bitmap_tokens(seen[r].cpu(), V) for r in range(rows)] == want
    assert torch.equal(seen.cpu(), fc.seen_bitmap(rows, V, [sorted(s) for s in want]))


# ------------------------------------------------------------------------------------------------------------ 6. rollout
def test_rollout_with_filters_and_penalty(hip_ops):
    """A 2-layer tiny model, G = 4, C = 12, top_p = 0.8, min_p = 0.05, repetition_penalty = 1.3: the native and the host step forms give equal tokens, and the
    tokens replayed step by step through the reference with the logits the rollout produced (penalised on the host from the replayed seen sets, bit-equal to
    what the sampler was handed) all pass draw_error."""
    import time_r1_amd  # noqa: F401
    from time_r1_amd.config import tiny_test
    from time_r1_amd.params import ModelParams
    from time_r1_amd.model import Engine
    from time_r1_amd.grpo import GRPOCore
    from time_r1_amd.synthetic import synthetic_prompt
    cfg = tiny_test(n_layers=2)
    ops = hip_ops
    eng = Engine(cfg, ops, ModelParams(cfg, ops, seed=1))
    G, C, T, top_k, top_p, min_p, pen, seed = 4, 12, 0.9, 50, 0.8, 0.05, 1.3, 5
    ids, pix, grid = synthetic_prompt(cfg, (4, 6, 8), 9, 7, seed=2, text_vocab=400)
    outs, raw, handed, prompt = [], [], [], []
    orig_pen, orig_samp, orig_mark = ops.penalize_logits, ops.sample_tokens, ops.mark_seen

    def spy_pen(logits, *a, **k):
        raw.append(logits.cpu().clone())
        return orig_pen(logits, *a, **k)

    def spy_samp(logits, *a, **k):
        assert k.get("top_p") == top_p and k.get("min_p") == min_p
        handed.append(logits.cpu().clone())
        return orig_samp(logits, *a, **k)

    def spy_mark(seen, V, ids=None, **k):
        if ids is not None:
            prompt.append(ids.cpu().tolist())
        return orig_mark(seen, V, ids=ids, **k)

    for native in (True, False):
        core = GRPOCore(eng, None, G, C, beta=0.0, temperature=T, top_k=top_k, seed=seed, rope_index_mode="hf4", top_p=top_p, min_p=min_p, repetition_penalty=pen)
        core.roll.native_decode = native
        if native:
            ops.penalize_logits, ops.sample_tokens, ops.mark_seen = spy_pen, spy_samp, spy_mark
        try:
            st = core.prepare(ids, pix, grid)
            core.rollout(st)
        finally:
            ops.penalize_logits, ops.sample_tokens, ops.mark_seen = orig_pen, orig_samp, orig_mark
        outs.append(st.completion_ids.cpu())
    assert torch.equal(outs[0], outs[1]), "native and host step forms draw different tokens"
    toks = outs[0]
    V = raw[0].shape[1]
    assert len(raw) == C and len(handed) == C and len(prompt) == 1 and toks.shape == (G, C)
    seen = [set(t for t in prompt[0] if 0 <= t < V) for _ in range(G)]
    n_checked = 0
    for s in range(C):
        x = raw[s].expand(G, V).contiguous()                    # step 0: the one prefill row
        want = fc.ref_penalize(x, [sorted(q) for q in seen], pen)
        assert torch.equal(bits(handed[s].expand(G, V)), bits(want)), "step %d: the sampler was not handed the penalised logits" % s
        for r in range(G):
            keep, cdf, margin = fc.ref_filter(want[r], T, top_k, top_p, min_p)
            if margin > vc.CDF_SLACK:
                e = vc.draw_error(keep, cdf, int(toks[r, s]), vc.philox_u(seed, r, s))
                assert e is None, (s, r, e)
                n_checked += 1
            seen[r].add(int(toks[r, s]))
    assert n_checked >= G * C - 4, "nearly every draw is far enough from a filter boundary to be judged (%d of %d)" % (n_checked, G * C)
    assert any((x != y).any() for x, y in zip(raw, handed)), "the penalty changed some logit"
