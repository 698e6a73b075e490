"""LoRA on the MI355X: tr1_lora_merge against the fp32 chain of tests/lora_cases.py bit for bit, tr1_lora_wgrad (and the composition it replaces) against fp64
at the any-order bound, the torch ops, and the HIP engine / trainer against the CPU stand-in (adapter gradients, one optimizer step, the step-0 equalities, the
frozen tensors, an fp8 rollout behind the merge, resume).  Cases and references: tests/lora_cases.py."""
import pytest
import torch

import lora_cases as lc
import optim_cases as oc
import ref_sync_cases as sc
from helpers import golden_params, load_case
from oracle.ref_ops import RefOps

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32


# ------------------------------------------------------------------------------------------------------------------ lora_merge
def _merge_run(ops, w0, a, bt, s, layout):
    """layout "slice": W and W0 are row slices at row offset 3 of taller matrices (ld = in); "ld": views with ld = in + 8 inside sentinel frames."""
    out, in_ = w0.shape
    dev = ops.device
    if layout == "slice":
        wb = oc.fill_sentinel(torch.empty((out + 5) * in_, dtype=BF16)).view(out + 5, in_).to(dev)
        w0b = oc.fill_sentinel(torch.empty((out + 5) * in_, dtype=BF16)).view(out + 5, in_)
        w0b[3:3 + out] = w0
        w0b = w0b.to(dev)
        wv, w0v = wb[3:3 + out], w0b[3:3 + out]
        keep = torch.ones(out + 5, in_, dtype=torch.bool)
        keep[3:3 + out] = False
        want_frame = oc.fill_sentinel(torch.empty((out + 5) * in_, dtype=BF16)).view(out + 5, in_)
        intact = lambda: torch.equal(sc.bits(wb.cpu()[keep]), sc.bits(want_frame[keep]))
    else:
        wb, wv = oc.framed(torch.zeros(out, in_, dtype=BF16), rows=2, cols=8, dev=dev)
        w0b, w0v = oc.framed(w0, rows=2, cols=8, dev=dev)
        intact = lambda: oc.frame_intact(wb, out, in_, rows=2)
    ad, btd = a.to(dev), bt.to(dev)
    ops.lora_merge(wv, w0v, ad, btd, s)
    assert intact(), "the rows / columns around W keep their bits"
    assert sc.same_bits(w0v, w0) and torch.equal(ad.cpu(), a) and torch.equal(btd.cpu(), bt), "W0, A and Bt are read only"
    return wv.cpu()


@pytest.mark.parametrize("out,in_", lc.MERGE_SHAPES)
def test_merge_is_the_fp32_chain_bit_for_bit(hip_ops, out, in_):
    for r in lc.MERGE_RANKS:
        for big, seed in lc.MERGE_DATA:
            w0, a, bt = lc.merge_data(out, in_, r, seed=seed, big=big)
            for s in lc.MERGE_SCALES:
                want = lc.merge_composite(w0, a, bt, s)
                for layout in ("slice", "ld"):
                    got = _merge_run(hip_ops, w0, a, bt, s, layout)
                    assert sc.same_bits(got, want), (out, in_, r, s, big, seed, layout, int((sc.bits(got) != sc.bits(want)).sum()))
                if s == 0.0:
                    assert sc.identity_ok(got, w0, lc.merge_acc(a, bt).to(BF16)), "s = 0 returns W0 (a zero takes the sign IEEE addition gives it)"


def test_merge_bad_arguments_are_errors(hip_ops):
    from time_r1_amd.hip import HipError
    dev = hip_ops.device
    w0, a, bt = [t.to(dev) for t in lc.merge_data(24, 72, 16)]
    w = torch.empty_like(w0)
    with pytest.raises(HipError, match="aliases"):
        hip_ops.lora_merge(w0, w0, a, bt, 1.0)
    with pytest.raises(HipError, match="r must be"):
        hip_ops.lora_merge(w, w0, a[:8].contiguous(), bt[:8].contiguous(), 1.0)
    with pytest.raises(HipError, match="multiples of 8"):
        hip_ops.lora_merge(w[:, :68], w0[:, :68], a[:, :68].contiguous(), bt, 1.0)


# ------------------------------------------------------------------------------------------------------------------ lora_wgrad
def _wgrad_run(ops, thin, wide, g0, scale, accumulate, composed=False):
    """thin in a frame with ldt = r + 8; wide as a column slice at column offset 8 of an [M + 2, Wd + 16] matrix; G in a frame with ldg = Wd + 8."""
    M, Wd = wide.shape
    r = thin.shape[1]
    dev = ops.device
    tb, tv = oc.framed(thin, rows=1, cols=8, dev=dev)
    wb = oc.fill_sentinel(torch.empty((M + 2) * (Wd + 16), dtype=BF16)).view(M + 2, Wd + 16)
    wb[1:M + 1, 8:8 + Wd] = wide
    wb = wb.to(dev)
    wv = wb[1:M + 1, 8:8 + Wd]
    gb, gv = oc.framed(g0, rows=1, cols=8, dev=dev)
    (ops.lora_wgrad_composed if composed else ops.lora_wgrad)(gv, tv, wv, scale, accumulate=accumulate)
    assert oc.frame_intact(gb, r, Wd, rows=1), "the columns of G past Wd and the rows around it keep their bits"
    assert oc.frame_intact(tb, M, r, rows=1) and sc.same_bits(tv, thin) and sc.same_bits(wv, wide), "both operands are read only"
    return gv.cpu()


@pytest.mark.parametrize("M", [1, 63, 64, 65, 300, "chunk+1"])
def test_wgrad_against_fp64_at_the_any_order_bound(hip_ops, M):
    """M: one row, around one 64-row transposed tile of the composition and half a staged step of the kernel, several steps with a ragged end, and one row more
    than the kernel's M-chunk (two splits at every width here: the planes + fixed-order reduction path)."""
    M = hip_ops.LORA_WGRAD_MCHUNK + 1 if M == "chunk+1" else M
    worst = 0.0
    for Wd in lc.WGRAD_WIDTHS:
        assert hip_ops.lora_wgrad_splits(M, Wd)[0] == (2 if M > hip_ops.LORA_WGRAD_MCHUNK else 1)
        for r in lc.WGRAD_RANKS:
            for scale in lc.WGRAD_SCALES:
                thin, wide, g0 = lc.wgrad_data(M, Wd, r, scale)
                for accumulate in (False, True):
                    want, bound = lc.wgrad64(thin, wide, scale, g0 if accumulate else None)
                    if M == 300:
                        drop = float(lc.f32(scale)) * (thin[-1].double()[:, None] * wide[-1].double()[None, :]).abs()
                        assert bool((drop > bound).any()), "a kernel that loses one row must miss the bound on this data"
                    got = _wgrad_run(hip_ops, thin, wide, g0, scale, accumulate)
                    err = (got.double() - want).abs()
                    worst = max(worst, float((err / bound.clamp(min=1e-300)).max()))
                    assert bool((err <= bound).all()), (M, Wd, r, scale, accumulate, float((err / bound.clamp(min=1e-300)).max()))
                    again = _wgrad_run(hip_ops, thin, wide, g0, scale, accumulate)
                    assert torch.equal(sc.bits(again), sc.bits(got)), "the same inputs give the same bits"
                    comp = _wgrad_run(hip_ops, thin, wide, g0, scale, accumulate, composed=True)
                    cerr = (comp.double() - want).abs()
                    assert bool((cerr <= bound).all()), ("composition", M, Wd, r, scale, accumulate, float((cerr / bound.clamp(min=1e-300)).max()))
    print("M=%d: worst error / bound = %.4f" % (M, worst))


def test_wgrad_routes_uncovered_shapes_to_the_composition(hip_ops):
    """A rank the kernel has no instance for (48) is outside it: lora_wgrad composes the product and meets the same bound."""
    M, Wd, r = 65, 136, 48
    thin, wide, g0 = lc.wgrad_data(M, Wd, r)
    dev = hip_ops.device
    tv, wv, g = thin.to(dev), wide.to(dev), g0.clone().to(dev)
    assert not hip_ops.lora_wgrad_covers(g, tv, wv)
    hip_ops.lora_wgrad(g, tv, wv, 1.0, accumulate=True)
    want, bound = lc.wgrad64(thin, wide, 1.0, g0)
    assert bool(((g.cpu().double() - want).abs() <= bound).all())


def test_torch_ops_are_registered_with_fakes(hip_ops):
    import time_r1_amd.torch_ops as T
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert "lora_merge" in T.OP_NAMES and "lora_wgrad" in T.OP_NAMES
    assert "Tensor(a0!) w" in str(torch.ops.timer1.lora_merge.default._schema) and "Tensor(a0!) g" in str(torch.ops.timer1.lora_wgrad.default._schema)
    dev = hip_ops.device
    w0, a, bt = lc.merge_data(24, 72, 16)
    w = torch.empty_like(w0).to(dev)
    torch.ops.timer1.lora_merge(w, w0.to(dev), a.to(dev), bt.to(dev), 0.25)
    assert sc.same_bits(w, lc.merge_composite(w0, a, bt, 0.25))
    thin, wide, g0 = lc.wgrad_data(65, 136, 16)
    g = g0.clone().to(dev)
    torch.ops.timer1.lora_wgrad(g, thin.to(dev), wide.to(dev), 2.0, True)
    want, bound = lc.wgrad64(thin, wide, 2.0, g0)
    assert bool(((g.cpu().double() - want).abs() <= bound).all())
    with FakeTensorMode():
        e = lambda *s, dt=BF16: torch.empty(*s, dtype=dt, device="cuda")
        assert torch.ops.timer1.lora_merge(e(24, 72), e(24, 72), e(16, 72, dt=F32), e(16, 24, dt=F32), 0.25) is None
        assert torch.ops.timer1.lora_wgrad(e(16, 136, dt=F32), e(65, 16), e(65, 136), 2.0, True) is None
    with pytest.raises(NotImplementedError):
        torch.ops.timer1.lora_merge(torch.empty_like(w0), w0, a, bt, 0.25)


# ------------------------------------------------------------------------------------------------------------------ engine / trainer on HipOps
CASES = {"qwen2_vl": "clip_beta", "qwen2_5_vl": "q25_clip_beta_ragged"}


def _pair(hip_ops, fx, tmp_path, peft, **over):
    """The HIP trainer and the CPU stand-in trainer on the same (bf16-representable) weights."""
    _, pol_h, _ = golden_params(hip_ops, fx)
    cpu = RefOps()
    _, pol_c, _ = golden_params(cpu, fx)
    pol_c.train.w16.copy_(pol_h.train.w16.float().cpu())
    pol_c.frozen.w16.copy_(pol_h.frozen.w16.float().cpu())
    th = lc.tiny_lora_trainer(hip_ops, fx, tmp_path / "hip", peft, pol=pol_h, **over)
    tc = lc.tiny_lora_trainer(cpu, fx, tmp_path / "cpu", peft, pol=pol_c, **over)
    return th, tc


def _set_bt(tr, seed=11):
    """Random Bt (bf16-representable) in every adapter, then the merge: with peft's Bt = 0 every dA is identically zero."""
    a, lora = tr.lora.train, tr.lora
    g = torch.Generator().manual_seed(seed)
    for i in range(tr.cfg.text.n_layers):
        for m, _, _, out, _ in lora.slices:
            bt = a.view(a.master, lora.name(i, m, "Bt"))
            bt[:lora.spec.r].copy_((torch.randn(lora.spec.r, out, generator=g) * 0.05).to(BF16).float())
    a.w16.copy_(a.master)
    lora.merge()


@pytest.mark.parametrize("variant", list(CASES))
@pytest.mark.parametrize("peft", [lc.ALL_LINEAR, lc.QV], ids=["all-linear-r16", "qv-r8"])
def test_adapter_gradients_and_one_step_against_the_cpu_stand_in(hip_ops, tmp_path, variant, peft):
    """The fixture's forced completions through compute_loss on both backends: every adapter gradient within the relative L2 of test_trainer_gpu.py's weight
    gradients (0.06), then one optimizer step + merge: the merged weights within that file's tolerance for updated weights (atol 1e-2), the frozen tensors
    untouched."""
    from helpers import frames_for
    fx = load_case(CASES[variant])
    th, tc = _pair(hip_ops, fx, tmp_path, peft)
    w_start = th.params.train.w16.clone()
    grads = []
    for tr in (th, tc):
        _set_bt(tr)
        frames = frames_for(fx)
        tr._video_inputs = lambda ex, f=frames: ([f], [2.0])
        row = dict(fx["row"])
        row["_forced_completion_ids"] = fx["completion_ids"].numpy()
        tr.compute_loss(tr.model, [row])
        a = tr.lora.train
        grads.append({n: a.g(n).detach().float().cpu().clone() for n in a.names()})
    worst = 0.0
    for n, gold in grads[1].items():
        assert float(gold.norm()) > 0, n
        rel = float((grads[0][n] - gold).norm() / gold.norm().clamp(min=1e-12))
        worst = max(worst, rel)
        assert rel < 0.06, (n, rel)
    print("worst adapter-gradient relative L2: %.4f" % worst)
    for tr in (th, tc):
        tr._optimizer_step(None, save=False)
    assert torch.allclose(th.params.train.w16.float().cpu(), tc.params.train.w16.float(), atol=1e-2)
    # (that tolerance is far above one step's s Bt^T A; this one bites) every merged matrix is the pinned fp32 chain of the base copy and the HIP masters
    lora, a = th.lora, th.lora.train
    for i in range(th.cfg.text.n_layers):
        for mod, mat, r0, out, _ in lora.slices:
            key = "l%d.%s.w" % (i, mat)
            want = lc.merge_composite(lora.base.w(key)[r0:r0 + out].cpu(), a.view(a.master, lora.name(i, mod, "A")).cpu(),
                                      a.view(a.master, lora.name(i, mod, "Bt")).cpu(), lora.spec.scale)
            assert sc.same_bits(th.params.train.w(key)[r0:r0 + out].cpu(), want), (key, mod)
    m = lc.targeted_mask(th)
    w_now = th.params.train.w16.cpu()
    assert torch.equal(w_now[~m], w_start.cpu()[~m]) and bool((w_now[m] != th.lora.base.w16.cpu()[m]).any())
    assert float(th.lora.train.grad.abs().max()) == 0.0, "AdamW zeroes the adapter gradients"


@pytest.mark.parametrize("variant", list(CASES))
def test_step_zero_equalities_and_frozen_tensors(hip_ops, tmp_path, variant):
    """Bt = 0 at construction: the merged weights are the loaded ones and the first micro-step's log-probs are the full-parameter trainer's bit for bit; after 3
    steps the base copy and every untargeted tensor keep their bits, the targeted ones moved."""
    fx = load_case(CASES[variant])
    _, pol, _ = golden_params(hip_ops, fx)
    loaded = pol.train.w16.clone()
    tr = lc.tiny_lora_trainer(hip_ops, fx, tmp_path / "lora", lc.QV, pol=pol)
    a = tr.params.train
    assert torch.equal(a.w16, loaded) and a.grad is None and a.master is None and a.m is None and a.v is None
    assert tr.ref_model is tr.lora.base and torch.equal(tr.lora.base.w16, loaded)
    snaps, first = lc.run_snapshots(tr)
    full = lc.tiny_lora_trainer(hip_ops, fx, tmp_path / "full", None)
    _, first_full = lc.run_snapshots(full)
    assert torch.equal(first["logp"], first_full["logp"])
    assert tr.state.log_history[1]["kl"] > 0
    assert [s["step"] for s in snaps] == [1, 2, 3]
    m = lc.targeted_mask(tr)
    end = snaps[-1]
    assert torch.equal(end["base"], loaded.cpu()) and torch.equal(end["w"][~m], loaded.cpu()[~m])
    o_off, o_shape = a.offsets["l0.o.w"]
    assert not bool(m[o_off: o_off + o_shape[0] * o_shape[1]].any()), "o_proj is not targeted by q/v adapters"
    assert bool((end["w"][m] != loaded.cpu()[m]).any())


@pytest.mark.parametrize("variant", list(CASES))
def test_step_zero_kl_is_exactly_zero(hip_ops, tmp_path, variant):
    """The merged policy IS the reference (the base copy) at step 0, and in LoRA mode the reference's forward takes the policy's two launches (prompt rows, then
    completion rows over a K/V cache: GRPOCore._ref_split_fwd), so the first step's KL is exactly 0.  The full-parameter trainer whose reference is a clone of
    its policy is printed beside it: its reference runs one pass over all rows, whose GEMM tiles follow another row count, and on tiny_test_25 its KL is
    5.6e-8 (12 of 32 log-probs differ in a last bf16 place) - the one-pass form gave the LoRA trainer the same figure."""
    fx = load_case(CASES[variant])
    tr = lc.tiny_lora_trainer(hip_ops, fx, tmp_path / "lora", lc.QV, n_rows=1)
    _, first = lc.run_snapshots(tr)
    full = lc.tiny_lora_trainer(hip_ops, fx, tmp_path / "full", None, n_rows=1)
    _, first_full = lc.run_snapshots(full)
    kl, kl_full = tr.state.log_history[0]["kl"], full.state.log_history[0]["kl"]
    d = (first["logp"].double() - first["ref_logp"].double()).abs()
    print("%s: step-0 kl %r (full-parameter trainer with reference = policy: %r); log-probs that differ from the reference's: %d of %d, largest %.3g"
          % (variant, kl, kl_full, int((d > 0).sum()), d.numel(), float(d.max())))
    assert kl == 0.0, kl


@pytest.mark.parametrize("shape", [(70, 4, 8), (37, 3, 5)], ids=lambda s: "P%d-G%d-C%d" % s)
@pytest.mark.parametrize("head_dim,section", [(32, (4, 6, 6)), (128, (16, 24, 24))], ids=["hd32", "hd128"])
def test_reference_forward_takes_the_policys_launches(hip_ops, head_dim, section, shape):
    """Engine level, Bt = 0 (merged weights == base copy): after prepare -> rollout -> forward_logps the reference's log-probs equal the policy's bit for bit.
    Head dim 128 is the production attention path (K and V read row-major: the reference's own V buffer, llm_fwd(v_cache=...)); head dim 32 reads V^T from the
    cache.  33 and 16 prediction rows: one above and well below the 32-row boundary of the skinny GEMMs."""
    import recompute_cases as rcc
    from time_r1_amd.config import TextConfig, tiny_test_25
    from time_r1_amd.grpo import GRPOCore
    from time_r1_amd.lora import LoraAdapters, LoraSpec
    from time_r1_amd.model import Engine
    from time_r1_amd.params import ModelParams
    P, G, C = shape
    cfg = tiny_test_25()
    if head_dim == 128:      # (the head-dim-128 decoder of test_trainer_gpu.py)
        cfg.text = TextConfig(vocab_size=512, hidden=512, intermediate=1024, n_layers=2, n_heads=4, n_kv_heads=2, head_dim=128, mrope_section=section)
        cfg.vision.out_hidden = 512
    assert cfg.text.head_dim == head_dim and tuple(cfg.text.mrope_section) == section
    pol = ModelParams(cfg, hip_ops, seed=1, optimizer_state=False, with_grad=False)
    eng = Engine(cfg, hip_ops, pol)
    lora = eng.lora = LoraAdapters(pol, LoraSpec(r=16, lora_alpha=32, target_modules="all-linear"), seed=3)
    assert torch.equal(pol.train.w16, lora.base.w16)
    core = GRPOCore(eng, lora.base, G, C, beta=0.04, use_grpo=False, seed=3, rope_index_mode="hf4", reuse_prefill=True)
    ids, pix, g3 = rcc.prompt_for(cfg, P)
    st = core.prepare(ids, pix, g3)
    core.rollout(st)
    core.forward_logps(st)
    d = (st.logp.double() - st.ref_logp.double()).abs()
    print("head dim %d, P %d, G*C %d: log-probs that differ from the reference's: %d of %d, largest %.3g" % (head_dim, P, G * C, int((d > 0).sum()), d.numel(), float(d.max())))
    assert bool(torch.isfinite(st.logp).all()) and torch.equal(st.logp, st.ref_logp)


def test_fp8_rollout_copies_follow_the_merge(hip_ops, tmp_path):
    """rollout_weight_dtype="fp8": the second rollout's fp8 codes are those of the weights the first step's merge wrote, not of the base weights."""
    fx = load_case("clip_beta")
    tr = lc.tiny_lora_trainer(hip_ops, fx, tmp_path, lc.ALL_LINEAR, n_rows=2, rollout_weight_dtype="fp8")
    want = {}

    class CB:
        def on_step_end(self, args, state, control, **kw):
            if state.global_step == 1:
                want["merged"] = hip_ops.quantize_fp8_rows(tr.params.train.w("l0.qkv.w"))[0].clone()
                want["base"] = hip_ops.quantize_fp8_rows(tr.lora.base.w("l0.qkv.w"))[0].clone()
    snaps, _ = lc.run_snapshots(tr, callbacks=[CB()])
    assert len(snaps) == 2 and all(bool(torch.isfinite(torch.tensor(l["loss"]))) for l in tr.state.log_history)
    codes = tr.core.roll._w8["layers"][0]["qkv.w"][0]
    assert torch.equal(codes, want["merged"]) and not torch.equal(codes, want["base"])


def test_resume_is_bit_for_bit(hip_ops, tmp_path):
    fx = load_case("clip_beta")
    tr = lc.tiny_lora_trainer(hip_ops, fx, tmp_path / "a", lc.ALL_LINEAR, n_rows=4, save_steps=2)
    snaps, _ = lc.run_snapshots(tr)
    tr2 = lc.tiny_lora_trainer(hip_ops, fx, tmp_path / "b", lc.ALL_LINEAR, n_rows=4)
    snaps2, _ = lc.run_snapshots(tr2, ckpt=str(tmp_path / "a" / "checkpoint-2"))
    assert [s["step"] for s in snaps2] == [3, 4]
    for k in ("w", "base", "master"):
        assert sc.same_bits(snaps2[0][k], snaps[2][k]) and sc.same_bits(snaps2[1][k], snaps[3][k]), k
    strip = lambda l: {k: v for k, v in l.items() if k in ("loss", "kl", "reward", "grad_norm", "generation_entropy")}
    assert [strip(l) for l in tr2.state.log_history[-2:]] == [strip(l) for l in tr.state.log_history[-2:]]
