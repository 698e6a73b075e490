"""Several clipped policy updates per rollout on the MI355X: tr1_grpo_loss_ratio against the fp64 reference of tests/ratio_cases.py (the cases and
tolerances of tests/vocab_cases.py), its determinism, the torch op under autograd, and the trainer's replay path on HipOps."""
import itertools

import pytest
import torch

import ratio_cases as rc
import vocab_cases as vc

pytestmark = pytest.mark.gpu


def _dev(c, ops):
    return {k: (v.to(ops.device).contiguous() if torch.is_tensor(v) else v) for k, v in c.items()}


@pytest.mark.parametrize("G,C", vc.GRPO_SHAPES)
def test_kernel_against_fp64_reference(hip_ops, G, C):
    """GRPO_SHAPES: one row, one column, 257 columns (no multiple of the 256-thread block), 64 rows (the limit), C = 1024 (four elements per thread)."""
    worst = 0.0
    for eps in rc.EPS_PAIRS:
        c = rc.ratio_case(G, C, eps)
        d = _dev(c, hip_ops)
        dead = (c["mask"] == 0)
        for beta, use_grpo, with_w, gs in itertools.product((0.0, 0.04), (False, True), (False, True), (1.0, 0.5)):
            w = c["tok_weight"] if with_w else None
            ref = rc.ref_grpo_ratio(c["logp"], c["old_logp"], c["ref_logp"], w, c["mask"], c["adv"], beta, use_grpo, eps[0], eps[1], gs)
            got = hip_ops.grpo_loss_ratio(d["logp"], d["old_logp"], d["ref_logp"], d["mask"], d["adv"], beta, use_grpo, eps[0], eps[1], gs,
                                          tok_weight=d["tok_weight"] if with_w else None)
            got = [t.cpu() for t in got]
            for name, a, b in zip(("dlogp", "out8", "row_len", "row_kl"), got, ref):
                assert torch.isfinite(a).all(), name
                r = vc.worst(a, b, vc.TOL_GRPO)[0]
                worst = max(worst, r)
                assert r <= 1.0, (name, eps, beta, use_grpo, with_w, gs, r)
            assert torch.allclose(got[1][3:6].double(), ref[1][3:6], atol=1e-6, rtol=0), (got[1][3:6], ref[1][3:6])
            assert bool((got[0][dead] == 0).all())
    print("G=%d C=%d: worst share of TOL_GRPO %.4f" % (G, C, worst))


@pytest.mark.parametrize("G,C", [(8, 200), (3, 257), (1, 1)])
@pytest.mark.parametrize("use_grpo", [False, True])
def test_old_policy_equal_to_policy_is_the_one_update_kernel(hip_ops, G, C, use_grpo):
    logp, ref, mask, adv = [t.to(hip_ops.device).contiguous() for t in vc.grpo_case(G, C)]
    for beta, gs in ((0.0, 1.0), (0.04, 0.5)):
        a = hip_ops.grpo_loss_ratio(logp, logp.clone(), ref, mask, adv, beta, use_grpo, 0.2, 0.2, gs)
        b = hip_ops.grpo_loss(logp, ref, mask, adv, beta, use_grpo, gs)
        assert vc.worst(a[0], b[0], vc.TOL_GRPO)[0] <= 1.0 and vc.worst(a[1][:3], b[1], vc.TOL_GRPO)[0] <= 1.0
        assert vc.worst(a[2], b[2], vc.TOL_GRPO)[0] <= 1.0 and vc.worst(a[3], b[3], vc.TOL_GRPO)[0] <= 1.0
        o = a[1].cpu()
        assert bool((o[3:7] == 0).all()) and float(o[7]) == 1.0, o


def test_two_calls_give_the_same_bits_and_leave_the_workspace_zero(hip_ops):
    d = _dev(rc.ratio_case(16, 1024, (0.2, 0.28)), hip_ops)
    outs = []
    for _ in range(2):
        r = hip_ops.grpo_loss_ratio(d["logp"], d["old_logp"], d["ref_logp"], d["mask"], d["adv"], 0.04, False, 0.2, 0.28, 0.5, tok_weight=d["tok_weight"])
        outs.append([t.clone() for t in r])
    ws = [v for k, v in hip_ops._ws.items() if k[0] == "grpo_loss_ratio"]
    assert len(ws) == 1 and ws[0].numel() == hip_ops.grpo_loss_ratio_ws_words() == 528
    assert int(ws[0].view(torch.int32)[0]) == 0, "the ticket counter must be zero again after a call"
    for a, b in zip(*outs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_more_than_64_rows_is_an_error(hip_ops):
    from time_r1_amd.hip import HipError
    d = _dev(rc.ratio_case(64, 300, (0.2, 0.2)), hip_ops)
    big = {k: torch.cat([v, v[:1]]).contiguous() for k, v in d.items() if torch.is_tensor(v)}
    assert big["logp"].shape[0] == 65
    with pytest.raises(HipError):
        hip_ops.grpo_loss_ratio(big["logp"], big["old_logp"], big["ref_logp"], big["mask"], big["adv"], 0.04, False, 0.2, 0.2)


def test_torch_op_under_autograd(hip_ops):
    import time_r1_amd.torch_ops as T
    assert "grpo_loss_ratio" in T.OP_NAMES
    c = rc.ratio_case(8, 200, (0.2, 0.28))
    d = _dev(c, hip_ops)
    lp = d["logp"].clone().requires_grad_(True)
    loss, kl, stats = T.grpo_loss_ratio(lp, d["old_logp"], d["ref_logp"], d["mask"], d["adv"], 0.04, False, 0.2, 0.28, tok_weight=d["tok_weight"])
    (3.0 * loss).backward()
    dlogp, out8, _, _ = hip_ops.grpo_loss_ratio(d["logp"], d["old_logp"], d["ref_logp"], d["mask"], d["adv"], 0.04, False, 0.2, 0.28, 1.0, tok_weight=d["tok_weight"])
    assert torch.equal(lp.grad, dlogp * 3.0)
    assert float(loss) == float(out8[0]) and float(kl) == float(out8[1]) and torch.equal(stats, out8[3:])
    ref = rc.ref_grpo_ratio(c["logp"], c["old_logp"], c["ref_logp"], c["tok_weight"], c["mask"], c["adv"], 0.04, False, 0.2, 0.28, 3.0)
    assert vc.worst(lp.grad, ref[0], vc.TOL_GRPO)[0] <= 1.0


def test_two_updates_per_rollout_and_resume_on_hip(hip_ops, tmp_path):
    """The scenario of test_policy_reuse_ref.py on HipOps with the default batched rollout: step arithmetic, rollout and reference-forward counts, step 1 equal
    to the mu = 1 run's within 2e-6 (the bound of test_configs_gpu.py's resume test: atomics ordering in the embedding gradient), metric keys, resume."""
    fx, tr2, _ = rc.check_reuse_scenario(hip_ops, tmp_path, atol_step1=2e-6)
    rc.check_resume(hip_ops, tmp_path, fx, tr2, atol=2e-6)


def test_replay_with_an_fp8_sampling_policy_passes_the_importance_weight_into_the_kernel(hip_ops, tmp_path):
    from helpers import load_case
    tr = rc.tiny_trainer(hip_ops, load_case("clip_beta"), tmp_path, mu=2, ga=2, n_rows=2, rollout_weight_dtype="fp8")
    assert tr._is_cap is not None
    seen = []
    orig = hip_ops.grpo_loss_ratio

    def spy(*a, **k):
        seen.append(k.get("tok_weight"))
        return orig(*a, **k)
    hip_ops.grpo_loss_ratio = spy
    try:
        rc.run_recorded(tr)
    finally:
        del hip_ops.grpo_loss_ratio
    assert tr.state.global_step == 2 and len(seen) == 2
    for w in seen:
        assert w is not None and w.dtype == torch.float32 and float(w.max()) <= tr._is_cap and float(w.min()) > 0
    log = tr.state.log_history[1]
    assert all(k in log for k in rc.REPLAY_KEYS) and "rollout_logp_drift" not in log and "rollout_logp_drift" in tr.state.log_history[0]


@pytest.mark.parametrize("fix_vit", [True, False])
def test_replay_on_unchanged_weights_reproduces_the_first_pass_gradient(hip_ops, tmp_path, fix_vit):
    """Both passes compute the same gradient in bf16 through different kernel paths (prefill + continuation against one forward over the packed sequence), and
    each is held within 6 % of fp32 by test_trainer_gpu.py; a replay that read a wrong buffer or a stale activation would be off by its whole size."""
    g1, g2, m = rc.first_pass_and_replay_grads(hip_ops, tmp_path, fix_vit)
    rel = float((g1 - g2).norm() / g1.norm())
    print("relative L2 distance of the replay gradient:", rel)
    assert float(g1.norm()) > 0 and rel <= 0.06, rel
    assert m["clip_ratio/region_mean"] == 0.0 and m["policy_kl_old"] < 1e-3
