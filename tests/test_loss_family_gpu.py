"""The GRPO objective family on the MI355X: tr1_grpo_policy_loss against the fp64 reference of tests/loss_family_cases.py (the shapes and tolerances of
tests/vocab_cases.py), against tr1_grpo_loss_ratio where the two coincide, its determinism, the torch op under autograd, and the trainer on HipOps."""
import pytest
import torch

import loss_family_cases as fc
import ratio_cases as rc
import vocab_cases as vc

pytestmark = pytest.mark.gpu


def _dev(c, ops):
    return {k: (v.to(ops.device).contiguous() if torch.is_tensor(v) else v) for k, v in c.items() if k != "empty"}


def _against_reference(hip_ops, c, eps):
    d, dead, worst = _dev(c, hip_ops), c["mask"] == 0, 0.0
    for norm, level, delta, beta, with_w in fc.settings():
        w = c["tok_weight"] if with_w else None
        ref = fc.ref_policy_loss(c["logp"], c["old_logp"], c["ref_logp"], w, c["mask"], c["adv"], beta, norm, level, eps[0], eps[1], delta, 0.5)
        got = hip_ops.grpo_policy_loss(d["logp"], d["old_logp"], d["ref_logp"], d["mask"], d["adv"], beta, norm, level, eps[0], eps[1], delta, 0.5,
                                       tok_weight=d["tok_weight"] if with_w else None)
        r = fc.compare([t.cpu() for t in got], ref, dead, (eps, norm, level, delta, beta, with_w))
        assert r <= 1.0, (eps, norm, level, delta, beta, with_w, r)
        worst = max(worst, r)
    return worst


@pytest.mark.parametrize("G,C", vc.GRPO_SHAPES)
def test_kernel_against_fp64_reference(hip_ops, G, C):
    """GRPO_SHAPES: one row, one column, 257 columns (no multiple of the 256-thread block), 64 rows (the limit), C = 1024 (four elements per thread); every
    norm x level x delta on / off x beta x tok_weight on / off, rows in all five clip regimes."""
    worst = max(_against_reference(hip_ops, fc.family_case(G, C, eps), eps) for eps in rc.EPS_PAIRS)
    print("G=%d C=%d: worst share of TOL_GRPO %.4f" % (G, C, worst))


@pytest.mark.parametrize("G,C", fc.EMPTY_SHAPES)
def test_rows_without_a_live_token(hip_ops, G, C):
    """Row 1 and the last row fully masked, then the whole grid: zeros, nothing non-finite (compare() checks both against the clamped fp64 reference)."""
    eps = rc.EPS_PAIRS[1]
    e = fc.family_case(G, C, eps)["empty"]
    worst = _against_reference(hip_ops, e, eps)
    print("G=%d C=%d with empty rows: worst share of TOL_GRPO %.4f" % (G, C, worst))
    d = _dev(e, hip_ops)
    for norm in fc.NORMS:
        for level in fc.LEVELS:
            got = hip_ops.grpo_policy_loss(d["logp"], d["old_logp"], d["ref_logp"], torch.zeros_like(d["mask"]), d["adv"], 0.04, norm, level, 0.2, 0.28, fc.DELTA,
                                           tok_weight=d["tok_weight"])
            assert all(bool((t == 0).all()) for t in got), (norm, level, got[1])


@pytest.mark.parametrize("G,C", [(8, 200), (3, 257), (1, 1), (64, 300)])
def test_token_mean_at_token_level_without_a_cap_is_the_ratio_kernel(hip_ops, G, C):
    """Both entry points launch one kernel, here with the same arguments but the floor of the token counts, which no row of these cases reaches: equal floats."""
    eps = rc.EPS_PAIRS[1]
    d = _dev(fc.family_case(G, C, eps), hip_ops)
    for beta, gs, w in ((0.0, 1.0, None), (0.04, 0.5, d["tok_weight"])):
        a = hip_ops.grpo_policy_loss(d["logp"], d["old_logp"], d["ref_logp"], d["mask"], d["adv"], beta, "token", "token", eps[0], eps[1], None, gs, tok_weight=w)
        b = hip_ops.grpo_loss_ratio(d["logp"], d["old_logp"], d["ref_logp"], d["mask"], d["adv"], beta, False, eps[0], eps[1], gs, tok_weight=w)
        for x, y in zip(a, b):
            assert torch.isfinite(x).all() and torch.equal(x, y)
        assert torch.equal(a[1][2:6], b[1][2:6])          # counts: exact


def test_two_calls_give_the_same_bits_and_leave_the_workspace_zero(hip_ops):
    d = _dev(fc.family_case(16, 1024, (0.2, 0.28)), hip_ops)
    for level in fc.LEVELS:
        outs = []
        for _ in range(2):
            r = hip_ops.grpo_policy_loss(d["logp"], d["old_logp"], d["ref_logp"], d["mask"], d["adv"], 0.04, "row", level, 0.2, 0.28, fc.DELTA, 0.5,
                                         tok_weight=d["tok_weight"])
            outs.append([t.clone() for t in r])
        for a, b in zip(*outs):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    ws = [v for k, v in hip_ops._ws.items() if k[0] == "grpo_policy_loss"]
    assert len(ws) == 1 and ws[0].numel() == hip_ops.grpo_policy_loss_ws_words() == 528
    assert int(ws[0].view(torch.int32)[0]) == 0, "the ticket counter must be zero again after a call"


def test_more_than_64_rows_is_an_error(hip_ops):
    from time_r1_amd.hip import HipError
    d = _dev(fc.family_case(64, 300, (0.2, 0.2)), hip_ops)
    big = {k: torch.cat([v, v[:1]]).contiguous() for k, v in d.items() if torch.is_tensor(v)}
    assert big["logp"].shape[0] == 65
    with pytest.raises(HipError):
        hip_ops.grpo_policy_loss(big["logp"], big["old_logp"], big["ref_logp"], big["mask"], big["adv"], 0.04, "row", "sequence", 0.2, 0.2)


def test_torch_op_under_autograd(hip_ops):
    import time_r1_amd.torch_ops as T
    assert "grpo_policy_loss" in T.OP_NAMES
    c = fc.family_case(8, 200, (0.2, 0.28))
    d = _dev(c, hip_ops)
    lp = d["logp"].clone().requires_grad_(True)
    loss, kl, stats = T.grpo_policy_loss(lp, d["old_logp"], d["ref_logp"], d["mask"], d["adv"], 0.04, "dr_grpo", "sequence", 0.2, 0.28, delta=fc.DELTA,
                                         tok_weight=d["tok_weight"])
    (3.0 * loss).backward()
    dlogp, out8, _, _ = hip_ops.grpo_policy_loss(d["logp"], d["old_logp"], d["ref_logp"], d["mask"], d["adv"], 0.04, "fixed", "sequence", 0.2, 0.28, fc.DELTA, 1.0,
                                                 tok_weight=d["tok_weight"])
    assert torch.equal(lp.grad, dlogp * 3.0)
    assert float(loss) == float(out8[0]) and float(kl) == float(out8[1]) and torch.equal(stats, out8[3:])
    ref = fc.ref_policy_loss(c["logp"], c["old_logp"], c["ref_logp"], c["tok_weight"], c["mask"], c["adv"], 0.04, 2, 1, 0.2, 0.28, fc.DELTA, 3.0)
    assert vc.worst(lp.grad, ref[0], vc.TOL_GRPO)[0] <= 1.0


def test_bnpo_and_the_sequence_level_reach_the_legacy_first_step_on_hip(hip_ops, tmp_path):
    """2e-6: the bound test_policy_reuse_gpu.py holds two runs of the same step to (atomics ordering in the embedding gradient)."""
    fc.check_first_step_equals_legacy(hip_ops, tmp_path, 2e-6)


def test_all_truncated_completions_leave_the_weights_bit_unchanged_on_hip(hip_ops, tmp_path):
    fc.check_all_truncated_leaves_the_weights_alone(hip_ops, tmp_path)
