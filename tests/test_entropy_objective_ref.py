"""The entropy options of the GRPO objective (GRPOConfig.entropy_coef, GRPOConfig.top_entropy_quantile), CPU side: the fp64 references of
tests/entropy_cases.py against autograd and against their fp32 stand-ins, config validation, the command line, the dispatcher registration, and the trainer on
the oracle op backend (RefOps).  tests/test_entropy_objective_gpu.py runs the HIP kernels and the HIP trainer against the same references."""
import pytest
import torch

import entropy_cases as ec
import vocab_cases as vc
from helpers import ref_ops_without
from oracle.ref_ops import RefOps
from time_r1_amd.trainer import GRPOConfig


# ------------------------------------------------------------------------------------------------------------ references
def test_reference_formula_is_the_autograd_gradient():
    """d (sum dlogp logp + sum dent H) / d logits by fp64 autograd of log_softmax == the closed form the kernel implements."""
    R, V = 37, 2048
    _, x, tg, _ = vc.stat_rows(R=R, V=V, seed=3)
    dlogp, dent = vc.bwd_dlogp(R, 3), ec.bwd_dent(R, 3)
    xx = x.double().clone().requires_grad_(True)
    ls = torch.log_softmax(xx, -1)
    lp = ls.gather(1, tg.long()[:, None])[:, 0]
    H = -(ls.exp() * ls).sum(-1)
    (lp * dlogp.double() + H * dent.double()).sum().backward()
    ref = ec.ref_dlogits_ent(x, tg, dlogp, dent)
    assert float((xx.grad - ref).abs().max()) < 1e-13
    pairs = {(bool(a == 0), bool(b == 0)) for a, b in zip(dlogp.tolist(), dent.tolist())}
    assert pairs == {(False, False), (True, False), (False, True), (True, True)}, "the four zero / non-zero pairs occur at R = 37"


@pytest.mark.parametrize("name,kw", [c for c in vc.bwd_cases() if c[1]["V"] <= 5008], ids=[c[0] for c in vc.bwd_cases() if c[1]["V"] <= 5008])
def test_fp32_standin_dlogits(name, kw):
    """RefOps.logp_entropy_bwd (fp32 arithmetic, one rounding to bf16) within TOL_DLOGITS of the fp64 reference; a null dent is logp_bwd."""
    ops = RefOps()
    _, x, tg, _ = vc.stat_rows(**kw)
    R = kw["R"]
    dlogp, dent = vc.bwd_dlogp(R, kw["seed"]), ec.bwd_dent(R, kw["seed"])
    stats = vc.ref_stats(x, tg)
    ref = ec.ref_dlogits_ent(x, tg, dlogp, dent, stats)
    got = ops.logp_entropy_bwd(x.contiguous(), tg, stats[2].float(), stats[1].float(), dlogp, dent, inplace=False)
    share = vc.worst(got, ref, vc.TOL_DLOGITS)[0]
    print("%s: %.3f of TOL_DLOGITS" % (name, share))
    assert share <= 1.0
    a = ops.logp_entropy_bwd(x.contiguous(), tg, stats[2].float(), stats[1].float(), dlogp, None, inplace=False)
    b = ops.logp_bwd(x.contiguous(), tg, stats[2].float(), dlogp, inplace=False)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))


@pytest.mark.parametrize("G,C", ec.QUANTILE_SHAPES)
def test_fp32_standin_selection(G, C):
    """RefOps.entropy_quantile_weight (fp32 torch.quantile) against the fp64 reference on every mask, both entropy sets, every rho."""
    ops = RefOps()
    left = 0
    for mname, mask in ec.quantile_masks(G, C).items():
        for kind in ("uniform", "zeros"):
            ent = ec.quantile_entropies(mask, kind)
            for rho in ec.RHOS:
                w, st = ops.entropy_quantile_weight(ent, mask, rho)
                left += ec.compare_quantile(w, st, ent, mask, rho, (G, C, mname, kind, rho))
    print("G=%d C=%d: %d tokens near a threshold left out" % (G, C, left))


def test_reference_selection_by_hand():
    ent = torch.tensor([[0.5, 3.0, float("nan"), 1.0], [2.0, float("nan"), 2.0, 0.0]])
    mask = torch.tensor([[1, 1, 0, 1], [1, 0, 1, 1]], dtype=torch.int32)
    # live, sorted: 0, 0.5, 1, 2, 2, 3; q = 0.5 -> pos 2.5 -> thr 1.5; q = 0.6 -> pos 3 -> thr 2 (both 2.0 tie with it and stay)
    w, thr, kept, n = ec.ref_quantile_weight(ent, mask, 0.5)
    assert (thr, kept, n) == (1.5, 3, 6) and w.tolist() == [[0, 1, 0, 0], [1, 0, 1, 0]]
    w, thr, kept, n = ec.ref_quantile_weight(ent, mask, 0.4)
    assert abs(thr - 2.0) < 1e-12 and kept == 3
    w, thr, kept, n = ec.ref_quantile_weight(ent, mask, 1.0)
    assert thr == 0.0 and kept == 6 and torch.equal(w, mask.float())
    assert ec.ref_quantile_weight(ent, torch.zeros_like(mask), 0.5)[1:] == (0.0, 0, 0)
    one = torch.zeros_like(mask)
    one[1, 3] = 1
    assert ec.ref_quantile_weight(ent, one, 0.2)[0].tolist() == [[0, 0, 0, 0], [0, 0, 0, 1]]


# ------------------------------------------------------------------------------------------------------------ configuration
def test_config_validation():
    for kw in (dict(entropy_coef=float("nan")), dict(entropy_coef=float("inf")), dict(entropy_coef="much"), dict(top_entropy_quantile=0.0),
               dict(top_entropy_quantile=-0.2), dict(top_entropy_quantile=1.5), dict(top_entropy_quantile=float("nan"))):
        with pytest.raises(ValueError):
            GRPOConfig(**kw)
    c = GRPOConfig()
    assert c.entropy_coef == 0.0 and c.top_entropy_quantile == 1.0
    c = GRPOConfig(entropy_coef="-0.01", top_entropy_quantile=None)
    assert c.entropy_coef == -0.01 and c.top_entropy_quantile == 1.0
    # both combine with every objective setting
    GRPOConfig(use_grpo=True, entropy_coef=0.01, top_entropy_quantile=0.2)
    GRPOConfig(loss_type="dr_grpo", importance_sampling_level="sequence", delta=1.5, num_iterations=2, mask_truncated_completions=True,
               entropy_coef=0.001, top_entropy_quantile=0.5)


def test_both_settings_parse_from_the_command_line(monkeypatch):
    import os
    import sys
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
    base = ["train_grpo.py", "--model_name_or_path", "m", "--train_data_path", "d"]
    monkeypatch.setattr(sys, "argv", base + ["--entropy_coef", "0.001", "--top_entropy_quantile", "0.2"])
    with pytest.raises(Stop):
        train_grpo.main()
    assert (seen["args"].entropy_coef, seen["args"].top_entropy_quantile) == (0.001, 0.2)
    monkeypatch.setattr(sys, "argv", base)
    with pytest.raises(Stop):
        train_grpo.main()
    assert (seen["args"].entropy_coef, seen["args"].top_entropy_quantile) == (0.0, 1.0)
    monkeypatch.setattr(sys, "argv", base + ["--top_entropy_quantile", "0"])
    with pytest.raises(ValueError, match="top_entropy_quantile"):
        train_grpo.main()


def test_torch_ops_are_registered_with_fake_kernels_and_no_cpu_fallback():
    import time_r1_amd.torch_ops as T
    from torch._subclasses.fake_tensor import FakeTensorMode
    for n in ("logp_entropy_bwd", "entropy_quantile_weight"):
        assert n in T.OP_NAMES
        assert str(getattr(torch.ops.timer1, n).default._schema).startswith("timer1::" + n)
    with FakeTensorMode():
        lg = torch.empty(37, 2048, dtype=torch.bfloat16, device="cuda")
        r = torch.empty(37, device="cuda")
        tg = torch.empty(37, dtype=torch.int32, device="cuda")
        assert torch.ops.timer1.logp_entropy_bwd(lg, tg, r, r, r, r).shape == (37, 2048)
        e = torch.empty(8, 200, device="cuda")
        w, st = T.entropy_quantile_weight(e, torch.empty(8, 200, dtype=torch.int32, device="cuda"), 0.2)
        assert w.shape == (8, 200) and w.dtype == torch.float32 and st.shape == (3,)
    with pytest.raises(NotImplementedError):
        T.entropy_quantile_weight(torch.zeros(2, 3), torch.ones(2, 3, dtype=torch.int32), 0.5)


def test_header_states_the_two_entry_points():
    from time_r1_amd import hip
    decls = hip.parse_header()
    assert [t for t, _ in decls["tr1_logp_entropy_bwd"][1]] == ["const void*", "int64_t", "const void*", "const void*", "const void*", "const void*", "const void*",
                                                              "void*", "int64_t", "int64_t", "int64_t", "void*"]
    assert [t for t, _ in decls["tr1_entropy_quantile_weight"][1]] == ["const void*", "const void*", "void*", "void*", "int64_t", "float", "void*"]
    txt = open(hip.HEADER).read()
    assert "timer1_trainer.py:473-481" in txt and "entropy_coeff" in txt and "top_entropy_quantile" in txt


# ------------------------------------------------------------------------------------------------------------ trainer (oracle backend)
def test_defaults_are_the_parent_run_and_need_neither_op(tmp_path):
    ec.check_defaults_are_the_parent_run(RefOps(), tmp_path, plain_ops=ref_ops_without("logp_entropy_bwd", "entropy_quantile_weight"))


def test_a_backend_without_the_ops_refuses_the_options(tmp_path):
    from helpers import load_case
    import ratio_cases as rc
    for over in (dict(entropy_coef=0.01), dict(top_entropy_quantile=0.5)):
        with pytest.raises(NotImplementedError, match="ref"):
            rc.tiny_trainer(ref_ops_without("logp_entropy_bwd", "entropy_quantile_weight"), load_case("clip_beta"), tmp_path, mu=1, **over)


def test_entropy_bonus_in_the_logged_loss(tmp_path):
    ec.check_entropy_bonus_in_the_logged_loss(RefOps(), tmp_path)


def test_top_entropy_quantile_changes_the_step(tmp_path):
    ec.check_top_entropy_quantile_changes_the_step(RefOps(), tmp_path)


def test_two_iterations_with_both_options(tmp_path):
    ec.check_two_iterations_with_both_options(RefOps(), tmp_path)


def test_all_truncated_completions_leave_the_weights_bit_unchanged(tmp_path):
    ec.check_all_truncated_leaves_the_weights_alone(RefOps(), tmp_path)


def test_selection_and_bonus_reach_the_loss_calls(tmp_path):
    """What GRPOCore hands on: the selection multiplies into tok_weight on the loss call, the bonus's dent reaches head_bwd with the path's normaliser, zero at
    masked positions, and the bonus covers every live token (not only the selected ones)."""
    from helpers import load_case
    import ratio_cases as rc
    ops = RefOps()
    seen = dict(tw=[], dent=[])
    tr = rc.tiny_trainer(ops, load_case("clip_beta"), tmp_path, mu=1, ga=1, n_rows=1, loss_type="dr_grpo", entropy_coef=0.5, top_entropy_quantile=0.5)
    o_loss, o_head = ops.grpo_policy_loss, tr.engine.head_bwd
    ops.grpo_policy_loss = lambda *a, **k: (seen["tw"].append((k["tok_weight"].clone(), a[3].clone())), o_loss(*a, **k))[1]
    tr.engine.head_bwd = lambda ctx, dlogp, n_dup, dent=None: (seen["dent"].append(dent.clone()), o_head(ctx, dlogp, n_dup, dent=dent))[1]
    rc.run_recorded(tr)
    (tw, mask), dent = seen["tw"][0], seen["dent"][0]
    G, C = mask.shape
    live = mask != 0
    assert bool(((tw == 0) | (tw == 1)).all()) and 0 < int(tw.sum()) < int(live.sum()) and bool((tw[~live] == 0).all())
    assert abs(int(tw.sum()) - 0.5 * int(live.sum())) <= 1
    assert dent.shape == (G * C,) and int((dent != 0).sum()) == int(live.sum())
    assert torch.allclose(dent[dent != 0], torch.full((int(live.sum()),), -0.5 / (G * C)), rtol=1e-6, atol=0)      # norm 2: 1 / (G C), grad_scale 1 / GA = 1
