"""Reference-policy sync (GRPOConfig.sync_ref_model), CPU side: the fp32 composite of tests/ref_sync_cases.py against the fp64 mix, config validation, and the
trainer's step rule / metric / checkpoint order on the oracle op backend (RefOps), on one process and on two ranks over gloo.
tests/test_ref_sync_gpu.py runs the HIP kernel and the HIP trainer against the same composite."""
import os
import sys

import pytest
import torch

import ref_sync_cases as sc
from helpers import load_case, ref_ops_without
from oracle.ref_ops import RefOps
from time_r1_amd.trainer import GRPOConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------------ the composite
def test_composite_against_the_fp64_mix():
    """On every case: within one bf16 ulp everywhere, and RNE of the fp64 mix wherever that is further than 2^-20 relative from a bf16 tie.  The share of finite
    elements excluded by that margin, over all cases together, stays under 1 % (printed per n)."""
    total = excluded = 0
    for n in sc.NS:
        t_n = e_n = 0
        for wild in (False, True):
            r, p = sc.make_data(n, wild)
            for alpha in sc.ALPHAS:
                assert sc.data_cancellation(r, p, alpha) <= sc.MAX_CANCELLATION, (n, wild, alpha)
                got = sc.composite(r, p, alpha)
                m = sc.mix64(r, p, alpha)
                want, dist, ulp = sc.bf16_rne64(m)
                fin = torch.isfinite(m)
                assert bool(torch.equal(torch.isnan(got.float()), torch.isnan(m))), "a NaN reaches its own element and no other"
                assert bool(torch.isfinite(got.float()[fin]).all()), "the mix must not overflow where the true mix is finite"
                assert bool(((got.double() - m).abs()[fin] <= ulp[fin]).all()), (n, wild, alpha)
                clear = fin & (dist > sc.TIE_MARGIN)
                assert bool(torch.equal(sc.bits(got)[clear], sc.bits(want)[clear])), (n, wild, alpha, int((sc.bits(got)[clear] != sc.bits(want)[clear]).sum()))
                t_n += int(fin.sum())
                e_n += int((fin & ~clear).sum())
        print("n=%d: %d of %d finite elements within 2^-20 of a tie" % (n, e_n, t_n))
        total, excluded = total + t_n, excluded + e_n
    share = excluded / total
    print("all cases: %d of %d excluded (%.5f %%)" % (excluded, total, 100 * share))
    assert share < 0.01, share


def test_cases_tell_a_fused_multiply_add_from_the_three_roundings():
    """The kernel's contract is three separately rounded fp32 operations.  A compiler that contracts two of them into an fma changes few bf16 results, and none
    at all on data where the policy sits a few bf16 steps from its reference: the shared cases must hold elements on which the two differ, or the GPU's
    bit-for-bit check could not see a contraction."""
    n = sc.NS[-1]                       # about one element in 10^5 lands close enough to a tie: the large case carries this check
    for wild in (False, True):
        r, p = sc.make_data(n, wild)
        # alpha = 0.6 only: at 2^-9 both products are exact in fp32 (9 x 8 significant bits), so there the fused form IS the composite
        differ = int((sc.bits(sc.fused_variant(r, p, 0.6)) != sc.bits(sc.composite(r, p, 0.6))).sum())
        print("n=%d wild=%s: %d elements differ under contraction" % (n, wild, differ))
        assert differ >= 8, (n, wild, differ)


def test_rne64_helper_agrees_with_torch_on_fp32_representable_values():
    """The fp64 -> bf16 rounding the check above leans on, against torch's own cast where no double rounding can occur (values that are exact in fp32)."""
    g = torch.Generator().manual_seed(3)
    x = torch.cat([torch.randn(4096, generator=g) * torch.pow(2.0, torch.randint(-130, 120, (4096,), generator=g).float()),
                   torch.tensor([0.0, -0.0, 2.0 ** -133, 1.5 * 2.0 ** -133, 2.5 * 2.0 ** -133, 2.0 ** -126, 1.0, 1.00390625, 1.01171875, 3e38, 3.39e38, 3.4e38])])
    want = x.to(torch.bfloat16)
    got, _, _ = sc.bf16_rne64(x.double())
    assert bool(torch.equal(sc.bits(got), sc.bits(want)))


@pytest.mark.parametrize("n", sc.NS[:-1])
def test_alpha_zero_and_one_are_identities_up_to_the_sign_of_zero(n):
    for wild in (False, True):
        r, p = sc.make_data(n, wild)
        assert sc.identity_ok(sc.composite(r, p, 0.0), r, p)
        assert sc.identity_ok(sc.composite(r, p, 1.0), p, r)


# ------------------------------------------------------------------------------------------------------------------ configuration
def test_config_validation_and_defaults():
    c = GRPOConfig()
    assert (c.sync_ref_model, c.ref_model_mixup_alpha, c.ref_model_sync_steps) == (False, 0.6, 512)
    for bad in (dict(ref_model_mixup_alpha=0.0), dict(ref_model_mixup_alpha=-0.1), dict(ref_model_mixup_alpha=1.5), dict(ref_model_mixup_alpha=float("nan")),
                dict(ref_model_mixup_alpha="x"), dict(ref_model_sync_steps=0), dict(ref_model_sync_steps=-4), dict(ref_model_sync_steps=2.5),
                dict(ref_model_sync_steps=None), dict(sync_ref_model=True, beta=0.0), dict(sync_ref_model=True, num_iterations=2, ref_model_sync_steps=3)):
        with pytest.raises(ValueError):
            GRPOConfig(**bad)
    c = GRPOConfig(sync_ref_model=True, ref_model_mixup_alpha="1", ref_model_sync_steps=4.0, num_iterations=2)
    assert c.sync_ref_model is True and c.ref_model_mixup_alpha == 1.0 and c.ref_model_sync_steps == 4 and isinstance(c.ref_model_sync_steps, int)
    GRPOConfig(num_iterations=3)                   # the option is off: its default step count need not divide


def test_trainer_checks_again_at_train_and_names_a_backend_without_the_op(tmp_path):
    import ratio_cases as rc
    fx = load_case("clip_beta")
    with pytest.raises(NotImplementedError, match="ref_mixup"):
        rc.tiny_trainer(ref_ops_without("ref_mixup"), fx, tmp_path, mu=1, sync_ref_model=True, ref_model_sync_steps=2)
    rc.tiny_trainer(ref_ops_without("ref_mixup"), fx, tmp_path, mu=1)  # off: the backend is never asked
    tr = rc.tiny_trainer(RefOps(), fx, tmp_path, mu=2, sync_ref_model=True, ref_model_sync_steps=2)
    tr.args.ref_model_sync_steps = 3               # settings changed after construction are checked again when train() starts
    with pytest.raises(ValueError, match="ref_model_sync_steps"):
        tr.train()


def test_the_three_settings_parse_from_the_command_line(monkeypatch):
    sys.path.insert(0, ROOT)
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
    monkeypatch.setattr(sys, "argv", base + ["--sync_ref_model", "true", "--ref_model_mixup_alpha", "0.9", "--ref_model_sync_steps", "64"])
    with pytest.raises(Stop):
        train_grpo.main()
    a = seen["args"]
    assert (a.sync_ref_model, a.ref_model_mixup_alpha, a.ref_model_sync_steps) == (True, 0.9, 64)
    monkeypatch.setattr(sys, "argv", base)
    with pytest.raises(Stop):
        train_grpo.main()
    a = seen["args"]
    assert (a.sync_ref_model, a.ref_model_mixup_alpha, a.ref_model_sync_steps) == (False, 0.6, 512)


# ------------------------------------------------------------------------------------------------------------------ the trainer on the stand-in backend
def _trainer(tmp_path, name, mu=1, ga=1, n_rows=3, **over):
    import ratio_cases as rc
    over = {**dict(sync_ref_model=True, ref_model_sync_steps=2), **over}
    return rc.tiny_trainer(RefOps(), load_case("clip_beta"), tmp_path / name, mu=mu, ga=ga, n_rows=n_rows, **over)


def test_reference_moves_on_the_sync_step_only_and_by_the_composite(tmp_path):
    alpha = 0.6
    tr = _trainer(tmp_path, "a", ref_model_mixup_alpha=alpha)
    ref0 = tr.ref_model.w16.clone()
    v0 = tr.ref_model.version
    snaps = sc.run_with_snapshots(tr)
    assert [s["step"] for s in snaps] == [1, 2, 3]
    assert sc.same_bits(snaps[0]["ref"], ref0), "no sync on step 1"
    want = sc.composite(ref0, snaps[1]["pol"], alpha)
    assert not sc.same_bits(want, ref0)
    assert sc.same_bits(snaps[1]["ref"], want), "step 2: the composite of (old reference, the policy after the step)"
    assert sc.same_bits(snaps[2]["ref"], want), "no sync on step 3"
    assert tr.ref_model.version == v0 + 1, "one sync, one bump: derived copies of the old reference are stale"
    logs = tr.state.log_history
    assert ["ref_sync/weight_distance" in l for l in logs] == [False, True, False]
    d = sc.distance64(ref0, snaps[1]["pol"])
    assert d > 0 and abs(logs[1]["ref_sync/weight_distance"] - d) <= sc.TOL_SUMSQ_RTOL * d, (logs[1]["ref_sync/weight_distance"], d)
    assert not tr._ref_sync_sums


def test_alpha_one_makes_the_next_rollout_start_at_zero_kl(tmp_path):
    tr = _trainer(tmp_path, "a", n_rows=4, ref_model_mixup_alpha=1.0)
    snaps = sc.run_with_snapshots(tr)
    assert sc.identity_ok(snaps[1]["ref"], snaps[1]["pol"], snaps[0]["ref"])
    kl = [l["kl"] for l in tr.state.log_history]
    assert kl[0] > 0 and kl[1] > 0
    assert kl[2] == 0.0, kl            # step 3 draws and scores against a reference that IS the policy
    assert kl[3] > 0, kl               # step 4: the policy has moved by one update, the reference (synced again only after it) has not


def test_with_two_updates_per_rollout_the_sync_follows_the_replay(tmp_path):
    tr = _trainer(tmp_path, "a", mu=2, n_rows=2, ref_model_mixup_alpha=0.6)
    ref0 = tr.ref_model.w16.clone()
    calls = []
    orig = tr.ops.ref_mixup
    tr.ops.ref_mixup = lambda *a, **k: (calls.append(tr.state.global_step), orig(*a, **k))[1]
    snaps = sc.run_with_snapshots(tr)
    assert [s["step"] for s in snaps] == [1, 2, 3, 4] and calls == [2, 4], "once per rollout, after its last update"
    assert sc.same_bits(snaps[0]["ref"], ref0)
    assert sc.same_bits(snaps[1]["ref"], sc.composite(ref0, snaps[1]["pol"], 0.6))
    assert sc.same_bits(snaps[2]["ref"], snaps[1]["ref"])
    assert sc.same_bits(snaps[3]["ref"], sc.composite(snaps[1]["ref"], snaps[3]["pol"], 0.6))
    assert ["ref_sync/weight_distance" in l for l in tr.state.log_history] == [False, True, False, True]


def test_option_off_changes_no_metric_key_and_calls_nothing(tmp_path):
    tr_on = _trainer(tmp_path, "on")
    tr_off = _trainer(tmp_path, "off", sync_ref_model=False)
    called = []
    tr_off.ops.ref_mixup = lambda *a, **k: called.append(1)
    ref0 = tr_off.ref_model.w16.clone()
    sc.run_with_snapshots(tr_on)
    sc.run_with_snapshots(tr_off)
    assert not called and sc.same_bits(tr_off.ref_model.w16, ref0)
    on, off = tr_on.state.log_history, tr_off.state.log_history
    assert all("ref_sync/weight_distance" not in l for l in off)
    assert sc.metric_keys(on[0]) == sc.metric_keys(off[0]) == sc.metric_keys(off[1]) == sc.metric_keys(on[1]) - {"ref_sync/weight_distance"}


def test_checkpoint_on_a_sync_step_holds_the_mixed_reference_and_resumes_bit_for_bit(tmp_path):
    tr = _trainer(tmp_path, "a", n_rows=4, save_steps=2, ref_model_mixup_alpha=0.6)
    snaps = sc.run_with_snapshots(tr)
    saved = torch.load(tmp_path / "a" / "checkpoint-2" / "reference_policy.pt", weights_only=False)["ref_w16"]
    assert sc.same_bits(saved, snaps[1]["ref"]), "the sync runs before the step's checkpoint is written"
    tr2 = _trainer(tmp_path, "b", n_rows=4, ref_model_mixup_alpha=0.6)
    snaps2 = sc.run_with_snapshots(tr2, ckpt=str(tmp_path / "a" / "checkpoint-2"))
    assert [s["step"] for s in snaps2] == [3, 4]
    assert sc.same_bits(snaps2[0]["ref"], snaps[2]["ref"])
    a, b = tr.params.train.master, tr2.params.train.master
    assert torch.allclose(a, b, atol=2e-6, rtol=0), float((a - b).abs().max())
    # the reference after step 4's sync: the composite of the SAME old reference and each run's own policy
    assert sc.same_bits(snaps2[1]["ref"], sc.composite(snaps[2]["ref"], snaps2[1]["pol"], 0.6))


# ------------------------------------------------------------------------------------------------------------------ two ranks over gloo
def _worker(rank, world, port, q, shard, out):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    torch.set_num_threads(2)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import ratio_cases as rc
    import ref_sync_cases as sc
    from helpers import load_case
    tr = rc.tiny_trainer(RefOps(), load_case("clip_beta"), os.path.join(out, "r%d" % rank), mu=1, ga=1, n_rows=4, sync_ref_model=True, ref_model_sync_steps=2,
                         ref_model_mixup_alpha=0.6, shard_optimizer=shard)
    assert tr.dp.enabled and tr.dp.world == 2 and (tr.params.train.shard is not None) == shard
    ref0 = tr.ref_model.w16.clone()
    snaps = sc.run_with_snapshots(tr)              # 4 rows over 2 ranks: 2 optimizer steps, a sync after the second
    assert [s["step"] for s in snaps] == [1, 2]
    want = sc.composite(ref0, snaps[1]["pol"], 0.6)
    q.put((rank, snaps[1]["ref"].float().numpy().copy(), sc.same_bits(snaps[0]["ref"], ref0), sc.same_bits(snaps[1]["ref"], want),
           tr.state.log_history[1].get("ref_sync/weight_distance")))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("shard", [True, False])
def test_two_ranks_hold_the_same_reference_after_a_sync(tmp_path, shard):
    import socket
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q, shard, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=300) for _ in range(2)], key=lambda x: x[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert all(r[2] and r[3] for r in res), "unchanged after step 1, the composite of (old reference, whole policy) after step 2 - on both ranks"
    assert (res[0][1] == res[1][1]).all(), "no collective: identical inputs give identical references"
    assert res[0][4] is not None and res[0][4] == res[1][4] and res[0][4] > 0
