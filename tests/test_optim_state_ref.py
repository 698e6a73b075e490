"""AdamW with bf16 moments and stochastic rounding (GRPOConfig.optimizer_state_dtype="bf16"), CPU side: the emulation of tests/optim_state_cases.py (Philox
stream, rounding rule, keying, unbiasedness against nearest-even), AdamWFlat on the stand-in backend (spans, checkpoints, shards over gloo) and the trainer's
interface.  tests/test_optim_state_gpu.py runs the HIP kernel against the same emulation bit for bit."""
import os
import re
import sys

import numpy as np
import pytest
import torch

import optim_cases as oc
import optim_state_cases as osc
from helpers import load_case, ref_ops_without
from oracle.ref_ops import RefOps, philox4x32_10
from time_r1_amd.optim import AdamWFlat
from time_r1_amd.trainer import GRPOConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16, F32 = torch.bfloat16, torch.float32


# ------------------------------------------------------------------------------------------------------------------ stream and rule
def test_vectorised_philox_matches_the_oracle():
    cs = [(0, 0, 0, 0), (1, 2, 3, 4), (0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF), (0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (7, 1, 5, osc.STREAM)]
    for k0, k1 in ((0, 0), (0xA4093822, 0x299F31D0), (0xFFFFFFFF, 0xFFFFFFFF), (42, 0)):
        got = osc.philox4x32_10(*[np.array([c[i] for c in cs], dtype=np.uint64) for i in range(4)], k0, k1)
        for j, c in enumerate(cs):
            assert tuple(int(w[j]) for w in got) == philox4x32_10(*c, k0, k1), (c, k0, k1)
    # the keying: element e -> block e >> 2 (64-bit, split over two counter words), word e & 3
    seed, step = (0x1234 << 32) | 0x9ABCDEF0, 77
    for e in (0, 1, 5, 1023, (1 << 32) + 6, (1 << 34) + 3, (1 << 40) + 1):
        want = philox4x32_10((e >> 2) & 0xFFFFFFFF, (e >> 2) >> 32, step, osc.STREAM, seed & 0xFFFFFFFF, seed >> 32)[e & 3]
        assert int(osc.random_words(1, seed, step, e)[0]) == want, e
        assert int(osc.random_words(9, seed, step, e - min(e, 3))[min(e, 3)]) == want, e


def test_kernel_source_pins_the_grid_cap_and_the_stream_word():
    src = open(os.path.join(ROOT, "time-r1_amd", "csrc", "optim.hip")).read()
    assert re.search(r"#define SR16_GRID_CAP %d\b" % osc.SR16_GRID_CAP, src) and re.search(r"#define SR16_STREAM 0x%Xu" % osc.STREAM, src)
    body, _ = oc.launcher_source("tr1_adamw_step_sr16", os.path.join(ROOT, "time-r1_amd", "csrc", "optim.hip"))
    assert "tr1_grid_1d(n / 8 + 1, 256, SR16_GRID_CAP)" in body
    assert osc.SR16_PASS < osc.TWO_TRIPS_N == max(c["n"] for c in osc.kernel_cases()), "the largest case must take more than one grid trip"


def test_rounding_patterns_through_an_exact_step():
    osc.check_patterns(RefOps())


def test_unbiased_where_nearest_even_freezes():
    v = osc.run_decay(RefOps())
    mean, want = float(v.double().mean()), osc.decay_want()
    print("OBS v decay: mean %.6f, exact %.6f, |diff| %.2e (bound %.0e)" % (mean, want, abs(mean - want), osc.DECAY_BOUND))
    assert abs(want - 0.904793) < 1e-6
    assert abs(mean - want) <= osc.DECAY_BOUND, (mean, want)
    frozen = osc.run_decay(osc.RneOps())
    assert bool((frozen.float() == 1.0).all()), "nearest even: 0.999 is nearer to 1.0 than to the bf16 value below it, v never moves"


# ------------------------------------------------------------------------------------------------------------------ keying
def test_keying_by_seed_step_and_global_index():
    osc.check_keying(RefOps())


def test_masters_follow_the_fp32_path_on_the_first_step(ref_ops):
    n = 4103
    p, _, _, g = osc._state(n)
    ss = (g.double() ** 2).sum().to(F32).reshape(1)
    a = [p.clone(), torch.zeros(n), torch.zeros(n), g.clone(), torch.zeros(n, dtype=BF16)]
    ref_ops.adamw_step(*a, 1e-3, oc.B1, oc.B2, oc.EPS, 0.01, 1, sumsq=ss, max_norm=1.0, grad_mult=0.5)
    b = [p.clone(), torch.zeros(n, dtype=BF16), torch.zeros(n, dtype=BF16), g.clone(), torch.zeros(n, dtype=BF16)]
    RefOps().adamw_step_sr16(*b, 1e-3, oc.B1, oc.B2, oc.EPS, 0.01, 1, 9, 0, sumsq=ss, max_norm=1.0, grad_mult=0.5)
    assert torch.equal(oc.bits32(a[0]), oc.bits32(b[0])) and torch.equal(oc.bits16(a[4]), oc.bits16(b[4]))
    assert float((b[1].float() - a[1]).abs().max()) <= float(a[1].abs().max()) * 2.0 ** -7 and bool((b[2].float() >= 0).all())


def test_oracle_step_on_the_shared_cases_holds_the_bounds():
    """The stand-in on the small shared cases: stored moments = the emulation (by construction), p inside the fp32-state kernel's bounds."""
    for case in osc.kernel_cases():
        if case["n"] > 200000:
            continue
        for use_g16 in (False, True):
            out = osc.run_sr16(RefOps(), case, use_g16=use_g16)
            osc.check_sr16(out, case, limit=oc.ORACLE_SHARE)
            assert bool((out["g"] == 0).all())


# ------------------------------------------------------------------------------------------------------------------ AdamWFlat
def _flat(ops, state_dtype, lazy=False, moment_dtype=F32, seed=3, **kw):
    params = osc.tiny_params(ops, moment_dtype=moment_dtype)
    opt = AdamWFlat(params, ops, lr=1e-3, weight_decay=0.01, state_dtype=state_dtype, seed=seed, **kw)
    if lazy:
        from time_r1_amd.model import Engine
        opt.lazy_zero = Engine(params.cfg, ops, params).lazy_zero_plan()
        assert opt.lazy_zero and len(opt._zero_spans(params.train.numel)[0]) == 3
    return params, opt


def test_adamw_flat_dtypes_spans_and_resume():
    ops = RefOps()
    params, opt = _flat(ops, BF16)
    a = params.train
    assert a.m.dtype == BF16 and a.v.dtype == BF16 and a.master.dtype == F32 and a.m.element_size() == 2 and a.moment_dtype == BF16 and opt.sr16
    grads = [osc.exact_grad(a.numel, k) for k in range(3)]
    osc.flat_steps(opt, grads)
    straight = osc.state_bits(a)
    assert bool((a.grad == 0).all()) and bool(a.m.float().abs().max() > 0)
    # the lazy-zero span form (three launches, index_base = each span's start) equals the single-span form
    p2, o2 = _flat(ops, None, lazy=True, moment_dtype=BF16)
    assert o2.sr16, "state_dtype=None keeps what the arena has"
    osc.flat_steps(o2, grads)
    lz = osc.state_bits(p2.train)
    assert all(torch.equal(straight[k], lz[k]) for k in straight)
    # state_dict at step 2 -> a fresh optimizer -> the third step: bit for bit
    p3, o3 = _flat(ops, BF16)
    osc.flat_steps(o3, grads[:2])
    sd = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in o3.state_dict().items()}
    assert sd["m"].dtype == BF16 and sd["v"].dtype == BF16 and sd["master"].dtype == F32
    p4, o4 = _flat(ops, BF16)
    o4.load_state_dict(sd)
    osc.flat_steps(o4, grads, start=2)
    resumed = osc.state_bits(p4.train)
    assert all(torch.equal(straight[k], resumed[k]) for k in straight)
    # another seed is another stream
    p5, o5 = _flat(ops, BF16, seed=4)
    osc.flat_steps(o5, grads)
    assert not torch.equal(osc.state_bits(p5.train)["m"], straight["m"])
    # cross-dtype loads: fp32 -> bf16 rounds to nearest even once, bf16 -> fp32 is exact
    p6, o6 = _flat(ops, F32)
    assert not o6.sr16 and p6.train.m.dtype == F32
    osc.flat_steps(o6, grads[:2])
    sd32 = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in o6.state_dict().items()}
    assert sd32["m"].dtype == F32
    p7, o7 = _flat(ops, BF16)
    o7.load_state_dict(sd32)
    assert torch.equal(oc.bits16(p7.train.m), oc.bits16(sd32["m"].to(BF16))) and torch.equal(oc.bits16(p7.train.v), oc.bits16(sd32["v"].to(BF16)))
    assert torch.equal(p7.train.master, sd32["master"]) and o7.step_count == 2
    p8, o8 = _flat(ops, F32)
    o8.load_state_dict(sd)
    assert p8.train.m.dtype == F32 and torch.equal(p8.train.m, sd["m"].float()) and torch.equal(p8.train.v, sd["v"].float())


def test_set_moment_dtype_converts_in_place_and_set_shard_keeps_it():
    ops = RefOps()
    params = osc.tiny_params(ops)
    a = params.train
    a.set_moment_dtype(F32)
    m0 = a.m
    a.set_moment_dtype(F32)
    assert a.m is m0, "matching dtype: nothing happens"
    a.m.copy_(torch.randn(a.numel, generator=torch.Generator().manual_seed(1)) * 1e-3)
    want = a.m.to(BF16)
    a.set_moment_dtype(BF16)
    assert a.m.dtype == BF16 and torch.equal(oc.bits16(a.m), oc.bits16(want)) and a.v.dtype == BF16 and not bool(a.v.any())
    a.set_moment_dtype(F32)
    assert a.m.dtype == F32 and torch.equal(a.m, want.float())
    # a weights-only arena sharded by the optimizer gets fresh moments of the arena's dtype; relayout passes it on
    from time_r1_amd.params import ModelParams
    q = ModelParams(params.cfg, ops, optimizer_state=False, moment_dtype=BF16)
    q.train.set_shard(1, 2)
    assert q.train.m.dtype == BF16 and q.train.m.numel() == q.train.numel // 2 and q.train.master.dtype == F32
    r = osc.tiny_params(ops, moment_dtype=BF16).relayout(True)
    assert r.train_vit and r.train.m.dtype == BF16 and r.train.moment_dtype == BF16


def _worker(rank, world, port, q, shard, wire):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    torch.set_num_threads(2)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import optim_state_cases as osc
    from time_r1_amd.dist import DataParallel
    from time_r1_amd.optim import AdamWFlat
    ops = RefOps()
    params = osc.tiny_params(ops)
    opt = AdamWFlat(params, ops, lr=1e-3, weight_decay=0.01, dp=DataParallel(), shard_optimizer=shard, state_dtype=torch.bfloat16, seed=3,
                    grad_wire_dtype=torch.bfloat16 if wire == "bf16" else torch.float32)
    a = params.train
    assert opt.sharded == shard and a.m.dtype == torch.bfloat16 and a.m.numel() == (a.numel // world if shard else a.numel)
    # every rank holds the same gradient: the sum over ranks is world x g, exactly, on either wire (small integers / 64)
    osc.flat_steps(opt, [osc.exact_grad(a.numel, k, world) for k in range(3)])
    q.put((rank, a.chunks(rank, world), {k: v.numpy().copy() for k, v in osc.state_bits(a).items()}))
    dist.barrier()
    dist.destroy_process_group()


def _spawn(world, shard, wire):
    import socket
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, shard, wire)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=300) for _ in range(world)], key=lambda x: x[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return res


@pytest.mark.parametrize("world,wire", [(2, "bf16"), (4, "fp32")])
def test_sharded_optimizer_equals_the_replicated_one_bit_for_bit(world, wire):
    sharded, plain = _spawn(world, True, wire), _spawn(world, False, wire)
    full = plain[0][2]
    for r in range(world):
        assert all((plain[r][2][k] == full[k]).all() for k in full), "the replicated ranks agree: the seed is the same on every rank"
        assert (sharded[r][2]["w16"] == full["w16"]).all(), "rank %d: the gathered working weights" % r
        for ca, cb, la in sharded[r][1]:
            for k in ("master", "m", "v"):
                assert (sharded[r][2][k][la:la + cb - ca] == full[k][ca:cb]).all(), "rank %d chunk [%d, %d): %s" % (r, ca, cb, k)
    assert full["m"].any() and full["v"].any()


# ------------------------------------------------------------------------------------------------------------------ interface
def test_config_values_and_command_line(monkeypatch):
    assert GRPOConfig().optimizer_state_dtype == "fp32" and GRPOConfig(optimizer_state_dtype="bf16").optimizer_state_dtype == "bf16"
    for bad in ("fp16", "bfloat16", None, 16, ""):
        with pytest.raises(ValueError, match="optimizer_state_dtype"):
            GRPOConfig(optimizer_state_dtype=bad)
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
    for extra, want in (([], "fp32"), (["--optimizer_state_dtype", "bf16"], "bf16")):
        monkeypatch.setattr(sys, "argv", base + extra)
        with pytest.raises(Stop):
            train_grpo.main()
        assert seen["args"].optimizer_state_dtype == want
    monkeypatch.setattr(sys, "argv", base + ["--optimizer_state_dtype", "fp8"])
    with pytest.raises(ValueError, match="optimizer_state_dtype"):
        train_grpo.main()


def test_backend_without_the_op_is_refused_and_the_default_never_asks(tmp_path):
    import ratio_cases as rc
    fx = load_case("clip_beta")
    with pytest.raises(NotImplementedError, match="adamw_step_sr16"):
        AdamWFlat(osc.tiny_params(RefOps()), ref_ops_without("adamw_step_sr16"), state_dtype=BF16)
    with pytest.raises(NotImplementedError, match="adamw_step_sr16"):
        rc.tiny_trainer(ref_ops_without("adamw_step_sr16"), fx, tmp_path / "x", mu=1, optimizer_state_dtype="bf16")
    # the default: only adamw_step, with fp32 moments
    ops = RefOps()
    calls = []
    orig = ops.adamw_step
    ops.adamw_step = lambda p32, m, v, *a, **k: (calls.append((m.dtype, v.dtype)), orig(p32, m, v, *a, **k))[1]
    ops.adamw_step_sr16 = lambda *a, **k: calls.append("sr16")
    tr = rc.tiny_trainer(ops, fx, tmp_path / "d", mu=1, ga=1, n_rows=2)
    assert tr.params.train.m.dtype == F32 and not tr.optimizer.sr16
    tr.train()
    assert calls and all(c == (F32, F32) for c in calls), calls


def test_trainer_with_bf16_state_trains_saves_and_resumes_exactly(tmp_path):
    import ratio_cases as rc
    fx = load_case("clip_beta")
    tr = rc.tiny_trainer(RefOps(), fx, tmp_path / "a", mu=1, ga=1, n_rows=4, save_steps=2, optimizer_state_dtype="bf16")
    a = tr.params.train
    assert a.m.dtype == BF16 and a.v.dtype == BF16 and tr.optimizer.sr16 and tr.optimizer.seed == tr.args.seed, "a caller's ModelParams is converted in place"
    tr.train()
    assert tr.state.global_step == 4 and all(np.isfinite(l["loss"]) for l in tr.state.log_history if "loss" in l)
    sd = torch.load(tmp_path / "a" / "checkpoint-2" / "optimizer_rank0.pt", weights_only=False)
    assert sd["m"].dtype == BF16 and sd["v"].dtype == BF16 and sd["master"].dtype == F32 and bool(sd["m"].float().abs().max() > 0)
    tr2 = rc.tiny_trainer(RefOps(), fx, tmp_path / "b", mu=1, ga=1, n_rows=4, optimizer_state_dtype="bf16")
    tr2.train(resume_from_checkpoint=str(tmp_path / "a" / "checkpoint-2"))
    assert tr2.state.global_step == 4
    b = tr2.params.train
    assert torch.equal(oc.bits32(a.master), oc.bits32(b.master)) and torch.equal(oc.bits16(a.m), oc.bits16(b.m)) and torch.equal(oc.bits16(a.v), oc.bits16(b.v))
    assert torch.equal(a.w16, b.w16)
    # a preset name: the trainer builds the arena itself, with bf16 moments from the start
    from oracle.text import FakeProcessor
    from time_r1_amd.config import tiny_test
    from time_r1_amd.trainer import TimeR1_Trainer
    tr3 = TimeR1_Trainer(tiny_test(), [rc.varied_reward], [], args=GRPOConfig(output_dir=str(tmp_path / "c"), optimizer_state_dtype="bf16"),
                         processing_class=FakeProcessor(tiny_test()), ops=RefOps())
    assert tr3.params.train.m.dtype == BF16 and tr3.params.train.moment_dtype == BF16
