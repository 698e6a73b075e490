"""GPU: AdamW with bf16 moments and stochastic rounding (tr1_adamw_step_sr16, csrc/optim.hip; GRPOConfig.optimizer_state_dtype="bf16") against the fp32 emulation
of tests/optim_state_cases.py.  The stored moments are compared BIT FOR BIT on every element (the kernel's chain sumsq -> coef -> gg -> m', v' runs without fma
contraction, so the emulation is exact); p against the fp64 step from the bf16-valued moments inside optim_cases.adamw_bounds; p16 == bf16(p) bit for bit.

Cases: optim_cases.adamw_cases() with both moments first rounded to bf16, up to n = GRID_PASS + 3.  The kernel's grid is capped at SR16_GRID_CAP = 4096 blocks of
256 lanes x 8 elements = 2^23 elements a trip (pinned by test_optim_state_ref.py): GRID_PASS + 3 is one partial trip and a tail, and 3 * GRID_PASS + 1 would be
no more than that, so it is left out; one case of 2^23 + 6149 elements (a full trip, part of a second, a tail; its index_base crosses 2^32) covers the loop.
Every case carries its own index_base (multiples of 4 and not; above 2^32) and seed.  Every check prints what it saw (`pytest -s`,
lines starting with OBS)."""
import numpy as np
import pytest
import torch

import optim_cases as oc
import optim_state_cases as osc
from oracle.ref_ops import RefOps

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
DEV = "cuda:0"
CASES = osc.kernel_cases()
BY_NAME = {c["name"]: c for c in CASES}


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_sr16_step(hip_ops, case):
    out = osc.run_sr16(hip_ops, case, DEV)
    r = osc.check_sr16(out, case, DEV)
    print("OBS sr16 %-40s index_base %d: m16, v16 bit-equal on %d elements, p %.3f of the bound" % (case["name"], case["index_base"], case["n"], r))
    assert int((oc.bits32(out["g"]) != 0).sum()) == 0, "zero_grad=True leaves +0.0 everywhere"


@pytest.mark.parametrize("name", ["lr1e-6-wd0.01-step2-trained", "clip-gm0.125", "n1", "n3", "n5", "n7", "n8", "n9", "n1023", "offs123057", "offs301273", "offs000011",
                                  "offs333333-n%d" % (oc.GRID_PASS + 3)])
def test_sr16_step_keeps_the_gradient_and_reads_the_bf16_form(hip_ops, name):
    """zero_grad=False leaves g bit for bit in both gradient forms; the g16 form equals the fp32 form fed g16.float() bit for bit and only zeroes the accumulator."""
    case = BY_NAME[name]
    a = osc.run_sr16(hip_ops, case, DEV, zero_grad=False)
    assert torch.equal(oc.bits32(a["g"]), oc.bits32(a["g_before"])), "fp32 form, zero_grad=False: g changed"
    osc.check_sr16(a, case, DEV)
    b = osc.run_sr16(hip_ops, case, DEV, zero_grad=False, use_g16=True)
    assert torch.equal(oc.bits32(b["g"]), oc.bits32(b["g_before"])), "g16 form, zero_grad=False: the fp32 accumulator changed"
    rb = osc.check_sr16(b, case, DEV)
    p, m16, v16, g, ss = osc.bf16_state(case)
    c = osc.run_sr16(hip_ops, case, DEV, inputs=(p, m16, v16, g.to(BF16).float(), ss))
    d = osc.run_sr16(hip_ops, case, DEV, use_g16=True)
    osc.check_sr16(d, case, DEV)
    assert int((oc.bits32(d["g"]) != 0).sum()) == 0, "g16 form, zero_grad=True: the accumulator is zeroed"
    for k in ("p", "m16", "v16", "p16"):
        fn = oc.bits32 if c[k].dtype == F32 else oc.bits16
        assert torch.equal(fn(c[k]), fn(d[k])), "%s: g16 form != fp32 form fed the same values" % k
    print("OBS sr16 keep-gradient %-26s g16 form p %.3f of the bound" % (name, rb))


def test_sr16_rounding_patterns(hip_ops):
    osc.check_patterns(hip_ops, DEV)


def test_sr16_keying_and_split_calls(hip_ops):
    got = osc.check_keying(hip_ops, DEV)
    want = osc.check_keying(RefOps())
    assert torch.equal(got[1], want[1]) and torch.equal(got[2], want[2]), "the kernel's stored moments are the CPU stand-in's"


def test_sr16_decay_is_unbiased_and_equals_the_cpu_bits(hip_ops):
    v = osc.run_decay(hip_ops, DEV)
    mean, want = float(v.double().mean()), osc.decay_want()
    print("OBS sr16 v decay: mean %.6f, exact %.6f, |diff| %.2e (bound %.0e)" % (mean, want, abs(mean - want), osc.DECAY_BOUND))
    assert abs(mean - want) <= osc.DECAY_BOUND, (mean, want)
    assert torch.equal(oc.bits16(v), oc.bits16(osc.run_decay(RefOps()))), "the emulation is exact: the same bits as on the CPU"


def test_sr16_argument_checks_and_empty_call(hip_ops):
    from time_r1_amd.hip import HipError
    z = lambda n, dt=F32: torch.zeros(n, dtype=dt, device=DEV)
    hip_ops.adamw_step_sr16(z(0), z(0, BF16), z(0, BF16), z(0), z(0, BF16), 1e-3, oc.B1, oc.B2, oc.EPS, 0.0, 1, 0, 0)      # n == 0: a no-op
    with pytest.raises(HipError):
        hip_ops.adamw_step_sr16(z(8), z(8, BF16), z(8, BF16), z(8), z(8, BF16), 1e-3, oc.B1, oc.B2, oc.EPS, 0.0, 0, 0, 0)  # step counts from 1
    with pytest.raises(AssertionError):
        hip_ops.adamw_step_sr16(z(8), z(8), z(8), z(8), z(8, BF16), 1e-3, oc.B1, oc.B2, oc.EPS, 0.0, 1, 0, 0)              # fp32 moments


def test_dispatcher_op_equals_the_hipops_call(hip_ops):
    from time_r1_amd import torch_ops as T
    assert "adamw_step_sr16" in T.OP_NAMES
    assert "Tensor(a0!) p32" in str(torch.ops.timer1.adamw_step_sr16.default._schema)
    n, seed, base = 4103, 77, (1 << 32) + 6
    p, m, v, g = (t.to(DEV) for t in osc._state(n))
    a = [p.clone(), m.clone(), v.clone(), g.clone(), torch.zeros(n, dtype=BF16, device=DEV)]
    norm = torch.ops.timer1.adamw_step_sr16(*a, 1e-3, oc.B1, oc.B2, oc.EPS, 0.01, 5, 1.0, 0.5, seed, base)
    b = [p.clone(), m.clone(), v.clone(), g.clone(), torch.zeros(n, dtype=BF16, device=DEV)]
    ss = torch.zeros(1, dtype=F32, device=DEV)
    hip_ops.sumsq_accum(b[3], ss)
    hip_ops.adamw_step_sr16(*b, 1e-3, oc.B1, oc.B2, oc.EPS, 0.01, 5, seed, base, sumsq=ss, max_norm=1.0, grad_mult=0.5)
    for x, y in zip(a, b):
        fn = oc.bits32 if x.dtype == F32 else oc.bits16
        assert torch.equal(fn(x), fn(y))
    assert float(norm) == float(ss.sqrt() * 0.5) and not bool(a[3].any())
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        e = lambda dt: torch.empty(64, dtype=dt, device="cuda")
        fake = torch.ops.timer1.adamw_step_sr16(e(F32), e(BF16), e(BF16), e(F32), e(BF16), 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 1.0, 1.0, 0, 0)
        assert fake.shape == (1,) and fake.dtype == F32
    with pytest.raises(NotImplementedError):
        c = [t.cpu() for t in b]
        torch.ops.timer1.adamw_step_sr16(*c, 1e-3, oc.B1, oc.B2, oc.EPS, 0.01, 5, 1.0, 0.5, seed, base)


def test_adamw_flat_bf16_state_memory_and_resume(hip_ops):
    from time_r1_amd.optim import AdamWFlat

    def built_in_a_pool_of_its_own(make, state_dtype=None):
        """torch.cuda.memory_allocated counts whole blocks, and a cached free block is handed out unsplit when less than 1 MiB of it would be left over: what an
        object adds to the count depends on what the tests before this one left in the allocator.  Each object is therefore built inside a fresh private pool -
        the same empty allocator state for both - and the count is read around the construction."""
        pool = torch.cuda.MemPool()
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        with torch.cuda.use_mem_pool(pool):
            params = make()
            opt = AdamWFlat(params, hip_ops, lr=1e-3, weight_decay=0.01, state_dtype=state_dtype, seed=3)
        return params, opt, torch.cuda.memory_allocated() - before, pool
    p32, o32, used32, pool32 = built_in_a_pool_of_its_own(lambda: osc.tiny_params(hip_ops))                          # the parent-style object first
    n = p32.train.numel
    nb32 = p32.train.m.nbytes + p32.train.v.nbytes
    assert p32.train.m.dtype == F32 and not o32.sr16
    del o32, p32
    p16, o16, used16, pool16 = built_in_a_pool_of_its_own(lambda: osc.tiny_params(hip_ops, moment_dtype=BF16), BF16)
    assert o16.sr16
    a = p16.train
    assert a.m.dtype == BF16 and a.v.dtype == BF16 and a.m.element_size() == 2
    assert nb32 - (a.m.nbytes + a.v.nbytes) == 4 * n, "the tensors: 4 B per parameter less"
    assert used32 - used16 == 4 * n, "the allocator: %d against %d B, %d elements" % (used32, used16, n)      # (the arena's length is a multiple of 512 elements)
    print("OBS sr16 AdamWFlat on %d elements: %d B allocated with fp32 moments, %d B with bf16 moments" % (n, used32, used16))
    # a caller's fp32 arena is converted in place
    del o16
    pc = osc.tiny_params(hip_ops)
    oc_ = AdamWFlat(pc, hip_ops, state_dtype=BF16)
    assert pc.train.m.dtype == BF16 and pc.train.v.dtype == BF16 and pc.train.m.nbytes + pc.train.v.nbytes == 4 * n and pc.train.master.dtype == F32
    del oc_, pc
    # three steps straight = two steps, state_dict -> a fresh optimizer, the third: bit for bit (given gradients: no atomics anywhere)
    o16 = AdamWFlat(p16, hip_ops, lr=1e-3, weight_decay=0.01, seed=3)
    grads = [osc.exact_grad(n, k) for k in range(3)]
    osc.flat_steps(o16, grads, DEV)
    straight = osc.state_bits(a)
    cpu_p = osc.tiny_params(RefOps(act_dtype=BF16), moment_dtype=BF16)
    cpu_o = AdamWFlat(cpu_p, cpu_p.ops, lr=1e-3, weight_decay=0.01, seed=3)
    osc.flat_steps(cpu_o, grads)
    cpu = osc.state_bits(cpu_p.train)
    assert torch.equal(straight["m"], cpu["m"]) and torch.equal(straight["v"], cpu["v"]), "the moments of three optimizer steps are the CPU stand-in's"
    q = osc.tiny_params(hip_ops, moment_dtype=BF16)
    oq = AdamWFlat(q, hip_ops, lr=1e-3, weight_decay=0.01, seed=3)
    osc.flat_steps(oq, grads[:2], DEV)
    sd = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in oq.state_dict().items()}
    assert sd["m"].dtype == BF16 and sd["v"].dtype == BF16
    r = osc.tiny_params(hip_ops, moment_dtype=BF16)
    orr = AdamWFlat(r, hip_ops, lr=1e-3, weight_decay=0.01, seed=3)
    orr.load_state_dict({k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in sd.items()})
    osc.flat_steps(orr, grads, DEV, start=2)
    resumed = osc.state_bits(r.train)
    assert all(torch.equal(straight[k], resumed[k]) for k in straight)


def test_tiny_trainer_with_bf16_state(hip_ops, tmp_path):
    """One tiny run: finite loss, bf16 moments in the arena and in the checkpoint.  (No bit equality of a resumed GPU trainer run: the embedding gradient's atomics
    make that "equal up to ordering", and a stochastic rounding can turn one such ulp into one bf16 step of a moment.)"""
    import ratio_cases as rc
    from helpers import load_case
    tr = rc.tiny_trainer(hip_ops, load_case("clip_beta"), tmp_path / "a", mu=1, ga=1, n_rows=2, save_steps=2, optimizer_state_dtype="bf16")
    a = tr.params.train
    assert a.m.dtype == BF16 and a.v.dtype == BF16 and tr.optimizer.sr16
    tr.train()
    torch.cuda.synchronize()
    assert tr.state.global_step == 2 and all(np.isfinite(l["loss"]) for l in tr.state.log_history if "loss" in l)
    assert bool(torch.isfinite(a.master).all()) and bool(a.m.float().abs().max() > 0) and bool((a.v.float() >= 0).all())
    sd = torch.load(tmp_path / "a" / "checkpoint-2" / "optimizer_rank0.pt", weights_only=False)
    assert sd["m"].dtype == BF16 and sd["v"].dtype == BF16 and sd["master"].dtype == F32
