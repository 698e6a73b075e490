"""Reference-policy sync on the MI355X: tr1_ref_mixup against the fp32 composite of tests/ref_sync_cases.py bit for bit (sentinels, the two sums, determinism,
the alpha = 0 / 1 identities), the torch op, and the HIP trainer: a sync with alpha = 1 must make the next rollout's KL exactly 0 (a stale copy derived from the
old reference weights would not), and a checkpoint written on a sync step must resume into the same reference."""
import pytest
import torch

import ratio_cases as rc
import ref_sync_cases as sc
from helpers import load_case

pytestmark = pytest.mark.gpu


def _run(ops, r, p, off, alpha):
    rb, pb, rv, pv = sc.framed(r, p, off, ops.device)
    sums = ops.ref_mixup(rv, pv, alpha)
    assert sums.shape == (2,) and sums.dtype == torch.float32
    assert sc.frames_intact(rb, pb, p, off), "sentinels on both sides of both arrays, and the policy itself, keep their bits"
    return rv.cpu(), sums.cpu()


@pytest.mark.parametrize("n", sc.NS)
def test_kernel_is_the_composite_bit_for_bit(hip_ops, n):
    """n: empty, one element, tails of 7 / 1 behind zero or one vector, 1023, 65537 (several blocks + a tail of 1), one pass of the capped grid + 3 (every
    thread takes a second trip or not, tail of 3).  Tame and wild data, both view offsets, every alpha."""
    for wild in (False, True):
        r, p = sc.make_data(n, wild)
        for off in sc.OFFS:
            for alpha in sc.ALPHAS:
                got, _ = _run(hip_ops, r, p, off, alpha)
                assert sc.same_bits(got, sc.composite(r, p, alpha)), (n, wild, off, alpha)


@pytest.mark.parametrize("n", sc.NS)
def test_sums_against_fp64_and_across_two_calls(hip_ops, n):
    r, p = sc.make_data(n, wild=False)
    want = sc.sums64(r, p)
    outs = [_run(hip_ops, r, p, off, 0.6) for off in (0, 0, 64)]
    for mixed, s in outs:
        assert torch.isfinite(s).all()
        assert bool(((s.double() - want).abs() <= sc.TOL_SUMSQ_RTOL * want).all()), (n, s, want)
        assert bool(torch.equal(sc.bits(s), sc.bits(outs[0][1]))), "the same inputs give the same two numbers (no float atomics)"
        assert sc.same_bits(mixed, outs[0][0])
    if n == 0:
        assert outs[0][1].tolist() == [0.0, 0.0]


def test_sums_of_unsummable_data_say_so(hip_ops):
    """The squares of +-3e38 overflow fp32 and a NaN is a NaN: neither sum may come back finite."""
    r, p = sc.make_data(1023, wild=True)
    _, s = _run(hip_ops, r, p, 0, 0.6)
    assert not torch.isfinite(s).any(), s


@pytest.mark.parametrize("n", sc.NS[1:])
def test_alpha_zero_and_one_are_identities(hip_ops, n):
    for wild in (False, True):
        r, p = sc.make_data(n, wild)
        got0, _ = _run(hip_ops, r, p, 0, 0.0)
        got1, _ = _run(hip_ops, r, p, 64, 1.0)
        assert sc.identity_ok(got0, r, p) and sc.identity_ok(got1, p, r)


def test_bad_arguments_are_errors(hip_ops):
    from time_r1_amd.hip import HipError
    r, p = [t.to(hip_ops.device) for t in sc.make_data(1023, False)]
    for alpha in (-0.01, 1.01, float("nan")):
        with pytest.raises(HipError, match="alpha"):
            hip_ops.ref_mixup(r.clone(), p, alpha)
    with pytest.raises(HipError, match="aligned"):
        hip_ops.ref_mixup(r.clone()[1:], p[1:], 0.5)
    with pytest.raises(HipError, match="aliased"):
        hip_ops.ref_mixup(r, r, 0.5)


def test_torch_op_fake_and_real_shapes_agree(hip_ops):
    import time_r1_amd.torch_ops as T
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert "ref_mixup" in T.OP_NAMES
    assert "Tensor(a0!) ref" in str(torch.ops.timer1.ref_mixup.default._schema)
    r, p = sc.make_data(1023, False)
    rd, pd = r.to(hip_ops.device), p.to(hip_ops.device)
    real = torch.ops.timer1.ref_mixup(rd, pd, 0.6)
    assert sc.same_bits(rd, sc.composite(r, p, 0.6))
    with FakeTensorMode():
        fake = torch.ops.timer1.ref_mixup(torch.empty(1023, dtype=torch.bfloat16, device="cuda"), torch.empty(1023, dtype=torch.bfloat16, device="cuda"), 0.6)
    assert fake.shape == real.shape and fake.dtype == real.dtype
    with pytest.raises(NotImplementedError):
        torch.ops.timer1.ref_mixup(r.clone(), p, 0.6)


def _trainer(ops, out, **over):
    over = {**dict(sync_ref_model=True, ref_model_sync_steps=2, ref_model_mixup_alpha=1.0), **over}
    return rc.tiny_trainer(ops, load_case("clip_beta"), out, mu=1, ga=1, n_rows=4, **over)


@pytest.mark.parametrize("fix_vit", [True, False])
def test_alpha_one_gives_zero_kl_on_the_next_rollout(hip_ops, tmp_path, fix_vit):
    """beta = 0.04 (the fixture's), alpha = 1, a sync every 2 steps: after step 2 the reference IS the policy, so step 3 scores its rollout against itself -
    kl exactly 0 unless the reference forward read something derived from the old reference weights (the padded vision projections are cached per
    Arena.version) - and step 4 sees the policy one update away."""
    tr = _trainer(hip_ops, tmp_path, fix_vit=fix_vit)
    assert tr.beta == 0.04
    snaps = sc.run_with_snapshots(tr)
    assert sc.identity_ok(snaps[1]["ref"], snaps[1]["pol"], snaps[0]["ref"])
    kl = [l["kl"] for l in tr.state.log_history]
    print("kl per step:", kl)
    assert kl[0] > 0 and kl[1] > 0
    assert kl[2] == 0.0, kl
    assert kl[3] > 0, kl
    assert ["ref_sync/weight_distance" in l for l in tr.state.log_history] == [False, True, False, True]


def test_resume_from_a_checkpoint_written_on_a_sync_step(hip_ops, tmp_path):
    """4 steps with a sync and a checkpoint at step 2 (and a sync at 4); checkpoint-2 resumed to step 4: the same reference bit for bit, the weights within
    the 2e-6 of test_configs_gpu.py's resume test (atomics ordering in the embedding gradient)."""
    tr = _trainer(hip_ops, tmp_path / "a", ref_model_mixup_alpha=0.6, save_steps=2)
    snaps = sc.run_with_snapshots(tr)
    saved = torch.load(tmp_path / "a" / "checkpoint-2" / "reference_policy.pt", weights_only=False)["ref_w16"]
    assert sc.same_bits(saved, snaps[1]["ref"]) and not sc.same_bits(saved, snaps[0]["ref"]), "the checkpoint holds the mixed reference"
    tr2 = _trainer(hip_ops, tmp_path / "b", ref_model_mixup_alpha=0.6)
    snaps2 = sc.run_with_snapshots(tr2, ckpt=str(tmp_path / "a" / "checkpoint-2"))
    assert [s["step"] for s in snaps2] == [3, 4]
    assert sc.same_bits(snaps2[0]["ref"], snaps[2]["ref"]), "the resumed run continues from the mixed reference"
    a, b = tr.params.train.master, tr2.params.train.master
    assert torch.allclose(a, b, atol=2e-6, rtol=0), float((a - b).abs().max())
    assert sc.same_bits(tr2.ref_model.w16, tr.ref_model.w16), "the reference after step 4's sync is the straight run's, bit for bit"
    assert sc.same_bits(tr2.ref_model.w16, sc.composite(snaps[2]["ref"], snaps2[1]["pol"], 0.6))
