"""Packed 12-bit gate/up weights on the GPU (csrc/gemm_pk.hip): the packer writes the torch reference's bytes, and the packed decode kernel stores the bits of
the bf16 kernel - random weights plus adversarial stages (patches, +-max, Inf / NaN, signed zeros) where the stream starts, ends and changes pair."""
import pytest
import torch

import time_r1_amd  # noqa: F401
import time_r1_amd.torch_ops as T

import pack12_cases as C

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


def _pack_matches_reference(hip_ops, w):
    rec, tails, ok = T.pack_bf16_glu_ref(w)
    image = hip_ops.pack_bf16_glu(w.cuda())
    n = rec.shape[0]
    assert image.numel() == n * (T.PK_REC + 4 * T.PK_TAIL_DW) + 16
    assert torch.equal(image[:n * T.PK_REC].cpu().view(n, T.PK_REC), rec), "records differ"
    assert torch.equal(image[n * T.PK_REC:-16].view(torch.int32).cpu().view(n, T.PK_TAIL_DW), tails), "tails differ"
    assert bool(hip_ops.pack_flag(image).item() == 0) == ok
    return ok


@pytest.mark.parametrize("name", ["normal", "uniform", "student_t", "zero", "denormal"])
def test_packer_writes_the_reference_bytes_on_distributions(hip_ops, name):
    assert _pack_matches_reference(hip_ops, C.distributions(64, 1536)[name])


@pytest.mark.parametrize("K", [1536, 2048, 3584])
def test_packer_writes_the_reference_bytes_on_adversarial_stages(hip_ops, K):
    I = 48
    w = C.distributions(I, K, seed=K)["student_t"].clone()
    for i, kind in enumerate(C.ADVERSARIAL):
        C.fill_stage(w, I, K, (i % 3, (3 * i) % 8, i % (K // 512)), kind)
    assert _pack_matches_reference(hip_ops, w)
    C.fill_stage(w, I, K, (2, 7, K // 512 - 1), "P_plus_1")                  # one stage too many patches: the flag, and still the reference's bytes
    assert not _pack_matches_reference(hip_ops, w)


def _adversarial_weight(I, K, second_pair):
    nst = K // 512
    w = C.distributions(I, K, seed=I + K)["normal"].clone()
    C.fill_stage(w, I, K, (0, 0, 0), "exactly_P")                            # the first stage of the stream
    C.fill_stage(w, I, K, (I // 16 - 1, 7, nst - 1), "inf_nan")              # the last one
    C.fill_stage(w, I, K, (second_pair, 0, 0), "max_one_tiny")               # the first stage of a block's second pair
    C.fill_stage(w, I, K, (0, 3, 1), "neg_zero")
    C.fill_stage(w, I, K, (0, 5, nst - 1), "inf_window")
    return w


def _twin_matches(hip_ops, w, I, K, rows, glu=True):
    g = torch.Generator().manual_seed(rows)
    x = torch.randn(rows, K, generator=g).to(BF16).cuda()
    lnw = (1 + 0.1 * torch.randn(K, generator=g)).to(BF16).cuda()
    w = w.cuda()
    image = hip_ops.pack_bf16_glu(w)
    assert int(hip_ops.pack_flag(image).item()) == 0
    want = hip_ops.norm_gemm(x, lnw, 1e-6, w, glu=glu)
    got = hip_ops.norm_gemm_glu_pk(x, lnw, 1e-6, image, I, glu=glu)
    assert want.shape == got.shape and C.same_bits(want.cpu(), got.cpu())


_WEIGHTS = {}


def _weights(I, K, second_pair=1):
    key = (I, K, second_pair)
    if key not in _WEIGHTS:
        _WEIGHTS[key] = (C.distributions(I, K, seed=I * K)["normal"], _adversarial_weight(I, K, second_pair))
    return _WEIGHTS[key]


@pytest.mark.parametrize("rows", [1, 9, 16])
@pytest.mark.parametrize("I", [32, 592])
@pytest.mark.parametrize("K", [1536, 3584])
def test_packed_kernel_stores_the_bf16_kernels_bits(hip_ops, K, I, rows):
    for w in _weights(I, K):
        _twin_matches(hip_ops, w, I, K, rows)


def test_packed_kernel_with_several_uneven_pairs_per_block(hip_ops):
    """More column-group pairs than CUs: blocks own one or two pairs, the adversarial stage sits at the start of a block's SECOND pair."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    K, NP = 2048, cus + cus // 6 + 1
    b = next(b for b in range(cus) if NP * (b + 1) // cus - NP * b // cus == 2)
    I = NP * 16
    for w in _weights(I, K, second_pair=NP * b // cus + 1):
        _twin_matches(hip_ops, w, I, K, 16)


def test_packed_kernel_fragment_major_output(hip_ops):
    I, K = 96, 1536
    for w in _weights(I, K):
        _twin_matches(hip_ops, w, I, K, 16, glu=2)


def _decode_logits(eng, cfg, ops, packed):
    """One rollout of a fresh core (same seed every time) -> (logits of every native decode step, tokens, per-layer 'packed copy used' of the plan)."""
    from time_r1_amd.grpo import GRPOCore
    from time_r1_amd.synthetic import synthetic_prompt
    core = GRPOCore(eng, None, 8, 5, beta=0.0, seed=5, rope_index_mode="hf4")
    core.roll.pack_gate_up, core.roll.PK_FROM_CALL = packed, 0
    ids, pix, grid = synthetic_prompt(cfg, (4, 6, 8), 9, 7, seed=2, text_vocab=400)
    rec, used, orig = [], [], ops.decode_step

    def spy(plan, *a, **k):
        out = orig(plan, *a, **k)
        rec.append(out.clone())
        used[:] = list(plan["pk"]) if plan.get("pk") is not None else []
        return out
    ops.decode_step = spy
    try:
        st = core.prepare(ids, pix, grid)
        core.rollout(st)
    finally:
        del ops.decode_step
    return torch.stack(rec).cpu(), st.completion_ids.cpu(), used


def test_decode_step_with_packed_copies_follows_the_weights(hip_ops):
    """2 layers of hidden 1536: the native decode step with packed gate/up copies gives the logits of the bf16 step bit for bit; after an in-place change of
    the weights and a version bump the copies are rebuilt; a matrix with an overflowing stage keeps the bf16 launch (and the logits)."""
    from time_r1_amd.config import tiny_test
    from time_r1_amd.params import ModelParams
    from time_r1_amd.model import Engine
    cfg = tiny_test(n_layers=2)
    t = cfg.text
    t.hidden, t.intermediate, t.n_heads, t.n_kv_heads, t.head_dim, t.mrope_section = 1536, 640, 12, 2, 128, (16, 24, 24)
    cfg.vision.out_hidden = 1536
    ops = hip_ops
    params = ModelParams(cfg, ops, seed=1)
    eng = Engine(cfg, ops, params)
    arena = params.train
    want, toks, used = _decode_logits(eng, cfg, ops, False)
    assert used == [] and want.shape[0] == 4
    got, toks_pk, used = _decode_logits(eng, cfg, ops, True)
    assert used == [True, True] and torch.equal(toks, toks_pk) and C.same_bits(want, got)
    # the weights change in place (as the optimizer's kernels change them) and the arena says so
    arena.w("l0.gu.w").mul_(-1.5)
    arena.version += 1
    got2, _, used = _decode_logits(eng, cfg, ops, True)
    want2, _, _ = _decode_logits(eng, cfg, ops, False)
    assert used == [True, True] and C.same_bits(want2, got2) and not C.same_bits(want2, want)
    # one stage of layer 1 with more patches than a tail holds: that layer keeps the bf16 launch
    w = arena.w("l1.gu.w")
    blk = w.cpu()
    C.fill_stage(blk, t.intermediate, t.hidden, (3, 2, 1), "P_plus_1")
    w.copy_(blk)
    arena.version += 1
    got3, _, used = _decode_logits(eng, cfg, ops, True)
    want3, _, _ = _decode_logits(eng, cfg, ops, False)
    assert used == [True, False] and C.same_bits(want3, got3)
