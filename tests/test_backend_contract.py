"""The op seam between the product backend and its CPU checker: every public method of oracle.ref_ops.RefOps exists on time_r1_amd.ops.HipOps with the same
parameters in the same order, except the HIP-only keywords listed here.  No device needed: both classes import without one."""
import inspect

import torch

import vocab_cases as vc
from oracle.ref_ops import RefOps
from time_r1_amd.ops import HipOps

# Parameters HipOps has and RefOps deliberately lacks.  attn_fwd: launch plans and layouts of the HIP kernels.  sample_tokens: next_ids feeds the fused decode
# step, done_count the early-stop poller - Rollout looks at the signature and falls back to copying / summing the finished flags on the oracle.
HIP_ONLY = {
    "attn_fwd": ("plan", "plan_mode", "v_rows", "live96"),
    "sample_tokens": ("next_ids", "done_count"),
}
# Ops HipOps has and RefOps must NOT have: each one switches an optional fast path of the engine on by its presence (hasattr / getattr), and the CPU
# tests and the recorded op sequences under tests/golden/ are of the plain path.
FAST_PATH_ONLY = ("greedy_tokens", "decode_step", "attn_plan", "wgrad_nn", "wgrad_sumsq", "wgrad_sumsq_partials", "vit_pad128_ok", "attn_fwd_rows_ok",
                  "pack_bf16_glu", "lora_wgrad_splits", "lora_wgrad_covers", "lora_wgrad_composed")


def _public_methods(cls):
    return {n: f for n, f in vars(cls).items() if not n.startswith("_") and callable(getattr(cls, n))}


def _params(cls, name):
    return [p for p in inspect.signature(getattr(cls, name)).parameters if p != "self"]


def test_every_oracle_op_is_a_hip_op_with_the_same_parameters():
    names = sorted(_public_methods(RefOps))
    assert len(names) >= 50 and {"gemm_nt", "grpo_policy_loss", "adamw_step_sr16", "lora_merge", "mark_seen"} <= set(names)
    seen_hip_only = {}
    for n in names:
        assert callable(getattr(HipOps, n, None)), "RefOps.%s has no counterpart on HipOps" % n
        ref, hip = _params(RefOps, n), _params(HipOps, n)
        extra = tuple(p for p in hip if p not in ref)
        assert ref == [p for p in hip if p not in extra], "%s: RefOps%s is not HipOps%s without its HIP-only parameters" % (n, ref, hip)
        if extra:
            seen_hip_only[n] = extra
    assert seen_hip_only == HIP_ONLY


def test_the_oracle_lacks_the_optional_fast_paths():
    for n in FAST_PATH_ONLY:
        assert hasattr(HipOps, n), n
        assert not hasattr(RefOps(), n), "RefOps.%s would switch a fast path of the engine on in the CPU tests" % n


def test_sampler_defaults_run_the_unfiltered_path_bit_for_bit():
    """top_p = 1 and min_p = 0 spelled out give the tokens and uniforms of a call that names neither (one vocab_cases sweep row set, top_k 0 and 50)."""
    rows, steps = 4, 3
    logits = vc.sweep_rows(rows, vc.V_FULL)
    for top_k in (0, 50):
        out = []
        for kw in ({}, dict(top_p=1.0, min_p=0.0)):
            tokens, u = torch.zeros(rows, steps, dtype=torch.int32), torch.zeros(rows, steps)
            for s in range(steps):
                RefOps().sample_tokens(logits, 0.7, top_k, vc.SWEEP_SEEDS[1], torch.tensor([s], dtype=torch.int32), tokens, None, -1, 0, False, u_out=u[:, s], **kw)
            out.append((tokens, u))
        assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
        assert len(set(out[0][0].reshape(-1).tolist())) > 1 and float(out[0][1].min()) > 0
