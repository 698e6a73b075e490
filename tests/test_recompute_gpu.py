"""activation_recompute="mlp" on HipOps: the three shapes of tests/recompute_cases.py bit for bit against "none" (both forward paths, a replay), the stream
rule over two consecutive micro-steps, and the peak-memory saving at 8192 rows.  The CPU side is tests/test_recompute_ref.py."""
import gc

import pytest
import torch

import recompute_cases as rcc

pytestmark = pytest.mark.gpu
MIB = 1 << 20


@pytest.fixture(autouse=True)
def _release():
    yield
    gc.collect()
    if torch.cuda.is_available():
        torch.cuda.empty_cache()


@pytest.mark.parametrize("reuse_prefill", [True, False], ids=["prefill+continuation", "full-sequence"])
@pytest.mark.parametrize("shape", list(rcc.SHAPES))
def test_hip_gradients_and_outputs_equal_the_none_run_bit_for_bit(hip_ops, shape, reuse_prefill):
    """gemm_glu runs its fused kernel above 64 rows and GEMM + swiglu below, the tile picker and rmsnorm's kernel vary with the row count: the recompute repeats
    the forward's launches over the forward's row ranges, so nothing may differ - there is no tolerance to loosen."""
    kw = dict(beta=0.04, reuse_prefill=reuse_prefill)
    none = rcc.micro_steps(hip_ops, rcc.SHAPES[shape], "none", **kw)
    mlp = rcc.micro_steps(hip_ops, rcc.SHAPES[shape], "mlp", **kw)
    rcc.assert_equal_runs(mlp, none, (shape, kw))


@pytest.mark.parametrize("variant,fix_vit", [("qwen2_vl", True), ("qwen2_5_vl", False)])
def test_hip_replayed_update_is_exact_too(hip_ops, variant, fix_vit):
    kw = dict(variant=variant, beta=0.04, fix_vit=fix_vit, replay=True, entropy_coef=0.01)
    none = rcc.micro_steps(hip_ops, rcc.SHAPES["tail"], "none", **kw)
    mlp = rcc.micro_steps(hip_ops, rcc.SHAPES["tail"], "mlp", **kw)
    assert not torch.equal(mlp[0]["replay_grad"], mlp[0]["grad"])
    rcc.assert_equal_runs(mlp, none, ("replay", kw))


def test_stream_rule_two_consecutive_micro_steps(hip_ops):
    """118 rows: "none" runs three of the four weight gradients per layer on the side stream.  "mlp" keeps all of them on the main stream - the one transient set
    is overwritten by the next layer (and by the next micro-step) - and opens no side stream at all; two micro-steps back to back still equal the "none" run."""
    kn, km = {}, {}
    none = rcc.micro_steps(hip_ops, rcc.SHAPES["short-continuation"], "none", beta=0.04, steps=2, keep=kn)
    mlp = rcc.micro_steps(hip_ops, rcc.SHAPES["short-continuation"], "mlp", beta=0.04, steps=2, keep=km)
    assert kn["eng"]._side is not None, "the none run is meant to be in the side-stream regime"
    assert km["eng"]._side is None
    assert not torch.equal(mlp[0]["grad"], mlp[1]["grad"])
    rcc.assert_equal_runs(mlp, none, "two micro-steps")


def test_peak_memory_drops_by_the_saved_activations(hip_ops):
    """tiny_test(n_layers=4), P = 4096, G = 4, C = 1024: 8192 rows, completions forced, no rollout.  The bound is arithmetic, not a measurement:
    what "none" saves and "mlp" does not (67.1 MB), less the one transient set (16.8 MB), less the caching allocator's 2 MiB large-block rounding on each of the
    transient set's four buffers (8.4 MB) - about 42 MB."""
    shape, peaks, retries = (4096, 4, 1024), {}, {}
    M = shape[0] + shape[1] * shape[2]
    for mode in ("none", "mlp"):
        keep = {}

        def before(eng):
            torch.cuda.synchronize()
            gc.collect()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            retries[mode] = torch.cuda.memory_stats().get("num_alloc_retries", 0)
        res = rcc.micro_steps(hip_ops, shape, mode, reuse_prefill=False, n_layers=4, grid=(4, 8, 8), before_step=before, keep=keep)
        torch.cuda.synchronize()
        peaks[mode] = torch.cuda.max_memory_allocated()
        retries[mode] = torch.cuda.memory_stats().get("num_alloc_retries", 0) - retries[mode]
        eng = keep.pop("eng")
        peaks[mode + "_ctx"] = eng.ctx_bytes(M)
        transient = eng.recompute_set_bytes(M)
        assert float(res[0]["grad"].abs().max()) > 0
        del res, eng
        gc.collect()
        torch.cuda.empty_cache()
    saved = peaks["none_ctx"] - peaks["mlp_ctx"]
    assert (saved, transient) == (67108864, 16777216)
    bound = saved - transient - 4 * 2 * MIB
    print("OBS peak allocated: none %.1f MB, mlp %.1f MB, difference %.1f MB (bound %.1f MB); allocator retries %s"
          % (peaks["none"] / 1e6, peaks["mlp"] / 1e6, (peaks["none"] - peaks["mlp"]) / 1e6, bound / 1e6, retries))
    assert peaks["none"] - peaks["mlp"] >= bound, (peaks, bound)
    assert retries["none"] == retries["mlp"] == 0, retries
