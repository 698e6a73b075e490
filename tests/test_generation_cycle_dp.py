"""GRPOConfig.steps_per_generation under data parallelism (CPU, two gloo ranks on the oracle op backend): every rank runs the same optimizer steps and the same
collectives per generation cycle, the overlapped gradient exchange begins in each window's last micro-step, and the ranks end on the same weights."""
import os
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _worker(rank, world, port, q, shard, out_dir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import generation_cycle_cases as gc
    from helpers import load_case
    from oracle.ref_ops import RefOps
    # 8 rows over 2 ranks: 4 batches a rank, 2 windows of GA = 2, one cycle of k = 2 with mu = 2: 4 optimizer steps
    tr = gc.cycle_trainer(RefOps(), load_case("clip_beta"), os.path.join(out_dir, "r%d" % rank), mu=2, n_rows=8, shard_optimizer=shard)
    assert tr.dp.enabled and tr.dp.world == 2
    begins, sync = [], tr.optimizer.sync
    o_begin = sync.begin

    def begin(*a, **k):
        begins.append(1)
        return o_begin(*a, **k)
    holder = {}
    sync.begin = begin
    o_lb = tr.core.loss_backward

    def lb(st, *a, **k):
        holder.setdefault("sync_at_update", []).append(k.get("grad_sync") is not None)
        return o_lb(st, *a, **k)
    tr.core.loss_backward = lb
    rec = gc.run_recorded(tr)
    a = tr.params.train
    q.put((rank, tr.state.global_step, gc.update_order(rec["events"]), gc.names(rec["events"]).count("step"), len(begins), holder["sync_at_update"],
           a.w16.float().numpy().copy(), [l["reward"] for l in tr.state.log_history if "reward" in l], tr.generated_tokens))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("shard", [False, True])
def test_two_ranks_run_the_same_steps_and_end_on_the_same_weights(tmp_path, shard):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    import socket
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
    (_, step0, order0, n0, b0, s0, w0, rew0, tok0), (_, step1, order1, n1, b1, s1, w1, rew1, tok1) = res
    assert step0 == step1 == 4 and n0 == n1 == 4
    assert order0 == order1 == [(1, 1), (2, 1), (1, 2), (2, 2)]
    assert b0 == b1 == 4                                         # one overlapped exchange per optimizer step ...
    assert s0 == s1 == [False, True] * 4                         # ... begun in each window's LAST micro-step (GA = 2), first pass and replay-form updates alike
    assert (w0 == w1).all(), "every rank must hold the same weights after every cycle"
    assert rew0 == rew1 and len(rew0) == 2                       # metrics are gathered over the ranks: the rollout's keys on the two first updates only
    assert tok0 == tok1 > 0
