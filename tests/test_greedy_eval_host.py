"""Batched greedy evaluation, host side (CPU, the oracle op backend - it has no greedy_tokens op, so the batched path keeps the top_k = 1 sampler and, with
no row-count-dependent kernels, must reproduce the one-row path exactly): batching, dataset order, sharding over ranks, the gather, the C ABI entry."""
import os
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ROWS, NEW_TOKENS = 5, 6


def _rows(fx):
    rows = []
    for i in range(N_ROWS):
        r = dict(fx["row"])
        r["problem"] = "event %d" % i
        r["video_frames"] = torch.randint(0, 256, (4, 3, 56, 84), generator=torch.Generator().manual_seed(300 + i), dtype=torch.uint8).float()
        rows.append(r)
    return rows


def _trainer():
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from helpers import load_case
    from test_trainer_host_logic import make_trainer
    fx = load_case("clip_nobeta")
    cfg, tr = make_trainer(fx)
    tr._video_inputs = lambda ex: ([ex["video_frames"]], [2.0])
    return fx, tr


def _strip(records):
    return [{k: v for k, v in r.items() if k != "index"} for r in records]


def test_batched_evaluation_equals_one_row_path_in_dataset_order():
    from time_r1_amd import evaluate as E
    from time_r1_amd import data as D
    fx, tr = _trainer()
    ds = D.RowDataset(_rows(fx))
    m0, rec0 = E.evaluate_grounding(tr, ds, max_new_tokens=NEW_TOKENS)
    assert len(rec0) == N_ROWS and all("index" not in r for r in rec0), "batch_size=None keeps the former record keys"
    assert len({r["completion"] for r in rec0}) > 1, "the rows must not all decode to the same text"
    for k in (1, 2, 3):
        m, rec = E.evaluate_grounding(tr, ds, max_new_tokens=NEW_TOKENS, batch_size=k)
        assert [r["index"] for r in rec] == list(range(N_ROWS))
        assert [r["problem"] for r in rec] == ["event %d" % i for i in range(N_ROWS)]
        assert _strip(rec) == rec0 and m == m0, k
    m, rec = E.evaluate_grounding(tr, ds, max_new_tokens=NEW_TOKENS, batch_size=2, limit=3)
    assert _strip(rec) == rec0[:3] and m == E.grounding_metrics([r["iou"] for r in rec0[:3]])
    for bad in (0, 65, -1, 2.5, True):
        with pytest.raises(ValueError):
            E.evaluate_grounding(tr, ds, max_new_tokens=NEW_TOKENS, batch_size=bad)
    with pytest.raises(ValueError):
        E.evaluate_grounding(tr, ds, max_new_tokens=NEW_TOKENS, batch_size=2, rank=2, world=2)


def test_strided_shards_cover_the_dataset_once():
    from time_r1_amd import evaluate as E
    from time_r1_amd import data as D
    fx, tr = _trainer()
    ds = D.RowDataset(_rows(fx))
    m0, rec0 = E.evaluate_grounding(tr, ds, max_new_tokens=NEW_TOKENS, batch_size=2)
    parts = []
    for rank in range(3):
        m, rec = E.evaluate_grounding(tr, ds, max_new_tokens=NEW_TOKENS, batch_size=2, rank=rank, world=3)
        assert m is None and [r["index"] for r in rec] == list(range(rank, N_ROWS, 3))
        parts += rec
    assert sorted(parts, key=lambda r: r["index"]) == rec0
    assert E.gather_evaluation(list(reversed(rec0))) == (m0, rec0), "one process: sorted by index, metrics of all rows"


def test_filter_files_do_not_depend_on_the_batched_path(tmp_path):
    """The filter stage writes the same two files from the batched records (extra key "index") as from the one-row records."""
    from time_r1_amd import evaluate as E
    from time_r1_amd import data as D
    from time_r1_amd import filtering
    fx, tr = _trainer()
    rows = _rows(fx)
    items = [{"video": "v%d.mp4" % i, "duration": 30.0, "timestamp": list(r["solution"]), "pred": None, "sentence": r["problem"], "qid": "q%d" % i,
              "video_start": None, "video_end": None} for i, r in enumerate(rows)]
    _, rec0 = E.evaluate_grounding(tr, D.RowDataset(rows), max_new_tokens=NEW_TOKENS)
    _, rec2 = E.evaluate_grounding(tr, D.RowDataset(rows), max_new_tokens=NEW_TOKENS, batch_size=2)
    out = []
    for name, rec in (("a", rec0), ("b", E.gather_evaluation(rec2)[1])):
        shares, path = filtering.filter_epoch(items, rec, str(tmp_path / name), "random_sample", 3)
        files = sorted(os.listdir(tmp_path / name))
        out.append((shares, files, [open(tmp_path / name / f).read() for f in files if not f.endswith("_random.json")]))
    assert out[0] == out[1] and "train_v4_cloud.json" in out[0][1]


def test_greedy_rollout_options_and_early_stop_on_host_backend():
    """Rollout(greedy=True) on a backend without the greedy op: top_k = 1, stop at EOS, pad-initialised tokens, and the early stop (count of finished rows
    polled every poll_every steps) ends the loop without changing the tokens."""
    from time_r1_amd.grpo import GRPOCore
    from time_r1_amd import evaluate as E
    fx, tr = _trainer()
    row = _rows(fx)[0]
    C = 40
    outs = {}
    for pe in (0, 4):
        core = GRPOCore(tr.engine, None, 1, C, beta=0.0, temperature=1.0, top_k=7, seed=0, rope_index_mode=tr.args.rope_index_mode, reuse_prefill=False, greedy=True)
        assert core.roll.greedy and core.roll.top_k == 1 and core.roll.stop_at_eos and core.roll.poll_every == 8
        core.roll.poll_every = pe
        sts = [E._prepare_row(tr, core, row) for _ in range(2)]
        if pe == 0:
            first = core.rollout_many(sts)[0].clone()
            assert core.roll.last_steps_run == C - 1
            core.roll.calls = 0
        eos = int(first[0, 3])
        old, core.cfg.eos_token_id = core.cfg.eos_token_id, eos
        try:
            toks = core.rollout_many(sts)
        finally:
            core.cfg.eos_token_id = old
        outs[pe] = (torch.stack([t.clone() for t in toks]), core.roll.last_steps_run)
    t0, n0 = outs[0]
    t4, n4 = outs[4]
    assert n0 == C - 1 and n4 <= 3 + 2 * 4 + 1 and n4 < C - 1, (n0, n4)
    assert torch.equal(t0, t4)
    ends = [int((t == eos).nonzero()[0, 1]) for t in t0]
    assert all(e <= 3 for e in ends) and all(bool((t[0, e + 1:] == core.cfg.pad_token_id).all()) for t, e in zip(t0, ends))
    assert not GRPOCore(tr.engine, None, 1, C, beta=0.0).roll.greedy


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from time_r1_amd import evaluate as E
    from time_r1_amd import data as D
    fx, tr = _trainer()
    assert tr.dp.world == world and tr.dp.rank == rank
    m, rec = E.evaluate_grounding(tr, D.RowDataset(_rows(fx)), max_new_tokens=NEW_TOKENS, batch_size=2, rank=tr.dp.rank, world=tr.dp.world)
    assert m is None and [r["index"] for r in rec] == list(range(rank, N_ROWS, world))
    metrics, records = E.gather_evaluation(rec)
    q.put((rank, metrics, records))
    dist.barrier()
    dist.destroy_process_group()


def test_two_gloo_ranks_gather_the_single_process_result():
    import socket
    from time_r1_amd import evaluate as E
    from time_r1_amd import data as D
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=300) for _ in range(2)], key=lambda x: x[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    fx, tr = _trainer()
    m0, rec0 = E.evaluate_grounding(tr, D.RowDataset(_rows(fx)), max_new_tokens=NEW_TOKENS, batch_size=2)
    for rank, metrics, records in res:
        assert records == rec0 and metrics == m0, rank


def test_greedy_entry_point_is_declared_exported_and_bound():
    import ctypes
    import time_r1_amd  # noqa: F401
    from time_r1_amd import hip
    from time_r1_amd.ops import HipOps
    decls = hip.parse_header()
    assert "tr1_greedy_tokens_step" in decls
    ret, args = decls["tr1_greedy_tokens_step"]
    assert ret == "int" and [n for _, n in args] == ["logits", "ld", "rows", "V", "step_ptr", "tokens", "tok_ld", "finished", "eos_id", "pad_id", "next_ids",
                                                     "done_count", "stream"]
    assert hasattr(ctypes.CDLL(hip.LIB_PATH), "tr1_greedy_tokens_step") and "tr1_greedy_tokens_step" in hip.lib().decls
    assert callable(getattr(HipOps, "greedy_tokens", None))
    assert "vllm_infer.py:80-113" in open(hip.HEADER).read()
