"""In-engine evaluation for temporal grounding: greedy rollout with the training engine (no vLLM), the reference's answer regex and
its IoU / R1@k / mIoU aggregation (reference evaluate.py:125-149 answer extraction, src/vllm_inference/eval_all.py:65-137 metrics)."""
import re

import numpy as np


_SPAN = re.compile(r"(\d+\.?\d*) (to|and) (\d+\.?\d*)")


def extract_answer_span(text):
    """The reference's `extract_answer(..., "tg")` (evaluate.py:125-149): the LAST 'a to b' / 'a and b' pair anywhere in the output
    (case-sensitive); only when the whole string has none, the first <answer>..</answer> body (single line) is searched."""
    s = _SPAN.findall(text)
    if not s:
        m = re.search(r"<answer>(.*?)</answer>", text)
        s = _SPAN.findall(m.group(1).strip()) if m else []
        if not s:
            return None
    return float(s[-1][0]), float(s[-1][2])


def compute_iou(pred, gt):
    """Temporal IoU of two [start, end] spans (eval_all.py:65-86 semantics: intersection clipped at 0, union of the hull)."""
    if pred is None:
        return 0.0
    (ps, pe), (gs, ge) = pred, gt
    inter = max(0.0, min(pe, ge) - max(ps, gs))
    union = max(pe, ge) - min(ps, gs)
    return inter / union if union > 0 else 0.0


def grounding_metrics(ious, thresholds=(0.3, 0.5, 0.7)):
    ious = np.asarray(ious, dtype=np.float64)
    out = {"mIoU": float(ious.mean() * 100) if ious.size else 0.0}
    for t in thresholds:
        out["R1@%.1f" % t] = float((ious > t).mean() * 100) if ious.size else 0.0     # strict, like eval_all.py:129
    out["avg"] = sum(out.values()) / len(out)                                          # eval_all.py:131
    return out


def _prepare_row(trainer, core, row):
    video_inputs, fps_inputs = trainer._video_inputs(row)
    conv = trainer.make_conversation_video(row)
    text = trainer.processing_class.apply_chat_template(conv, tokenize=False, add_generation_prompt=True)
    pi = trainer.processing_class(text=[text], images=None, videos=[video_inputs[0]], fps=[fps_inputs[0]], padding=True, return_tensors="pt",
                                  padding_side="left", add_special_tokens=False)
    return core.prepare(np.asarray(pi["input_ids"]).reshape(-1), pi["pixel_values_videos"], np.asarray(pi["video_grid_thw"]))


def _score_row(trainer, row, toks):
    completion = trainer.processing_class.batch_decode(toks, skip_special_tokens=True)[0]
    iou = compute_iou(extract_answer_span(completion), row["solution"])
    return {"problem": row["problem"], "solution": list(row["solution"]), "completion": completion, "iou": iou}


def evaluate_grounding(trainer, dataset, max_new_tokens=None, limit=None, batch_size=None, rank=0, world=1, repetition_penalty=1.0):
    """Greedy-decodes one completion per row with the trainer's engine and scores it. Returns (metrics, per-row records).
    repetition_penalty != 1 (SamplingParams(repetition_penalty=...) of the reference's vllm_infer.py:106-111): the argmax is taken over the penalised logits.

    batch_size=None: one row at a time through the top_k = 1 sampler, every decode step enqueued.
    batch_size in [1, 64]: rows rank, rank + world, ... of the first `limit` rows (the reference's --curr_idx / --total_idx sharding, evaluate.py:44-45),
    `batch_size` prompts decoded together (one row each, the last batch may be short) on a greedy core: argmax tokens from one launch per step, and the decode
    loop ends soon after every row of the batch has produced EOS (rollout.Rollout).  Records stay in dataset order and also carry "index" (the dataset
    index).  world > 1: returns (None, this rank's records); gather_evaluation() completes them on every rank."""
    from .grpo import GRPOCore
    a = trainer.args
    n = len(dataset) if limit is None else min(limit, len(dataset))
    C = max_new_tokens or trainer.max_completion_length
    if batch_size is not None:
        if isinstance(batch_size, bool) or int(batch_size) != batch_size or not 1 <= int(batch_size) <= 64:
            raise ValueError("batch_size must be None or an integer in [1, 64] (the decode step holds at most 64 rows), got %r" % (batch_size,))
        if not 0 <= int(rank) < int(world):
            raise ValueError("need 0 <= rank < world, got rank %r, world %r" % (rank, world))
        core = GRPOCore(trainer.engine, None, 1, C, beta=0.0, temperature=1.0, top_k=1, seed=0, rope_index_mode=a.rope_index_mode, stop_at_eos=True,
                        reuse_prefill=False, greedy=True, repetition_penalty=repetition_penalty)
        mine = list(range(int(rank), n, int(world)))
        records = []
        for k in range(0, len(mine), int(batch_size)):
            idx = mine[k:k + int(batch_size)]
            rows = [dataset[i] for i in idx]
            toks = core.rollout_many([_prepare_row(trainer, core, row) for row in rows])
            for i, row, t in zip(idx, rows, toks):
                rec = _score_row(trainer, row, t.cpu())
                rec["index"] = i
                records.append(rec)
        if int(world) > 1:
            return None, records
        return grounding_metrics([r["iou"] for r in records]), records
    core = GRPOCore(trainer.engine, None, 1, C, beta=0.0, temperature=1.0, top_k=1, seed=0,
                    rope_index_mode=a.rope_index_mode, stop_at_eos=True, reuse_prefill=False, repetition_penalty=repetition_penalty)
    records = []
    for i in range(n):
        row = dataset[i]
        toks = core.rollout(_prepare_row(trainer, core, row)).cpu()
        records.append(_score_row(trainer, row, toks))
    return grounding_metrics([r["iou"] for r in records]), records


def gather_evaluation(records):
    """This rank's records of evaluate_grounding(..., rank, world) -> (metrics, all records sorted by "index") on EVERY rank
    (torch.distributed.all_gather_object; a single process gets its own records back)."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        parts = [None] * dist.get_world_size()
        dist.all_gather_object(parts, records)
        records = [r for p in parts for r in p]
    records = sorted(records, key=lambda r: r["index"])
    return grounding_metrics([r["iou"] for r in records]), records
