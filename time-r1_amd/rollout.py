"""Rollout: G sampled completions per prompt, replacing `unwrapped_model.generate(..., num_return_sequences=G)`
(reference src/time_r1/rl/timer1_trainer.py:568-578, GenerationConfig at :371-377).

MI355X-first structure: the vision tower and the ~3.4k-token prompt are processed ONCE (the reference replicates
them G times), the prompt's K/V live once in the cache and are shared by all G rows through the two-interval attention mask, and
each decode step is a batch of single-token rows whose GEMMs take the HBM-streaming skinny kernel.  Decode is weight-bandwidth
bound, so the prompts of one gradient-accumulation window (weights are constant inside it) are decoded TOGETHER: with GA = 2 and
G = 8 every weight byte read from HBM serves 16 rows instead of 8.  Attention stays per prompt (own prefix, own KV cache).
"""
import inspect
from collections import namedtuple

import numpy as np
import torch

from .positions import PackedLayout

I32 = torch.int32


class KVCache:
    """Per layer ONE K buffer [B*s_cap, kv_dim] and ONE V^T buffer [kv_dim, B*s_cap] for the B prompts decoded together; prompt b owns
    slots [b*s_cap, (b+1)*s_cap) and sees them through views, so a single fused kernel appends the new K/V of all B*G rows."""

    def __init__(self, ops, n_layers, kv_dim, s_cap, B):
        self.s_cap, self.B = s_cap, B
        self.k = [ops.zeros(B * s_cap, kv_dim) for _ in range(n_layers)]
        self.vt = [ops.zeros(kv_dim, B * s_cap) for _ in range(n_layers)]

    def views(self, b):
        a, e = b * self.s_cap, (b + 1) * self.s_cap
        return [(k[a:e], vt[:, a:e]) for k, vt in zip(self.k, self.vt)]


class Rollout:
    """greedy=True (evaluation / sample filtering, the reference's SamplingParams(temperature=0) at src/vllm_inference/vllm_infer.py:80-113): every token is
    the lowest index among its row's maxima (ops.greedy_tokens, one launch per step; a backend without that op keeps the top_k = 1 sampler), rows stop at
    EOS and the decode loop stops early: every `poll_every` steps the count of finished rows is copied to pinned host memory behind an event, and before a
    step is enqueued the host reads only a copy recorded at least `poll_every` steps earlier - it never waits on the step it has just enqueued, the queue
    never drains, and no per-step .item() / synchronize() exists.  Up to 2 * poll_every padding-only steps may therefore run after the last row has
    finished; the result equals running all C - 1 steps, because finished rows only ever receive pad_token_id (tokens start as pad_token_id in this mode).
    poll_every=0 switches the early stop off.  last_steps_run = decode steps enqueued by the last call.  greedy=False: nothing of this is executed, unless
    the attribute early_stop is set (GRPOConfig.trim_completions): with stop_at_eos and poll_every > 0 the sampled loop then runs the same poller, native
    step and op-by-op step alike.  Its tokens start as pad_token_id too, and the sampler kernels count the rows they finish on the device (done_count of
    ops.sample_tokens) as the greedy kernel does; a backend whose sample_tokens has no done_count argument is polled through finished.sum().  Steps that
    were not enqueued leave track_logp's log-probs at 0 behind the last EOS (a full run writes the pad token's there); both lie outside the completion mask.

    top_p / min_p / repetition_penalty (HF generate's order: penalty, temperature, top-k, top-p, min-p; defaults 1 / 0 / 1 = off, and then no call differs
    from a Rollout without them).  A token is seen by a row when it is in the row's prompt or was drawn for the row before (padding of finished rows
    does not count); a seen token's logit x becomes x * penalty (x < 0) or x / penalty, rounded to bf16, in a buffer of its own - track_logp keeps
    reading the raw logits, as it already ignores top-k.  Greedy mode honours the penalty and ignores top_p / min_p (the argmax survives both).  A
    backend whose sample_tokens lacks top_p / min_p, or that has no penalize_logits / mark_seen, raises NotImplementedError when a non-default is asked."""

    def __init__(self, engine, num_generations, max_completion_length, temperature=1.0, top_k=50, seed=1234, stop_at_eos=False, greedy=False, poll_every=8,
                 top_p=1.0, min_p=0.0, repetition_penalty=1.0):
        self.eng = engine
        self.top_p, self.min_p = 1.0 if top_p is None else float(top_p), 0.0 if min_p is None else float(min_p)
        self.repetition_penalty = 1.0 if repetition_penalty is None else float(repetition_penalty)
        if not 0.0 < self.top_p <= 1.0:
            raise ValueError("top_p must be in (0, 1] (1 = off), got %r" % (top_p,))
        if not 0.0 <= self.min_p <= 1.0:
            raise ValueError("min_p must be in [0, 1] (0 = off), got %r" % (min_p,))
        if not 0.0 < self.repetition_penalty < float("inf"):
            raise ValueError("repetition_penalty must be a positive number (1 = off), got %r" % (repetition_penalty,))
        self.G, self.C = int(num_generations), int(max_completion_length)
        self.temperature, self.top_k, self.seed, self.stop_at_eos = float(temperature), int(top_k or 0), int(seed), bool(stop_at_eos)
        self.greedy, self.poll_every = bool(greedy), int(poll_every or 0)
        self.early_stop = False       # sampled mode: end the decode loop once every row has drawn its EOS (needs stop_at_eos and poll_every > 0)
        if self.greedy:
            self.top_k, self.stop_at_eos = 1, True
        self.last_steps_run = 0
        self._cache = None
        self.calls = 0
        self.native_decode = True     # one native call per decode step (HipOps); False = op-by-op from the host (tests compare the two)
        self.weight_dtype = "bf16"    # "fp8" / "fp8-mfma": decode GEMMs read an e4m3 copy of the decoder matrices + lm_head (row scales), re-quantised
        #                               per call; "fp8" converts the codes to bf16 in registers (W8A16), "fp8-mfma" feeds them to the fp8 matrix
        #                               instruction with block-quantised e4m3 activations (W8A8, BASELINE config "CDNA4 fp8 MFMA")
        self._w8 = None
        self._pk_now = None           # this call's packed gate/up copies (_pack12)
        self.pack_gate_up = True      # bf16 rollouts: the native decode step streams a losslessly packed 12-bit image of the gate/up weights (csrc/gemm_pk.hip):
        #                               the same tokens bit for bit, 0.77x the bytes of the step's largest launch.  Repacked when the weights change (_pack12)
        self.fp8_keep_bf16 = ()       # matrices of the fp8 sampling policy that stay bf16: any of "qkv", "o", "gu", "down", "lm_head" (drift study)
        self.track_logp = False       # also record, per drawn token, its full-softmax log-prob under the logits it was SAMPLED from (one more pass
        #                               over the step's L2-resident logits): the drift of a quantised sampling policy against the bf16 policy of the
        #                               update is then a logged number (trainer metric rollout_logp_drift), and an importance weight is available
        self.last_sample_logp = None
        self.last_prefill = []        # per prompt of the last call: (saved prompt activations, cache views)
        self.decode_events = []       # HIP event pairs around the decode loops (read and cleared by the trainer's log(), never waited for here)

    def _kv(self, B, s_cap):
        t = self.eng.cfg.text
        c = self._cache
        if self.greedy:      # evaluation: every batch has other prompt lengths - round the capacity up and keep a cache that is large enough
            s_cap = (s_cap + 511) // 512 * 512
            if c is not None and c.B == B and c.s_cap >= s_cap:
                return c
        if c is None or c.s_cap != s_cap or c.B != B:
            self._cache = None      # release before re-allocating
            c = self._cache = KVCache(self.eng.ops, t.n_layers, t.kv_dim, s_cap, B)
        return c

    MATS = ("qkv.w", "o.w", "gu.w", "down.w")
    QBITS = {"qkv": 1, "o": 2, "gu": 4, "down": 8, "lm_head": 16}

    @staticmethod
    def cap_nsplit(nsplit, n_prompts, G, n_heads, n_kv, n_cus):
        """Split count of the decode attention such that (prompts x kv heads x 64-row query tiles) x splits stays within ONE round of blocks (a split-KV block
        takes a whole CU); never below 2 (the split-KV launch is what makes a decode step), unchanged when the launch is not split."""
        if nsplit <= 1:
            return nsplit
        groups = n_prompts * n_kv * ((G * (n_heads // n_kv) + 63) // 64)
        return max(2, min(nsplit, n_cus // max(1, groups)))

    def fp8_mask(self):
        keep = set(self.fp8_keep_bf16 or ())
        assert keep <= set(self.QBITS), "fp8_keep_bf16: unknown matrix in %r" % (keep,)
        return sum(b for n, b in self.QBITS.items() if n not in keep)

    def _quantize(self, arena, w_lm):
        """fp8 copies of the decode weights for THIS rollout (the weights change every optimizer step).  Only the sampling policy sees
        them: prefill, log-probs and the update keep bf16.  Buffers are allocated once and reused."""
        ops, t = self.eng.ops, self.eng.cfg.text
        if self._w8 is None:
            shapes = {"qkv.w": (t.qkv_dim, t.hidden), "o.w": (t.hidden, t.q_dim), "gu.w": (2 * t.intermediate, t.hidden), "down.w": (t.hidden, t.intermediate)}
            self._w8 = dict(layers=[{n: (torch.empty(*shapes[n], dtype=torch.uint8, device=ops.device), ops.empty(shapes[n][0], dtype=torch.float32))
                                     for n in self.MATS} for _ in range(t.n_layers)],
                            lm=(torch.empty(*w_lm.shape, dtype=torch.uint8, device=ops.device), ops.empty(w_lm.shape[0], dtype=torch.float32)))
        qm = self.fp8_mask()
        for i, L in enumerate(self._w8["layers"]):
            for n in self.MATS:
                if qm & self.QBITS[n[:-2]]:
                    ops.quantize_fp8_rows(arena.w("l%d.%s" % (i, n)), q=L[n][0], scale=L[n][1])
        if qm & 16:
            ops.quantize_fp8_rows(w_lm, q=self._w8["lm"][0], scale=self._w8["lm"][1])
        return self._w8

    PK_HEADROOM = 8 << 30     # device memory that must stay free after the packed copies are allocated
    PK_FROM_CALL = 1          # the copies are allocated from this call of the Rollout on (0: at once - tests)

    def _pack12(self, arena, rows):
        """Packed 12-bit copies of the layers' gate/up weights for the native bf16 decode step: -> dict(layers=[image], host=flags, event, ...), or
        None where there are none (backend, shape, memory).  The copies belong to the engine - one set, whichever Rollout decodes (training, evaluation,
        filtering) - and are rebuilt when the bytes the decode reads have changed: another arena, another arena.version (optimizer step, checkpoint load,
        LoRA merge) or a torch-side write into w16.  They are allocated from the SECOND call on and only where 8 GB of device memory stay free afterwards:
        by then torch's pool holds the peak of a whole step, so the copies (5.8 GB at 7B) can neither push the run's peak over the device nor make the
        allocator retry; a run without that room keeps the bf16 launch."""
        ops, t = self.eng.ops, self.eng.cfg.text
        if not (self.pack_gate_up and hasattr(ops, "pack_bf16_glu") and ops.glu_pk_ok(rows, t.intermediate, t.hidden)):
            return None
        pk = getattr(self.eng, "glu_pk", None)
        if pk is None:
            nb = ops.pack_bf16_glu_image_bytes(t.intermediate, t.hidden)
            if self.calls < self.PK_FROM_CALL or torch.cuda.mem_get_info(ops.device)[0] < t.n_layers * (nb + 1024) + self.PK_HEADROOM:
                return None
            pk = self.eng.glu_pk = dict(key=None, layers=[ops.empty(nb, dtype=torch.uint8) for _ in range(t.n_layers)], flags=ops.zeros(t.n_layers, dtype=I32),
                                        host=torch.zeros(t.n_layers, dtype=I32, pin_memory=True), event=torch.cuda.Event())
        key = (id(arena), arena.w16.data_ptr(), arena.w16._version, getattr(arena, "version", 0))
        if pk["key"] != key:
            for i, image in enumerate(pk["layers"]):
                ops.pack_bf16_glu(arena.w("l%d.gu.w" % i), image)
                pk["flags"][i:i + 1].copy_(ops.pack_flag(image))
            pk["host"].copy_(pk["flags"], non_blocking=True)
            pk["event"].record()
            pk["key"] = key
        return pk

    def generate(self, arena, prompt_ids, vid_embeds, vid_rows, prompt_pos3, delta, save_prefill=False):
        """One prompt. prompt_ids: int32 device tensor [P]; prompt_pos3: numpy [3, P]; returns (tokens int32 [G, C] on device, layout)."""
        return self.generate_many(arena, [(prompt_ids, vid_embeds, vid_rows, prompt_pos3, delta)], save_prefill)[0]

    def _filter_kwargs(self, ops):
        """Extra keyword arguments of ops.sample_tokens: none at the defaults (and in greedy mode), so a backend without them keeps working."""
        if self.greedy or (self.top_p == 1.0 and self.min_p == 0.0):
            return {}
        pars = inspect.signature(ops.sample_tokens).parameters
        if not ({"top_p", "min_p"} <= set(pars) or any(p.kind == p.VAR_KEYWORD for p in pars.values())):
            raise NotImplementedError("top_p = %g / min_p = %g: the %r backend's sample_tokens has no top_p / min_p arguments"
                                      % (self.top_p, self.min_p, getattr(ops, "name", type(ops).__name__)))
        return dict(top_p=self.top_p, min_p=self.min_p)

    def _stops_early(self):
        """The decode loop runs the early-stop poller: always in greedy mode, in sampled mode when early_stop asks for it and rows do stop at EOS."""
        return self.poll_every > 0 and (self.greedy or (self.early_stop and self.stop_at_eos))

    def _count_kwargs(self, ops, buf):
        """done_count for ops.sample_tokens where this call keeps a counter and the backend's sampler takes it (else none: the poller sums the flags)."""
        if buf.greedy_op or buf.done_count is None:
            return {}
        return dict(done_count=buf.done_count)

    def _penalized(self, buf, logits, r0=0):
        """The logits the selection reads: `logits` itself without a penalty, else their penalised copy in buf.pen[r0 : r0 + rows]."""
        if buf.seen is None:
            return logits
        n = logits.shape[0]
        return self.eng.ops.penalize_logits(logits, buf.seen[r0:r0 + n], self.repetition_penalty, out=buf.pen[r0:r0 + n])

    def _mark_drawn(self, buf, col, r0=0, n=None):
        """Column `col` of the tokens (just written) into the seen sets of rows [r0, r0 + n); finished rows hold padding there and are skipped."""
        if buf.seen is None:
            return
        n = buf.tokens.shape[0] - r0 if n is None else n
        self.eng.ops.mark_seen(buf.seen[r0:r0 + n], buf.seen_vocab, tokens=buf.tokens[r0:r0 + n], step_dev=buf.steps[col:col + 1],
                               finished=buf.finished[r0:r0 + n] if self.stop_at_eos else None)

    def _buffers(self, items, greedy_op, V=None):
        """What one call allocates: the per-row outputs, the packed layouts and the KV cache; with a repetition penalty also the seen bitmap
        (one bit per token of the V-token vocabulary and row) and the buffer of penalised logits."""
        ops, G, C, R = self.eng.ops, self.G, self.C, len(items) * self.G
        steps = ops.tensor(np.arange(C, dtype=np.int32), I32)
        sampled_stop = not self.greedy and self._stops_early()
        tokens = torch.full((R, C), int(self.eng.cfg.pad_token_id), dtype=I32, device=steps.device) if (self.greedy or sampled_stop) else ops.zeros(R, C, dtype=I32)
        finished = ops.zeros(R, dtype=I32)
        counted = greedy_op
        if sampled_stop:
            pars = inspect.signature(ops.sample_tokens).parameters
            counted = "done_count" in pars or any(p.kind == p.VAR_KEYWORD for p in pars.values())
        done_count = ops.zeros(1, dtype=I32) if counted else None      # rows that selected EOS; zeroed here, once per call
        slogp = ops.zeros(R, C, dtype=torch.float32) if self.track_logp else None
        lays = [PackedLayout(int(it[0].shape[0]), G, C) for it in items]
        seen = pen = None
        if self.repetition_penalty != 1.0:
            if not (hasattr(ops, "penalize_logits") and hasattr(ops, "mark_seen")):
                raise NotImplementedError("repetition_penalty = %g: the %r backend has no penalize_logits / mark_seen"
                                          % (self.repetition_penalty, getattr(ops, "name", type(ops).__name__)))
            V = int(self.eng.cfg.text.vocab_size if V is None else V)
            seen, pen = ops.zeros(R, (V + 31) // 32, dtype=I32), ops.empty(R, V)
        return _Buffers(greedy_op, steps, tokens, finished, done_count, slogp, lays, self._kv(len(items), max(l.S_cap for l in lays)), seen, pen, V)

    def release_cache(self):
        """Let go of the KV cache: the next call allocates its own.  For a caller that decodes again while a saved prefill of the last call - which holds
        views of that call's cache - is still to be read."""
        self._cache = None

    def _prefill(self, arena, w_lm, buf, b, item, save_prefill, slot=None):
        """Prompt b: prefill into its cache slots, first token (and its log-prob), and this prompt's decode tables.  slot: the engine's activation buffer set
        a saved prefill goes to (default b)."""
        prompt_ids, vid_embeds, vid_rows, prompt_pos3, delta = item
        eng, ops, cfg, t = self.eng, self.eng.ops, self.eng.cfg, self.eng.cfg.text
        G, C, half = self.G, self.C, t.head_dim // 2
        P, lay, kv_views = int(prompt_ids.shape[0]), buf.lays[b], buf.cache.views(b)
        seed = self.seed + 7919 * self.calls
        self.calls += 1
        # ---- prefill (prompt once, K/V written straight into the cache)
        pos_p = ops.tensor(np.ascontiguousarray(prompt_pos3.astype(np.int32)), I32)
        cos, sin = ops.mrope_table(pos_p, t.head_dim, t.mrope_section, t.rope_theta)
        masks = [ops.tensor(a, I32) for a in lay.prompt_masks()]
        h = eng.embed(arena, prompt_ids, vid_embeds, vid_rows)
        # save_prefill: the prompt rows' activations go straight into [P + G*C, .] buffers that the update's continuation forward completes
        bufs, is_stash = eng.alloc_ctx_bufs(lay.M, slot=b if slot is None else slot, prefill_rows=P) if save_prefill else (None, False)
        # (only the last prompt row's output is read: first-token logits here, the first prediction row of the update later)
        hL, pctx = eng.llm_fwd(arena, h, cos, sin, masks, save=save_prefill, kv_cache=kv_views, bufs=bufs, tail_from=eng.tail_rows_from(P, lay.M))
        if is_stash:
            pctx["stash"] = True
        hn, _, _ = ops.rmsnorm_fwd(hL[P - 1:P], arena.w("norm"), t.rms_eps, need_rstd=False)
        logits = ops.gemm_nt(hn, w_lm)  # [1, V]
        tokens, finished = buf.tokens[b * G:(b + 1) * G], buf.finished[b * G:(b + 1) * G]
        sel = logits      # what the selection reads: with a penalty, the one prefill row penalised by the prompt's tokens (all G rows have seen just those)
        if buf.seen is not None:
            ops.mark_seen(buf.seen[b * G:(b + 1) * G], buf.seen_vocab, ids=prompt_ids.contiguous())
            sel = self._penalized(buf, logits, b * G)
        if buf.greedy_op:
            ops.greedy_tokens(sel if G == 1 else sel.expand(G, sel.shape[1]).contiguous(), buf.steps[0:1], tokens, finished, cfg.eos_token_id,
                              cfg.pad_token_id, done_count=buf.done_count)
        else:
            ops.sample_tokens(sel.expand(G, sel.shape[1]), self.temperature, self.top_k, seed, buf.steps[0:1], tokens, finished,
                              cfg.eos_token_id, cfg.pad_token_id, self.stop_at_eos, **self._filter_kwargs(ops), **self._count_kwargs(ops, buf))
        self._mark_drawn(buf, 0, b * G, G)
        if buf.slogp is not None:      # (the first token is drawn from the bf16 prefill's logits in every mode)
            buf.slogp[b * G:(b + 1) * G, 0] = ops.logp_entropy_fwd(logits.expand(G, logits.shape[1]).contiguous(), tokens[:, 0].contiguous())[0]
        # ---- per-step tables (positions, slots, masks) built once
        comp_pos = (P + delta + np.arange(C, dtype=np.int64))
        pos_c = ops.tensor(np.repeat(comp_pos[None, :], 3, 0).astype(np.int32), I32)            # [3, C]
        cos_c, sin_c = ops.mrope_table(pos_c, t.head_dim, t.mrope_section, t.rope_theta)          # [C, hd/2]
        slots_all = ops.tensor(np.stack([lay.completion_slots(s) for s in range(C)]), I32)       # [C, G]
        pre_d, lo_d, _ = [ops.tensor(a, I32) for a in lay.decode_masks(0)]
        return dict(lay=lay, kv=kv_views, prefill_ctx=pctx, seed=seed, tokens=tokens, finished=finished, slots=slots_all, pre=pre_d, lo=lo_d,
                    cos=cos_c.view(C, 1, half).expand(C, G, half), sin=sin_c.view(C, 1, half).expand(C, G, half),
                    nsplit=max(1, min(28, ((P + 63) // 64 + 3) // 2)))

    def _step_tables(self, per, cache, n_cus):
        """The prompts' tables side by side, and the split count of the decode attention for all of them."""
        t = self.eng.cfg.text

        def cat(key, dim):
            return torch.cat([st[key] for st in per], dim).contiguous()
        # ONE round of blocks: a split-KV block takes a whole CU (145 KB of LDS), so (prompts x kv heads x 64-row query tiles) x splits above the CU count runs
        # as two rounds - 32 decode rows at 7B = 16 groups x 27 splits = 432 blocks took 25.1 us per layer at step 1 against 19.8 with 14 splits (round 5)
        nsplit = self.cap_nsplit(max(st["nsplit"] for st in per), len(per), self.G, t.n_heads, t.n_kv_heads, n_cus)
        slots = torch.cat([st["slots"] + b * cache.s_cap for b, st in enumerate(per)], 1).contiguous()
        return _StepTables(cat("cos", 1), cat("sin", 1), slots, cat("slots", 1), cat("pre", 0), cat("lo", 0), nsplit)

    def generate_many(self, arena, items, save_prefill=False, slot0=0):
        """items: list of (prompt_ids, vid_embeds, vid_rows, prompt_pos3, delta), decoded together. Returns [(tokens [G, C], layout)].
        save_prefill: keep the prompt rows' activations so the policy forward of the update can skip the prompt (same weights).  One flag for all items, or
        one per item: the saved ones take the engine's buffer sets slot0, slot0 + 1, ... in item order (slot0 > 0: an earlier call's saved prefills are
        still to be read), and last_prefill holds (None, cache views) for the others.
        Each prompt keeps its own sampling stream (seed advances per prompt), so results do not depend on how prompts are batched."""
        eng, ops, t = self.eng, self.eng.ops, self.eng.cfg.text
        G, C, B = self.G, self.C, len(items)
        dev = getattr(ops, "device", None)      # what the backend offers, looked at once per call (tests patch ops between calls)
        on_gpu = dev is not None and torch.device(dev).type == "cuda"
        greedy_op = self.greedy and hasattr(ops, "greedy_tokens")      # (a backend without the op: the top_k = 1 sampler, as before)
        w_lm = eng.params.lm_head_w(arena)
        self._filter_kwargs(ops)      # (a backend that cannot honour top_p / min_p: refuse before anything is computed)
        buf = self._buffers(items, greedy_op, int(w_lm.shape[0]))
        fused = B * G <= 64        # the fused decode kernels hold all rows of a step in one MFMA column block set
        native = fused and self.native_decode and hasattr(ops, "decode_step")
        self._pk_now = self._pack12(arena, B * G) if native and on_gpu and self.weight_dtype == "bf16" else None      # (the packers run ahead of the prefill)
        if isinstance(save_prefill, (list, tuple)):
            assert len(save_prefill) == B, "save_prefill: one flag per item"
            saves = [bool(x) for x in save_prefill]
            per = [self._prefill(arena, w_lm, buf, b, it, saves[b], slot=int(slot0) + sum(saves[:b])) for b, it in enumerate(items)]
        else:
            per = [self._prefill(arena, w_lm, buf, b, it, save_prefill) for b, it in enumerate(items)]
        tab = self._step_tables(per, buf.cache, int(torch.cuda.get_device_properties(dev).multi_processor_count) if on_gpu else 256)
        w8 = None
        if self.weight_dtype in ("fp8", "fp8-mfma"):
            assert fused and t.hidden % 128 == 0 and t.intermediate % 128 == 0 and t.q_dim % 128 == 0, "fp8 decode: <= 64 rows, K % 128 == 0"
            w8 = self._quantize(arena, w_lm)
        step = (_NativeStep if native else _HostStep)(self, arena, w_lm, buf, tab, per, w8)
        if on_gpu:
            ev0 = torch.cuda.Event(enable_timing=True)
            ev0.record()
        stop = _EarlyStop(buf, B * G, C, self.poll_every) if self._stops_early() else None
        self.last_steps_run = 0
        for s in range(C - 1):
            if stop is not None and stop.before(s):
                break
            self.last_steps_run = s + 1
            logits = step(s)
            step.select(s, logits)
            if buf.slogp is not None:
                buf.slogp[:, s + 1] = ops.logp_entropy_fwd(logits.contiguous(), buf.tokens[:, s + 1].contiguous())[0]
        if on_gpu:
            ev1 = torch.cuda.Event(enable_timing=True)
            ev1.record()
            self.decode_events = (self.decode_events + [(ev0, ev1)])[-64:]
        self.last_sample_logp = [buf.slogp[b * G:(b + 1) * G] for b in range(B)] if buf.slogp is not None else None
        self.last_prefill = [(st["prefill_ctx"], st["kv"]) for st in per]
        return [(st["tokens"], st["lay"]) for st in per]


# One call's allocations: tokens / slogp [B*G, C], finished [B*G], done_count [1] (greedy_op, or a sampled early stop whose backend counts; else None),
# steps = arange(C), one layout per prompt, the KV cache
# seen int32 [B*G, ceil(seen_vocab / 32)] / pen [B*G, seen_vocab]: only with a repetition penalty (else None)
_Buffers = namedtuple("_Buffers", "greedy_op steps tokens finished done_count slogp lays cache seen pen seen_vocab")
# cos / sin [C, B*G, half]; slots [C, B*G] into the unified cache; hi [C, B*G]: hi of step s = the slot just appended (cache-local); pre / lo [B*G]
_StepTables = namedtuple("_StepTables", "cos sin slots hi pre lo nsplit")


class _EarlyStop:
    """The poller of greedy mode and of a sampled early stop (Rollout's docstring): counts of finished rows copied to pinned host memory, read poll_every
    steps later.  The count is the kernels' own counter where the call keeps one, else the sum of the finished flags."""

    def __init__(self, buf, rows, C, poll_every):
        self.buf, self.rows, self.pe = buf, rows, poll_every
        self.on_dev = buf.steps.device.type == "cuda"
        self.host_counts = torch.zeros((C - 1) // poll_every + 1, dtype=I32, pin_memory=self.on_dev)
        self.polls = []          # (decode steps enqueued when the copy was recorded, slot in host_counts, event or None)

    def before(self, s):
        """Called before step s is enqueued: True = every row had finished at the oldest copy; records the next copy when one is due."""
        pe, polls, buf = self.pe, self.polls, self.buf
        if polls and s - polls[0][0] >= pe:          # a copy recorded >= poll_every steps ago: waiting for it leaves >= poll_every steps queued
            _, slot, ev = polls.pop(0)
            if ev is not None:
                ev.synchronize()
            if int(self.host_counts[slot]) >= self.rows:
                return True
        if s > 0 and s % pe == 0:
            slot = s // pe
            self.host_counts[slot:slot + 1].copy_(buf.done_count if buf.done_count is not None else buf.finished.sum(dtype=I32).reshape(1), non_blocking=True)
            ev = None
            if self.on_dev:
                ev = torch.cuda.Event()
                ev.record()
            polls.append((s, slot, ev))
        return False


class _Step:
    """One decode step of all B*G rows: logits = step(s) reads column s of the tokens, step.select(s, logits) writes column s + 1."""

    def __init__(self, roll, arena, w_lm, buf, tab, per, w8):
        self.roll, self.arena, self.w_lm, self.buf, self.tab, self.per, self.w8 = roll, arena, w_lm, buf, tab, per, w8
        self.ops, self.cfg, self.t = roll.eng.ops, roll.eng.cfg, roll.eng.cfg.text
        self.qmask, self.a8 = roll.fp8_mask(), roll.weight_dtype == "fp8-mfma"
        self.R, self.B, self.scale = tab.hi.shape[1], len(per), self.t.head_dim ** -0.5
        self.count_kw = roll._count_kwargs(self.ops, buf)      # looked at once per call, not per step


class _NativeStep(_Step):
    """The whole step enqueued by ONE native call (csrc/decode.hip): the host stays ahead of the GPU, no idle gaps between kernels.  The only place
    that does arithmetic on device addresses: step s reads row s of the cos / sin / slots / hi tables."""

    def __init__(self, *args):
        super().__init__(*args)
        ops, t, arena, w8, qmask, cache, tab = self.ops, self.t, self.arena, self.w8, self.qmask, self.buf.cache, self.tab

        def mat(i, n):      # fp8 codes, or the bf16 weight itself where there is no fp8 copy or the mask keeps this matrix in bf16
            return w8["layers"][i][n][0] if w8 is not None and qmask & self.roll.QBITS[n[:-2]] else arena.w("l%d.%s" % (i, n))

        pk, images = self.roll._pk_now, {}
        if pk is not None:         # packed gate/up copies; a layer whose matrix is not representable (flag 1) keeps the bf16 launch
            pk["event"].synchronize()
            images = {i: image for i, (f, image) in enumerate(zip(pk["host"].tolist(), pk["layers"])) if not int(f)}

        def layer_tensors(i):      # the slots of HipOps.DECODE_LAYER_SLOTS this step uses
            L = {n: arena.w("l%d.%s" % (i, n)) for n in ("ln1", "qkv.b", "ln2")}
            L.update({n: mat(i, n) for n in self.roll.MATS}, k=cache.k[i], vt=cache.vt[i])
            if w8 is not None:
                L.update({n[:-1] + "scale": w8["layers"][i][n][1] for n in self.roll.MATS})
            if i in images:
                L["gu.pk"] = images[i]
            return L
        fp8 = w8 is not None
        self.plan = ops.decode_plan([layer_tensors(i) for i in range(t.n_layers)], t.hidden, t.n_heads, t.n_kv_heads, t.head_dim, t.intermediate, t.vocab_size,
                                    self.R, self.B, cache.s_cap, tab.nsplit, weights=self.roll.weight_dtype if fp8 else "bf16", qmask=qmask if fp8 else 0)
        lm_p, lm_scale_p = (w8["lm"][0].data_ptr(), w8["lm"][1].data_ptr()) if fp8 and qmask & 16 else (self.w_lm.data_ptr(), 0)
        self.ids = ops.zeros(self.R, dtype=I32)
        self.fixed_p = (arena.w("embed").data_ptr(), arena.w("norm").data_ptr(), lm_p, lm_scale_p, self.ids.data_ptr())
        self.cos_p, self.sin_p, self.slot_p, self.hi_p = tab.cos.data_ptr(), tab.sin.data_ptr(), tab.slots.data_ptr(), tab.hi.data_ptr()
        self.pre_p, self.lo_p = tab.pre.data_ptr(), tab.lo.data_ptr()
        self.row_bytes, self.rope_bytes = self.R * 4, self.R * (t.head_dim // 2) * 4      # one step's row of the int32 [C, R] / fp32 [C, R, half] tables

    def __call__(self, s):
        if s == 0:
            self.ids.copy_(self.buf.tokens[:, 0])          # later steps: the sampler wrote the drawn tokens into ids itself (next_ids)
        return self.ops.decode_step(self.plan, *self.fixed_p, self.cos_p + s * self.rope_bytes, self.sin_p + s * self.rope_bytes,
                                    self.slot_p + s * self.row_bytes, self.pre_p, self.lo_p, self.hi_p + s * self.row_bytes, self.t.rms_eps, self.scale)

    def select(self, s, logits):
        roll, ops, cfg, buf = self.roll, self.ops, self.cfg, self.buf
        logits = roll._penalized(buf, logits)
        if buf.greedy_op:
            ops.greedy_tokens(logits, buf.steps[s + 1:s + 2], buf.tokens, buf.finished, cfg.eos_token_id, cfg.pad_token_id, next_ids=self.ids,
                              done_count=buf.done_count)
        else:
            # all prompts of the window in ONE sampler launch set; every prompt keeps its own Philox stream (seed_b = seed_0 + 7919 b)
            ops.sample_tokens(logits, roll.temperature, roll.top_k, self.per[0]["seed"], buf.steps[s + 1:s + 2], buf.tokens, buf.finished, cfg.eos_token_id,
                              cfg.pad_token_id, roll.stop_at_eos, group_rows=roll.G, seed_stride=7919, next_ids=self.ids, **roll._filter_kwargs(ops),
                              **self.count_kw)
        roll._mark_drawn(buf, s + 1)


class _HostStep(_Step):
    """The step op by op from the host: more than 64 rows, a backend without decode_step, or Rollout.native_decode = False (tests compare the tokens)."""

    def __init__(self, *args):
        super().__init__(*args)
        self.fused = self.R <= 64
        self.plan = self.ops.attn_plan(self.roll.G, self.t.n_heads, self.t.n_kv_heads, self.B) if self.fused and hasattr(self.ops, "attn_plan") else None

    def __call__(self, s):
        ops, t, arena, w8, tab = self.ops, self.t, self.arena, self.w8, self.tab
        ids_s = self.buf.tokens[:, s].contiguous()
        h = ops.gather_rows(arena.w("embed"), ids_s)
        rows = (tab.cos[s], tab.sin[s], tab.slots[s], tab.hi[s])
        for i in range(t.n_layers):
            h = self._layer(i, h, *rows)
        if w8 is not None and self.qmask & 16:
            return ops.gemm_w8(h, w8["lm"][0], w8["lm"][1], lnw=arena.w("norm"), eps=t.rms_eps, a8=self.a8)
        if self.fused:
            return ops.norm_gemm(h, arena.w("norm"), t.rms_eps, self.w_lm)
        hn, _, _ = ops.rmsnorm_fwd(h, arena.w("norm"), t.rms_eps, need_rstd=False)
        return ops.gemm_nt(hn, self.w_lm)

    def _layer(self, i, h, cs, sn, slots, hi):
        """Decoder layer i for one step.  Every kernel choice of the op-by-op path is made here; the counterpart is the layer loop of decode_step_impl in
        csrc/decode.hip.  Mirrored from it (up to 64 rows): norm + q/k/v projection + M-RoPE + KV append in one launch (head dim % 32 == 0), norm + gate/up
        + SwiGLU in one launch, the split-K fix-up down projection from 16 rows and intermediate 8192, and the attention tile plan that layer 0 publishes
        and the others read.  NOT mirrored: the fragment-major o projection (o_frag) and the fragment-major down projection on the fragment-major SwiGLU
        output (down_frag) - here gemm_nt / norm_gemm(glu=True) do that work; the W8A8 fix-up down projection is not chosen here either, ops.gemm_w8
        picks it by shape.  The final norm + lm_head (__call__) follows the native step's rule.  Above 64 rows (no native step exists) every projection is rmsnorm / gemm_nt / swiglu.  The tests ask for equal tokens."""
        ops, t, arena, a8, fused, cache, tab = self.ops, self.t, self.arena, self.a8, self.fused, self.buf.cache, self.tab
        hd, p = t.head_dim, "l%d." % i
        Q = self.w8["layers"][i] if self.w8 is not None else None
        q8 = (lambda n: Q is not None and bool(self.qmask & self.roll.QBITS[n]))        # this matrix of the sampling policy is fp8
        if q8("qkv"):
            qkv = ops.gemm_w8(h, Q["qkv.w"][0], Q["qkv.w"][1], lnw=arena.w(p + "ln1"), eps=t.rms_eps, bias=arena.w(p + "qkv.b"), a8=a8)
        elif fused and hd % 32 == 0:
            qkv = None
            q = ops.norm_gemm_qkv(h, arena.w(p + "ln1"), t.rms_eps, arena.w(p + "qkv.w"), arena.w(p + "qkv.b"), cs, sn, cache.k[i], cache.vt[i],
                                  slots, t.n_heads, t.n_kv_heads, hd)
        elif fused:      # rmsnorm folded into the projection's operand load (one launch instead of two)
            qkv = ops.norm_gemm(h, arena.w(p + "ln1"), t.rms_eps, arena.w(p + "qkv.w"), bias=arena.w(p + "qkv.b"))
        else:
            xn, _, _ = ops.rmsnorm_fwd(h, arena.w(p + "ln1"), t.rms_eps, need_rstd=False)
            qkv = ops.gemm_nt(xn, arena.w(p + "qkv.w"), bias=arena.w(p + "qkv.b"))
        if qkv is not None:
            q = ops.decode_qkv_post(qkv, cs, sn, cache.k[i], cache.vt[i], slots, t.n_heads, t.n_kv_heads, hd)
        # one launch for all prompts of the window: problem b = rows [b*G,(b+1)*G) over cache slots [b*s_cap, (b+1)*s_cap)
        pk = dict(plan=self.plan, plan_mode=1 if i == 0 else 2) if self.plan is not None and tab.nsplit > 1 else {}
        o, _ = ops.attn_fwd(q, cache.k[i], cache.vt[i], tab.pre, tab.lo, hi, t.n_heads, t.n_kv_heads, cache.s_cap, hd, self.scale,
                            nsplit=tab.nsplit, need_lse=False, n_batch=self.B, kv_batch_slots=cache.s_cap, **pk)
        h2 = ops.gemm_w8(o, Q["o.w"][0], Q["o.w"][1], residual=h, a8=a8) if q8("o") else ops.gemm_nt(o, arena.w(p + "o.w"), residual=h)
        if q8("gu"):
            a = ops.gemm_w8(h2, Q["gu.w"][0], Q["gu.w"][1], lnw=arena.w(p + "ln2"), eps=t.rms_eps, glu=True, a8=a8)
        elif fused:      # the [R, 2I] intermediate never reaches HBM
            a = ops.norm_gemm(h2, arena.w(p + "ln2"), t.rms_eps, arena.w(p + "gu.w"), glu=True)
        else:
            xn2, _, _ = ops.rmsnorm_fwd(h2, arena.w(p + "ln2"), t.rms_eps, need_rstd=False)
            a = ops.swiglu_fwd(ops.gemm_nt(xn2, arena.w(p + "gu.w")))
        if q8("down"):
            return ops.gemm_w8(a, Q["down.w"][0], Q["down.w"][1], residual=h2, a8=a8)
        if fused and self.R >= 16 and t.intermediate >= 8192:
            return ops.gemm_skinny_fixup(a, arena.w(p + "down.w"), residual=h2)
        return ops.gemm_nt(a, arena.w(p + "down.w"), residual=h2)

    def select(self, s, logits):
        roll, ops, cfg, buf, G = self.roll, self.ops, self.cfg, self.buf, self.roll.G
        logits = roll._penalized(buf, logits)
        if buf.greedy_op:
            ops.greedy_tokens(logits, buf.steps[s + 1:s + 2], buf.tokens, buf.finished, cfg.eos_token_id, cfg.pad_token_id, done_count=buf.done_count)
        for b, st in enumerate(() if buf.greedy_op else self.per):      # every prompt with its own seed and row slices
            ops.sample_tokens(logits[b * G:(b + 1) * G], roll.temperature, roll.top_k, st["seed"], buf.steps[s + 1:s + 2], st["tokens"],
                              st["finished"], cfg.eos_token_id, cfg.pad_token_id, roll.stop_at_eos, **roll._filter_kwargs(ops), **self.count_kw)
        roll._mark_drawn(buf, s + 1)
