"""One GRPO micro-step on device: vision tower once -> shared-prefix rollout -> policy / reference log-probs on the packed
sequence -> loss gradient -> hand-written backward.  Restates the tensor algebra of TimeR1_Trainer.compute_loss
(reference src/time_r1/rl/timer1_trainer.py:512-782) without the G-fold replication.

Host-side pieces that the reference also runs on the host (text decode, reward callbacks, group statistics on G floats)
stay in trainer.py; everything with a FLOP count lives here and goes through ops (HIP kernels).
"""

import numpy as np
import torch

from .model import Engine
from .positions import PackedLayout, rope_index
from .rollout import Rollout

I32 = torch.int32
F32 = torch.float32


class StepState:
    """Per-prompt device state handed between the phases of a micro-step.  Every field a phase hands over is declared here and is None until its
    phase has run (or when its option is off); callers - bench.py, the tests - may hang further attributes on a state."""

    def __init__(self):
        # prepare(): the prompt, its rope positions and the vision features
        self.P = self.grid = self.prompt_ids_host = self.prompt_ids = self.vid_rows = self.pos3_prompt = self.delta = None
        self.feats = self.vis_perm = self.vid_embeds = self.merger_ctx = None
        self.pixels = None                   # kept only while a training tower (or a replay of it) reads them again
        # rollout() / rollout_many(): the completions; prefill = the rollout's saved prompt activations and K/V, sample_logp = log-probs under the
        # sampling policy's logits (Rollout.track_logp), completion_ids_host = the tokens once a caller has copied them to the host
        self.layout = self.completion_ids = self.completion_ids_host = self.prefill = self.sample_logp = None
        # forward_logps(): the packed sequence, the saved contexts of the backward, the log-probs
        self.ids_packed = self.pos3 = self.cos = self.sin = self.masks = self.pred_rows = self.targets = self.perm = self.inv_perm = None
        self.llm_ctx = self.head_ctx = None
        self.logp = self.entropy = self.ref_logp = None
        # trim_completions: decode_steps = the decode steps the rollout enqueued for this prompt's batch; prefill_tail_from = the tail_from the rollout's prefill
        # ran with (it was decided on the untrimmed row count; the passes that repeat that prefill launch for launch read it here)
        # full_C = the configured completion length of a state that trim() has cut (None: not cut) - the width everything [G, C]-shaped keeps
        self.decode_steps = self.prefill_tail_from = self.full_C = None


class GRPOCore:
    def __init__(self, engine: Engine, ref_arena=None, num_generations=8, max_completion_length=200, beta=0.04, use_grpo=False,
                 temperature=1.0, top_k=50, seed=1234, rope_index_mode="hf4", stop_at_eos=False, reuse_prefill=True, greedy=False,
                 top_p=1.0, min_p=None, repetition_penalty=1.0, objective=None, entropy_coef=0.0, top_entropy_quantile=1.0, activation_recompute=None,
                 trim_completions=False):
        self.eng = engine
        # trim_completions (GRPOConfig.trim_completions): the sampled rollout ends once every row has drawn its EOS (Rollout.early_stop), and trim() cuts an
        # update's packed sequence to the columns some row still lives in.  False: neither exists for any call below.
        self.trim_completions = bool(trim_completions)
        # "none" | "mlp" (Engine.activation_recompute): what the update's forwards save for the backward; None keeps the engine's own setting
        if activation_recompute is not None:
            engine.set_activation_recompute(activation_recompute)
        # entropy_coef (verl's actor.entropy_coeff): the loss gains -entropy_coef * sum n H, H the per-token entropy of the policy and n the per-token normaliser of the
        # policy term (a positive coefficient rewards entropy).  top_entropy_quantile = rho < 1 (trl): only the live tokens whose entropy is at or above the
        # (1 - rho) quantile of this micro-step's live entropies carry the advantage term; KL, the normaliser and the bonus keep every live token.  trl selects
        # over the batch gathered across ranks, here the selection is per micro-step - one prompt's G completions on one rank - like loss_type="bnpo"'s normaliser.
        # At the defaults (0, 1) neither reaches any code below.
        self.entropy_coef = float(entropy_coef)
        self.top_entropy_quantile = 1.0 if top_entropy_quantile is None else float(top_entropy_quantile)
        missing = [n for n, on in (("logp_entropy_bwd", self.entropy_coef != 0.0), ("entropy_quantile_weight", self.top_entropy_quantile < 1.0))
                   if on and not hasattr(engine.ops, n)]
        if missing:
            raise NotImplementedError("entropy_coef = %g / top_entropy_quantile = %g: the %r backend has no %s"
                                      % (self.entropy_coef, self.top_entropy_quantile, getattr(engine.ops, "name", type(engine.ops).__name__), " / ".join(missing)))
        # None: the two loss branches of the reference (grpo_loss, grpo_loss_ratio on a replay).  A dict(norm, level, eps_low, eps_high, delta): every update
        # goes through grpo_policy_loss (trl's loss_type / importance_sampling_level / delta, rows without a live token) - policy_objective() below builds it
        self.objective = objective
        self.ops = engine.ops
        self.cfg = engine.cfg
        self.ref_arena = ref_arena
        self.G, self.C = int(num_generations), int(max_completion_length)
        self.beta, self.use_grpo = float(beta), bool(use_grpo)
        self.rope_index_mode = rope_index_mode
        self.second_per_grid_t = 1.0
        # The rollout's prefill IS the policy forward over the prompt rows (same weights inside an accumulation window): keep its
        # activations and run the update's policy forward over the G*C completion rows only.
        self.reuse_prefill = bool(reuse_prefill)
        self.roll = Rollout(engine, self.G, self.C, temperature, top_k, seed, stop_at_eos, greedy=greedy, top_p=top_p, min_p=min_p,
                            repetition_penalty=repetition_penalty)      # greedy: evaluation (argmax tokens, early stop)
        if self.trim_completions:
            self.roll.stop_at_eos = self.roll.early_stop = True
        if self.beta != 0.0 and ref_arena is None:
            raise ValueError("beta != 0 needs a reference-policy arena (reference timer1_trainer.py:295-307)")
        # algorithmic work of what was run since the trainer last read it (TimeR1_Trainer.log -> perf/* keys): bytes the decode steps must
        # stream (HBM-bound family) and FLOPs of the log-prob forwards + backward (MFMA-bound family); formulas in DESIGN.md section 4
        self.work = dict(decode_bytes=0.0, train_flops=0.0, decode_ms_events=0.0)

    # ------------------------------------------------------------------------------------------------------- work accounting
    def _llm_flops(self, rows, pairs):
        t = self.cfg.text
        lin = 2.0 * rows * (t.hidden * t.qkv_dim + t.q_dim * t.hidden + 3 * t.hidden * t.intermediate)
        att = 4.0 * pairs * t.head_dim * t.n_heads
        return t.n_layers * (lin + att)

    def _count_decode(self, states, steps=None):      # states: the prompt lengths P of one batched rollout; steps: the decode steps it enqueued (None: all C - 1)
        t = self.cfg.text
        wb = 1.0 if self.roll.weight_dtype in ("fp8", "fp8-mfma") else 2.0
        w_bytes = wb * (t.n_layers * (t.hidden * t.qkv_dim + t.q_dim * t.hidden + 3 * t.hidden * t.intermediate) + t.vocab_size * t.hidden)
        G, C = self.G, self.C
        n = C - 1 if steps is None else int(steps)
        kv = sum(sum(P + G * s for s in range(1, n + 1)) for P in states) * t.kv_dim * 2 * 2.0 * t.n_layers   # prefix once per prompt + every group's suffix
        self.work["decode_bytes"] += n * w_bytes + kv
        for e0, e1 in self.roll.decode_events:
            e1.synchronize()
            self.work["decode_ms_events"] += e0.elapsed_time(e1)
        self.roll.decode_events = []

    def _count_update(self, st, reused_prefill, with_ref=True):
        t = self.cfg.text
        P, G, C = st.P, self.G, st.layout.C      # the rows actually run (trim())
        M = P + G * C
        pairs_c = G * (C * P + C * (C + 1) / 2.0)
        pairs_all = P * (P + 1) / 2.0 + pairs_c
        head = 2.0 * G * C * t.vocab_size * t.hidden
        fl = (self._llm_flops(G * C, pairs_c) if reused_prefill else self._llm_flops(M, pairs_all)) + head        # policy forward
        if self.beta != 0.0 and with_ref:
            fl += self._llm_flops(M, pairs_all) + head                                                           # reference-policy forward (a replay reuses its log-probs)
        lin_all = self._llm_flops(M, 0.0)
        wg = 1.0 if self.eng.lora is not None else 2.0      # LoRA mode: no full-size weight gradients (the rank-r products are below 1 % of a dgrad and not counted)
        fl += wg * lin_all + 2.5 * (self._llm_flops(M, pairs_all) - lin_all) + wg * head                         # backward (dgrad + wgrad; flash backward = 5 products)
        self.work["train_flops"] += fl

    def _count_score(self, st):
        """forward_logps(score=True): the policy's and the reference's full-sequence forwards, no backward."""
        t = self.cfg.text
        P, G, C = st.P, self.G, st.layout.C
        pairs_all = P * (P + 1) / 2.0 + G * (C * P + C * (C + 1) / 2.0)
        one = self._llm_flops(P + G * C, pairs_all) + 2.0 * G * C * t.vocab_size * t.hidden
        self.work["train_flops"] += one * (2.0 if self.beta != 0.0 else 1.0)

    # ------------------------------------------------------------------------------------------------------- phase 1
    def prepare(self, input_ids, pixel_values_videos, video_grid_thw):
        """input_ids: 1-D ints (prompt with <|video_pad|> expanded); pixel_values_videos: float [N_v, patch_dim] as produced by
        the HF video processor (reference timer1_trainer.py:547-565); video_grid_thw: [(t, h, w)]."""
        ops, cfg, eng = self.ops, self.cfg, self.eng
        st = StepState()
        ids = np.asarray(input_ids, dtype=np.int64).reshape(-1)
        grid = [tuple(int(x) for x in g) for g in np.asarray(video_grid_thw).reshape(-1, 3)]
        st.P = self.last_P = int(ids.shape[0])
        st.grid = grid
        st.prompt_ids_host = ids
        st.prompt_ids = ops.tensor(ids.astype(np.int32), I32)
        vid_rows = np.nonzero(ids == cfg.video_token_id)[0].astype(np.int32)
        st.vid_rows = ops.tensor(vid_rows, I32)
        # Qwen2.5-VL spaces temporal ids by tokens_per_second * second_per_grid_t (modeling_qwen2_5_vl.py:1043); the reference's logprob
        # forwards omit second_per_grid_ts (timer1_trainer.py:452-457) -> 1 s per grid step, which is also what its default FPS=2 gives
        # the rollout (temporal_patch_size / fps = 1.0), so one rule serves both phases here.
        interval = int(cfg.tokens_per_second * self.second_per_grid_t) if cfg.vision.variant == "qwen2_5_vl" else 1
        st.pos3_prompt, st.delta = rope_index(ids, grid, cfg.video_token_id, cfg.image_token_id, cfg.vision.spatial_merge_size,
                                              mode=self.rope_index_mode, time_interval=interval)
        v = cfg.vision
        pix = torch.as_tensor(pixel_values_videos)
        n_vid_tokens = sum(t * h * w for t, h, w in grid) // v.merge_unit
        assert n_vid_tokens == vid_rows.shape[0], "video pad tokens (%d) != merged patches (%d)" % (vid_rows.shape[0], n_vid_tokens)
        if pix.dim() == 2 and pix.shape[1] == v.patch_dim_padded and pix.dtype == ops.act_dtype and pix.device == ops.device:
            pp = pix        # already staged on the device in the kernels' layout (K padded to a multiple of 64)
        else:
            assert pix.dim() == 2 and pix.shape[1] == v.patch_dim, pix.shape
            pp = ops.zeros(pix.shape[0], v.patch_dim_padded)
            pp[:, : v.patch_dim] = pix.to(pp.device).to(pp.dtype)
        st.feats, st.vis_perm = eng.vit_features(pp, grid)        # frozen blocks: once per prompt (reference: 3 x G times)
        st.pixels = pp if eng.params.train_vit else None          # fix_vit=False: the reference tower and the backward's recompute read them again
        # (LoRA mode: the merger is frozen, its backward never runs - nothing of it is kept)
        st.vid_embeds, st.merger_ctx = eng.merger_fwd(eng.params.train, st.feats, save=eng.lora is None, perm=st.vis_perm)
        return st

    # ------------------------------------------------------------------------------------------------------- phase 2
    def rollout(self, st):
        tokens, lay = self.roll.generate(self.eng.params.train, st.prompt_ids, st.vid_embeds, st.vid_rows, st.pos3_prompt, st.delta,
                                         save_prefill=self.reuse_prefill)
        st.layout = lay
        st.completion_ids = tokens        # int32 [G, C] on device
        st.prefill = self.roll.last_prefill[0] if self.reuse_prefill else None
        st.sample_logp = self.roll.last_sample_logp[0] if self.roll.last_sample_logp is not None else None
        st.decode_steps = self.roll.last_steps_run
        self._pending_decode = (getattr(self, "_pending_decode", []) + [([st.P], st.decode_steps)])[-64:]
        return tokens

    def rollout_many(self, states, save_prefill=None, slot0=0):
        """Decode the prompts of one accumulation window together (weights are constant inside it): every weight byte streamed
        from HBM serves len(states)*G rows. Sampling streams stay per prompt, so tokens equal the one-by-one rollout's.
        save_prefill: one flag per state - a generation cycle keeps the prefill of its first window's prompts only - with slot0 the number of prefills the
        cycle's earlier groups saved (Rollout.generate_many); None = every state's, where reuse_prefill is on."""
        saves = [self.reuse_prefill] * len(states) if save_prefill is None else [bool(x) for x in save_prefill]
        kw = dict(save_prefill=self.reuse_prefill) if save_prefill is None else dict(save_prefill=saves, slot0=slot0)
        outs = self.roll.generate_many(self.eng.params.train, [(st.prompt_ids, st.vid_embeds, st.vid_rows, st.pos3_prompt, st.delta) for st in states], **kw)
        for b, (st, (tokens, lay)) in enumerate(zip(states, outs)):
            st.layout, st.completion_ids = lay, tokens
            st.prefill = self.roll.last_prefill[b] if saves[b] else None
            st.sample_logp = self.roll.last_sample_logp[b] if self.roll.last_sample_logp is not None else None
            st.decode_steps = self.roll.last_steps_run
        self._pending_decode = (getattr(self, "_pending_decode", []) + [([st.P for st in states], self.roll.last_steps_run)])[-64:]
        return [st.completion_ids for st in states]

    def drain_work(self):
        """-> the work counters since the last call (decode events are resolved here, i.e. when the trainer logs - never inside a step)."""
        for states, steps in getattr(self, "_pending_decode", []):
            self._count_decode(states, steps)
        self._pending_decode = []
        w, self.work = self.work, dict.fromkeys(self.work, 0.0)
        return w

    # ------------------------------------------------------------------------------------------------------- phase 3
    TRIM_FLOOR = 8      # no update runs on fewer completion columns than this (the shapes the kernels are tested on)

    def trim(self, st, completion_ids_host, eos_token_id):
        """trim_completions: cut the state to the live columns, ahead of forward_logps.  L = the largest (first EOS index + 1) over the rows (C for a row
        without EOS), Ct = min(C, max(TRIM_FLOOR, L)).  Ct < C: the layout becomes PackedLayout(P, G, Ct) and completion_ids the contiguous [:, :Ct], so every
        pass that runs the model - policy and reference forward, head, backward, every replay - sees P + G*Ct rows.  The columns that leave lie behind every
        row's EOS: their mask is 0 (eos_mask).  What is [G, C]-shaped stays so (_to_gc pads with 0), the loss kernels and their normalisers with it; only
        dlogp[:, :Ct] enters the backward.  The rollout's saved prefill belongs to the untrimmed layout: its buffers, stash and K/V cache are used as
        [: P + G*Ct] views and its tail_from travels in the saved context (forward_logps).  Callers keep the host's full [G, C] rows for rewards and
        decoding - the reference decodes what follows the EOS too.  -> Ct"""
        ids = np.asarray(completion_ids_host)
        G, C = ids.shape
        is_eos = ids == eos_token_id
        L = int(np.where(is_eos.any(1), is_eos.argmax(1) + 1, C).max())
        Ct = min(C, max(self.TRIM_FLOOR, L))
        if Ct < C:
            st.full_C = C
            st.layout = PackedLayout(st.P, G, Ct)
            st.completion_ids = st.completion_ids[:, :Ct].contiguous()
        return Ct

    def _packed_inputs(self, st):
        ops, lay = self.ops, st.layout
        comp = st.completion_ids
        st.ids_packed = torch.cat([st.prompt_ids, comp.reshape(-1)])
        st.pos3 = ops.tensor(lay.positions(st.pos3_prompt, st.delta), I32)
        t = self.cfg.text
        st.cos, st.sin = ops.mrope_table(st.pos3, t.head_dim, t.mrope_section, t.rope_theta)
        st.masks = [ops.tensor(a, I32) for a in lay.masks()]
        st.pred_rows = ops.tensor(lay.pred_rows(), I32)
        G, C = lay.G, lay.C
        st.targets = torch.cat([comp[:, 0], comp[:, 1:].reshape(-1)]).contiguous()
        # permutation between [G, C] order and pred_rows order
        perm = np.concatenate([np.arange(G) * C, (np.arange(G)[:, None] * C + 1 + np.arange(C - 1)[None, :]).reshape(-1)])
        st.perm = torch.as_tensor(perm, dtype=torch.long, device=comp.device)          # pred order -> flat (g, s) index
        st.inv_perm = torch.empty_like(st.perm)
        st.inv_perm[st.perm] = torch.arange(G * C, device=comp.device)

    def _to_gc(self, st, x_pred_order):
        """pred_rows order -> [G, C]; a trimmed state keeps its configured C: the columns >= layout.C hold 0 (their mask is 0)."""
        x = x_pred_order[st.inv_perm].view(st.layout.G, st.layout.C)
        if st.full_C is None:
            return x
        out = torch.zeros(st.layout.G, st.full_C, dtype=x.dtype, device=x.device)
        out[:, :st.layout.C] = x
        return out

    def forward_logps(self, st, replay=False, score=False):
        """Policy log-probs / entropy (activations saved for backward) and reference log-probs (no grad).
        score=True: the scoring form for a window whose update comes after the weights have moved (GRPOConfig.steps_per_generation): the policy forward
        saves nothing and no backward follows it.  It takes the launches the replay's forward takes - the whole packed sequence in one decoder pass, the head
        in its saved form - so on unmoved weights st.logp agrees with a replay's as closely as a replay agrees with a first pass; the reference forward is
        the first pass's.  The vision embeddings are prepare()'s (same weights); what only a backward would read is released.
        replay=True: a further update on the SAME rollout after the weights have moved (GRPOConfig.num_iterations > 1).  The vision merger (and the tower,
        when it trains) runs again on the kept features / pixels, the decoder takes the full-sequence path - the rollout's saved prefill belongs to the old
        weights - and the reference-policy forward is skipped: its weights are frozen, so st.ref_logp of the first pass still holds."""
        eng, ops = self.eng, self.ops
        tr = eng.params.train
        if score:
            return self._score_logps(st)
        if replay:
            if eng.params.train_vit:
                st.feats = eng.vit_features(st.pixels, st.grid)[0]
            st.vid_embeds, st.merger_ctx = eng.merger_fwd(tr, st.feats, save=eng.lora is None, perm=st.vis_perm)
            st.prefill = None
        else:
            self._packed_inputs(st)
        pf = st.prefill
        split = pf is not None and pf[0] is not None
        self._count_update(st, split, with_ref=not replay)
        if split:
            # continuation: only the G*C completion rows; the prompt rows' activations and K/V come from the rollout's prefill
            P, M = st.P, st.layout.M
            pctx, kv = pf
            st.prefill_tail_from = int(pctx.get("tail_from", 0) or 0) or None      # (= Engine.tail_rows_from(P, the rollout's M): None or P - 1)
            if pctx.get("stash"):            # large sequences: this prompt's prefill rows were parked; the one full buffer set is free now
                pctx = eng.unstash_ctx(pctx, P, M)
            hc = ops.gather_rows(tr.w("embed"), st.ids_packed[P:].contiguous())
            cmask = [m[P:].contiguous() for m in st.masks]
            hLc, cctx = eng.llm_fwd(tr, hc, st.cos[P:].contiguous(), st.sin[P:].contiguous(), cmask, save=True, kv_cache=kv, row0=P,
                                    bufs=pctx.get("bufs"))
            st.llm_ctx = eng.merge_ctx(pctx, cctx, kv, st.masks, st.cos, st.sin, M)
            # the head only needs the last prompt row (it predicts every group's first completion token) and the completion rows
            hL = ops.zeros(M, hLc.shape[1])
            hL[P:] = hLc
            hL[P - 1:P] = pctx["h_last"][P - 1:P]
            st.prefill = None
        else:
            h0 = eng.embed(tr, st.ids_packed, st.vid_embeds, st.vid_rows)
            # a replay writes its saved activations into the engine's slot-0 buffer set (free: every earlier backward of the window has been enqueued), like the
            # prefill + continuation pair of the first pass - no second set beside the pooled one
            bufs = eng.alloc_ctx_bufs(st.layout.M, slot=0) if replay else None
            hL, st.llm_ctx = eng.llm_fwd(tr, h0, st.cos, st.sin, st.masks, save=True, bufs=bufs,
                                         tail_from=eng.tail_rows_from(st.P, st.layout.M))    # the head reads rows >= P - 1 only (pred_rows)
        logp, ent, st.head_ctx = eng.head_fwd(tr, hL, st.pred_rows, st.targets, save=True)
        st.logp = self._to_gc(st, logp).contiguous()
        st.entropy = self._to_gc(st, ent).contiguous()
        if replay:
            return
        self._ref_logps(st, split)

    def _ref_logps(self, st, split):
        """The reference policy's log-probs of the state's packed sequence (no grad); split: the policy forward ran as prefill + continuation."""
        eng = self.eng
        st.ref_logp = None
        if self.beta != 0.0:
            ra = self.ref_arena
            # fix_vit=False: the reference policy's features come from the INITIAL tower (its copy in the reference arena, reference :295-307)
            ref_feats = eng.vit_features(st.pixels, st.grid, arena=ra)[0] if eng.params.train_vit else st.feats
            ref_vid, _ = eng.merger_fwd(ra, ref_feats, save=False, perm=st.vis_perm)
            if split and eng.lora is not None:
                hLr = self._ref_split_fwd(st, ra, ref_vid)
            else:
                h0r = eng.embed(ra, st.ids_packed, ref_vid, st.vid_rows)
                hLr, _ = eng.llm_fwd(ra, h0r, st.cos, st.sin, st.masks, save=False, tail_from=eng.tail_rows_from(st.P, st.layout.M))
            rlogp, _, _ = eng.head_fwd(ra, hLr, st.pred_rows, st.targets, save=False, **({"as_saved": True} if eng.lora is not None else {}))
            st.ref_logp = self._to_gc(st, rlogp).contiguous()

    def _score_logps(self, st):
        """forward_logps(score=True)."""
        eng = self.eng
        tr = eng.params.train
        self._packed_inputs(st)
        self._count_score(st)
        h0 = eng.embed(tr, st.ids_packed, st.vid_embeds, st.vid_rows)
        hL, _ = eng.llm_fwd(tr, h0, st.cos, st.sin, st.masks, save=False, tail_from=eng.tail_rows_from(st.P, st.layout.M))
        logp, ent, _ = eng.head_fwd(tr, hL, st.pred_rows, st.targets, save=False, as_saved=True)
        st.logp = self._to_gc(st, logp).contiguous()
        st.entropy = self._to_gc(st, ent).contiguous()
        st.vid_embeds = st.merger_ctx = st.prefill = None      # the replay runs the merger again, on the weights of its own step
        self._ref_logps(st, False)

    def _ref_split_fwd(self, st, ra, ref_vid):
        """LoRA mode: the reference policy's decoder pass in the policy's own two launches - the prompt's P rows as the rollout's prefill runs them, then the
        G*C completion rows over a K/V cache - instead of one pass over all P + G*C rows.  The work is the same; the point is the bits: a GEMM's tile and
        its summation order follow the row count, so the one-pass form gives log-probs that differ from the policy's in a last bf16 place even on equal
        weights (measured on tiny_test_25: 12 of 32, step-0 KL 5.6e-8).  Under peft the reference IS the policy with its adapters switched off - one code
        path - and KL is exactly 0 until the adapters move; here the base copy takes the same path as the merged weights, launch for launch, for that.
        The reference's cache (K, and V row-major or transposed as the attention kernel of this head dim reads it) is kept between calls: at 7B and
        5.1k rows 0.29 GB.  Full-parameter training keeps the one-pass form: its reference is a model of its own, as the reference trainer's is."""
        eng, ops, t, lay = self.eng, self.ops, self.cfg.text, st.layout
        P, M = st.P, lay.M
        kv, vc = self._ref_cache(lay.S_cap)
        pos_p = ops.tensor(np.ascontiguousarray(st.pos3_prompt.astype(np.int32)), I32)
        cos_p, sin_p = ops.mrope_table(pos_p, t.head_dim, t.mrope_section, t.rope_theta)
        h = eng.embed(ra, st.prompt_ids, ref_vid, st.vid_rows)
        # tail_from: the decision the rollout's prefill took (on its own, untrimmed row count), not a new one on this layout's M
        hp, _ = eng.llm_fwd(ra, h, cos_p, sin_p, [ops.tensor(a, I32) for a in lay.prompt_masks()], save=False, kv_cache=kv, v_cache=vc,
                            tail_from=st.prefill_tail_from)
        hc = ops.gather_rows(ra.w("embed"), st.ids_packed[P:].contiguous())
        hLc, _ = eng.llm_fwd(ra, hc, st.cos[P:].contiguous(), st.sin[P:].contiguous(), [m[P:].contiguous() for m in st.masks], save=False, kv_cache=kv,
                             v_cache=vc, row0=P)
        hL = ops.zeros(M, hLc.shape[1])
        hL[P:] = hLc
        hL[P - 1:P] = hp[P - 1:P]
        return hL

    def _ref_cache(self, s_cap):
        """-> (per layer (K [cap, kv_dim], V^T [kv_dim, cap] or None), per layer V [cap, kv_dim] or None), cap >= s_cap, kept while it is large enough."""
        eng, ops, t = self.eng, self.ops, self.cfg.text
        c = getattr(self, "_ref_kv", None)
        if c is None or c[0] < s_cap:
            self._ref_kv = None      # release before re-allocating
            cap = (s_cap + 511) // 512 * 512
            rows = getattr(ops, "attn_fwd_rows_ok", lambda *a, **kw: False)(t.head_dim)
            k = [ops.zeros(cap, t.kv_dim) for _ in range(t.n_layers)]
            vt = [None if rows else ops.zeros(t.kv_dim, cap) for _ in range(t.n_layers)]
            c = self._ref_kv = (cap, list(zip(k, vt)), [ops.zeros(cap, t.kv_dim) for _ in range(t.n_layers)] if rows else None)
        return c[1], c[2]

    # ------------------------------------------------------------------------------------------------------- phase 4
    def loss_backward(self, st, completion_mask, advantages, grad_scale=1.0, grad_sync=None, tok_weight=None, old_logp=None, eps=(0.2, 0.2),
                      keep_pixels=False):
        """completion_mask int32 [G, C], advantages fp32 [G] (device). Accumulates grads into the trainable arena.
        grad_sync: a dist.GradSync in its begin() state when this is the LAST micro-step of the accumulation window - parameter ranges
        are handed to the all-reduce as soon as their gradients are final, overlapping the exchange with the rest of the backward.
        old_logp (fp32 [G, C]): the log-probs of the policy that drew the completions, for a replayed update (forward_logps(replay=True)): the loss is then
        the ratio kernel's (rho = exp(logp - old_logp) clipped to [1 - eps[0], 1 + eps[1]], tok_weight inside the kernel) and out8 is returned in place of out3.
        With self.objective set, first pass and replays alike run grpo_policy_loss with the objective's clip range (`eps` is the ratio kernel's) and return out8.
        keep_pixels: further replays of this state follow (the training tower's backward reads st.pixels again).
        Returns (out3 = [loss, mean kl, sum mask] - or the kernel's out8, as above -, row_len [G]) as device tensors.  Three jobs, one method each: _loss_grad,
        _entropy_bonus, _backward."""
        if self.top_entropy_quantile < 1.0:
            # the entropy of THIS forward (a replay selects on its own, as trl recomputes the mask in every compute_loss); it multiplies with an importance cap
            sel, _ = self.ops.entropy_quantile_weight(st.entropy, completion_mask, self.top_entropy_quantile)
            tok_weight = sel if tok_weight is None else tok_weight.to(torch.float32) * sel
        dlogp, out3, row_len = self._loss_grad(st, completion_mask, advantages, grad_scale, tok_weight, old_logp, eps)
        dent = None
        if self.entropy_coef != 0.0:
            out3, dent = self._entropy_bonus(st, completion_mask, out3, row_len, grad_scale)
        self._backward(st, dlogp, dent, grad_sync, keep_pixels)
        return out3, row_len

    def _normaliser(self, st, out3, row_len):
        """The per-token normaliser of the policy term on this path, from the kernel's own counts on the device: a live token weighs 1 / (d * k) -> (d, k).
        Row mean (use_grpo, loss_type "grpo"): d = the row's live tokens, k = G; token mean: d = all live tokens; "dr_grpo": k = G * C.  A row (or a grid)
        without a live token has d = 1 and no live token to weigh.  The two users divide in their own order, (m / d) / k and m / (d * k): the roundings differ."""
        norm = self.objective["norm"] if self.objective is not None else (0 if self.use_grpo else 1)
        if norm == 0:
            return row_len.reshape(-1, 1).to(F32).clamp(min=1.0), float(st.layout.G)
        if norm == 1:
            return out3[2].to(F32).clamp(min=1.0), 1.0
        return 1.0, float(st.layout.G) * float(st.full_C or st.layout.C)      # (the configured C, as loss.hip divides: a trimmed layout's C is smaller)

    def _loss_grad(self, st, completion_mask, advantages, grad_scale, tok_weight, old_logp, eps):
        """The loss entry point of this path and what tok_weight means on it -> (dlogp [G, C], out3 or out8, row_len [G])."""
        ops = self.ops
        tw = None if tok_weight is None else tok_weight.to(torch.float32).contiguous()
        if self.objective is not None:
            # the objective family: first pass (old_logp None: ratio 1, tok_weight inside the kernel) and replays alike; out8 is returned in place of out3
            o = self.objective
            dlogp, out3, row_len, _ = ops.grpo_policy_loss(st.logp, old_logp, st.ref_logp, completion_mask, advantages, self.beta, o["norm"], o["level"],
                                                           o["eps_low"], o["eps_high"], o["delta"], grad_scale, tok_weight=tw)
        elif old_logp is not None:
            dlogp, out3, row_len, _ = ops.grpo_loss_ratio(st.logp, old_logp, st.ref_logp, completion_mask, advantages, self.beta, self.use_grpo,
                                                          float(eps[0]), float(eps[1]), grad_scale, tok_weight=tw)
        else:
            dlogp, out3, row_len, _ = ops.grpo_loss(st.logp, st.ref_logp, completion_mask, advantages, self.beta, self.use_grpo, grad_scale)
            if tw is not None:
                # optional truncated importance weight rho[g, t] (a constant) on the advantage term, for completions drawn from a quantised sampling
                # policy: l = -rho * A + beta * kl = l_plain + (1 - rho) * A, same normalisation as the kernel (which takes no tok_weight).  None (the
                # default) leaves the reference algebra untouched - this branch is then not executed at all.
                d, k = self._normaliser(st, out3, row_len)
                corr = (1.0 - tw) * advantages.reshape(-1, 1).to(torch.float32) * (completion_mask.to(torch.float32) / d / k)
                dlogp = dlogp + (corr * float(grad_scale)).to(dlogp.dtype)
                out3 = out3.clone()
                out3[0] = out3[0] + corr.sum().to(out3.dtype)
        return dlogp, out3, row_len

    def _entropy_bonus(self, st, completion_mask, out3, row_len, grad_scale):
        """loss - entropy_coef * sum n H over ALL live tokens (the top-entropy selection does not apply), n = the normaliser of the policy term on this path; a
        row (or a grid) without a live token contributes 0 -> (out3 with the bonus in its loss, the gradient at the entropy [G, C])."""
        live = completion_mask != 0
        d, k = self._normaliser(st, out3, row_len)
        n = live.to(torch.float32) / (d * k)
        H = torch.where(live, st.entropy.to(torch.float32), torch.zeros_like(n))
        out3 = out3.clone()
        out3[0] = out3[0] - (self.entropy_coef * (n * H).sum()).to(out3.dtype)
        return out3, (-self.entropy_coef * float(grad_scale)) * n

    def _backward(self, st, dlogp, dent, grad_sync, keep_pixels):
        """The backward chain from the gradients at the log-probs (and at the entropy, or None) [G, C] into the trainable arena."""
        eng = self.eng
        tr = eng.params.train
        hook = None
        if grad_sync is not None and grad_sync.active and eng.lora is None:      # (LoRA mode: the adapters' small exchange happens in the optimizer step)
            hook = lambda i: grad_sync.ready(*tr.range_of("l%d." % i))
        Cr = st.layout.C      # the columns the model ran on (trim()): gradients behind them are zero and stay out
        to_pred = lambda x: (x if x.shape[1] == Cr else x[:, :Cr]).reshape(-1)[st.perm].contiguous()
        dh = eng.head_bwd(st.head_ctx, to_pred(dlogp), st.layout.G, dent=None if dent is None else to_pred(dent))
        if hook is not None and not self.cfg.text.tie_word_embeddings:
            grad_sync.ready(*tr.range_of("norm"))          # final norm + untied lm_head gradients are complete after the head backward
            grad_sync.ready(*tr.range_of("lm_head"))
        dh0 = eng.llm_bwd(st.llm_ctx, dh, on_layer_done=hook)
        dfeats = None
        if eng.lora is None:      # (LoRA mode: embedding, merger and vision tower are frozen, as under peft - the backward ends at the decoder's input)
            ids_g = st.ids_packed.clone()
            ids_g[st.vid_rows.long()] = -1
            dvid = eng.embed_bwd(dh0, ids_g, st.vid_rows)
            dfeats = eng.merger_bwd(st.merger_ctx, dvid)
        st.llm_ctx = st.head_ctx = st.merger_ctx = None
        if dfeats is not None:
            # fix_vit=False: the tower's activations are recomputed here, one prompt at a time (prepare() keeps none), then its backward runs.
            # Its gradient ranges are handed to the exchange by grad_sync.finish() (GradSync / ShardSync cover every range nobody announced).
            _, _, vctx = eng.vit_features(st.pixels, st.grid, save=True)
            eng.vit_bwd(vctx, dfeats)
        if not keep_pixels:
            st.pixels = None


def eos_mask(completion_ids, eos_token_id):
    """completion_mask[g, t] = 1 for t <= first EOS (EOS kept), all ones when there is none (reference timer1_trainer.py:580-590).
    completion_ids: numpy int [G, C] -> numpy int32 [G, C]."""
    G, C = completion_ids.shape
    is_eos = completion_ids == eos_token_id
    eos_idx = np.full(G, C, dtype=np.int64)
    has = is_eos.any(1)
    eos_idx[has] = is_eos.argmax(1)[has]
    return (np.arange(C)[None, :] <= eos_idx[:, None]).astype(np.int32)


def truncation_mask(completion_ids, eos_token_id, mask):
    """trl's mask_truncated_completions: a completion that holds no EOS among its C tokens ran into the length limit; its mask row is zeroed, so it leaves
    the loss.  completion_ids numpy int [G, C], mask numpy int32 [G, C] (eos_mask) -> (mask with those rows zeroed, truncated bool [G])."""
    truncated = ~(completion_ids == eos_token_id).any(1)
    return (mask * (~truncated)[:, None]).astype(np.int32), truncated


NO_CLIP_EPS = (1.0, 3.0e38)     # clip range [0, 3e38]: a ratio is positive and finite in fp32, so neither side of the clamp is ever taken


def policy_objective(use_grpo=False, loss_type=None, importance_sampling_level="token", delta=None, mask_truncated_completions=False,
                     epsilon_low=0.2, epsilon_high=0.2):
    """GRPOCore's `objective` for the settings of GRPOConfig: None while every one of them is at its default (the reference's two branches run unchanged),
    else the arguments of grpo_policy_loss.  loss_type None keeps the branch's own normaliser: the row mean for use_grpo, the token mean for the clip branch.
    use_grpo has no clip; it gets here only through mask_truncated_completions and then runs with NO_CLIP_EPS."""
    if loss_type is None and importance_sampling_level == "token" and delta is None and not mask_truncated_completions:
        return None
    from .ops import GRPO_LEVELS, GRPO_NORM_MODES, LOSS_TYPE_NORM
    norm = LOSS_TYPE_NORM[loss_type] if loss_type is not None else GRPO_NORM_MODES["row" if use_grpo else "token"]
    lo, hi = NO_CLIP_EPS if use_grpo else (float(epsilon_low), float(epsilon_high))
    return dict(norm=norm, level=GRPO_LEVELS[importance_sampling_level], eps_low=lo, eps_high=hi, delta=float(delta) if delta else 0.0)


def group_advantages(rewards_per_func, num_generations, scale=True):
    """rewards_per_func: torch fp32 [B*G, n_funcs] -> (rewards, advantages, std) exactly as reference timer1_trainer.py:700-712
    (sum over funcs, per-group mean, UNBIASED std, eps 1e-4).  scale=False (trl's scale_rewards=False, Dr. GRPO): advantages = rewards - group mean, not
    divided by the group's std; the returned std is the same."""
    rewards = rewards_per_func.sum(dim=1)
    mean = rewards.view(-1, num_generations).mean(dim=1).repeat_interleave(num_generations, dim=0)
    std = rewards.view(-1, num_generations).std(dim=1).repeat_interleave(num_generations, dim=0)
    adv = (rewards - mean) / (std + 1e-4) if scale else rewards - mean
    return rewards, adv, std
