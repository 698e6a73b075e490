"""Drop-in trainer boundary: `TimeR1_Trainer` / `TimeR1_Trainer_ft` with the reference's constructor, `train()`, `compute_loss()`,
`log()`, `save_model()` and callback protocol (reference src/time_r1/rl/timer1_trainer.py:184-438, :512-793; ft variant
timer1_trainer_ft.py:551-563, :670-691, :789-842; wiring main.py:573-625), driving the MI355X engine instead of
transformers.Trainer + trl + DeepSpeed (all absent offline, and replaced here by design).

What is kept identical for the caller: constructor signature, dataset-row schema, identity collation (one prompt per device per
micro-step, reference fact "only inputs[0]" :524/:548-551), processor calls (apply_chat_template / __call__ / batch_decode),
reward callback protocol (prompts=, completions=, **row columns x G), metric keys, `state.global_step` / `trainer_state.json` /
`checkpoint-N` layout used by main.py's resume arithmetic (:589-618), TrainerCallback hooks (on_epoch_end etc., main.py:520-539).
What differs by construction: compute_loss also runs the backward (there is no autograd graph to return) and returns the loss value.
"""
import dataclasses
import json
import math
import os
import time
import types
from collections import defaultdict
from typing import Any, Callable, List, Optional, Union

import numpy as np
import torch

from .config import ModelConfig, PRESETS
from .dist import DataParallel, shard_world_ok
from .grpo import GRPOCore, eos_mask, group_advantages, policy_objective, truncation_mask
from .model import Engine
from .optim import AdamWFlat
from .params import ModelParams
from . import vision_process as VP

SYSTEM_PROMPT = "You are a video analysis expert."

# Prompt wording is data the policy was trained with; kept verbatim (reference timer1_trainer.py:63-67, timer1_trainer_ft.py:61-85).
QUESTION_TEMPLATE_TG_v1 = """To accurately pinpoint the event "[EVENT]" in the video, determine the precise time period of the event.

Output your thought process within the <think> </think> tags, including analysis with either specific time ranges (xx.xx to xx.xx) in <timestep> </timestep> tags.

Then, provide the start and end times (in seconds, precise to two decimal places) in the format "start time to end time" within the <answer> </answer> tags. For example: "12.54 to 17.83"."""

QUESTION_TEMPLATE_TG_v2 = """To accurately pinpoint the event "[EVENT]" in the video, determine the precise time period of the event.

Provide the start and end times (in seconds, precise to two decimal places) in the format "start time to end time" within the <answer> </answer> tags. For example: "12.54 to 17.83"."""

QUESTION_TEMPLATE_TG_v3 = """Carefully analyze the video content to determine the precise time period during which "[EVENT]" occurs.  Within the `<think>` tags, provide a detailed description of your thought process, following the format below:
```
<think>
Step-by-step Analysis:
<timestep>Time period 1 (start time to end time)</timestep>: Describe the video content within this time period and determine if it is related to "[EVENT]".
<timestep>Time period 2 (start time to end time)</timestep>: Describe the video content within this time period and determine if it is related to "[EVENT]".
Based on the above analysis, state the precise time period during which "[EVENT]" occurs.
</think>
```
Finally, in the `<answer>` tags, provide the start and end times of "[EVENT]" in the format "start time to end time" (in seconds, precise to two decimal places). For example: "12.54 to 17.83".
```
<answer>
start time to end time
</answer>
```"""

_TEMPLATES = {"v1": QUESTION_TEMPLATE_TG_v1, "v2": QUESTION_TEMPLATE_TG_v2, "v3": QUESTION_TEMPLATE_TG_v3}


def generation_config_dict(cfg, args):
    """What save_model writes as generation_config.json; top_p / min_p / repetition_penalty only when they are not the defaults."""
    d = {"eos_token_id": cfg.eos_token_id, "pad_token_id": cfg.pad_token_id, "do_sample": True, "temperature": float(getattr(args, "temperature", 1.0))}
    top_p, min_p, rep = getattr(args, "top_p", 1.0), getattr(args, "min_p", None), getattr(args, "repetition_penalty", 1.0)
    if top_p is not None and float(top_p) != 1.0:
        d["top_p"] = float(top_p)
    if min_p is not None and float(min_p) != 0.0:
        d["min_p"] = float(min_p)
    if rep is not None and float(rep) != 1.0:
        d["repetition_penalty"] = float(rep)
    return d


def generation_windows(a, num_iterations=None, loader_windows=None):
    """steps_per_generation of the arguments `a` against the settings it cannot work with -> k, the accumulation windows one rollout serves (1 for None).
    Every rule raises ValueError with the values it objects to.  num_iterations: the trainer's own (default: the arguments'); loader_windows: the windows
    of one epoch, once train() knows them."""
    spg = getattr(a, "steps_per_generation", None)
    if spg is None:
        return 1
    try:
        whole = not isinstance(spg, bool) and int(spg) == float(spg) and int(spg) >= 1
    except (TypeError, ValueError, OverflowError):
        whole = False
    if not whole:
        raise ValueError("steps_per_generation must be None or an integer >= 1, got %r" % (spg,))
    spg, ga = int(spg), max(1, int(a.gradient_accumulation_steps))
    if spg % ga != 0:
        raise ValueError("steps_per_generation (%d) must be a multiple of gradient_accumulation_steps (%d): a rollout serves whole accumulation windows, and "
                         "generating more than once per window is not offered" % (spg, ga))
    k = spg // ga
    if k == 1:
        return 1
    mu = int(getattr(a, "num_iterations", 1) if num_iterations is None else num_iterations)
    if getattr(a, "use_grpo", False):
        raise ValueError("steps_per_generation = %d with gradient_accumulation_steps = %d updates %d window(s) on completions of an older policy, and use_grpo=True "
                         "has no clip on the probability ratio: it needs use_grpo=False" % (spg, ga, k - 1))
    if not getattr(a, "rollout_batching", True):
        raise ValueError("steps_per_generation = %d with gradient_accumulation_steps = %d decodes %d windows together: it needs rollout_batching=True" % (spg, ga, k))
    if getattr(a, "save_strategy", "no") == "steps" and a.save_steps and int(a.save_steps) % (k * mu) != 0:
        raise ValueError("save_steps (%d) must be a multiple of steps_per_generation / gradient_accumulation_steps x num_iterations = %d x %d = %d: checkpoints "
                         "are written at the end of a generation cycle only" % (a.save_steps, k, mu, k * mu))
    if getattr(a, "sync_ref_model", False) and int(a.ref_model_sync_steps) % (k * mu) != 0:
        raise ValueError("ref_model_sync_steps (%d) must be a multiple of steps_per_generation / gradient_accumulation_steps x num_iterations = %d x %d = %d: the "
                         "reference moves at the end of a generation cycle only" % (a.ref_model_sync_steps, k, mu, k * mu))
    if loader_windows is not None and k > loader_windows:
        raise ValueError("steps_per_generation = %d is %d accumulation windows of %d micro-steps, and an epoch holds %d: an epoch shorter than a generation cycle"
                         % (spg, k, ga, loader_windows))
    return k


@dataclasses.dataclass
class GRPOConfig:
    """The training arguments the reference reads (trl.GRPOConfig + main.py:44-70 MY_GRPOConfig), as a plain dataclass."""
    output_dir: str = "timer1-GRPO"
    # GRPO
    num_generations: int = 8
    max_prompt_length: int = 512            # accepted, never enforced (reference quirk)
    max_completion_length: int = 256
    temperature: float = 0.9
    top_k: Optional[int] = 50               # transformers 4.51 GenerationConfig default
    top_p: float = 1.0                      # nucleus filter behind top-k (GenerationConfig.top_p / trl.GRPOConfig.top_p / vLLM SamplingParams.top_p); 1 = off
    min_p: Optional[float] = None           # keep tokens with p >= min_p * p_max (GenerationConfig.min_p / trl.GRPOConfig.min_p); None or 0 = off
    repetition_penalty: float = 1.0         # logits of tokens in the prompt or already drawn: x / penalty (x > 0), x * penalty (x < 0); 1 = off

    def __post_init__(self):
        self.top_p = 1.0 if self.top_p is None else float(self.top_p)
        self.min_p = None if self.min_p is None else float(self.min_p)
        self.repetition_penalty = 1.0 if self.repetition_penalty is None else float(self.repetition_penalty)
        if not 0.0 < self.top_p <= 1.0:
            raise ValueError("top_p must be in (0, 1], got %r" % (self.top_p,))
        self.trim_completions = bool(self.trim_completions)
        if self.trim_completions:
            self.stop_at_eos = True      # trimming is about rows that END: a finished row is padded, and the rollout stops once every row is
        if self.min_p is not None and not 0.0 <= self.min_p <= 1.0:
            raise ValueError("min_p must be None or in [0, 1], got %r" % (self.min_p,))
        if not 0.0 < self.repetition_penalty < float("inf"):
            raise ValueError("repetition_penalty must be a positive number, got %r" % (self.repetition_penalty,))
        if int(self.num_iterations) != self.num_iterations or int(self.num_iterations) < 1:
            raise ValueError("num_iterations must be an integer >= 1, got %r" % (self.num_iterations,))
        self.num_iterations = int(self.num_iterations)
        self.epsilon_low = float(self.epsilon_low)
        if not 0.0 < self.epsilon_low < 1.0:
            raise ValueError("epsilon_low must be in (0, 1), got %r" % (self.epsilon_low,))
        if self.epsilon_high is not None:
            self.epsilon_high = float(self.epsilon_high)
            if not 0.0 < self.epsilon_high < float("inf"):
                raise ValueError("epsilon_high must be None or a positive number, got %r" % (self.epsilon_high,))
        if self.loss_type is not None and self.loss_type not in ("grpo", "bnpo", "dr_grpo"):
            raise ValueError('loss_type must be None, "grpo", "bnpo" or "dr_grpo", got %r (trl\'s "dapo" normalises over the whole accumulated batch across '
                             'ranks, which one micro-step\'s kernel cannot see: out of scope)' % (self.loss_type,))
        if self.loss_type is not None and self.use_grpo:
            raise ValueError("loss_type=%r selects a clipped objective and use_grpo=True the unclipped one: set one of the two" % (self.loss_type,))
        if self.importance_sampling_level not in ("token", "sequence"):
            raise ValueError('importance_sampling_level must be "token" or "sequence", got %r' % (self.importance_sampling_level,))
        if self.delta is not None:
            self.delta = float(self.delta)
            top = 1.0 + (self.epsilon_low if self.epsilon_high is None else self.epsilon_high)
            if not top < self.delta < float("inf"):
                raise ValueError("delta (%r) must exceed the upper clip bound 1 + epsilon_high = %r" % (self.delta, top))
        if self.use_grpo and (self.importance_sampling_level != "token" or self.delta is not None):
            raise ValueError("use_grpo=True has no clip on the probability ratio: importance_sampling_level and delta must stay at their defaults")
        self.scale_rewards, self.mask_truncated_completions = bool(self.scale_rewards), bool(self.mask_truncated_completions)
        try:
            self.entropy_coef = float(self.entropy_coef)
        except (TypeError, ValueError):
            raise ValueError("entropy_coef must be a finite number, got %r" % (self.entropy_coef,))
        if not math.isfinite(self.entropy_coef):
            raise ValueError("entropy_coef must be a finite number, got %r" % (self.entropy_coef,))
        self.top_entropy_quantile = 1.0 if self.top_entropy_quantile is None else float(self.top_entropy_quantile)
        if not 0.0 < self.top_entropy_quantile <= 1.0:
            raise ValueError("top_entropy_quantile must be in (0, 1], got %r" % (self.top_entropy_quantile,))
        self.sync_ref_model = bool(self.sync_ref_model)
        try:
            self.ref_model_mixup_alpha = float(self.ref_model_mixup_alpha)
        except (TypeError, ValueError):
            raise ValueError("ref_model_mixup_alpha must be in (0, 1], got %r" % (self.ref_model_mixup_alpha,))
        if not 0.0 < self.ref_model_mixup_alpha <= 1.0:
            raise ValueError("ref_model_mixup_alpha must be in (0, 1], got %r" % (self.ref_model_mixup_alpha,))
        try:
            whole = int(self.ref_model_sync_steps) == float(self.ref_model_sync_steps) and int(self.ref_model_sync_steps) >= 1
        except (TypeError, ValueError, OverflowError):
            whole = False
        if not whole:
            raise ValueError("ref_model_sync_steps must be an integer >= 1, got %r" % (self.ref_model_sync_steps,))
        self.ref_model_sync_steps = int(self.ref_model_sync_steps)
        if self.activation_recompute not in ("none", "mlp"):
            raise ValueError('activation_recompute must be "none" or "mlp", got %r' % (self.activation_recompute,))
        if self.optimizer_state_dtype not in ("fp32", "bf16"):
            raise ValueError('optimizer_state_dtype must be "fp32" or "bf16", got %r' % (self.optimizer_state_dtype,))
        if self.sync_ref_model and float(self.beta) == 0.0:
            raise ValueError("sync_ref_model needs a reference policy: beta = 0 keeps none")
        if self.sync_ref_model and self.ref_model_sync_steps % self.num_iterations != 0:
            raise ValueError("ref_model_sync_steps (%d) must be a multiple of num_iterations (%d): the reference moves after the last update on a rollout "
                             "(the replayed updates reuse the reference log-probs of the first)" % (self.ref_model_sync_steps, self.num_iterations))
        if self.steps_per_generation is not None:
            self.steps_per_generation = generation_windows(self) * max(1, int(self.gradient_accumulation_steps))

    beta: float = 0.04
    use_grpo: bool = False
    num_iterations: int = 1                 # mu of the GRPO paper (trl.GRPOConfig.num_iterations): optimizer steps per rollout.  Steps 2 .. mu replay the window's
                                            # completions against the log-probs of the policy that drew them (PPO clip); 1 = one update per rollout, as the reference runs
    steps_per_generation: Optional[int] = None   # trl.GRPOConfig.steps_per_generation, in micro-steps: one rollout serves this many of them.  None = gradient_accumulation_steps
                                            # (every optimizer step draws its own window).  A multiple k * GA: the prompts of k windows are decoded together with the
                                            # current weights - wider decode batches - and windows 2 .. k are updated, one optimizer step each, against log-probs scored
                                            # by a no-grad forward at generation time (the clipped objective on completions one .. k - 1 steps old)
    epsilon_low: float = 0.2                # clip range of the probability ratio: [1 - epsilon_low, 1 + epsilon_high] (the reference hard-codes 0.2 / 0.2, :388-393)
    epsilon_high: Optional[float] = None    # None = same as epsilon_low
    loss_type: Optional[str] = None         # trl.GRPOConfig.loss_type: "grpo" = clip + mean over each completion, then over completions; "bnpo" = clip + mean over all
                                            # live tokens; "dr_grpo" = clip + sum / (num_generations * max_completion_length).  None = the reference's two branches (use_grpo)
    importance_sampling_level: str = "token"   # "sequence" (GSPO): one ratio per completion, the exp of its mean per-token log-ratio, clipped as a whole
    delta: Optional[float] = None           # two-sided clipping: the ratio in the unclipped term is capped at delta (bounds the loss for negative advantages); > 1 + epsilon_high
    scale_rewards: bool = True              # False: advantages = rewards - group mean, without the division by the group's std (Dr. GRPO)
    mask_truncated_completions: bool = False   # completions without an EOS among their max_completion_length tokens leave the loss
    entropy_coef: float = 0.0               # entropy bonus (verl's actor.entropy_coeff): loss - entropy_coef * (the policy's per-token entropy under the loss's own normaliser);
                                            # > 0 rewards entropy, < 0 penalises it, 0 = off (the entropy stays the logged generation_entropy only)
    top_entropy_quantile: float = 1.0       # trl.GRPOConfig.top_entropy_quantile: only the top share of the live tokens by entropy carries the policy-gradient term
                                            # (selected per micro-step: one prompt's completions on one rank; trl selects over the gathered batch); 1 or None = all
    sync_ref_model: bool = False            # trl.GRPOConfig.sync_ref_model (the TR-DPO rule): every ref_model_sync_steps optimizer steps the reference policy becomes
                                            # (1 - ref_model_mixup_alpha) * reference + ref_model_mixup_alpha * policy; False = the snapshot taken at construction never moves
    ref_model_mixup_alpha: float = 0.6      # in (0, 1]; 1 = the reference becomes the policy
    ref_model_sync_steps: int = 512         # a multiple of num_iterations: the reference moves after the last update on a rollout
    activation_recompute: str = "none"      # "mlp": the update saves no xn / xn2 / gate-up / SwiGLU tensors (81 % of the saved activation bytes at 7B width: 157 704 ->
                                            # 29 704 B per row and layer); the backward rebuilds them layer by layer with the forward's own launches - one more gate/up GEMM
                                            # per layer, every gradient bit for bit the "none" run's.  This is what buys the memory the reference
                                            # gets from --gradient_checkpointing
    optimizer_state_dtype: str = "fp32"     # "bf16": the Adam moments m / v are kept in bf16 and rounded stochastically (4 of the trainable arena's 18 B per parameter
                                            # less: -30.6 GB at 7B, and 8 of the optimizer kernel's 30 B of traffic); the random bits are a function of (seed, optimizer
                                            # step, parameter index), so a run repeats, a resume continues bit for bit and the sharded optimizer equals the replicated
                                            # one.  Master weights, gradients and the update rule stay fp32; optimizer_rank*.pt then holds bf16 m / v
    prompt_type: str = "v1"
    fix_vit: bool = True
    stop_at_eos: bool = False               # the reference's GenerationConfig carries no eos_token_id (a6): always C tokens
    trim_completions: bool = False          # rollouts end at EOS: sets stop_at_eos=True; the sampled decode loop stops once every row has drawn its EOS (polled, never a
                                            # per-step wait), and the update - policy and reference forward, head, backward, every replay - runs on the columns up to
                                            # the last row's EOS only (at least 8), P + G*Ct rows instead of P + G*C.  Masks, normalisers (dr_grpo keeps 1 / (G*C)),
                                            # rewards and metrics see the full [G, C]; one more metric key, completions/trimmed_length.  DESIGN.md section 7t
    rollout_batching: bool = True           # decode the prompts of one accumulation window together (same weights, same results)
    grad_wire_dtype: str = "bf16"           # data-parallel gradient exchange wire format ("bf16" | "fp32")
    shard_optimizer: Optional[bool] = None  # ZeRO-style: master/m/v on 1/world of every arena segment, reduce-scatter grads, all-gather bf16 weights.
                                            # None = on for 2 / 4 / 8 ranks (what a zero2 / zero3 `deepspeed` json of the reference scripts selects;
                                            # a non-zero json or False selects the replicated optimizer); no effect on one GPU
    gpu_video_preprocess: Optional[bool] = None   # uint8 frames -> fused HIP resize/normalise/patchify instead of the host processor's pixel path.
                                            # None = automatic: on whenever the row carries pre-decoded uint8 frames; False forces the host processor
    rollout_weight_dtype: str = "bf16"      # "fp8": the SAMPLING policy reads e4m3 copies of the decoder matrices (row scales, re-quantised every window);
                                            # log-probs, KL and the update keep bf16 weights (BASELINE config "fp8 weights")
    disable_log_print: bool = False         # keep log() from printing on rank 0 (bench.py prints exactly one JSON line)
    log_rollout_drift: Optional[bool] = None   # metric rollout_logp_drift = mean |logp under the SAMPLING policy's logits - policy logp| over the
                                            # completion tokens; None = on whenever the rollout reads quantised weights (or an importance cap is set)
    rollout_fp8_keep_bf16: Optional[tuple] = None   # fp8 sampling policies: matrices that stay bf16 ("qkv", "o", "gu", "down", "lm_head").  None = AUTO: the fp8-MFMA
    #                                     policy keeps the attention projections ("qkv", "o": 12 % of the decoder's weight bytes) in bf16 - at 16 decode rows their fp8 kernels
    #                                     are no faster than the bf16 ones (latency-bound; the fp8 q|k|v path also pays a separate rope / KV-append launch), and the policy
    #                                     drifts less: 589.5 ms / 0.244 nat against 593.6 ms / 0.303 nat with every matrix in fp8; () = every matrix fp8
    lazy_grad_zero: bool = True      # the optimizer leaves the decoder layers' large gradient matrices un-zeroed (the next window's first weight gradients
    #                                  overwrite them: Engine.lazy_zero_plan); False = zero the whole gradient arena every step
    rollout_importance_cap: Optional[float] = None   # c: advantage term weighted by min(exp(policy logp - sampling logp), c) per token (truncated
                                            # importance sampling).  None = AUTO: off for a bf16 sampling policy (the reference algebra unchanged), c = 2 for the
                                            # fp8 sampling policies, whose tokens are drawn ~0.2-0.3 nat off the update policy at 7B (e4m3's 3-bit
                                            # mantissa bounds this from below, so the policy-gradient term is CORRECTED instead); 0 = off explicitly
    dataloader_prefetch: int = 2            # batches whose host preprocessing (decode / resize / tokenise) runs ahead on a worker thread; 0 = inline
    rope_index_mode: str = "hf4"            # position rule of the transformers version the reference pins
    # optimisation (HF TrainingArguments names)
    learning_rate: float = 1e-6
    weight_decay: float = 0.0
    adam_beta1: float = 0.9
    adam_beta2: float = 0.999
    adam_epsilon: float = 1e-8
    max_grad_norm: float = 1.0
    lr_scheduler_type: str = "linear"
    warmup_steps: int = 0
    num_train_epochs: float = 1.0
    max_steps: int = -1
    per_device_train_batch_size: int = 1
    gradient_accumulation_steps: int = 1
    seed: int = 42
    data_seed: Optional[int] = None
    bf16: bool = True
    # bookkeeping
    logging_steps: int = 1
    save_strategy: str = "steps"            # "steps" | "epoch" | "no"
    save_steps: int = 500
    save_only_model: bool = False
    report_to: Any = None
    resume_from_checkpoint: Optional[str] = None
    # accepted for CLI compatibility; no effect on the MI355X engine (no DeepSpeed / no sliding window).  gradient_checkpointing changes nothing either, so the
    # reference's scripts keep their speed: its memory effect is obtained with --activation_recompute mlp
    gradient_checkpointing: bool = False
    deepspeed: Optional[str] = None
    model_init_kwargs: Optional[dict] = None
    slide_window: bool = False
    max_window_layers: int = 2
    sliding_window_length: int = 4096
    attn_implementation: str = "flash_attention_2"


class TrainerState:
    def __init__(self):
        self.global_step = 0
        self.max_steps = 0
        self.epoch = 0.0
        self.num_train_epochs = 0
        self.log_history = []
        self.is_world_process_zero = True
        self.is_local_process_zero = True

    def to_json(self):
        return {k: v for k, v in self.__dict__.items()}


class TrainerControl:
    def __init__(self):
        self.should_training_stop = False
        self.should_save = False
        self.should_log = False
        self.should_epoch_stop = False


def _call(cb, name, *a, **k):
    fn = getattr(cb, name, None)
    if fn is not None:
        r = fn(*a, **k)
        return r


class _PhaseClock:
    """Phase boundaries of the micro-steps (preprocess | vision | rollout | logps | backward | optimizer) as HIP events on the stream the
    kernels run on - recording costs ~2 us and never waits; the durations are read when `log()` builds the throughput keys.
    On a CPU op backend (tests) it falls back to the host clock.  A generation cycle of several windows (steps_per_generation) adds the phase `score`: the
    no-grad policy and reference forwards of the deferred windows."""

    def __init__(self, ops):
        dev = getattr(ops, "device", None)
        self.cuda = dev is not None and torch.device(dev).type == "cuda"
        self.marks = []

    def mark(self, name):
        if self.cuda:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
        else:
            e = time.perf_counter()
        self.marks.append((name, e))
        if len(self.marks) > 4096:           # nobody is reading (a caller driving micro-steps without log()): keep the tail only
            del self.marks[:2048]

    def drain(self):
        """-> {phase: milliseconds} summed over the marks recorded so far ("start" marks open an interval and carry no time)."""
        marks, self.marks = self.marks, []
        out = {}
        if self.cuda and marks:
            marks[-1][1].synchronize()
        for (n0, e0), (n1, e1) in zip(marks[:-1], marks[1:]):
            if n1 == "start":
                continue
            dt = e0.elapsed_time(e1) if self.cuda else (e1 - e0) * 1e3
            out[n1] = out.get(n1, 0.0) + dt
        return out


FP8_MFMA_KEEP_BF16 = ("qkv", "o")      # default of GRPOConfig.rollout_fp8_keep_bf16 for the fp8-MFMA sampling policy
FP8_IMPORTANCE_CAP = 2.0      # default truncation c of the per-token importance weight for quantised sampling policies (GRPOConfig.rollout_importance_cap)


# The device half of a micro-step's metric record: one fp32 vector with these slots, for a first pass and a replay, with and without an objective.  loss, kl and
# entropy always carry a value; the record's has_clip / has_drift / has_kl_old say which of the others do (TimeR1_Trainer._update, _flush_metrics)
DEV_SLOTS = ("loss", "kl", "entropy", "clip_low", "clip_high", "clip_region", "drift", "kl_old")


def clip_ratio_metrics(logp, old_logp, advantages, mask, eps_low=0.2, eps_high=0.2):
    """Fractions of completion tokens whose probability ratio exp(logp - old_logp) left the PPO clip range on the side that matters for
    the sign of the advantage: (low, high, either), each sum(flag * mask) / sum(mask) (reference timer1_trainer_ft.py:820-829)."""
    coef = torch.exp(logp - old_logp)
    adv = advantages.reshape(-1, 1)
    m = mask.to(coef.dtype)
    is_low = (coef < 1 - eps_low) & (adv < 0)
    is_high = (coef > 1 + eps_high) & (adv > 0)
    tot = m.sum()
    return (is_low * m).sum() / tot, (is_high * m).sum() / tot, ((is_low | is_high) * m).sum() / tot


def config_from_hf(hc, name="model"):
    """transformers config dict (config.json / PretrainedConfig.to_dict()) of a Qwen2-VL or Qwen2.5-VL checkpoint -> ModelConfig."""
    tc = hc.get("text_config") or hc
    vc = hc["vision_config"]
    from .config import TextConfig, VisionConfig
    rope = tc.get("rope_parameters") or tc.get("rope_scaling") or {}
    text = TextConfig(vocab_size=tc["vocab_size"], hidden=tc["hidden_size"], intermediate=tc["intermediate_size"], n_layers=tc["num_hidden_layers"],
                      n_heads=tc["num_attention_heads"], n_kv_heads=tc["num_key_value_heads"], head_dim=tc["hidden_size"] // tc["num_attention_heads"],
                      rms_eps=tc.get("rms_norm_eps", 1e-6), rope_theta=float(rope.get("rope_theta", tc.get("rope_theta", 1e6))),
                      mrope_section=tuple(rope.get("mrope_section", (16, 24, 24))), tie_word_embeddings=bool(hc.get("tie_word_embeddings", tc.get("tie_word_embeddings", False))))
    tps = 2.0
    if "Qwen2_5" in "".join(hc.get("architectures") or []) or hc.get("model_type") == "qwen2_5_vl":
        # Qwen2.5-VL vision config (configuration_qwen2_5_vl.py): hidden_size = ViT width, out_hidden_size = LLM width
        vision = VisionConfig(depth=vc["depth"], embed_dim=vc["hidden_size"], num_heads=vc["num_heads"], mlp_dim=vc["intermediate_size"],
                              out_hidden=vc["out_hidden_size"], patch_size=vc.get("patch_size", 14), temporal_patch_size=vc.get("temporal_patch_size", 2),
                              spatial_merge_size=vc.get("spatial_merge_size", 2), in_channels=vc.get("in_channels", vc.get("in_chans", 3)),
                              variant="qwen2_5_vl", window_size=vc.get("window_size", 112),
                              fullatt_block_indexes=tuple(vc.get("fullatt_block_indexes", (7, 15, 23, 31))))
        tps = float(vc.get("tokens_per_second", 2))
    else:
        vision = VisionConfig(depth=vc["depth"], embed_dim=vc["embed_dim"], num_heads=vc["num_heads"], mlp_dim=int(vc["embed_dim"] * vc.get("mlp_ratio", 4)),
                              out_hidden=vc["hidden_size"], patch_size=vc.get("patch_size", 14), temporal_patch_size=vc.get("temporal_patch_size", 2),
                              spatial_merge_size=vc.get("spatial_merge_size", 2), in_channels=vc.get("in_channels", vc.get("in_chans", 3)))
    cfg = ModelConfig(text=text, vision=vision, image_token_id=hc["image_token_id"], video_token_id=hc["video_token_id"],
                      vision_start_token_id=hc["vision_start_token_id"], vision_end_token_id=hc["vision_end_token_id"],
                      eos_token_id=tc.get("eos_token_id", hc.get("eos_token_id", 151645)) or 151645, pad_token_id=tc.get("pad_token_id", hc.get("pad_token_id", 151643)) or 151643,
                      tokens_per_second=tps, name=name)
    if isinstance(cfg.eos_token_id, list):
        cfg.eos_token_id = cfg.eos_token_id[0]
    return cfg


def load_model_dir(path, ops, train_vit=False, moment_dtype=torch.float32, **params_kw):
    """HF checkpoint directory (config.json + *.safetensors) -> (ModelConfig, ModelParams); train_vit: the tower in the trainable arena."""
    from safetensors.torch import load_file
    cfg = config_from_hf(json.load(open(os.path.join(path, "config.json"))), name=os.path.basename(os.path.normpath(path)))
    sd = {}
    for f in sorted(os.listdir(path)):
        if f.endswith(".safetensors"):
            sd.update(load_file(os.path.join(path, f)))
    params = ModelParams(cfg, ops, init="none", train_vit=train_vit, moment_dtype=moment_dtype, **params_kw)
    params.load_hf_state_dict(sd)
    return cfg, params


def load_hf_module(model, ops, train_vit=False, moment_dtype=torch.float32, **params_kw):
    """A loaded transformers model (reference timer1_trainer.py:184-206, :244-262 accepts a `PreTrainedModel` instance as well as a path) ->
    (ModelConfig, ModelParams): its config and state dict are copied into the engine's arenas; the module itself is not kept."""
    hc = model.config.to_dict()
    cfg = config_from_hf(hc, name=str(getattr(model.config, "_name_or_path", "") or type(model).__name__).rstrip("/").split("/")[-1])
    params = ModelParams(cfg, ops, init="none", train_vit=train_vit, moment_dtype=moment_dtype, **params_kw)
    params.load_hf_state_dict({k: v.detach() for k, v in model.state_dict().items()})
    return cfg, params


class TimeR1_Trainer:
    """GRPO post-training trainer (video decoded inside compute_loss, reference timer1_trainer.py:518-534)."""
    _is_ft = False

    def __init__(self, model, reward_funcs, metric_funcs, args: GRPOConfig = None, train_dataset=None, eval_dataset=None,
                 processing_class=None, reward_processing_classes=None, callbacks=None, optimizers=(None, None), peft_config=None,
                 max_pixels: Optional[int] = 12845056, min_pixels: Optional[int] = 3136, attn_implementation: str = "flash_attention_2",
                 ops=None):
        if args is None:
            name = model if isinstance(model, str) else getattr(getattr(model, "cfg", None), "name", None) or getattr(getattr(model, "config", None), "_name_or_path", None) or "model"
            args = GRPOConfig(output_dir="%s-GRPO" % str(name).split("/")[-1])
        self.args = args
        # peft_config (reference :264-293, main.py's get_peft_config(model_args)): LoRA on the decoder's projections, kept merged (lora.py)
        self.lora_spec = None
        if peft_config is not None:
            from .lora import LoraSpec
            self.lora_spec = LoraSpec.from_config(peft_config)
            if getattr(args, "sync_ref_model", False):
                raise NotImplementedError("peft_config with sync_ref_model=True: the reference policy is the frozen base copy the merge reads, it cannot move")
            if getattr(args, "shard_optimizer", None):
                raise ValueError("peft_config with shard_optimizer=True: the adapters' optimizer state is a few hundred MB and stays replicated")
        mik = getattr(args, "model_init_kwargs", None) or {}
        td = mik.get("torch_dtype")
        if isinstance(td, str) and td not in ("auto", "bfloat16", "float16", "float32"):   # reference :221-235
            raise ValueError("Invalid `torch_dtype` passed to `GRPOConfig`: %s" % td)
        if ops is None:
            from .ops import HipOps   # fails loudly without the HIP library / a GPU: there is no CPU fallback in the product
            ops = HipOps("cuda:%d" % int(os.environ.get("LOCAL_RANK", "0")))
            ops.use_priority_stream()
        self.ops = ops
        # ---- model.  fix_vit=False (the reference's default, main.py:44-49; GRPOConfig keeps True): the patch embedding, the vision blocks and the
        # merger all train (reference :267-288) - the tower's weights live in the trainable arena (ModelParams(train_vit=True)), so AdamW, the clipping
        # norm, the data-parallel exchange, the reference snapshot and the checkpoints cover them with the rest of the arena
        train_vit = not getattr(args, "fix_vit", True)
        if self.lora_spec is not None:
            from .lora import check_backend
            check_backend(ops)
            # as under peft nothing but the adapters trains: the vision tower stays frozen whatever fix_vit says (the reference's message, :285-286)
            if int(os.environ.get("RANK", "0")) == 0:
                print("[INFO] fix_vit=%s ignored because LoRA/PEFT is enabled." % getattr(args, "fix_vit", True), flush=True)
            train_vit = False
        lora_on = self.lora_spec is not None
        base_kw = dict(optimizer_state=False, with_grad=False) if lora_on else {}      # LoRA: the base arena holds bf16 weights only
        # the moments are allocated in their final dtype wherever this constructor builds the arena (fp32 moments never exist at 7B with "bf16"); a
        # caller's ModelParams is converted in place by AdamWFlat(state_dtype=) below
        mdt = torch.bfloat16 if getattr(args, "optimizer_state_dtype", "fp32") == "bf16" else torch.float32
        if isinstance(model, str):
            if model in PRESETS:
                self.cfg = PRESETS[model]()
                self.params = ModelParams(self.cfg, ops, seed=args.seed, train_vit=train_vit, moment_dtype=mdt, **base_kw)
            else:
                self.cfg, self.params = load_model_dir(model, ops, train_vit=train_vit, moment_dtype=mdt, **base_kw)
        elif isinstance(model, ModelParams):
            # a ModelParams of the other layout is copied by name into a new one (optimizer state included) while the caller's stays alive: two copies
            # of the model at once, which a 7B model does not fit on one card - there, pass a preset / checkpoint directory / ModelConfig, or build
            # ModelParams(train_vit=not fix_vit) yourself (no copy)
            self.cfg, self.params = model.cfg, model.relayout(train_vit)
        elif isinstance(model, ModelConfig):
            self.cfg, self.params = model, ModelParams(model, ops, seed=args.seed, train_vit=train_vit, moment_dtype=mdt, **base_kw)
        elif hasattr(model, "state_dict") and hasattr(model, "config"):
            self.cfg, self.params = load_hf_module(model, ops, train_vit=train_vit, moment_dtype=mdt, **base_kw)      # a loaded transformers model, like the reference accepts
        else:
            raise TypeError("model must be a checkpoint path, a preset name, a ModelConfig, a ModelParams or a loaded transformers model")
        self.model = self.params
        self.engine = Engine(self.cfg, ops, self.params, activation_recompute=getattr(args, "activation_recompute", "none"))
        self.beta = args.beta
        self.lora = None
        if lora_on:
            # the adapters' arena + the frozen base copy W0, which is also the reference policy (the reference keeps ref_model = None under peft and disables
            # the adapter for the reference log-probs, :304-307); kept with beta = 0 too: the merge reads it
            from .lora import LoraAdapters
            self.params.drop_training_state()            # (a caller's ModelParams: its gradient buffer and optimizer state are released)
            self.lora = self.engine.lora = LoraAdapters(self.params, self.lora_spec, seed=args.seed, moment_dtype=mdt)
            self.ref_model = self.lora.base
        else:
            self.ref_model = self.params.train.clone_weights_only() if self.beta != 0.0 else None    # reference :295-307
        # ---- processor
        if processing_class is None:
            if not isinstance(model, str) or model in PRESETS:
                raise ValueError("processing_class is required when the model is not a checkpoint directory")
            from transformers import AutoProcessor
            processing_class = AutoProcessor.from_pretrained(model)
            if hasattr(processing_class, "image_processor"):
                processing_class.image_processor.max_pixels = max_pixels     # reference :317-319
                processing_class.image_processor.min_pixels = min_pixels
        self.processing_class = processing_class
        if hasattr(processing_class, "tokenizer"):                       # reference :321-323 sets both unconditionally
            processing_class.pad_token_id = processing_class.tokenizer.pad_token_id
            processing_class.eos_token_id = processing_class.tokenizer.eos_token_id
        # ---- rewards / metrics
        if not isinstance(reward_funcs, list):
            reward_funcs = [reward_funcs]
        for f in reward_funcs:
            if not callable(f):
                raise NotImplementedError("reward models given as ids/modules are not supported; pass Python callables (main.py:416-420)")
        self.reward_funcs = reward_funcs
        self.metric_funcs = metric_funcs if isinstance(metric_funcs, list) else ([metric_funcs] if metric_funcs else [])
        self.reward_processing_classes = reward_processing_classes or [None] * len(reward_funcs)
        # ---- GRPO settings (reference :362-395)
        self.max_prompt_length = args.max_prompt_length
        self.max_completion_length = args.max_completion_length
        self.num_generations = args.num_generations
        self.use_grpo = args.use_grpo
        self.prompt_type = args.prompt_type
        self.epsilon_low = float(getattr(args, "epsilon_low", 0.2))          # the reference hard-codes 0.2 / 0.2 (:388-393): the defaults
        eh = getattr(args, "epsilon_high", None)
        self.epsilon_high = self.epsilon_low if eh is None else float(eh)
        self.num_iterations = int(getattr(args, "num_iterations", 1) or 1)
        self.scale_rewards = bool(getattr(args, "scale_rewards", True))
        self.mask_truncated = bool(getattr(args, "mask_truncated_completions", False))
        # None while loss_type / importance_sampling_level / delta / mask_truncated_completions are at their defaults: then the loss kernels and metric keys are the
        # reference branches'.  Otherwise every update, first pass and replay, runs grpo_policy_loss and logs the clip_ratio/* keys and policy_kl_old
        self._objective = policy_objective(self.use_grpo, getattr(args, "loss_type", None), getattr(args, "importance_sampling_level", "token"),
                                           getattr(args, "delta", None), self.mask_truncated, self.epsilon_low, self.epsilon_high)
        self._check_reuse_args()
        self._check_ref_sync_args()
        self._check_generation_args()
        self._ref_sync_sums = []             # sync_ref_model: the [2] device sums of the syncs since the last log (ref_sync/weight_distance)
        self._reuse = None                   # num_iterations > 1: what the window's micro-steps keep for the replayed updates (optimizer_window)
        self._replays_since_log = 0
        self.train_dataset, self.eval_dataset = train_dataset, eval_dataset
        self.data_collator = lambda features: features       # identity (:360-361)
        self.callbacks = list(callbacks or [])
        self.dp = DataParallel()
        self.accelerator = types.SimpleNamespace(device=ops.device, gather_for_metrics=self.dp.gather, num_processes=self.dp.world,
                                                 is_main_process=self.dp.rank == 0, unwrap_model=lambda m: m)
        self.core = GRPOCore(self.engine, self.ref_model, self.num_generations, self.max_completion_length, beta=self.beta,
                             use_grpo=self.use_grpo, temperature=args.temperature, top_k=args.top_k, seed=args.seed + 1000 * self.dp.rank,
                             rope_index_mode=args.rope_index_mode, stop_at_eos=args.stop_at_eos, top_p=getattr(args, "top_p", 1.0),
                             min_p=getattr(args, "min_p", None), repetition_penalty=getattr(args, "repetition_penalty", 1.0), objective=self._objective,
                             entropy_coef=getattr(args, "entropy_coef", 0.0), top_entropy_quantile=getattr(args, "top_entropy_quantile", 1.0),
                             activation_recompute=getattr(args, "activation_recompute", "none"), trim_completions=getattr(args, "trim_completions", False))
        self.core.roll.weight_dtype = getattr(args, "rollout_weight_dtype", "bf16")
        keep = getattr(args, "rollout_fp8_keep_bf16", None)
        if keep is None:
            keep = FP8_MFMA_KEEP_BF16 if self.core.roll.weight_dtype == "fp8-mfma" else ()
        self.core.roll.fp8_keep_bf16 = tuple(keep)
        drift = getattr(args, "log_rollout_drift", None)
        cap = getattr(args, "rollout_importance_cap", None)
        if cap is None and self.core.roll.weight_dtype != "bf16":
            cap = FP8_IMPORTANCE_CAP          # an fp8 sampling policy is off-policy by construction: truncated importance weights by default
        self._is_cap = float(cap) if cap else None
        self.core.roll.track_logp = bool(drift) if drift is not None else (self.core.roll.weight_dtype != "bf16" or self._is_cap is not None)
        if optimizers[0] is not None:
            raise NotImplementedError("custom torch optimizers are not supported; the engine owns a fused AdamW over its flat arena")
        self.optimizer = AdamWFlat(self.lora if lora_on else self.params, ops, lr=args.learning_rate, betas=(args.adam_beta1, args.adam_beta2), eps=args.adam_epsilon,
                                   weight_decay=args.weight_decay, max_grad_norm=args.max_grad_norm, dp=self.dp,
                                   grad_wire_dtype=torch.bfloat16 if getattr(args, "grad_wire_dtype", "bf16") == "bf16" else torch.float32,
                                   shard_optimizer=False if lora_on else self._wants_shard(args, self.dp), state_dtype=mdt, seed=args.seed)
        # the decoder layers' large gradient matrices are overwritten by the first micro-step of every window: the optimizer does not zero them
        self.optimizer.lazy_zero = self.engine.lazy_zero_plan() if (getattr(args, "lazy_grad_zero", True) and not lora_on) else None
        self.engine.lazy_zero_active = self.optimizer.lazy_zero is not None
        self.optimizer.lazy_zero_ok = lambda eng=self.engine: bool(eng.wgrad_overwrite_first)      # re-checked at every step (A/B attribute)
        self._metrics_store = defaultdict(list)
        self._pending = []                   # micro-steps whose device-side metric values have not been fetched yet (_flush_metrics)
        self._zeros3 = None
        self._clock = _PhaseClock(ops)
        self._tok_since_log, self._micro_at_log, self._t_last_log = 0.0, 0, None
        self.generated_tokens, self.phase_ms_total = 0.0, defaultdict(float)
        self.state = TrainerState()
        self.state.is_world_process_zero = self.dp.rank == 0
        self.control = TrainerControl()
        self.is_deepspeed_enabled = False
        self._micro = 0
        self._loss_acc, self._tr_loss_last, self._steps_per_epoch = [], 0.0, 0

    def _check_reuse_args(self):
        """num_iterations > 1 against the settings it cannot work with (checked at construction and again when train() starts: args is mutable)."""
        a, mu = self.args, self.num_iterations
        if mu <= 1:
            return
        if self.use_grpo:
            raise ValueError("use_grpo=True has no clip on the probability ratio: an update on a rollout of an older policy would be unbounded; "
                             "num_iterations > 1 needs use_grpo=False")
        if getattr(a, "save_strategy", "no") == "steps" and a.save_steps and int(a.save_steps) % mu != 0:
            raise ValueError("save_steps (%d) must be a multiple of num_iterations (%d): checkpoints are written after the last update on a rollout"
                             % (a.save_steps, mu))

    def _check_generation_args(self, loader_windows=None):
        """steps_per_generation against the settings it cannot work with (at construction and again when train() starts: args is mutable; train() adds the
        windows of an epoch) -> k, the accumulation windows of one generation cycle."""
        return generation_windows(self.args, self.num_iterations, loader_windows)

    def _check_ref_sync_args(self):
        """sync_ref_model against the settings it cannot work with (at construction and again when train() starts: args is mutable) -> the option is on."""
        a = self.args
        if not getattr(a, "sync_ref_model", False):
            return False
        if getattr(self, "lora_spec", None) is not None:
            raise NotImplementedError("peft_config with sync_ref_model=True: the reference policy is the frozen base copy the merge reads, it cannot move")
        if self.ref_model is None:
            raise ValueError("sync_ref_model needs a reference policy: beta = 0 keeps none")
        if not 0.0 < float(a.ref_model_mixup_alpha) <= 1.0:
            raise ValueError("ref_model_mixup_alpha must be in (0, 1], got %r" % (a.ref_model_mixup_alpha,))
        if int(a.ref_model_sync_steps) != a.ref_model_sync_steps or int(a.ref_model_sync_steps) < 1:
            raise ValueError("ref_model_sync_steps must be an integer >= 1, got %r" % (a.ref_model_sync_steps,))
        if int(a.ref_model_sync_steps) % self.num_iterations != 0:
            raise ValueError("ref_model_sync_steps (%d) must be a multiple of num_iterations (%d): the reference moves after the last update on a rollout "
                             "(the replayed updates reuse the reference log-probs of the first)" % (a.ref_model_sync_steps, self.num_iterations))
        if not hasattr(self.ops, "ref_mixup"):
            raise NotImplementedError("sync_ref_model: the %s op backend has no ref_mixup" % type(self.ops).__name__)
        return True

    def _sync_ref_model(self):
        """reference <- (1 - alpha) reference + alpha policy over the whole arena (with fix_vit=False the tower's copy in the reference arena too).  Runs after
        optimizer.step has returned (sharded optimizer: the all-gathers have been waited for, params.train.w16 is whole on every rank); every rank launches
        the same kernel on identical inputs, so the references stay bit-identical without a collective."""
        ref = self.ref_model
        self._ref_sync_sums.append(self.ops.ref_mixup(ref.w16, self.params.train.w16, float(self.args.ref_model_mixup_alpha)))
        ref.version = getattr(ref, "version", 0) + 1       # the kernel's writes are invisible to torch: what the engine derived from the old weights is stale now

    @staticmethod
    def _wants_shard(args, dp=None):
        so = getattr(args, "shard_optimizer", None)
        ds = getattr(args, "deepspeed", None)       # reference scripts: --deepspeed scripts/zero3.json | zero3_offload.json | zero2.json
        # None: follow `deepspeed` when one is given (every reference multi-GPU script passes a zero json); without one, N > 1 ranks still
        # default to sharding - the exchange moves the same bytes as the all-reduce and each rank streams 1/N of the AdamW state
        if so is not None:
            want = bool(so)
        elif isinstance(ds, str):
            want = "zero" in os.path.basename(ds).lower()
        else:
            want = dp is not None and dp.enabled
        if want and dp is not None and dp.enabled and not shard_world_ok(dp.world):
            # arena segments split into 1/2/4/8 equal 128-byte-aligned chunks (params.SEG_ALIGN); other world sizes train with the replicated
            # optimizer (same results, more optimizer-state memory) instead of failing at construction where the reference script ran
            if dp.rank == 0:
                print("[time-r1_amd] optimizer sharding supports 2 / 4 / 8 ranks; world size %d falls back to the replicated optimizer" % dp.world, flush=True)
            return False
        return want

    # ------------------------------------------------------------------------------------------------------ prompt building
    def make_conversation_video(self, example):
        if self.prompt_type not in _TEMPLATES or (not self._is_ft and self.prompt_type != "v1"):
            raise ValueError("unsupported prompt_type %r" % self.prompt_type)
        text = _TEMPLATES[self.prompt_type].replace("[EVENT]", example["problem"])
        return [{"role": "user", "content": [{"type": "text", "text": text},
                                             {"type": "video", "video": example["video_path"], "video_start": example.get("video_start"),
                                              "video_end": example.get("video_end"), "total_pixels": 3584 * 28 * 28, "min_pixels": 16 * 28 * 28}]}]

    def _video_inputs(self, example):
        """-> ([frames float T x 3 x H x W], [fps]). Non-ft: decode the whole file (the reference ignores video_start/end here)."""
        ele = {"type": "video", "video": example["video_path"], "total_pixels": 3584 * 28 * 28, "min_pixels": 16 * 28 * 28}
        if "video_frames" in example:      # pre-decoded uint8/float frames supplied by the caller (no decoder offline)
            ele["video"] = example["video_frames"]
        _, vids, kw = VP.process_vision_info_v3([[{"role": "user", "content": [ele]}]], return_video_kwargs=True)
        return vids, kw["fps"]

    def _prepare_inputs(self, inputs):
        return inputs

    def _prompt_ids(self, text, n_video_tokens):
        """Token ids of the chat-templated prompt with the single <|video_pad|> placeholder expanded to n_video_tokens copies
        (what Qwen2VLProcessor.__call__ does before tokenising, processing_qwen2_vl.py)."""
        pc = self.processing_class
        if hasattr(pc, "prompt_ids"):
            return pc.prompt_ids(text, n_video_tokens)
        tok = getattr(pc, "tokenizer", pc)
        pad = "<|video_pad|>"
        return tok(text.replace(pad, pad * n_video_tokens, 1), add_special_tokens=False)["input_ids"]

    # ------------------------------------------------------------------------------------------------------ the micro-step
    def compute_loss(self, model, inputs, return_outputs=False, num_items_in_batch=None):
        if return_outputs:
            raise ValueError("The GRPOTrainer does not support returning outputs")
        ctx = self._step_prepare(inputs)
        if ctx["forced"] is None:
            self.core.rollout(ctx["st"])
        return self._step_finish(ctx)

    def _host_prepare(self, inputs):
        """Host half of a micro-step's preparation (no GPU work): chat template, video decode / frame sampling / resize (or only the size
        plan when the pixels are produced on the GPU), processor call.  Runs inline or on the prefetch thread (decode and
        resize leave the step's critical path)."""
        example = inputs[0]
        prompts = [self.make_conversation_video(ex) for ex in inputs]
        prompts_text = [self.processing_class.apply_chat_template(p, tokenize=False, add_generation_prompt=True) for p in prompts]
        frames = example.get("video_frames")
        gpu_pre = getattr(self.args, "gpu_video_preprocess", None)
        if (gpu_pre is None or gpu_pre) and torch.is_tensor(frames) and frames.dtype == torch.uint8:
            # pre-decoded uint8 frames: size plan on the host (integers), pixels on the GPU (fused resize + normalise + patchify kernel)
            ele = {"total_pixels": 3584 * 28 * 28, "min_pixels": 16 * 28 * 28}
            T, _, H, W = frames.shape
            th, tw = VP.video_target_size(ele, T, H, W)
            v = self.cfg.vision          # the grid follows from the size plan, so the prompt is tokenised here (prefetch thread) too
            n_tok = ((T + v.temporal_patch_size - 1) // v.temporal_patch_size) * (th // v.patch_size) * (tw // v.patch_size) // v.merge_unit
            ids = np.asarray(self._prompt_ids(prompts_text[0], n_tok)).reshape(-1)
            return dict(prompts=prompts, text=prompts_text, gpu_frames=frames.contiguous(), target=(th, tw), ids_gpu=ids, n_tok=n_tok)
        video_inputs, fps_inputs = self._video_inputs(example)
        prompt_inputs = self.processing_class(text=[prompts_text[0]], images=None, videos=[video_inputs[0]], fps=[fps_inputs[0]], padding=True,
                                              return_tensors="pt", padding_side="left", add_special_tokens=False)
        return dict(prompts=prompts, text=prompts_text, ids=np.asarray(prompt_inputs["input_ids"]).reshape(-1),
                    pixels=prompt_inputs["pixel_values_videos"], grid=np.asarray(prompt_inputs["video_grid_thw"]))

    def _step_prepare(self, inputs):
        """Host preprocessing + vision tower for one micro-step (one prompt: reference facts :524, :548-551)."""
        example = inputs[0]
        hp = example.pop("_host_prepared", None) if isinstance(example, dict) else None
        hp = hp.result() if hp is not None else self._host_prepare(inputs)
        prompts, prompts_text = hp["prompts"], hp["text"]
        if "gpu_frames" in hp:
            v = self.cfg.vision
            pixels, grid = self.ops.video_preprocess(hp["gpu_frames"].to(self.ops.device, non_blocking=True), hp["target"], v.patch_dim_padded, v.patch_size,
                                                     v.temporal_patch_size, v.spatial_merge_size)
            self._clock.mark("preprocess")
            n_tok = grid[0] * grid[1] * grid[2] // v.merge_unit
            ids = hp["ids_gpu"] if hp.get("n_tok") == n_tok else np.asarray(self._prompt_ids(prompts_text[0], n_tok)).reshape(-1)
            st = self.core.prepare(ids, pixels, np.asarray([grid]))
        else:
            st = self.core.prepare(hp["ids"], hp["pixels"], hp["grid"])
        self._clock.mark("vision")
        forced = example.get("_forced_completion_ids")       # test hook: teacher-forced completions instead of sampling
        if forced is not None:
            from .positions import PackedLayout
            st.layout = PackedLayout(st.P, self.num_generations, self.max_completion_length)
            st.completion_ids = self.ops.tensor(np.asarray(forced, dtype=np.int32), torch.int32)
        return dict(inputs=inputs, st=st, prompts=prompts, forced=forced)

    def _step_finish(self, ctx, last_in_window=False):
        """Log-probs, rewards, loss gradient and backward of one prompt: `_step_score`, then `_update`.  Returns the micro-step loss as a DEVICE scalar (HF's
        compute_loss returns a device tensor too): nothing in here waits for the GPU after the backward is enqueued - the metric values that live on the
        device (loss, KL, entropy, clip ratios) are packed into one small vector per micro-step and fetched with ONE copy when `log()` (or
        anybody reading `self._metrics`) asks for them, so the host prepares the next micro-step while this one's backward runs."""
        s = self._step_score(ctx)
        st = s["st"]
        if self._reuse is not None:      # num_iterations > 1: keep what the replayed updates read (the policy's log-probs are the OLD policy's from now on)
            self._reuse.append(dict(st=st, old_logp=st.logp.clone(), mask=s["mask"], adv=s["adv"], tokw=s["tokw"]))
        return self._update(st, s["mask"], s["adv"], tokw=s["tokw"], last=last_in_window, keep_pixels=self._reuse is not None,
                            maskf=s["maskf"], rollout=s["rollout"], clip3=s["clip3"], drift=s["drift"])

    def _step_score(self, ctx, deferred=False):
        """The half of a micro-step that belongs to the rollout: the policy's and the reference's log-probs of the completions, rewards, advantages, masks, the
        truncated importance weights and the rollout's metric values -> dict(st, mask, adv, maskf, tokw, clip3, drift, rollout).
        deferred: a window of a generation cycle whose update comes after an optimizer step (steps_per_generation).  Its policy forward saves nothing
        (GRPOCore.forward_logps(score=True)): st.logp is the OLD policy's from the start, and the update is a replay against it."""
        inputs, st, prompts = ctx["inputs"], ctx["st"], ctx["prompts"]
        G = self.num_generations
        tokens = st.completion_ids
        # tokens first, THEN the log-prob forwards: a device-to-host copy waits for everything queued before it on the stream, so in this
        # order the host decodes / scores / normalises while the GPU is busy with the policy and reference forwards
        comp_host = st.completion_ids_host
        if comp_host is None:
            comp_host = tokens.cpu().numpy()
        # trim_completions: the model runs on the columns up to the last row's EOS; comp_host keeps the full [G, C] rows for the mask, the rewards and the decoded
        # completions (the reference decodes what follows the EOS too)
        trimmed = self.core.trim(st, comp_host, self.processing_class.eos_token_id) if self.core.trim_completions else None
        self.core.forward_logps(st, **({"score": True} if deferred else {}))
        mask_np = eos_mask(comp_host, self.processing_class.eos_token_id)
        lengths, truncated = mask_np.sum(1).astype(np.float32), None      # completion_length and the token counts keep the rollout's lengths
        if self.mask_truncated:
            mask_np, truncated = truncation_mask(comp_host, self.processing_class.eos_token_id, mask_np)
        completions = self.processing_class.batch_decode(torch.as_tensor(comp_host), skip_special_tokens=True)
        prompts_rep = [p for p in prompts for _ in range(G)]
        reward_kwargs = {k: [] for k in inputs[0].keys() if k not in ("prompt", "completion") and not k.startswith("_")}
        for k in reward_kwargs:
            for ex in inputs:
                reward_kwargs[k].extend([ex[k]] * G)
        rewards_per_func = torch.zeros(len(prompts_rep), len(self.reward_funcs))
        for i, fn in enumerate(self.reward_funcs):
            rewards_per_func[:, i] = torch.tensor(fn(prompts=prompts_rep, completions=completions, **reward_kwargs), dtype=torch.float32)
        rewards, advantages, std = group_advantages(rewards_per_func, G) if self.scale_rewards else group_advantages(rewards_per_func, G, scale=False)
        metric_vals = None
        if self._is_ft and self.metric_funcs:
            metric_vals = torch.stack([torch.tensor(fn(prompts=prompts_rep, completions=completions, **reward_kwargs), dtype=torch.float32)
                                       for fn in self.metric_funcs], 1)
        self._clock.mark("score" if deferred else "logps")
        mask_dev = self.ops.tensor(mask_np, torch.int32)
        adv_dev = self.ops.tensor(advantages.numpy(), torch.float32)
        # device-side metric pieces are computed BEFORE the backward releases the step's tensors; tiny [G, C] work on the same stream
        maskf = mask_dev.to(torch.float32)
        clip3 = None
        if self._is_ft and not self.use_grpo and self._objective is None and not deferred:   # reference timer1_trainer_ft.py:820-842 (undefined there for use_grpo: coef_1 does not exist)
            lp = st.logp.float()
            clip3 = torch.stack(clip_ratio_metrics(lp, lp, adv_dev, maskf, self.epsilon_low, self.epsilon_high))   # old policy == policy (one update per rollout)
        drift_t, tokw = None, None
        if st.sample_logp is not None and ctx["forced"] is None:
            d = (st.logp.float() - st.sample_logp.to(st.logp.device).float())          # log importance ratio of every drawn token: update policy / sampling policy
            drift_t = (d.abs() * maskf).sum() / maskf.sum().clamp(min=1)
            if self._is_cap is not None:
                tokw = torch.exp(d).clamp(max=float(self._is_cap))
        # ---- metrics (reference :739-777; ft adds metrics/<fn> and clip ratios :789-842): per-sample host values + the device vector,
        # turned into the reference's gathered means by _flush_metrics
        rollout = dict(length=lengths, rpf=rewards_per_func.numpy().copy(), reward=rewards.numpy().copy(), std=std.numpy().copy(),
                       mvals=None if metric_vals is None else metric_vals.numpy(), truncated=truncated, trimmed=trimmed)
        self.last_completions = completions
        self.last_rewards = rewards
        return dict(st=st, mask=mask_dev, adv=adv_dev, maskf=maskf, tokw=tokw, clip3=clip3, drift=drift_t, rollout=rollout)

    def _update(self, st, mask_dev, adv_dev, tokw=None, old_logp=None, last=False, keep_pixels=False, maskf=None, rollout=None, clip3=None, drift=None):
        """Loss gradient and backward of one micro-step whose log-probs are in `st`: a rollout's first update (old_logp None) or a replay against the kept
        log-probs of the policy that drew it.  last: the window's last micro-step (the gradient exchange overlaps its backward, its weight-gradient epilogues
        leave the clipping norm); keep_pixels: a replay of this state follows; maskf: the mask as fp32 where the caller has it already.  What only a rollout
        has goes into its record: `rollout` (the host values _host_fields names), `clip3` (the ft trainer's own clip fractions) and `drift`.  Appends one
        record to `_pending` and returns the loss as a device scalar."""
        scale = 1.0 / max(1, self.args.gradient_accumulation_steps)     # HF divides the loss by GA (model_accepts_loss_kwargs=False, :421-424)
        sync = None
        if last and self.dp.enabled and self.lora is None:      # (LoRA: the adapters' exchange is not overlapped, optimizer.step begins it)
            sync = self.optimizer.sync
            sync.begin()                      # overlap the gradient exchange with this (last) micro-step's backward
        if maskf is None:
            maskf = mask_dev.to(torch.float32)
        ent_mean = ((st.entropy.float() * maskf).sum(1) / maskf.sum(1).clamp(min=1)).mean()
        extra = dict(tok_weight=tokw, old_logp=old_logp, eps=None if old_logp is None else (self.epsilon_low, self.epsilon_high), keep_pixels=keep_pixels or None)
        extra = {k: v for k, v in extra.items() if v is not None}      # only what is set: the rest keeps loss_backward's own defaults
        if last:      # the final gradient passes through this backward's weight-gradient epilogues: they leave its squared norm (AdamWFlat.step)
            self.engine.norm_sink = self.optimizer.norm_sink_begin(self.engine)
        try:
            out, _ = self.core.loss_backward(st, mask_dev, adv_dev, scale, grad_sync=sync, **extra)
        finally:
            self.engine.norm_sink = None
        self._clock.mark("backward")
        o = out.float()
        from_kernel = o.numel() == 8          # out8 of the ratio / policy kernels: the clip fractions and the k3 distance to the old policy come with the loss
        clip = o[3:6] if from_kernel else clip3
        if self._zeros3 is None:
            self._zeros3 = torch.zeros(3, dtype=torch.float32, device=o.device)      # what a slot without a value holds
        z = self._zeros3
        dev = torch.cat([o[:2], ent_mean.reshape(1).float(), z if clip is None else clip.float(), z[:1] if drift is None else drift.reshape(1).float(),
                         o[6:7] if from_kernel else z[:1]])      # DEV_SLOTS, in one launch
        self._pending.append(dict(dev=dev, rollout=rollout, has_clip=clip is not None, has_drift=drift is not None, has_kl_old=from_kernel))
        return o[0]

    # ------------------------------------------------------------------------------------------------------ deferred metrics
    @property
    def _metrics(self):
        """The reference's `self._metrics` (defaultdict of per-micro-step lists, timer1_trainer.py:739-777).  Reading it resolves the micro-steps
        whose device-side values are still pending with one packed device-to-host copy.  Under data parallelism resolving them is a COLLECTIVE
        (the reference gathers every metric over the ranks), so a plain attribute read never does it - a rank-0-only callback or debug print
        reading `trainer._metrics` would otherwise enter an all-gather alone and hang until the process-group timeout.  There the pending
        micro-steps are resolved by `log()` (every rank calls it at the same optimizer step) or an explicit `flush_metrics()` on ALL ranks."""
        if not self.dp.enabled:
            self._flush_metrics()
        return self._metrics_store

    def flush_metrics(self):
        """Resolve the pending micro-steps' metrics now.  Collective under data parallelism: every rank must call it."""
        self._flush_metrics()
        return self._metrics_store

    def _host_fields(self, pend):
        """The host half of a record, per rollout: ((name, width), ...) in the order they are packed - and read back - in."""
        G = self.num_generations
        mvals = next((r["rollout"]["mvals"] for r in pend if r["rollout"] is not None), None)
        return (("length", G), ("rpf", G * len(self.reward_funcs)), ("reward", G), ("std", G), ("mvals", 0 if mvals is None else G * mvals.shape[1]),
                ("truncated", G if self.mask_truncated else 0),      # mask_truncated_completions: one more value per row, 1 = no EOS
                ("trimmed", 1 if self.core.trim_completions else 0))  # trim_completions: the completion columns the update ran on

    def _flush_metrics(self):
        pend, self._pending = self._pending, []
        if not pend:
            return
        nf = len(self.reward_funcs)
        fields = self._host_fields(pend)
        names, widths = zip(*fields)
        n_host = sum(widths)
        dev = torch.stack([r["dev"] for r in pend])                     # [n, len(DEV_SLOTS)] on the device
        blank = np.zeros(n_host, dtype=np.float32)                       # replayed updates carry device values only
        host = np.stack([blank if r["rollout"] is None else
                         np.concatenate([np.asarray(r["rollout"][name], dtype=np.float32).reshape(-1) for name, w in fields if w]) for r in pend])
        if self.dp.enabled:
            both = torch.cat([self.ops.tensor(host, torch.float32), dev], 1)
            allv = self.dp.gather(both[None]).cpu()                      # [world, n, L]
        else:
            allv = torch.cat([torch.as_tensor(host), dev.cpu()], 1)[None]
        M = self._metrics_store
        for i, r in enumerate(pend):
            v = allv[:, i]                                               # [world, L]: rank-major, like accelerator.gather's concatenation
            d = dict(zip(DEV_SLOTS, v[:, n_host:].unbind(1)))            # slot name -> [world]
            h = dict(zip(names, v[:, :n_host].split(list(widths), 1))) if r["rollout"] is not None else None      # field name -> [world, width]
            # a replay is a further update on a rollout already counted: it logs the loss-side keys only; rewards, lengths, drift and the generated-token
            # count belong to the rollout and are appended by its first update
            if h is not None:
                M["completion_length"].append(h["length"].reshape(-1).mean().item())
                rpf = h["rpf"].reshape(-1, nf).mean(0)
                for j, fn in enumerate(self.reward_funcs):
                    M["rewards/%s" % fn.__name__].append(rpf[j].item())
                M["reward"].append(h["reward"].reshape(-1).mean().item())
                M["reward_std"].append(h["std"].reshape(-1).mean().item())
            if self.beta != 0.0:
                M["kl"].append(d["kl"].mean().item())
            M["generation_entropy"].append(d["entropy"].mean().item())
            if h is not None and h["mvals"].shape[1]:
                mv = h["mvals"].reshape(-1, len(self.metric_funcs))
                for j, fn in enumerate(self.metric_funcs):
                    M["metrics/%s" % fn.__name__].append(mv[:, j].mean().item())
            if r["has_clip"]:
                g_low, g_high, g_reg = d["clip_low"], d["clip_high"], d["clip_region"]
                M["clip_ratio/low_mean"].append(g_low.nanmean().item())
                M["clip_ratio/low_min"].append(g_low[~g_low.isnan()].min().item() if (~g_low.isnan()).any() else float("nan"))
                M["clip_ratio/high_mean"].append(g_high.nanmean().item())
                M["clip_ratio/high_max"].append(g_high[~g_high.isnan()].max().item() if (~g_high.isnan()).any() else float("nan"))
                M["clip_ratio/region_mean"].append(g_reg.nanmean().item())
            if r["has_kl_old"]:
                M["policy_kl_old"].append(d["kl_old"].mean().item())
            if h is not None and h["truncated"].shape[1]:
                M["completions/clipped_ratio"].append(h["truncated"].reshape(-1).mean().item())
            if h is not None and h["trimmed"].shape[1]:
                M["completions/trimmed_length"].append(h["trimmed"].reshape(-1).mean().item())
            if r["has_drift"]:
                M["rollout_logp_drift"].append(d["drift"].mean().item())
            if h is not None:
                self._tok_since_log += float(h["length"].sum())
                self.generated_tokens += float(h["length"].sum())        # cumulative, all ranks

    def accumulation_window(self, batches):
        """All micro-steps of one optimizer step. With rollout_batching the G x len(batches) completions are decoded together
        (weights do not change inside the window, so this equals the reference's sequential micro-steps). Returns the losses
        (device scalars; nothing here waits for the backward)."""
        clock = self._clock
        clock.mark("start")
        if not getattr(self.args, "rollout_batching", True):
            # one prompt at a time, rollout and update interleaved: a sequential rollout keeps its saved prefill (prompt activations, K/V)
            # in the single slot-0 buffers, which the NEXT prompt's prefill overwrites - so each prompt is finished before the next starts
            losses = []
            for i, b in enumerate(batches):
                c = self._step_prepare(b)
                if c["forced"] is None:
                    self.core.rollout(c["st"])
                clock.mark("rollout")
                losses.append(self._step_finish(c, last_in_window=(i == len(batches) - 1)))
            return losses
        ctxs = [self._step_prepare(b) for b in batches]
        todo = [c["st"] for c in ctxs if c["forced"] is None]
        if len(todo) > 1:
            self.core.rollout_many(todo)
        elif todo:
            self.core.rollout(todo[0])
        for st in todo:
            st.completion_ids_host = st.completion_ids.cpu().numpy()        # one wait for the decode loop, ahead of every update
        clock.mark("rollout")
        return [self._step_finish(c, last_in_window=(i == len(ctxs) - 1)) for i, c in enumerate(ctxs)]

    def optimizer_window(self, window, t_start=None):
        """One optimizer step = the unit `train()` repeats: the window's micro-steps, the (clipped, fused) AdamW step with the data-parallel
        gradient exchange, LR schedule, `on_step_end`, logging and step-based checkpoints (TF trainer.py:1892-1961 inner loop body).
        `bench.py` times exactly this method.  With `num_iterations` = mu > 1 one call takes mu optimizer steps on the window's one rollout: the first by the
        same code, the others by `_replay_window`; returns the last step's gradient norm."""
        mu = self.num_iterations
        if self._t_last_log is None:         # driven without train() (bench.py): the throughput keys count from the first window
            self._t_last_log, self._micro_at_log = time.perf_counter(), self._micro
        self._reuse = [] if mu > 1 else None
        try:
            self._loss_acc.extend(self.accumulation_window(window))
        finally:
            recs, self._reuse = self._reuse, None
        self._micro += len(window)
        gnorm = self._optimizer_step(t_start, save=(mu == 1))
        # num_iterations > 1: mu - 1 further optimizer steps on the same completions.  Each replays every micro-step of the window (policy forward on the moved
        # weights, ratio loss against the kept log-probs, backward) with the first pass's last-in-window handling, so every rank runs the same collectives
        for it in range(1, mu):
            if self.control.should_training_stop or (self.state.max_steps > 0 and self.state.global_step >= self.state.max_steps):
                break
            self._loss_acc.extend(self._replay_window(recs, more=(it < mu - 1)))
            gnorm = self._optimizer_step(t_start, save=(it == mu - 1))
        return gnorm

    def _replay_window(self, recs, more, first=False):
        """One further optimizer step's micro-steps on a window already rolled out (recs: what _step_finish kept).  No decode loop, no reference-policy
        forward, no reward calls; more: another replay follows (the states keep their pixels).
        first: the FIRST update of a deferred window of a generation cycle (recs: what _score_window kept) - the same update against the log-probs scored at
        generation time; its records carry the rollout's host metrics and drift, and its micro-steps count as the window's own, not as replays."""
        self._clock.mark("start")
        losses = []
        for i, r in enumerate(recs):
            self.core.forward_logps(r["st"], replay=True)
            self._clock.mark("logps")
            own = dict(rollout=r["rollout"], drift=r["drift"]) if first else {}
            losses.append(self._update(r["st"], r["mask"], r["adv"], tokw=r["tokw"], old_logp=r["old_logp"], last=(i == len(recs) - 1), keep_pixels=more, **own))
            if not first:
                self._replays_since_log += 1
        return losses

    # ------------------------------------------------------------------------------------------------------ several windows per rollout
    rollout_group_rows = 32      # a generation cycle decodes in groups of whole prompts of at most this many rows: the LDS-resident skinny decode kernels end at 32
    #                              rows, and the generic ones above them were slower per sample (64 rows 11.19 ms a step against 4.83 at 32)

    def _rollout_cycle(self, todo):
        """Decode the prompts of a generation cycle with the current weights.  todo: (state, save its prefill) in prompt order; the groups follow that order, so
        the sampling streams (seed + 7919 x calls, one call per prompt) are those of any other grouping.  A saved prefill keeps views of its group's K/V
        cache and one of the engine's activation buffer sets: the next group gets a cache of its own, and the saved sets are numbered across the groups."""
        core = self.core
        per = max(1, int(self.rollout_group_rows) // self.num_generations)
        groups = [todo[i:i + per] for i in range(0, len(todo), per)]
        slot0 = 0
        for gi, grp in enumerate(groups):
            saves = [bool(save) and core.reuse_prefill for _, save in grp]
            core.rollout_many([st for st, _ in grp], save_prefill=saves, slot0=slot0)
            slot0 += sum(saves)
            if any(saves) and gi < len(groups) - 1:
                core.roll.release_cache()
        for st, _ in todo:
            st.completion_ids_host = st.completion_ids.cpu().numpy()        # one wait per decode loop, ahead of every update

    def _score_window(self, ctxs):
        """A deferred window of a generation cycle, before the cycle's first optimizer step: what `_step_finish` computes ahead of its update, with a policy
        forward that saves nothing -> records of the `_reuse` shape (st, old_logp, mask, adv, tokw) plus the rollout's host metrics and drift, which are
        logged with the window's first update."""
        recs = []
        for c in ctxs:
            s = self._step_score(c, deferred=True)
            st = s["st"]
            recs.append(dict(st=st, old_logp=st.logp, mask=s["mask"], adv=s["adv"], tokw=s["tokw"], rollout=s["rollout"], drift=s["drift"]))
            st.logp = st.entropy = st.sample_logp = None      # the replay's forward writes its own; the record holds the old policy's
        return recs

    def generation_cycle(self, windows, t_start=None):
        """k = steps_per_generation / gradient_accumulation_steps accumulation windows on ONE rollout (windows: k lists of GA batches): k x num_iterations
        optimizer steps; returns the last one's gradient norm.  k = 1 is `optimizer_window`.  Otherwise every prompt of the cycle is prepared and decoded with
        the current weights, in groups of at most `rollout_group_rows` rows.  Window 1 is updated as ever (saved-prefill continuation, ratio 1).  Windows
        2 .. k are scored before the first optimizer step - a no-grad policy forward in the replay's launches, the reference forward, rewards, advantages, masks,
        importance weights - and each is then updated like a replay, against those log-probs, one optimizer step per window.  With num_iterations = mu the order
        is trl's, iteration-major: (1,1) .. (k,1), (1,2) .. (k,mu), and iterations 2 .. mu replay every window.  Checkpoints and the reference sync wait for the
        cycle's last step.  max_steps or a callback stop inside a cycle ends it after that optimizer step; the rest of its rollouts is dropped."""
        k, mu = len(windows), self.num_iterations
        if k != self._check_generation_args():
            raise ValueError("generation_cycle got %d window(s); steps_per_generation = %r with gradient_accumulation_steps = %d makes %d"
                             % (k, self.args.steps_per_generation, self.args.gradient_accumulation_steps, self._check_generation_args()))
        if k == 1:
            return self.optimizer_window(windows[0], t_start)
        if self._t_last_log is None:         # driven without train(): the throughput keys count from the first cycle
            self._t_last_log, self._micro_at_log = time.perf_counter(), self._micro
        clock = self._clock
        clock.mark("start")
        ctxs = [[self._step_prepare(b) for b in w] for w in windows]
        # only window 1 saves its prefill for the backward: a deferred window's would belong to weights that have moved by then, and it is large
        self._rollout_cycle([(c["st"], wi == 0) for wi, w in enumerate(ctxs) for c in w if c["forced"] is None])
        clock.mark("rollout")
        for w in ctxs[1:]:
            for c in w:
                c["st"].merger_ctx = None      # no backward follows prepare()'s merger pass of a deferred window: 0.10 GB per prompt at 7B, ahead of the step's peak
        self._reuse = [] if mu > 1 else None
        try:
            self._loss_acc.extend(self._step_finish(c, last_in_window=(i == len(ctxs[0]) - 1)) for i, c in enumerate(ctxs[0]))
        finally:
            first, self._reuse = self._reuse, None
        recs = [first] + [self._score_window(w) for w in ctxs[1:]]
        del ctxs
        stopped = lambda: self.control.should_training_stop or (self.state.max_steps > 0 and self.state.global_step >= self.state.max_steps)
        gnorm = None
        for it in range(mu):
            for wi in range(k):
                if gnorm is not None and stopped():
                    return gnorm
                if it == 0:
                    self._micro += len(windows[wi])
                if it > 0 or wi > 0:
                    self._loss_acc.extend(self._replay_window(recs[wi], more=(it < mu - 1), first=(it == 0)))
                if it == mu - 1:
                    recs[wi] = None          # the window's last update is enqueued: its states, features and [G, C] tensors go
                gnorm = self._optimizer_step(t_start, save=(it == mu - 1 and wi == k - 1))
        return gnorm

    def _optimizer_step(self, t_start, save=True):
        """AdamW step + schedule + callbacks + logging (+ step-based checkpoint when `save`: with num_iterations > 1 only after a rollout's last update).
        `save` also marks the last update on a rollout: the only place the reference policy may move (sync_ref_model), ahead of the log and the checkpoint."""
        a = self.args
        gnorm = self.optimizer.step(lr=self._lr(self.state.global_step))
        if self.lora is not None:
            self.lora.merge()                 # the policy's weights from the base copy and the updated adapter masters
        self.state.global_step += 1
        if save and getattr(a, "sync_ref_model", False) and self.state.global_step % int(a.ref_model_sync_steps) == 0:
            self._sync_ref_model()
        self._clock.mark("optimizer")
        if self._steps_per_epoch:
            self.state.epoch = self.state.global_step / self._steps_per_epoch
        for cb in self.callbacks:
            _call(cb, "on_step_end", a, self.state, self.control)
        if a.logging_steps and self.state.global_step % a.logging_steps == 0:
            # HF logs the mean of the micro-step losses since the last log (training_step returns loss / GA, summed over GA micro-steps);
            # the losses and the gradient norm are device scalars until here - this is the one place per optimizer step the host waits
            losses, self._loss_acc = self._loss_acc, []
            mean_loss = float(torch.stack([torch.as_tensor(x).float().reshape(()) for x in losses]).mean()) if losses else 0.0
            self._tr_loss_last = mean_loss
            self.log({"loss": round(mean_loss, 6), "grad_norm": float(gnorm), "learning_rate": self._lr(self.state.global_step - 1)}, t_start)
        if save and a.save_strategy == "steps" and a.save_steps and self.state.global_step % a.save_steps == 0:
            self._save_checkpoint()
        return gnorm

    # ------------------------------------------------------------------------------------------------------ training loop
    def get_train_dataloader(self):
        """Batches of `per_device_train_batch_size` dataset rows (identity collation), sharded rank-wise: perm(seed)[rank::world], the
        permutation wrapped to a multiple of `world` first (torch DistributedSampler / accelerate even_batches semantics), so every rank
        sees the SAME number of batches - ranks with different step counts would dead-lock in the gradient exchange."""
        n = len(self.train_dataset)
        bs = self.args.per_device_train_batch_size
        seed = self.args.data_seed if self.args.data_seed is not None else self.args.seed
        trainer = self

        class _Loader:
            def __init__(self):
                self.gen = torch.Generator().manual_seed(seed)
                self.skip_next = 0            # batches the NEXT iteration leaves out at its start (mid-epoch resume), without loading their rows

            def per_rank(self):
                return (n + trainer.dp.world - 1) // trainer.dp.world

            def __len__(self):
                return self.per_rank() // bs

            def skip_epochs(self, k):
                """Advance the sampler past k fully consumed epochs (resume) without touching the dataset."""
                for _ in range(k):
                    torch.randperm(n, generator=self.gen)

            def __iter__(self):
                perm = torch.randperm(n, generator=self.gen).tolist()
                world = trainer.dp.world
                total = self.per_rank() * world
                while len(perm) < total:                  # wrap-around padding, like DistributedSampler(drop_last=False)
                    perm += perm[: total - len(perm)]
                mine = perm[trainer.dp.rank::world]
                first, self.skip_next = self.skip_next * bs, 0
                for i in range(first, len(mine) - bs + 1, bs):
                    yield [trainer.train_dataset[j] for j in mine[i:i + bs]]
        return _Loader()

    def _lr(self, step):
        a = self.args
        base = a.learning_rate
        if a.warmup_steps and step < a.warmup_steps:
            return base * float(step) / float(max(1, a.warmup_steps))
        if a.lr_scheduler_type == "constant":
            return base
        prog = float(step - a.warmup_steps) / float(max(1, self.state.max_steps - a.warmup_steps))
        if a.lr_scheduler_type == "cosine":
            return base * max(0.0, 0.5 * (1.0 + math.cos(math.pi * prog)))
        return base * max(0.0, 1.0 - prog)     # linear (HF default)

    def _prefetching(self, loader, skip=0):
        """Iterate `loader` while a worker thread runs _host_prepare for the next `dataloader_prefetch` batches (video decode / resize /
        tokenisation overlap the GPU step; results travel with the batch under the private key `_host_prepared`)."""
        import collections
        import itertools
        depth = int(getattr(self.args, "dataloader_prefetch", 0) or 0)
        if skip and hasattr(loader, "skip_next"):
            loader.skip_next, skip = skip, 0
        it = itertools.islice(iter(loader), skip, None)
        if depth <= 0:
            yield from it
            return
        from concurrent.futures import ThreadPoolExecutor
        pool = ThreadPoolExecutor(max_workers=1, thread_name_prefix="tr1-prefetch")
        q = collections.deque()

        def fill():
            while len(q) < depth:
                try:
                    b = next(it)
                except StopIteration:
                    return
                b = [dict(ex) for ex in b]                # private copy: the future is attached to the row
                b[0]["_host_prepared"] = pool.submit(self._host_prepare, b)
                q.append(b)
        try:
            fill()
            while q:
                b = q.popleft()
                fill()
                yield b
            pool.shutdown(wait=False)        # exhausted: batches already handed out may still be waiting for their worker result
        except BaseException:                # closed early (max_steps / callback stop) or failed: drop the work nobody will read
            pool.shutdown(wait=False, cancel_futures=True)
            raise

    def training_step(self, inputs):
        return self.compute_loss(self.params, inputs)

    def train(self, resume_from_checkpoint=None):
        """The loop that replaces transformers.Trainer.train for main.py:589-625: accumulation windows of `gradient_accumulation_steps`
        micro-steps, optimizer step + LR schedule, callbacks, checkpoints, and HF's resume arithmetic: a checkpoint at global step s
        restarts in epoch s // steps_per_epoch after skipping the (s % steps_per_epoch) * GA batches that epoch already consumed (with
        num_iterations = mu > 1 a loader window yields mu optimizer steps: steps_per_epoch = windows_per_epoch * mu, ((s // mu) % windows_per_epoch) * GA batches); the
        run ends at state.max_steps (main.py sets max_steps = global_step + epochs * steps_per_epoch before resuming, :600-618).
        steps_per_generation = k * GA groups the windows into generation cycles of k (`generation_cycle`): a cycle never spans an epoch, the windows that do
        not fill one are dropped, steps_per_epoch = (windows_per_epoch // k) * k * mu, and a checkpoint sits at a cycle's end - so does a resume."""
        a = self.args
        loader = self.get_train_dataloader()
        ga = max(1, a.gradient_accumulation_steps)
        self._check_reuse_args()
        self._check_ref_sync_args()
        k = self._check_generation_args(len(loader) // ga)
        mu = self.num_iterations
        windows_per_epoch = max(len(loader) // ga, 1) // k * k      # (k = 1: every window; else the windows of the epoch's whole cycles)
        steps_per_epoch = windows_per_epoch * mu              # optimizer steps: one loader window yields num_iterations of them
        self._steps_per_epoch = steps_per_epoch
        if self.state.max_steps <= 0:
            self.state.max_steps = a.max_steps if a.max_steps > 0 else math.ceil(a.num_train_epochs * steps_per_epoch)
        n_epochs = math.ceil(self.state.max_steps / steps_per_epoch)
        self.state.num_train_epochs = n_epochs
        start_step = 0
        ckpt = resume_from_checkpoint if resume_from_checkpoint is not None else a.resume_from_checkpoint
        if ckpt:
            start_step = self._load_checkpoint(ckpt)
        if k > 1 and (start_step % steps_per_epoch) % (k * mu) != 0:
            raise ValueError("checkpoint at global step %d lies inside a generation cycle of %d x %d optimizer steps: resume it with the steps_per_generation "
                             "it was written with" % (start_step, k, mu))
        epoch = start_step // steps_per_epoch                  # fully trained epochs: the sampler is advanced, nothing is replayed
        loader.skip_epochs(epoch)
        skip_batches = ((start_step // mu) % windows_per_epoch) * ga      # consumed part of the current epoch (skipped before any prefetch work)
        self.state.epoch = self.state.global_step / steps_per_epoch
        for cb in self.callbacks:
            _call(cb, "on_train_begin", a, self.state, self.control)
        t_start = time.time()
        self._t_last_log, self._micro_at_log = time.perf_counter(), self._micro
        self._loss_acc, self._tr_loss_last = [], 0.0
        self.control.should_training_stop = False
        while not self.control.should_training_stop and self.state.global_step < self.state.max_steps and epoch < n_epochs:
            window, cycle = [], []
            for batch in self._prefetching(loader, skip_batches):
                window.append(batch)
                if len(window) < ga:
                    continue
                if k == 1:
                    self.optimizer_window(window, t_start)
                else:
                    cycle.append(window)
                    if len(cycle) == k:
                        self.generation_cycle(cycle, t_start)
                        cycle = []
                window = []
                if self.state.global_step >= self.state.max_steps or self.control.should_training_stop:
                    break
            if cycle and self.dp.rank == 0:
                print("[time-r1_amd] epoch %d: %d trailing window(s) do not fill a generation cycle of %d and are dropped (steps_per_epoch = "
                      "len(loader) // GA // %d * %d * num_iterations)" % (epoch, len(cycle), k, k, k), flush=True)
            if window and len(loader) < ga and self.state.global_step < self.state.max_steps and not self.control.should_training_stop:
                # an epoch shorter than one accumulation window (small dataset / many ranks): HF steps on the last batch of a short epoch
                # (TF trainer.py do_sync_step at steps_in_epoch) - without this the run would end after zero optimizer steps
                self.optimizer_window(window, t_start)
            elif window and self.dp.rank == 0:
                print("[time-r1_amd] epoch %d: %d trailing batch(es) do not fill an accumulation window of %d and are dropped (steps_per_epoch = "
                      "len(loader) // GA, the arithmetic main.py's resume logic uses)" % (epoch, len(window), ga), flush=True)
            skip_batches = 0
            if self.state.global_step < (epoch + 1) * steps_per_epoch:
                break                      # stopped inside the epoch (max_steps / callback): no epoch-end event
            epoch += 1
            self.state.epoch = float(epoch)
            for cb in self.callbacks:
                _call(cb, "on_epoch_end", a, self.state, self.control)
            if a.save_strategy == "epoch":
                self._save_checkpoint()
        for cb in self.callbacks:
            _call(cb, "on_train_end", a, self.state, self.control)
        if self._loss_acc:                 # micro-steps since the last log (logging_steps > 1)
            self._tr_loss_last = float(torch.stack([torch.as_tensor(x).float().reshape(()) for x in self._loss_acc]).mean())
            self._loss_acc = []
        return types.SimpleNamespace(global_step=self.state.global_step, training_loss=self._tr_loss_last, metrics={"train_runtime": time.time() - t_start})

    # ------------------------------------------------------------------------------------------------------ logging / saving
    def log(self, logs, start_time=None):
        """The reference's keys (timer1_trainer.py:784-793: means of the per-micro-step metric lists, then cleared) plus the throughput keys
        SURVEY 5.5 asks this build to emit beside them: `samples_per_sec` / `rollout_tokens_per_sec` (whole job) and the two roofline
        fractions of the step's dominant kernel families (`perf/*`, from HIP-event phase times and the algorithmic work of the shapes run)."""
        metrics = {k: sum(v) / len(v) for k, v in self.flush_metrics().items()}     # reference :784-793 (all ranks are here: see _metrics)
        if self._ref_sync_sums:
            # sync_ref_model: ||policy - reference|| / ||reference|| just before each sync since the last log (identical on every rank: no gather); the two
            # sums stayed on the device until here, where the host fetches the step's values anyway
            sums, self._ref_sync_sums = torch.stack(self._ref_sync_sums).double().cpu(), []
            dist_ = sums[:, 0].sqrt() / sums[:, 1].clamp(min=torch.finfo(torch.float32).tiny).sqrt()
            metrics["ref_sync/weight_distance"] = float(dist_.mean())
        logs = {**logs, **metrics, **self._throughput_keys()}
        if self.state.epoch is not None:
            logs["epoch"] = round(self.state.epoch, 4)
        self.state.log_history.append({**logs, "step": self.state.global_step})
        for cb in self.callbacks:
            _call(cb, "on_log", self.args, self.state, self.control, logs=logs)
        if self.dp.rank == 0 and not getattr(self.args, "disable_log_print", False):
            print(logs, flush=True)
        self._metrics_store.clear()

    def _throughput_keys(self):
        """Whole-job rates since the previous log.  Wall time is this rank's (ranks step in lock-step through the gradient exchange); generated
        tokens are the gathered completion lengths; phase times are HIP events on the compute stream (read here, after the step was enqueued)."""
        now = time.perf_counter()
        ph = self._clock.drain()
        n_micro = self._micro - self._micro_at_log
        out = {}
        if self._t_last_log is not None and n_micro > 0 and now > self._t_last_log:
            out["samples_per_sec"] = n_micro * self.dp.world / (now - self._t_last_log)
        toks, self._tok_since_log = self._tok_since_log, 0.0
        roll_ms = ph.get("rollout", 0.0)
        if roll_ms > 0 and toks > 0:
            out["rollout_tokens_per_sec"] = toks / (roll_ms * 1e-3)
        n_replay, self._replays_since_log = self._replays_since_log, 0      # replayed micro-steps: phase time and FLOPs, no new samples or tokens
        n_work = n_micro + n_replay
        if n_work > 0:
            w = self.core.drain_work()
            dec_ms = w.get("decode_ms_events") or 0.0
            if w.get("decode_bytes") and roll_ms > 0:
                # decode steps stream every decoder + lm_head weight once per step (+ the KV cache): HBM-bound family, peak 8 TB/s
                out["perf/decode_hbm_frac"] = w["decode_bytes"] / ((dec_ms or roll_ms) * 1e-3) / 8.0e12
            mm_ms = ph.get("logps", 0.0) + ph.get("backward", 0.0)
            if w.get("train_flops") and mm_ms > 0:
                # log-prob forwards + backward: MFMA-bound family, peak 2.5 PFLOP/s dense bf16
                out["perf/train_mfma_frac"] = w["train_flops"] / (mm_ms * 1e-3) / 2.5e15
        for k, v in ph.items():
            out["perf/ms_%s" % k] = v / max(n_work, 1)
            self.phase_ms_total[k] += v
        self._t_last_log, self._micro_at_log = now, self._micro
        return out

    def save_model(self, output_dir=None, _internal_call=False):
        """16-bit weights under transformers key names in one safetensors file (what the reference's ZeRO-3 save gathers, zero3.json:32)."""
        output_dir = output_dir or self.args.output_dir
        if self.dp.rank != 0:
            return
        os.makedirs(output_dir, exist_ok=True)
        from safetensors.torch import save_file
        save_file(self.params.export_hf_state_dict(), os.path.join(output_dir, "model.safetensors"), metadata={"format": "pt"})
        if self.lora is not None:
            # the merged weights above keep from_pretrained, the evaluation and the filter stages working; the adapter itself goes beside them in peft's layout
            tensors, acfg = self.lora.export_adapter(getattr(self.cfg, "name", None))
            save_file(tensors, os.path.join(output_dir, "adapter_model.safetensors"), metadata={"format": "pt"})
            json.dump(acfg, open(os.path.join(output_dir, "adapter_config.json"), "w"), indent=1)
        json.dump(dataclasses.asdict(self.cfg), open(os.path.join(output_dir, "timer1_model_config.json"), "w"), indent=1)
        from .config import to_hf_config
        json.dump(to_hf_config(self.cfg), open(os.path.join(output_dir, "config.json"), "w"), indent=1)   # reference: save_pretrained via Trainer
        # HF Trainer._save also writes the processor / tokenizer, so `--model_name_or_path <output_dir>/checkpoint-N` reloads (train_rl_SF.sh, eval)
        sp = getattr(self.processing_class, "save_pretrained", None)
        if sp is not None:
            sp(output_dir)
        json.dump(generation_config_dict(self.cfg, self.args), open(os.path.join(output_dir, "generation_config.json"), "w"), indent=1)

    def _save_checkpoint(self):
        d = os.path.join(self.args.output_dir, "checkpoint-%d" % self.state.global_step)
        self.save_model(d)
        if self.dp.rank == 0:
            json.dump({"global_step": self.state.global_step, "max_steps": self.state.max_steps, "epoch": self.state.epoch,
                       "num_train_epochs": self.state.num_train_epochs, "log_history": self.state.log_history,
                       "train_batch_size": self.args.per_device_train_batch_size}, open(os.path.join(d, "trainer_state.json"), "w"), indent=1)
        if not self.args.save_only_model:
            os.makedirs(d, exist_ok=True)
            # (optimizer_state_dtype="bf16": m and v are saved as bf16, 4 B per parameter less; a checkpoint of the other dtype loads too - AdamWFlat.state_dict)
            sd = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in self.optimizer.state_dict().items()}
            sd["rollout_calls"] = self.core.roll.calls
            sd["micro"] = self._micro
            torch.save(sd, os.path.join(d, "optimizer_rank%d.pt" % self.dp.rank))
            if self.ref_model is not None and self.dp.rank == 0:
                # the frozen reference policy is identical on every rank: one copy per checkpoint (15 GB at 7B), not one per rank
                torch.save({"ref_w16": self.ref_model.w16.cpu()}, os.path.join(d, "reference_policy.pt"))
        for cb in self.callbacks:
            _call(cb, "on_save", self.args, self.state, self.control)
        self.dp.barrier()

    def _load_checkpoint(self, d):
        from safetensors.torch import load_file
        opt = os.path.join(d, "optimizer_rank%d.pt" % self.dp.rank)
        if self.lora is not None and not os.path.exists(opt):
            # model.safetensors holds the MERGED weights: without the adapter masters the first merge would overwrite them with W0 + fresh adapters
            raise ValueError("LoRA: %s has no %s (saved with save_only_model=True?) - the adapter state is in it, and a resume without it would silently "
                             "restart from the base model; load the merged model.safetensors as the base model instead" % (d, os.path.basename(opt)))
        self.params.load_hf_state_dict(load_file(os.path.join(d, "model.safetensors")))
        st = json.load(open(os.path.join(d, "trainer_state.json")))
        self.state.global_step = int(st["global_step"])
        self.state.log_history = st.get("log_history", [])
        self.state.epoch = float(st.get("epoch") or 0.0)
        if os.path.exists(opt):
            sd = torch.load(opt, weights_only=False)
            self.params.train.version += 1
            self.optimizer.load_state_dict({k: (v.to(self.ops.device) if torch.is_tensor(v) else v) for k, v in sd.items() if k in ("step", "master", "m", "v", "shard")})
            self.core.roll.calls = sd.get("rollout_calls", 0)
            self._micro = sd.get("micro", 0)
            refp = os.path.join(d, "reference_policy.pt")
            if self.ref_model is not None and os.path.exists(refp):
                self.ref_model.w16.copy_(torch.load(refp, weights_only=False)["ref_w16"].to(self.ops.device))
            elif self.ref_model is not None and "ref_w16" in sd:      # checkpoints written before round 3 embedded it per rank
                self.ref_model.w16.copy_(sd["ref_w16"].to(self.ops.device))
            if self.lora is not None:
                self.lora.merge()      # W0 and the adapter masters are back: the merge gives the saved weights bit for bit
        return self.state.global_step

    def push_to_hub(self, *a, **k):
        raise RuntimeError("no network in this deployment; copy %s instead" % self.args.output_dir)

    def create_model_card(self, *a, **k):
        return None


class TimeR1_Trainer_ft(TimeR1_Trainer):
    """Fine-tune variant: dataset rows carry pre-decoded frames (`video_inputs`, `video_kwargs`), three prompt templates, shaping metrics
    (reference timer1_trainer_ft.py:511-563, :670-691, :789-842; row format finetune.py:594-623)."""
    _is_ft = True

    def _video_inputs(self, example):
        if example.get("video_inputs") is None:
            return super()._video_inputs(example)
        vids = example["video_inputs"]
        while isinstance(vids, (list, tuple)) and vids and isinstance(vids[0], (list, tuple)):
            vids = vids[0]          # the reference's dataset wraps the loaded list once more (finetune.py:598-611)
        kw = example.get("video_kwargs") or {"fps": [VP.FPS]}
        if isinstance(kw, (list, tuple)):
            kw = kw[0]
        vids = [torch.as_tensor(v).float() for v in vids]
        return vids, kw["fps"]
