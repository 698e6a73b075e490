"""Golden GRPO micro-step whose completions all end early, captured like the cases of gen_grpo_golden.py (the reference's UNMODIFIED
`TimeR1_Trainer.compute_loss`, tiny random-init Qwen2-VL, fp32, CPU):  C = 16 and every row holds an EOS - first EOS at columns 8, 8, 5, 8 - so
GRPOConfig.trim_completions cuts the update to Ct = 9 of 16 columns.  The reference itself runs all 16 columns and decodes what follows each EOS.

Run here:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_short_golden.py   ->  tests/golden/grpo_step_clip_beta_short.pt

Loaded with helpers.load_case("clip_beta_short"); not part of helpers.CASES (those cases each keep a row without EOS).
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_grpo_golden import run_case  # noqa: E402

if __name__ == "__main__":
    run_case("clip_beta_short", False, 0.04, {0: 8, 1: 8, 2: 5, 3: 8}, 424, C=16)
