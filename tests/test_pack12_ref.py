"""The packed 12-bit gate/up format in plain torch (torch_ops.pack_bf16_glu_ref / unpack_bf16_glu_ref): unpack(pack(w)) is w bit for bit, and a stage with
more patches than the tail holds reports the matrix as not representable."""
import pytest
import torch

import time_r1_amd  # noqa: F401
import time_r1_amd.torch_ops as T

import pack12_cases as C

I, K = 64, 1536          # 4 column-group pairs x 8 waves x 3 stages


def _round_trip(w):
    rec, tails, ok = T.pack_bf16_glu_ref(w)
    assert rec.shape == (I // 16 * 8 * (K // 512), T.PK_REC) and rec.dtype == torch.uint8 and tails.shape == (rec.shape[0], T.PK_TAIL_DW)
    return rec, tails, ok, T.unpack_bf16_glu_ref(rec, tails, I, K)


@pytest.mark.parametrize("name", ["normal", "uniform", "student_t", "zero", "denormal"])
def test_round_trip_of_weight_distributions(name):
    w = C.distributions(I, K)[name]
    _, _, ok, back = _round_trip(w)
    assert ok and C.same_bits(back, w)


@pytest.mark.parametrize("kind", C.ADVERSARIAL)
def test_round_trip_of_adversarial_stages(kind):
    w = C.distributions(I, K)["normal"].clone()
    where = (1, 7, 2)
    n = C.fill_stage(w, I, K, where, kind)
    _, tails, ok, back = _round_trip(w)
    stage = (where[0] * 8 + where[1]) * (K // 512) + where[2]
    assert int(tails[stage, 1]) == n and ok and C.same_bits(back, w)


def test_a_stage_with_more_patches_than_the_tail_holds_is_not_representable():
    w = C.distributions(I, K)["normal"].clone()
    assert C.fill_stage(w, I, K, (3, 0, 0), "P_plus_1") == T.PK_P + 1
    _, tails, ok, _ = _round_trip(w)
    assert not ok and int(tails[3 * 8 * 3, 1]) == T.PK_P


def test_patch_capacity_matches_the_shared_cases():
    assert C.P == T.PK_P
