"""The C-ABI shared library loads on a CPU-only machine and exports every symbol include/timer1_hip.h declares (no compute calls)."""
import ctypes
import os
import re

import time_r1_amd  # noqa: F401
from time_r1_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_built_in_tree():
    assert os.path.exists(hip.LIB_PATH), "run `python -c 'import __graft_entry__ as g; g.build()'` first"
    assert hip.LIB_PATH.startswith(ROOT), "the extension must live in-tree so the GPU box sees it"


def test_every_declared_symbol_is_exported_and_bound():
    decls = hip.parse_header()
    assert len(decls) >= 35
    raw = ctypes.CDLL(hip.LIB_PATH)
    for name in decls:
        assert hasattr(raw, name), "declared in include/timer1_hip.h but not exported: " + name
    L = hip.lib()
    assert set(L.decls) == set(decls)
    assert L.cdll.tr1_version() >= 1


def test_header_cites_reference_for_each_group():
    txt = open(hip.HEADER).read()
    for token in ("timer1_trainer.py", "TF:", "zero3"):
        assert token in txt
    # every extern "C" definition in csrc/ is declared in the header (no hidden entry points)
    defined = set()
    csrc = os.path.join(ROOT, "time-r1_amd", "csrc")
    for f in os.listdir(csrc):
        if f.endswith(".hip"):
            defined |= set(re.findall(r'extern "C" (?:int64_t|int|const char\*) (tr1_\w+)\(', open(os.path.join(csrc, f)).read()))
    assert defined == set(hip.parse_header()), (defined ^ set(hip.parse_header()))


PK_SYMBOLS = ("tr1_glu_pk_ok", "tr1_glu_pk_image_bytes", "tr1_pack_bf16_glu", "tr1_norm_glu_pk")


def test_packed_gate_up_has_its_own_symbols_and_one_decode_step():
    decls, raw, txt = hip.parse_header(), ctypes.CDLL(hip.LIB_PATH), open(hip.HEADER).read()
    for name in PK_SYMBOLS + ("tr1_decode_step",):
        assert name in decls and hasattr(raw, name), name
    for name in ("tr1_decode_step_w8", "tr1_decode_step_w8a8"):
        assert name not in decls and name not in txt and not hasattr(raw, name), name
    assert [a for _, a in decls["tr1_decode_step"][1]][4:6] == ["lm_head", "lm_head_scale"]


def _rejected(name, *args):
    """The call returns from an argument check (no GPU on this machine: nothing else could return 1000) -> its message."""
    L = hip.lib()
    assert L.raw(name)(*args) == 1000, name
    return L.cdll.tr1_last_error().decode()


def test_norm_gemm_skinny_rejects_glu_outside_0_1_2():
    for glu in (3, 4, 5, -1):
        assert "glu" in _rejected("tr1_norm_gemm_skinny", 0, 0, 0, 0, 0, 1, 16, 1536, 1536, 1536, 16, 1e-6, glu, 0)


PK_M, PK_I, PK_K = (0, 1, 16, 17), (0, 16, 24, 592), (512, 1536, 2048, 2560, 3584, 4096)


def test_glu_pk_ok_is_the_shape_rule():
    ok = hip.lib().raw("tr1_glu_pk_ok")
    for M in PK_M:
        for I in PK_I:
            for K in PK_K:
                assert bool(ok(M, I, K)) == (1 <= M <= 16 and I >= 16 and I % 16 == 0 and K in (3584, 2048, 1536)), (M, I, K)


def test_glu_pk_image_bytes_is_the_reference_formats_size():
    from time_r1_amd import torch_ops as T
    nbytes = hip.lib().raw("tr1_glu_pk_image_bytes")
    for I in PK_I:
        for K in (3584, 2048, 1536):
            assert nbytes(I, K) == (I // 16) * 8 * (K // 512) * (T.PK_REC + 4 * T.PK_TAIL_DW) + 16, (I, K)


def test_decode_step_rejects_a_wrong_mode_mask_or_packed_slot():
    """1 layer of hidden 1536, 1 row.  The layer table and dims are real host arrays; work and logits are only compared with NULL before the checks."""
    from time_r1_amd.ops import HipOps
    slots = HipOps.DECODE_LAYER_SLOTS
    assert len(slots) == 14 and slots.index("gu.pk") == 13

    def step(mask, mode, gu_pk=None):
        table = (ctypes.c_void_p * len(slots))()
        table[slots.index("gu.pk")] = gu_pk
        dims = (ctypes.c_int64 * 13)(1, 1536, 12, 2, 128, 640, 512, 1, 1, 64, 1, mask, mode)
        return _rejected("tr1_decode_step", ctypes.cast(table, ctypes.c_void_p), dims, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0x1000, 1 << 20, 0x1000, 1e-6, 0.1, 0)
    msgs = [step(0, 3), step(0, -1), step(4, 0), step(32, 1), step(0, 1, gu_pk=0x1000), step(0, 2, gu_pk=0x1000)]
    assert "mode" in msgs[0] and msgs[1] == msgs[0]
    assert "fp8_mask" in msgs[2] and msgs[3] == msgs[2]
    assert "gu.pk" in msgs[4] and msgs[5] == msgs[4]
    assert len(set(msgs)) == 3


def test_product_has_no_oracle_import_and_no_cpu_fallback():
    pkg = os.path.join(ROOT, "time-r1_amd")
    for f in os.listdir(pkg):
        if f.endswith(".py") and f != "smoke.py":        # smoke() is the one sanctioned checker call site
            src = open(os.path.join(pkg, f)).read()
            assert "oracle" not in re.sub(r'""".*?"""', "", src, flags=re.S).replace("# oracle", ""), f + " must not import the oracle"
    import pytest
    import torch
    from time_r1_amd.ops import HipOps
    with pytest.raises(Exception):
        HipOps("cpu")
