"""CPU guard for the tile-height cases of tests/test_ops_gpu.py: every entry point of the phased 8-wave GEMM (csrc/gemm.hip) launches four kernels, one per
tile height (224 / 256 / 288 / 320 rows), and each is a separate first launch.  The GPU tests reach a height only through the launcher's cost model and only
while their HipOps wrapper takes the fused path - a shape that stops doing either would go on passing and test nothing.  This replays both on the CPU."""
import os
import re

import optim_cases as oc
import test_ops_gpu as tg

OPS_PY = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "time-r1_amd", "ops.py")
ALL = {224, 256, 288, 320}


def rows(M, N, first):
    """Tile height for M rows x ceil(N / 256) column tiles (optim_cases._replay is the launcher's picker: K-major = first 256, NT = first 224)."""
    return oc._replay(M, N, first == 256)


def nt_takes_8wave(M, N):
    """tr1_gemm_nt_bf16: the 8-wave tile only where strictly cheaper than 128 x 128 (512 slots, efficiency 0.80)."""
    if M < 512 or N < 256:
        return False
    bm = rows(M, N, 224)
    t8, t128 = ((M + bm - 1) // bm) * ((N + 255) // 256), ((M + 127) // 128) * ((N + 127) // 128)
    c8 = float((t8 + 255) // 256) * 256.0 * float(bm * 256) / {224: 0.94, 256: 1.0, 288: 1.025, 320: 1.03}[bm]
    return c8 < float((t128 + 511) // 512) * 512.0 * float(128 * 128) / 0.80


def splitk(M, N, K):        # HipOps._splitk_ok with SPLITK at its default
    return M > 64 and K >= 2048 and K % 64 == 0 and N % 8 == 0 and ((M + 255) // 256) * ((N + 255) // 256) <= 128 and 8 * M * N * 4 <= (1 << 31)


def covers(M, N):           # the >= 192-tile rule of gemm_nn and dgrad_glu_bwd
    return ((M + 255) // 256) * ((N + 255) // 256) >= 192


# test -> (shapes added for the tile heights, shape -> (M, columns that the picker tiles by 256), first, shape -> does its HipOps wrapper take the fused path)
FORMS = {
    "test_gemm_nt": ([(7169, 1032, 64), (11425, 1032, 64), (13057, 1032, 64), (14689, 1032, 64)], lambda s: (s[0], s[1]), 224,
                     lambda s: s[2] % 64 == 0 and s[1] % 8 == 0 and not splitk(*s) and nt_takes_8wave(s[0], s[1])),
    "test_gemm_nn": ([(9729, 1032, 64), (11425, 1032, 64), (14689, 1032, 64)], lambda s: (s[0], s[1]), 256,
                     lambda s: s[0] >= 512 and s[1] >= 256 and s[2] % 64 == 0 and s[1] % 8 == 0 and covers(s[0], s[1])),
    # gate/up: 128 gate + 128 up columns per tile = 256-column tiles of the [M, 2I] projection
    "test_gemm_glu_fused_epilogue": ([(11425, 520, 64, True), (13057, 520, 64, False)], lambda s: (s[0], 2 * s[1]), 256,
                                     lambda s: s[0] > 64 and s[2] % 64 == 0 and s[1] % 8 == 0),
    "test_gemm_quickgelu_and_biased_glu_fused_epilogue": ([(11425, 1032, 64), (13057, 1032, 64), (14689, 1032, 64)], lambda s: (s[0], s[1]), 256,
                                                          lambda s: s[0] > 64 and s[2] % 64 == 0 and s[1] % 8 == 0),
    "test_gemm_qkv_rope_fused_epilogue": ([(11425, 6, 2, 64, 0), (13057, 6, 2, 64, 5), (14689, 6, 2, 64, 0)], lambda s: (s[0], (s[1] + 2 * s[2]) * 128), 256,
                                          lambda s: s[0] > 64 and s[1] % 2 == 0 and s[2] % 2 == 0 and s[3] % 64 == 0),
    "test_gemm_qkv_rope_vit_padded_heads": ([(3809, 16, 64), (4353, 16, 64)], lambda s: (s[0], 6 * s[1] * 40), 256,
                                            lambda s: (s[1] * 40) % 128 == 0 and s[2] % 64 == 0),
    "test_dgrad_glu_bwd_fused_epilogue": ([(13057, 1032, 64)], lambda s: (s[0], s[1]), 256,
                                          lambda s: s[0] >= 512 and s[1] >= 256 and s[2] % 64 == 0 and s[1] % 8 == 0 and covers(s[0], s[1])),
}


def test_every_8wave_form_is_run_at_every_tile_height():
    for name, (added, tiled, first, fused) in FORMS.items():
        mark = [m for m in getattr(tg, name).pytestmark if m.name == "parametrize"]
        assert len(mark) == 1, name
        shapes = [tuple(s) for s in mark[0].args[1]]
        for s in added:
            assert s in shapes, (name, s)
            assert fused(s), "%s%s would take the unfused path of its HipOps wrapper and test nothing" % (name, s)
        reached = {rows(*tiled(s), first) for s in shapes if fused(s)}
        assert reached == ALL, "%s reaches %s - re-pick the shapes" % (name, sorted(reached))
    # the two orders of the picker agree on every shape above (the NT and NN forms of test_gemm_nn are compared bit for bit)
    for added, tiled, _, _ in FORMS.values():
        for s in added:
            assert rows(*tiled(s), 224) == rows(*tiled(s), 256)


def test_the_wrapper_conditions_replayed_above_are_those_of_ops_py():
    src = re.sub(r"\s+", " ", open(OPS_PY).read())
    for text in ("return bool(self.SPLITK and M > 64 and K >= 2048 and K % 64 == 0 and N % 8 == 0 and ((M + 255) // 256) * ((N + 255) // 256) <= 128 and 8 * M * N * 4 <= (1 << 31))",
                 "if M >= 512 and N >= 256 and K % 64 == 0 and N % 8 == 0 and ((M + 255) // 256) * ((N + 255) // 256) >= 192:",
                 "if not out_f32 and self._splitk_ok(M, N, K) and a.stride(1) == 1 and b.stride(1) == 1:",
                 "if self.FUSE_EPI and M > 64 and K % 64 == 0 and N % 8 == 0 and x.stride(1) == 1 and w.stride(1) == 1:",
                 "if self.FUSE_EPI and M > 64 and K % 64 == 0 and I % 8 == 0 and x.stride(1) == 1 and w_gu.stride(1) == 1:",
                 "if (self.FUSE_EPI and M > 64 and head_dim == 128 and n_heads % 2 == 0 and n_kv % 2 == 0 and K % 64 == 0 and x.stride(1) == 1 and w_qkv.stride(1) == 1 and bias is not None):",
                 "return bool(self.FUSE_EPI and head_dim < 128 and head_dim % 16 == 0 and half <= 64 and (n_heads * half) % 128 == 0)",
                 "if (self.FUSE_EPI and M >= 512 and I >= 256 and H % 64 == 0 and I % 8 == 0 and dh.stride(1) == 1 and w_down.stride(1) == 1 and gu.stride(1) == 1 and ((M + 255) // 256) * ((I + 255) // 256) >= 192):"):
        assert text in src, text
