"""GPU: every attention kernel (csrc/attn_fwd.hip, attn_fwd32.hip, attn_fwd64.hip, attn_bwd.hip) against the fp64 references of tests/attn_cases.py, at
per-element bounds derived from the kernels' rounding points.  tests/test_attention_ref.py shows on the CPU that the fp32 oracle sits within a tenth of
these bounds, that an emulation of the rounding points stays within them, that they catch every mask mutant and that the cases reach the mechanisms they
are named for.

THE BOUNDS (u = 2^-8, the bf16 unit roundoff).  The accumulating operand of the second product (P forward, P and dS backward) is rounded to bf16 before its
MFMA, the output is rounded to bf16 once, everything else is fp32:
    tol_O   = 1.05 u (sum_j p_j |v_jd| + |O|) + 2^-20 max|v|
    tol_dV  = 1.05 u (sum_i P_ij |dO_id| + |dV|) + 2^-20 max|dO|
    tol_dQ  = 1.05 u (scale sum_j |dS_ij| |k_jd| + |dQ|) + scale sum_j E_ij |k_jd| + 2^-20 max|k|          (tol_dK: the same with q and the sums over i)
    tol_dK at head dim 128 counts the dS sum TWICE: attn_bwd_dkdv32_kernel forms dS from the bf16 P of its exchange buffer (attn_cases.ref_bwd; found on the
    MI355X: with the dS sum counted once, dK of `rows257` stood at 1.04 of the bound, `rows256-g2` at 0.95, `causal-200` at 0.92)
    E_ij    = P_ij 2^-17 (sum_d |dO_id v_jd| + sum_d |dO_id O_id|)        the fp32 128-term accumulations under the cancellation in dP - delta
    tol_lse = 2^-17 max_j (scale sum_d |q_d k_jd|) + 2^-22 |lse| + 1e-5
(1.05: the second-order fp32 terms.)  With the RoPE backward folded in, the bound passes through the rotation with absolute values and gains one more
1.05 u |result| for the rounding after the rotation (attn_cases._rope_bwd).  The backward reference is the flash formula of the inputs the kernel is
given - bf16 O and fp32 lse of the fp64 forward - so that only the backward is under test.

Every check prints `OBS <what> max err, share of bound` (`pytest -s`); the worst shares seen on an MI355X stand next to each test."""
import math

import pytest
import torch

import attn_cases as ac

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
I32 = torch.int32
DEV = "cuda:0"
SENT = 7.0                                  # sentinel in every output element that no launch may write


def bits(t):
    return t.contiguous().view(torch.int16).cpu()


def check(got, ref, tol, what):
    sh, err = ac.share(got, ref, tol)
    print("OBS %-64s max err %.3e  (%.3f of the bound)" % (what, err, sh))
    assert sh <= 1.0, "%s: max err %.4g is %.3g x the bound" % (what, err, sh)
    return sh


def masks_dev(c):
    return [x.to(I32).to(DEV) for x in (c.pre, c.lo, c.hi)]


class Wide:
    """q / k / v / out as column views of ONE buffer [rows, q | k | v | out | 8 pad]: the queries are rows r0 .. r0 + T (r0 = n_slots - T: the completion rows
    of a continuation forward), K / V rows past n_slots are NaN, the rest of the q columns is NaN and the rest of the out columns holds the sentinel."""

    def __init__(self, c):
        qd, kvd = c.nh * c.hd, c.nkv * c.hd
        rows, self.r0 = c.k.shape[0], c.S - c.T
        assert self.r0 >= 0
        host = torch.full((rows, 2 * qd + 2 * kvd + 8), math.nan, dtype=BF16)
        host[self.r0:self.r0 + c.T, :qd] = c.q
        host[:, qd:qd + kvd] = c.k
        host[:, qd + kvd:qd + 2 * kvd] = c.v
        host[:, qd + 2 * kvd:] = SENT
        self.host, self.c, self.o0 = host, c, qd + 2 * kvd
        self.buf = host.to(DEV)
        self.q = self.buf[self.r0:self.r0 + c.T, :qd]
        self.k, self.v = self.buf[:, qd:qd + kvd], self.buf[:, qd + kvd:qd + 2 * kvd]
        self.out = self.buf[self.r0:self.r0 + c.T, self.o0:self.o0 + qd]

    def reset_out(self):
        self.buf[:, self.o0:] = SENT

    def assert_untouched(self, what, out_cols=None):
        """Inputs bit-identical, sentinel intact outside the output view (out_cols: bool [qd], the columns of the view the launch writes)."""
        c, after = self.c, self.buf.cpu()
        assert torch.equal(bits(after[:, :self.o0]), bits(self.host[:, :self.o0])), what + ": an input was written"
        keep = torch.ones(after.shape[0], after.shape[1] - self.o0, dtype=torch.bool)
        keep[self.r0:self.r0 + c.T, :c.nh * c.hd] = False if out_cols is None else ~out_cols[None, :]
        assert bool((after[:, self.o0:][keep].float() == SENT).all()), what + ": wrote outside the output view"


def check_fwd(c, r, o, lse, what):
    sh = [check(o, r.O, r.tol_O, what + " O")]
    if lse is not None:
        sh.append(check(lse, r.lse, r.tol_lse, what + " lse"))
    # exact: a row with ONE visible key returns that V row bit for bit (p = 1 exactly); a row with none returns 0 (and lse = -inf: checked by share())
    n_vis = r.vis.sum(1)
    og = o.cpu().view(c.T, c.nh, c.hd)
    for t in torch.nonzero(n_vis == 1).flatten().tolist():
        j = int(r.vis[t].float().argmax())
        vrow = c.v[j].view(c.nkv, c.hd).repeat_interleave(c.group, 0)
        assert torch.equal(bits(og[t]), bits(vrow)), "%s: token %d sees only key %d and must return its V row exactly" % (what, t, j)
    blind = n_vis == 0
    assert bool((og[blind].float() == 0).all()), what + ": rows that see nothing must return 0"
    return sh


# ------------------------------------------------------------------------------------------------------------ A. forward, single pass
# attn_fwd_kernel<D, 2, 1> (V^T operand; head dims 32 / 64 / 80 / 120 / 128), attn_fwd32_kernel<8> (v_rows) and attn_fwd64_kernel (TR1_FWD64=1), each against fp64.
# Worst share of the bound seen on MI355X over the 26 cases (tol_O | tol_lse):
#   attn_fwd_kernel<32>    0.680 (clamped-d32)      | 0.023        attn_fwd_kernel<64>   0.705 (tile-edges-64-32) | 0.055 (long-prefix-d64)
#   attn_fwd_kernel<96>    0.580 (causal-65)        | 0.027        attn_fwd_kernel<128>  0.733 (tile-edges-65-31) | 0.035 (head dim 120, d_real < D: 0.709 | 0.027, prefix-d120)
#   attn_fwd32_kernel<8>   0.789 (long-causal)      | 0.035        attn_fwd64_kernel     0.789 (long-causal)      | 0.035 (every figure equal to the 32-row kernel's)
# The largest LSE error was 1.0e-5 (long-causal, rows with 60-nat scores): tol_lse is an fp32 worst case, the MFMA accumulation stays far inside it.
@pytest.mark.parametrize("name", ac.CASE_NAMES)
def test_forward_single_pass(hip_ops, name, monkeypatch):
    c, r = ac.case(name), ac.ref_fwd_of(name)
    w = Wide(c)
    pre, lo, hi = masks_dev(c)
    vt = ac.vt_of(c).to(DEV)
    vt0 = bits(vt)
    args = (pre, lo, hi, c.nh, c.nkv, c.S, c.hd, c.scale)
    o, lse = hip_ops.attn_fwd(w.q, w.k, vt, *args, out=w.out)
    assert o.data_ptr() == w.out.data_ptr()
    check_fwd(c, r, o, lse, "fwd %s attn_fwd_kernel<%d>" % (name, (c.hd + 31) // 32 * 32))
    w.assert_untouched(name + " V^T kernel")
    assert torch.equal(bits(vt), vt0), "V^T was written"
    if c.hd != 128:
        return
    assert hip_ops.attn_fwd_rows_ok(c.hd, n_slots=c.S, ld=w.k.stride(0))
    for env, kern in (("0", "attn_fwd32_kernel<8>"), ("1", "attn_fwd64_kernel")):
        monkeypatch.setenv("TR1_FWD64", env)
        w.reset_out()
        o, lse = hip_ops.attn_fwd(w.q, w.k, None, *args, v_rows=w.v, out=w.out)
        torch.cuda.synchronize()
        check_fwd(c, r, o, lse, "fwd %s %s" % (name, kern))
        w.assert_untouched("%s %s" % (name, kern))


# attn_fwd32_kernel<6> (live96=True): features 96..127 of q / k / v zero, columns 96..127 of every head of the output left alone.
# Worst seen on MI355X: O 0.714 of tol_O (tile-edges-65-31), lse 0.028 of tol_lse.
@pytest.mark.parametrize("name", ["causal-200", "segments-128", "clamped", "gap", "tile-edges-65-31", "continuation"])
def test_forward_live96(hip_ops, name, monkeypatch):
    monkeypatch.setenv("TR1_FWD64", "0")
    c = ac.zero_tail_features(ac.case(name))
    r = ac.ref_fwd(c)
    w = Wide(c)
    o, lse = hip_ops.attn_fwd(w.q, w.k, None, *masks_dev(c), c.nh, c.nkv, c.S, c.hd, c.scale, v_rows=w.v, out=w.out, live96=True)
    live = (torch.arange(c.hd) < 96).repeat(c.nh)
    w.assert_untouched(name + " live-96", out_cols=live)
    got = torch.where(live[None, :], o.cpu().float(), torch.zeros(()))          # the reference is exactly 0 in the dead columns (v is 0 there)
    assert bool((r.O[:, ~live] == 0).all())
    check_fwd(c, r, got.to(BF16), lse, "fwd %s attn_fwd32_kernel<6>" % name)


# ------------------------------------------------------------------------------------------------------------ B. split-KV
SPLIT_CASES = ["causal-200", "gap", "prefix-only", "rows255-g3", "tile-edges-64-32", "long-prefix-d64", "dec-step0", "dec-p33", "dec-d64-ragged"]


# attn_fwd_kernel<D, 1, 3> + the merge: attn_combine128_kernel (d = 128, o_ld % 8 == 0), attn_combine_kernel<128> (o_ld % 8 == 4), attn_combine_kernel<64>.
# nsplit 16 / 64 exceed the relevant tiles of most blocks: empty splits enter the merge with m = -inf, l = 0; short rows have all their keys in one split.
# Worst seen on MI355X (the same for every nsplit): attn_combine128_kernel and attn_combine_kernel<128> O 0.682 (prefix-only), lse 0.028;
# attn_combine_kernel<64> O 0.705 (tile-edges-64-32), lse 0.055.
@pytest.mark.parametrize("nsplit", [2, 3, 16, 64])
@pytest.mark.parametrize("name", SPLIT_CASES)
def test_forward_split_kv(hip_ops, name, nsplit):
    c, r = ac.case(name), ac.ref_fwd_of(name)
    pre, lo, hi = masks_dev(c)
    q, k, vt = c.q.to(DEV), c.k.to(DEV), ac.vt_of(c).to(DEV)
    qd = c.nh * c.hd
    for pad in (0, 4):
        obuf = torch.full((c.T, qd + pad), SENT, dtype=BF16, device=DEV)
        o, lse = hip_ops.attn_fwd(q, k, vt, pre, lo, hi, c.nh, c.nkv, c.S, c.hd, c.scale, nsplit=nsplit, out=obuf[:, :qd])
        kern = "attn_combine128_kernel" if (c.hd == 128 and pad == 0) else "attn_combine_kernel<%d>" % c.hd
        check_fwd(c, r, o, lse, "split %s nsplit %d %s" % (name, nsplit, kern))
        assert pad == 0 or bool((obuf[:, qd:].float() == SENT).all()), "wrote outside the output view"
    assert torch.equal(bits(k), bits(c.k)) and torch.equal(bits(q), bits(c.q))


# plan_mode 1 (publishes the tile lists) then plan_mode 2 on the same masks: attn_dec32_kernel at d = 128 with n_slots % 64 == 0, the attn_fwd_kernel fallback
# otherwise (dec-ragged, and head dim 64).
# Worst seen on MI355X: attn_dec32_kernel O 0.698 (dec-p64), lse 0.026; attn_fwd_kernel<128,1,3> O 0.698 / lse 0.026 (mode 1) and 0.517 / 0.021 (the mode 2
# fallback, dec-ragged); attn_fwd_kernel<64,1,3> O 0.610, lse 0.015.
@pytest.mark.parametrize("nsplit", [4, 16])
@pytest.mark.parametrize("name", ac.DECODE_NAMES)
def test_forward_decode_plan(hip_ops, name, nsplit):
    c, r = ac.case(name), ac.ref_fwd_of(name)
    pre, lo, hi = masks_dev(c)
    q, k, vt = c.q.to(DEV), c.k.to(DEV), ac.vt_of(c).to(DEV)
    plan = hip_ops.attn_plan(c.T, c.nh, c.nkv)
    dec32 = c.hd == 128 and c.S % 64 == 0
    for mode in (1, 2):
        o, lse = hip_ops.attn_fwd(q, k, vt, pre, lo, hi, c.nh, c.nkv, c.S, c.hd, c.scale, nsplit=nsplit, plan=plan, plan_mode=mode)
        kern = "attn_dec32_kernel" if (dec32 and mode == 2) else "attn_fwd_kernel<%d,1,3>" % c.hd
        check_fwd(c, r, o, lse, "plan %s nsplit %d mode %d %s" % (name, nsplit, mode, kern))
    o, lse = hip_ops.attn_fwd(q, k, vt, pre, lo, hi, c.nh, c.nkv, c.S, c.hd, c.scale, nsplit=nsplit, need_lse=False, plan=plan, plan_mode=2)
    assert lse is None
    check_fwd(c, r, o, None, "plan %s nsplit %d mode 2 without lse" % (name, nsplit))


def _batch_pair():
    a = ac.case("dec-p32")
    b = ac.build("dec-p32/b", a.hd, a.nh, a.nkv, ac.masks_decode(32, 8, 32, [0, 31, 5, 31, 30, 2, 31, 9], S=a.S), seed=777, blocks=ac.DECODE_BLOCKS, alloc_pad=64, rot=5)
    return a, b


# n_batch = 2 with kv_batch_slots (problem b reads the cache from slot b * kv_batch_slots; the slots between the problems are NaN), row-major and
# fragment-major output (attn_fwd_frag, un-fragmented on the host by its documented index formula; the pad rows of the last 16-row group are not asserted).
# Worst seen on MI355X: O 0.618 of tol_O in both layouts (bit-identical), lse 0.020 of tol_lse.
@pytest.mark.parametrize("nsplit", [3, 16])
def test_forward_decode_batched_and_fragment_major(hip_ops, nsplit):
    a, b = _batch_pair()
    ra, rb = ac.ref_fwd_of("dec-p32"), ac.ref_fwd(b)
    kvs = a.k.shape[0]                                          # 320 slots + 64 NaN rows per problem
    assert kvs == b.k.shape[0] and kvs % 64 == 0 and kvs > a.S
    k = torch.cat([a.k, b.k]).to(DEV)
    vt = torch.full((a.nkv * a.hd, 2 * kvs + 8), math.nan, dtype=BF16)
    vt[:, :a.S], vt[:, kvs:kvs + b.S] = a.v[:a.S].t(), b.v[:b.S].t()
    vt = vt.to(DEV)
    q = torch.cat([a.q, b.q]).to(DEV)
    pre, lo, hi = [torch.cat([x, y]).to(I32).to(DEV) for x, y in zip((a.pre, a.lo, a.hi), (b.pre, b.lo, b.hi))]
    plan = hip_ops.attn_plan(a.T, a.nh, a.nkv, n_batch=2)
    args = (q, k, vt, pre, lo, hi, a.nh, a.nkv, a.S, a.hd, a.scale)
    for mode in (1, 2):
        o, _ = hip_ops.attn_fwd(*args, nsplit=nsplit, need_lse=False, n_batch=2, kv_batch_slots=kvs, plan=plan, plan_mode=mode)
        check_fwd(a, ra, o[:a.T], None, "batched nsplit %d mode %d problem 0" % (nsplit, mode))
        check_fwd(b, rb, o[a.T:], None, "batched nsplit %d mode %d problem 1" % (nsplit, mode))
        of = hip_ops.attn_fwd_frag(*args, nsplit, n_batch=2, kv_batch_slots=kvs, plan=plan, plan_mode=mode)
        rows = ac.unfrag(of.cpu(), 2 * a.T, a.nh)
        check_fwd(a, ra, rows[:a.T], None, "fragment-major nsplit %d mode %d problem 0" % (nsplit, mode))
        check_fwd(b, rb, rows[a.T:], None, "fragment-major nsplit %d mode %d problem 1" % (nsplit, mode))
        assert torch.equal(bits(rows), bits(o)), "fragment-major and row-major merges differ"
    o, lse = hip_ops.attn_fwd(*args, nsplit=nsplit, n_batch=2, kv_batch_slots=kvs)      # no plan, with the LSE [n_batch * n_heads, T]
    check(lse[:a.nh], ra.lse, ra.tol_lse, "batched nsplit %d lse problem 0" % nsplit)
    check(lse[a.nh:], rb.lse, rb.tol_lse, "batched nsplit %d lse problem 1" % nsplit)


# ------------------------------------------------------------------------------------------------------------ C. backward
def _bwd_inputs(c, r):
    o16, lse32 = ac.bf(r.O), r.lse.float()
    return o16, lse32, [t.to(DEV) for t in (c.q, c.k, c.v, o16, c.do, lse32)]


def check_bwd(c, r, b, dq, dk, dv, what):
    sh = [check(dq, b.dQ, b.tol_dQ, what + " dQ"), check(dk, b.dK, b.tol_dK, what + " dK"), check(dv, b.dV, b.tol_dV, what + " dV")]
    assert bool((dk.cpu().float()[c.unseen] == 0).all()) and bool((dv.cpu().float()[c.unseen] == 0).all()), what + ": dK / dV must be 0 on the slots that no row sees"
    dqh = dq.cpu().float()
    assert bool((dqh[r.vis.sum(1) == 0] == 0).all()), what + ": dQ must be 0 on rows that see nothing"
    assert bool((dqh[(c.do.float() == 0).all(1)] == 0).all()), what + ": dO == 0 rows must give dQ == 0 exactly"
    return sh


# tr1_attn_bwd: attn_bwd_dq_kernel<D> + attn_bwd_dkdv_kernel<D, 4> in the 4-wave Q^T form (head dims 32, 80) and <D, 8> in the 8-wave form (64, and 120 in
# the kernels padded to 128: d_real < D), attn_bwd_dq32_kernel + attn_bwd_dkdv32_kernel (128); QS == 1 (causal-1, causal-64, causal-33-d120) and QS > 1 with
# attn_bwd_reduce_kernel<false>.
# Worst share of the bound seen on MI355X over the 26 cases (tol_dQ | tol_dK | tol_dV):
#   head dim 32   0.784 (clamped-d32)      | 0.694 (clamped-d32) | 0.735 (causal-9)           head dim 64    0.769 (tile-edges-64-32) | 0.753 (gap-d64) | 0.638
#   head dim 80   0.780 (segments)         | 0.751 (segments)    | 0.759 (causal-65)          head dim 128   0.872 (rows256-g2)       | 0.698 (rows257) | 0.828 (causal-64)
#   head dim 120  0.850 (prefix-d120)      | 0.671 (prefix-d120) | 0.726 (prefix-d120)
# (head dim 128 dK with the bf16-P term of attn_cases.ref_bwd; without it 1.04 / 0.95 / 0.92 on rows257 / rows256-g2 / causal-200.)
@pytest.mark.parametrize("name", ac.CASE_NAMES)
def test_backward(hip_ops, name):
    c, r = ac.case(name), ac.ref_fwd_of(name)
    o16, lse32, (q, k, v, o, do, lse) = _bwd_inputs(c, r)
    b = ac.ref_bwd(c, o16, lse32)
    pre, lo, hi = masks_dev(c)
    dq, dk, dv = hip_ops.attn_bwd(q, k, v, o, do, lse, pre, lo, hi, c.nh, c.nkv, c.S, c.hd, c.scale)
    check_bwd(c, r, b, dq, dk, dv, "bwd %s d%d" % (name, c.hd))
    for t, h in ((q, c.q), (k, c.k), (v, c.v), (o, o16), (do, c.do)):
        assert torch.equal(bits(t), bits(h)), "the backward wrote an input"


# Head dim 128 with Q / dO past the 32-bit byte offsets of attn_bwd_dkdv32_kernel's LDS DMA (T * ld * 2 >= 2^32): q and dO are column views of one [T, ld] device
# buffer of about 4.3 GB, of which only the two views are ever written or read.  The launch takes attn_delta_kernel + attn_bwd_dq32_kernel without its fused
# prologue (K / V are ordinary) + attn_bwd_dkdv_kernel<128, 8> (64-bit addressing, fp32 P in the dK product: the dS sum of tol_dK counts ONCE) +
# attn_bwd_reduce_kernel<false> (QS = 5).
# Worst seen on MI355X: dQ 0.809, dK 0.670 (at the bound that counts the dS sum once), dV 0.755 of the bounds.
def test_backward_q_and_dO_past_the_32_bit_dma_range(hip_ops):
    c, r = ac.case("rows257"), ac.ref_fwd_of("rows257")
    o16, lse32, (_, k, v, o, _, lse) = _bwd_inputs(c, r)
    b = ac.ref_bwd(c, o16, lse32, dk_bf16_p=False)
    qd = c.nh * c.hd
    ld = -(-(1 << 32) // (2 * c.T * 8)) * 8                     # the smallest multiple of 8 with T * ld * 2 >= 2^32
    assert c.T * ld * 2 >= 1 << 32 > c.T * (ld - 8) * 2 and ld >= 2 * qd
    buf = torch.empty(c.T, ld, dtype=BF16, device=DEV)
    q, do = buf[:, :qd], buf[:, qd:2 * qd]
    q.copy_(c.q)
    do.copy_(c.do)
    dq, dk, dv = hip_ops.attn_bwd(q, k, v, o, do, lse, *masks_dev(c), c.nh, c.nkv, c.S, c.hd, c.scale)
    check_bwd(c, r, b, dq, dk, dv, "bwd rows257 q / dO stride %d" % ld)
    for t, h in ((q, c.q), (k, c.k), (v, c.v), (o, o16), (do, c.do)):
        assert torch.equal(bits(t), bits(h)), "the backward wrote an input"


@pytest.mark.parametrize("name", ["causal-200", "tile-edges-64-32", "segments"])
def test_backward_zero_dO_rows_add_nothing(hip_ops, name):
    """Rows with dO == 0 contribute exact zeros (P^T dO = 0, dS = P (0 - 0) = 0): hiding them from every key leaves dK and dV bit for bit as they were."""
    c, r = ac.case(name), ac.ref_fwd_of(name)
    _, _, (q, k, v, o, do, lse) = _bwd_inputs(c, r)
    zero = (c.do.float() == 0).all(1)
    assert int(zero.sum()) >= 3
    args = lambda m: (q, k, v, o, do, lse, *[x.to(I32).to(DEV) for x in m], c.nh, c.nkv, c.S, c.hd, c.scale)
    _, dk, dv = hip_ops.attn_bwd(*args((c.pre, c.lo, c.hi)))
    hidden = (torch.where(zero, 0, c.pre), torch.where(zero, 1, c.lo), torch.where(zero, 0, c.hi))
    _, dk2, dv2 = hip_ops.attn_bwd(*args(hidden))
    assert torch.equal(bits(dk), bits(dk2)) and torch.equal(bits(dv), bits(dv2))


# tr1_attn_bwd_rope at head dim 128 into column views of one [T, q | k | v | 8 pad] buffer (n_slots == T): the rotation in the dQ kernel's epilogue and in
# attn_bwd_reduce_kernel<true> (QS > 1); causal-64 has QS == 1, where dK is rotated by the separate kernel after its bf16 rounding.
# Worst seen on MI355X: dQ 0.770 (long-prefix), dK 0.657 (rows257), dV 0.828 (causal-64) of the rotated bounds.
@pytest.mark.parametrize("name", ["causal-64", "causal-200", "rows257", "tile-edges-63-33", "prefix-only", "segments-128", "long-prefix"])
def test_backward_rope_folded_in(hip_ops, name):
    c, r = ac.case(name), ac.ref_fwd_of(name)
    assert c.T == c.S and c.hd == 128
    o16, lse32, (q, k, v, o, do, lse) = _bwd_inputs(c, r)
    cos, sin = ac.rope_tables(c.T, c.hd)
    b = ac.ref_bwd(c, o16, lse32, rope=(cos, sin))
    qd, kvd = c.nh * c.hd, c.nkv * c.hd
    buf = torch.full((c.T, qd + 2 * kvd + 8), SENT, dtype=BF16, device=DEV)
    dq, dk, dv = hip_ops.attn_bwd(q, k, v, o, do, lse, *masks_dev(c), c.nh, c.nkv, c.S, c.hd, c.scale, dq_out=buf[:, :qd], dk_out=buf[:, qd:qd + kvd],
                                  dv_out=buf[:, qd + kvd:qd + 2 * kvd], rope=(cos.to(DEV), sin.to(DEV)))
    check_bwd(c, r, b, dq, dk, dv, "bwd+rope %s" % name)
    assert bool((buf[:, qd + 2 * kvd:].float() == SENT).all()), "wrote outside the output views"
