"""GPU: the optimizer-side HIP kernels (csrc/optim.hip, tr1_wgrad_f32_sumsq of csrc/gemm.hip) against the fp64 references of tests/optim_cases.py.

Cases, references and the derivation of every bound live in optim_cases.py; tests/test_optim_side_ref.py shows on the CPU that the fp32 oracle
sits at or below 0.75 of every bound on the same cases.  Every check prints the worst figure it saw (`pytest -s`, lines starting with OBS).

A. adamw_step: ONE step from a given fp32 state against fp64, at the trainer's settings (lr 1e-6 .. 1e-3, steps 1 .. 100 000), over the lengths
   that enter the grid-stride loop once, twice and three times, on views at every 4-byte offset (what AdamWFlat.step and _step_sharded pass).
   Out of scope: non-finite gradients (NaN, as clip_grad_norm_); `1.f - lr * wd` is exactly 1 in fp32 when lr * wd < 2^-25 (lr 1e-6, wd 0.01),
   which is torch's own fp32 behaviour and lies inside the ulp term of the bound.
B. The grad-norm pieces on integer data whose fp32 sum is exact in any order: bit equality with the count, no tolerance.
C. One launch past 2^31 elements of each kernel the 7B step runs at that size.

Checked against edited copies of optim.hip (none of them kept): the AdamW tail loop starting at n4 * 4 + 1 fails test_adamw_step (every case with a
tail); the same edit in the fp32 sum fails test_sumsq_accum_exact (planted tail element) and the 2^31 + 5 case; dropping `/ bc1` fails test_adamw_step
at steps 1 .. 7; zero_grad ignored fails test_adamw_step_keeps_the_gradient_and_reads_the_bf16_form; 32-bit indices in the bf16 sum fail
test_sumsq_accum_beyond_2_31_elements[bf16].  Dropping only the int64 casts of the grid stride changes no value at any length (the stride is at most
4096 * 256 and is added to a 64-bit index of 16-byte groups), so no test can tell it apart.
"""
import functools

import pytest
import torch

import optim_cases as oc

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
F32 = torch.float32
DEV = "cuda:0"

CASES = oc.adamw_cases()
BY_NAME = {c["name"]: c for c in CASES}


def scalar(v=oc.OUT0):
    return torch.tensor([v], dtype=F32, device=DEV)


# ------------------------------------------------------------------------------------------------------------ A. adamw_step
# Bounds (optim_cases.py): |p' - ref| <= 2 ulp32(max(|p|, |ref|)) + 26u (lr / bc1)(|b1 m| + |(1 - b1) gg|) / denom, |m' - ref| <= 9u (|b1 m| + |(1 - b1) gg|),
# |v' - ref| <= 17u ref, u = 2^-24.
# Worst seen on MI355X over the 33 cases, as a share of the bound: p 0.428 (n 12 582 913), m 0.345 (clip-just-above), v 0.357 (n 12 582 913);
# the g16 form and zero_grad=False: p 0.422, m 0.216, v 0.205.  The fp32 oracle on the CPU: p 0.647, m 0.253, v 0.254.
@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_adamw_step(hip_ops, case):
    out = oc.run_adamw(hip_ops, case, DEV)
    r = oc.check_adamw(out, case, 1.0, DEV)
    print("OBS adamw %-40s p %.3f  m %.3f  v %.3f of the bound" % (case["name"], r["p"], r["m"], r["v"]))
    assert int((oc.bits32(out["g"]) != 0).sum()) == 0, "zero_grad=True leaves +0.0 everywhere"


@pytest.mark.parametrize("name", ["lr1e-6-wd0.01-step2-trained", "clip-gm0.125", "n1", "n3", "n5", "n1023", "offs123057", "offs301273", "offs000011",
                                  "offs333333-n%d" % (oc.GRID_PASS + 3)])
def test_adamw_step_keeps_the_gradient_and_reads_the_bf16_form(hip_ops, name):
    """zero_grad=False leaves g bit for bit (fp32 and g16 forms: the lazy-zero plan relies on it for the large matrices); the g16 form equals the fp32 form
    fed g16.float() bit for bit, and never reads the fp32 accumulator."""
    case = BY_NAME[name]
    a = oc.run_adamw(hip_ops, case, DEV, zero_grad=False)
    assert torch.equal(oc.bits32(a["g"]), oc.bits32(a["g_before"])), "fp32 form, zero_grad=False: g changed"
    ra = oc.check_adamw(a, case, 1.0, DEV)
    b = oc.run_adamw(hip_ops, case, DEV, zero_grad=False, use_g16=True)
    assert torch.equal(oc.bits32(b["g"]), oc.bits32(b["g_before"])), "g16 form, zero_grad=False: the fp32 accumulator changed"
    rb = oc.check_adamw(b, case, 1.0, DEV)
    p, m, v, g, ss = oc.adamw_inputs(case)
    c = oc.run_adamw(hip_ops, case, DEV, inputs=(p, m, v, g.to(BF16).float(), ss))
    d = oc.run_adamw(hip_ops, case, DEV, use_g16=True)
    for k in ("p", "m", "v"):
        assert torch.equal(oc.bits32(b[k]), oc.bits32(c[k])) and torch.equal(oc.bits32(d[k]), oc.bits32(c[k])), "g16 form differs from the fp32 form in " + k
    assert torch.equal(oc.bits16(b["p16"]), oc.bits16(c["p16"])) and torch.equal(oc.bits16(d["p16"]), oc.bits16(c["p16"]))
    assert int((oc.bits32(d["g"]) != 0).sum()) == 0 and int((oc.bits32(c["g"]) != 0).sum()) == 0
    print("OBS adamw keep-gradient %-26s fp32 form p %.3f m %.3f v %.3f, g16 form p %.3f m %.3f v %.3f of the bound" % (
        name, ra["p"], ra["m"], ra["v"], rb["p"], rb["m"], rb["v"]))


@pytest.mark.parametrize("rot", oc.BF16_ROTATIONS)
def test_adamw_bf16_rounding(hip_ops, rot):
    """lr = wd = 0 on an empty state leaves the master weights bit for bit, and the bf16 copy is round-to-nearest-even of each pattern of the table in
    the vector body (pack2bf) and in the scalar tail (f2bf): ties both ways, a carry into the exponent, -0.0, the edge of bf16 max / inf, denormals."""
    p, want = oc.bf16_case(rot)
    case = oc._case("bf16-rot%d" % rot, oc.BF16_N, lr=0.0, wd=0.0, step=1, clip=None, gm=1.0)
    z = torch.zeros(oc.BF16_N)
    for offs in ((0, 0, 0, 0, 0, 0), (1, 1, 1, 1, 3, 1)):
        out = oc.run_adamw(hip_ops, dict(case, offs=offs), DEV, inputs=(p, z, z.clone(), z.clone(), None))
        bad = (oc.bits32(out["p"]).cpu() != oc.bits32(p)).nonzero().flatten().tolist()
        assert not bad, "master weights changed at %s: %s" % (bad[:8], [hex(int(oc.bits32(p)[i]) & 0xFFFFFFFF) for i in bad[:8]])
        got = oc.bits16(out["p16"]).cpu()
        bad = (got != want).nonzero().flatten().tolist()
        assert not bad, "bf16 copy wrong at %s: fp32 %s -> %s, want %s" % (bad[:8], [hex(int(oc.bits32(p)[i]) & 0xFFFFFFFF) for i in bad[:8]],
                                                                         [hex(int(got[i]) & 0xFFFF) for i in bad[:8]], [hex(int(want[i]) & 0xFFFF) for i in bad[:8]])
        print("OBS adamw bf16 rounding rot %d offs %s: %d master weights and %d bf16 patterns bit-exact" % (rot, offs[:1] + offs[4:5], oc.BF16_N, oc.BF16_N))


# ------------------------------------------------------------------------------------------------------------ B. exact sums
# No tolerance anywhere in this section: the data are integers whose squares sum to less than 2^24, `out` starts at 5 and must end at 5 + the count.
@pytest.mark.parametrize("name,dtype,n,off", oc.sumsq_cases(), ids=[c[0] for c in oc.sumsq_cases()])
def test_sumsq_accum_exact(hip_ops, name, dtype, n, off):
    x = oc.int_data(n, 100 + n % 97 + off, dtype)
    s = oc.exact_sumsq(x)
    (buf,), (vw,) = oc.views([x], [off], DEV)
    out = scalar()
    hip_ops.sumsq_accum(vw, out)
    assert float(out) == oc.OUT0 + s, "%s: got %r, the count is %d + %d" % (name, float(out), oc.OUT0, s)
    assert oc.sentinels_intact(buf, off, n) and torch.equal(vw.cpu(), x), "sumsq_accum does not write its input"
    vw.zero_()
    pos = oc.planted_positions(n, dtype)
    for q in pos:
        vw[q] = 1.0
        out = scalar()
        hip_ops.sumsq_accum(vw, out)
        vw[q] = 0.0
        assert float(out) == oc.OUT0 + 1.0, "%s: a single 1 at element %d of %d was counted as %r" % (name, q, n, float(out) - oc.OUT0)
    print("OBS sumsq_accum %-28s exact: %d + %d, %d planted positions" % (name, oc.OUT0, s, len(pos)))


@pytest.mark.parametrize("n", oc.PARTIALS_N)
def test_sumsq_partials_accum_exact(hip_ops, n):
    buf, s = oc.partials_case(n)
    d = buf.to(DEV)
    out = scalar()
    hip_ops.sumsq_partials_accum(d, n, out)
    assert float(out) == oc.OUT0 + s, "n %d: got %r, the count is %d + %d" % (n, float(out), oc.OUT0, s)
    got = d.cpu()
    assert torch.equal(oc.bits32(got[:n]), oc.bits32(buf[:n])), "partials[:n] changed"
    assert torch.equal(oc.bits32(got[n + 256:]), oc.bits32(buf[n + 256:])), "the sentinel behind the 256 scratch floats changed"
    out2 = scalar()
    hip_ops.sumsq_partials_accum(d, n, out2)               # stale scratch from the first call must not enter the second
    assert float(out2) == oc.OUT0 + s
    print("OBS sumsq_partials_accum n %-7d exact: %d + %d" % (n, oc.OUT0, s))


@pytest.mark.parametrize("case", oc.periodic_cases(), ids=[c[0] for c in oc.periodic_cases()])
def test_sumsq_and_zero_ranges_periodic_exact(hip_ops, case):
    name, base, stride, count, ranges = case
    for kind in ("in", "out", "mixed"):
        arena, mask, s = oc.periodic_arena(case, kind)
        d = arena.to(DEV)
        out = scalar()
        hip_ops.sumsq_ranges_periodic(d, base, stride, count, ranges, out)
        assert float(out) == oc.OUT0 + s, "%s/%s: got %r, the count is %d + %d" % (name, kind, float(out), oc.OUT0, s)
        assert torch.equal(oc.bits32(d.cpu()), oc.bits32(arena)), "the sum does not write the arena"
        print("OBS sumsq_ranges_periodic %-16s %-5s exact: %d + %d" % (name, kind, oc.OUT0, s))
    gen = torch.Generator().manual_seed(9)
    arena = torch.randn(arena.numel(), generator=gen) - 0.0
    arena[::7] = -0.0
    d = arena.to(DEV)
    hip_ops.zero_ranges_periodic(d, base, stride, count, ranges)
    got = oc.bits32(d.cpu())
    assert torch.equal(got[~mask], oc.bits32(arena)[~mask]), "%s: an element outside the ranges changed" % name
    assert int((got[mask] != 0).sum()) == 0, "%s: an element inside the ranges is not +0.0" % name
    print("OBS zero_ranges_periodic %-16s exact: %d elements +0.0, %d untouched" % (name, int(mask.sum()), int((~mask).sum())))


@functools.lru_cache(maxsize=2)
def _wgrad_case(N, K, Mp, T):
    return oc.wgrad_case(N, K, Mp, T)


def _operands(dy, x, T, kmajor):
    """dY^T [N, Mp] and the second operand (X [Mp, K] as stored, rows T.. unreadable, or X^T [K, Mp], zero-padded), as views of larger buffers whose
    neighbouring rows and columns hold values the kernel must not read."""
    dyt_buf, dyt = oc.framed(dy.t().contiguous().to(BF16), fill=oc.PLANT_BIG, dev=DEV)
    if kmajor:
        b_buf, b = oc.framed(x.to(BF16), fill=oc.PLANT_BIG, dev=DEV)
    else:
        xt = torch.zeros(x.shape[1], x.shape[0])
        xt[:, :T] = x[:T].t()
        b_buf, b = oc.framed(xt.to(BF16), fill=oc.PLANT_BIG, dev=DEV)
    return (dyt_buf, b_buf), dyt, b


@pytest.mark.parametrize("kmajor", [False, True], ids=["nt", "kmajor"])
@pytest.mark.parametrize("shape", oc.WGRAD_SHAPES, ids=["%dx%d-tile%d" % (s[0], s[1], s[4]) for s in oc.WGRAD_SHAPES])
def test_wgrad_sumsq_exact(hip_ops, shape, kmajor):
    """The weight-gradient epilogue on integer data: the gradient equals the fp64 product exactly, the per-wave sums add up to the sum of squares of
    what was stored bit for bit (overwrite and accumulate), the wire copy is its bf16 rounding; partial tiles in both directions at every tile
    height; padding rows, neighbouring rows and the slots of `part` outside [offset, offset + n) are neither read nor written."""
    N, K, Mp, T, bm = shape
    dy, x, gw0, over, acc = _wgrad_case(N, K, Mp, T)
    keep, dyt, b = _operands(dy, x, T, kmajor)
    bound = hip_ops.wgrad_sumsq_partials(N, K)
    n_want = 8 * ((N + bm - 1) // bm) * ((K + 255) // 256)
    for accumulate, ref in ((False, over), (True, acc)):
        part0 = oc.fill_sentinel(torch.empty(oc.WGRAD_OFFSET + bound + 256 + 16, dtype=F32))
        part = part0.to(DEV)
        gw_buf, gw = oc.framed(gw0 if accumulate else torch.full((N, K), 7.0), cols=4, dev=DEV)
        wire_buf, wire = oc.framed(torch.full((N, K), 3.0).to(BF16), dev=DEV)
        n = hip_ops.wgrad_sumsq(dyt, b, gw, accumulate, part, oc.WGRAD_OFFSET, b_kmajor=kmajor, b_rows=T, wire=wire)
        torch.cuda.synchronize()
        what = "%dx%d %s %s" % (N, K, "kmajor" if kmajor else "nt", "accumulate" if accumulate else "overwrite")
        assert 0 < n <= bound and n == n_want, "%s: %d partial sums, the replayed tile choice gives %d (bound %d)" % (what, n, n_want, bound)
        got = gw.cpu()
        assert torch.isfinite(got).all(), what + ": the kernel read a padding row / a neighbouring row"
        assert torch.equal(got.double(), ref), what + ": gradient differs from the exact product in %d places" % int((got.double() != ref).sum())
        assert torch.equal(wire.cpu(), got.to(BF16)), what + ": wire copy != bf16(gradient)"
        pc = part.cpu()
        s_got, s_ref = float(pc[oc.WGRAD_OFFSET: oc.WGRAD_OFFSET + n].double().sum()), oc.exact_sumsq(ref)
        assert s_got == float(s_ref), "%s: the partial sums add up to %r, the stored values' squares to %d" % (what, s_got, s_ref)
        untouched = torch.ones(pc.numel(), dtype=torch.bool)
        untouched[oc.WGRAD_OFFSET: oc.WGRAD_OFFSET + n] = False
        assert torch.equal(oc.bits32(pc[untouched]), oc.bits32(part0[untouched])), what + ": a slot of part outside [offset, offset + n) changed"
        assert oc.frame_intact(gw_buf, N, K) and oc.frame_intact(wire_buf, N, K), what + ": wrote outside the gradient / wire view"
        print("OBS wgrad_sumsq %-40s exact: sum of squares %d in %d partial sums" % (what, s_ref, n))


# rtol 1e-4: the project's own tolerance for a sum of squares.  Worst seen on MI355X: 8.9e-8 relative (0.0009 of it).
@pytest.mark.parametrize("kmajor", [False, True], ids=["nt", "kmajor"])
def test_wgrad_sumsq_random_data_with_a_dominant_element(hip_ops, kmajor):
    """Random bf16 operands; one element of the gradient holds about half of the total, at the last valid row and column, at the first row of the last
    (partial) row tile, and at the corner of the first tile: dropped or counted twice, the sum is off by a third or more."""
    N, K, Mp, T = 1000, 776, 128, 100
    bm = oc.wgrad_tile_rows(N, K, kmajor)
    gen = torch.Generator().manual_seed(21)
    dy, x = torch.zeros(Mp, N), torch.zeros(Mp, K)
    dy[:T] = (torch.randn(T, N, generator=gen) * 0.1).to(BF16).float()
    x[:T] = (torch.randn(T, K, generator=gen) * 0.5).to(BF16).float()
    prod = dy[:T].double().t() @ x[:T].double()
    x[T:] = float("inf")
    total = float((prod ** 2).sum())
    keep, dyt, b = _operands(dy, x, T, kmajor)
    last_tile = ((N + bm - 1) // bm - 1) * bm
    assert 0 < last_tile < N and N - last_tile < bm
    for r, c in ((N - 1, K - 1), (last_tile, K // 2), (0, 0)):
        gw0 = torch.zeros(N, K)
        gw0[r, c] = total ** 0.5
        gw = gw0.clone().to(DEV)
        part = torch.zeros(hip_ops.wgrad_sumsq_partials(N, K) + 256 + 16, device=DEV)
        n = hip_ops.wgrad_sumsq(dyt, b, gw, True, part, 0, b_kmajor=kmajor, b_rows=T)
        assert n > 0
        stored = gw.cpu().double()
        ref = float((stored ** 2).sum())
        assert 0.3 < stored[r, c] ** 2 / ref < 0.7
        got = float(part[:n].double().sum())
        rel = abs(got - ref) / ref
        print("OBS wgrad_sumsq random %s planted (%d, %d): sum %.6e, of the stored values %.6e, rel err %.2e (rtol %g)" % (
            "kmajor" if kmajor else "nt", r, c, got, ref, rel, oc.TOL_SUMSQ_RTOL))
        assert rel <= oc.TOL_SUMSQ_RTOL
        assert float((stored - (gw0.double() + prod)).abs().max()) <= 1e-5 * (total ** 0.5) + 1e-4, "gradient far from the fp64 product"


def test_grad_norm_composition_equals_one_pass(hip_ops):
    """A synthetic arena - prefix, 4 periods of (small, matrix, small, matrix, small), suffix, all integer-valued - put together the way
    AdamWFlat._norm_from_sink does (epilogue partial sums, prefix and suffix, periodic small ranges) equals one sumsq_accum over the arena bit for bit."""
    from time_r1_amd.optim import AdamWFlat
    prefix, suffix, count, T = 1000, 516, 4, 64
    mats, smalls = ((512, 256), (640, 264)), (36, 260, 8)
    keep, pos = [], smalls[0]
    for (N, K), s in zip(mats, smalls[1:]):
        keep.append((pos, pos + N * K))
        pos += N * K + s
    stride = pos
    n = prefix + count * stride + suffix
    lz = dict(base=prefix, stride=stride, count=count, keep=keep)
    o = AdamWFlat.__new__(AdamWFlat)
    o.lazy_zero, o.lazy_zero_ok = lz, None
    spans, small = o._zero_spans(n)
    assert bool((oc.zero_plan_cover(n, spans, small, lz) == 1).all())
    arena = oc.int_data(n, 31, budget=1 << 30)
    arena[arena == 0] = 1.0
    for l in range(count):
        for a, b in keep:
            arena[prefix + l * stride + a: prefix + l * stride + b] = 1.0e4        # overwritten by the weight gradients below
    grad = arena.to(DEV)
    need = sum(hip_ops.wgrad_sumsq_partials(N, K) for N, K in mats) * count
    part = torch.zeros(need + 512, device=DEV)
    ntot = 0
    for l in range(count):
        for j, ((N, K), (a, b)) in enumerate(zip(mats, keep)):
            dy = oc._sparse_ints((T, N), 40 + 2 * l + j, 0.035)
            x = oc._sparse_ints((T, K), 60 + 2 * l + j, 0.035)
            kmajor = bool(j)
            bb = x if kmajor else x.t().contiguous()
            gw = grad[prefix + l * stride + a: prefix + l * stride + b].view(N, K)
            k = hip_ops.wgrad_sumsq(dy.t().contiguous().to(BF16).to(DEV), bb.to(BF16).to(DEV), gw, False, part, ntot, b_kmajor=kmajor, b_rows=T)
            assert k > 0
            ntot += k
            assert torch.equal(gw.cpu().double(), dy.double().t() @ x.double())
    assert ntot <= need
    lo, hi = lz["base"], lz["base"] + stride * count
    out = scalar()
    hip_ops.sumsq_partials_accum(part, ntot, out)
    for x, y in ((0, lo), (hi, n)):
        hip_ops.sumsq_accum(grad[x:y], out)
    hip_ops.sumsq_ranges_periodic(grad, lz["base"], stride, count, small, out)
    whole = scalar()
    hip_ops.sumsq_accum(grad, whole)
    s = oc.exact_sumsq(grad.cpu())
    print("OBS grad-norm composition: pieces %r, one pass %r, the count %d + %d" % (float(out), float(whole), oc.OUT0, s))
    assert torch.equal(oc.bits32(out), oc.bits32(whole)) and float(whole) == oc.OUT0 + s


# ------------------------------------------------------------------------------------------------------------ C. beyond 2^31 elements
# One launch each; everything is built on the device.  On the MI355X run (288 GB) none of the three was skipped for memory: the two sums were exact (5 + 14, 5 + 30),
# exactly 3 elements of p, m and v changed (p 0.104, m 0.097, v 0.071 of the bounds of A), the bf16 copy and the zeroed gradient held everywhere.
CHUNK = 1 << 27


def _need(gib, what):
    torch.cuda.empty_cache()            # blocks the caching allocator still holds for earlier tests do not count as free
    free = torch.cuda.mem_get_info(0)[0] / 2.0 ** 30
    if free < gib:
        pytest.skip("%s needs %.0f GiB of free device memory, %.0f GiB are free" % (what, gib, free))


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_sumsq_accum_beyond_2_31_elements(hip_ops, dtype):
    n = (1 << 31) + 5 if dtype == F32 else (1 << 32) + 11
    _need(12, "sumsq_accum on %d elements" % n)
    x = torch.zeros(n, dtype=dtype, device=DEV)
    plant = {(1 << 31) - 1: 1.0, 1 << 31: 2.0, n - 1: 3.0}
    if dtype == BF16:
        plant[1 << 32] = 4.0
    for q, val in plant.items():
        x[q] = val
    out = scalar()
    hip_ops.sumsq_accum(x, out)
    s = sum(int(v * v) for v in plant.values())
    print("OBS sumsq_accum %s n %d: got %r, the count is %d + %d" % ("f32" if dtype == F32 else "bf16", n, float(out), oc.OUT0, s))
    assert float(out) == oc.OUT0 + s
    del x
    torch.cuda.empty_cache()


def test_adamw_step_beyond_2_31_elements(hip_ops):
    """p constant, g zero except at 2^31 - 1, 2^31 and n - 1, no history, wd = 0: exactly the planted elements change, within the bounds of A; everything
    else keeps its bits; the bf16 copy is the rounding of the master weights; the gradient is zeroed."""
    n = (1 << 31) + 5
    _need(48, "adamw_step on %d elements" % n)
    lr, step, p0 = oc.f32(1e-3), 1, 0.5
    plant = {(1 << 31) - 1: 0.01, 1 << 31: -0.02, n - 1: 0.03}
    p = torch.full((n,), p0, dtype=F32, device=DEV)
    m, v, g = (torch.zeros(n, dtype=F32, device=DEV) for _ in range(3))
    p16 = torch.zeros(n, dtype=BF16, device=DEV)
    for q, val in plant.items():
        g[q] = val
    hip_ops.adamw_step(p, m, v, g, p16, lr, oc.B1, oc.B2, oc.EPS, 0.0, step, sumsq=None, max_norm=0.0, grad_mult=1.0, zero_grad=True)
    changed = {"p": 0, "m": 0, "v": 0, "g": 0, "p16": 0}
    for a in range(0, n, CHUNK):
        b = min(n, a + CHUNK)
        changed["p"] += int((p[a:b] != p0).sum())
        changed["m"] += int((m[a:b] != 0).sum())
        changed["v"] += int((v[a:b] != 0).sum())
        changed["g"] += int((oc.bits32(g[a:b]) != 0).sum())
        changed["p16"] += int((oc.bits16(p16[a:b]) != oc.bits16(p[a:b].to(BF16))).sum())
    idx = torch.tensor(sorted(plant), device=DEV)
    got = [t[idx].cpu() for t in (p, m, v)]
    del p, m, v, g, p16
    torch.cuda.empty_cache()
    k = len(plant)
    gp = torch.tensor([plant[q] for q in sorted(plant)], dtype=F32)
    ref = oc.ref_adamw(torch.full((k,), p0), torch.zeros(k), torch.zeros(k), gp, lr, 0.0, step)
    r = oc.adamw_ratios(got[0], got[1], got[2], ref)
    print("OBS adamw n %d: changed %s; planted elements p %.3f m %.3f v %.3f of the bound" % (n, changed, r["p"], r["m"], r["v"]))
    assert changed == {"p": k, "m": k, "v": k, "g": 0, "p16": 0}
    assert bool((got[0] != p0).all()) and max(r.values()) <= 1.0
