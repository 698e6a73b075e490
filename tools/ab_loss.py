"""Every output of tr1_grpo_loss_ratio and tr1_grpo_policy_loss on the cases of tests/ratio_cases.py and tests/loss_family_cases.py, saved to a file: run
under two builds (TR1_HIP_LIB=..., a fresh process each) and compare the files to show that a kernel edit left every float where it was.
    python tools/ab_loss.py run a.pt;  TR1_HIP_LIB=tools/_var_ref.so python tools/ab_loss.py run b.pt;  python tools/ab_loss.py cmp a.pt b.pt
cmp holds every output to torch.equal (+0 == -0) with NaNs in the same places.  One exception: dlogp of the policy entry point at token level, where the two
former kernels rounded -w A c + beta dkl differently and the ratio kernel's form was kept; it is held to TOL_GRPO against the fp64 reference, largest difference printed."""
import itertools, os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import loss_family_cases as fc, ratio_cases as rc, vocab_cases as vc  # noqa: E402
SHAPES = ((1, 1), (3, 257), (8, 200), (64, 300))


def run(path):
    import time_r1_amd  # noqa: F401
    from time_r1_amd.ops import HipOps
    ops, out = HipOps("cuda:0"), {}
    dev = lambda c: {k: v.to(ops.device).contiguous() for k, v in c.items() if torch.is_tensor(v)}  # noqa: E731
    def ratio(tag, d, eps):
        for beta, ug, w, gs in itertools.product((0.0, 0.04), (False, True), (False, True), (1.0, 0.5)):
            r = ops.grpo_loss_ratio(d["logp"], d["old_logp"], d["ref_logp"], d["mask"], d["adv"], beta, ug, eps[0], eps[1], gs, tok_weight=d["tok_weight"] if w else None)
            out[("ratio", tag, eps, beta, ug, w, gs)] = [t.cpu() for t in r]
    for (G, C), eps in itertools.product(SHAPES, rc.EPS_PAIRS):
        ratio((G, C), dev(rc.ratio_case(G, C, eps)), eps)
        c = fc.family_case(G, C, eps)
        for tag, d in (("full", dev(c)), ("empty", dev(c["empty"]))):
            for norm, level, delta, beta, w in fc.settings():
                r = ops.grpo_policy_loss(d["logp"], d["old_logp"], d["ref_logp"], d["mask"], d["adv"], beta, norm, level, eps[0], eps[1], delta, 0.5,
                                         tok_weight=d["tok_weight"] if w else None)
                out[("policy", (G, C), tag, eps, norm, level, delta, beta, w)] = [t.cpu() for t in r]
    d = dev(rc.ratio_case(8, 200, rc.EPS_PAIRS[1]))
    d["mask"][1] = 0
    ratio("masked row", d, rc.EPS_PAIRS[1])
    d["mask"].zero_()
    ratio("masked grid", d, rc.EPS_PAIRS[1])
    torch.cuda.synchronize()
    torch.save(out, path)
    print("saved %d cases to %s" % (len(out), path))


def same(a, b):
    return torch.equal(a.isnan(), b.isnan()) and torch.equal(a[~a.isnan()], b[~b.isnan()])


def cmp(pa, pb):
    A, B = torch.load(pa), torch.load(pb)
    assert A.keys() == B.keys()
    n = {"ratio": [0, 0], "policy": [0, 0]}
    bad, worst, share = [], 0.0, 0.0
    for k in A:
        eq = [same(x, y) for x, y in zip(A[k], B[k])]
        n[k[0]][0] += 1
        n[k[0]][1] += all(eq)
        if all(eq):
            continue
        if k[0] == "policy" and k[5] == 0 and all(eq[1:]):      # token level: dlogp alone, against the fp64 reference
            (G, C), tag, eps, norm, level, delta, beta, w = k[1:]
            c = fc.family_case(G, C, eps)
            c = c["empty"] if tag == "empty" else c
            ref = fc.ref_policy_loss(c["logp"], c["old_logp"], c["ref_logp"], c["tok_weight"] if w else None, c["mask"], c["adv"], beta, norm, level, eps[0], eps[1], delta, 0.5)[0]
            worst = max(worst, float((A[k][0] - B[k][0]).abs().max()))
            share = max(share, vc.worst(A[k][0], ref, vc.TOL_GRPO)[0], vc.worst(B[k][0], ref, vc.TOL_GRPO)[0])
        else:
            bad.append(k)
    for name, (cases, equal) in n.items():
        print("%s entry point: %d cases, %d equal" % (name, cases, equal))
    print("policy entry point, token level: largest |dlogp difference| %.3g, worst share of TOL_GRPO against fp64 %.4f" % (worst, share))
    print("FAIL: %d cases differ where they may not: %s" % (len(bad), bad[:5]) if bad or share > 1.0 else "PASS")
    return 1 if bad or share > 1.0 else 0


if __name__ == "__main__":
    sys.exit(run(sys.argv[2]) if sys.argv[1] == "run" else cmp(sys.argv[2], sys.argv[3]))
