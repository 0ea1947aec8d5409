"""The measurement behind profiles/l0_step_timing.txt (needs a HIP device; run from the repository root): hip_ops.pgdl0_step next
to the sort-based eager formulation of the same arithmetic, which must agree with it bit for bit.  HIP events, B = 128,
T = 64 600, k in {64, 1024}, one hot buffer set, alternating rounds, no profiler; then the projection alone and apgdl1_step in
the same process for the per-pass reading."""
import math, statistics, sys
sys.path.insert(0, ".")
import torch
from audio_deepfake_adversarial_attacks_amd import hip_ops as ops

dev = torch.device("cuda:0")
B, T = 128, 64_600
STEP = 0.15 * T
g = torch.Generator().manual_seed(1)
x = torch.rand(B, T, generator=g)
grad_rand = 1e-3 * torch.randn(B, T, generator=g)
x_tie = torch.full((B, T), 0.5)
grad_tie = 1e-3 * torch.sign(torch.randn(B, T, generator=g))
xd, gd, xtd, gtd = (t.to(dev) for t in (x, grad_rand, x_tie, grad_tie))


def eager(cur, grad, x, k, gn):
    u = cur + (STEP * grad) / (gn[:, None] + 1e-10)
    d = u - x
    c = torch.minimum(torch.maximum(d, -x), 1.0 - x)
    r = d - c
    s = d * d - r * r
    order = torch.sort(s, dim=1, descending=True, stable=True)[1]
    keep = torch.zeros_like(s, dtype=torch.bool)
    keep.scatter_(1, order[:, :k], True)
    return torch.where(keep, (x + c).clamp(0.0, 1.0), x)


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / n


print(f"device {torch.cuda.get_device_name(0)}")
for label, xs, cur, gr in (("random gradient, cur = the projected random start", xd, None, gd), ("tie input, cur = x = 0.5", xtd, xtd, gtd)):
    for k in (64, 1024):
        c0 = ops.l0_box_project(xs, xs + (torch.rand(B, T, device=dev) * 2 - 1), k) if cur is None else cur
        out = torch.empty_like(c0)
        got, stats = ops.pgdl0_step(c0, gr, xs, STEP, k, out=out, return_stats=True)
        want = eager(c0, gr, xs, k, stats[:, 0])
        torch.cuda.synchronize()
        ties_left = ((stats[:, 3] + 1) < T).sum().item()
        print(f"{label}, k = {k}: bit-identical to eager: {torch.equal(got, want)}; changed max {(got != xs).sum(dim=1).max().item()}; "
              f"gt min {stats[:, 2].min().item():.0f} max {stats[:, 2].max().item():.0f}; cut min {stats[:, 3].min().item():.0f}")
        kern = lambda: ops.pgdl0_step(c0, gr, xs, STEP, k, out=out)
        eag = lambda: eager(c0, gr, xs, k, stats[:, 0])
        for _ in range(5):
            kern(), eag()
        torch.cuda.synchronize()
        ks, es = [], []
        for _ in range(5):
            ks.append(timed(kern, 50)), es.append(timed(eag, 10))
        print(f"  pgdl0_step us/launch min {min(ks):.1f} median {statistics.median(ks):.1f} max {max(ks):.1f}")
        print(f"  eager sort us/launch min {min(es):.1f} median {statistics.median(es):.1f} max {max(es):.1f}   eager / kernel = {statistics.median(es) / statistics.median(ks):.1f}")
# the projection alone and apgdl1_step in the same process, for the per-pass reading
u = xd + torch.randn(B, T, device=dev)
ut = xtd + 0.25 * torch.sign(torch.randn(B, T, device=dev))
out = torch.empty_like(u)
for label, fn in (("l0_box_project, u = x + N(0, 1), k = 64 (12 passes)", lambda: ops.l0_box_project(xd, u, 64, out=out)),
                  ("l0_box_project, tie input, k = 64 (12 + 6 passes)", lambda: ops.l0_box_project(xtd, ut, 64, out=out)),
                  ("l0_box_project, tie input, k = T (12 passes, no cut)", lambda: ops.l0_box_project(xtd, ut, T, out=out))):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    rs = [timed(fn, 20) for _ in range(3)]
    print(f"{label}: {min(rs):.1f} - {max(rs):.1f} us")
step = torch.full((B,), 20.0, device=dev)
topk = torch.full((B,), 0.2, device=dev)
c1 = ops.apgdl1_init(xd, 20.0, seed=1)
fn = lambda: ops.apgdl1_step(c1, gd, xd, step, topk, 20.0, out=out)
for _ in range(5):
    fn()
torch.cuda.synchronize()
rs = [timed(fn, 50) for _ in range(5)]
print(f"apgdl1_step (same process, for comparison): min {min(rs):.1f} median {statistics.median(rs):.1f} max {max(rs):.1f} us")
