"""The measurement behind profiles/l0_step_timing.txt (needs a HIP device; run from the repository root): hip_ops.pgdl0_step next
to the sort-based eager formulation of the same arithmetic, which must agree with it bit for bit.  HIP events, B = 128,
T = 64 600, k in {64, 1024}, one hot buffer set, alternating rounds, no profiler; then the projection alone and apgdl1_step in
the same process for the per-pass reading; then l1_box_project and apgdl1_init, and the five search kernels at B = 1024
(profiles/row_search_refactor_timing.txt)."""
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
# the other two kernels with row_workgroup.h's digit_search that the lines above do not reach, then every search kernel at
# B = 1024: four rows per CU, where the kernels' occupancy (one or two resident rows per CU) can show
for label, fn in (("l1_box_project, u = x + N(0, 1), eps = 20", lambda: ops.l1_box_project(xd, u, 20.0, out=out)),
                  ("apgdl1_init (Philox), eps = 20", lambda: ops.apgdl1_init(xd, 20.0, seed=1, out=out))):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    rs = [timed(fn, 50) for _ in range(5)]
    print(f"{label}: min {min(rs):.1f} median {statistics.median(rs):.1f} max {max(rs):.1f} us")
del u, ut, out, c1
B8 = 8 * B
x8, g8 = xd.repeat(8, 1), gd.repeat(8, 1)
u8 = x8 + torch.randn(B8, T, device=dev)
out8 = torch.empty_like(x8)
step8, topk8 = torch.full((B8,), 20.0, device=dev), torch.full((B8,), 0.2, device=dev)
c8 = ops.apgdl1_init(x8, 20.0, seed=1)
p8 = ops.l0_box_project(x8, u8, 64)
for label, fn in ((f"B = {B8}: pgdl0_step, random gradient, k = 64", lambda: ops.pgdl0_step(p8, g8, x8, STEP, 64, out=out8)),
                  (f"B = {B8}: l0_box_project, u = x + N(0, 1), k = 64", lambda: ops.l0_box_project(x8, u8, 64, out=out8)),
                  (f"B = {B8}: apgdl1_step", lambda: ops.apgdl1_step(c8, g8, x8, step8, topk8, 20.0, out=out8)),
                  (f"B = {B8}: l1_box_project, u = x + N(0, 1), eps = 20", lambda: ops.l1_box_project(x8, u8, 20.0, out=out8)),
                  (f"B = {B8}: apgdl1_init (Philox), eps = 20", lambda: ops.apgdl1_init(x8, 20.0, seed=1, out=out8))):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    rs = [timed(fn, 10) for _ in range(5)]
    print(f"{label}: min {min(rs):.1f} median {statistics.median(rs):.1f} max {max(rs):.1f} us")
