"""The measurement behind DESIGN.md section 4v's timing (needs a HIP device): hip_ops.seg_pgd_step — one launch, 16 B per sample —
beside hip_ops.row_pgd_l2_step, the three-launch per-row L2 step it stands in for (32 B per sample), and beside
hip_ops.row_pgd_linf_step, a one-launch step with the same 16 B per sample and no reduction at all (the yardstick for what the
reductions cost), at the flagship batch shape, with HIP events.

The steps are warmed up, then timed in alternating blocks of `--iters` launches (one event pair per block, so the events'
own cost is spread over the block); the figure is the median block.  `--sets` rotates the launches over that many sets of
adv / grad / orig / out buffers: one set (132 MB at the default shape) fits the 256 MB Infinity Cache, four do not.  Prints one
line per configuration and one JSON line.

    python tools/snr_step_timing.py [--B 128 --T 64600 --iters 200 --blocks 15]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from audio_deepfake_adversarial_attacks_amd import hip_ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=128)
    ap.add_argument("--T", type=int, default=64_600)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=15)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no HIP device: this is a measurement, there is nothing to fall back to")
    dev = torch.device("cuda")
    B, T = args.B, args.T
    rho, alpha_rel, eps_div = 10.0 ** -1.5, 0.25, 1e-10
    result = {"B": B, "T": T, "iters": args.iters, "blocks": args.blocks}
    for sets in (1, 4):
        g = torch.Generator(device=dev).manual_seed(sets)
        bufs = []
        for _ in range(sets):
            orig = torch.rand(B, T, device=dev, generator=g)
            adv = (orig + (torch.rand(B, T, device=dev, generator=g) * 2 - 1) * 0.05).clamp(0, 1)
            grad = torch.randn(B, T, device=dev, generator=g) * 1e-3
            bufs.append((adv, grad, orig, torch.empty_like(adv)))
        c = torch.full((B,), -0.5, device=dev)
        eps_rows = hip_ops.snr_row_radius(bufs[0][2], c, rho)

        def seg(k):
            adv, grad, orig, out = bufs[k % sets]
            hip_ops.seg_pgd_step(adv, grad, orig, c, rho, alpha_rel, eps_div, out=out)

        def row(k):
            adv, grad, orig, out = bufs[k % sets]
            hip_ops.row_pgd_l2_step(adv, grad, orig, eps_rows, 0.0, alpha_rel, eps_div, out=out)

        def linf(k):
            adv, grad, orig, out = bufs[k % sets]
            hip_ops.row_pgd_linf_step(adv, grad, orig, eps_rows, 0.0, alpha_rel, out=out)

        steps = {"seg_pgd_step": seg, "row_pgd_l2_step": row, "row_pgd_linf_step": linf}
        for fn in steps.values():
            for k in range(50):
                fn(k)
        torch.cuda.synchronize()
        times = {name: [] for name in steps}
        for _ in range(args.blocks):
            for name, fn in steps.items():                       # alternating: all see the same machine
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for k in range(args.iters):
                    fn(k)
                b.record()
                b.synchronize()
                times[name].append(a.elapsed_time(b) * 1e3 / args.iters)
        for name, per_sample in (("seg_pgd_step", 16), ("row_pgd_l2_step", 32), ("row_pgd_linf_step", 16)):
            us = statistics.median(times[name])
            tbs = per_sample * B * T / (us * 1e-6) / 1e12
            print(f"sets={sets} {name}: median {us:.2f} us (min {min(times[name]):.2f}, max {max(times[name]):.2f}), "
                  f"{per_sample} B/sample -> {tbs:.2f} TB/s")
            result[f"{name}/sets{sets}/us"] = round(us, 3)
            result[f"{name}/sets{sets}/us_min"] = round(min(times[name]), 3)
            result[f"{name}/sets{sets}/us_max"] = round(max(times[name]), 3)
            result[f"{name}/sets{sets}/TBps"] = round(tbs, 3)
        del bufs
    print(json.dumps(result))


if __name__ == "__main__":
    main()
