"""The measurement behind DESIGN.md's randomized-smoothing section (needs a HIP device): the noise fill of torchattacks.Smoothing
beside an eager formulation of the same fill, its two floors, its error against a float64 twin, and its share of a certify run.

    smooth_noise(x -> (ns, B, T))   against   x + sigma * torch.randn(ns, B, T)
                                              model: 4 B read + 4 ns B written per sample; the eager fill also writes and
                                              re-reads the noise and the scaled noise (16 B per copy sample)

Method and output format are tools/universal_probe.py's (its `timed_pairs`): the versions are warmed up, then timed in alternating
blocks of `--iters` launches, a block being one replay of a hipGraph of those launches, so the window holds device time only;
median block, min .. max over the blocks; hot (one set of buffers: x stays in the cache, the ns output slots of 33 MB each
do not fit beside each other).

The floors.  STORE: 4 ns B per sample against the 8 TB/s HBM peak (and against universal_apply's recorded 4.28 TB/s, the
streaming yardstick of profiles/universal_probe.txt).  VALU: the instructions per quad of samples in the slot loop of the
vector-route kernel, counted in the code object's disassembly (`--valu`, `--trans`: hipcc --cuda-device-only -S on
csrc/smooth.hip with build.py's flags, one in_row block of the loop: 162 vector instructions of which 8 are v_log / v_sqrt /
v_sin / v_cos; 34 of the 154 others are the 32-bit integer multiplies of the Philox rounds, priced here like an add), at
2 cycles per plain wave64 instruction and 4 per transcendental on each of 1024 SIMDs at 2.4 GHz.

`--error` measures max |out - twin64| / sigma on a (16, 65 536), 8-slot fill against tests/smooth_cpu_ops.smooth_noise_np's
float64 form: the figure tests/test_gpu_smooth.py's tolerance is twice of.

`--loop N` adds one certify run over N synthetic utterances on LCNN (`--certify 0.05 --synthetic N`, NO_ATTACK) with
`--samples` / `--select` copies: utterances / s and the share of the run's wall time the two kernels' launches take (HIP events
round every launch, `hip_ops.start_profile`) — the rest is the forward of the copies.

    python tools/smooth_probe.py [--B 128 --T 64600 --ns 8 --iters 24 --blocks 15 --error --loop 128] [--out profiles/smooth_noise_timing.txt]"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from audio_deepfake_adversarial_attacks_amd import hip_ops  # noqa: E402
from universal_probe import HBM_PEAK, timed_pairs  # noqa: E402  (tools/ is the script's directory)

YARDSTICK_TBPS = 4.28      # universal_apply, eight buffer sets, profiles/universal_probe.txt
SIMDS, CLOCK_HZ, CYC_PLAIN, CYC_TRANS = 1024, 2.4e9, 2.0, 4.0


def error_against_twin(dev, sigma=0.05, seed=7, offset=3):
    import numpy as np
    from tests import smooth_cpu_ops as S
    B, T, ns = 16, 65_536, 8
    x = torch.rand(B, T, generator=torch.Generator().manual_seed(11)) * 2.0 - 1.0
    out = hip_ops.smooth_noise(x.to(dev), sigma, seed, offset, s0=0, ns=ns).cpu().numpy().astype(np.float64)
    twin = S.smooth_noise_np(x, sigma, seed, offset, 0, ns, dtype=np.float64)
    twin32 = S.smooth_noise_np(x, sigma, seed, offset, 0, ns, dtype=np.float32).astype(np.float64)
    return (float(np.max(np.abs(out - twin))) / float(np.float32(sigma)), float(np.max(np.abs(twin32 - twin))) / float(np.float32(sigma)),
            float(np.max(np.abs(out))))


def loop_figures(n_utt, batch, T, samples, select):
    from audio_deepfake_adversarial_attacks_amd.datasets.synthetic import SyntheticDetectionDataset
    from audio_deepfake_adversarial_attacks_amd.evaluation import generate_attacks
    cfg = {"data": {"seed": 42}, "checkpoint": {"path": ""},
           "model": {"name": "lcnn", "parameters": {"frontend_algorithm": ["lfcc"], "input_channels": 1}}}

    def run(n, profile):
        data = SyntheticDetectionDataset(n, num_samples=T)
        if profile:
            hip_ops.start_profile("smooth_noise", "smooth_tally")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rep = generate_attacks([None, None, None], cfg, "cuda", batch_size=batch, dataset=data, shuffle=False, num_workers=0,
                               certify=0.05, certify_samples=samples, certify_select=select)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        ms = hip_ops.stop_profile() if profile else {}
        return rep, wall, ms

    run(batch, False)                                                  # one batch: warms kernels, plans and allocator up
    rep, wall, _ = run(n_utt, False)                                   # the rate, without event brackets
    _, wall_p, ms = run(n_utt, True)
    kernels = {k: sum(v) / 1e3 for k, v in ms.items()}
    return {"loop/utterances": n_utt, "loop/samples": samples, "loop/select": select, "loop/utt_per_s": round(n_utt / wall, 2),
            "loop/wall_s": round(wall, 2), "loop/profiled_wall_s": round(wall_p, 2),
            "loop/noise_s": round(kernels.get("smooth_noise", 0.0), 4), "loop/tally_s": round(kernels.get("smooth_tally", 0.0), 5),
            "loop/kernel_share": round(sum(kernels.values()) / wall_p, 4),
            "loop/certified/abstained": rep["certified/abstained"], "loop/certified/accuracy": rep["certified/accuracy"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=128)
    ap.add_argument("--T", type=int, default=64_600)
    ap.add_argument("--ns", type=int, default=8)
    ap.add_argument("--iters", type=int, default=24)
    ap.add_argument("--blocks", type=int, default=15)
    ap.add_argument("--valu", type=int, default=162, help="vector instructions per quad of samples in the slot loop (disassembly)")
    ap.add_argument("--trans", type=int, default=8, help="of them transcendental (v_log, v_sqrt, v_sin, v_cos)")
    ap.add_argument("--error", action="store_true")
    ap.add_argument("--loop", type=int, default=0, metavar="N")
    ap.add_argument("--samples", type=int, default=200)
    ap.add_argument("--select", type=int, default=50)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "smooth_noise_timing.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no HIP device: this is a measurement, there is nothing to fall back to")
    dev = torch.device("cuda")
    B, T, ns = args.B, args.T, args.ns
    seed, sigma = 0x1234567887654321, 0.05
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    result = {"B": B, "T": T, "ns": ns, "iters": args.iters, "blocks": args.blocks, "window": "graph replay"}
    if args.error:
        err, twin_err, top = error_against_twin(dev)
        result.update({"error/max_over_sigma": err, "error/twin32_max_over_sigma": twin_err})
        say(f"(16, 65536) x 8 slots, sigma 0.05: max |out - twin64| / sigma = {err:.3e} (the float32 libm twin against the same "
            f"twin64: {twin_err:.3e}); max |out| = {top:.4f}")
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.rand(B, T, device=dev, generator=g) - 0.5
    slots = torch.empty(ns, B, T, device=dev)

    def fill(k):
        hip_ops.smooth_noise(x, sigma, seed, k * ns, s0=0, ns=ns, out=slots)

    def fill_eager(k):
        torch.add(x, sigma * torch.randn(ns, B, T, device=dev), out=slots)

    times = timed_pairs({"smooth_noise": fill, "eager_fill": fill_eager}, args.iters, args.blocks, True)
    med = {name: statistics.median(t) for name, t in times.items()}
    per_sample = 4 + 4 * ns
    for name, t in times.items():
        tbs = per_sample * B * T / (med[name] * 1e-6)
        say(f"{name}: median {med[name]:.2f} us (min {min(t):.2f}, max {max(t):.2f}) = {med[name] / ns:.2f} us per slot, "
            f"{per_sample} B/sample -> {tbs / 1e12:.2f} TB/s = {100 * tbs / HBM_PEAK:.0f} % of HBM peak, "
            f"{tbs / 1e12 / YARDSTICK_TBPS:.2f} of the yardstick")
        result[f"{name}/us"], result[f"{name}/us_min"], result[f"{name}/us_max"] = round(med[name], 3), round(min(t), 3), round(max(t), 3)
    say(f"eager_fill / smooth_noise: {med['eager_fill'] / med['smooth_noise']:.2f}x")
    store_peak = 4 * ns * B * T / HBM_PEAK * 1e6
    store_yard = 4 * ns * B * T / (YARDSTICK_TBPS * 1e12) * 1e6
    cycles_per_quad = (args.valu - args.trans) * CYC_PLAIN + args.trans * CYC_TRANS       # per wave64 instruction stream
    valu = ns * B * ((T + 3) // 4) * cycles_per_quad / 64 / SIMDS / CLOCK_HZ * 1e6
    floor = max(store_peak, valu)
    result.update({"floor/store_peak_us": round(store_peak, 2), "floor/store_yardstick_us": round(store_yard, 2),
                   "floor/valu_us": round(valu, 2), "over_larger_floor": round(med["smooth_noise"] / floor, 3)})
    say(f"floors for {ns} slots: store {store_peak:.2f} us at the 8 TB/s peak ({store_yard:.2f} us at the {YARDSTICK_TBPS} TB/s "
        f"yardstick); VALU {valu:.2f} us ({args.valu} vector instructions per quad, {args.trans} transcendental, "
        f"{cycles_per_quad / 4:.1f} cycles per sample and SIMD lane group); measured / larger floor = {med['smooth_noise'] / floor:.2f}")
    if args.loop:
        result.update(loop_figures(args.loop, B, T, args.samples, args.select))
        say(f"loop, certify 0.05 (n {args.samples}, n0 {args.select}), NO_ATTACK, {args.loop} utterances, batch {B}, LCNN: "
            f"{result['loop/utt_per_s']} utt/s; kernels {result['loop/noise_s']} s noise + {result['loop/tally_s']} s tally of "
            f"{result['loop/profiled_wall_s']} s = {100 * result['loop/kernel_share']:.2f} % of the run; abstained "
            f"{result['loop/certified/abstained']:.1f} %, certified accuracy {result['loop/certified/accuracy']:.1f} %")
    say(json.dumps(result))
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
