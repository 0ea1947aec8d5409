"""The measurement behind DESIGN.md's SmoothAdv section (needs a HIP device): the three kernels of torchattacks.SmoothAdvPGD beside
what they replace or extend, their traffic floors, the error of the soft-vote kernel against a float64 twin, and the kernels' share
of a loop run.

    smoothadv_fill(adv -> (m, B, T))     beside   smooth_noise on the same buffers (the same body behind one multiply and one add per
                                                  sample), with and without scale / shift: 4 B read + 4 m B written per sample
    smoothadv_step, L2 and L-inf         against  grads.sum(0) + pgd_l2_step / pgd_linf_step (the eager composition: the sum is
                                                  written and read again), and against the traffic floors of the issue's model:
                                                  L2 launch 1 (m + 1) * 4 B per sample, L-inf (m + 4) * 4 B, at the 8 TB/s peak

Method and output format are tools/universal_probe.py's (its `timed_pairs`): the versions are warmed up, then timed in alternating
blocks of `--iters` launches, a block being one replay of a hipGraph of those launches, so the window holds device time only;
median block, min .. max over the blocks; hot (one set of buffers).  `--split` also times `smoothadv_step` at m = 1 and reports
the difference per extra slot: the marginal rate of the slot stream, which is what the floors are about (at m = 1 the L2 step is
its two row passes and a copy).

`--error` measures the soft vote against tests/smoothadv_cpu_ops.loss_grad_np's float64 form on (m, B) = (8, 4096) logits drawn
N(0, 3^2) with saturated, mixed and near-zero rows: max |dz - ref| over the row's max |ref|, and max |cost - ref| / max(|ref|, 1):
the figures tests/test_gpu_smoothadv.py's tolerance is twice of.

`--loop N` adds one loop run over N synthetic utterances on LCNN with SMOOTHADV (`--steps`, `--samples`) and `--certify 0.05`:
utterances / s and the share of the run's wall time the three kernels' launches take (HIP events round every launch,
`hip_ops.start_profile`) — the rest is the forward and backward of the copies.

    python tools/smoothadv_probe.py [--B 128 --T 64600 --m 8 --iters 24 --blocks 15 --error --split --loop 128] [--out profiles/smoothadv_timing.txt]"""
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


def error_against_twin(dev, m=8, B=4096):
    import numpy as np
    from tests import smoothadv_cpu_ops as A
    from tests.smoothadv_cpu_ops import loss_error, probe_logits
    worst = [0.0, 0.0, 0.0, 0.0]
    for scale in (1.0, -1.0):
        z, y = probe_logits(m, B, 17)
        dz, cost = hip_ops.smoothadv_loss_grad(z.to(dev), y.to(dev), scale)
        ref = A.loss_grad_np(z, y, scale, dtype=np.float64)
        twin32 = A.loss_grad_np(z, y, scale, dtype=np.float32)
        e = loss_error(dz.cpu().numpy().astype(np.float64), cost.cpu().numpy().astype(np.float64), *ref)
        t = loss_error(twin32[0].astype(np.float64), twin32[1].astype(np.float64), *ref)
        worst = [max(a, b) for a, b in zip(worst, e + t)]
    return worst


def loop_figures(n_utt, batch, T, steps, samples):
    from audio_deepfake_adversarial_attacks_amd.aa.aa_types import AttackEnum
    from audio_deepfake_adversarial_attacks_amd.datasets.synthetic import SyntheticDetectionDataset
    from audio_deepfake_adversarial_attacks_amd.evaluation import generate_attacks
    cfg = {"data": {"seed": 42}, "checkpoint": {"path": ""},
           "model": {"name": "lcnn", "parameters": {"frontend_algorithm": ["lfcc"], "input_channels": 1}}}
    method, params = AttackEnum["SMOOTHADV"].value
    params = {**params, "steps": steps, "samples": samples}
    names = ("smoothadv_fill", "smoothadv_loss_grad", "smoothadv_step")

    def run(n, profile):
        data = SyntheticDetectionDataset(n, num_samples=T)
        if profile:
            hip_ops.start_profile(*names)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rep = generate_attacks([None, None, None], cfg, "cuda", attack_model_config=cfg, attack_method=method, attack_params=params,
                               batch_size=batch, dataset=data, share_weights=True, shuffle=False, num_workers=0,
                               certify=0.05, certify_samples=64, certify_select=16)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        ms = hip_ops.stop_profile() if profile else {}
        return rep, wall, ms

    run(batch, False)                                                  # one batch: warms kernels, plans and allocator up
    rep, wall, _ = run(n_utt, False)                                   # the rate, without event brackets
    _, wall_p, ms = run(n_utt, True)
    kernels = {k: sum(v) / 1e3 for k, v in ms.items()}
    out = {"loop/utterances": n_utt, "loop/steps": steps, "loop/samples": samples, "loop/utt_per_s": round(n_utt / wall, 2),
           "loop/wall_s": round(wall, 2), "loop/profiled_wall_s": round(wall_p, 2),
           "loop/kernel_share": round(sum(kernels.values()) / wall_p, 4), "loop/certified/violations": rep["certified/violations"],
           "loop/certified/attacked_accuracy": rep["certified/attacked_accuracy"], "loop/adv_eval/accuracy": rep["adv_eval/accuracy"]}
    out.update({f"loop/{k}_s": round(kernels.get(k, 0.0), 5) for k in names})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=128)
    ap.add_argument("--T", type=int, default=64_600)
    ap.add_argument("--m", type=int, default=8)
    ap.add_argument("--iters", type=int, default=24)
    ap.add_argument("--blocks", type=int, default=15)
    ap.add_argument("--error", action="store_true")
    ap.add_argument("--split", action="store_true")
    ap.add_argument("--loop", type=int, default=0, metavar="N")
    ap.add_argument("--loop_batch", type=int, default=16)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "smoothadv_timing.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no HIP device: this is a measurement, there is nothing to fall back to")
    dev = torch.device("cuda")
    B, T, m = args.B, args.T, args.m
    seed, sigma = 0x1234567887654321, 0.05
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    result = {"B": B, "T": T, "m": m, "iters": args.iters, "blocks": args.blocks, "window": "graph replay"}
    if args.error:
        dz_err, cost_err, dz_twin, cost_twin = error_against_twin(dev)
        result.update({"error/dz_rel": dz_err, "error/cost_rel": cost_err, "error/twin32_dz_rel": dz_twin, "error/twin32_cost_rel": cost_twin})
        say(f"soft vote, (8, 4096) logits, scale +-1: max |dz - twin64| / row max = {dz_err:.3e}, max |cost - twin64| / max(|cost|, 1) = "
            f"{cost_err:.3e} (the float32 libm twin against the same twin64: {dz_twin:.3e}, {cost_twin:.3e})")
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.rand(B, T, device=dev, generator=g)
    adv = (x + (torch.rand(B, T, device=dev, generator=g) - 0.5) * 0.01).clamp_(0, 1)
    scale = torch.rand(B, device=dev, generator=g) + 0.5
    shift = -torch.rand(B, device=dev, generator=g)
    slots = torch.empty(m, B, T, device=dev)
    grads = torch.randn(m, B, T, device=dev, generator=g)
    gsum, out = torch.empty_like(x), torch.empty_like(x)
    eps, alpha = 0.1, 0.02

    # ---- the fill beside smooth_noise -------------------------------------------------------------------------------------------------
    fills = {"smooth_noise": lambda k: hip_ops.smooth_noise(adv, sigma, seed, k * m, s0=0, ns=m, out=slots),
             "smoothadv_fill": lambda k: hip_ops.smoothadv_fill(adv, sigma, seed, k * m, s0=0, ns=m, out=slots),
             "smoothadv_fill_affine": lambda k: hip_ops.smoothadv_fill(adv, sigma, seed, k * m, s0=0, ns=m, scale=scale, shift=shift,
                                                                       out=slots)}
    times = timed_pairs(fills, args.iters, args.blocks, True)
    med = {name: statistics.median(t) for name, t in times.items()}
    per_sample = 4 + 4 * m
    for name, t in times.items():
        tbs = per_sample * B * T / (med[name] * 1e-6)
        say(f"{name}: median {med[name]:.2f} us (min {min(t):.2f}, max {max(t):.2f}), {per_sample} B/sample -> {tbs / 1e12:.2f} TB/s = "
            f"{100 * tbs / HBM_PEAK:.0f} % of HBM peak, {tbs / 1e12 / YARDSTICK_TBPS:.2f} of the yardstick")
        result[f"{name}/us"], result[f"{name}/us_min"], result[f"{name}/us_max"] = round(med[name], 3), round(min(t), 3), round(max(t), 3)
    spread = max(max(t) - min(t) for t in times.values())
    say(f"smoothadv_fill_affine - smooth_noise: {med['smoothadv_fill_affine'] - med['smooth_noise']:+.2f} us; smoothadv_fill - smooth_noise: "
        f"{med['smoothadv_fill'] - med['smooth_noise']:+.2f} us; largest min .. max spread of a version over the blocks: {spread:.2f} us")

    # ---- the step against the eager composition and its floors --------------------------------------------------------------------------
    for norm, plain, floor_words, model_words in (("L2", hip_ops.pgd_l2_step, m + 1, None), ("Linf", hip_ops.pgd_linf_step, m + 4, m + 4)):
        def fused(k, norm=norm):
            hip_ops.smoothadv_step(adv, x, grads, alpha, eps, norm=norm, out=out, gsum=gsum)

        def eager(k, plain=plain):
            torch.sum(grads, dim=0, out=gsum)
            plain(adv, gsum, x, alpha, eps, out=out)

        versions = {f"smoothadv_step_{norm}": fused, f"eager_sum_then_pgd_{norm}": eager}
        if args.split:
            one = grads[:1]
            versions[f"smoothadv_step_{norm}_m1"] = lambda k, norm=norm: hip_ops.smoothadv_step(adv, x, one, alpha, eps, norm=norm, out=out,
                                                                                              gsum=gsum)
        times = timed_pairs(versions, args.iters, args.blocks, True)
        med = {name: statistics.median(t) for name, t in times.items()}
        for name, t in times.items():
            say(f"{name}: median {med[name]:.2f} us (min {min(t):.2f}, max {max(t):.2f})")
            result[f"{name}/us"], result[f"{name}/us_min"], result[f"{name}/us_max"] = round(med[name], 3), round(min(t), 3), round(max(t), 3)
        f_us, e_us = med[f"smoothadv_step_{norm}"], med[f"eager_sum_then_pgd_{norm}"]
        floor = floor_words * 4 * B * T / HBM_PEAK * 1e6
        say(f"eager / smoothadv_step ({norm}): {e_us / f_us:.2f}x; floor {floor:.2f} us for {floor_words} * 4 B per sample at the 8 TB/s peak"
            + (" (launch 1 only: the two row passes on top are pgd_l2_step's)" if norm == "L2" else ""))
        result[f"floor_{norm}/us"] = round(floor, 2)
        if model_words is not None:
            tbs = model_words * 4 * B * T / (f_us * 1e-6)
            say(f"smoothadv_step_{norm}: {model_words * 4} B/sample -> {tbs / 1e12:.2f} TB/s = {100 * tbs / HBM_PEAK:.0f} % of HBM peak, "
                f"{tbs / 1e12 / YARDSTICK_TBPS:.2f} of the yardstick; measured / floor = {f_us / floor:.2f}")
            result[f"smoothadv_step_{norm}/tbps"] = round(tbs / 1e12, 3)
        if args.split:
            extra = (f_us - med[f"smoothadv_step_{norm}_m1"]) / (m - 1) if m > 1 else float("nan")
            tbs = 4 * B * T / (extra * 1e-6) if extra > 0 else float("nan")
            say(f"smoothadv_step_{norm}: {extra:.2f} us per extra slot = {tbs / 1e12:.2f} TB/s for its 4 B per sample "
                f"({tbs / 1e12 / YARDSTICK_TBPS:.2f} of the yardstick); at m = 1 the step is {med[f'smoothadv_step_{norm}_m1']:.2f} us")
            result[f"smoothadv_step_{norm}/us_per_extra_slot"] = round(extra, 3)

    if args.loop:
        result.update(loop_figures(args.loop, args.loop_batch, T, args.steps, args.samples))
        say(f"loop, SMOOTHADV ({args.steps} steps, {args.samples} draws) with certify 0.05 (n 64, n0 16), {args.loop} utterances, batch "
            f"{args.loop_batch}, LCNN: {result['loop/utt_per_s']} utt/s; kernels {result['loop/smoothadv_fill_s']} s fill + "
            f"{result['loop/smoothadv_loss_grad_s']} s soft vote + {result['loop/smoothadv_step_s']} s step of "
            f"{result['loop/profiled_wall_s']} s = {100 * result['loop/kernel_share']:.2f} % of the run; certified/violations "
            f"{result['loop/certified/violations']}, certified/attacked_accuracy {result['loop/certified/attacked_accuracy']:.1f} %, "
            f"adv_eval/accuracy {result['loop/adv_eval/accuracy']:.1f} %")
    say(json.dumps(result))
    path = Path(args.out)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
