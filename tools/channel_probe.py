"""The measurement behind DESIGN.md's channel section (needs a HIP device): the forward and the fused adjoint step of the simulated
audio channel beside eager formulations of the same steps, at the flagship batch shape, with HIP events.

    channel_apply(x -> (K, B, T))      against   gather by the delay + mask;  grouped conv1d (K B groups);  c + g * y + a * (2 rand - 1)
                                                 models: 4 + 4 K B per sample;  2 K L unfused float32 operations per sample
    channel_eot_step(adv, orig, gy)    against   gather + mask;  grouped conv1d with the taps unflipped (the transposed
                                                 convolution);  sum over the draws;  hip_ops.pgd_linf_step
                                                 models: 4 K + 12 B per sample;  2 K L operations per sample

Method and output format are tools/universal_probe.py's (its `timed_pairs`): the versions of a pair are warmed up, then timed in
alternating blocks of `--iters` launches, a block being one replay of a hipGraph of those launches, so the window holds device
time only; median block, min .. max over the blocks; once with the launches rotating over one set of input buffers (hot) and
once over eight (from HBM).  Unlike the streaming attack kernels these two are not bound by HBM at every L: each line prices the
time against BOTH derived floors — the byte model at the 8 TB/s HBM peak, and 2 K L B T unfused operations at the vector ALUs'
rate for separate v_mul_f32 / v_add_f32 (a quarter of the 157.3 TFLOP/s peak, which counts a packed fused multiply-add as four;
-ffp-contract=off and the ABI's one-rounding-per-operation rule out the fusing) — and says which of the two is the larger.

`--loop N` adds one EOTPGD evaluation run over N synthetic utterances on LCNN (what `--attack EOTPGD --synthetic N --share_weights`
runs): utterances / s and the share of the run's wall time that the two kernels' launches take (HIP events round every launch,
`hip_ops.start_profile`) — the rest is eot_iter forward + backward passes per step.

    python tools/channel_probe.py [--B 128 --T 64600 --K 8 --L 64 256 --iters 12 --blocks 9 --loop 4096] [--out profiles/channel_probe.txt]"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from audio_deepfake_adversarial_attacks_amd import hip_ops  # noqa: E402
from universal_probe import HBM_PEAK, timed_pairs  # noqa: E402  (tools/ is the script's directory)

UNFUSED_OPS_PEAK = 157.3e12 / 4      # v_mul_f32 / v_add_f32 per second: 16 lanes x 4 SIMDs x 256 CUs x 2.4 GHz


def delayed(src, first, n):
    """(..., n): src[..., first + p] for p = 0 .. n - 1 inside the row, 0 outside; first (...,) int64 per row."""
    idx = first[..., None] + torch.arange(n, device=src.device)
    ok = (idx >= 0) & (idx < src.shape[-1])
    return torch.gather(src, -1, idx.clamp(0, src.shape[-1] - 1)) * ok


def eager_apply(x, center, taps, shift, gain, noise):
    K, B, L = taps.shape
    T = x.shape[1]
    xc = (x - center[:, None]).expand(K, B, T)
    win = delayed(xc, -shift.long() - (L - 1), T + L - 1)                              # (K, B, T + L - 1)
    y = F.conv1d(win.reshape(1, K * B, -1), taps.flip(-1).reshape(K * B, 1, L), groups=K * B).reshape(K, B, T)
    return (center[None, :, None] + gain[..., None] * y) + noise[..., None] * (2.0 * torch.rand_like(y) - 1.0)


def eager_step(adv, orig, grads, taps, shift, gain, alpha, eps, out):
    K, B, L = taps.shape
    T = adv.shape[1]
    win = delayed(grads, shift.long(), T + L - 1)
    acc = F.conv1d(win.reshape(1, K * B, -1), taps.reshape(K * B, 1, L), groups=K * B).reshape(K, B, T)
    return hip_ops.pgd_linf_step(adv, (gain[..., None] * acc).sum(0), orig, alpha, eps, out=out)


def loop_figures(n_utt, batch, T):
    from audio_deepfake_adversarial_attacks_amd.aa.aa_types import AttackEnum
    from audio_deepfake_adversarial_attacks_amd.datasets.synthetic import SyntheticDetectionDataset
    from audio_deepfake_adversarial_attacks_amd.evaluation import generate_attacks
    cfg = {"data": {"seed": 42}, "checkpoint": {"path": ""},
           "model": {"name": "lcnn", "parameters": {"frontend_algorithm": ["lfcc"], "input_channels": 1}}}
    method, params = AttackEnum["EOTPGD"].value

    def run(n, profile):
        data = SyntheticDetectionDataset(n, num_samples=T)
        if profile:
            hip_ops.start_profile("channel_apply", "channel_eot_step")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rep = generate_attacks([None, None, None], cfg, "cuda", attack_model_config=cfg, attack_method=method, attack_params=params,
                               batch_size=batch, dataset=data, share_weights=True, shuffle=False, num_workers=0)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        ms = hip_ops.stop_profile() if profile else {}
        return rep, wall, ms

    run(batch, False)                                                  # one batch: warms kernels, plans and allocator up
    rep, wall, _ = run(n_utt, False)                                   # the rate, without event brackets
    _, wall_p, ms = run(n_utt, True)
    kernels = {k: sum(v) / 1e3 for k, v in ms.items()}
    return {"loop/utterances": n_utt, "loop/EOTPGD/utt_per_s": round(n_utt / wall, 1), "loop/EOTPGD/accuracy": float(rep["adv_eval/accuracy"]),
            "loop/EOTPGD/wall_s": round(wall, 2), "loop/EOTPGD/profiled_wall_s": round(wall_p, 2),
            "loop/EOTPGD/apply_s": round(kernels.get("channel_apply", 0.0), 4),
            "loop/EOTPGD/eot_step_s": round(kernels.get("channel_eot_step", 0.0), 4),
            "loop/EOTPGD/kernel_share": round(sum(kernels.values()) / wall_p, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=128)
    ap.add_argument("--T", type=int, default=64_600)
    ap.add_argument("--K", type=int, default=8)
    ap.add_argument("--L", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--loop", type=int, default=0, metavar="N")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "channel_probe.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no HIP device: this is a measurement, there is nothing to fall back to")
    dev = torch.device("cuda")
    B, T, K = args.B, args.T, args.K
    seed, alpha, eps = 0x1234567887654321, 0.000125, 0.0005
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    result = {"B": B, "T": T, "K": K, "L": args.L, "iters": args.iters, "blocks": args.blocks, "window": "graph replay"}
    g = torch.Generator(device=dev).manual_seed(1)
    center = torch.full((B,), 0.5, device=dev)
    through = torch.empty(K, B, T, device=dev)                                         # written only: one set serves both runs
    for L in args.L:
        taps = torch.randn(K, B, L, device=dev, generator=g) * 0.1
        taps[..., 0] = 1.0
        shift = torch.randint(-160, 161, (K, B), device=dev, generator=g).to(torch.int32)
        gain = torch.rand(K, B, device=dev, generator=g) + 0.5
        noise = torch.full((K, B), 0.01, device=dev)
        ops = 2.0 * K * L * B * T
        for sets in (1, 8):
            xs = [torch.rand(B, T, device=dev, generator=g) for _ in range(sets)]
            origs = [torch.rand(B, T, device=dev, generator=g) for _ in range(sets)]
            grads = [torch.randn(K, B, T, device=dev, generator=g) for _ in range(sets)]
            outs = [torch.empty(B, T, device=dev) for _ in range(sets)]

            def apply(k):
                hip_ops.channel_apply(xs[k % sets], center, taps, shift, gain, noise, seed, k, out=through)

            def apply_eager(k):
                eager_apply(xs[k % sets], center, taps, shift, gain, noise)

            def step(k):
                hip_ops.channel_eot_step(xs[k % sets], origs[k % sets], grads[k % sets], taps, shift, gain, alpha, eps, out=outs[k % sets])

            def step_eager(k):
                eager_step(xs[k % sets], origs[k % sets], grads[k % sets], taps, shift, gain, alpha, eps, outs[k % sets])

            for pair, per_sample in (({"channel_apply": apply, "eager_apply": apply_eager}, 4 + 4 * K),
                                     ({"channel_eot_step": step, "eager_eot_step": step_eager}, 4 * K + 12)):
                times = timed_pairs(pair, args.iters, args.blocks, True)
                med = {name: statistics.median(t) for name, t in times.items()}
                floor_bytes, floor_ops = per_sample * B * T / HBM_PEAK * 1e6, ops / UNFUSED_OPS_PEAK * 1e6
                bound = "ALU" if floor_ops > floor_bytes else "HBM"
                for name, t in times.items():
                    tbs, tops = per_sample * B * T / (med[name] * 1e-6), ops / (med[name] * 1e-6)
                    say(f"L={L} sets={sets} {name}: median {med[name]:.1f} us (min {min(t):.1f}, max {max(t):.1f}); {per_sample} B/sample "
                        f"-> {tbs / 1e12:.2f} TB/s (floor {floor_bytes:.1f} us); {2 * K * L} op/sample -> {tops / 1e12:.2f} Top/s "
                        f"(floor {floor_ops:.1f} us); {bound}-bound floor / time = {max(floor_bytes, floor_ops) / med[name]:.2f}")
                    result[f"{name}/L{L}/sets{sets}/us"] = round(med[name], 2)
                    result[f"{name}/L{L}/sets{sets}/us_min"] = round(min(t), 2)
                    result[f"{name}/L{L}/sets{sets}/us_max"] = round(max(t), 2)
                fused, eager = list(pair)
                say(f"L={L} sets={sets} {eager} / {fused}: {med[eager] / med[fused]:.2f}x")
            del xs, origs, grads, outs
    if args.loop:
        result.update(loop_figures(args.loop, B, T))
        say(f"loop, EOTPGD (10 steps x 4 draws, channel mild), {args.loop} utterances, batch {B}, LCNN: {result['loop/EOTPGD/utt_per_s']} "
            f"utt/s; kernels {result['loop/EOTPGD/apply_s']} s apply + {result['loop/EOTPGD/eot_step_s']} s step of "
            f"{result['loop/EOTPGD/profiled_wall_s']} s = {100 * result['loop/EOTPGD/kernel_share']:.2f} % of the run")
    say(json.dumps(result))
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
