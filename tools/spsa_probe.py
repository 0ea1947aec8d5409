"""The measurement behind DESIGN.md's SPSA section (needs a HIP device): the two kernels of the score-based black-box attack
beside an eager formulation of the same two steps, at the flagship batch shape, with HIP events.

    spsa_probe(adv -> (S, B, T))   against   v materialised as (B, n, T);  clamp(adv[:, None] +- delta * v, 0, 1)
                                             model: 4 B read + 4 S B written per sample
    spsa_step(adv, orig, z)        against   g = (d[:, :, None] * v).sum(1);  pgd_linf_step(adv, g, orig)
                                             model: 12 B per sample (+ the (S, B) logits)

Method and output format are tools/universal_probe.py's (its `timed_pairs`): the versions of a pair are warmed up, then timed in
alternating blocks of `--iters` launches, a block being one replay of a hipGraph of those launches, so the window holds device
time only; median block, min .. max over the blocks; once with the launches rotating over one set of buffers (hot: the step's
100 MB fit the 256 MB Infinity Cache, the probe's S output slots do not) and once over eight (from HBM).  Bytes per second count
the traffic models above against the 8 TB/s HBM peak; the streaming yardstick is universal_apply's recorded 4.28 TB/s
(profiles/universal_probe.txt).  The eager versions read a stored v, which the kernels never have: their own traffic is larger
than the model they are priced at.

`--loop N` adds one SPSA evaluation run over N synthetic utterances on LCNN (what `--attack SPSA --synthetic N --share_weights`
runs): utterances / s, mean queries, and the share of the run's wall time that the two kernels' launches take (HIP events round
every launch, `hip_ops.start_profile`) — the rest is the forward of S * B rows per iteration.

    python tools/spsa_probe.py [--B 128 --T 64600 --n 8 --iters 48 --blocks 15 --loop 1024] [--out profiles/spsa_probe.txt]"""
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


def loop_figures(n_utt, batch, T):
    from audio_deepfake_adversarial_attacks_amd.aa.aa_types import AttackEnum
    from audio_deepfake_adversarial_attacks_amd.datasets.synthetic import SyntheticDetectionDataset
    from audio_deepfake_adversarial_attacks_amd.evaluation import generate_attacks
    cfg = {"data": {"seed": 42}, "checkpoint": {"path": ""},
           "model": {"name": "lcnn", "parameters": {"frontend_algorithm": ["lfcc"], "input_channels": 1}}}
    method, params = AttackEnum["SPSA"].value

    def run(n, profile):
        data = SyntheticDetectionDataset(n, num_samples=T)
        if profile:
            hip_ops.start_profile("spsa_probe", "spsa_step")
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
    return {"loop/utterances": n_utt, "loop/SPSA/utt_per_s": round(n_utt / wall, 1), "loop/SPSA/queries_mean": rep["blackbox/queries_mean"],
            "loop/SPSA/stopped_early": rep["blackbox/stopped_early"], "loop/SPSA/accuracy": float(rep["adv_eval/accuracy"]),
            "loop/SPSA/wall_s": round(wall, 2), "loop/SPSA/profiled_wall_s": round(wall_p, 2),
            "loop/SPSA/probe_s": round(kernels.get("spsa_probe", 0.0), 4), "loop/SPSA/step_s": round(kernels.get("spsa_step", 0.0), 4),
            "loop/SPSA/kernel_share": round(sum(kernels.values()) / wall_p, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=128)
    ap.add_argument("--T", type=int, default=64_600)
    ap.add_argument("--n", type=int, default=8)
    ap.add_argument("--iters", type=int, default=48)
    ap.add_argument("--blocks", type=int, default=15)
    ap.add_argument("--loop", type=int, default=0, metavar="N")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "spsa_probe.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no HIP device: this is a measurement, there is nothing to fall back to")
    dev = torch.device("cuda")
    B, T, n = args.B, args.T, args.n
    S = 1 + 2 * n
    seed, delta, alpha, eps = 0x1234567887654321, 0.0005, 0.000125, 0.0005
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    result = {"B": B, "T": T, "n": n, "S": S, "iters": args.iters, "blocks": args.blocks, "window": "graph replay"}
    g = torch.Generator(device=dev).manual_seed(1)
    v = (torch.randint(0, 2, (B, n, T), device=dev, generator=g) * 2 - 1).float()      # the eager versions' stored directions
    z = torch.randn(S, B, device=dev, generator=g)
    y = torch.randint(0, 2, (B,), device=dev, generator=g)
    z[0] = 2.0 * y.float() - 1.0                                                       # no row fooled: every row does the work
    d = ((1.0 - 2.0 * y.float())[None] * (z[1::2] - z[2::2])).t().contiguous()         # (B, n)
    queries = torch.zeros(B, dtype=torch.int32, device=dev)
    slots = torch.empty(S, B, T, device=dev)                                           # written only: one set serves both runs
    for sets in (1, 8):
        bufs = [(torch.rand(B, T, device=dev, generator=g), torch.rand(B, T, device=dev, generator=g), torch.empty(B, T, device=dev))
                for _ in range(sets)]

        def probe(k):
            hip_ops.spsa_probe(bufs[k % sets][0], delta, seed, k, s0=0, ns=S, out=slots)

        def probe_eager(k):
            a = bufs[k % sets][0][:, None, :]
            torch.clamp(a + delta * v, 0, 1), torch.clamp(a - delta * v, 0, 1)

        def step(k):
            hip_ops.spsa_step(bufs[k % sets][0], bufs[k % sets][1], z, y, queries, alpha, eps, seed, k, out=bufs[k % sets][2])

        def step_eager(k):
            est = (d[:, :, None] * v).sum(1)
            hip_ops.pgd_linf_step(bufs[k % sets][0], est, bufs[k % sets][1], alpha, eps, out=bufs[k % sets][2])

        for pair, per_sample in (({"spsa_probe": probe, "eager_probe": probe_eager}, 4 + 4 * S),
                                 ({"spsa_step": step, "eager_step": step_eager}, 12)):
            times = timed_pairs(pair, args.iters, args.blocks, True)
            med = {name: statistics.median(t) for name, t in times.items()}
            for name, t in times.items():
                tbs = per_sample * B * T / (med[name] * 1e-6)
                say(f"sets={sets} {name}: median {med[name]:.2f} us (min {min(t):.2f}, max {max(t):.2f}), {per_sample} B/sample "
                    f"-> {tbs / 1e12:.2f} TB/s = {100 * tbs / HBM_PEAK:.0f} % of HBM peak, {tbs / 1e12 / YARDSTICK_TBPS:.2f} of the yardstick")
                result[f"{name}/sets{sets}/us"] = round(med[name], 3)
                result[f"{name}/sets{sets}/us_min"] = round(min(t), 3)
                result[f"{name}/sets{sets}/us_max"] = round(max(t), 3)
                result[f"{name}/sets{sets}/TBps"] = round(tbs / 1e12, 3)
            fused, eager = list(pair)
            say(f"sets={sets} {eager} / {fused}: {med[eager] / med[fused]:.2f}x")
        del bufs
    if args.loop:
        result.update(loop_figures(args.loop, B, T))
        say(f"loop, SPSA (20 steps x 17 slots), {args.loop} utterances, batch {B}, LCNN: {result['loop/SPSA/utt_per_s']} utt/s, "
            f"mean queries {result['loop/SPSA/queries_mean']:.1f}, stopped early {result['loop/SPSA/stopped_early']:.3f}; kernels "
            f"{result['loop/SPSA/probe_s']} s probe + {result['loop/SPSA/step_s']} s step of {result['loop/SPSA/profiled_wall_s']} s "
            f"= {100 * result['loop/SPSA/kernel_share']:.2f} % of the run")
    say(json.dumps(result))
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
