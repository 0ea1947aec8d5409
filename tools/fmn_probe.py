"""The measurement behind DESIGN.md's FMN section (needs a HIP device): the launches of torchattacks.FMN beside the eager torch
formulation of the same step, their traffic floors, and the kernels' share of a loop run.

    fmn_norms                      12 B per sample (adv, grad, orig read)
    fmn_step, L-inf                16 B per sample (+ 4 per copied sample): the decision, the copy, the move and the projection
    fmn_step, L2                   12 + 16 B per sample (+ 8 per copied sample): decision + delta launch, projection launch
    fmn_step, move = 0             8 B per copied sample
    eager                          the same recurrence in torch ops (tests/fmn_cpu_ops.py's expressions on the device): four row
                                   reductions, the (B,) decision, torch.where for the copy, the move and the projection

Each fused version is timed with no row improving (the steady state: a row copies only when it beats its best) and with every
row improving.  Method and output format are tools/universal_probe.py's (`timed_pairs`): warmed up, then timed in alternating
blocks of `--iters` launches, a block being one replay of a hipGraph of those launches, so the window holds device time only;
median block, min .. max over the blocks; hot (one set of buffers).  Floors are the documented bytes at the 8 TB/s peak.

`--loop N` adds one loop run over N synthetic utterances on LCNN with FMN (`--steps`): utterances / s and the share of the run's
wall time the launches take (HIP events round every launch, `hip_ops.start_profile`) — the rest is the model's passes.

    python tools/fmn_probe.py [--B 128 --T 64600 --iters 24 --blocks 15 --loop 64] [--out profiles/fmn_timing.txt]"""
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

NAMES = ("fmn_begin", "fmn_norms", "fmn_step")


def eager_step(adv, grad, orig, z, y, state, best_adv, alpha, gamma, norm, eps_div=1e-10):
    """One FMN step in torch ops; returns (new state, out).  best_adv is updated in place."""
    d = adv - orig
    if norm == "L2":
        dn, gq = d.square().sum(dim=1).sqrt(), grad.square().sum(dim=1).sqrt()
        gn = gq
    else:
        dn, gq = d.abs().amax(dim=1), grad.abs().sum(dim=1)
        gn = grad.square().sum(dim=1).sqrt()
    e, best, found = state[0], state[1], state[2] != 0
    is_adv = (z > 0).long() != y
    better = is_adv & (dn < best)
    best1 = torch.where(better, dn, best)
    reach = (dn + torch.where(gq > 0, z.abs() / gq, torch.full_like(gq, float("inf")))) * (1 + gamma)
    eps1 = torch.where(is_adv, torch.minimum(e, best1) * (1 - gamma), torch.where(found, e * (1 + gamma), reach))
    best_adv.copy_(torch.where(better[:, None], adv, best_adv))
    d1 = (adv + alpha * (grad / (gn + eps_div)[:, None])) - orig
    if norm == "L2":
        dn1 = d1.square().sum(dim=1).sqrt()
        f = torch.where(dn1 == 0, torch.ones_like(dn1), torch.minimum((1.0 / dn1) * eps1, torch.ones_like(dn1)))
        out = torch.clamp(orig + d1 * f[:, None], 0.0, 1.0)
    else:
        out = torch.clamp(orig + torch.maximum(torch.minimum(d1, eps1[:, None]), -eps1[:, None]), 0.0, 1.0)
    return torch.stack([eps1, best1, (found | is_adv).float(), dn]), out


def loop_figures(n_utt, batch, T, steps, member):
    from audio_deepfake_adversarial_attacks_amd.aa.aa_types import AttackEnum
    from audio_deepfake_adversarial_attacks_amd.datasets.synthetic import SyntheticDetectionDataset
    from audio_deepfake_adversarial_attacks_amd.evaluation import generate_attacks
    cfg = {"data": {"seed": 42}, "checkpoint": {"path": ""},
           "model": {"name": "lcnn", "parameters": {"frontend_algorithm": ["lfcc"], "input_channels": 1}}}
    method, params = AttackEnum[member].value
    params = {**params, "steps": steps}

    def run(n, profile):
        data = SyntheticDetectionDataset(n, num_samples=T)
        if profile:
            hip_ops.start_profile(*NAMES)
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
    out = {"loop/member": member, "loop/utterances": n_utt, "loop/steps": steps, "loop/utt_per_s": round(n_utt / wall, 2),
           "loop/wall_s": round(wall, 2), "loop/profiled_wall_s": round(wall_p, 2),
           "loop/kernel_share": round(sum(kernels.values()) / wall_p, 4)}
    out.update({f"loop/{k}": rep[k] for k in rep if k.startswith("min_radius/")})
    out.update({f"loop/{k}_s": round(kernels.get(k, 0.0), 5) for k in NAMES})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=128)
    ap.add_argument("--T", type=int, default=64_600)
    ap.add_argument("--iters", type=int, default=24)
    ap.add_argument("--blocks", type=int, default=15)
    ap.add_argument("--loop", type=int, default=0, metavar="N")
    ap.add_argument("--loop_batch", type=int, default=16)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "fmn_timing.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no HIP device: this is a measurement, there is nothing to fall back to")
    dev = torch.device("cuda")
    B, T = args.B, args.T
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    result = {"B": B, "T": T, "iters": args.iters, "blocks": args.blocks, "window": "graph replay"}
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.rand(B, T, device=dev, generator=g)
    adv = (x + (torch.rand(B, T, device=dev, generator=g) - 0.5) * 0.01).clamp_(0, 1)
    grad = torch.randn(B, T, device=dev, generator=g) * 0.05
    y = torch.ones(B, dtype=torch.int64, device=dev)
    z_none, z_all = torch.ones(B, device=dev), -torch.ones(B, device=dev)             # no row adversarial | every row adversarial
    found = torch.stack([torch.full((B,), 0.004, device=dev), torch.full((B,), float("inf"), device=dev),
                         torch.ones(B, device=dev), torch.zeros(B, device=dev)])      # best = inf: an adversarial row always improves
    new, out, best = torch.empty_like(found), torch.empty_like(x), x.clone()
    ws = hip_ops.fmn_workspace(B, T, dev)
    alpha, gamma = 0.37, 0.05
    n = B * T

    def floor_us(nbytes):
        return nbytes * n / HBM_PEAK * 1e6

    versions = {"fmn_norms": lambda k: hip_ops.fmn_norms(adv, grad, x, ws=ws),
                "eager_norms": lambda k: ((adv - x).square().sum(dim=1), (adv - x).abs().amax(dim=1), grad.square().sum(dim=1),
                                          grad.abs().sum(dim=1))}
    times = timed_pairs(versions, args.iters, args.blocks, True)
    med = {name: statistics.median(t) for name, t in times.items()}
    for name, t in times.items():
        say(f"{name}: median {med[name]:.2f} us (min {min(t):.2f}, max {max(t):.2f})")
        result[f"{name}/us"], result[f"{name}/us_min"], result[f"{name}/us_max"] = round(med[name], 3), round(min(t), 3), round(max(t), 3)
    say(f"fmn_norms: 12 B/sample -> {12 * n / (med['fmn_norms'] * 1e-6) / 1e12:.2f} TB/s, floor {floor_us(12):.2f} us at the 8 TB/s peak, "
        f"measured / floor = {med['fmn_norms'] / floor_us(12):.2f}; eager / fused = {med['eager_norms'] / med['fmn_norms']:.2f}x")

    hip_ops.fmn_norms(adv, grad, x, ws=ws)                                            # the partials every step below re-reduces
    for norm, base, copied in (("Linf", 16, 4), ("L2", 28, 8)):
        def fused(z, norm=norm):
            return lambda k: hip_ops.fmn_step(adv, grad, x, z, y, found, best, ws, alpha, gamma, norm, state_out=new, out=out)

        def eager(z, norm=norm):
            return lambda k: eager_step(adv, grad, x, z, y, found, best, alpha, gamma, norm)

        versions = {f"fmn_step_{norm}_no_copy": fused(z_none), f"fmn_step_{norm}_all_copy": fused(z_all),
                    f"eager_step_{norm}_no_copy": eager(z_none)}
        times = timed_pairs(versions, args.iters, args.blocks, True)
        med = {name: statistics.median(t) for name, t in times.items()}
        for name, t in times.items():
            say(f"{name}: median {med[name]:.2f} us (min {min(t):.2f}, max {max(t):.2f})")
            result[f"{name}/us"], result[f"{name}/us_min"], result[f"{name}/us_max"] = round(med[name], 3), round(min(t), 3), round(max(t), 3)
        f0, f1, e0 = med[f"fmn_step_{norm}_no_copy"], med[f"fmn_step_{norm}_all_copy"], med[f"eager_step_{norm}_no_copy"]
        say(f"fmn_step {norm}: {base} B/sample -> {base * n / (f0 * 1e-6) / 1e12:.2f} TB/s, floor {floor_us(base):.2f} us, measured / floor = "
            f"{f0 / floor_us(base):.2f}; every row copied: {base + copied} B/sample, floor {floor_us(base + copied):.2f} us, measured / floor = "
            f"{f1 / floor_us(base + copied):.2f}; eager step (its own norms included) / (fmn_norms + fmn_step) = "
            f"{e0 / (result['fmn_norms/us'] + f0):.2f}x")
        result[f"floor_step_{norm}/us"] = round(floor_us(base), 2)

    versions = {"fmn_step_last_no_copy": lambda k: hip_ops.fmn_step(adv, None, x, z_none, y, found, best, ws, 0.0, gamma, "Linf", move=False,
                                                                   state_out=new),
                "fmn_step_last_all_copy": lambda k: hip_ops.fmn_step(adv, None, x, z_all, y, found, best, ws, 0.0, gamma, "Linf", move=False,
                                                                    state_out=new)}
    times = timed_pairs(versions, args.iters, args.blocks, True)
    for name, t in times.items():
        m = statistics.median(t)
        say(f"{name}: median {m:.2f} us (min {min(t):.2f}, max {max(t):.2f})")
        result[f"{name}/us"] = round(m, 3)
    say(f"fmn_step move = 0, every row copied: 8 B/sample, floor {floor_us(8):.2f} us, measured / floor = "
        f"{result['fmn_step_last_all_copy/us'] / floor_us(8):.2f}")

    if args.loop:
        for member in ("FMN", "FMN_L2"):
            r = loop_figures(args.loop, args.loop_batch, T, args.steps, member)
            result.update({f"{member}/{k}": v for k, v in r.items()})
            say(f"loop, {member} ({args.steps} steps), {args.loop} utterances, batch {args.loop_batch}, LCNN: {r['loop/utt_per_s']} utt/s; kernels "
                f"{r['loop/fmn_norms_s']} s norms + {r['loop/fmn_step_s']} s step + {r['loop/fmn_begin_s']} s begin of {r['loop/profiled_wall_s']} s = "
                f"{100 * r['loop/kernel_share']:.2f} % of the run; min_radius/median {r.get('loop/min_radius/median')}, unflipped share "
                f"{r.get('loop/min_radius/unflipped_share')}")
    say(json.dumps(result))
    path = Path(args.out)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
