"""The measurement behind DESIGN.md's HopSkipJump section (needs a HIP device): the kernels of the label-only black-box attack at
the flagship batch shape, with HIP events, and the candidates kernel beside an eager formulation of the same step.

    hsj_search_next(cur, orig -> probe)      model: 12 B per sample (open and close are the same kernel's other modes, with the
                                             same traffic for a row that moves; they are not timed separately)
    hsj_probe(cur -> (8, B, T))              one fill of max_rows / B = 8 slots; model: 4 B read + 4 * 8 B written per sample
    hsj_candidates(cur, z (n, B) -> (K, B, T))   at n = 32 and n = 256, K = 4; model: 4 B read + 4 K B written per sample — the
                                             kernel is priced against this traffic although it is bound by the vector ALUs
        against   v STORED as (B, n, T) float32;  est = bmm(phi - mean phi, v);  clamp(cur + xi_k * sign(est), 0, 1)
                                             (its own traffic is 4 n B per sample more than the model it is priced at)
    hsj_take(cur, cand -> cur)               every row moves; model: 8 B per sample

Method and output format are tools/universal_probe.py's (its `timed_pairs`): the versions of a pair are warmed up (50 launches),
then timed in alternating blocks of `--iters` launches, a block being one replay of a hipGraph of those launches, so the window holds
device time only; median block, min .. max over the blocks.  The launches rotate over one set of buffers (hot).  Bytes per second
count the traffic models above against the 8 TB/s HBM peak.

`--loop N` adds one HopSkipJump evaluation run over N synthetic utterances on LCNN (what `--attack HSJ --synthetic N
--share_weights` runs): utterances / s, mean queries, and the share of the run's wall time that the kernels' launches take (HIP
events round every launch, `hip_ops.start_profile`) — the rest is the forward of the probes.

    python tools/hsj_probe.py [--B 128 --T 64600 --iters 96 --blocks 15 --loop 1024] [--out profiles/hsj_probe.txt]"""
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

KERNELS = ("hsj_search_open", "hsj_search_next", "hsj_search_close", "hsj_probe", "hsj_candidates", "hsj_take")


def loop_figures(n_utt, batch, T):
    from audio_deepfake_adversarial_attacks_amd.aa.aa_types import AttackEnum
    from audio_deepfake_adversarial_attacks_amd.datasets.synthetic import SyntheticDetectionDataset
    from audio_deepfake_adversarial_attacks_amd.evaluation import generate_attacks
    cfg = {"data": {"seed": 42}, "checkpoint": {"path": ""},
           "model": {"name": "lcnn", "parameters": {"frontend_algorithm": ["lfcc"], "input_channels": 1}}}
    method, params = AttackEnum["HSJ"].value

    def run(n, profile):
        data = SyntheticDetectionDataset(n, num_samples=T)
        if profile:
            hip_ops.start_profile(*KERNELS, "perturbation_stats")
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
    out = {"loop/utterances": n_utt, "loop/HSJ/utt_per_s": round(n_utt / wall, 2), "loop/HSJ/queries_mean": rep["blackbox/queries_mean"],
           "loop/HSJ/stopped_early": rep["blackbox/stopped_early"], "loop/HSJ/accuracy": float(rep["adv_eval/accuracy"]),
           "loop/HSJ/wall_s": round(wall, 2), "loop/HSJ/profiled_wall_s": round(wall_p, 2),
           "loop/HSJ/kernel_share": round(sum(kernels.values()) / wall_p, 4)}
    out.update({f"loop/HSJ/{k}_s": round(v, 4) for k, v in kernels.items()})
    out.update({k: v for k, v in rep.items() if k.startswith("min_radius/")})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=128)
    ap.add_argument("--T", type=int, default=64_600)
    ap.add_argument("--K", type=int, default=4)
    ap.add_argument("--iters", type=int, default=96)
    ap.add_argument("--blocks", type=int, default=15)
    ap.add_argument("--loop", type=int, default=0, metavar="N")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "hsj_probe.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no HIP device: this is a measurement, there is nothing to fall back to")
    dev = torch.device("cuda")
    B, T, K = args.B, args.T, args.K
    seed = 0x1234567887654321
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    result = {"B": B, "T": T, "K": K, "iters": args.iters, "blocks": args.blocks, "window": "graph replay", "sets": 1}
    g = torch.Generator(device=dev).manual_seed(1)
    orig = torch.rand(B, T, device=dev, generator=g)
    cur = torch.rand(B, T, device=dev, generator=g)
    out = torch.empty(B, T, device=dev)
    y = torch.randint(0, 2, (B,), device=dev, generator=g)
    active = torch.ones(B, dtype=torch.int32, device=dev)              # every row does the work
    queries = torch.zeros(B, dtype=torch.int32, device=dev)
    dist = hip_ops.perturbation_stats(orig, cur)[0].contiguous()
    mag = (dist * 2.0 ** -6).contiguous()
    z1 = torch.randn(B, device=dev, generator=g)
    state = hip_ops.hsj_search_open(cur, orig, dist, active, out)
    state2 = torch.empty_like(state)
    slots = torch.empty(8, B, T, device=dev)
    cand = torch.rand(K, B, T, device=dev, generator=g)
    zc = ((1.0 - 2.0 * y.float())[None] * torch.ones(K, 1, device=dev)).contiguous()   # slot 0 is adversarial: every row is copied
    scales = (0.5 ** torch.arange(K, device=dev, dtype=torch.float32))

    def report(pair, per_sample):
        times = timed_pairs(pair, args.iters, args.blocks, True)
        med = {name: statistics.median(t) for name, t in times.items()}
        for name, t in times.items():
            tbs = per_sample * B * T / (med[name] * 1e-6)
            say(f"{name}: median {med[name]:.2f} us (min {min(t):.2f}, max {max(t):.2f}), {per_sample} B/sample "
                f"-> {tbs / 1e12:.2f} TB/s = {100 * tbs / HBM_PEAK:.0f} % of HBM peak")
            result[f"{name}/us"] = round(med[name], 3)
            result[f"{name}/us_min"] = round(min(t), 3)
            result[f"{name}/us_max"] = round(max(t), 3)
            result[f"{name}/TBps"] = round(tbs / 1e12, 3)
        return med

    report({"hsj_search_next": lambda k: hip_ops.hsj_search_next(cur, orig, z1, y, active, state, out, state_out=state2)}, 12)
    report({"hsj_probe_8_slots": lambda k: hip_ops.hsj_probe(cur, mag, active, seed, k, s0=0, ns=8, out=slots)}, 4 + 4 * 8)
    report({"hsj_take": lambda k: hip_ops.hsj_take(cur, cand, zc, y, active, queries, 32, out=out)}, 8)
    for n in (32, 256):
        z = torch.randn(n, B, device=dev, generator=g)
        v = torch.empty(B, n, T, device=dev).bernoulli_(0.5, generator=g).mul_(2.0).sub_(1.0)    # the eager version's stored directions
        cout = torch.empty(K, B, T, device=dev)

        def fused(k, z=z, cout=cout):
            hip_ops.hsj_candidates(cur, z, y, dist, active, 0.5, K, seed, k, out=cout)

        def eager(k, z=z, v=v):
            phi = ((z > 0) != (y == 1)[None]).float().t()                                           # (B, n)
            est = torch.bmm((phi - phi.mean(dim=1, keepdim=True))[:, None, :], v)[:, 0]             # (B, T)
            xi = (dist * 0.5)[None, :, None] * scales[:, None, None]
            torch.clamp(cur[None] + xi * torch.sign(est)[None], 0, 1)

        med = report({f"hsj_candidates_n{n}": fused, f"eager_candidates_n{n}": eager}, 4 + 4 * K)
        ratio = med[f"eager_candidates_n{n}"] / med[f"hsj_candidates_n{n}"]
        say(f"n={n}: eager_candidates / hsj_candidates: {ratio:.2f}x" + ("" if ratio > 1 else "  (the kernel is NOT faster)"))
        result[f"candidates_n{n}/eager_over_fused"] = round(ratio, 3)
        del v, z, cout
    if args.loop:
        result.update(loop_figures(args.loop, B, T))
        shares = ", ".join(f"{k} {result.get(f'loop/HSJ/{k}_s', 0.0)} s" for k in KERNELS + ("perturbation_stats",))
        say(f"loop, HSJ (10 steps, budget 889), {args.loop} utterances, batch {B}, LCNN: {result['loop/HSJ/utt_per_s']} utt/s, "
            f"mean queries {result['loop/HSJ/queries_mean']:.1f}, stopped early {result['loop/HSJ/stopped_early']:.3f}; kernels: "
            f"{shares} of {result['loop/HSJ/profiled_wall_s']} s = {100 * result['loop/HSJ/kernel_share']:.2f} % of the run")
        started = 1.0 - result["min_radius/already_wrong_share"] - result["min_radius/unflipped_share"]
        say(f"loop: {100 * result['min_radius/already_wrong_share']:.1f} % of the utterances were wrong from the start, "
            f"{100 * started:.1f} % found a start"
            + ("" if started > 0 else ": the random-init detector answers one class for every utterance and for noise, so NO row was "
               "ever active in this run.  The batch shape never changes, so the run still forwarded every probe and the search, probe "
               "and take kernels moved every byte they would have; hsj_candidates took its copy path.  The rate stands for the "
               "loop's cost per utterance, not for what the attack achieves, which has not been measured."))
    say(json.dumps(result))
    path = Path(args.out)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
