"""The measurement behind DESIGN.md's FMNSparse section (needs a HIP device): the one launch of torchattacks.FMNSparse's step
beside its siblings of the same run — apgdl1_step and pgdl0_step, whose projections it shares — and beside the eager torch
formulation of the same step, which sorts.

    fmn_sparse_step, L1      the norms, the decision, the move and the box-aware L1 projection into the row's radius:
                             apgdl1_step's work minus its 12 selection passes over grad, plus one norm pass
    fmn_sparse_step, L0      ... and the exact-k projection, at a radius of about 64 and about 1024 samples per row and on the
                             all-tie input (adv = orig = 0.5, one gradient magnitude: the index cut walks 16 bits):
                             pgdl0_step's work plus one norm pass
                             (the two steps move differently, so on the random input they project different points: the
                             rows whose scores tie at the threshold, which alone run the index cut, are counted for both)
    fmn_sparse_step, move=0  the norms of d and the decision; + 8 B per copied sample
    eager                    the same step in torch ops: four row reductions, the (B,) decision, torch.where for the copy, the
                             move, and a projection by torch.sort with a radius per row (L1: the 2T breakpoints of phi; L0: the
                             k_b-th largest score)

Method and output format are tools/fmn_probe.py's (`timed_pairs` of tools/universal_probe.py): warmed up, then timed in
alternating blocks of `--iters` launches, a block being one replay of a hipGraph of those launches, so the window holds device
time only; median block, min .. max over the blocks; hot (one set of buffers: at (128, 64 600) they stay cache resident, which
is the attack's own regime between the model's passes only in part).  No row improves (the steady state) unless stated.

`--loop N` adds one loop run over N synthetic utterances on LCNN with FMN_L1 and FMN_L0: utterances / s and the share of the
run's wall time the launches take (HIP events round every launch, `hip_ops.start_profile`).

    python tools/fmn_sparse_probe.py [--B 128 --T 64600 --iters 12 --blocks 11 --loop 32] [--out profiles/fmn_sparse_timing.txt]"""
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
from universal_probe import timed_pairs  # noqa: E402  (tools/ is the script's directory)

NAMES = ("fmn_begin", "fmn_sparse_step")
INF = float("inf")


def eager_l1_project(x, u, eps):
    """The box-aware L1 projection with a radius per row, by sorting the 2T breakpoints of phi(lam) = sum min(max(|d| - lam, 0), cap)."""
    d = u - x
    ad, cap = d.abs(), torch.where(d > 0, 1.0 - x, x)
    T = x.shape[1]
    bp = torch.cat([ad, (ad - cap).clamp_min(0.0)], dim=1)                 # a sample starts to move at |d|, saturates at |d| - cap
    sign = torch.cat([torch.ones_like(ad), -torch.ones_like(ad)], dim=1)
    bp, order = torch.sort(bp, dim=1, descending=True)
    active = torch.cumsum(sign.gather(1, order), dim=1)                    # moving samples just below breakpoint j
    drop = torch.cat([bp[:, :-1] - bp[:, 1:], bp[:, -1:]], dim=1)          # down to the next breakpoint, the last one down to 0
    phi = torch.cumsum(active * drop, dim=1)                               # phi at the next breakpoint
    j = torch.searchsorted(phi, eps[:, None].contiguous()).clamp_max(2 * T - 1)
    phi_j, act_j, lo_j = phi.gather(1, j), active.gather(1, j).clamp_min(1.0), (bp - drop).gather(1, j)
    lam = torch.where(phi[:, -1:] > eps[:, None], lo_j + (phi_j - eps[:, None]) / act_j, torch.zeros_like(phi_j))
    return torch.clamp(x + torch.sign(d) * torch.minimum((ad - lam).clamp_min(0.0), cap), 0.0, 1.0)


def eager_l0_project(x, u, k):
    """The exact-k projection with a count per row, by a descending sort of the scores (ties at the threshold all kept)."""
    d = u - x
    c = torch.minimum(torch.maximum(d, -x), 1.0 - x)
    r = d - c
    s = d * d - r * r
    kk = k.clamp(1, x.shape[1]).long()
    thr = torch.sort(s, dim=1, descending=True)[0].gather(1, (kk - 1)[:, None])
    return torch.where((s >= thr) & (k >= 1)[:, None], torch.clamp(x + c, 0.0, 1.0), x)


def rows_with_threshold_ties(x, u, k):
    """How many rows have more scores at or above their k-th largest than k: those run the projection's second search (the index
    cut, ceil(bits(T - 1) / 3) more passes), and a launch lasts as long as its slowest row."""
    d = u - x
    c = torch.minimum(torch.maximum(d, -x), 1.0 - x)
    r = d - c
    s = d * d - r * r
    kk = min(int(k), x.shape[1])
    thr = torch.topk(s, kk, dim=1).values[:, -1:]
    return int(((s >= thr).sum(dim=1) > kk).sum().item())


def eager_step(adv, grad, orig, z, y, state, best_adv, alpha, gamma, norm, eps_div=1e-10):
    """One FMNSparse step in torch ops; returns (new state, out).  best_adv is updated in place."""
    d = adv - orig
    T = adv.shape[1]
    gsq = grad.square().sum(dim=1)
    e, best, found = state[0], state[1], state[2] != 0
    is_adv = (z > 0).long() != y
    if norm == "L1":
        dn, gq = d.abs().sum(dim=1), grad.abs().amax(dim=1)
        better = is_adv & (dn < best)
        best1 = torch.where(better, dn, best)
        reach = (dn + torch.where(gq > 0, z.abs() / gq, torch.full_like(gq, INF))) * (1 + gamma)
        eps1 = torch.where(is_adv, torch.minimum(e, best1) * (1 - gamma), torch.where(found, e * (1 + gamma), reach))
    else:
        dn = (d != 0).sum(dim=1).float()
        better = is_adv & (dn < best)
        best1 = torch.where(better, dn, best)
        e1 = torch.where(e == INF, torch.ones_like(e), e)
        down = torch.minimum(torch.minimum(e1 - 1, torch.floor(e1 * (1 - gamma))), best1)
        eps1 = torch.where(is_adv, down, torch.maximum(e1 + 1, torch.floor(e1 * (1 + gamma)))).clamp(0.0, float(T))
    best_adv.copy_(torch.where(better[:, None], adv, best_adv))
    u = adv + alpha * (grad / (gsq.sqrt() + eps_div)[:, None])
    out = eager_l1_project(orig, u, eps1) if norm == "L1" else eager_l0_project(orig, u, eps1)
    return torch.stack([eps1, best1, (found | is_adv).float(), dn]), out


def loop_figures(n_utt, batch, T, member):
    from audio_deepfake_adversarial_attacks_amd.aa.aa_types import AttackEnum
    from audio_deepfake_adversarial_attacks_amd.datasets.synthetic import SyntheticDetectionDataset
    from audio_deepfake_adversarial_attacks_amd.evaluation import generate_attacks
    cfg = {"data": {"seed": 42}, "checkpoint": {"path": ""},
           "model": {"name": "lcnn", "parameters": {"frontend_algorithm": ["lfcc"], "input_channels": 1}}}
    method, params = AttackEnum[member].value

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
    out = {"loop/member": member, "loop/utterances": n_utt, "loop/steps": params["steps"], "loop/utt_per_s": round(n_utt / wall, 2),
           "loop/wall_s": round(wall, 2), "loop/profiled_wall_s": round(wall_p, 2),
           "loop/kernel_share": round(sum(kernels.values()) / wall_p, 4)}
    out.update({f"loop/{k}": rep[k] for k in rep if k.startswith("min_radius/")})
    out.update({f"loop/{k}_s": round(kernels.get(k, 0.0), 5) for k in NAMES})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=128)
    ap.add_argument("--T", type=int, default=64_600)
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--blocks", type=int, default=11)
    ap.add_argument("--loop", type=int, default=0, metavar="N")
    ap.add_argument("--loop_batch", type=int, default=16)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "fmn_sparse_timing.txt"))
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
    half = torch.full((B, T), 0.5, device=dev)
    tie_grad = torch.where(torch.arange(T, device=dev) % 3 == 0, -0.05, 0.05).expand(B, T).contiguous()
    y = torch.ones(B, dtype=torch.int64, device=dev)
    z_none, z_all = torch.ones(B, device=dev), -torch.ones(B, device=dev)             # no row adversarial | every row adversarial
    alpha, gamma = 0.37, 0.05

    def found_state(eps):                                                             # found before, best = inf: not adversarial -> eps grows
        return torch.stack([torch.full((B,), float(eps), device=dev), torch.full((B,), INF, device=dev), torch.ones(B, device=dev),
                            torch.zeros(B, device=dev)])

    new, out, best = torch.empty(4, B, device=dev), torch.empty_like(x), x.clone()

    def record(times):
        med = {name: statistics.median(t) for name, t in times.items()}
        for name, t in times.items():
            say(f"{name}: median {med[name]:.2f} us (min {min(t):.2f}, max {max(t):.2f})")
            result[f"{name}/us"], result[f"{name}/us_min"], result[f"{name}/us_max"] = round(med[name], 3), round(min(t), 3), round(max(t), 3)
        return med

    # ---- L1: eps' = 19.05 * 1.05 = 20 per row, APGDL1's radius; the move's L1 length is about 75: the projection searches ----
    st = found_state(20.0 / 1.05)
    step_size, topk = torch.full((B,), 20.0, device=dev), torch.full((B,), 0.2, device=dev)
    _, got = hip_ops.fmn_sparse_step(adv, grad, x, z_none, y, st, best, alpha, gamma, "L1", state_out=new, out=out)
    _, want = eager_step(adv, grad, x, z_none, y, st, best.clone(), alpha, gamma, "L1")
    say(f"L1 eager against fused: max |diff| = {(got - want).abs().max().item():.3e}; ||out - x||_1 of row 0 = "
        f"{(got[0] - x[0]).abs().sum().item():.4f} at eps' = {new[0, 0].item():.4f}")
    med = record(timed_pairs({
        "fmn_sparse_step_L1": lambda k: hip_ops.fmn_sparse_step(adv, grad, x, z_none, y, st, best, alpha, gamma, "L1", state_out=new, out=out),
        "fmn_sparse_step_L1_all_copy": lambda k: hip_ops.fmn_sparse_step(adv, grad, x, z_all, y, st, best, alpha, gamma, "L1", state_out=new,
                                                                         out=out),
        "apgdl1_step": lambda k: hip_ops.apgdl1_step(adv, grad, x, step_size, topk, 20.0, out=out),
        "eager_step_L1": lambda k: eager_step(adv, grad, x, z_none, y, st, best, alpha, gamma, "L1")}, args.iters, args.blocks, True))
    say(f"L1: fused / apgdl1_step = {med['fmn_sparse_step_L1'] / med['apgdl1_step']:.2f}; eager / fused = "
        f"{med['eager_step_L1'] / med['fmn_sparse_step_L1']:.2f}x")

    # ---- L0 at about 64 and about 1024 samples per row, and the all-tie input ----
    for label, e0, k, a_, g_, x_ in (("k64", 61.0, 64, adv, grad, x), ("k1024", 975.0, 1024, adv, grad, x), ("tie_k1024", 975.0, 1024, half, tie_grad, half)):
        st0 = found_state(e0)
        _, got = hip_ops.fmn_sparse_step(a_, g_, x_, z_none, y, st0, best, alpha, gamma, "L0", state_out=new, out=out)
        changed = (got != x_).sum(dim=1)
        say(f"L0 {label}: eps' = {new[0, 0].item():g}, changed samples per row {changed.min().item()} .. {changed.max().item()}")
        # the two steps move differently (alpha g / ||g||_2 against 0.15 g / ||g||_1), so they project different points
        u_fused = a_ + alpha * (g_ / (g_.square().sum(dim=1).sqrt() + 1e-10)[:, None])
        u_pgdl0 = a_ + (0.15 * g_) / (g_.abs().sum(dim=1) + 1e-10)[:, None]
        ties = rows_with_threshold_ties(x_, u_fused, new[0, 0].item()), rows_with_threshold_ties(x_, u_pgdl0, k)
        result[f"L0_{label}/tie_rows_fused"], result[f"L0_{label}/tie_rows_pgdl0"] = ties
        say(f"L0 {label}: rows of {B} that tie at the threshold and run the index cut search: fused step {ties[0]}, pgdl0_step {ties[1]}")
        pairs = {f"fmn_sparse_step_L0_{label}": lambda k_, a_=a_, g_=g_, x_=x_, st0=st0: hip_ops.fmn_sparse_step(
                     a_, g_, x_, z_none, y, st0, best, alpha, gamma, "L0", state_out=new, out=out),
                 f"pgdl0_step_{label}": lambda k_, a_=a_, g_=g_, x_=x_, k=k: hip_ops.pgdl0_step(a_, g_, x_, 0.15, k, out=out)}
        if label != "tie_k1024":
            pairs[f"eager_step_L0_{label}"] = lambda k_, st0=st0: eager_step(adv, grad, x, z_none, y, st0, best, alpha, gamma, "L0")
        med = record(timed_pairs(pairs, args.iters, args.blocks, True))
        line = f"L0 {label}: fused / pgdl0_step = {med[f'fmn_sparse_step_L0_{label}'] / med[f'pgdl0_step_{label}']:.2f}"
        if label != "tie_k1024":
            line += f"; eager / fused = {med[f'eager_step_L0_{label}'] / med[f'fmn_sparse_step_L0_{label}']:.2f}x"
        say(line)

    # ---- the last call: norms of d and the decision; + the copy ----
    st = found_state(20.0)
    record(timed_pairs({
        "fmn_sparse_step_last_no_copy": lambda k: hip_ops.fmn_sparse_step(adv, None, x, z_none, y, st, best, 0.0, gamma, "L1", move=False,
                                                                          state_out=new),
        "fmn_sparse_step_last_all_copy": lambda k: hip_ops.fmn_sparse_step(adv, None, x, z_all, y, st, best, 0.0, gamma, "L1", move=False,
                                                                           state_out=new)}, args.iters, args.blocks, True))

    if args.loop:
        for member in ("FMN_L1", "FMN_L0"):
            r = loop_figures(args.loop, args.loop_batch, T, member)
            result.update({f"{member}/{k}": v for k, v in r.items()})
            say(f"loop, {member} ({r['loop/steps']} steps), {args.loop} utterances, batch {args.loop_batch}, LCNN: {r['loop/utt_per_s']} utt/s; kernels "
                f"{r['loop/fmn_sparse_step_s']} s step + {r['loop/fmn_begin_s']} s begin of {r['loop/profiled_wall_s']} s = "
                f"{100 * r['loop/kernel_share']:.2f} % of the run; min_radius/median {r.get('loop/min_radius/median')}, unflipped share "
                f"{r.get('loop/min_radius/unflipped_share')}")
    say(json.dumps(result))
    path = Path(args.out)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
