"""The measurement behind DESIGN.md section 4x's timing (needs a HIP device): the two kernels of the universal perturbation
beside the eager formulation each replaces, at the flagship batch shape, with HIP events.

    universal_colsum(g, w)          against   (g * w[:, None]).sum(0)                       4 B per sample (+ the group planes)
    universal_apply(x, delta, w)    against   torch.clamp(x + w[:, None] * delta, 0, 1)     8 B per sample

The two versions of a pair are warmed up, then timed in alternating blocks of `--iters` launches (one event pair per block, so
the events' own cost is spread over the block); the figure is the median block and the spread is min .. max over the blocks of
that same run.  A block is one replay of a hipGraph that holds the `--iters` launches, so the window holds device time only:
launched one by one from Python, each of these calls costs 11 to 16 us of host time whatever its kernels do (`--eager_launch`
times that instead).  Every pair is timed twice, its launches rotating over one set of buffers (33 / 66 MB: inside the 256 MB
Infinity Cache) and over eight (outside it).  The condition printed at the end: each fused op's median is no slower than its eager pair's, beyond the
spread between the blocks.  Bytes per second count the algorithm's compulsory bytes against the 8 TB/s HBM peak.  Prints one line
per configuration and one JSON line; `--loop N` adds the evaluation loop's utterances / s with a loaded perturbation next to a
NO_ATTACK run over N synthetic utterances.

    python tools/universal_probe.py [--B 128 --T 64600 --iters 96 --blocks 15 --loop 1024] [--eager_launch]"""
import argparse
import json
import statistics
import sys
import tempfile
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from audio_deepfake_adversarial_attacks_amd import hip_ops  # noqa: E402

HBM_PEAK = 8.0e12      # bytes / s, HBM3E spec


def replayed(fn, iters, side):
    """A graph of `iters` launches of fn, captured on `side` after a warm-up there (scratch buffers are keyed by stream)."""
    with torch.cuda.stream(side):
        for k in range(16):
            fn(k)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        for k in range(iters):
            fn(k)
    return graph


def timed_pairs(pairs, iters, blocks, graph):
    """{name: [us per launch, one per block]} for the functions of `pairs`, alternating block by block.  graph: a block is one
    replay of `iters` captured launches (device time: the host is out of the window); else `iters` launches from Python."""
    for fn in pairs.values():
        for k in range(50):
            fn(k)
    torch.cuda.synchronize()
    if graph:
        side = torch.cuda.Stream()
        graphs = {name: replayed(fn, iters, side) for name, fn in pairs.items()}
        for g in graphs.values():
            g.replay()
        torch.cuda.synchronize()
    times = {name: [] for name in pairs}
    for _ in range(blocks):
        for name, fn in pairs.items():                               # alternating: all see the same machine
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            if graph:
                graphs[name].replay()
            else:
                for k in range(iters):
                    fn(k)
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) * 1e3 / iters)
    return times


def loop_rate(n, batch, T, attack, load=None):
    from audio_deepfake_adversarial_attacks_amd.aa.aa_types import AttackEnum
    from audio_deepfake_adversarial_attacks_amd.datasets.synthetic import SyntheticDetectionDataset
    from audio_deepfake_adversarial_attacks_amd.evaluation import generate_attacks
    cfg = {"data": {"seed": 42}, "checkpoint": {"path": ""},
           "model": {"name": "lcnn", "parameters": {"frontend_algorithm": ["lfcc"], "input_channels": 1}}}
    method, params = AttackEnum[attack].value
    data = SyntheticDetectionDataset(n, num_samples=T)
    rates = []
    for _ in range(3):                                               # the first run warms kernels, plans and allocator up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        generate_attacks([None, None, None], cfg, "cuda", attack_model_config=cfg if method else None, attack_method=method,
                         attack_params=params, batch_size=batch, dataset=data, share_weights=True, shuffle=False, num_workers=0,
                         **({"universal_load": load} if load else {}))
        torch.cuda.synchronize()
        rates.append(n / (time.perf_counter() - t0))
    return rates[1:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=128)
    ap.add_argument("--T", type=int, default=64_600)
    ap.add_argument("--iters", type=int, default=96)
    ap.add_argument("--eager_launch", action="store_true", help="launch from Python inside the window instead of replaying a graph")
    ap.add_argument("--blocks", type=int, default=15)
    ap.add_argument("--loop", type=int, default=0, metavar="N")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no HIP device: this is a measurement, there is nothing to fall back to")
    dev = torch.device("cuda")
    B, T = args.B, args.T
    result = {"B": B, "T": T, "iters": args.iters, "blocks": args.blocks, "window": "python launches" if args.eager_launch else "graph replay"}
    ok = True
    for sets in (1, 8):
        g = torch.Generator(device=dev).manual_seed(sets)
        bufs = [(torch.randn(B, T, device=dev, generator=g) * 1e-3, torch.rand(B, T, device=dev, generator=g),
                 torch.empty(B, T, device=dev)) for _ in range(sets)]
        w = torch.rand(B, device=dev, generator=g) + 0.5
        delta = (torch.rand(T, device=dev, generator=g) * 2 - 1) * 0.001
        s_out = torch.empty(1, T, device=dev)

        def colsum(k):
            hip_ops.universal_colsum(bufs[k % sets][0], w, out=s_out)

        def colsum_eager(k):
            (bufs[k % sets][0] * w[:, None]).sum(0)

        def apply(k):
            hip_ops.universal_apply(bufs[k % sets][1], delta, w, out=bufs[k % sets][2])

        def apply_eager(k):
            torch.clamp(bufs[k % sets][1] + w[:, None] * delta, 0, 1)

        same = torch.allclose(hip_ops.universal_colsum(bufs[0][0], w).reshape(-1), (bufs[0][0] * w[:, None]).sum(0), rtol=1e-4,
                              atol=1e-7)
        same = same and torch.equal(hip_ops.universal_apply(bufs[0][1], delta, w), torch.clamp(bufs[0][1] + w[:, None] * delta, 0, 1))
        result[f"sets{sets}/outputs_agree"] = bool(same)
        for pair, per_sample in (({"universal_colsum": colsum, "eager_colsum": colsum_eager}, 4),
                                 ({"universal_apply": apply, "eager_apply": apply_eager}, 8)):
            times = timed_pairs(pair, args.iters, args.blocks, not args.eager_launch)
            med = {name: statistics.median(t) for name, t in times.items()}
            for name, t in times.items():
                tbs = per_sample * B * T / (med[name] * 1e-6)
                print(f"sets={sets} {name}: median {med[name]:.2f} us (min {min(t):.2f}, max {max(t):.2f}), {per_sample} B/sample "
                      f"-> {tbs / 1e12:.2f} TB/s = {100 * tbs / HBM_PEAK:.0f} % of HBM peak")
                result[f"{name}/sets{sets}/us"] = round(med[name], 3)
                result[f"{name}/sets{sets}/us_min"] = round(min(t), 3)
                result[f"{name}/sets{sets}/us_max"] = round(max(t), 3)
                result[f"{name}/sets{sets}/TBps"] = round(tbs / 1e12, 3)
                result[f"{name}/sets{sets}/hbm_share"] = round(tbs / HBM_PEAK, 3)
            fused, eager = list(pair)
            spread = max(times[fused]) - min(times[fused])
            holds = med[fused] <= med[eager] + spread
            ok = ok and holds
            print(f"sets={sets} {fused} <= {eager} + spread ({spread:.2f} us): {holds}  ({med[eager] / med[fused]:.2f}x)")
            result[f"{fused}/sets{sets}/no_slower_than_eager"] = bool(holds)
        del bufs
    if args.loop:
        from audio_deepfake_adversarial_attacks_amd import torchattacks
        from audio_deepfake_adversarial_attacks_amd.models.models import get_model
        with tempfile.TemporaryDirectory() as tmp:
            path = Path(tmp) / "uap.npz"
            atk = torchattacks.UniversalPGD(get_model("lcnn", {"frontend_algorithm": ["lfcc"], "input_channels": 1}, "cuda").to(dev),
                                            source_label=0)
            atk._delta = ((torch.rand(1, T, device=dev) * 2 - 1) * 0.0005).contiguous()
            atk.save_delta(path)
            result["loop/utterances"] = args.loop
            result["loop/UAP_SPOOF_loaded/utt_per_s"] = [round(r, 1) for r in loop_rate(args.loop, B, T, "UAP_SPOOF", str(path))]
            result["loop/NO_ATTACK/utt_per_s"] = [round(r, 1) for r in loop_rate(args.loop, B, T, "NO_ATTACK")]
        print(f"loop, {args.loop} utterances, batch {B}: loaded UAP_SPOOF {result['loop/UAP_SPOOF_loaded/utt_per_s']} utt/s, "
              f"NO_ATTACK {result['loop/NO_ATTACK/utt_per_s']} utt/s")
    result["each_fused_op_no_slower_than_eager"] = bool(ok)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
