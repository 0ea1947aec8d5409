"""The measurement behind DESIGN.md's universal-filter section (needs a HIP device): the three kernels of include/advstep_filter.h at
the flagship batch shape, with HIP events, each priced against both derived floors, and beside what stood in for them before.

    filter_apply(x -> (B, T))           against   channel_apply(K = 1, the taps replicated per row) + eager clamp      (L <= 255)
                                                  models: 8 B per sample;  2 L unfused float32 operations per sample
    filter_tap_grad((B, T) x 3 -> ws)   against   the eager FFT formulation: irfft(conj(rfft(gm)) rfft(xc)), summed over the rows
                                                  models: 12 B per sample;  2 L operations per sample, fused (fmaf)
    filter_tap_update(ws -> L taps)     alone:    4 B per partial (B ceil(T / 4096) L floats); one thread per tap adds B ceil(T /
                                                  4096) partials in the fixed order, so its time is that chain's latency

Method and output format are tools/channel_probe.py's (tools/universal_probe.py's `timed_pairs`): the versions of a pair are
warmed up, then timed in alternating blocks of `--iters` launches, a block being one replay of a hipGraph of those launches;
median block, min .. max over the blocks; once with the launches rotating over one set of input buffers (hot) and once over
eight (from HBM).  Floors: the byte model at the 8 TB/s HBM peak; 2 L B T operations at HALF the 157.3 TFLOP/s vector peak for the
forward's separate v_mul_f32 / v_add_f32 and at the whole of it for the tap gradient's v_fmac_f32: a wave64 vector instruction
issues in 2 cycles, 32 lanes per SIMD and clock, so 256 CUs x 4 SIMDs x 32 lanes x 2.4 GHz = 78.6 T instructions-lanes per second,
and the peak is a fused multiply-add in every one of them.  (The first version of this probe priced both at half these rates,
the floors the feature was designed against: 107 and 54 us at L = 255.  filter_apply then ran UNDER its floor, at 100 us, with no
packed instruction in its code — the floor was wrong, not the clock.)  filter_apply is the channel's arithmetic with fewer loads: where it is slower than the K = 1
channel pair beyond the two measurements' own min .. max spread, the file says so in a line that begins with DEFECT.

`--loop N` adds one FILTER_SPOOF run over N synthetic utterances on LCNN: utterances / s of the frozen-filter loop (the filter
fitted on the first batch, saved, and the run repeated with `universal_load`), and the share of a fit step's wall time that the
three kernels' launches take (HIP events round every launch, `hip_ops.start_profile`).

    python tools/filter_probe.py [--B 128 --T 64600 --L 129 255 1025 --iters 12 --blocks 9 --loop 1024] [--out profiles/filter_timing.txt]"""
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
from universal_probe import HBM_PEAK, loop_rate, timed_pairs  # noqa: E402  (tools/ is the script's directory)

VECTOR_PEAK = 157.3e12               # float32 operations per second: a fused multiply-add per lane, 32 lanes per SIMD and clock
TILE = 4096


def eager_tap_grad(x, center, grad, out_adv, L):
    """dh (L,) by three batched FFTs: corr[k] = sum_t gm[t] xc[t + k], k = P - i, summed over the rows."""
    B, T = x.shape
    P = (L - 1) // 2
    gm = torch.where((out_adv > 0) & (out_adv < 1), grad, torch.zeros_like(grad))
    n = T + L
    corr = torch.fft.irfft(torch.fft.rfft(gm, n).conj() * torch.fft.rfft(x - center[:, None], n), n).sum(0)
    return corr[(P - torch.arange(L, device=x.device)) % n]


def loop_figures(n_utt, batch, T):
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    from audio_deepfake_adversarial_attacks_amd.aa.aa_types import AttackEnum
    from audio_deepfake_adversarial_attacks_amd.datasets.synthetic import synthetic_waveforms
    from audio_deepfake_adversarial_attacks_amd.models.models import get_model
    _, params = AttackEnum["FILTER_SPOOF"].value
    torch.manual_seed(0)
    model = get_model("lcnn", {"frontend_algorithm": ["lfcc"], "input_channels": 1}, "cuda").to("cuda").eval()
    atk = torchattacks.UniversalFilter(model, **params)
    atk.set_training_mode(model_training=True, batchnorm_training=False)
    x, y = synthetic_waveforms(batch, num_samples=T)
    x01, mn, mx = hip_ops.to_minmax(x.to("cuda"))
    y = y.to("cuda")
    names = ("filter_apply", "filter_tap_grad", "filter_tap_update")

    def steps(n, profile):
        if profile:
            hip_ops.start_profile(*names)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            atk.set_minmax(mn, mx)
            atk.partial_fit(x01, y)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        return wall / n, ({k: sum(v) / 1e3 / n for k, v in hip_ops.stop_profile().items()} if profile else {})

    steps(3, False)
    step_s, _ = steps(10, False)
    step_p, kernels = steps(10, True)
    with tempfile.TemporaryDirectory() as tmp:
        path = str(Path(tmp) / "filter.npz")
        atk.save_delta(path)
        rates = loop_rate(n_utt, batch, T, "FILTER_SPOOF", load=path)
    out = {"loop/utterances": n_utt, "loop/FILTER_SPOOF/frozen_utt_per_s": round(statistics.median(rates), 1),
           "loop/FILTER_SPOOF/fit_step_ms": round(step_s * 1e3, 2), "loop/FILTER_SPOOF/profiled_fit_step_ms": round(step_p * 1e3, 2)}
    for k in names:
        out[f"loop/FILTER_SPOOF/{k}_ms"] = round(kernels.get(k, 0.0) * 1e3, 4)
    out["loop/FILTER_SPOOF/kernel_share"] = round(sum(kernels.values()) / step_p, 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=128)
    ap.add_argument("--T", type=int, default=64_600)
    ap.add_argument("--L", type=int, nargs="+", default=[129, 255, 1025])
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--loop", type=int, default=0, metavar="N")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "filter_timing.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no HIP device: this is a measurement, there is nothing to fall back to")
    dev = torch.device("cuda")
    B, T = args.B, args.T
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("")

    def say(line):                                                                     # line by line: a run that ends early leaves what it measured
        print(line, flush=True)
        with out.open("a") as f:
            f.write(line + "\n")

    result = {"B": B, "T": T, "L": args.L, "iters": args.iters, "blocks": args.blocks, "window": "graph replay"}
    g = torch.Generator(device=dev).manual_seed(1)
    center = torch.rand(B, device=dev, generator=g) * 0.4 + 0.3
    mask = (torch.arange(B, device=dev) % 2 == 0).float()                              # every other row is of the source class
    ones, zeros = torch.ones(1, B, device=dev), torch.zeros(1, B, device=dev)
    for L in args.L:
        P = (L - 1) // 2
        taps = torch.randn(L, device=dev, generator=g) * (0.3 / L ** 0.5)
        taps[P] += 1.0
        shift = torch.full((1, B), -P, dtype=torch.int32, device=dev)
        per_row = taps.reshape(1, 1, L).repeat(1, B, 1).contiguous() if L <= 256 else None
        h, am, av = taps.clone(), torch.zeros(L, device=dev), torch.zeros(L, device=dev)
        ops = 2.0 * L * B * T
        partial_bytes = 4.0 * B * -(-T // TILE) * L
        for sets in (1, 8):
            xs = [torch.rand(B, T, device=dev, generator=g) for _ in range(sets)]
            grads = [torch.randn(B, T, device=dev, generator=g) for _ in range(sets)]
            advs = [hip_ops.filter_apply(x, center, taps) for x in xs]
            outs = [torch.empty(B, T, device=dev) for _ in range(sets)]
            through = torch.empty(1, B, T, device=dev)

            def apply(k):
                hip_ops.filter_apply(xs[k % sets], center, taps, out=outs[k % sets])

            def apply_masked(k):
                hip_ops.filter_apply(xs[k % sets], center, taps, mask, out=outs[k % sets])

            def channel_pair(k):
                hip_ops.channel_apply(xs[k % sets], center, per_row, shift, ones, zeros, 1, 0, out=through)
                torch.clamp(through[0], 0.0, 1.0, out=outs[k % sets])

            def tap_grad(k):
                hip_ops.filter_tap_grad(xs[k % sets], center, grads[k % sets], advs[k % sets], L)

            def tap_grad_eager(k):
                eager_tap_grad(xs[k % sets], center, grads[k % sets], advs[k % sets], L)

            def tap_update(k):
                hip_ops.filter_tap_update(h, am, av, B, T, k + 1, 1e-6)

            forward = {"filter_apply": apply, "filter_apply_masked_half": apply_masked}
            if per_row is not None:
                forward["channel_apply_k1_clamp"] = channel_pair
            tap_grad(0)                                                                # the partials filter_tap_update folds
            for pair, per_sample, peak, launch_bytes in ((forward, 8, VECTOR_PEAK / 2, None),
                                                         ({"filter_tap_grad": tap_grad, "eager_fft_tap_grad": tap_grad_eager}, 12,
                                                          VECTOR_PEAK, None),
                                                         ({"filter_tap_update": tap_update}, 0, None, partial_bytes)):
                times = timed_pairs(pair, args.iters, args.blocks, True)
                med = {name: statistics.median(t) for name, t in times.items()}
                nbytes = launch_bytes if launch_bytes is not None else per_sample * B * T
                floor_bytes = nbytes / HBM_PEAK * 1e6
                floor_ops = ops / peak * 1e6 if peak else 0.0
                bound = "ALU" if floor_ops > floor_bytes else "HBM"
                for name, t in times.items():
                    say(f"L={L} sets={sets} {name}: median {med[name]:.1f} us (min {min(t):.1f}, max {max(t):.1f}); "
                        f"{nbytes / 1e6:.1f} MB -> {nbytes / (med[name] * 1e-6) / 1e12:.2f} TB/s (floor {floor_bytes:.1f} us); "
                        + (f"{2 * L} op/sample -> {ops / (med[name] * 1e-6) / 1e12:.2f} Top/s (floor {floor_ops:.1f} us); " if peak else "")
                        + f"{bound}-bound floor / time = {max(floor_bytes, floor_ops) / med[name]:.2f}")
                    result[f"{name}/L{L}/sets{sets}/us"] = round(med[name], 2)
                    result[f"{name}/L{L}/sets{sets}/us_min"] = round(min(t), 2)
                    result[f"{name}/L{L}/sets{sets}/us_max"] = round(max(t), 2)
                if "eager_fft_tap_grad" in pair:
                    say(f"L={L} sets={sets} eager_fft_tap_grad / filter_tap_grad: {med['eager_fft_tap_grad'] / med['filter_tap_grad']:.2f}x")
                if "channel_apply_k1_clamp" in pair:
                    ours, theirs = times["filter_apply"], times["channel_apply_k1_clamp"]
                    say(f"L={L} sets={sets} channel_apply_k1_clamp / filter_apply: {med['channel_apply_k1_clamp'] / med['filter_apply']:.2f}x")
                    if min(ours) > max(theirs):
                        say(f"DEFECT L={L} sets={sets}: filter_apply (min {min(ours):.1f} us) is slower than the K = 1 channel pair "
                            f"(max {max(theirs):.1f} us) beyond both spreads")
            del xs, grads, advs, outs, through
    if args.loop:
        result.update(loop_figures(args.loop, B, T))
        say(f"loop, FILTER_SPOOF (129 taps), {args.loop} utterances, batch {B}, LCNN: frozen filter "
            f"{result['loop/FILTER_SPOOF/frozen_utt_per_s']} utt/s; a fit step {result['loop/FILTER_SPOOF/fit_step_ms']} ms, of which the "
            f"three kernels take {100 * result['loop/FILTER_SPOOF/kernel_share']:.2f} % (apply {result['loop/FILTER_SPOOF/filter_apply_ms']} "
            f"ms, tap_grad {result['loop/FILTER_SPOOF/filter_tap_grad_ms']} ms, tap_update {result['loop/FILTER_SPOOF/filter_tap_update_ms']} ms)")
    say(json.dumps(result))


if __name__ == "__main__":
    main()
