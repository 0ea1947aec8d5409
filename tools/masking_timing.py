"""The measurement behind DESIGN.md's PsyPGD section (needs a HIP device): the masking kernels at the flagship batch shape.

    masking_hinge_grad(adv, x, theta -> grad, stats)   a zero fill and one launch.  Traffic floor: adv, x read (8 B per sample), theta
                                                 read (257 * 4 B per hop = 8 B per sample at hop 128), grad zero-filled and written
                                                 (8 B): 24 B per sample
        against   the eager formulation: torch.stft(adv - x) -> |.|^2 -> relu(. - theta).sum() and autograd back through it
        against   the frontend's own forward + backward pair (advstep_stft_bands_f32 + advstep_stft_bands_backward_f32 on the LFCC
                  filterbank): the same two transforms in two launches, with the band rows through memory
    psy_step(cur, g_ce, g_mask, x -> out)            two passes over the gradients; model: 24 B per sample (the second pass re-reads
                                                 the gradients from L2)
    stft_power(x -> P)                               once per batch (the threshold)

Method: tools/universal_probe.py's `timed_pairs` — versions warmed up, then timed in alternating blocks; for the library kernels a
block is one replay of a hipGraph of `--iters` launches (device time only), for the eager formulation `--iters` launches from
Python (its kernels are long enough to keep the queue full).  Median block, min .. max.  `--loop N` adds a PSYPGD evaluation run
over N synthetic utterances on LCNN and the share of its wall time spent in the two kernels.

    python tools/masking_timing.py [--B 128 --T 64600 --hop 128 --iters 32 --blocks 9 --loop 512] [--out profiles/masking_timing.txt]"""
import argparse
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from audio_deepfake_adversarial_attacks_amd import _lib, frontend_ops, frontends, hip_ops  # noqa: E402
from audio_deepfake_adversarial_attacks_amd.torchattacks import MaskingModel  # noqa: E402
from universal_probe import timed_pairs  # noqa: E402  (tools/ is the script's directory)

ROW_RATE = 6.2e12      # bytes / s the row kernels reach on this part


def loop_figures(n_utt, batch, T):
    from audio_deepfake_adversarial_attacks_amd.aa.aa_types import AttackEnum
    from audio_deepfake_adversarial_attacks_amd.datasets.synthetic import SyntheticDetectionDataset
    from audio_deepfake_adversarial_attacks_amd.evaluation import generate_attacks
    cfg = {"data": {"seed": 42}, "checkpoint": {"path": ""},
           "model": {"name": "lcnn", "parameters": {"frontend_algorithm": ["lfcc"], "input_channels": 1}}}
    method, params = AttackEnum["PSYPGD"].value

    def run(n, profile):
        data = SyntheticDetectionDataset(n, num_samples=T)
        if profile:
            hip_ops.start_profile("masking_hinge_grad", "psy_step", "stft_power", graph_ok=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rep = generate_attacks([None, None, None], cfg, "cuda", attack_model_config=cfg, attack_method=method, attack_params=params,
                               batch_size=batch, dataset=data, share_weights=True, shuffle=False, num_workers=0)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        return rep, wall, (hip_ops.stop_profile() if profile else {})

    run(2 * batch, False)                                              # warms kernels, plans, captures and the allocator up
    rep, wall, _ = run(n_utt, False)
    _, wall_p, ms = run(n_utt, True)
    out = {"loop/utterances": n_utt, "loop/PSYPGD/utt_per_s": round(n_utt / wall, 2), "loop/PSYPGD/wall_s": round(wall, 3),
           "loop/PSYPGD/profiled_wall_s": round(wall_p, 3)}
    for k, v in ms.items():
        out[f"loop/PSYPGD/{k}_s"] = round(sum(v) / 1e3, 4)
        out[f"loop/PSYPGD/{k}_share"] = round(sum(v) / 1e3 / wall_p, 4)
    out.update({k: v for k, v in rep.items() if k.startswith("masking/")})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=128)
    ap.add_argument("--T", type=int, default=64_600)
    ap.add_argument("--hop", type=int, default=128)
    ap.add_argument("--iters", type=int, default=32)
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--loop", type=int, default=0)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    B, T, hop = a.B, a.T, a.hop
    NF = 1 + T // hop
    g = torch.Generator(device="cpu").manual_seed(0)
    x = torch.rand(B, T, generator=g).to(dev)
    adv = (x + 0.002 * (torch.rand(B, T, generator=g).to(dev) - 0.5)).clamp(0, 1)
    g_ce = torch.randn(B, T, generator=g).to(dev)
    mm = MaskingModel(hop=hop)
    window = mm.window(dev)
    # a threshold that about 40 % of the cells exceed (the share the tests use): the overlap-add skips sums that are exactly 0,
    # so a perturbation that is masked everywhere would time a cheaper kernel
    Pd = hip_ops.stft_power(adv, x, window, hop)
    theta = Pd.median() * (0.3 + 2.7 * torch.rand(Pd.shape, generator=g).to(dev))
    s = 1.0 / (Pd.amax(dim=(1, 2)) * float(NF * 257))
    grad, stats, out, power = torch.empty_like(x), torch.empty(B, 3, device=dev), torch.empty_like(x), torch.empty_like(theta)

    # the frontend's own pair on the LFCC filterbank, through the C ABI
    lib = _lib.load()
    tables = frontend_ops.filterbank_tables(frontends.LFCC().filter_mat.to(dev))
    M = int(tables.fb_start.numel())
    band = torch.empty(B, NF, M, device=dev)
    bmax = torch.empty(max(lib.advstep_stft_bands_block_count(B, NF), 1), device=dev)
    dband = torch.randn(B, NF, M, device=dev)
    dx = torch.empty_like(x)

    def frontend_pair(_):
        st = torch.cuda.current_stream().cuda_stream
        _lib.check(lib.advstep_stft_bands_f32(adv.data_ptr(), window.data_ptr(), tables.fb_start.data_ptr(), tables.fb_w.data_ptr(),
                                              tables.span, band.data_ptr(), bmax.data_ptr(), B, T, NF, hop, 512, M, st), "bands")
        _lib.check(lib.advstep_stft_bands_backward_f32(adv.data_ptr(), window.data_ptr(), dband.data_ptr(), tables.fbt_start.data_ptr(),
                                                       tables.fbt_w.data_ptr(), tables.span_t, dx.data_ptr(), B, T, NF, hop, 512, M, st),
                   "bands_backward")

    def eager(_):
        d = (adv - x).requires_grad_(True)
        X = torch.stft(d, 512, hop_length=hop, window=window, center=True, pad_mode="reflect", return_complex=True)
        P = (X.real ** 2 + X.imag ** 2).transpose(1, 2)
        loss = (s * torch.relu(P - theta).sum(dim=(1, 2))).sum()
        return torch.autograd.grad(loss, d)[0]

    ref = eager(0)
    got, st0 = hip_ops.masking_hinge_grad(adv, x, window, theta, s, hop)
    active = (st0[:, 1].mean() / (NF * 257)).item()
    agree =((got - ref).abs().amax(dim=1) / ref.abs().amax(dim=1).clamp_min(1e-30)).max().item()

    fused = {"masking_hinge_grad": lambda _: hip_ops.masking_hinge_grad(adv, x, window, theta, s, hop, out=grad, stats=stats),
             "frontend forward + backward pair": frontend_pair,
             "psy_step": lambda _: hip_ops.psy_step(adv, g_ce, grad, x, 1.0, 1e-4, 1e-3, out=out),
             "stft_power": lambda _: hip_ops.stft_power(x, None, window, hop, out=power)}
    times = timed_pairs(fused, a.iters, a.blocks, graph=True)
    times.update(timed_pairs({"eager stft + autograd hinge": eager,
                              "masking_hinge_grad (launched from Python)": fused["masking_hinge_grad"]}, max(a.iters // 4, 4),
                             a.blocks, graph=False))
    floor_us = 24.0 * B * T / ROW_RATE * 1e6
    lines = [f"masking kernels at ({B}, {T}), hop {hop}, NF {NF}, hot; us per launch: median (min .. max) over {a.blocks} blocks",
             f"traffic floor of the hinge: 24 B per sample = {24.0 * B * T / 1e6:.1f} MB = {floor_us:.1f} us at {ROW_RATE / 1e12:.1f} TB/s",
             f"{active:.2f} of the cells are over the threshold; eager (float32 torch.stft) and fused gradients differ by at most "
             f"{agree:.2e} of a row's scale (cells within float32 rounding of the threshold fall either side: each moves the "
             "gradient by a whole cell's term; tests/test_gpu_masking.py holds the kernel to 1e-6 against float64)"]
    for name, t in times.items():
        lines.append(f"{name:45s} {statistics.median(t):9.1f} ({min(t):.1f} .. {max(t):.1f})")
    hinge = statistics.median(times["masking_hinge_grad"])
    lines.append(f"hinge / floor: {hinge / floor_us:.2f}; eager / hinge: "
                 f"{statistics.median(times['eager stft + autograd hinge']) / hinge:.1f}; pair / hinge: "
                 f"{statistics.median(times['frontend forward + backward pair']) / hinge:.2f}")
    if a.loop:
        for k, v in loop_figures(a.loop, B, T).items():
            lines.append(f"{k}: {v}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)


if __name__ == "__main__":
    main()
