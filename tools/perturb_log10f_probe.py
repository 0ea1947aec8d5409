"""The measurement behind DESIGN.md section 4q's log10f allowance (needs a HIP device): over the rows of
tests/test_gpu_perturb.py::test_kernel_against_float64, re-add the sums of hip_ops.perturbation_stats on the host in the kernel's
order (csrc/perturb.hip; checked bit for bit against the energy, l2 and l1_mean planes), then compare snr_db with 10 log10 in
float64 of the float32 quotient the kernel itself formed (`log_stage_db`), and with the float64 reference less the derived
sum term (`beyond_sum_term_db`).  Prints one line per case and the maxima as JSON.

    python tools/perturb_log10f_probe.py"""
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from audio_deepfake_adversarial_attacks_amd import hip_ops  # noqa: E402
from tests import perturb_ref as R  # noqa: E402
from tests.test_gpu_perturb import CASES, K_DB, U, chain, make_case  # noqa: E402

f32 = np.float32


def butterfly(v):
    for off in (32, 16, 8, 4, 2, 1):
        v = (v + v[..., np.arange(64) ^ off]).astype(f32)
    return v[..., 0]


def wg(v):
    w = butterfly(v.reshape(v.shape[:-1] + (4, 64)))
    return (((w[..., 0] + w[..., 1]).astype(f32) + w[..., 2]).astype(f32) + w[..., 3]).astype(f32)


def tile_sums(a):
    B, T = a.shape
    C = -(-T // 4096)
    p = np.zeros((B, C * 4096), dtype=f32)
    p[:, :T] = a
    p = p.reshape(B, C, 4, 256, 4)
    q = ((p[..., 0] + p[..., 1]).astype(f32) + (p[..., 2] + p[..., 3]).astype(f32)).astype(f32)
    acc = np.zeros((B, C, 256), dtype=f32)
    for j in range(4):
        acc = (acc + q[:, :, j]).astype(f32)
    return wg(acc)


def row_sum(part):
    B, C = part.shape
    v = np.zeros((B, 256), dtype=f32)
    for i in range(C):
        v[:, i % 256] = (v[:, i % 256] + part[:, i]).astype(f32)
    return wg(v)


def main():
    dev = torch.device("cuda:0")
    worst_log, worst_literal, worst_seg, rows = 0.0, -1.0, 0.0, []
    for B, T, shift in CASES:
        x, adv, planted = make_case(B, T, seed=CASES.index((B, T, shift)))
        buf_x = torch.zeros(B * T + 8, device=dev)
        buf_a = torch.zeros(B * T + 8, device=dev)
        xd, ad = buf_x[shift:shift + B * T].view(B, T), buf_a[shift:shift + B * T].view(B, T)
        xd.copy_(torch.from_numpy(x)), ad.copy_(torch.from_numpy(adv))
        got = hip_ops.perturbation_stats(xd, ad).cpu().numpy()
        d = R.difference(x, adv)
        ref = R.perturb_ref(x, d)
        with np.errstate(all="ignore"):
            ex = row_sum(tile_sums((x * x).astype(f32)))
            ed = row_sum(tile_sums((d * d).astype(f32)))
            l1 = row_sum(tile_sums(np.abs(d)))
            same = (np.array_equal(ex, got[3], equal_nan=True), np.array_equal(np.sqrt(ed).astype(f32), got[2], equal_nan=True),
                    np.array_equal((l1 / f32(T)).astype(f32), got[1], equal_nan=True))
            r32 = (ex / ed).astype(f32)
            want = 10.0 * np.log10(r32.astype(np.float64))
        fin = np.isfinite(ref[4])
        dev_log = np.abs(got[4].astype(np.float64) - want)[fin]
        literal = (np.abs(got[4].astype(np.float64) - ref[4]) - K_DB * (2 * (chain(T) + 1) + 1) * U)[fin]
        seg = np.abs(got[5].astype(np.float64) - ref[5])[np.isfinite(ref[5])]
        row = {"case": [B, T, shift], "sums_bit_equal": [bool(s) for s in same],
               "log_stage_db": float(dev_log.max()) if dev_log.size else None,
               "beyond_sum_term_db": float(literal.max()) if literal.size else None,
               "snr_db_range": [float(ref[4][fin].min()), float(ref[4][fin].max())] if fin.any() else None,
               "seg_abs_err_db": float(seg.max()) if seg.size else None}
        rows.append(row)
        print(row, flush=True)
        if dev_log.size:
            worst_log, worst_literal = max(worst_log, dev_log.max()), max(worst_literal, literal.max())
        if seg.size:
            worst_seg = max(worst_seg, seg.max())
    out = {"rows": rows, "log_stage_db_max": worst_log, "beyond_sum_term_db_max": worst_literal, "seg_abs_err_db_max": worst_seg}
    print(json.dumps({k: v for k, v in out.items() if k != "rows"}))


if __name__ == "__main__":
    main()
