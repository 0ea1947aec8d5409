#!/usr/bin/env python
"""Every FAB entry point (include/advstep_fab.h) on fixed seeded inputs, all outputs into one .npz — to show that two
builds of the library compute the same bits (the tests compare against float64 at 2e-5 / 8e-3 and would not see a
changed summation order).  The library is the one ADVSTEP_LIB names (default: the in-tree build); one process per build.

    ADVSTEP_LIB=/path/to/other/libadvstep.so python tools/fab_kernel_outputs.py a.npz
    python tools/fab_kernel_outputs.py b.npz
    python tools/fab_kernel_outputs.py --compare a.npz b.npz       # np.array_equal on the uint32 views, per array
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

NORMS = ("Linf", "L2", "L1")
CASES = []   # (name, description), in the order they ran


def compare(path_a, path_b):
    a, b = np.load(path_a), np.load(path_b)
    names = sorted(set(a.files) | set(b.files))
    bad = 0
    for n in names:
        assert all(n not in f.files or f[n].dtype == np.float32 for f in (a, b)), f"{n}: the uint32 view needs float32"
        same = n in a.files and n in b.files and a[n].shape == b[n].shape and np.array_equal(a[n].view(np.uint32),
                                                                                             b[n].view(np.uint32))
        bad += not same
        print(f"{n:44s} {str(a[n].shape) if n in a.files else '-':14s} {'equal' if same else 'DIFFERENT'}")
    print(f"{len(names)} arrays, {bad} different")
    return 1 if bad else 0


def main(out_path):
    import torch
    from audio_deepfake_adversarial_attacks_amd import hip_ops as ops
    dev = torch.device("cuda:0")
    res = {}

    def on_gpu(x, shift=False):
        """A device copy; shift: the same values one float past a 16-byte boundary (rows no longer float4-addressable)."""
        if not shift:
            return x.to(dev)
        flat = torch.empty(x.numel() + 1, dtype=x.dtype, device=dev)
        flat[1:].copy_(x.reshape(-1))
        return flat[1:].view(x.shape)

    def keep(name, *tensors):
        for i, t in enumerate(tensors):
            res[f"{name}.{i}"] = t.detach().cpu().numpy().copy()

    def projection_rows(R, T, gen):
        """tests/helpers.fab_projection_inputs' rows: exact 0 / 1 points, zero normals, near to out-of-reach planes."""
        t = torch.rand(R, T, generator=gen)
        t[:, ::7] = 0.0
        t[:, 3::11] = 1.0
        w = torch.randn(R, T, generator=gen) * 0.01
        w[:, ::13] = 0.0
        b = (w * t).sum(1) + torch.tensor([1e-4, -1e-3, 0.05, -0.2, 0.45, 5.0])[torch.arange(R) % 6] * w.abs().sum(1)
        return t, w, b

    def all_entry_points(name, T, what, shift=False):
        CASES.append((name, f"T = {T}: {what}"))
        gen = torch.Generator().manual_seed(T + 7 * shift)
        R = 6
        t, w, b = projection_rows(R, T, gen)
        gz = torch.randn(R, T, generator=gen) * 1e-3
        z = torch.tensor([2.5, -1.0, 0.0, 1e-3, -30.0, 4.0])
        la = torch.tensor([1, 0, 1, 0, 0, 0])
        x0 = torch.rand(R, T, generator=gen)
        x1 = (x0 + torch.randn(R, T, generator=gen) * 0.01).clamp(0, 1)
        adv = torch.rand(R, T, generator=gen)
        d1, d2 = torch.randn(R, T, generator=gen) * 0.1, torch.randn(R, T, generator=gen) * 0.1
        n1 = torch.tensor([0.3, 0.0, 1e-9, 5.0, 0.2, 0.7])
        n2 = torch.tensor([0.1, 0.0, 2.0, 1e-3, 0.2, 0.1])
        flags = torch.tensor([1, 1, 1, 0, 0, 1], dtype=torch.uint8)      # rows 3, 4: not adversarial
        for norm in NORMS:
            keep(f"{name}.projection.{norm}", *ops.fab_projection(on_gpu(t, shift), on_gpu(w, shift), b.to(dev), norm))
            keep(f"{name}.hyperplane.{norm}", *ops.fab_hyperplane(on_gpu(gz, shift), on_gpu(t, shift), z.to(dev), la.to(dev), norm))
            keep(f"{name}.hyperplane_stats.{norm}", *ops.fab_hyperplane(on_gpu(gz, shift), on_gpu(t, shift), None, None, norm)[2:])
            big = float((x1 - x0).abs().sum(1).max()) * 2                # above every norm of every row
            res2 = torch.tensor([1e10, 1e-6, big, 1e10, 1e-6, big])      # rows 1, 4: farther than their best
            g1, ga, gr = on_gpu(x1, shift), on_gpu(adv, shift), res2.to(dev)
            ops.fab_backward_step(g1, on_gpu(x0, shift), ga, gr, flags.to(dev), 0.9, norm)
            keep(f"{name}.backward_step.{norm}", g1, ga, gr)
        args = [on_gpu(v, shift) for v in (x1, x0, d1, d2)] + [n1.to(dev), n2.to(dev)]
        keep(f"{name}.combine", ops.fab_combine(*args, 1.05, 0.1))
        assert ops.fab_combine(*args, 10.0, 0.1, out=args[0]) is args[0]
        keep(f"{name}.combine_onto_x1", args[0])

    all_entry_points("T257", 257, "scalar, less than one pass of the workgroup")
    all_entry_points("T4099", 4099, "scalar")
    all_entry_points("T4100", 4100, "float4, 1025 quads: the strided loop runs twice with one thread left over")
    all_entry_points("T64600", 64600, "float4, the repo's row length")
    all_entry_points("T4100_shifted", 4100, "T % 4 == 0 with every (R, T) base one float past alignment: scalar", shift=True)

    CASES.append(("shared_normals", "projection, T = 2048, R = 10, w_rows = R / 2, wscale = (2, -2, 2, 0, -2)"))
    gen = torch.Generator().manual_seed(3)
    pts, gz = torch.rand(10, 2048, generator=gen), torch.randn(5, 2048, generator=gen) * 0.02
    wscale, b = torch.tensor([2.0, -2.0, 2.0, 0.0, -2.0]), torch.randn(10, generator=gen) * 0.5
    for norm in NORMS:
        keep(f"shared_normals.projection.{norm}", *ops.fab_projection(pts.to(dev), gz.to(dev), b.to(dev), norm, wscale.to(dev)))

    CASES.append(("edge_rows", "projection, T = 515: on the hyperplane, saturated points, all |w| equal (L1's tie-group scan)"))
    gen = torch.Generator().manual_seed(9)
    t = torch.rand(4, 515, generator=gen)
    t[1] = (t[1] > 0.5).float()
    w = torch.randn(4, 515, generator=gen) * 0.05
    w[2] = w[2].sign() * 0.03
    b = (w * t).sum(1) + torch.tensor([0.0, 0.2, -0.4, 1e-7])
    for norm in NORMS:
        keep(f"edge_rows.projection.{norm}", *ops.fab_projection(t.to(dev), w.to(dev), b.to(dev), norm))

    torch.cuda.synchronize()
    np.savez(out_path, **res)
    for name, what in CASES:
        print(f"case {name:16s} {what}")
    print(f"{len(res)} arrays -> {out_path}")
    return 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1]))
