#!/usr/bin/env python
"""Every entry point of include/advstep_apgdl1.h and include/advstep_l0.h on fixed seeded inputs, all outputs (the stats planes
included) into one .npz — to show that two builds of the library compute the same bits (l1-APGD is tested to an absolute
tolerance only).  Sibling of tools/fab_kernel_outputs.py, which does the same for include/advstep_fab.h; the three files share
row_workgroup.h's digit_search.  The library is the one ADVSTEP_LIB names (default: the in-tree build); one process per build.

    ADVSTEP_LIB=/path/to/other/libadvstep.so python tools/row_search_outputs.py a.npz
    python tools/row_search_outputs.py b.npz
    python tools/row_search_outputs.py --compare a.npz b.npz       # np.array_equal on the uint32 views, per array
"""
import math
import sys
import types
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

R = 6          # rows per case
EPS = 12.0     # the L1 radius
NAN, INF = math.nan, math.inf
CASES = []     # (name, description), in the order they ran


def compare(path_a, path_b):
    a, b = np.load(path_a), np.load(path_b)
    names = sorted(set(a.files) | set(b.files))
    bad = 0
    for n in names:
        same = n in a.files and n in b.files and a[n].shape == b[n].shape and a[n].dtype == b[n].dtype
        if same:  # float32 by its bits (NaN payloads and signed zeros count); the checkpoint's uint8 flags as they are
            same = np.array_equal(a[n].view(np.uint32), b[n].view(np.uint32)) if a[n].dtype == np.float32 else np.array_equal(a[n], b[n])
        bad += not same
        print(f"{n:44s} {str(a[n].shape) if n in a.files else '-':14s} {'equal' if same else 'DIFFERENT'}")
    print(f"{len(names)} arrays, {bad} different")
    return 1 if bad else 0


def main(out_path):
    import torch
    from audio_deepfake_adversarial_attacks_amd import hip_ops as ops
    dev = torch.device("cuda:0")
    res = {}

    def keep(name, *tensors):
        for i, t in enumerate(tensors):
            res[f"{name}.{i}"] = t.detach().cpu().numpy().copy()

    def all_entry_points(name, T, what, shift=False):
        CASES.append((name, f"T = {T}: {what}"))
        gen = torch.Generator().manual_seed(T + 7 * shift)

        def on_gpu(x):
            """A device copy; shift: the same values one float past a 16-byte boundary (rows no longer float4-addressable)."""
            if not shift or x.shape != (R, T):
                return x.to(dev)
            flat = torch.empty(x.numel() + 1, dtype=x.dtype, device=dev)
            flat[1:].copy_(x.reshape(-1))
            return flat[1:].view(x.shape)

        x = torch.rand(R, T, generator=gen) * 0.98 + 0.01
        x[:, ::7] = 0.0
        x[:, 3::11] = 1.0
        x[2] = torch.where((x[2] == 0.0) | (x[2] == 1.0), x[2], torch.full_like(x[2], 0.5))   # the tie row
        noise = torch.randn(R, T, generator=gen)
        sparse = (torch.rand(R, T, generator=gen) < 0.1).float()

        # u of the projections.  rows: 0 x + N(0, 1); 1 feasible for both balls (5 interior samples off x by 1e-3: the L1 search
        # is skipped, L0 keeps them all from k = 16 on); 2 the tie row (every interior sample moves by the same amount);
        # 3 a 10 %-sparse 1e-3 step; 4 u = x; 5 x + 5 N(0, 1) (almost every sample capped by the box)
        u = x + noise
        u[1] = x[1]
        u[1, [1, 2, 4, 5, 6]] += 1e-3
        u[3] = x[3] + 1e-3 * noise[3] * sparse[3]
        u[4] = x[4]
        u[5] = x[5] + 5.0 * noise[5]
        u_l1, u_l0 = u.clone(), u.clone()
        u_l1[2] = x[2] + 0.01 * torch.sign(noise[2])
        u_l0[2] = x[2] + 0.25 * torch.sign(noise[2])

        # gradients of the steps.  rows: 0 random; 1 zero; 2 the tie row (|g| equal everywhere); 3 one NaN; 4 zeros at every
        # 13th sample; 5 random, a few +-inf
        grad = 1e-3 * torch.randn(R, T, generator=gen)
        grad[1] = 0.0
        grad[2] = 1e-3 * torch.sign(noise[2])
        grad[3, 7] = NAN
        grad[4, ::13] = 0.0
        grad[5, [0, 9]] = torch.tensor([INF, -INF])

        xd = on_gpu(x)
        # ---- include/advstep_apgdl1.h ----
        keep(f"{name}.l1_box_project", ops.l1_box_project(xd, on_gpu(u_l1), EPS))
        alias = on_gpu(u_l1)
        ops.l1_box_project(xd, alias, EPS, out=alias)
        keep(f"{name}.l1_box_project_onto_u", alias)
        keep(f"{name}.apgdl1_init_draw", ops.apgdl1_init(xd, EPS, draw=on_gpu(noise)))
        start = ops.apgdl1_init(xd, EPS, seed=1234 + T, offset=8)
        keep(f"{name}.apgdl1_init_philox", start)
        cur = start.cpu()
        cur[1] = x[1]                                                        # with its zero gradient: a feasible row
        step_size = torch.tensor([EPS, EPS / 10, EPS / 2, EPS, 0.3 * EPS, EPS])
        topk = torch.tensor([0.2, 0.2, 0.2, 1.0, 0.0, NAN])
        for label, tk in (("", topk), ("_topk_rolled", topk.roll(3))):      # every row under two topk of {0, 0.2, 1, NaN}
            keep(f"{name}.apgdl1_step{label}", *ops.apgdl1_step(on_gpu(cur), on_gpu(grad), xd, step_size.to(dev), tk.to(dev), EPS,
                                                               return_stats=True))
        state = types.SimpleNamespace(flags=torch.tensor([2, 0, 6, 4, 3, 0], dtype=torch.uint8, device=dev),
                                      sp_old=torch.tensor([T / 2, 5.0, T / 1.0, 1.0, T / 3, 2.0], device=dev),
                                      topk=topk.nan_to_num(0.1).to(dev), step_size=step_size.to(dev))
        ops.apgdl1_checkpoint(on_gpu(cur), on_gpu(u_l1.clamp(0, 1)), xd, state, EPS)
        keep(f"{name}.apgdl1_checkpoint", state.flags, state.sp_old, state.topk, state.step_size)

        # ---- include/advstep_l0.h ----
        cur0 = (x + 1e-3 * noise * sparse).clamp(0.0, 1.0)
        cur0[1] = x[1]
        cur0[1, [1, 2, 4, 5, 6]] += 1e-3
        cur0[2] = x[2]
        for k in (1, 16, T):
            for cap_name, eps_inf in (("", INF), ("_capped", 0.05)):         # without and with eps_inf
                keep(f"{name}.l0_box_project.k{k}{cap_name}", ops.l0_box_project(xd, on_gpu(u_l0), k, eps_inf))
                keep(f"{name}.pgdl0_step.k{k}{cap_name}",
                     *ops.pgdl0_step(on_gpu(cur0), on_gpu(grad), xd, 0.15 * T, k, eps_inf, return_stats=True))
        alias = on_gpu(cur0)
        ops.pgdl0_step(alias, on_gpu(grad), xd, 0.15 * T, 16, out=alias)
        keep(f"{name}.pgdl0_step_onto_cur", alias)

    all_entry_points("T257", 257, "scalar, less than one pass of the workgroup")
    all_entry_points("T4099", 4099, "scalar")
    all_entry_points("T4100", 4100, "float4, 1025 quads: the strided loop runs twice with one thread left over")
    all_entry_points("T64600", 64600, "float4, the repo's row length")
    all_entry_points("T4100_shifted", 4100, "T % 4 == 0 with every (R, T) base one float past alignment: scalar", shift=True)

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
