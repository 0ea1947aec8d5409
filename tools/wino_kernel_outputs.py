#!/usr/bin/env python
"""Every entry point that goes through csrc/lcnn_wino.hip's launch_wino, and both weight-preparation functions in all their
modes, on fixed seeded inputs through the C ABI; all outputs into one .npz — to show that two builds of the library compute
the same bits (the tests compare against float64 with a tolerance and would not see a changed summation order).  The library is
the one ADVSTEP_LIB names (default: the in-tree build); one process per build.  Sibling of tools/fab_kernel_outputs.py.

    ADVSTEP_LIB=/path/to/other/libadvstep.so python tools/wino_kernel_outputs.py a.npz
    python tools/wino_kernel_outputs.py b.npz
    python tools/wino_kernel_outputs.py --compare a.npz b.npz       # np.array_equal on the raw bytes, per array

The cases are the smallest that reach all 48 instantiations of wino3x3_kernel (N <= 3, planes 7 x 10 and 6 x 9): for a reduction
size on each side of 64 (resident / streamed weights) an even and an odd width, output rows whose last slice is half empty
(one-tile launch) and not, 20-channel layers (an odd number of k-steps), K1 + K2 with K2 in {0, 1, 2, 4}, few in {1, 2}, and the
one-slice compact backward with ADVSTEP_WINO_HALVES at both settings.  That every instantiation runs is shown by a kernel
trace of this tool, not here.  Output buffers start from a fill pattern, so what a kernel leaves unwritten is compared too.
"""
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

PLANES = ((2, 7, 10), (3, 6, 9))            # (N, H, W): even width with an odd height, odd width; 15 tiles per sample at N = 3
CASES = []                                  # (name, description), in the order they ran


def compare(path_a, path_b):
    a, b = np.load(path_a), np.load(path_b)
    names = sorted(set(a.files) | set(b.files))
    bad = 0
    for n in names:
        same = (n in a.files and n in b.files and a[n].shape == b[n].shape and a[n].dtype == b[n].dtype
                and np.array_equal(a[n].reshape(-1).view(np.uint8), b[n].reshape(-1).view(np.uint8)))
        bad += not same
        print(f"{n:58s} {str(a[n].shape) if n in a.files else '-':18s} {'equal' if same else 'DIFFERENT'}")
    print(f"{len(names)} arrays, {bad} different")
    return 1 if bad else 0


def main(out_path):
    import torch
    from audio_deepfake_adversarial_attacks_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    res = {}

    def rnd(gen, *shape, scale=1.0):
        return (torch.randn(*shape, generator=gen) * scale).to(dev)

    def codes(gen, high, *shape):
        return torch.randint(0, high, shape, generator=gen, dtype=torch.uint8).to(dev)

    def out_f32(*shape):
        return torch.full(shape, 123.0, device=dev)

    def out_u8(*shape):
        return torch.full(shape, 171, dtype=torch.uint8, device=dev)

    def ptr(t):
        return None if t is None else t.data_ptr()

    def ok(status, what):
        _lib.check(status, what)

    def keep(name, *tensors):
        for i, t in enumerate(tensors):
            res[f"{name}.{i}"] = t.detach().cpu().numpy().copy()

    def case(name, what):
        CASES.append((name, what))
        return torch.Generator().manual_seed(len(CASES) * 7919)

    # ---- LCNN blocks: Conv2d(Cin, 2C, 3) + max-feature-map [+ pool] [+ BatchNorm] and their input gradients -----------------------
    def prepared(weight, gscale, Cin, Cout, mode):
        U = out_f32(lib.advstep_conv3x3_prepared_floats(Cin, Cout, mode))
        ok(lib.advstep_conv3x3_prepare_f32(ptr(weight), ptr(gscale), ptr(U), Cin, Cout, mode, st), "conv3x3_prepare")
        return U

    for Cin, C in ((32, 16), (80, 32)):                 # reduction over Cin: resident (<= 64), streamed
        for N, H, W in PLANES:
            name = f"lcnn_fwd.Cin{Cin}.C{C}.{N}x{H}x{W}"
            gen = case(name, "pooled and un-pooled forward, with bias + BatchNorm and without")
            x, w = rnd(gen, N, Cin, H, W), rnd(gen, 2 * C, Cin, 3, 3, scale=0.1)
            bias, mean, invstd = rnd(gen, 2 * C), rnd(gen, C), (torch.rand(C, generator=gen) + 0.5).to(dev)
            U = prepared(w, None, Cin, 2 * C, 0)
            keep(f"{name}.prepare_mode0", U)
            for tag, b, m, s in (("bias_bn", bias, mean, invstd), ("plain", None, None, None)):
                y, idx = out_f32(N, C, H // 2, W // 2), out_u8(N, C, H // 2, W // 2)
                ok(lib.advstep_conv3x3_mfm_pool2_forward_f32(ptr(x), ptr(U), ptr(b), ptr(m), ptr(s), ptr(y), ptr(idx), N, Cin, C, H, W,
                                                             st), name)
                keep(f"{name}.pool2_forward.{tag}", y, idx)
                y, sel = out_f32(N, C, H, W), out_u8(lib.advstep_conv3x3_mfm_sel_bytes(N, C, H, W))
                ok(lib.advstep_conv3x3_mfm_forward_f32(ptr(x), ptr(U), ptr(b), ptr(m), ptr(s), ptr(y), ptr(sel), N, Cin, C, H, W, st), name)
                keep(f"{name}.mfm_forward.{tag}", y, sel)

    # input gradients, reduction over K = 2C: Cin = 48 has a half-empty last slice (one-tile launch next to the two-tile one),
    # Cin = 32 is the one-slice layer the compact backward runs as two halves
    for Cin, C in ((48, 32), (48, 64), (32, 32), (32, 48), (64, 16)):
        for N, H, W in PLANES:
            name = f"lcnn_bwd.Cin{Cin}.K{2 * C}.{N}x{H}x{W}"
            gen = case(name, "dense input gradient (prepare mode 1) and compact backward (mode 2), ADVSTEP_WINO_HALVES unset and 0")
            w, gscale = rnd(gen, 2 * C, Cin, 3, 3, scale=0.1), (torch.rand(C, generator=gen) + 0.5).to(dev)
            gout = rnd(gen, N, 2 * C, H, W)
            gy, idx = rnd(gen, N, C, H // 2, W // 2), codes(gen, 8, N, C, H // 2, W // 2)
            for tag, gs in (("scaled", gscale), ("plain", None)):
                U1, U2 = prepared(w, gs, Cin, 2 * C, 1), prepared(w, gs, Cin, 2 * C, 2)
                keep(f"{name}.prepare_mode1.{tag}", U1)
                keep(f"{name}.prepare_mode2.{tag}", U2)
            gx = out_f32(N, Cin, H, W)
            ok(lib.advstep_conv3x3_backward_data_f32(ptr(gout), ptr(U1), ptr(gx), N, Cin, 2 * C, H, W, st), name)
            keep(f"{name}.backward_data", gx)
            for halves in (None, "0"):
                if halves is None:
                    os.environ.pop("ADVSTEP_WINO_HALVES", None)
                else:
                    os.environ["ADVSTEP_WINO_HALVES"] = halves
                gx = out_f32(N, Cin, H, W)
                ok(lib.advstep_conv3x3_mfm_pool2_backward_f32(ptr(gy), ptr(idx), ptr(U2), ptr(gx), N, Cin, C, H, W, st), name)
                keep(f"{name}.pool2_backward.halves_{halves or 'default'}", gx)
            os.environ.pop("ADVSTEP_WINO_HALVES", None)

    # ---- the detectors' residual blocks: plain convolutions over K1 (3x3) + K2 (1x1) channels ---------------------------------
    def res_prepared(w3, w1, rscale, kscale, rows, K1, K2, transpose):
        U = out_f32(lib.advstep_resconv_prepared_floats(K1, K2, rows))
        ok(lib.advstep_resconv_prepare_f32(ptr(w3), ptr(w1), ptr(rscale), ptr(kscale), ptr(U), rows, K1, K2, transpose, st),
           "resconv_prepare")
        return U

    # (K1, K2, rows): 20-channel layers (5 k-steps), K1 + K2 on each side of 64, K2 in {0, 1, 2, 4}; rows = 48 has a half-empty
    # last slice (one-tile launch), 20 and 64 have not
    for K1, K2, rows in ((20, 0, 20), (20, 2, 48), (8, 1, 20), (60, 4, 64), (64, 20, 48), (80, 0, 20), (64, 4, 64)):
        for N, H, W in PLANES:
            name = f"resconv.K{K1}+{K2}.rows{rows}.{N}x{H}x{W}"
            gen = case(name, "forward with and without sign bytes, pooled forward; prepare with and without row / channel scales")
            x1, x2 = rnd(gen, N, K1, H, W), rnd(gen, N, K2, H, W) if K2 else None
            w3, w1 = rnd(gen, rows, K1, 3, 3, scale=0.1), rnd(gen, rows, K2, scale=0.1) if K2 else None
            shift, rscale, kscale = rnd(gen, rows), rnd(gen, rows), rnd(gen, K1)
            U = res_prepared(w3, w1, None, None, rows, K1, K2, 0)
            keep(f"{name}.prepare", U, res_prepared(w3, w1, rscale, kscale, rows, K1, K2, 0))
            y, act = out_f32(N, rows, H, W), out_u8(N, rows, (H + 1) // 2, (W + 1) // 2)
            ok(lib.advstep_resconv_forward_act_f32(ptr(x1), ptr(x2), ptr(U), ptr(shift), 0.3, ptr(y), ptr(act), N, K1, K2, rows, H, W,
                                                   st), name)
            keep(f"{name}.forward_act", y, act)
            y = out_f32(N, rows, H, W)
            ok(lib.advstep_resconv_forward_f32(ptr(x1), ptr(x2), ptr(U), None, 1.0, ptr(y), N, K1, K2, rows, H, W, st), name)
            keep(f"{name}.forward", y)
            y, sel = out_f32(N, rows, H // 2, W // 2), out_u8(N, rows, H // 2, W // 2)
            ok(lib.advstep_resconv_pool2_forward_f32(ptr(x1), ptr(x2), ptr(U), ptr(shift), ptr(y), ptr(sel), N, K1, K2, rows, H, W,
                                                     st), name)
            keep(f"{name}.pool2_forward", y, sel)

    for K1, few, rows in ((20, 2, 20), (20, 1, 48), (80, 2, 20), (72, 1, 64)):
        for N, H, W in PLANES:
            name = f"resconv_few.K{K1}.few{few}.rows{rows}.{N}x{H}x{W}"
            gen = case(name, "pooled forward with the few-channel 1x1 convolution in the epilogue")
            x1, x2 = rnd(gen, N, K1, H, W), rnd(gen, N, few, H, W)
            U = res_prepared(rnd(gen, rows, K1, 3, 3, scale=0.1), None, None, None, rows, K1, 0, 0)
            wd, bias = rnd(gen, rows, few, scale=0.1), rnd(gen, rows)
            y, sel = out_f32(N, rows, H // 2, W // 2), out_u8(N, rows, H // 2, W // 2)
            ok(lib.advstep_resconv_pool2_forward_few_f32(ptr(x1), ptr(x2), ptr(U), ptr(wd), ptr(bias), ptr(y), ptr(sel), N, K1, few, rows,
                                                         H, W, st), name)
            keep(f"{name}.pool2_forward_few", y, sel)

    for K, rows in ((20, 20), (20, 48), (64, 64), (80, 48), (80, 20)):
        for N, H, W in PLANES:
            name = f"pooled_grad.K{K}.rows{rows}.{N}x{H}x{W}"
            gen = case(name, "input gradient from a pooled gradient + selection bytes: plain, times lrelu' from h, from sign bytes")
            w3, w1 = rnd(gen, K, rows, 3, 3, scale=0.1), None
            U = res_prepared(w3, w1, None, None, rows, K, 0, 1)
            keep(f"{name}.prepare_transposed", U, res_prepared(w3, w1, rnd(gen, rows), rnd(gen, K), rows, K, 0, 1))
            gy, sel = rnd(gen, N, K, H // 2, W // 2), codes(gen, 4, N, K, H // 2, W // 2)
            h, act = rnd(gen, N, rows, H, W), codes(gen, 16, N, rows, (H + 1) // 2, (W + 1) // 2)
            for tag, hh, slope in (("plain", None, 1.0), ("from_h", h, 0.3)):
                g = out_f32(N, rows, H, W)
                ok(lib.advstep_resconv_pooled_grad_f32(ptr(gy), ptr(sel), ptr(U), ptr(hh), slope, ptr(g), N, K, rows, H, W, st), name)
                keep(f"{name}.pooled_grad.{tag}", g)
            g = out_f32(N, rows, H, W)
            ok(lib.advstep_resconv_pooled_grad_act_f32(ptr(gy), ptr(sel), ptr(U), ptr(act), 0.3, ptr(g), N, K, rows, H, W, st), name)
            keep(f"{name}.pooled_grad_act", g)

    # the transposed preparation with a 1x1 part (the input gradient of conv2 + downsample)
    gen = case("resconv_prepare_transposed.K64+20.rows20", "prepare, transpose = 1, with w1")
    keep("resconv_prepare_transposed.K64+20.rows20", res_prepared(rnd(gen, 64, 20, 3, 3, scale=0.1), rnd(gen, 20, 20, scale=0.1), None,
                                                                  None, 20, 64, 20, 1))

    torch.cuda.synchronize()
    np.savez(out_path, **res)
    for name, what in CASES:
        print(f"case {name:44s} {what}")
    print(f"{len(res)} arrays -> {out_path}")
    return 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1]))
