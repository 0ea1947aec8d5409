#!/usr/bin/env python
"""Launches the row kernels of the attack steps 30 times each at B = 128, T = 64 600, for a kernel trace:

    rocprofv3 --kernel-trace --stats --output-format csv -- python tools/attack_kernel_trace_probe.py
"""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from audio_deepfake_adversarial_attacks_amd import hip_ops as ops

d = torch.device("cuda:0")
B, T = 128, 64600
g = torch.Generator().manual_seed(1)
x = torch.rand(B, T, generator=g).to(d)
adv = (x + (torch.rand(B, T, generator=g).to(d) - 0.5) * 0.01).clamp(0, 1)
grad = (torch.randn(B, T, generator=g) * 1e-3).to(d)
prev = (x + (torch.rand(B, T, generator=g).to(d) - 0.5) * 0.01).clamp(0, 1)
w = (torch.randn(B, T, generator=g) * 2).to(d)
step = torch.full((B,), 0.2, device=d)
mom = torch.zeros(B, T, device=d)
out = torch.empty_like(x)
N = 30
for it in range(N):
    ops.to_minmax(grad)
    os.environ["ADVSTEP_L2_SINGLE_PASS"] = "0"
    ops.pgd_l2_step(adv, grad, x, 0.2, 0.1, out=out)
    os.environ["ADVSTEP_L2_SINGLE_PASS"] = "1"
    ops.pgd_l2_step(adv, grad, x, 0.2, 0.1, out=out)
    ops.pgd_linf_step(adv, grad, x, 2 / 255, 0.003, out=out)
    ops.cw_tanh_sqdist(w, x)
    ops.apgd_l2_step(adv, prev, grad, x, step, 0.1, 0.75, out=out)
    ops.mi_step(adv, grad, x, mom, 2 / 255, 0.003, 1.0, out=out)
torch.cuda.synchronize()
print("probe ok", N)
