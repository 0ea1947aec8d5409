#!/usr/bin/env python
"""Generate tests/golden/momentum.npz from the REFERENCE'S UNMODIFIED MIFGSM, NIFGSM, VMIFGSM and VNIFGSM
(adversarial_attacks/torchattacks/attacks/{mifgsm,nifgsm,vmifgsm,vnifgsm}.py).

Run ONLY where the Python reference is available (see generate_golden.py), as generate_golden_apgd.py is run:

    python tests/golden/generate_golden_momentum.py            # tests/golden/momentum.npz
    python tests/golden/generate_golden_momentum.py --out DIR  # the same recipe into DIR (nothing under tests/ is touched)
    ATEN_CPU_CAPABILITY=avx2 DNNL_MAX_CPU_ISA=AVX2 MKL_ENABLE_INSTRUCTIONS=AVX2 python tests/golden/generate_golden_momentum.py --out DIR
    python tests/golden/generate_golden_momentum.py --isa-overlay DIR avx2  # tests/golden/momentum_avx2.npz, written only if an
                                                                            # array differs (none did when this was recorded)

How the reference is run
  * the set-up of generate_golden_apgd.py: (B, 1, 1, T) "images", the TwoLogit wrapper over the surrogate detector, B = 6,
    T = 403, single-threaded, the same model and batch (rows 0 and 3 start misclassified);
  * MI and NI at 1 / 5 / 10 / 25 steps with eps 0.005, alpha 0.001, decay 1.0; MI with decay 0.5; MI targeted at 1 - y
    (set_mode_targeted_by_function);
  * VMI and VNI at 3 steps, N = 4, beta 1.5: every Tensor.uniform_ call made while the attack runs is recorded, in order
    (one per neighbour), and stored as (steps, N, B, T);
  * MI through a wrapper that scales the logits: the scale is doubled until the loss gradient of at least one row is exactly
    zero at the first step (a saturated softmax), which pins the row whose momentum turns NaN and stays NaN;
  * str(atk) of each class built with its defaults on the bare surrogate.
"""
from __future__ import annotations

import contextlib
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))

from tests.golden.generate_golden import Surrogate, _import_reference, npy, write_isa_overlay  # noqa: E402
from tests.golden.generate_golden_apgd import B, T, TwoLogit, model_and_batch  # noqa: E402

EPS, ALPHA = 0.005, 0.001
STEPS = (1, 5, 10, 25)
VT = dict(steps=3, N=4, beta=1.5)


class ScaledTwoLogit(torch.nn.Module):
    """TwoLogit with the logit multiplied by `scale`."""

    def __init__(self, body, scale):
        super().__init__()
        self.body, self.scale = body, scale

    def forward(self, x):
        z = self.body(x.reshape(x.shape[0], -1)) * self.scale
        return torch.cat([-z, z], 1)


@contextlib.contextmanager
def recorded_uniform():
    draws = []
    uniform_ = torch.Tensor.uniform_

    def wrapped(self, *a, **kw):
        out = uniform_(self, *a, **kw)
        draws.append(out.detach().clone())
        return out

    torch.Tensor.uniform_ = wrapped
    try:
        yield draws
    finally:
        torch.Tensor.uniform_ = uniform_


def zero_gradient_scale(body, x4, y):
    """The first power of two at which the mean cross-entropy's gradient is exactly zero in at least one row of x."""
    scale = 1.0
    while True:
        xr = x4.clone().requires_grad_(True)
        cost = torch.nn.CrossEntropyLoss()(ScaledTwoLogit(body, scale)(xr), y)
        (g,) = torch.autograd.grad(cost, xr)
        zero = (g.reshape(B, -1) == 0).all(dim=1)
        if zero.any():
            return scale, zero
        scale *= 2.0
        assert scale < 2.0 ** 20


def main(out_dir=None):
    _import_reference()
    from adversarial_attacks.torchattacks.attacks.mifgsm import MIFGSM
    from adversarial_attacks.torchattacks.attacks.nifgsm import NIFGSM
    from adversarial_attacks.torchattacks.attacks.vmifgsm import VMIFGSM
    from adversarial_attacks.torchattacks.attacks.vnifgsm import VNIFGSM
    torch.set_num_threads(1)
    body, x, y = model_and_batch()
    model = TwoLogit(body).eval()
    x4 = x.reshape(B, 1, 1, T)
    out = {"x": npy(x), "y": npy(y), "eps": np.float64(EPS), "alpha": np.float64(ALPHA)}
    out.update({f"model_{k}": npy(v) for k, v in body.state_dict().items()})

    def run(atk):
        return npy(atk(x4, y)).reshape(B, T)

    for name, cls in (("MI", MIFGSM), ("NI", NIFGSM)):
        for steps in STEPS:
            out[f"{name}_{steps}_adv"] = run(cls(model, eps=EPS, alpha=ALPHA, steps=steps, decay=1.0))
    out["MI_decay05_adv"] = run(MIFGSM(model, eps=EPS, alpha=ALPHA, steps=10, decay=0.5))
    atk = MIFGSM(model, eps=EPS, alpha=ALPHA, steps=10, decay=1.0)
    atk.set_mode_targeted_by_function(lambda images, labels: 1 - labels)
    out["MI_targeted_adv"] = run(atk)

    for name, cls in (("VMI", VMIFGSM), ("VNI", VNIFGSM)):
        atk = cls(model, eps=EPS, alpha=ALPHA, steps=VT["steps"], decay=1.0, N=VT["N"], beta=VT["beta"])
        with recorded_uniform() as draws:
            out[f"{name}_adv"] = run(atk)
        assert len(draws) == VT["steps"] * VT["N"] and all(d.shape == x4.shape for d in draws)
        out[f"{name}_draws"] = np.stack([npy(d).reshape(B, T) for d in draws]).reshape(VT["steps"], VT["N"], B, T)
    out.update({f"VT_{k}": np.float64(v) for k, v in VT.items()})

    scale, zero = zero_gradient_scale(body, x4, y)
    out["MI_zero_scale"] = np.float64(scale)
    out["MI_zero_rows"] = npy(zero).astype(np.uint8)
    out["MI_zero_adv"] = run(MIFGSM(ScaledTwoLogit(body, scale).eval(), eps=EPS, alpha=ALPHA, steps=5, decay=1.0))

    bare = Surrogate()
    for cls in (MIFGSM, NIFGSM, VMIFGSM, VNIFGSM):
        out[f"str_{cls.__name__}"] = np.array(str(cls(bare)))

    dst = Path(out_dir) if out_dir else HERE
    dst.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(dst / "momentum.npz", **out)
    print(f"{dst / 'momentum.npz'}: {(dst / 'momentum.npz').stat().st_size / 1e6:.2f} MB")


if __name__ == "__main__":
    if sys.argv[1:2] == ["--isa-overlay"]:
        import tests.golden.generate_golden as G
        G.ISA_OVERLAY_FIXTURES = ("momentum",)
        write_isa_overlay(sys.argv[2], sys.argv[3])
    elif sys.argv[1:2] == ["--out"]:
        main(sys.argv[2])
    else:
        main()
