#!/usr/bin/env python
"""Generate tests/golden/eotpgd.npz from the REFERENCE'S UNMODIFIED EOTPGD (adversarial_attacks/torchattacks/attacks/eotpgd.py).

Run ONLY where the Python reference is available (see generate_golden.py), as generate_golden_momentum.py is run:

    python tests/golden/generate_golden_eot.py            # tests/golden/eotpgd.npz
    python tests/golden/generate_golden_eot.py --out DIR  # the same recipe into DIR (nothing under tests/ is touched)
    python tests/golden/generate_golden_eot.py --isa-overlay DIR avx2   # tests/golden/eotpgd_avx2.npz, written only if an array differs

How the reference is run
  * the set-up of generate_golden_apgd.py / generate_golden_momentum.py: (B, 1, 1, T) "images", the TwoLogit wrapper over the
    surrogate detector, B = 6, T = 403, single-threaded, the same model and batch (rows 0 and 3 start misclassified);
  * eps 0.005, alpha 0.001, 5 steps, eot_iter 1 and 3, default mode and targeted at 1 - y (set_mode_targeted_by_function);
  * the random start is what the reference draws: the one Tensor.uniform_ call made while the attack runs is recorded
    (generate_golden_momentum.recorded_uniform) and stored beside the result as `<case>_noise` (B, T);
  * str(atk) of the class built with its defaults on the bare surrogate.
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))

from tests.golden.generate_golden import Surrogate, _import_reference, npy, write_isa_overlay  # noqa: E402
from tests.golden.generate_golden_apgd import B, T, TwoLogit, model_and_batch  # noqa: E402
from tests.golden.generate_golden_momentum import recorded_uniform  # noqa: E402

EPS, ALPHA, STEPS = 0.005, 0.001, 5
EOT_ITERS = (1, 3)


def main(out_dir=None):
    _import_reference()
    from adversarial_attacks.torchattacks.attacks.eotpgd import EOTPGD
    torch.set_num_threads(1)
    body, x, y = model_and_batch()
    model = TwoLogit(body).eval()
    x4 = x.reshape(B, 1, 1, T)
    out = {"x": npy(x), "y": npy(y), "eps": np.float64(EPS), "alpha": np.float64(ALPHA), "steps": np.int64(STEPS)}
    out.update({f"model_{k}": npy(v) for k, v in body.state_dict().items()})
    for mode in ("default", "targeted"):
        for k in EOT_ITERS:
            torch.manual_seed(100 + k)
            atk = EOTPGD(model, eps=EPS, alpha=ALPHA, steps=STEPS, eot_iter=k, random_start=True)
            if mode == "targeted":
                atk.set_mode_targeted_by_function(lambda images, labels: 1 - labels)
            with recorded_uniform() as draws:
                adv = atk(x4, y)
            assert len(draws) == 1 and draws[0].shape == x4.shape
            out[f"{mode}_{k}_adv"] = npy(adv).reshape(B, T)
            out[f"{mode}_{k}_noise"] = npy(draws[0]).reshape(B, T)
    out["str_EOTPGD"] = np.array(str(EOTPGD(Surrogate())))

    dst = Path(out_dir) if out_dir else HERE
    dst.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(dst / "eotpgd.npz", **out)
    print(f"{dst / 'eotpgd.npz'}: {(dst / 'eotpgd.npz').stat().st_size / 1e6:.2f} MB")


if __name__ == "__main__":
    if sys.argv[1:2] == ["--isa-overlay"]:
        import tests.golden.generate_golden as G
        G.ISA_OVERLAY_FIXTURES = ("eotpgd",)
        write_isa_overlay(sys.argv[2], sys.argv[3])
    elif sys.argv[1:2] == ["--out"]:
        main(sys.argv[2])
    else:
        main()
