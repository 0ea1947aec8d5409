#!/usr/bin/env python
"""Generate tests/golden/apgd.npz from the REFERENCE'S UNMODIFIED APGD (adversarial_attacks/torchattacks/attacks/apgd.py).

Run ONLY in the build container, where the Python reference is mounted read-only at /root/reference:

    python tests/golden/generate_golden_apgd.py            # tests/golden/apgd.npz
    python tests/golden/generate_golden_apgd.py --out DIR  # the same recipe into DIR (nothing under tests/ is touched)
    ATEN_CPU_CAPABILITY=avx2 DNNL_MAX_CPU_ISA=AVX2 MKL_ENABLE_INSTRUCTIONS=AVX2 python tests/golden/generate_golden_apgd.py --out DIR
    python tests/golden/generate_golden_apgd.py --isa-overlay DIR avx2       # tests/golden/apgd_avx2.npz (see generate_golden.py)

How the reference is run
  * inputs are (B, 1, 1, T) "images" (the reference's attack_single_run keeps a 4-D input as it is); the attacked model is a
    wrapper that reshapes them to (B, T), runs the surrogate detector of tests/helpers.py (weights stored in the fixture) and
    returns the two-logit adapter cat([-z, z], 1) — the reference's own APGD would otherwise see one logit;
  * the random starts are what the reference draws: every torch.rand / torch.randn call made while `perturb` runs is
    recorded (one per restart that runs, shaped like the rows still classified correctly), with the rows it was drawn
    for; the fixture stores them scattered into full-batch (n_restarts, B, T) arrays (zeros in rows a restart skips);
  * some rows start misclassified (their label is flipped), the surrogate's bias puts the logits near the boundary so
    that the attack fools some rows in the first restart and not others, and the second restart runs on the rest.
"""
from __future__ import annotations

import contextlib
import sys
from pathlib import Path

import numpy as np
import torch

REF = Path("/root/reference")
HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))

from tests.golden.generate_golden import Surrogate, npy, write_isa_overlay  # noqa: E402  (the same surrogate detector)

B, T = 6, 403
CASES = [(norm, steps) for norm in ("Linf", "L2") for steps in (1, 4, 10, 25)]
EPS = {"Linf": 0.005, "L2": 0.1}


class TwoLogit(torch.nn.Module):
    """(B, 1, 1, T) -> cat([-z, z], 1) with z = surrogate((B, T))."""

    def __init__(self, body):
        super().__init__()
        self.body = body

    def forward(self, x):
        z = self.body(x.reshape(x.shape[0], -1))
        return torch.cat([-z, z], 1)


def model_and_batch():
    torch.manual_seed(1234)
    body = Surrogate().eval()
    x = torch.rand(B, T, generator=torch.Generator().manual_seed(77)) * 0.5 + 0.25
    with torch.no_grad():
        body.fc.bias -= body(x).mean() / 4.0                    # logits near the decision boundary
        y = (body(x).reshape(-1) > 0).to(torch.int64)
    y[0] = 1 - y[0]                                              # rows 0 and 3 start misclassified
    y[3] = 1 - y[3]
    return body, x, y


@contextlib.contextmanager
def recorded_draws():
    draws = []
    rand, randn = torch.rand, torch.randn

    def rec(fn):
        def wrapped(*a, **kw):
            t = fn(*a, **kw)
            draws.append(t.detach().clone())
            return t
        return wrapped

    torch.rand, torch.randn = rec(rand), rec(randn)
    try:
        yield draws
    finally:
        torch.rand, torch.randn = rand, randn


def run_case(APGD, body, x, y, norm, steps, n_restarts=2, seed=0):
    eot_iter = 2 if steps == 4 else 1
    model = TwoLogit(body).eval()
    atk = APGD(model, norm=norm, eps=EPS[norm], steps=steps, n_restarts=n_restarts, seed=seed, loss="ce", eot_iter=eot_iter)
    runs = []
    single = atk.attack_single_run

    def recording_single_run(x_in, y_in):
        res = single(x_in, y_in)
        runs.append(res[1].detach().clone())                     # acc of the restart
        return res

    atk.attack_single_run = recording_single_run
    x4 = x.reshape(B, 1, 1, T)
    with torch.no_grad():
        acc = model(x4).max(1)[1] == y
    with recorded_draws() as draws:
        adv = atk(x4, y)
    full = np.zeros((n_restarts, B, T), np.float32)
    assert len(draws) == len(runs) <= n_restarts
    rows = acc.nonzero().reshape(-1)
    for r, (d, acc_curr) in enumerate(zip(draws, runs)):
        assert d.shape == (rows.numel(), 1, 1, T)
        full[r, rows.numpy()] = npy(d).reshape(rows.numel(), T)
        rows = rows[acc_curr != 0]
    return {"adv": npy(adv).reshape(B, T), "draws": full, "eps": np.float64(EPS[norm]), "steps": np.int64(steps),
            "eot_iter": np.int64(eot_iter), "n_restarts": np.int64(n_restarts), "seed": np.int64(seed),
            "restarts_run": np.int64(len(draws)), "start_acc": npy(acc).astype(np.uint8)}


def main(out_dir=None):
    if not REF.exists():
        sys.exit("the reference is not mounted at /root/reference; fixtures can only be generated in the build container")
    sys.path.insert(0, str(REF))
    from adversarial_attacks.torchattacks.attacks.apgd import APGD
    torch.set_num_threads(1)
    body, x, y = model_and_batch()
    out = {"x": npy(x), "y": npy(y)}
    out.update({f"model_{k}": npy(v) for k, v in body.state_dict().items()})
    for norm, steps in CASES:
        for k, v in run_case(APGD, body, x, y, norm, steps).items():
            out[f"{norm}_{steps}_{k}"] = v
    dst = Path(out_dir) if out_dir else HERE
    dst.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(dst / "apgd.npz", **out)
    print(f"{dst / 'apgd.npz'}: {(dst / 'apgd.npz').stat().st_size / 1e6:.2f} MB")


if __name__ == "__main__":
    if sys.argv[1:2] == ["--isa-overlay"]:
        import tests.golden.generate_golden as G
        G.ISA_OVERLAY_FIXTURES = ("apgd",)
        write_isa_overlay(sys.argv[2], sys.argv[3])
    elif sys.argv[1:2] == ["--out"]:
        main(sys.argv[2])
    else:
        main()
