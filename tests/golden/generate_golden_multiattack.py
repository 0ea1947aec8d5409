#!/usr/bin/env python
"""Generate tests/golden/multiattack.npz from the REFERENCE'S UNMODIFIED MultiAttack
(adversarial_attacks/torchattacks/attacks/multiattack.py) over the reference's MIFGSM / NIFGSM.

Run ONLY where the Python reference is available (see generate_golden.py), as generate_golden_apgd.py is run:

    python tests/golden/generate_golden_multiattack.py            # tests/golden/multiattack.npz
    python tests/golden/generate_golden_multiattack.py --out DIR  # the same recipe into DIR (nothing under tests/ is touched)

How the reference is run
  * the set-up of generate_golden_apgd.py: (B, 1, 1, T) "images", the TwoLogit wrapper over the surrogate detector — with two
    logits the reference's `torch.max(outputs, 1)` routing is well defined — B = 6, T = 403, single-threaded, the same model
    and batch (rows 0 and 3 start misclassified: they count as successes of the first member);
  * the members alternate MIFGSM / NIFGSM at 5 steps, alpha = eps / 5, decay 1, one member per radius of the case;
  * case 1: radii (0.001, 0.003, 0.01): records [6, 4, 3, 1], row 4 is never flipped and comes back bit-equal to its input;
    case 2: radii (0.0002, 0.001, 0.004, 0.02): records [6, 4, 4, 2, 0] — a stage without any success, and the loop ends on
    its break;  both asserted here;
  * per case the final batch, the records of the call (what `_update_multi_atk_records` received) and the `sr` list of
    `save(loader, return_verbose=True)` over a loader of two such batches.
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))

from tests.golden.generate_golden import _import_reference, npy  # noqa: E402
from tests.golden.generate_golden_apgd import B, T, TwoLogit, model_and_batch  # noqa: E402

STEPS = 5
CASES = {"case1": ((0.001, 0.003, 0.01), [6, 4, 3, 1]),
         "case2": ((0.0002, 0.001, 0.004, 0.02), [6, 4, 4, 2, 0])}
UNFLIPPED = {"case1": [4], "case2": []}


def main(out_dir=None):
    _import_reference()
    from adversarial_attacks.torchattacks.attacks.mifgsm import MIFGSM
    from adversarial_attacks.torchattacks.attacks.multiattack import MultiAttack
    from adversarial_attacks.torchattacks.attacks.nifgsm import NIFGSM
    torch.set_num_threads(1)
    body, x, y = model_and_batch()
    model = TwoLogit(body).eval()
    x4 = x.reshape(B, 1, 1, T)
    out = {"x": npy(x), "y": npy(y), "steps": np.int64(STEPS)}
    out.update({f"model_{k}": npy(v) for k, v in body.state_dict().items()})

    for case, (radii, want_records) in CASES.items():
        members = [(MIFGSM, NIFGSM)[i % 2](model, eps=eps, alpha=eps / STEPS, steps=STEPS, decay=1.0)
                   for i, eps in enumerate(radii)]
        atk = MultiAttack(members)
        seen = []
        update = atk._update_multi_atk_records
        atk._update_multi_atk_records = lambda records: (seen.append(list(records)), update(records))[1]
        # the records of one call reach _update_multi_atk_records only while a save() accumulates them
        rob_acc, sr, l2, _ = atk.save([(x4, y), (x4, y)], verbose=False, return_verbose=True)
        assert seen == [want_records, want_records], (case, seen)
        adv = npy(atk(x4, y)).reshape(B, T)
        same = [b for b in range(B) if np.array_equal(adv[b], npy(x)[b])]
        assert same == UNFLIPPED[case], (case, same)
        out[f"{case}_eps"] = np.asarray(radii, np.float64)
        out[f"{case}_adv"] = adv
        out[f"{case}_records"] = np.asarray(want_records, np.int64)
        out[f"{case}_sr"] = np.asarray(sr, np.float64)

    dst = Path(out_dir) if out_dir else HERE
    dst.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(dst / "multiattack.npz", **out)
    print(f"{dst / 'multiattack.npz'}: {(dst / 'multiattack.npz').stat().st_size / 1e6:.2f} MB")


if __name__ == "__main__":
    if sys.argv[1:2] == ["--out"]:
        main(sys.argv[2])
    else:
        main()
