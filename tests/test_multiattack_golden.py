"""CPU: torchattacks.MultiAttack on the CPU table (tests/multiattack_cpu_ops.py) against tests/golden/multiattack.npz, which the
REFERENCE'S UNMODIFIED MultiAttack produced over the reference's MIFGSM / NIFGSM on a two-logit model
(tests/golden/generate_golden_multiattack.py): the final batches, the records of a call and the success rates of `save`."""
import os
import sys

import numpy as np
import pytest
import torch

from tests import multiattack_cpu_ops as C
from tests.helpers import GOLDEN, golden_for_this_cpu, surrogate_from

T = torch.from_numpy
CASES = {"case1": [6, 4, 3, 1], "case2": [6, 4, 4, 2, 0]}


@pytest.fixture(autouse=True)
def one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)  # the fixture was generated single-threaded
    yield
    torch.set_num_threads(n)


def multi_attack(g, case, ops, extra=()):
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    model, steps = surrogate_from(g), int(g["steps"])
    members = [(torchattacks.MIFGSM, torchattacks.NIFGSM)[i % 2](model, eps=float(eps), alpha=float(eps) / steps, steps=steps,
                                                                   decay=1.0)
               for i, eps in enumerate(g[f"{case}_eps"])] + [cls(model) for cls in extra]
    atk = torchattacks.MultiAttack(members)
    for a in members + [atk]:
        a.ops = ops
    return atk


def recorded(atk):
    """What each call hands to _update_multi_atk_records (only while records are accumulated, as in the reference)."""
    seen, update = [], atk._update_multi_atk_records
    atk._update_multi_atk_records = lambda records: (seen.append(list(records)), update(records))[1]
    return seen


@pytest.mark.parametrize("case", CASES)
def test_final_batch_and_records_bit_identical_to_reference(golden, case):
    g = golden_for_this_cpu(golden, "multiattack")
    assert g[f"{case}_records"].tolist() == CASES[case]
    atk = multi_attack(g, case, C.ReferenceLoss())
    seen = recorded(atk)
    atk._start_multi_atk_records()
    x, y = T(g["x"]), T(g["y"])
    adv = atk(x, y)
    assert seen == [CASES[case]]
    assert torch.equal(adv, T(g[f"{case}_adv"]))
    assert adv.data_ptr() != x.data_ptr() and torch.equal(x, T(g["x"]))           # the caller's batch is not written


def test_unflipped_row_is_the_input_and_early_successes_belong_to_the_first_member(golden):
    """Case 1 leaves row 4 standing: it comes back as the original samples, not as the last adversarial attempt.  Rows 0
    and 3 are misclassified before any attack: they carry the first member's output (they moved)."""
    g = golden_for_this_cpu(golden, "multiattack")
    x, want = T(g["x"]), T(g["case1_adv"])
    assert [b for b in range(x.shape[0]) if torch.equal(want[b], x[b])] == [4]
    eps0 = float(g["case1_eps"][0])
    for b in (0, 3):
        d = (want[b] - x[b]).abs().max().item()
        assert 0 < d <= eps0 + 2.0 ** -23                                           # one float32 ulp of a sample below 1


def test_loop_breaks_when_nothing_is_left(golden):
    """Case 2 ends with no survivor after its fourth member: a fifth is never called."""
    from audio_deepfake_adversarial_attacks_amd import torchattacks

    class NeverCalled(torchattacks.Attack):
        def __init__(self, model):
            super().__init__("NeverCalled", model)

        def forward(self, images, labels):
            raise AssertionError("called with nothing left to attack")

    g = golden_for_this_cpu(golden, "multiattack")
    atk = multi_attack(g, "case2", C.ReferenceLoss(), extra=(NeverCalled,))
    assert torch.equal(atk(T(g["x"]), T(g["y"])), T(g["case2_adv"]))


@pytest.mark.parametrize("case", CASES)
def test_save_success_rates_as_reference(golden, case, capsys):
    g = golden_for_this_cpu(golden, "multiattack")
    atk = multi_attack(g, case, C.ReferenceLoss())
    atk.verbose = True
    batch = (T(g["x"]), T(g["y"]))
    rob_acc, sr, l2, elapsed = atk.save([batch, batch], verbose=False, return_verbose=True)
    assert sr == g[f"{case}_sr"].tolist()
    n = CASES[case]
    assert sr == [(1 - 2 * n[i] / (2 * n[0])) * 100 for i in range(1, len(n))]
    assert capsys.readouterr().out == ""                                            # save() silences the per-call line ...
    assert atk.verbose is True and atk._multi_atk_records == [0.0] and atk._accumulate_multi_atk_records is False
    atk(*batch)
    assert capsys.readouterr().out == atk._return_sr_record(n) + "\n"               # ... and restores it
    assert atk._multi_atk_records == [0.0]                                          # nothing accumulates outside save()


def test_shipped_closed_form_loss_gives_the_same_records(golden):
    """The shipped loss (closed form) may differ from autograd's dz in the last bit (tests/test_momentum_golden.py); the
    routing is the same."""
    g = golden_for_this_cpu(golden, "multiattack")
    for case, want in CASES.items():
        atk = multi_attack(g, case, C)
        seen = recorded(atk)
        atk._start_multi_atk_records()
        atk(T(g["x"]), T(g["y"]))
        assert seen == [want]


def test_recipe_reproduces_the_committed_fixture(tmp_path):
    """tests/golden/generate_golden_multiattack.py rebuilds multiattack.npz byte for byte into a scratch directory (nothing
    under tests/ is touched).  Needs the reference's sources, which are not part of this repository."""
    sys.path.insert(0, str(GOLDEN))
    try:
        import generate_golden_multiattack as gen
    finally:
        sys.path.pop(0)
    from tests.golden.generate_golden import REF
    if not os.path.isdir(REF) or not os.access(REF, os.R_OK | os.X_OK):       # (os.path: an unreadable parent is "absent" too)
        pytest.skip("the reference's sources are not available here")
    before = list(sys.path)
    try:
        gen.main(tmp_path)
    finally:
        sys.path[:] = before
    new, old = np.load(tmp_path / "multiattack.npz"), np.load(GOLDEN / "multiattack.npz")
    assert set(new.files) == set(old.files)
    for k in old.files:
        assert new[k].shape == old[k].shape and new[k].dtype == old[k].dtype, k
        assert new[k].tobytes() == old[k].tobytes(), f"multiattack.npz:{k} differs from the committed fixture"
