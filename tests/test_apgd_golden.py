"""CPU: the APGD attack (torchattacks.APGD on the CPU table tests/apgd_cpu_ops.py) against tests/golden/apgd.npz, which the
REFERENCE'S UNMODIFIED APGD produced (tests/golden/generate_golden_apgd.py): Linf and L2, 1 / 4 / 10 / 25 steps, two
restarts (the second runs on the rows the first did not fool), eot_iter = 2 at 4 steps, two rows misclassified at the start.

The reference's random draws are installed per restart (set_init_noise with one (B, T) draw per restart)."""
import pytest
import torch

from tests import apgd_cpu_ops as C
from tests.helpers import golden_for_this_cpu, surrogate_from

T = torch.from_numpy
CASES = [(norm, steps) for norm in ("Linf", "L2") for steps in (1, 4, 10, 25)]


@pytest.fixture(autouse=True)
def one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)  # the fixture was generated single-threaded
    yield
    torch.set_num_threads(n)


def attack(g, norm, steps, ops):
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    p = f"{norm}_{steps}_"
    atk = torchattacks.APGD(surrogate_from(g), norm=norm, eps=float(g[p + "eps"]), steps=steps,
                            n_restarts=int(g[p + "n_restarts"]), seed=int(g[p + "seed"]), eot_iter=int(g[p + "eot_iter"]))
    atk.ops = ops
    atk.set_init_noise([T(d) for d in g[p + "draws"]])
    return atk(T(g["x"]), T(g["y"]))


@pytest.mark.parametrize("norm,steps", CASES)
def test_apgd_bit_identical_to_reference_with_the_reference_loss(golden, norm, steps):
    """Every step, checkpoint, restart and tracking decision as the reference computes it: with the reference's loss
    arithmetic (autograd through CrossEntropyLoss) in the eval op, the output is the reference's, bit for bit."""
    g = golden_for_this_cpu(golden, "apgd")
    assert int(g[f"{norm}_{steps}_restarts_run"]) == 2
    adv = attack(g, norm, steps, C.ReferenceLoss())
    assert torch.equal(adv, T(g[f"{norm}_{steps}_adv"]))


@pytest.mark.parametrize("steps", [1, 4, 10, 25])
def test_apgd_linf_bit_identical_to_reference(golden, steps):
    """The shipped loss (closed form, as the kernels compute it) changes dz in the last bit for some logits; L-inf uses
    only sign(grad), and its output is the reference's bit for bit."""
    g = golden_for_this_cpu(golden, "apgd")
    assert torch.equal(attack(g, "Linf", steps, C), T(g[f"Linf_{steps}_adv"]))


@pytest.mark.parametrize("steps", [1, 4, 10, 25])
def test_apgd_l2_with_the_closed_form_loss(golden, steps):
    """L2 with the shipped closed-form loss: dz differs from autograd's in the last bit for about half the logits, the
    L2 step passes that on through g / ||g||, and an ulp-level difference in a loss can flip a strict comparison
    (improved, oscillation count) and send a row down another trajectory: no per-sample bound tighter than the eps-ball
    holds after many steps.  What does hold: the same rows are fooled, and each output row is in the
    ball around x and in [0, 1]."""
    g = golden_for_this_cpu(golden, "apgd")
    x, want = T(g["x"]), T(g[f"L2_{steps}_adv"])
    adv = attack(g, "L2", steps, C)
    assert torch.equal((adv != x).any(dim=1), (want != x).any(dim=1))
    # x + d rounds to float32 sample by sample: with |d| ~ eps / sqrt(T) that is ~1e-5 of the norm here (the reference too)
    bound = float(g[f"L2_{steps}_eps"]) * (1 + 1e-5)
    assert ((adv - x).double().norm(dim=1) <= bound).all() and ((want - x).double().norm(dim=1) <= bound).all()
    assert adv.min() >= 0 and adv.max() <= 1
    if steps == 1:                                      # one step: the difference is still at the rounding level
        assert (adv - want).abs().max() <= 2.4e-7
