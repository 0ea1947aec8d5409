"""CPU: SmoothAdvPGD's host side — the numpy twin (tests/smoothadv_cpu_ops.py) against float64 autograd, smooth_noise's twin and
the PGD expressions; the attack on the analytic linear detector through the twin's op table; the registry, chunk formation,
noise offsets and validation; `--noise_sigma` and the trainer's noise seam; the certify-sigma hand-over of the loop."""
import logging
import random

import numpy as np
import pytest
import torch

from audio_deepfake_adversarial_attacks_amd import evaluation, torchattacks
from audio_deepfake_adversarial_attacks_amd import trainer as T
from audio_deepfake_adversarial_attacks_amd.aa.aa_types import AttackEnum
from tests import radius_cpu_ops as R
from tests import smooth_cpu_ops as S
from tests import smoothadv_cpu_ops as A
from tests.helpers import Surrogate, TinyDetectionSet


# ---- the twin ------------------------------------------------------------------------------------------------------------------------

def logits(m, B, seed):
    """(m, B) float32 logits: ordinary rows, then rows at |z| = 80, all-saturated on either side, mixed, and one near zero."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(m, B, generator=g) * 3.0
    y = torch.randint(0, 2, (B,), generator=g)
    if B >= 6:
        s = (2 * y - 1).float()
        z[:, 0] = -80.0 * s[0]                                                        # every slot saturated on the wrong side: w = 1 / m
        z[:, 1] = 80.0 * s[1]                                                         # every slot saturated on the right side
        z[:, 2] = torch.where(torch.arange(m) % 2 == 0, 80.0, -80.0)                  # mixed
        z[:, 3] = -80.0 * s[3]
        z[0, 3] = -79.0 * s[3]
        z[:, 4] = 1e-3
    return z, y


@pytest.mark.parametrize("m", [1, 2, 5, 8])
@pytest.mark.parametrize("scale", [1.0, -1.0])
def test_twin_loss_and_gradient_equal_float64_autograd(m, scale):
    z, y = logits(m, 9, 10 * m)
    dz, cost = A.loss_grad_np(z, y, scale, dtype=np.float64)
    zz = z.double().requires_grad_(True)
    s = (2 * y - 1).double()
    ref = -torch.log(torch.sigmoid(s * zz).mean(dim=0))
    (g,) = torch.autograd.grad(ref.sum(), zz)
    np.testing.assert_allclose(cost, ref.detach().numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(dz, scale * g.numpy(), rtol=1e-12, atol=1e-12)
    assert np.isfinite(dz).all() and np.isfinite(cost).all()
    np.testing.assert_allclose(np.abs(dz[:, 0]), (1.0 / m) * 1.0, rtol=1e-12)        # all-saturated: w = 1 / m, sigmoid(80) = 1
    assert cost[0] == pytest.approx(80.0, rel=1e-12)
    dz32, cost32 = A.loss_grad_np(z, y, scale, dtype=np.float32)                       # the float32 form: the same formula
    assert dz32.dtype == np.float32 and cost32.dtype == np.float32
    assert (np.abs(dz32 - dz) <= 1e-5 * np.abs(dz).max(axis=0, keepdims=True)).all()
    np.testing.assert_allclose(cost32, cost, rtol=1e-5, atol=1e-5)


def test_twin_nan_logit_poisons_only_its_row():
    z, y = logits(5, 9, 3)
    clean = A.loss_grad_np(z, y)
    z[2, 6] = float("nan")
    dz, cost = A.loss_grad_np(z, y)
    assert np.isnan(dz[:, 6]).all() and np.isnan(cost[6])
    keep = np.arange(9) != 6
    assert np.array_equal(dz[:, keep], clean[0][:, keep]) and np.array_equal(cost[keep], clean[1][keep])


def test_twin_fill_without_scale_is_smooth_noise():
    x = torch.rand(3, 37, generator=torch.Generator().manual_seed(1)) - 0.5
    for dtype in (np.float32, np.float64):
        np.testing.assert_array_equal(A.fill_np(x, 0.05, 9, offset=5, s0=2, ns=3, dtype=dtype),
                                      S.smooth_noise_np(x, 0.05, 9, offset=5, s0=2, ns=3, dtype=dtype))
    mn, mx = torch.tensor([-0.3, -1.0, 0.1]), torch.tensor([0.7, 2.0, 0.4])
    got = A.fill_np(x, 0.05, 9, offset=5, ns=2, scale=mx - mn, shift=mn)
    reverted = ((x * (mx - mn)[:, None]) + mn[:, None])                               # minmax_revert's expression, float32
    np.testing.assert_array_equal(got, S.smooth_noise_np(reverted, 0.05, 9, offset=5, ns=2))


@pytest.mark.parametrize("m", [1, 3])
def test_twin_step_is_the_slot_order_sum_then_pgd(m):
    g = torch.Generator().manual_seed(m)
    B, Tn = 4, 133
    x = torch.rand(B, Tn, generator=g)
    adv = (x + (torch.rand(B, Tn, generator=g) - 0.5) * 0.002).clamp(0, 1)   # inside the ball: ||adv - x|| <= 0.012
    grads = torch.randn(m, B, Tn, generator=g)
    grads[:, 2] = 0.0                                                                  # a row without a gradient
    total = grads[0].clone()
    for i in range(1, m):
        total = total + grads[i]
    eps, alpha = 0.05, 0.02
    out, gsum = A.smoothadv_step(adv, x, grads, alpha, eps, norm="L2", gsum=torch.empty_like(adv))
    assert torch.equal(gsum, total)
    want = R.row_pgd_l2_step(adv, total, x, torch.full((B,), eps), alpha, 0.0)
    assert torch.equal(out, want) and float((out[2] - adv[2]).abs().max()) <= 2.0 ** -23   # no gradient: the row stays
    out = A.smoothadv_step(adv, x, grads, alpha, eps, norm="Linf")
    assert torch.equal(out, R.row_pgd_linf_step(adv, total, x, torch.full((B,), eps), alpha, 0.0))
    with pytest.raises(ValueError, match="norm"):
        A.smoothadv_step(adv, x, grads, alpha, eps, norm="L1")


# ---- the attack on the analytic case ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T_,steps,alpha", [(1028, 4, None), (1030, 3, None), (1028, 2, 0.1 * 0.45 * S.LINEAR_SIGMA)],
                         ids=["whole_radius", "odd_length", "short_of_the_radius"])
def test_attack_on_the_linear_detector(T_, steps, alpha):
    model, x01, y, k, sigma = A.unit_box_linear_case(T_)
    eps = 0.45 * sigma
    atk = torchattacks.SmoothAdvPGD(model, eps=eps, alpha=alpha, steps=steps, sigma=sigma, samples=4, random_start=False)
    atk.ops = A
    torch.manual_seed(11)
    adv = atk(x01, y)
    assert adv.dtype == torch.float32 and adv.shape == x01.shape and float(adv.min()) > 0.2 and float(adv.max()) < 0.8
    A.check_linear_attack(adv, x01, model, y, k, sigma, eps, steps, atk.alpha)
    assert all(p.requires_grad for p in model.parameters())


def test_targeted_mode_moves_the_other_way():
    model, x01, y, k, sigma = A.unit_box_linear_case(1028)
    eps = 0.45 * sigma
    atk = torchattacks.SmoothAdvPGD(model, eps=eps, steps=2, sigma=sigma, samples=2, random_start=False)
    atk.ops = A
    atk.set_mode_targeted_by_function(lambda images, labels: 1 - labels)
    adv = atk(x01, y)
    A.check_linear_attack(adv, x01, model, y, k, sigma, eps, 2, atk.alpha)          # towards the target = away from the label
    atk.set_mode_targeted_by_function(lambda images, labels: labels)
    w = model.w.detach()
    along = (atk(x01, y).double() - x01.double()) @ (w / w.norm())
    assert bool((along * (2 * y - 1).double() > 0).all())                             # towards the label's own side


# ---- registry, properties, chunks, offsets, validation ------------------------------------------------------------------------------

def test_enum_members_and_exports():
    assert "SmoothAdvPGD" in torchattacks.__all__ and torchattacks.SmoothAdvPGD.__module__.endswith("attacks.smoothadv")
    assert len(set(torchattacks.__all__)) == len(torchattacks.__all__)
    for name, l2 in (("SMOOTHADV", "PGDL2"), ("SMOOTHADV_eps15", "PGDL2_eps15"), ("SMOOTHADV_eps20", "PGDL2_eps20")):
        method, params = AttackEnum[name].value
        assert method is torchattacks.SmoothAdvPGD
        assert params == {"eps": AttackEnum[l2].value[1]["eps"], "steps": 10, "sigma": 0.05, "samples": 8}
    assert len({e.name for e in AttackEnum}) == len(AttackEnum.__members__)
    atk = AttackEnum.SMOOTHADV.value[0](Surrogate(), **AttackEnum.SMOOTHADV.value[1])
    assert atk.alpha == pytest.approx(2 * 0.1 / 10) and atk.norm == "L2" and atk.random_start and not atk.fresh_noise
    assert atk.wants_minmax is True and atk.replays_from_graph is False and atk.max_rows == 1024
    assert str(atk) == ("SmoothAdvPGD(model_name=Surrogate, device=cpu, eps=0.1, alpha=0.02, steps=10, sigma=0.05, samples=8, "
                        "norm=L2, random_start=True, fresh_noise=False, max_rows=1024, attack_mode=default, return_type=float)")
    assert torchattacks.SmoothAdvPGD(Surrogate(), eps=0.3, alpha=0.01).alpha == 0.01


class SpyDetector(torch.nn.Module):
    """One logit per row, the sizes of the calls recorded."""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.tensor(0.5))
        self.sizes = []

    def forward(self, x):
        self.sizes.append(x.shape[0])
        return (x.mean(dim=1, keepdim=True) - 0.5) * self.w * 10.0


class RecordingTable:
    """The twin's table with every call of the named ops recorded as (name, kwargs and positionals of interest)."""

    def __init__(self, base=A):
        self.base, self.calls = base, []

    def __getattr__(self, name):
        fn = getattr(self.base, name)

        def call(*args, **kw):
            self.calls.append((name, args, kw))
            return fn(*args, **kw)
        return call


@pytest.mark.parametrize("B,m,max_rows", [(8, 5, 20), (8, 5, 3), (4, 5, 1024), (3, 2, 4)])
def test_chunks_are_formed_as_smoothing_votes_forms_them(B, m, max_rows):
    x = torch.rand(B, 64, generator=torch.Generator().manual_seed(B))
    y = torch.arange(B) % 2
    spy = SpyDetector()
    sm = torchattacks.Smoothing(0.05, n=m, n0=m, max_rows=max_rows)
    sm.ops = A
    sm.votes(spy, x, m, 0)
    want, spy.sizes = spy.sizes, []
    assert sum(want) == m * B and (max_rows >= m * B or len(want) > 1)
    atk = torchattacks.SmoothAdvPGD(spy, eps=0.01, steps=2, sigma=0.05, samples=m, random_start=False, max_rows=max_rows)
    atk.ops = A
    atk(x, y)
    assert spy.sizes == want + want                                                   # two steps, each the certifier's chunks


def test_fixed_and_fresh_noise_offsets_and_the_minmax_hand_over():
    x = torch.rand(3, 40, generator=torch.Generator().manual_seed(2))
    y = torch.tensor([0, 1, 1])
    for fresh, offsets in ((False, [0, 0, 0]), (True, [0, 4, 8])):
        table = RecordingTable()
        atk = torchattacks.SmoothAdvPGD(SpyDetector(), eps=0.01, steps=3, sigma=0.05, samples=4, random_start=False, fresh_noise=fresh)
        atk.ops = table
        torch.manual_seed(5)
        atk(x, y)
        fills = [c for c in table.calls if c[0] == "smoothadv_fill"]
        assert [c[1][3] for c in fills] == offsets and len({c[1][2] for c in fills}) == 1   # one key per call
        assert all(c[2]["ns"] == 4 and c[2]["s0"] == 0 and c[2]["scale"] is None and c[2]["shift"] is None for c in fills)
        assert [c[0] for c in table.calls].count("smoothadv_step") == 3
        first_key = fills[0][1][2]
        atk(x, y)
        assert [c for c in table.calls if c[0] == "smoothadv_fill"][-1][1][2] != first_key   # a new key at the next call
    mn, mx = torch.tensor([[-0.5], [-1.0], [0.0]]), torch.tensor([[0.5], [3.0], [0.25]])
    table = RecordingTable()
    atk = torchattacks.SmoothAdvPGD(SpyDetector(), eps=0.01, steps=1, sigma=0.05, samples=2, random_start=False)
    atk.ops = table
    atk.set_minmax(mn, mx)
    atk(x, y)
    (fill,) = [c for c in table.calls if c[0] == "smoothadv_fill"]
    assert torch.equal(fill[2]["scale"], (mx - mn).reshape(-1)) and torch.equal(fill[2]["shift"], mn.reshape(-1))
    atk(x, y)                                                                          # handed over for ONE call
    assert [c for c in table.calls if c[0] == "smoothadv_fill"][-1][2]["scale"] is None
    atk.set_minmax(mn[:2], mx[:2])
    with pytest.raises(ValueError, match="one value per utterance"):
        atk(x, y)


def test_random_start_draws_like_pgdl2_and_pgd():
    x = torch.rand(2, 32, generator=torch.Generator().manual_seed(4)) * 0.5 + 0.25
    y = torch.tensor([0, 1])
    for norm, init in (("L2", "pgd_l2_init"), ("Linf", "pgd_linf_init")):
        table = RecordingTable()
        atk = torchattacks.SmoothAdvPGD(SpyDetector(), eps=0.01, steps=1, sigma=0.05, samples=2, norm=norm)
        atk.ops = table
        torch.manual_seed(6)
        atk(x, y)
        names = [c[0] for c in table.calls]
        assert names[0] == init and names.count(init) == 1
        seeds = [table.calls[0][2]["seed"], [c for c in table.calls if c[0] == "smoothadv_fill"][0][1][2]]
        torch.manual_seed(6)
        assert seeds == [atk._fresh_seed(), atk._fresh_seed()]                        # the start's key, then the noise key
        step = [c for c in table.calls if c[0] == "smoothadv_step"][0]
        assert step[2]["norm"] == norm


@pytest.mark.parametrize("kw, word", [({"sigma": 0.0}, "sigma"), ({"sigma": -1.0}, "sigma"), ({"sigma": float("nan")}, "sigma"),
                                      ({"sigma": float("inf")}, "sigma"), ({"steps": 0}, "steps, samples"), ({"samples": 0}, "steps, samples"),
                                      ({"max_rows": 0}, "steps, samples"), ({"norm": "L1"}, "norm"), ({"eps": -0.1}, "eps"),
                                      ({"eps": float("nan")}, "eps"), ({"alpha": -1.0}, "alpha")])
def test_validation_errors(kw, word):
    with pytest.raises(ValueError, match=word):
        torchattacks.SmoothAdvPGD(Surrogate(), **kw)


# ---- the loop's hand-over -------------------------------------------------------------------------------------------------------------

def test_certify_sigma_is_handed_to_the_attack(caplog):
    import inspect
    atk = torchattacks.SmoothAdvPGD(Surrogate(), sigma=0.05)
    assert evaluation.adopt_certify_sigma(atk, None) is False and atk.sigma == 0.05
    with caplog.at_level(logging.INFO, logger=evaluation.LOGGER.name):
        assert evaluation.adopt_certify_sigma(atk, 0.25) is True
    assert atk.sigma == 0.25 and len([r for r in caplog.records if "SmoothAdvPGD" in r.getMessage()]) == 1
    other = torchattacks.PGDL2(Surrogate())
    assert evaluation.adopt_certify_sigma(other, 0.25) is False and not hasattr(other, "sigma")
    assert evaluation.adopt_certify_sigma(None, 0.25) is False
    assert "adopt_certify_sigma(atk, certify)" in inspect.getsource(evaluation.generate_attacks)


# ---- the trainer ------------------------------------------------------------------------------------------------------------------------

def test_noise_sigma_flag_parses():
    import train_models_on_adversarial_attacks as cli
    assert cli.parse_args([]).noise_sigma is None
    assert cli.parse_args(["--noise_sigma", "0.05"]).noise_sigma == 0.05
    assert T.Trainer.noise_sigma is None and T.Trainer().noise_sigma is None


def fit(noise_sigma, attacks=("FGSM_eps001",), table=None):
    random.seed(3)
    np.random.seed(3)
    torch.manual_seed(3)
    model = Surrogate().train()
    tr = T.AdversarialGDTrainer(epochs=2, batch_size=4, device="cpu", optimizer_kwargs={"lr": 1e-3})
    tr.attack_ops = table if table is not None else RecordingTable()
    tr.noise_sigma = noise_sigma
    trained = tr.train(dataset=TinyDetectionSet(16, 1024, 21), model=model, attack_model=model, adversarial_attacks=list(attacks),
                       test_dataset=TinyDetectionSet(8, 1024, 22))
    return tr, {k: v.clone() for k, v in trained.state_dict().items()}


def test_trainer_without_noise_calls_nothing_new():
    tr, sd = fit(None)
    assert "smooth_noise" not in [c[0] for c in tr.attack_ops.calls] and tr.attack_ops.calls
    import oracle.torch_ops as plain                                                   # and the same run on the plain table: same weights
    _, sd_plain = fit(None, table=plain)
    assert all(torch.equal(sd[k], sd_plain[k]) for k in sd)


def test_trainer_with_noise_calls_once_per_training_step():
    tr, sd = fit(0.05)
    noise = [c for c in tr.attack_ops.calls if c[0] == "smooth_noise"]
    assert len(noise) == 2 * 4                                                         # 2 epochs x 16 / 4 training steps; validation is clean
    offsets = [c[2]["offset"] for c in noise]
    assert offsets == list(range(8)) and len({c[1][2] for c in noise}) == 1           # strictly distinct offsets under one key
    assert all(c[1][1] == 0.05 and c[2]["ns"] == 1 and tuple(c[1][0].shape) == (4, 1024) for c in noise)
    _, sd_clean = fit(None)
    assert any(not torch.equal(sd[k], sd_clean[k]) for k in sd) and all(torch.isfinite(v).all() for v in sd.values())
    plain = T.GDTrainer(epochs=1, batch_size=4, device="cpu")                           # the plain trainer hands it on
    plain.noise_sigma, plain.attack_ops = 0.05, RecordingTable()
    plain.train(TinyDetectionSet(16, 1024, 21), Surrogate().train(), test_dataset=TinyDetectionSet(8, 1024, 22))
    assert [c[0] for c in plain.attack_ops.calls] == ["smooth_noise"] * 4
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="noise_sigma"):
            fit(bad)


def test_smoothadv_training_on_the_twin_table():
    """--noise_sigma with SMOOTHADV among the attacks is SmoothAdv training: the trainer is the attack API's second caller."""
    table = RecordingTable()
    random.seed(3)
    torch.manual_seed(3)
    model = Surrogate().train()
    tr = T.EqualAdversarialGDTrainer(epochs=1, batch_size=4, device="cpu", optimizer_kwargs={"lr": 1e-3})
    tr.attack_ops, tr.noise_sigma = table, 0.05
    real = tr.init_adv_attacks

    def small(attack_model, names):                                                    # the enum's attack at 2 steps of 2 draws
        attacks = real(attack_model, names)
        for _, atk in attacks:
            atk.steps, atk.samples = 2, 2
        return attacks
    tr.init_adv_attacks = small
    before = {k: v.clone() for k, v in model.state_dict().items()}
    out = tr.train(dataset=TinyDetectionSet(8, 1024, 21), model=model, attack_model=model, adversarial_attacks=["SMOOTHADV"],
                   test_dataset=TinyDetectionSet(4, 1024, 22))
    names = [c[0] for c in table.calls]
    assert names.count("smooth_noise") == 2 and names.count("smoothadv_step") >= 2 * 2
    fills = [c for c in table.calls if c[0] == "smoothadv_fill"]
    assert all(c[2]["scale"] is not None for c in fills)                               # the trainer handed mn / mx over
    assert any(not torch.equal(v, before[k]) for k, v in out.state_dict().items())
    assert all(torch.isfinite(v).all() for v in out.state_dict().values())
