"""CPU: the adversarial-training caller (audio_deepfake_adversarial_attacks_amd/trainer.py) against runs of the
REFERENCE's own trainers (src/trainer.py) recorded in tests/golden/trainer.npz — same seeds, same tiny in-memory set,
surrogate detector, FGSM attacks through the CPU op table.  Everything the reference logs and the final weights must
come out identical: the strategies draw from `random` / torch's generator exactly where the reference does."""
import logging
import random

import numpy as np
import pytest
import torch

from audio_deepfake_adversarial_attacks_amd import trainer as T
from audio_deepfake_adversarial_attacks_amd.aa.aa_trainer_types import AdversarialGDTrainerEnum
from oracle import torch_ops
from tests.helpers import Surrogate, TinyDetectionSet, golden_for_this_cpu

RUNS = {
    "RANDOM": ["FGSM", "FGSM_eps00075", "FGSM_eps001"],
    "EQUAL": ["FGSM_eps001"],
    "ONLY_ADV": ["FGSM_eps00075"],
    "ADAPTIVE": ["FGSM", "FGSM_eps001"],
    "ADAPTIVE_V2": ["FGSM", "FGSM_eps00075", "FGSM_eps001"],
}


@pytest.fixture(autouse=True)
def one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def _model_from(g, prefix):
    m = Surrogate()
    m.load_state_dict({k[len(prefix):]: torch.from_numpy(v) for k, v in g.items() if k.startswith(prefix)})
    return m


def _run(strategy, attacks, g):
    model = _model_from(g, "init_model_").train()     # constructing a module draws from torch's generator: seed afterwards
    random.seed(3)
    np.random.seed(3)
    torch.manual_seed(3)
    records = []
    handler = logging.Handler()
    handler.emit = lambda rec: records.append(rec.getMessage())
    T.LOGGER.setLevel(logging.INFO)
    T.LOGGER.addHandler(handler)
    try:
        tr = AdversarialGDTrainerEnum[strategy].value(epochs=2, batch_size=4, device="cpu", optimizer_kwargs={"lr": 1e-3})
        tr.attack_ops = torch_ops
        trained = tr.train(dataset=TinyDetectionSet(16, 1024, 21), model=model, attack_model=model,
                           adversarial_attacks=attacks, test_dataset=TinyDetectionSet(8, 1024, 22))
    finally:
        T.LOGGER.removeHandler(handler)
    return tr, trained, [m for m in records if m.startswith(("Epoch [", "[0"))]


@pytest.mark.parametrize("strategy", list(RUNS))
def test_strategy_reproduces_reference_run(golden, strategy):
    g = golden_for_this_cpu(golden, "trainer")
    tr, trained, log = _run(strategy, RUNS[strategy], g)
    want_log = [str(m) for m in g[f"{strategy}_log"]]
    assert log == want_log, "\n".join(f"{a!r}\n{b!r}" for a, b in zip(log, want_log) if a != b)
    for k, v in trained.state_dict().items():
        assert np.array_equal(v.numpy(), g[f"{strategy}_model_{k}"]), (strategy, k)
    if f"{strategy}_weights" in g:
        assert np.array_equal(np.array(tr.adv_attacks_weights, dtype=np.float64), g[f"{strategy}_weights"])


def test_registry_and_rules():
    assert [e.name for e in AdversarialGDTrainerEnum] == ["ONLY_ADV", "RANDOM", "ADAPTIVE", "ADAPTIVE_V2", "EQUAL"]
    assert T.AdversarialGDTrainer.multi_f1_score([0.5, 0.5]) == 0.5
    assert abs(T.AdversarialGDTrainer.multi_f1_score([0.9, 0.6, 0.3]) - 3 * 0.162 / 1.8) < 1e-12
    with pytest.raises(AssertionError, match="only one attack"):
        T.OnlyOneAdversarialGDTrainer().init_adv_attacks(Surrogate(), ["FGSM", "FGSM_eps001"])
    tr = T.Trainer()
    assert (tr.epochs, tr.batch_size, tr.device, tr.use_scheduler, tr.optimizer_kwargs) == (20, 32, "cpu", False, {"lr": 1e-3})


def test_plain_gd_trainer_learns(tmp_path):
    """GDTrainer (src/trainer.py:76-210): a separable toy problem is fitted; save_model writes the reference's layout."""
    torch.manual_seed(0)
    random.seed(0)

    class Toy(torch.utils.data.Dataset):
        def __init__(self, n):
            self.y = torch.arange(n) % 2
            self.x = torch.randn(n, 256) * 0.01 + (self.y.float() * 2 - 1).unsqueeze(1) * 0.3     # class = sign of the DC offset

        def __len__(self):
            return len(self.y)

        def __getitem__(self, i):
            return self.x[i], 16_000, int(self.y[i])

    model = Surrogate().train()
    out = T.GDTrainer(epochs=6, batch_size=8, optimizer_kwargs={"lr": 5e-2}).train(Toy(64), model, test_len=0.25)
    with torch.no_grad():
        d = Toy(64)
        acc = ((out(d.x).reshape(-1) > 0).long() == d.y).float().mean().item()
    assert acc >= 0.9
    T.save_model(out, tmp_path, "toy", epoch=3)
    T.save_model(out, tmp_path, "toy")
    assert (tmp_path / "toy" / "ckpt_03.pth").exists() and (tmp_path / "toy" / "ckpt.pth").exists()
