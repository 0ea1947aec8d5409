"""The optional per-run reports of evaluation.generate_attacks, end to end on the CPU: the loop runs with a stub detector, the
torch expressions of the min-max kernels and a stub attack that hands out per-utterance rows derived from its input.  Pinned:
the report's key order, each block against the metrics.*_summary of the rows the stub handed out, the `scores` arrays with
their dtypes, and the sequence of log lines."""
import logging

import numpy as np
import pytest
import torch
from torch import nn

from audio_deepfake_adversarial_attacks_amd import evaluation, metrics

N, T, B = 8, 512, 4
BASE_KEYS = ["adv_eval/eer", "adv_eval/accuracy", "adv_eval/precision", "adv_eval/recall", "adv_eval/f1_score", "adv_eval/auc",
             "num_total"]
RADIUS_KEYS = ["min_radius/median", "min_radius/p10", "min_radius/p90", "min_radius/unflipped_share",
               "min_radius/already_wrong_share", "min_radius/robust_acc@0.002", "min_radius/robust_acc@0.006"]
QUERY_KEYS = ["blackbox/queries_mean", "blackbox/queries_median", "blackbox/stopped_early", "blackbox/budget"]
SPARSE_KEYS = ["sparse/changed_mean", "sparse/changed_median", "sparse/changed_max", "sparse/k"]
MASKING_KEYS = ["masking/over_share_mean", "masking/over_share_median", "masking/worst_db_median", "masking/worst_db_p90",
                "masking/loss_mean"]
ROW_ATTRIBUTES = ("last_radius", "last_queries", "last_changed", "last_masking")


class Detector(nn.Module):
    weights_path = "stub"

    def forward(self, x):                                     # (B, T) -> (B, 1)
        return x.mean(dim=1, keepdim=True) * 40.0


class Utterances(torch.utils.data.Dataset):
    """8 utterances of 512 samples, labels 0, 1, 0, 1, ...: both classes exist, so the EER and the AUC are defined."""

    def __init__(self):
        g = torch.Generator().manual_seed(7)
        self.x = torch.randn(N, T, generator=g) * 0.05 + torch.linspace(-0.03, 0.03, N)[:, None]

    def __len__(self):
        return N

    def __getitem__(self, i):
        return [self.x[i], 16_000, i % 2, ("-", f"stub/{i}.wav", "val", T / 16_000)]


def stub_attack(carried=ROW_ATTRIBUTES):
    """A fresh attack class that carries the row attributes named in `carried` (None until called, like the shipped attacks) and
    records what it handed out, per batch, in `cls.handed`."""

    class StubAttack:
        report_at, budget, k = (0.002, 0.006), 900, 50_000
        handed = {name: [] for name in carried}

        def __init__(self, model, **params):
            self.model = model

        def set_training_mode(self, model_training=False, batchnorm_training=False):
            pass

        def __call__(self, x01, y):
            m = x01.mean(dim=1)
            rows = {"last_radius": torch.where(y == 1, m * 0.01, torch.full_like(m, float("inf"))),
                    "last_queries": (m * 1000).to(torch.int32),
                    "last_changed": (m * 100_000).to(torch.int64),
                    "last_masking": torch.stack([m, (x01 > 0.5).sum(dim=1).float(), x01.amax(dim=1) + m], dim=1)}
            for name in carried:
                setattr(self, name, rows[name])
                self.handed[name].append(rows[name])
            return x01 * 0.9 + 0.05

    for name in carried:
        setattr(StubAttack, name, None)
    return StubAttack


@pytest.fixture
def loop(monkeypatch, caplog):
    """run(attack class or None, **keywords) -> (report, the log lines after the loop's preamble)."""
    monkeypatch.setattr(evaluation, "load_model", lambda config, device: Detector())

    def to_minmax(x):
        mn, mx = x.amin(dim=1, keepdim=True), x.amax(dim=1, keepdim=True)
        return (x - mn) / (mx - mn), mn, mx

    monkeypatch.setattr(evaluation.aa_utils, "to_minmax", to_minmax)
    monkeypatch.setattr(evaluation.aa_utils, "revert_minmax", lambda x01, mn, mx: x01 * (mx - mn) + mn)
    caplog.set_level(logging.INFO)

    def run(attack, **keywords):
        caplog.clear()
        report = evaluation.generate_attacks(
            [None, None, None], {"data": {"seed": 42}}, "cpu", attack_model_config={} if attack is not None else None,
            attack_method=attack, dataset=Utterances(), batch_size=B, shuffle=False, num_workers=0, device_pad=False, **keywords)
        lines = [r.getMessage() for r in caplog.records]
        start = max(i for i, line in enumerate(lines) if line.startswith(("Attack using", "No attack applied")))
        return report, lines[start + 1:]

    return run


def handed_out(attack):
    return {name: torch.cat(parts).numpy() for name, parts in attack.handed.items()}


def test_all_attack_borne_reports_keys_values_scores_and_log(loop):
    attack = stub_attack()
    report, lines = loop(attack, return_scores=True)
    assert list(report) == BASE_KEYS + ["scores"] + RADIUS_KEYS + QUERY_KEYS + SPARSE_KEYS + MASKING_KEYS
    rows = handed_out(attack)
    assert all(len(v) == N for v in rows.values())

    def block(prefix):
        return {k: v for k, v in report.items() if k.startswith(prefix)}

    np.testing.assert_equal(block("min_radius/"), metrics.radius_summary(rows["last_radius"], attack.report_at))
    np.testing.assert_equal(block("blackbox/"), metrics.query_summary(rows["last_queries"], attack.budget))
    np.testing.assert_equal(block("sparse/"), metrics.sparsity_summary(rows["last_changed"], attack.k))
    np.testing.assert_equal(block("masking/"), metrics.masking_summary(rows["last_masking"], (1 + T // 128) * 257))
    assert report["num_total"] == N and report["blackbox/budget"] == 900 and report["sparse/k"] == 50_000

    scores = report["scores"]
    assert list(scores) == ["y_pred", "y_pred_label", "y", "min_radius", "queries", "changed", "masking"]
    for key, name, dtype, shape in (("min_radius", "last_radius", np.float32, (N,)), ("queries", "last_queries", np.int32, (N,)),
                                    ("changed", "last_changed", np.int64, (N,)), ("masking", "last_masking", np.float32, (N, 3))):
        assert scores[key].dtype == dtype and scores[key].shape == shape, key
        np.testing.assert_array_equal(scores[key], rows[name])
    np.testing.assert_array_equal(scores["y"], np.arange(N) % 2)

    assert lines == [evaluation.format_report(report), evaluation.format_min_radius(report), evaluation.format_blackbox(report),
                     evaluation.format_sparse(report), evaluation.format_masking(report)]
    assert "blackbox/budget: 900" in lines[2] and "sparse/k: 50000" in lines[3]      # the integer suffixes print as integers


def test_scores_are_left_out_without_return_scores(loop):
    report, lines = loop(stub_attack())
    assert list(report) == BASE_KEYS + RADIUS_KEYS + QUERY_KEYS + SPARSE_KEYS + MASKING_KEYS
    assert len(lines) == 5


def test_only_the_carried_attribute_reports(loop):
    attack = stub_attack(("last_queries",))
    report, lines = loop(attack, return_scores=True)
    assert list(report) == BASE_KEYS + ["scores"] + QUERY_KEYS
    assert list(report["scores"]) == ["y_pred", "y_pred_label", "y", "queries"]
    np.testing.assert_equal({k: report[k] for k in QUERY_KEYS}, metrics.query_summary(handed_out(attack)["last_queries"], 900))
    assert lines == [evaluation.format_report(report), evaluation.format_blackbox(report)]


@pytest.mark.parametrize("attack", [stub_attack(()), None], ids=["plain_attack", "no_attack"])
def test_no_optional_report_gives_the_base_keys_and_one_line(loop, attack):
    report, lines = loop(attack)
    assert list(report) == BASE_KEYS
    assert lines == [evaluation.format_report(report)]
    report, _ = loop(attack, return_scores=True)
    assert list(report) == BASE_KEYS + ["scores"] and list(report["scores"]) == ["y_pred", "y_pred_label", "y"]


@pytest.mark.parametrize("keyword", [{"universal_fit": 1}, {"universal_load": "delta.npz"}, {"universal_save": "delta.npz"}])
def test_universal_keywords_need_a_universal_attack(loop, keyword):
    with pytest.raises(ValueError) as err:
        loop(stub_attack(), **keyword)
    assert str(err.value) == "universal_fit / universal_load / universal_save need a universal attack (AttackEnum UAP*)"
