"""CPU: randomized smoothing's host side — the numpy twin's normals are standard normal, the Clopper-Pearson bound and the
certified radius (metrics.py) have the properties the certificate's soundness rests on, `certified_summary` on hand-made rows,
the CLI flags and the validation errors, and `_active_reports` with the arguments it had before `certify=` existed."""
import inspect
from pathlib import Path

import numpy as np
import pytest
import torch
from scipy import stats

from audio_deepfake_adversarial_attacks_amd import evaluation, metrics
from tests import smooth_cpu_ops as S

ROOT = Path(__file__).resolve().parent.parent


# ---- the twin's normals -----------------------------------------------------------------------------------------------------------------

def test_twin_normals_are_standard_normal():
    """Seed 7, 16 x 65 536 draws: mean and variance within 5 standard errors of 0 and 1 (the variance's standard error is
    sqrt(2 / N)), and a Kolmogorov-Smirnov test on the first 200 000 does not reject at 1e-3."""
    z = S.normals_np(16, 65_536, seed=7, counter=0).astype(np.float64).ravel()
    N = z.size
    print(f"mean {z.mean():.3e} variance {z.var():.5f} fourth moment {np.mean(z ** 4):.4f}")
    assert abs(z.mean()) < 5.0 / np.sqrt(N)
    assert abs(z.var() - 1.0) < 5.0 * np.sqrt(2.0 / N)
    p = stats.kstest(z[:200_000], "norm").pvalue
    print(f"KS p = {p:.3f}")
    assert p > 1e-3
    assert np.abs(z).max() <= np.sqrt(-2.0 * np.log(2.0 ** -24)) * (1 + 1e-6)       # 5.77: the 24-bit uniforms' reach


def test_twin_forms_agree_and_slots_take_consecutive_counters():
    x = torch.rand(3, 37, generator=torch.Generator().manual_seed(1)) - 0.5
    a32 = S.smooth_noise_np(x, 0.05, seed=9, offset=5, s0=2, ns=3)
    a64 = S.smooth_noise_np(x, 0.05, seed=9, offset=5, s0=2, ns=3, dtype=np.float64)
    assert a32.dtype == np.float32 and a64.dtype == np.float64 and a32.shape == (3, 3, 37)
    assert np.abs(a32 - a64).max() < 0.05 * 2e-6 + 2.0 ** -24                        # libm float32 against float64, and the final add
    for i in range(3):                                                              # slot s is counter offset + s, whole or alone
        np.testing.assert_array_equal(a32[i], S.smooth_noise_np(x, 0.05, seed=9, offset=7 + i, s0=0, ns=1)[0])
    hi = S.smooth_noise_np(x, 0.05, seed=9, offset=2 ** 32 - 1, s0=0, ns=2)         # the carry into the high counter word
    np.testing.assert_array_equal(hi[1], S.smooth_noise_np(x, 0.05, seed=9, offset=2 ** 32, s0=0, ns=1)[0])
    assert not np.array_equal(hi[1], S.smooth_noise_np(x, 0.05, seed=9, offset=0, s0=0, ns=1)[0])


def test_tally_twin():
    z = np.array([[np.nan, 0.0, -0.0, np.inf], [1e-45, -1e-45, -np.inf, 3.0]], dtype=np.float32)
    np.testing.assert_array_equal(S.smooth_tally_np(z, np.array([5, 0, 0, 1], np.int32)), [6, 0, 0, 3])


# ---- the statistics -----------------------------------------------------------------------------------------------------------------------

def test_clopper_pearson_lower_properties():
    n, alpha = 100, 0.001
    assert metrics.clopper_pearson_lower(0, n, alpha) == 0.0
    for m in (1, 100, 1000):                                                        # k == n in closed form
        assert abs(metrics.clopper_pearson_lower(m, m, alpha) - alpha ** (1.0 / m)) < 1e-12
        assert abs(metrics.clopper_pearson_lower(m, m, alpha) - stats.beta.ppf(alpha, m, 1)) < 1e-12
    p100 = metrics.clopper_pearson_lower(100, 100, alpha)
    assert abs(p100 - 0.933254) < 1e-6
    # the issue quotes 1.5007 sigma for this radius; norm.ppf(0.9332543) is 1.50048 (Phi(1.5) = 0.9331928, phi(1.5) = 0.1295):
    # pinned to the value, which agrees with the quoted figure to 3e-4
    r100 = metrics.certified_radius(100, 100, alpha, 1.0)
    assert abs(r100 - stats.norm.ppf(p100)) < 1e-12 and abs(r100 - 1.5007) < 3e-4
    k = np.arange(1, n)
    p = metrics.clopper_pearson_lower(k, n, alpha)
    np.testing.assert_allclose(stats.binom.sf(k - 1, n, p), alpha, rtol=0, atol=1e-9)  # P(X >= k | p_lower) = alpha: the definition
    full = metrics.clopper_pearson_lower(np.arange(0, n + 1), n, alpha)
    assert (np.diff(full) > 0).all() and (full < np.arange(0, n + 1) / n + 1e-15).all()   # monotone in k, and below k / n
    for n_ in (1, 7, 100, 1000):                                                      # k <= n / 2 abstains
        ks = np.arange(0, n_ // 2 + 1)
        assert (np.asarray(metrics.certified_radius(ks, n_, alpha, 0.25)) == -1.0).all()
    r = np.asarray(metrics.certified_radius(np.arange(0, 1001), 1000, alpha, 0.05))
    cert = r[r >= 0]
    assert (np.diff(cert) > 0).all() and abs(cert[-1] - 0.05 * stats.norm.ppf(alpha ** 0.001)) < 1e-15
    assert abs(cert[-1] / 0.05 - 2.46) < 0.005                                        # the ceiling at n = 1000: 2.46 sigma
    with pytest.raises(ValueError):
        metrics.clopper_pearson_lower(3, 2, alpha)
    with pytest.raises(ValueError):
        metrics.clopper_pearson_lower(1, 2, 1.0)


def test_smoothed_prediction_is_the_binomial_test():
    n0, alpha = 64, 0.001
    c1 = np.arange(0, n0 + 1)
    got = metrics.smoothed_prediction(c1, n0, alpha)
    for c, g in zip(c1, got):
        abstain = stats.binomtest(int(max(c, n0 - c)), n0, 0.5).pvalue > alpha
        assert g == (-1 if abstain else int(2 * c > n0))
    assert got[0] == 0 and got[n0] == 1 and got[n0 // 2] == -1
    assert (metrics.smoothed_prediction(np.arange(0, 9), 8, alpha) == -1).all()         # 2 / 2^8 > 0.001: 8 votes never decide


def test_certified_summary_on_hand_made_rows():
    sigma, n, n0, alpha = 0.05, 1000, 100, 0.001
    #        class kA     label span
    table = [(1, 1000, 1, 1.0),        # right, the ceiling: 2.46 sigma = 0.1232, normalised 0.1232
             (0, 990, 0, 0.5),         # right, normalised = radius / 0.5
             (1, 900, 0, 1.0),         # certified for the WRONG class
             (0, 500, 0, 1.0),         # abstains (kA <= n / 2)
             (1, 530, 1, 2.0),         # abstains: 0.53 is not significantly above one half at n = 1000
             (1, 700, 1, 0.25)]        # right, a small radius over a small span
    rows = np.array([(c, k) for c, k, _, _ in table])
    y = np.array([t[2] for t in table])
    span = np.array([t[3] for t in table])
    out = metrics.certified_summary(rows, y, span, sigma, n, n0, alpha)
    radius = np.array([sigma * stats.norm.ppf(stats.beta.ppf(alpha, k, n - k + 1)) if k < n else sigma * stats.norm.ppf(alpha ** (1 / n))
                       for k in rows[:, 1]])
    assert radius[3] < 0 and radius[4] < 0 and (radius[[0, 1, 2, 5]] > 0).all()           # the table's comments hold
    right = [0, 1, 5]
    assert list(out) == ["certified/accuracy", "certified/abstained", "certified/radius_median", "certified/radius_norm_median",
                         "certified/accuracy_at_0.1", "certified/accuracy_at_0.15", "certified/accuracy_at_0.2",
                         "certified/radius_max", "certified/sigma", "certified/n", "certified/alpha"]
    assert out["certified/accuracy"] == pytest.approx(100 * 3 / 6) and out["certified/abstained"] == pytest.approx(100 * 2 / 6)
    assert out["certified/radius_median"] == pytest.approx(np.median(radius[right]), abs=1e-15)       # abstentions and the wrong row excluded
    rnorm = radius / span
    assert out["certified/radius_norm_median"] == pytest.approx(np.median(rnorm[right]), abs=1e-15)
    # the thresholds act on the NORMALISED radius: row 1 (radius 0.098 < 0.1, normalised 0.197) counts at 0.1 and 0.15,
    # row 5 (radius 0.018, normalised 0.07) at none, row 0 (0.123) at 0.1 only
    assert radius[1] < 0.1 < 0.15 < rnorm[1] < 0.2 and rnorm[5] < 0.1 < rnorm[0] < 0.15
    assert out["certified/accuracy_at_0.1"] == pytest.approx(100 * 2 / 6)
    assert out["certified/accuracy_at_0.15"] == pytest.approx(100 * 1 / 6)
    assert out["certified/accuracy_at_0.2"] == 0.0
    assert out["certified/radius_max"] == pytest.approx(radius[0], abs=1e-15) and out["certified/radius_max"] / sigma == pytest.approx(2.46, abs=0.005)
    assert (out["certified/sigma"], out["certified/n"], out["certified/alpha"]) == (0.05, 1000, 0.001)
    assert isinstance(out["certified/n"], int)
    other = metrics.certified_summary(rows, y, span, sigma, n, n0, alpha, report_at=(0.05,))
    assert other["certified/accuracy_at_0.05"] == pytest.approx(100 * 3 / 6) and "certified/accuracy_at_0.1" not in other
    none = metrics.certified_summary(rows[3:5], y[3:5], span[3:5], sigma, n, n0, alpha)  # everything abstained: no median
    assert none["certified/abstained"] == 100.0 and np.isnan(none["certified/radius_median"]) and none["certified/accuracy"] == 0.0


# ---- flags, validation, defaults -------------------------------------------------------------------------------------------------------------

def test_cli_flags_reach_generate_attacks(monkeypatch):
    import evaluate_models_on_adversarial_attacks as cli
    args = cli.parse_arguments(["--certify", "0.05", "--certify_samples", "32", "--certify_select", "8", "--certify_alpha", "0.01",
                                "--synthetic", "8", "--config", str(ROOT / "configs" / "aa_evaluation" / "lcnn.yaml")])
    assert (args.certify, args.certify_samples, args.certify_select, args.certify_alpha) == (0.05, 32, 8, 0.01)
    plain = cli.parse_arguments([])
    assert (plain.certify, plain.certify_samples, plain.certify_select, plain.certify_alpha) == (None, 1000, 100, 0.001)
    seen = {}
    monkeypatch.setattr(cli, "generate_attacks", lambda **kw: seen.update(kw) or {})
    monkeypatch.setattr(cli.torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(cli.torch.cuda, "set_device", lambda i: None)
    monkeypatch.setattr(cli, "set_seed", lambda s: None)
    cli.main(args)
    assert (seen["certify"], seen["certify_samples"], seen["certify_select"], seen["certify_alpha"]) == (0.05, 32, 8, 0.01)
    sig = inspect.signature(evaluation.generate_attacks).parameters
    assert [sig[k].default for k in ("certify", "certify_samples", "certify_select", "certify_alpha")] == [None, 1000, 100, 0.001]


@pytest.mark.parametrize("kw, word", [({"certify": 0.0}, "sigma"), ({"certify": -0.1}, "sigma"), ({"certify": float("nan")}, "sigma"),
                                      ({"certify": 0.05, "certify_samples": 0}, "n, n0"), ({"certify": 0.05, "certify_select": 0}, "n, n0"),
                                      ({"certify": 0.05, "certify_alpha": 0.0}, "alpha"), ({"certify": 0.05, "certify_alpha": 1.0}, "alpha")])
def test_validation_errors(kw, word):
    with pytest.raises(ValueError, match=word):
        evaluation._active_reports(None, "cpu", 0, None, 2, False, False, None, 1, None, None, None, **kw)
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    names = {"certify": "sigma", "certify_samples": "n", "certify_select": "n0", "certify_alpha": "alpha"}
    with pytest.raises(ValueError, match=word):
        torchattacks.Smoothing(**{"sigma": 0.05, **{names[k]: v for k, v in kw.items()}})


def test_active_reports_defaults_are_todays():
    """With the arguments it had before `certify=`, `_active_reports` returns what it returned: nothing for a plain run, and no
    certify scorer beside another report; the new parameters are the last four and have defaults."""
    assert evaluation._active_reports(None, "cpu", 0, None, 2, False, False, None, 1, None, None, None) == []
    only = evaluation._active_reports(None, "cpu", 0, None, 2, False, True, None, 1, None, None, None)
    assert [type(r).__name__ for r in only] == ["_RowReport"] and only[0].key == "masking"
    names = list(inspect.signature(evaluation._active_reports).parameters)
    assert names[-4:] == ["certify", "certify_samples", "certify_select", "certify_alpha"] and names[-5] == "universal_save"
    got = evaluation._active_reports(None, "cpu", 0, None, 2, False, True, None, 1, None, None, None, certify=0.05,
                                     certify_samples=32, certify_select=8)
    assert [type(r).__name__ for r in got] == ["_RowReport", "_CertifyScorer"]
    sc = got[-1]
    assert (sc.smooth.sigma, sc.smooth.n, sc.smooth.n0, sc.smooth.alpha, sc.attacked, sc.offset) == (0.05, 32, 8, 0.001, False, 0)
    assert evaluation.format_certified({"certified/accuracy": 50.0, "certified/n": 32, "certified/violations": 0, "adv_eval/eer": 0.1}) \
        == "certified/accuracy: 50, certified/n: 32, certified/violations: 0"


def test_linear_case_is_what_it_says():
    for T in (1028, 1030):
        model, x, y, k, sigma = S.linear_case(T)
        z = (x.double() @ model.w.detach() + model.bias)
        wn = model.w.detach().norm()
        np.testing.assert_allclose((z / (sigma * wn)).numpy(), k.numpy(), rtol=0, atol=1e-6)   # the clean logit is k sigma ||w||
        assert abs(float(wn) - 64.0) < 1e-4 and x.shape == (8, T) and float(x.abs().max()) <= 0.25
        stacked = torch.cat([x, x, x])                                                         # slot-major rows get their own row's bias
        assert torch.equal(model(stacked).reshape(3, 8), model(x).reshape(1, 8).expand(3, 8))
