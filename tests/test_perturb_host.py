"""CPU: the float64 reference of the perturbation report on rows that can be checked by hand, the run-level summary, the
argument validation of the C ABI (no device needed: every check fails or returns before a launch) and the CLI flag."""
import ctypes
import math

import numpy as np
import pytest

from tests import perturb_ref as R


def planes(x, d):
    out = R.perturb_ref(np.asarray(x, dtype=np.float32), np.asarray(d, dtype=np.float32))
    return {name: out[k] for k, name in enumerate(R.PLANES)}


# ---- tests/perturb_ref.py -------------------------------------------------------------------------------------------------

def test_reference_on_a_constant_row_is_20_db():
    T = 1024
    p = planes(np.ones((1, T)), np.full((1, T), 0.1))
    d = float(np.float32(0.1))
    assert p["linf"][0] == d and p["l1_mean"][0] == pytest.approx(d, rel=1e-15)
    assert p["l2"][0] == pytest.approx(d * math.sqrt(T), rel=1e-15) and p["energy"][0] == T
    assert p["snr_db"][0] == pytest.approx(20.0, abs=1e-6) and p["seg_snr_db"][0] == pytest.approx(20.0, abs=1e-6)


def test_reference_clamps_segments_at_both_ends():
    x = np.ones((1, 512))
    d = np.concatenate([np.full(256, 10.0 ** -2.5), np.full(256, 10.0 ** 1.5)])[None]   # 50 dB, then -30 dB
    terms = R.segment_terms(x.astype(np.float32), d.astype(np.float32))
    assert terms.tolist() == [[35.0, -10.0]]
    p = planes(x, d)
    assert p["seg_snr_db"][0] == 12.5
    assert p["snr_db"][0] == pytest.approx(10 * math.log10(512 / (256 * 1e-5 + 256 * 1e3)), abs=1e-5)   # unclamped


def test_reference_corner_rows():
    T = 600                                                  # two full segments and 88 samples that belong to none
    x = np.linspace(-1, 1, T)[None]
    still = planes(x, np.zeros((1, T)))                      # nothing moved
    assert still["snr_db"][0] == np.inf and still["seg_snr_db"][0] == 35.0 and still["linf"][0] == 0 == still["l2"][0]
    silent = planes(np.zeros((1, T)), np.full((1, T), 0.25))  # silence attacked
    assert silent["snr_db"][0] == -np.inf and silent["seg_snr_db"][0] == -10.0 and silent["energy"][0] == 0
    both = planes(np.zeros((1, T)), np.zeros((1, T)))
    assert np.isnan(both["snr_db"][0]) and both["seg_snr_db"][0] == 35.0      # e_d == 0 counts 35 also when e_x == 0
    tail = np.zeros((1, T))
    tail[0, 512:] = 0.5                                      # moved only past the last full segment
    p = planes(x, tail)
    assert p["seg_snr_db"][0] == 35.0 and np.isfinite(p["snr_db"][0]) and p["linf"][0] == 0.5
    nan = np.zeros((1, T))
    nan[0, 300] = np.nan
    p = planes(x, nan)
    assert all(np.isnan(p[k][0]) for k in ("linf", "l1_mean", "l2", "snr_db", "seg_snr_db")) and np.isfinite(p["energy"][0])


def test_reference_without_a_full_segment():
    p = planes(np.ones((2, 255)), np.full((2, 255), 0.1))
    assert np.isnan(p["seg_snr_db"]).all() and p["snr_db"] == pytest.approx([20.0, 20.0], abs=1e-6)
    empty = planes(np.zeros((3, 0)), np.zeros((3, 0)))
    assert [empty[k].tolist() for k in ("linf", "l2", "energy")] == [[0.0] * 3] * 3
    assert all(np.isnan(empty[k]).all() for k in ("l1_mean", "snr_db", "seg_snr_db"))


def test_difference_rounds_once_to_float32():
    x, adv = np.array([[0.1, 1.0]]), np.array([[0.1 + 1e-9, 1.0 + 1e-3]])
    d = R.difference(x, adv)
    assert d.dtype == np.float32 and d[0, 0] == np.float32(0.1 + 1e-9) - np.float32(0.1)
    with pytest.raises(AssertionError):
        R.perturb_ref(x, d.astype(np.float64))


# ---- metrics.perturbation_summary ------------------------------------------------------------------------------------------

KEYS = ("linf_max", "linf_mean", "l2_mean", "l2_median", "snr_db_median", "snr_db_min", "seg_snr_db_mean", "seg_snr_db_min")


def test_summary_with_infinite_and_nan_rows():
    from audio_deepfake_adversarial_attacks_amd import hip_ops, metrics
    assert hip_ops.PERTURBATION_PLANES == metrics.PERTURBATION_PLANES == R.PLANES
    nan, inf = float("nan"), float("inf")
    stats = {"linf": [0.1, 0.3, 0.0, 0.2, 0.5], "l1_mean": [0.0] * 5, "l2": [1.0, 3.0, 0.0, 2.0, 9.0], "energy": [1.0] * 5,
             "snr_db": [20.0, 10.0, inf, nan, 30.0], "seg_snr_db": [15.0, 5.0, 35.0, 20.0, nan]}
    wrong = np.array([True, False, True, True, True])
    s = metrics.perturbation_summary(stats, wrong)
    assert set(s) == {f"perturbation/{k}" for k in KEYS} | {f"perturbation/misclassified/{k}" for k in KEYS} | \
        {"perturbation/nan_rows"}
    assert s["perturbation/nan_rows"] == 2                                   # rows 3 and 4 are left out of everything
    assert s["perturbation/linf_max"] == 0.3 and s["perturbation/linf_mean"] == pytest.approx(0.4 / 3)
    assert s["perturbation/l2_mean"] == pytest.approx(4 / 3) and s["perturbation/l2_median"] == 1.0
    assert s["perturbation/snr_db_median"] == 20.0 and s["perturbation/snr_db_min"] == 10.0    # +inf takes part as it is
    assert s["perturbation/seg_snr_db_mean"] == pytest.approx(55 / 3) and s["perturbation/seg_snr_db_min"] == 5.0
    assert s["perturbation/misclassified/linf_max"] == 0.1 and s["perturbation/misclassified/l2_median"] == 0.5
    assert s["perturbation/misclassified/snr_db_median"] == inf and s["perturbation/misclassified/snr_db_min"] == 20.0
    # the same from the (6, N) array of hip_ops.perturbation_stats
    again = metrics.perturbation_summary(np.array([stats[k] for k in R.PLANES]), wrong)
    assert all(again[k] == v or (np.isnan(again[k]) and np.isnan(v)) for k, v in s.items())


def test_summary_with_nobody_misclassified():
    from audio_deepfake_adversarial_attacks_amd import metrics
    stats = np.array([[0.1, 0.2], [0, 0], [1.0, 2.0], [1, 1], [20.0, 30.0], [10.0, 12.0]])
    s = metrics.perturbation_summary(stats, np.zeros(2, dtype=bool))
    assert all(np.isnan(s[f"perturbation/misclassified/{k}"]) for k in KEYS)
    assert s["perturbation/nan_rows"] == 0 and s["perturbation/snr_db_median"] == 25.0 and s["perturbation/linf_max"] == 0.2
    with pytest.raises(ValueError):
        metrics.perturbation_summary(stats, np.zeros(3, dtype=bool))
    none = metrics.perturbation_summary(np.full((6, 2), np.nan), np.ones(2, dtype=bool))      # NaN rows only
    assert none["perturbation/nan_rows"] == 2 and all(np.isnan(none[f"perturbation/{k}"]) for k in KEYS)


# ---- C ABI ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from audio_deepfake_adversarial_attacks_amd import build
    build.build()
    from audio_deepfake_adversarial_attacks_amd import _lib
    return _lib.load()


def test_workspace_formula(lib):
    size = lib.advstep_perturb_stats_workspace_bytes
    for B, T in ((1, 1), (3, 255), (2, 4096), (3, 4097), (7, 8191), (128, 64_600), (65_535, 12_289)):
        need = 5 * B * math.ceil(T / 4096) * 4
        assert size(B, T) == (need + 15) // 16 * 16, (B, T)          # five float planes back to back, rounded up to 16 bytes
    assert size(128, 64_600) == 5 * 128 * 16 * 4
    assert size(0, 5) == size(5, 0) == size(-1, 5) == 0


def test_argument_validation_needs_no_device(lib):
    """Everything here is rejected, or found empty, before any launch."""
    OK, EINVAL, EWORKSPACE = 0, 1, 2
    call = lib.advstep_perturb_stats_f32
    x, adv, stats, ws = (ctypes.c_void_p(a) for a in (0x100000, 0x200000, 0x300000, 0x400000))   # never dereferenced
    B, T = 2, 8
    need = lib.advstep_perturb_stats_workspace_bytes(B, T)
    assert need == 48
    assert call(x, adv, stats, ws, need, -1, T, None) == EINVAL
    assert call(x, adv, stats, ws, need, B, -1, None) == EINVAL
    assert call(x, adv, stats, ws, 1 << 30, 65_536, T, None) == EINVAL                           # B is the grid's y extent
    for args in ((None, adv, stats, ws), (x, None, stats, ws), (x, adv, None, ws), (x, adv, stats, None)):
        assert call(*args, need, B, T, None) == EINVAL
    assert call(x, adv, None, None, 0, B, 0, None) == EINVAL                                     # empty rows still write stats
    rows = B * T * 4
    inside = lambda base, off: ctypes.c_void_p(base + off)                                       # noqa: E731
    assert call(x, adv, inside(0x100000, rows - 4), ws, need, B, T, None) == EINVAL               # stats over the end of x
    assert call(x, adv, inside(0x200000, -44), ws, need, B, T, None) == EINVAL                   # stats over the start of adv
    assert call(x, adv, stats, inside(0x200000, 16), need, B, T, None) == EINVAL                 # ws inside adv
    assert call(x, adv, stats, inside(0x100000, -32), need, B, T, None) == EINVAL                # ws over the start of x
    assert call(x, adv, stats, inside(0x300000, 32), need, B, T, None) == EINVAL                 # ws over stats
    assert call(x, adv, stats, ws, need - 1, B, T, None) == EWORKSPACE
    assert call(x, adv, stats, ws, 0, B, T, None) == EWORKSPACE
    assert call(x, adv, stats, inside(0x400000, 4), need, B, T, None) == EWORKSPACE              # not 16-byte aligned
    # no rows: OK, nothing launched, nothing read
    assert call(None, None, None, None, 0, 0, 64_600, None) == OK
    assert call(None, None, None, None, 0, 0, 0, None) == OK


# ---- CLI ----------------------------------------------------------------------------------------------------------------------

def test_cli_flag_parses_and_defaults_to_false():
    import evaluate_models_on_adversarial_attacks as cli
    assert cli.parse_arguments([]).perturbation_stats is False
    assert cli.parse_arguments(["--perturbation_stats", "--attack", "FGSM_eps001"]).perturbation_stats is True
    import inspect

    from audio_deepfake_adversarial_attacks_amd.aa.qualitative.attacks_analysis import AttackAnalyser
    from audio_deepfake_adversarial_attacks_amd.evaluation import generate_attacks
    assert inspect.signature(generate_attacks).parameters["perturbation_stats"].default is False
    assert inspect.signature(AttackAnalyser.__init__).parameters["stats_csv"].default is False
