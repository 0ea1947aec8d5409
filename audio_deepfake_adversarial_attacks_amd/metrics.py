"""Final aggregate of the evaluation loop (reference: src/metrics.py:9-14 and the sklearn calls of
evaluate_models_on_adversarial_attacks.py:267-293), restated in numpy so the GPU box needs neither sklearn nor
scipy.  Each function documents the library routine it reproduces; tests pin them against values the
reference's own calls produced (tests/golden/metrics.npz).  `perturbation_summary` is this package's own: the run-level
digest of the per-utterance perturbation report (include/advstep_perturb.h); so is `radius_summary`, the digest of the
per-utterance minimal radii of torchattacks.MinRadiusPGD, `universal_summary`, the fitted / held-out split of a run with one
universal perturbation (torchattacks.UniversalPGD), `query_summary`, the digest of the per-utterance model queries of a
score-based attack (torchattacks.SPSA), `sparsity_summary`, the digest of the per-utterance changed-sample counts of a
sparse attack (torchattacks.PGDL0), and the statistics of randomized smoothing (torchattacks.Smoothing): `clopper_pearson_lower`,
`certified_radius`, `smoothed_prediction` and `certified_summary` — these four import scipy where they run."""
from typing import Dict, Optional, Sequence, Tuple

import numpy as np


def roc_curve(y_true: np.ndarray, y_score: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """sklearn.metrics.roc_curve(y_true, y_score) with drop_intermediate=True, positive label 1."""
    y_true = np.asarray(y_true).ravel() == 1
    y_score = np.asarray(y_score, dtype=np.float64).ravel()
    order = np.argsort(y_score, kind="mergesort")[::-1]
    y_score, y_true = y_score[order], y_true[order]
    distinct = np.where(np.diff(y_score))[0]
    idx = np.r_[distinct, y_true.size - 1]
    tps = np.cumsum(y_true, dtype=np.float64)[idx]
    fps = 1 + idx - tps
    thresholds = y_score[idx]
    if len(fps) > 2:  # drop collinear interior points
        keep = np.where(np.r_[True, np.logical_or(np.diff(fps, 2), np.diff(tps, 2)), True])[0]
        fps, tps, thresholds = fps[keep], tps[keep], thresholds[keep]
    tps = np.r_[0, tps]
    fps = np.r_[0, fps]
    thresholds = np.r_[np.inf, thresholds]
    fpr = fps / fps[-1] if fps[-1] > 0 else np.full_like(fps, np.nan)
    tpr = tps / tps[-1] if tps[-1] > 0 else np.full_like(tps, np.nan)
    return fpr, tpr, thresholds


def _interp_linear(xs: np.ndarray, ys: np.ndarray, x: float) -> float:
    """scipy.interpolate.interp1d(xs, ys)(x) for 1-D linear interpolation, which scipy evaluates with np.interp:
    on a run of equal xs (vertical ROC segments) the LAST point of the run is used."""
    return float(np.interp(x, xs, ys))


def _brentq(f, a: float, b: float, xtol: float = 2e-12, rtol: float = 8.881784197001252e-16, maxiter: int = 100):
    """scipy.optimize.brentq (Brent 1973, as in scipy/optimize/Zeros/brentq.c)."""
    xpre, xcur = a, b
    fpre, fcur = f(xpre), f(xcur)
    if fpre == 0:
        return xpre
    if fcur == 0:
        return xcur
    if np.sign(fpre) == np.sign(fcur):
        raise ValueError("f(a) and f(b) must have different signs")
    xblk = fblk = spre = scur = 0.0
    for _ in range(maxiter):
        if fpre != 0 and fcur != 0 and np.sign(fpre) != np.sign(fcur):
            xblk, fblk = xpre, fpre
            spre = scur = xcur - xpre
        if abs(fblk) < abs(fcur):
            xpre, xcur, xblk = xcur, xblk, xcur
            fpre, fcur, fblk = fcur, fblk, fcur
        delta = (xtol + rtol * abs(xcur)) / 2
        sbis = (xblk - xcur) / 2
        if fcur == 0 or abs(sbis) < delta:
            return xcur
        if abs(spre) > delta and abs(fcur) < abs(fpre):
            if xpre == xblk:
                stry = -fcur * (xcur - xpre) / (fcur - fpre)  # secant
            else:  # inverse quadratic extrapolation
                dpre = (fpre - fcur) / (xpre - xcur)
                dblk = (fblk - fcur) / (xblk - xcur)
                stry = -fcur * (fblk * dblk - fpre * dpre) / (dblk * dpre * (fblk - fpre))
            if 2 * abs(stry) < min(abs(spre), 3 * abs(sbis) - delta):
                spre, scur = scur, stry
            else:
                spre = scur = sbis
        else:
            spre = scur = sbis
        xpre, fpre = xcur, fcur
        xcur += scur if abs(scur) > delta else (delta if sbis > 0 else -delta)
        fcur = f(xcur)
    raise RuntimeError("brentq failed to converge")


def calculate_eer(y, y_score) -> Tuple[float, float, np.ndarray, np.ndarray]:
    """src/metrics.py:9-14: ROC of (y, -y_score); EER = root of 1 - x - tpr(x) on [0, 1]; threshold at the EER."""
    fpr, tpr, thresholds = roc_curve(y, -np.asarray(y_score, dtype=np.float64))
    eer = _brentq(lambda x: 1.0 - x - _interp_linear(fpr, tpr, x), 0.0, 1.0)
    thresh = _interp_linear(fpr, thresholds, eer)
    return thresh, eer, fpr, tpr


def roc_auc_score(y_true, y_score) -> float:
    """sklearn.metrics.roc_auc_score for binary labels: trapezoidal area under roc_curve(drop_intermediate=False)."""
    y_true = np.asarray(y_true).ravel() == 1
    y_score = np.asarray(y_score, dtype=np.float64).ravel()
    if y_true.all() or not y_true.any():
        raise ValueError("Only one class present in y_true. ROC AUC score is not defined in that case.")
    order = np.argsort(y_score, kind="mergesort")[::-1]
    y_score, y_true = y_score[order], y_true[order]
    idx = np.r_[np.where(np.diff(y_score))[0], y_true.size - 1]
    tps = np.r_[0, np.cumsum(y_true, dtype=np.float64)[idx]]
    fps = np.r_[0, 1 + idx - tps[1:]]
    trapezoid = getattr(np, "trapezoid", None) or np.trapz
    return float(trapezoid(tps / tps[-1], fps / fps[-1]))


def precision_recall_f1_binary(y_true, y_pred) -> Tuple[float, float, float]:
    """sklearn.metrics.precision_recall_fscore_support(average='binary', beta=1.0), positive label 1
    (zero_division -> 0.0, as sklearn's default 'warn' returns)."""
    y_true = np.asarray(y_true).ravel() == 1
    y_pred = np.asarray(y_pred).ravel() == 1
    tp = float(np.sum(y_true & y_pred))
    pred_pos, true_pos = float(np.sum(y_pred)), float(np.sum(y_true))
    precision = tp / pred_pos if pred_pos > 0 else 0.0
    recall = tp / true_pos if true_pos > 0 else 0.0
    f1 = 2 * precision * recall / (precision + recall) if (precision + recall) > 0 else 0.0
    return precision, recall, f1


def adversarial_report(y: np.ndarray, y_pred: np.ndarray, y_pred_label: np.ndarray) -> dict:
    """The six numbers of the reference's final log line (evaluate_models_on_adversarial_attacks.py:267-298)."""
    y = np.asarray(y).ravel()
    accuracy = 100.0 * float(np.sum(np.asarray(y_pred_label).ravel() == y)) / max(len(y), 1)
    precision, recall, f1 = precision_recall_f1_binary(y, y_pred_label)
    auc = roc_auc_score(y, y_pred)
    _, eer, _, _ = calculate_eer(y=1 - y, y_score=y_pred)  # "For EER flip values" (:282-283)
    return {"adv_eval/eer": eer, "adv_eval/accuracy": accuracy, "adv_eval/precision": precision,
            "adv_eval/recall": recall, "adv_eval/f1_score": f1, "adv_eval/auc": auc}


# ---------------------------------------------------------------------------------------------------------
# perturbation report
# ---------------------------------------------------------------------------------------------------------

# the planes of hip_ops.perturbation_stats, in the order of include/advstep_perturb.h
PERTURBATION_PLANES = ("linf", "l1_mean", "l2", "energy", "snr_db", "seg_snr_db")
# (key, plane, statistic) of the summary; the same eight once more under perturbation/misclassified/
_PERTURBATION_SUMMARY = (("linf_max", "linf", np.max), ("linf_mean", "linf", np.mean),
                         ("l2_mean", "l2", np.mean), ("l2_median", "l2", np.median),
                         ("snr_db_median", "snr_db", np.median), ("snr_db_min", "snr_db", np.min),
                         ("seg_snr_db_mean", "seg_snr_db", np.mean), ("seg_snr_db_min", "seg_snr_db", np.min))


def perturbation_summary(stats, misclassified) -> Dict[str, float]:
    """Run-level digest of the per-utterance perturbation planes.  `stats`: {plane name: (N,) array} or a (6, N) array in the
    order of PERTURBATION_PLANES; `misclassified`: (N,) bool, the utterances whose post-attack label differs from y.

    A row with a NaN in any of the four summarised planes (linf, l2, snr_db, seg_snr_db) is a NaN row: it is left out of every
    statistic, of both groups, and counted in perturbation/nan_rows.  Infinite SNRs (an utterance the attack did not move:
    +inf) take part as they are, so a median stays finite while most rows are finite.  A group without rows — no
    misclassified utterance, or NaN rows only — has NaN for every value."""
    if not isinstance(stats, dict):
        stats = dict(zip(PERTURBATION_PLANES, np.asarray(stats)))
    planes = {name: np.asarray(stats[name], dtype=np.float64).ravel() for _, name, _ in _PERTURBATION_SUMMARY}
    wrong = np.asarray(misclassified).ravel().astype(bool)
    nan_row = np.zeros(wrong.shape, dtype=bool)
    for v in planes.values():
        if v.shape != wrong.shape:
            raise ValueError(f"planes and misclassified must hold one value per utterance, got {v.shape} and {wrong.shape}")
        nan_row |= np.isnan(v)
    out: Dict[str, float] = {}
    with np.errstate(invalid="ignore"):                  # a median between +inf and -inf is NaN, quietly
        for prefix, rows in (("perturbation/", ~nan_row), ("perturbation/misclassified/", ~nan_row & wrong)):
            for key, name, stat in _PERTURBATION_SUMMARY:
                out[prefix + key] = float(stat(planes[name][rows])) if rows.any() else float("nan")
    out["perturbation/nan_rows"] = int(nan_row.sum())
    return out


# ---------------------------------------------------------------------------------------------------------
# minimal-radius report
# ---------------------------------------------------------------------------------------------------------

def _quantile_keeping_inf(ordered: np.ndarray, q: float) -> float:
    """The q-quantile of an ascending vector by linear interpolation between order statistics (numpy's default), with
    +inf taking part as a value: the result is +inf as soon as the upper neighbour carries weight and is +inf (numpy's own
    interpolation would turn inf - inf into NaN)."""
    pos = q * (len(ordered) - 1)
    i = int(np.floor(pos))
    frac = pos - i
    lo, hi = float(ordered[i]), float(ordered[min(i + 1, len(ordered) - 1)])
    if frac == 0.0 or lo == hi:
        return lo
    if np.isinf(hi):
        return hi
    return lo + (hi - lo) * frac


def radius_summary(radii, report_at: Sequence[float] = ()) -> Dict[str, float]:
    """Run-level digest of the per-utterance minimal radii of torchattacks.MinRadiusPGD (`last_radius`: 0 = the clean input is
    already misclassified, +inf = no radius up to eps_max flipped the utterance, in the attack's domain: the min-max-normalised
    waveform).

    min_radius/median, p10, p90      quantiles over ALL rows; +inf stays +inf (more than half unflipped: the median is +inf)
    min_radius/unflipped_share       the share of +inf rows, in [0, 1]
    min_radius/already_wrong_share   the share of rows with radius 0
    min_radius/robust_acc@<eps>      100 x the share of rows whose radius is > eps, for every eps of report_at, compared as
                                     float32 (the precision of the search state, so a radius that IS the grid point eps
                                     counts as broken at eps): the accuracy a PGD run at radius eps would leave, were success
                                     monotone in the radius (an upper bound otherwise: the radii are witnessed, not minimal)
    An empty vector gives NaN everywhere."""
    r32 = np.sort(np.asarray(radii, dtype=np.float32).ravel())
    r = r32.astype(np.float64)
    n = r.size
    out: Dict[str, float] = {}
    for key, q in (("median", 0.5), ("p10", 0.1), ("p90", 0.9)):
        out[f"min_radius/{key}"] = _quantile_keeping_inf(r, q) if n else float("nan")
    out["min_radius/unflipped_share"] = float(np.mean(np.isinf(r))) if n else float("nan")
    out["min_radius/already_wrong_share"] = float(np.mean(r == 0.0)) if n else float("nan")
    for eps in report_at:
        # in the radii's own precision: the search's grid points are float32 (float32(0.001) > 0.001 as a float64), and a row
        # that flipped AT eps is not robust at eps
        out[f"min_radius/robust_acc@{eps:g}"] = 100.0 * float(np.mean(r32 > np.float32(eps))) if n else float("nan")
    return out


# ---------------------------------------------------------------------------------------------------------
# universal-perturbation report
# ---------------------------------------------------------------------------------------------------------

def universal_summary(y, y_pred_label, fitted, delta, source_label: Optional[int] = None) -> Dict[str, float]:
    """Run-level digest of a run that applied ONE perturbation (torchattacks.UniversalPGD) to every utterance.  `y`,
    `y_pred_label`: (N,) labels and post-attack hard labels; `fitted`: (N,) bool, the utterances the perturbation was fitted on
    (all False for a loaded one); `delta`: the perturbation, in its own domain.

    universal/fit_utterances, heldout_utterances     the sizes of the two groups
    universal/accuracy_fit, accuracy_heldout         100 x the share of correct labels in each group (what generalises is the
                                                     held-out figure; the fitted one is the optimiser's own training score)
    universal/source_flipped_fit, _heldout           with a source label: 100 x the share of the group's SOURCE-class utterances
                                                     whose post-attack label is the other class
    universal/delta_linf, delta_l2                   max |delta| and ||delta||_2, accumulated in float64
    A group without utterances (of the source class) has NaN."""
    y, lab = np.asarray(y).ravel(), np.asarray(y_pred_label).ravel()
    fitted = np.asarray(fitted).ravel().astype(bool)
    if not (y.shape == lab.shape == fitted.shape):
        raise ValueError(f"y, y_pred_label and fitted must hold one value per utterance, got {y.shape}, {lab.shape}, {fitted.shape}")
    d = np.asarray(delta, dtype=np.float64).ravel()

    def share(rows, hit):
        return 100.0 * float(np.mean(hit[rows])) if rows.any() else float("nan")

    out: Dict[str, float] = {"universal/fit_utterances": int(fitted.sum()), "universal/heldout_utterances": int((~fitted).sum()),
                             "universal/accuracy_fit": share(fitted, lab == y),
                             "universal/accuracy_heldout": share(~fitted, lab == y)}
    if source_label is not None:
        src = y == source_label
        out["universal/source_flipped_fit"] = share(fitted & src, lab != y)
        out["universal/source_flipped_heldout"] = share(~fitted & src, lab != y)
    out["universal/delta_linf"] = float(np.max(np.abs(d))) if d.size else float("nan")
    out["universal/delta_l2"] = float(np.sqrt(np.sum(d * d)))
    return out


def filter_summary(taps, n_fft: int = 4096) -> Dict[str, float]:
    """What a universal FIR filter (torchattacks.UniversalFilter) does to a spectrum, from its taps alone: host, float64, from
    |rfft(h, n_fft)| on n_fft / 2 + 1 frequencies between 0 and half the sampling rate.

    filter/taps                        the filter's length L
    filter/gain_db_max, gain_db_min    the largest and the smallest gain over those frequencies, 20 log10 |H| (a null: -inf)
    filter/dc_gain_db                  the gain at frequency 0, 20 log10 |sum h|
    filter/identity_distance           ||h - delta||_2, delta the centred unit impulse: 0 for the filter a fit starts from"""
    h = np.asarray(taps, dtype=np.float64).ravel()
    if h.size < 1 or h.size % 2 == 0 or h.size > n_fft:
        raise ValueError(f"taps must hold an odd number of values, at most {n_fft}, got {h.size}")
    mag = np.abs(np.fft.rfft(h, n_fft))
    with np.errstate(divide="ignore"):
        db = 20.0 * np.log10(mag)
    impulse = np.zeros_like(h)
    impulse[(h.size - 1) // 2] = 1.0
    return {"filter/taps": int(h.size), "filter/gain_db_max": float(db.max()), "filter/gain_db_min": float(db.min()),
            "filter/dc_gain_db": float(db[0]), "filter/identity_distance": float(np.sqrt(np.sum((h - impulse) ** 2)))}


# ---------------------------------------------------------------------------------------------------------
# black-box query report
# ---------------------------------------------------------------------------------------------------------

def query_summary(queries, budget: int) -> Dict[str, float]:
    """Run-level digest of the model queries a score-based attack spent per utterance (torchattacks.SPSA's `last_queries`;
    `budget` = steps * slots, what an utterance that is never fooled costs).

    blackbox/queries_mean, queries_median   over all utterances
    blackbox/stopped_early                  the share of utterances below the full budget, in [0, 1]: those the attack stopped
                                            on because the detector's own answer showed them fooled (0 queries: the clean
                                            input already was)
    blackbox/budget                         `budget` itself
    An empty vector gives NaN for the three statistics."""
    q = np.asarray(queries, dtype=np.float64).ravel()
    n = q.size
    return {"blackbox/queries_mean": float(np.mean(q)) if n else float("nan"),
            "blackbox/queries_median": float(np.median(q)) if n else float("nan"),
            "blackbox/stopped_early": float(np.mean(q < budget)) if n else float("nan"),
            "blackbox/budget": int(budget)}


# ---------------------------------------------------------------------------------------------------------
# sparse (L0) report
# ---------------------------------------------------------------------------------------------------------

def sparsity_summary(changed, k: int) -> Dict[str, float]:
    """Run-level digest of the samples a sparse attack changed per utterance (torchattacks.PGDL0's `last_changed`, #{adv != x};
    `k` = the attack's budget, which no count may exceed).

    sparse/changed_mean, changed_median     over all utterances
    sparse/changed_max                      the largest count (an int; 0 for an empty vector)
    sparse/k                                `k` itself
    An empty vector gives NaN for the mean and the median."""
    c = np.asarray(changed, dtype=np.float64).ravel()
    n = c.size
    return {"sparse/changed_mean": float(np.mean(c)) if n else float("nan"),
            "sparse/changed_median": float(np.median(c)) if n else float("nan"),
            "sparse/changed_max": int(np.max(c)) if n else 0,
            "sparse/k": int(k)}


# ---------------------------------------------------------------------------------------------------------
# psychoacoustic masking report
# ---------------------------------------------------------------------------------------------------------

def masking_summary(stats, cells: int) -> Dict[str, float]:
    """Run-level digest of the masking statistics per utterance (torchattacks.PsyPGD's `last_masking`, or the one pass of
    `generate_attacks(..., masking_stats=True)`): `stats` (N, 3) = (hinge loss, time-frequency cells whose perturbation power
    exceeds the clean utterance's masking threshold, the largest ratio of power to threshold); `cells` = NF * 257, the cells of
    an utterance.

    masking/over_share_mean, over_share_median   cells over the threshold / cells, over all utterances
    masking/worst_db_median, worst_db_p90        10 log10 of the largest ratio (-inf where the perturbation is 0)
    masking/loss_mean                            the mean hinge loss
    An empty array gives NaN everywhere."""
    s = np.asarray(stats, dtype=np.float64).reshape(-1, 3)
    if not s.shape[0]:
        nan = float("nan")
        return {"masking/over_share_mean": nan, "masking/over_share_median": nan, "masking/worst_db_median": nan,
                "masking/worst_db_p90": nan, "masking/loss_mean": nan}
    share = s[:, 1] / float(cells)
    with np.errstate(divide="ignore", invalid="ignore"):
        db = 10.0 * np.log10(s[:, 2])
    return {"masking/over_share_mean": float(np.mean(share)), "masking/over_share_median": float(np.median(share)),
            "masking/worst_db_median": float(np.median(db)), "masking/worst_db_p90": float(np.percentile(db, 90)),
            "masking/loss_mean": float(np.mean(s[:, 0]))}


# ---------------------------------------------------------------------------------------------------------
# randomized-smoothing certificate (torchattacks.Smoothing; Cohen, Rosenfeld and Kolter, ICML 2019)
# ---------------------------------------------------------------------------------------------------------
# Host-side float64, once at the end of a run.  scipy is imported where it is used: the rest of this module needs numpy alone.

CERTIFIED_REPORT_AT = (0.1, 0.15, 0.2)           # the PGDL2 triplet of AttackEnum, in the normalised unit (radius / span)


def clopper_pearson_lower(k, n: int, alpha: float):
    """The one-sided Clopper-Pearson lower confidence bound of a binomial proportion from k successes in n trials, at level
    1 - alpha: the p with P(Binomial(n, p) >= k) = alpha, i.e. scipy.stats.beta.ppf(alpha, k, n - k + 1); 0 for k == 0 and
    alpha ** (1 / n) for k == n (the same value in closed form).  `k` may be an array; float64."""
    from scipy.stats import beta
    k = np.asarray(k, dtype=np.float64)
    n = int(n)
    if n < 1 or not 0.0 < float(alpha) < 1.0:
        raise ValueError(f"need n >= 1 and 0 < alpha < 1, got n = {n} and alpha = {alpha}")
    if ((k < 0) | (k > n)).any():
        raise ValueError(f"k must lie in 0 .. {n}")
    inner = (k > 0) & (k < n)
    p = np.where(k >= n, float(alpha) ** (1.0 / n), 0.0)
    if inner.any():
        p = np.where(inner, beta.ppf(float(alpha), np.where(inner, k, 1.0), np.where(inner, n - k + 1.0, 1.0)), p)
    return p if p.ndim else float(p)


def certified_radius(k, n: int, alpha: float, sigma: float):
    """Cohen's certified L2 radius of the class that got k of n noisy votes: sigma * Phi^-1(p_lower) where p_lower =
    clopper_pearson_lower(k, n, alpha) > 0.5, in sigma's unit; otherwise the procedure ABSTAINS, coded -1.  k <= n / 2 always
    abstains.  `k` may be an array; float64."""
    from scipy.stats import norm
    p = np.asarray(clopper_pearson_lower(k, n, alpha), dtype=np.float64)
    ok = p > 0.5
    r = np.where(ok, float(sigma) * norm.ppf(np.where(ok, p, 0.75)), -1.0)
    return r if r.ndim else float(r)


def smoothed_prediction(c1, n0: int, alpha: float):
    """Cohen's PREDICT from c1 class-1 votes among n0: the majority class (a tie goes to class 0), or -1 (abstain) when the
    two-sided test scipy.stats.binomtest(max(c1, n0 - c1), n0, 0.5).pvalue > alpha.  `c1` may be an array; int64."""
    from scipy.stats import binomtest
    c = np.asarray(c1, dtype=np.int64)
    top = np.maximum(c, int(n0) - c)
    pvalue = {int(m): binomtest(int(m), int(n0), 0.5).pvalue for m in np.unique(top)}
    keep = np.array([pvalue[int(m)] <= alpha for m in top.ravel()], dtype=bool).reshape(top.shape)
    out = np.where(keep, (2 * c > int(n0)).astype(np.int64), -1)
    return out if out.ndim else int(out)


def certified_summary(rows, labels, spans, sigma: float, n: int, n0: int, alpha: float,
                      report_at: Sequence[float] = CERTIFIED_REPORT_AT) -> Dict[str, float]:
    """Run-level digest of Cohen's CERTIFY per utterance.  `rows` (N, 2) = (the class the n0 selection votes picked, kA = that
    class's count among the n estimation votes); `labels` (N,); `spans` (N,) = each clean utterance's max - min, the unit of every
    `eps` of AttackEnum; `sigma` and the radii in the waveform's units.

    certified/accuracy               per cent of utterances not abstained and of the right class
    certified/abstained              per cent abstained
    certified/radius_median          the median radius over the certified-and-right rows (NaN without any)
    certified/radius_norm_median     the same of radius / span
    certified/accuracy_at_<r>        per cent certified, right and with radius / span >= r, for every r of report_at
    certified/radius_max             sigma * Phi^-1(alpha ** (1 / n)): the ceiling this n can certify
    certified/sigma, n, alpha        the run's parameters (n0 does not enter the radius)
    An empty run gives NaN for the shares and medians."""
    from scipy.stats import norm
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 2)
    y = np.asarray(labels, dtype=np.int64).ravel()
    span = np.asarray(spans, dtype=np.float64).ravel()
    if not (rows.shape[0] == y.size == span.size):
        raise ValueError(f"rows, labels and spans must hold one entry per utterance, got {rows.shape[0]}, {y.size}, {span.size}")
    N = y.size
    radius = np.asarray(certified_radius(rows[:, 1], n, alpha, sigma), dtype=np.float64).reshape(-1)
    abstained = radius < 0.0
    right = ~abstained & (rows[:, 0] == y)
    with np.errstate(divide="ignore", invalid="ignore"):
        rnorm = radius / span
    nan = float("nan")

    def pct(mask):
        return 100.0 * float(np.mean(mask)) if N else nan

    out: Dict[str, float] = {"certified/accuracy": pct(right), "certified/abstained": pct(abstained),
                             "certified/radius_median": float(np.median(radius[right])) if right.any() else nan,
                             "certified/radius_norm_median": float(np.median(rnorm[right])) if right.any() else nan}
    for r in report_at:
        out[f"certified/accuracy_at_{r:g}"] = pct(right & (rnorm >= float(r)))
    out["certified/radius_max"] = float(sigma) * float(norm.ppf(float(alpha) ** (1.0 / int(n))))
    out["certified/sigma"], out["certified/n"], out["certified/alpha"] = float(sigma), int(n), float(alpha)
    return out
