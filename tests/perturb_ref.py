"""Float64 restatement of the six per-utterance perturbation figures of include/advstep_perturb.h (numpy only).

`d` is taken as the float32 difference adv - x, rounded once as the kernel rounds it, so every decision that hangs on an
exact zero (a segment nothing moved, an utterance nothing moved) is the kernel's; everything after that is float64."""
import numpy as np

PLANES = ("linf", "l1_mean", "l2", "energy", "snr_db", "seg_snr_db")
SEGMENT = 256
SEG_LO_DB, SEG_HI_DB = -10.0, 35.0


def difference(x, adv):
    """adv - x in float32, one rounding per sample."""
    return np.asarray(adv, dtype=np.float32) - np.asarray(x, dtype=np.float32)


def ratio_db(ex, ed):
    """10 log10(ex / ed): +inf for ed == 0 < ex, -inf for ex == 0 < ed, NaN for 0 / 0 and for NaN."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return 10.0 * np.log10(np.asarray(ex, dtype=np.float64) / np.asarray(ed, dtype=np.float64))


def segment_terms(x, d):
    """(B, S) clamped segment SNRs over the S = T // 256 full segments."""
    x, d = np.asarray(x, dtype=np.float64), np.asarray(d, dtype=np.float64)
    B, T = x.shape
    S = T // SEGMENT
    ex = (x[:, :S * SEGMENT].reshape(B, S, SEGMENT) ** 2).sum(axis=2)
    ed = (d[:, :S * SEGMENT].reshape(B, S, SEGMENT) ** 2).sum(axis=2)
    with np.errstate(invalid="ignore"):
        clamped = np.clip(ratio_db(ex, ed), SEG_LO_DB, SEG_HI_DB)     # NaN stays NaN
    return np.where(ed == 0.0, SEG_HI_DB, clamped)                    # nothing moved: 35, also in silence


def perturb_ref(x, d):
    """x (B, T), d (B, T) = difference(x, adv)  ->  (6, B) float64 in the order of PLANES."""
    d = np.asarray(d)
    assert d.dtype == np.float32, "d is the float32 difference (difference(x, adv))"
    x, d = np.asarray(x, dtype=np.float32).astype(np.float64), d.astype(np.float64)
    B, T = x.shape
    out = np.full((6, B), np.nan)
    ex, ed = (x ** 2).sum(axis=1), (d ** 2).sum(axis=1)
    out[0] = np.abs(d).max(axis=1) if T else 0.0                       # np.max propagates NaN
    with np.errstate(invalid="ignore"):
        out[1] = np.abs(d).sum(axis=1) / np.float64(T) if T else np.nan
    out[2] = np.sqrt(ed)
    out[3] = ex
    out[4] = ratio_db(ex, ed)
    if T // SEGMENT:
        out[5] = segment_terms(x, d).mean(axis=1)
    return out
