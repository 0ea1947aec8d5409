"""The frequency-masking threshold of a clean utterance (no counterpart in the reference tree).

A perturbation whose short-time power spectrum stays under the masking threshold of the speech it is added to is masked by
that speech (Qin et al., ICML 2019; Schoenherr et al., NDSS 2019).  `MaskingModel.threshold(x)` builds that threshold once per
batch with torch ops — it is not on the hot path; the kernels of include/advstep_masking.h take it as data:

    z(f)      = 13 atan(0.00076 f) + 3.5 atan((f / 7500)^2)                       the Bark scale, at f_k = k sr / 512
    ATH_dB(f) = 3.64 (f/1000)^-0.8 - 6.5 exp(-0.6 (f/1000 - 3.3)^2) + 1e-3 (f/1000)^4,  f >= 20 Hz    Terhardt's threshold in quiet
    ath_rel_k = 10^((ATH_dB(f_k) - 96) / 10)                                     anchored as Qin et al. do: loudest cell = 96 dB
    SF_dB(d)  = 15.81 + 7.5 (d + 0.474) - 17.5 sqrt(1 + (d + 0.474)^2)           Schroeder's spreading function
    M[k, j]   = 10^((SF_dB(z_k - z_j) - 14.5 - z_j) / 10) / n_k,   n_k = #{i : |z_i - z_k| < 0.5}
    P_x       = |STFT(x)|^2 with bins 0 and 1 zeroed (the offset of the min-max domain lives there)
    ref_b     = max_{f, k} P_x  (clamped away from 0)
    theta     = ref_b max(ath_rel, (P_x / ref_b) M^T)
    s_b       = 1 / (ref_b NF 257)

Everything is relative to the utterance's own loudest cell, so the threshold is the same in the attack's normalised domain and
in the waveform's.  A DEPARTURE from Qin et al.: every bin of the clean spectrum acts as a masker with the tonal offset (dense
spreading); their tonal / noise masker selection is not done.  Nobody has measured either against listeners."""
from __future__ import annotations

import torch

N_FFT, BINS = 512, 257
_TINY = 1e-30


def bark(f: torch.Tensor) -> torch.Tensor:
    return 13.0 * torch.atan(0.00076 * f) + 3.5 * torch.atan((f / 7500.0) ** 2)


def ath_db(f: torch.Tensor) -> torch.Tensor:
    k = torch.clamp(f, min=20.0) / 1000.0
    return 3.64 * k ** -0.8 - 6.5 * torch.exp(-0.6 * (k - 3.3) ** 2) + 1e-3 * k ** 4


def spreading_db(d: torch.Tensor) -> torch.Tensor:
    return 15.81 + 7.5 * (d + 0.474) - 17.5 * torch.sqrt(1.0 + (d + 0.474) ** 2)


def tables(sr: int = 16000, dtype=torch.float64):
    """(z (257), ath_rel (257), M (257, 257), n (257)) in `dtype` on the CPU."""
    f = torch.arange(BINS, dtype=dtype) * (sr / N_FFT)
    z = bark(f)
    ath_rel = 10.0 ** ((ath_db(f) - 96.0) / 10.0)
    n = ((z[None, :] - z[:, None]).abs() < 0.5).sum(dim=1).to(dtype)
    M = 10.0 ** ((spreading_db(z[:, None] - z[None, :]) - 14.5 - z[None, :]) / 10.0) / n[:, None]
    return z, ath_rel, M, n


class MaskingModel:
    """The tables above for one sample rate and hop, and `threshold(x)`.  Tables are built in float64 on the CPU and kept as
    float32 per device."""

    def __init__(self, sr: int = 16000, hop: int = 128):
        if not 128 <= int(hop) <= N_FFT:
            raise ValueError(f"hop must lie in [128, {N_FFT}] (the kernels' framing), got {hop!r}")
        self.sr, self.hop = int(sr), int(hop)
        _, ath_rel, M, _ = tables(self.sr)
        self._cpu = (torch.hann_window(N_FFT, periodic=True, dtype=torch.float64).float(), ath_rel.float(),
                     M.float().t().contiguous())
        self._dev = {}

    def on(self, device):
        """(window (512), ath_rel (257), M^T (257, 257)) as float32 on `device`."""
        key = str(device)
        if key not in self._dev:
            self._dev[key] = tuple(t.to(device) for t in self._cpu)
        return self._dev[key]

    def window(self, device) -> torch.Tensor:
        return self.on(device)[0]

    def frames(self, T: int) -> int:
        return 1 + int(T) // self.hop

    def threshold(self, x: torch.Tensor, ops=None):
        """x (B, T) float32 on a HIP device -> (theta (B, NF, 257), s (B)), both float32 on x's device.  No host read."""
        if ops is None:
            from .. import hip_ops as ops
        window, ath_rel, Mt = self.on(x.device)
        B = x.shape[0]
        P = ops.stft_power(x.reshape(B, -1).contiguous(), None, window, self.hop)
        P[:, :, :2] = 0.0
        ref = P.amax(dim=(1, 2)).clamp_min(_TINY)
        theta = torch.maximum(ath_rel, (P / ref[:, None, None]) @ Mt) * ref[:, None, None]
        s = 1.0 / (ref * float(P.shape[1] * BINS))
        return theta.contiguous(), s.contiguous()


def worst_db(worst: torch.Tensor) -> torch.Tensor:
    """10 log10 of the stats' third column."""
    return 10.0 * torch.log10(worst)


__all__ = ["MaskingModel", "tables", "bark", "ath_db", "spreading_db", "worst_db", "N_FFT", "BINS"]
