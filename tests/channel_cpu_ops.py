"""TEST INFRASTRUCTURE — the channel entry points of hip_ops (channel_apply, channel_adjoint, channel_eot_step;
include/advstep_channel.h) restated on the CPU in numpy float32 WITH THE KERNELS' OPERATION ORDER, and the noise restated with
tests.apgd_cpu_ops' Philox; every other op is tests.radius_cpu_ops' (whose LinearDetector the end-to-end tests run on).  Inputs may
live on any device; results go back to the input's device, so the table can stand in for hip_ops inside torchattacks.EOTPGD.

Everything in the three kernels is an exact-order float32 computation: x - c rounds once, every tap is one rounded product and one
rounded sum in tap order from +0, the gain, the centre and the noise are one rounding each, the draws are summed in draw order
from +0, and the move is the three roundings of the PGD L-inf step.  numpy float32 arithmetic rounds each of these the same way, so
the GPU tests compare BYTES with this table, with no tolerance."""
import numpy as np
import torch

from tests import radius_cpu_ops as _base
from tests.apgd_cpu_ops import _c, _emit, _u01, philox4x32_10
from tests.radius_cpu_ops import LinearDetector  # noqa: F401  (re-exported)
from tests.spsa_cpu_ops import pgd_linf_step_np

NAME = "channel_cpu"
MAX_TAPS, MAX_DRAWS = 256, 64      # ADVSTEP_CHANNEL_MAX_TAPS, ADVSTEP_CHANNEL_MAX_DRAWS of include/advstep_channel.h


def __getattr__(name):  # every op this table does not restate
    return getattr(_base, name)


def channel_noise(B, T, seed, offset=0):
    """(B, T) float32 in [-1, 1): n[b, t] = 2 u01(R.v[t & 3]) - 1, R = philox4x32_10(lo32(t >> 2), b, lo32(O), hi32(O), lo32(seed),
    hi32(seed)) with O = offset (the caller adds the draw's index)."""
    O = int(offset) & 0xFFFFFFFFFFFFFFFF
    Q = (T + 3) // 4
    q, b = np.meshgrid(np.arange(Q, dtype=np.uint32), np.arange(B, dtype=np.uint32))
    r = philox4x32_10(q, b, np.full(q.shape, O & 0xFFFFFFFF, np.uint32), np.full(q.shape, O >> 32, np.uint32),
                      seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    u = np.stack([_u01(w) for w in r], axis=-1).reshape(B, Q * 4)[:, :T]
    return (np.float32(2.0) * u - np.float32(1.0)).astype(np.float32)


def _gather(row, idx):
    """row[idx] where 0 <= idx < len(row), 0 elsewhere; idx int64."""
    ok = (idx >= 0) & (idx < row.shape[0])
    return np.where(ok, row[np.where(ok, idx, 0)], np.float32(0.0)).astype(np.float32)


def _fir(row, h, first):
    """acc[t] = sum_i, in order from +0, of h[i] * row[first(t, i)] (0 outside the row)."""
    T = row.shape[0]
    t = np.arange(T, dtype=np.int64)
    acc = np.zeros(T, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(h.shape[0]):
            acc = (acc + (h[i] * _gather(row, first(t, i))).astype(np.float32)).astype(np.float32)
    return acc


def channel_apply_np(x, center, taps, shift, gain, noise, seed, offset=0):
    """(K, B, T) float32 from x (B, T), center (B), taps (K, B, L), shift (K, B) integers, gain and noise (K, B)."""
    B, T = x.shape
    K = taps.shape[0]
    out = np.empty((K, B, T), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(K):
            n = channel_noise(B, T, seed, int(offset) + j)
            for b in range(B):
                c, s = np.float32(center[b]), int(shift[j, b])
                acc = _fir((x[b] - c).astype(np.float32), taps[j, b], lambda t, i: t - s - i)
                y = (c + (np.float32(gain[j, b]) * acc).astype(np.float32)).astype(np.float32)
                out[j, b] = (y + (np.float32(noise[j, b]) * n[b]).astype(np.float32)).astype(np.float32)
    return out


def channel_adjoint_np(grads, taps, shift, gain):
    """(B, T) float32 from grads (K, B, T)."""
    K, B, T = grads.shape
    G = np.zeros((B, T), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(K):
            for b in range(B):
                s = int(shift[j, b])
                acc = _fir(grads[j, b], taps[j, b], lambda u, i: u + s + i)
                G[b] = (G[b] + (np.float32(gain[j, b]) * acc).astype(np.float32)).astype(np.float32)
    return G


def channel_eot_step_np(adv, orig, grads, taps, shift, gain, alpha, eps, lo=0.0, hi=1.0):
    with np.errstate(invalid="ignore"):
        return pgd_linf_step_np(adv, channel_adjoint_np(grads, taps, shift, gain), orig, alpha, eps, lo, hi)


# ---- the table's ops -----------------------------------------------------------------------------------------------------------------

def _np2(t):
    a = _c(t).numpy()
    return a.reshape(a.shape[0], -1)


def _np3(t):
    a = _c(t).numpy()
    return a.reshape(a.shape[0], a.shape[1], -1)


def _params(taps, shift, gain):
    return _c(taps).numpy(), _c(shift).numpy().astype(np.int64), _c(gain).numpy()


def channel_apply(x, center, taps, shift, gain, noise, seed, offset=0, out=None):
    res = torch.from_numpy(channel_apply_np(_np2(x), _c(center).numpy().reshape(-1), *_params(taps, shift, gain), _c(noise).numpy(),
                                            seed, offset))
    if out is not None:
        with torch.no_grad():
            out.copy_(res.reshape(out.shape).to(out.device))
        return out
    return res.reshape((taps.shape[0],) + tuple(x.shape)).to(x.device)


def channel_adjoint(grads, taps, shift, gain, out=None):
    return _emit(torch.from_numpy(channel_adjoint_np(_np3(grads), *_params(taps, shift, gain))), grads[0], out)


def channel_eot_step(adv, orig, grads, taps, shift, gain, alpha, eps, lo=0.0, hi=1.0, out=None):
    res = channel_eot_step_np(_np2(adv), _np2(orig), _np3(grads), *_params(taps, shift, gain), alpha, eps, lo, hi)
    return _emit(torch.from_numpy(res), adv, out)
