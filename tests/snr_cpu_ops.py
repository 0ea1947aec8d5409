"""TEST INFRASTRUCTURE — the SNR-budget entry points of hip_ops (seg_pgd_step, snr_row_radius; include/advstep_snr.h) restated
on the CPU in float64 from the float32 operands, and the bounds the tests hold the kernels to; every other op is
tests.radius_cpu_ops' (whose LinearDetector the closed-form tests run on).  The table's two ops are the float64 restatement
rounded ONCE to float32, so the table can stand in for hip_ops inside PGDSNR; the `_ref64` forms return float64 and the
intermediate quantities a tolerance is scaled to.  Inputs may live on any device.

THE BOUNDS (first order in u = 2^-24; every operation is correctly rounded, sqrtf and the division included; no constant here
was measured).  A segment sum is a thread's (p + q) + (r + s) and 6 shuffle levels: 8 additions deep over squares that round
once, so a sum of squares of exact operands is within 9u, relatively, and its square root within 5.5u.  Per segment, relative:
    x + c           1        (x + c)^2      3        e_x           11       sqrtf         6.5      r = rho * .    7.5
    sum g^2         9        sqrtf          5.5      gn = . + eps_div       6.5
    a = alpha_rel r 8.5      g / gn         7.5      s = a (g / gn)         17
With M_t = |adv_t| + |s_t| + |x_t| (the cancellation in d makes every later error absolute, on this scale):
    d = (adv + s) - x          |err| <= 17u|s| + u(|adv| + |s|) + u|d|                         <= 19u M_t
    dn = sqrtf(sum d^2)        |err| <= 5.5u dn + 19u ||M||_seg                                 <= 24.5u ||M||_seg
    f = min((1 / dn) r, 1)     relative err(dn) / dn + 9.5u where f < 1 (min is 1-Lipschitz), exact where both sides take 1
    p = d f                    |err| <= 19u M_t + |d_t| f (err(dn) / dn + 9.5u) + u |d_t| f     <= 29.5u M_t + 24.5u ||M||_seg
                               (|d_t| <= dn and f <= 1 bound |d_t| f err(dn) / dn by err(dn))
    out = clamp(x + p)         + u |x + p| <= 2u M_t; the clamp is 1-Lipschitz
so  |out - out64| <= (32 M_t + 25 ||M||_seg) u                                                 (step_tolerance)

The budget, recomputed in float64 from the kernel's float32 output: |p_t| <= |d_t| (r / dn)(1 + 3u) in the kernel's own
numbers, its dn is within 5.5u of the norm of its own d, its r within 7.5u of r64: ||p|| <= r64 (1 + 16u).  x + p then rounds
onto float32's grid, |err| <= u (1 + |p_t|) for x in [0, 1], and the clamp moves a sample towards x:
    ||out - x||_seg <= r64 (1 + (16 + sqrt(n)) u) + u sqrt(n),   n = the segment's in-row samples        (seg_ball_bound)
which is  sum (out - x)^2 <= rho^2 sum (x + c)^2 (1 + k u)  with k = 2 (16 + sqrt(n) (1 + 1 / r64)): the absolute term is the
grid of the output, not the kernel's arithmetic, and it is what is left of the inequality in a quiet segment.

The global radii: the row sum's chain has radius_cpu_ops.chain(T) additions over squares of x + c (3u each):
    |e - e64| <= ((chain + 3) / 2 + 2) u e64                                                     (radius_rel_bound)"""
import math

import numpy as np
import torch

from tests import radius_cpu_ops as _base
from tests.apgd_cpu_ops import _c, _emit
from tests.radius_cpu_ops import LinearDetector, U, chain  # noqa: F401  (re-exported)

NAME = "snr_cpu"
SEGMENT = 256


def __getattr__(name):  # every op this table does not restate
    return getattr(_base, name)


def _f32(v):
    """A launch scalar as the float32 the library receives, in double."""
    return float(np.float32(v))


def rho_of(snr_db):
    return 10.0 ** (-float(snr_db) / 20.0)


def segments(t, fill=0.0):
    """(B, T) -> (B, S, 256), S = ceil(T / 256); the last segment is padded with `fill`."""
    B, T = t.shape
    S = -(-T // SEGMENT)
    return torch.nn.functional.pad(t, (0, S * SEGMENT - T), value=fill).reshape(B, S, SEGMENT)


def _offset64(offset_rows, B):
    if offset_rows is None:
        return torch.zeros(B, 1, dtype=torch.float64)
    return _c(offset_rows).double().reshape(B, 1)


def segment_radii_ref64(orig, offset_rows, rho):
    """(B, S) float64: rho * sqrt(sum (x + c)^2) over each segment's in-row samples."""
    x = _c(orig).double()
    sig = segments(x + _offset64(offset_rows, x.shape[0])) * segments(torch.ones_like(x))
    return _f32(rho) * (sig * sig).sum(-1).sqrt()


def seg_pgd_step_ref64(adv, grad, orig, offset_rows, rho, alpha_rel, eps_div, lo=0.0, hi=1.0, parts=False):
    """The segmental step in float64 from the float32 operands: (B, T) float64; with parts also M = |adv| + |s| + |x| (B, T),
    its norm per segment broadcast to the samples (B, T), and the segments' radii (B, S)."""
    a, g, x = _c(adv).double(), _c(grad).double(), _c(orig).double()
    B, T = a.shape
    mask = segments(torch.ones_like(x))
    r = segment_radii_ref64(orig, offset_rows, rho).unsqueeze(-1)
    a_s, g_s, x_s = segments(a), segments(g), segments(x)
    gn = (g_s * g_s).sum(-1, keepdim=True).sqrt() + _f32(eps_div)
    s = (_f32(alpha_rel) * r) * (g_s / gn)
    d = ((a_s + s) - x_s) * mask
    d = torch.where(mask > 0, d, torch.zeros_like(d))                  # a NaN norm must not leak through 0 * NaN
    dn = (d * d).sum(-1, keepdim=True).sqrt()
    one = torch.ones_like(dn)
    f = torch.where(dn == 0, one, torch.minimum(r / torch.where(dn == 0, one, dn), one))
    out = torch.clamp(x_s + d * f, min=lo, max=hi).reshape(B, -1)[:, :T]
    if not parts:
        return out
    M = (a_s.abs() + s.abs() + x_s.abs()) * mask
    Mn = (M * M).sum(-1, keepdim=True).sqrt().expand_as(M)
    return out, M.reshape(B, -1)[:, :T], Mn.reshape(B, -1)[:, :T], r.squeeze(-1)


def snr_row_radius_ref64(x, offset_rows, rho):
    """(B,) float64: rho * sqrt(sum_t (x + c)^2)."""
    x64 = _c(x).double()
    sig = x64.reshape(x64.shape[0], -1) + _offset64(offset_rows, x64.shape[0])
    return _f32(rho) * (sig * sig).sum(-1).sqrt()


# ---- the table's ops: the restatement, rounded once ------------------------------------------------------------------------------

def seg_pgd_step(adv, grad, orig, offset_rows, rho, alpha_rel, eps_div, lo=0.0, hi=1.0, out=None):
    return _emit(seg_pgd_step_ref64(adv, grad, orig, offset_rows, rho, alpha_rel, eps_div, lo, hi).float(), adv, out)


def snr_row_radius(x, offset_rows, rho, out=None):
    res = snr_row_radius_ref64(x, offset_rows, rho).float()
    if out is not None:
        with torch.no_grad():
            out.copy_(res.to(out.device))
        return out
    return res.to(x.device)


def row_pgd_l2_step(adv, grad, orig, eps_rows, alpha_abs, alpha_rel, eps_div=1e-10, lo=0.0, hi=1.0, out=None):
    """radius_cpu_ops' L2 step in float64 (the global mode's step), rounded once."""
    a, g, x = _c(adv).double(), _c(grad).double(), _c(orig).double()
    B = a.shape[0]
    e = _c(eps_rows).double().reshape(B, 1)
    al = _f32(alpha_abs) + _f32(alpha_rel) * e
    gn = (g * g).sum(-1, keepdim=True).sqrt() + _f32(eps_div)
    d = (a + al * (g / gn)) - x
    dn = (d * d).sum(-1, keepdim=True).sqrt()
    one = torch.ones_like(dn)
    f = torch.where(dn == 0, one, torch.minimum(e / torch.where(dn == 0, one, dn), one))
    return _emit(torch.clamp(x + d * f, min=lo, max=hi).float(), adv, out)


# ---- bounds (derived in the module docstring) ------------------------------------------------------------------------------------

def step_tolerance(M, M_seg):
    return (32.0 * M + 25.0 * M_seg) * U


def seg_ball_bound(r, n):
    """||out - x||_2 over a segment of n in-row samples at radius r (float64 tensors or numbers)."""
    return r * (1.0 + (16.0 + n ** 0.5) * U) + U * n ** 0.5


def radius_rel_bound(T):
    return ((chain(T) + 3) / 2 + 2) * U


def segment_sizes(T):
    """(S,) float64: in-row samples per segment."""
    return segments(torch.ones(1, T, dtype=torch.float64)).sum(-1).reshape(-1)
