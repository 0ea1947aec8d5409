"""TEST INFRASTRUCTURE — the universal-perturbation entry points of hip_ops (universal_colsum, universal_apply;
include/advstep_universal.h) restated on the CPU in float64 from the float32 operands, and the bounds the tests hold the kernels
to; every other op is tests.radius_cpu_ops' (whose LinearDetector the closed-form tests run on).  The table's two ops are the
float64 restatement rounded ONCE to float32, so the table can stand in for hip_ops inside UniversalPGD; the `_ref64` forms return
float64.  Inputs may live on any device.

THE BOUNDS (u = 2^-24; no constant here was measured).

Column sum.  The kernel forms p_b = fl(w_b g_bt), |p_b - w_b g_bt| <= u |w_b g_bt| (w_b g_bt itself is exact in float64: two
24-bit significands), and adds the B values p_b in SOME order, interleaved with additions of an exact 0 (a partial's and the
fold's start), which round nothing.  Any order of adding B numbers is a binary tree with B - 1 rounded additions, and a term
passes through at most B - 1 of them, so to first order
    |out - sum_b p_b| <= (B - 1) u sum_b |p_b|,   and with the products   |out - out64| <= B u sum_b |w_b g_bt|.
The second-order remainder is below (B u)^2 / 2 of the same sum — at B = 33 that is 6e-11 of it, against the u = 6e-8 that
    colsum_tolerance = (B + 1) u sum_b |w_b g_bt|
leaves for it.  The bound holds for every summation order, so it does not pin the kernel's grouping.  (The test's operands are
of normal size: no product underflows.)

Broadcast.  out = clamp(fl(x + fl(w delta))) rounds twice, exactly like float32 `torch.clamp(x + w[:, None] * delta, lo, hi)` on
the CPU (a multiplication and an addition, neither fused): the GPU test asks for the same bits, no tolerance.  The float64
restatement below is what the CPU table rounds once; it differs from the kernel by at most u |w delta| + u |x + w delta|.

On the linear detector (z = x . w + bias, accumulated in float64) a row of the source class that no clamp touches moves by
exactly delta, rounded once per sample, so  z(adv) - z(x) = delta . w  within  u sum_t |w_t| |adv_t|  (`logit_tolerance`, plus
the one rounding of the float32 logit itself)."""
import torch

from tests import radius_cpu_ops as _base
from tests.apgd_cpu_ops import _c, _emit
from tests.radius_cpu_ops import LinearDetector, U, norm_rel_bound  # noqa: F401  (re-exported)

NAME = "universal_cpu"
GROUP_ROWS = 16       # ADVSTEP_UNIVERSAL_GROUP_ROWS of include/advstep_universal.h


def __getattr__(name):  # every op this table does not restate
    return getattr(_base, name)


def _weights64(row_weight, B):
    if row_weight is None:
        return torch.ones(B, 1, dtype=torch.float64)
    return _c(row_weight).double().reshape(B, 1)


def universal_colsum_ref64(grad, row_weight=None, parts=False):
    """(T,) float64: sum_b w_b g_bt from the float32 operands; with parts also sum_b |w_b g_bt|.  0 * NaN = NaN, as written."""
    g = _c(grad).double()
    g = g.reshape(g.shape[0], -1)
    p = _weights64(row_weight, g.shape[0]) * g
    return (p.sum(0), p.abs().sum(0)) if parts else p.sum(0)


def universal_apply_ref64(x, delta, row_weight=None, lo=0.0, hi=1.0):
    """x's shape, float64: clamp(x + w_b delta_t, lo, hi)."""
    x64 = _c(x).double()
    B = x64.shape[0]
    moved = x64.reshape(B, -1) + _weights64(row_weight, B) * _c(delta).double().reshape(1, -1)
    return torch.clamp(moved, min=lo, max=hi).reshape(x64.shape)


def universal_apply_f32(x, delta, row_weight=None, lo=0.0, hi=1.0):
    """The kernel's own two roundings in float32 eager on the CPU: the reference of the GPU test's bit comparison."""
    xc = _c(x)
    B = xc.shape[0]
    w = torch.ones(B, 1) if row_weight is None else _c(row_weight).reshape(B, 1)
    return torch.clamp(xc.reshape(B, -1) + w * _c(delta).reshape(1, -1), lo, hi).reshape(xc.shape)


# ---- the table's ops: the restatement, rounded once ------------------------------------------------------------------------------

def universal_colsum(grad, row_weight=None, out=None):
    res = universal_colsum_ref64(grad, row_weight).float().reshape(1, -1)
    if out is not None:
        with torch.no_grad():
            out.copy_(res.reshape(out.shape).to(out.device))
        return out
    return res.to(grad.device)


def universal_apply(x, delta, row_weight=None, lo=0.0, hi=1.0, out=None):
    return _emit(universal_apply_ref64(x, delta, row_weight, lo, hi).float(), x, out)


# ---- bounds (derived in the module docstring) ------------------------------------------------------------------------------------

def colsum_tolerance(B, abs_sum):
    return (B + 1) * U * abs_sum


def logit_tolerance(w, adv, z):
    """Of z(adv) on the LinearDetector against its exact value: the samples' one rounding and the float32 logit's."""
    return U * (_c(adv).double().abs() @ _c(w).double().abs()) + U * z.abs()
