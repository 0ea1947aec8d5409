"""TEST INFRASTRUCTURE — the L0 entry points of hip_ops (include/advstep_l0.h) restated in float32 torch eager on the CPU with a
stable sort: `torch.sort(stable=True, descending=True)` of the scores, the first min(k, T) indices kept.  The step takes an
optional `gnorm=` (B) so that a test can hand it the device's own row sum of |grad|: with that, u is elementwise IEEE
arithmetic and the selection is exact, so device and table agree bit for bit.  Every other op is tests/apgd_cpu_ops.py's.
Inputs may live on any device; results go back to the input's device, into `out` when given, so the table can stand in for
hip_ops inside the attack and can recompute a GPU launch from its inputs."""
import math

import torch

from tests import apgd_cpu_ops as _base
from tests.apgd_cpu_ops import _c, _emit

NAME = "l0_cpu"


def __getattr__(name):  # every op this table does not restate
    return getattr(_base, name)


def scores(xc, uc, eps_inf=math.inf):
    """(c, s) of include/advstep_l0.h for CPU rows, expression by expression (torch eager rounds every op: no contraction)."""
    cap = torch.tensor(eps_inf, dtype=xc.dtype)
    d = uc - xc
    lb, ub = torch.maximum(-xc, -cap), torch.minimum(1.0 - xc, cap)
    c = torch.minimum(torch.maximum(d, lb), ub)
    r = d - c
    return c, d * d - r * r


def kept_mask(s, k):
    """The first min(k, T) indices of a stable descending sort of the scores s (B, T), as a mask, and the sort's order."""
    B, T = s.shape
    order = torch.sort(s, dim=1, descending=True, stable=True)[1]
    keep = torch.zeros(B, T, dtype=torch.bool)
    keep.scatter_(1, order[:, :min(int(k), T)], True)
    return keep, order


def project(xc, uc, k, eps_inf=math.inf, return_stats=False):
    """P0(u; x, k, eps_inf) on CPU rows (B, T); return_stats: also (thr, gt, cut) per row in the rows' dtype."""
    B, T = xc.shape
    kk = min(int(k), T)
    c, s = scores(xc, uc, eps_inf)
    keep, order = kept_mask(s, k)
    res = torch.where(keep, (xc + c).clamp(0.0, 1.0), xc)
    if not return_stats:
        return res
    thr = s.gather(1, order[:, kk - 1:kk])                          # the kk-th largest score
    gt = (s > thr).sum(dim=1).to(xc.dtype)
    idx = torch.arange(T).expand(B, T)
    cut = torch.where(keep & (s == thr), idx, torch.full_like(idx, -1)).max(dim=1)[0].to(xc.dtype)
    return res, thr.reshape(-1), gt, cut


def l0_box_project(x, u, k, eps_inf=math.inf, out=None):
    B = x.shape[0]
    return _emit(project(_c(x).reshape(B, -1), _c(u).reshape(B, -1), k, eps_inf), u, out)


def step_point(c, g, step, gn):
    """u = cur + (step * g) / (gnorm + 1e-10) on CPU rows, gn (B)."""
    return c + (torch.tensor(step, dtype=c.dtype) * g) / (gn[:, None] + torch.tensor(1e-10, dtype=c.dtype))


def pgdl0_step(cur, grad, x, step, k, eps_inf=math.inf, out=None, return_stats=False, gnorm=None):
    c, g, xc = _c(cur), _c(grad), _c(x)
    B = c.shape[0]
    c, g, xc = c.reshape(B, -1), g.reshape(B, -1), xc.reshape(B, -1)
    gn = g.abs().sum(dim=1) if gnorm is None else _c(gnorm).reshape(B).to(c.dtype)
    u = step_point(c, g, step, gn)
    res, thr, gt, cut = project(xc, u, k, eps_inf, return_stats=True)
    res = _emit(res, cur, out)
    if return_stats:
        return res, torch.stack([gn, thr, gt, cut], 1).to(cur.device)
    return res
