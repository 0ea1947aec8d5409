"""TEST INFRASTRUCTURE — the l1-APGD entry points of hip_ops (include/advstep_apgdl1.h) restated in float32 torch eager on the
CPU with a sort: torch.sort for the top-k threshold, a bisection over the 31 bits of lambda for the projection (the same
definition as the kernels', with torch's own float32 row sum as phi).  apgd_eval / apgd_track and every other op are
tests/apgd_cpu_ops.py's.  Inputs may live on any device; results go back to the input's device, into `out` / the state
tensors when given, so the table can stand in for hip_ops inside the attack and can recompute a GPU launch from its inputs."""
import torch

from tests import apgd_cpu_ops as _base
from tests.apgd_cpu_ops import _c, _emit, apgd_eval, apgd_track, philox_draw  # noqa: F401  (re-exported)

NAME = "apgdl1_cpu"


def __getattr__(name):  # every op this table does not restate
    return getattr(_base, name)


def _f32(v):
    return torch.tensor(v, dtype=torch.float32)


def _moves(ad, cap, lam):
    """m_i(lam) = min(max(|d_i| - lam, 0), cap_i); lam (B, 1)."""
    return torch.minimum(torch.clamp(ad - lam, min=0.0), cap)


def project(xc, uc, eps):
    """P(u; x, eps) of include/advstep_apgdl1.h on CPU float32 rows: lambda* = the smallest non-negative float32 with
    phi(lambda*) <= eps, found one bit at a time (31 evaluations of phi); phi is torch's float32 row sum."""
    d = uc - xc
    ad, cap = d.abs(), torch.where(d > 0, 1.0 - xc, xc)
    B = xc.shape[0]
    e = _f32(eps)
    infeasible = _moves(ad, cap, torch.zeros(B, 1)).sum(dim=1) > e
    rho = torch.zeros(B, dtype=torch.int32)                    # the largest float32 pattern with phi > eps
    for bit in range(30, -1, -1):
        cand = rho | (1 << bit)
        over = _moves(ad, cap, cand.view(torch.float32)[:, None]).sum(dim=1) > e
        rho = torch.where(over, cand, rho)
    lam = torch.where(infeasible, (rho + 1).view(torch.float32), torch.zeros(B))
    return (xc + torch.sign(d) * _moves(ad, cap, lam[:, None])).clamp(0.0, 1.0)


def l1_box_project(x, u, eps, out=None):
    B = x.shape[0]
    return _emit(project(_c(x).reshape(B, -1), _c(u).reshape(B, -1), eps), u, out)


def apgdl1_init(x, eps, draw=None, seed=None, offset=0, out=None):
    xc = _c(x)
    B = xc.shape[0]
    xc = xc.reshape(B, -1)
    t = _c(draw).reshape(B, -1) if draw is not None else philox_draw(B, xc.shape[1], "L2", seed, offset)
    return _emit(project(xc, xc + t, eps), x, out)


def topk_threshold(g, topk):
    """(n, thr, s, cnt) of the step for CPU rows g (B, T) and fractions topk (B)."""
    T = g.shape[1]
    n = ((1 - topk) * T).clamp(0, T - 1).long()
    thr = g.abs().sort(dim=1)[0].gather(1, n[:, None])         # ascending, NaN last
    s = torch.where(g.abs() >= thr, torch.sign(g), torch.zeros_like(g))
    s = torch.where(torch.isnan(g), torch.zeros_like(g), s)
    return n, thr.reshape(-1), s, s.abs().sum(dim=1)


def apgdl1_step(cur, grad, x, step_size, topk, eps, out=None, return_stats=False):
    c, g, xc = _c(cur), _c(grad), _c(x)
    B = c.shape[0]
    c, g, xc = c.reshape(B, -1), g.reshape(B, -1), xc.reshape(B, -1)
    _, thr, s, cnt = topk_threshold(g, _c(topk).reshape(-1))
    u = c + _c(step_size).reshape(-1, 1) * s / (cnt[:, None] + 1e-10)
    res = _emit(project(xc, u, eps), cur, out)
    if return_stats:
        return res, torch.stack([thr, cnt], 1).to(cur.device)
    return res


def apgdl1_checkpoint(cur, x_best, x, state, eps):
    f = _c(state.flags)
    c, xb, xc = _c(cur), _c(x_best), _c(x)
    B = c.shape[0]
    c, xb, xc = c.reshape(B, -1), xb.reshape(B, -1), xc.reshape(B, -1)
    T = c.shape[1]
    best = torch.where(((f & 2) != 0)[:, None], c, xb)
    sp = ((best - xc) != 0).sum(dim=1).to(torch.float32)
    red = (sp / _c(state.sp_old)) < _f32(0.95)
    e = _f32(eps)
    step = torch.where(red, e, _c(state.step_size) / 1.5)
    step = torch.minimum(torch.maximum(step, e / 10.0), e)
    state.topk.copy_((sp / float(T) / 1.5).to(state.topk.device))
    state.step_size.copy_(step.to(state.step_size.device))
    state.sp_old.copy_(sp.to(state.sp_old.device))
    state.flags.copy_(((f & 0xFB) | (red.to(torch.uint8) << 2)).to(state.flags.device))
