"""TEST INFRASTRUCTURE — the momentum entry points of hip_ops (mi_step, vt_*) restated in float32 torch eager on the CPU,
expression by expression (include/advstep_momentum.h); every other op is oracle.torch_ops'.  Inputs may live on any device:
they are copied to the CPU, and results go back to the input's device (into `out` / `momentum` / `nes_out` / `gv` when given),
so the table can stand in for hip_ops inside the attacks and can recompute a GPU launch from its own inputs."""
import numpy as np
import torch

from oracle import torch_ops as _base
from tests.apgd_cpu_ops import _c, _emit, _u01, philox4x32_10

NAME = "momentum_cpu"


def __getattr__(name):  # every op this table does not restate
    return getattr(_base, name)


def philox_uniform(n: int, bound: float, seed: int, offset: int = 0) -> torch.Tensor:
    """The n draws advstep_vt_neighbor_philox_f32 regenerates: the flat uniform stream of pgd_linf_init_philox (counter =
    (flat index / 4, offset)), scaled as Tensor.uniform_(-bound, bound) does: u * (bound - (-bound)) + (-bound)."""
    s_lo, s_hi = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    o_lo, o_hi = offset & 0xFFFFFFFF, (offset >> 32) & 0xFFFFFFFF
    i = np.arange(n, dtype=np.uint64)
    q = i >> np.uint64(2)
    r = philox4x32_10((q & np.uint64(0xFFFFFFFF)).astype(np.uint32), (q >> np.uint64(32)).astype(np.uint32),
                      np.full(q.shape, o_lo, np.uint32), np.full(q.shape, o_hi, np.uint32), s_lo, s_hi)
    u = _u01(np.choose((i & np.uint64(3)).astype(np.int64), r))
    lo = np.float32(-np.float32(bound))
    rng = np.float32(np.float32(bound) - lo)
    return torch.from_numpy((u * rng).astype(np.float32) + lo)


def mi_tail(adv, orig, m_new, alpha, eps, lo=0.0, hi=1.0, nes_scale=None):
    """The last four lines of the update, which have no re-association: out (and nes when nes_scale is given) from m'."""
    x1 = adv + alpha * m_new.sign()
    delta = torch.clamp(x1 - orig, min=-eps, max=eps)
    out = torch.clamp(orig + delta, min=lo, max=hi)
    return out if nes_scale is None else (out, out + nes_scale * m_new)


def mi_step(adv, grad, orig, momentum, alpha, eps, decay, v=None, nes_out=None, nes_scale=0.0, lo=0.0, hi=1.0, out=None,
            return_mean=False):
    """mifgsm.py:70-76 (nifgsm.py:67-71, vmifgsm.py:77-79, 99-101) on (B, T) rows; `momentum` is updated in place."""
    a_c, g, x, m = _c(adv), _c(grad), _c(orig), _c(momentum)
    B = a_c.shape[0]
    a = g if v is None else g + _c(v)
    mu = torch.mean(torch.abs(a.reshape(B, -1)), dim=1, keepdim=True).reshape([B] + [1] * (a.dim() - 1))
    n = a / mu
    m_new = n + m * decay
    res, nes = mi_tail(a_c, x, m_new, alpha, eps, lo, hi, nes_scale)
    with torch.no_grad():
        momentum.copy_(m_new.to(momentum.device))
        if nes_out is not None:
            nes_out.copy_(nes.to(nes_out.device))
    res = _emit(res, adv, out)
    return (res, mu.reshape(B).to(adv.device)) if return_mean else res


def vt_neighbor(adv, bound, draw=None, seed=None, offset=0, out=None):
    """vmifgsm.py:84-85."""
    a = _c(adv)
    d = _c(draw) if draw is not None else philox_uniform(a.numel(), bound, seed, offset).reshape(a.shape)
    return _emit(a + d, adv, out)


def vt_accumulate(gv, g, first):
    """vmifgsm.py:82, 94-95: the accumulator starts from zeros."""
    acc = torch.zeros_like(_c(gv)) if first else _c(gv)
    acc = acc + _c(g)
    with torch.no_grad():
        gv.copy_(acc.to(gv.device))


def vt_variance(gv, adv_grad, N, out=None):
    """vmifgsm.py:97."""
    return _emit(_c(gv) / N - _c(adv_grad), gv, out)


class ReferenceLoss:
    """This table with the reference's loss arithmetic: d cost / d z from autograd through CrossEntropyLoss (mean reduction)
    over cat([-z, z], 1), negated when targeted (mifgsm.py:52, 61-64), instead of the closed form the library uses.
    Everything else is the table above: it isolates the one deliberate difference in the arithmetic."""

    def __getattr__(self, name):
        return getattr(__import__(__name__, fromlist=["_"]), name)

    @staticmethod
    def ce2_loss_grad(z, labels, scale=1.0):
        zc = _c(z).reshape(-1, 1).requires_grad_(True)
        with torch.enable_grad():
            cost = torch.nn.CrossEntropyLoss()(torch.cat([-zc, zc], 1), _c(labels).reshape(-1))
            cost = -cost if scale < 0 else cost
            (dz,) = torch.autograd.grad(cost, [zc])
        return dz.reshape(z.shape).to(z.device), cost.detach().reshape(1).to(z.device)
