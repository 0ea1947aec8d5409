"""TEST INFRASTRUCTURE — the APGD entry points of hip_ops restated in float32 torch eager on the CPU, expression by expression
(include/advstep_apgd.h); every other op is oracle.torch_ops'.  Inputs may live on any device: they are copied to the CPU,
and results go back to the input's device (into `out` / the state tensors when given), so the table can stand in for
hip_ops inside the attack and can recompute a GPU launch from its own inputs."""
import numpy as np
import torch

from oracle import torch_ops as _base

NAME = "apgd_cpu"


def __getattr__(name):  # every op this table does not restate
    return getattr(_base, name)


def _c(t):
    return t.detach().to("cpu").contiguous()


def _emit(res, like, out):
    res = res.reshape(like.shape)
    if out is not None:
        with torch.no_grad():
            out.copy_(res.to(out.device))
        return out
    return res.to(like.device)


# ---- Philox4x32-10, the stream of the library's random starts -------------------------------------------------------------

def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Vectorised Philox4x32-10 over uint32 numpy arrays (the same rounds as csrc/advstep_common.h)."""
    m0, m1, mask = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0xFFFFFFFF)
    c0, c1, c2, c3 = (np.asarray(v, np.uint32) for v in (c0, c1, c2, c3))
    k0, k1 = np.uint32(k0), np.uint32(k1)
    for _ in range(10):
        p0, p1 = c0.astype(np.uint64) * m0, c2.astype(np.uint64) * m1
        hi0, lo0 = (p0 >> np.uint64(32)).astype(np.uint32), (p0 & mask).astype(np.uint32)
        hi1, lo1 = (p1 >> np.uint64(32)).astype(np.uint32), (p1 & mask).astype(np.uint32)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0 = np.uint32((int(k0) + 0x9E3779B9) & 0xFFFFFFFF)
        k1 = np.uint32((int(k1) + 0xBB67AE85) & 0xFFFFFFFF)
    return c0, c1, c2, c3


def _u01(bits, open0=False):
    return ((bits >> np.uint32(8)) + np.uint32(1 if open0 else 0)).astype(np.float32) * np.float32(5.9604644775390625e-08)


def philox_draw(B: int, T: int, norm: str, seed: int, offset: int = 0) -> torch.Tensor:
    """The (B, T) draw advstep_apgd_init_philox_f32 regenerates: U[0, 1) from the flat stream of pgd_linf_init_philox
    (L-inf) or the Box-Muller normals of pgd_l2_init_philox (L2; libm here, the device's hardware transcendentals there:
    not bit-identical, ~1e-6 relative)."""
    s_lo, s_hi = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    o_lo, o_hi = offset & 0xFFFFFFFF, (offset >> 32) & 0xFFFFFFFF
    if norm == "Linf":
        i = np.arange(B * T, dtype=np.uint64)
        q = i >> np.uint64(2)
        r = philox4x32_10((q & np.uint64(0xFFFFFFFF)).astype(np.uint32), (q >> np.uint64(32)).astype(np.uint32),
                          np.full(q.shape, o_lo, np.uint32), np.full(q.shape, o_hi, np.uint32), s_lo, s_hi)
        bits = np.choose((i & np.uint64(3)).astype(np.int64), r)
        return torch.from_numpy(_u01(bits).reshape(B, T))
    Q = (T + 3) // 4
    q, b = np.meshgrid(np.arange(Q, dtype=np.uint32), np.arange(B, dtype=np.uint32))
    r = philox4x32_10(q, b, np.full(q.shape, o_lo, np.uint32), np.full(q.shape, o_hi, np.uint32), s_lo, s_hi)
    r0 = np.sqrt(np.float32(-2.0) * np.log(_u01(r[0], True)))
    r1 = np.sqrt(np.float32(-2.0) * np.log(_u01(r[2], True)))
    t0 = np.float32(6.283185307179586) * _u01(r[1])
    t1 = np.float32(6.283185307179586) * _u01(r[3])
    n = np.stack([r0 * np.cos(t0), r0 * np.sin(t0), r1 * np.cos(t1), r1 * np.sin(t1)], axis=-1).astype(np.float32)
    return torch.from_numpy(np.ascontiguousarray(n.reshape(B, Q * 4)[:, :T]))


# ---- the entry points ------------------------------------------------------------------------------------------------------

def apgd_init(x, eps, norm="Linf", draw=None, seed=None, offset=0, lo=0.0, hi=1.0, out=None):
    """apgd.py:89-95 on (B, T) rows."""
    xc = _c(x)
    B = xc.shape[0]
    xc = xc.reshape(B, -1)
    d = _c(draw).reshape(B, -1) if draw is not None else philox_draw(B, xc.shape[1], norm, seed, offset)
    ones = torch.ones([B, 1])
    if norm == "Linf":
        t = 2 * d - 1
        res = xc + eps * ones * t / (t.reshape([B, -1]).abs().max(dim=1, keepdim=True)[0])
    elif norm == "L2":
        t = d
        res = xc + eps * ones * t / ((t ** 2).sum(dim=1, keepdim=True).sqrt() + 1e-12)
    else:
        raise ValueError(norm)
    return _emit(res.clamp(lo, hi), x, out)


def apgd_eval(z, labels, state=None, mode="grad", i=0):
    zc, y = _c(z).reshape(-1), _c(labels).reshape(-1)
    flip = 1.0 - 2.0 * y.to(torch.float32)
    u = flip * (2.0 * zc)
    loss = torch.clamp(u, min=0.0) + torch.log1p(torch.exp(-u.abs()))
    sig = 1.0 / (1.0 + torch.exp(-u))
    dz = 2.0 * (flip * sig)
    pred = (zc > 0).to(torch.int64) == y
    if mode != "grad":
        st = {k: _c(getattr(state, k)) for k in ("acc", "flags", "loss_best", "loss_best_last_check",
                                                  "reduced_last_check", "loss_steps")}
        if mode == "start":
            st["acc"] = pred.to(torch.uint8)
            st["loss_best"] = loss.clone()
            st["loss_best_last_check"] = loss.clone()
            st["reduced_last_check"] = torch.ones_like(st["reduced_last_check"])
            st["flags"] = torch.zeros_like(st["flags"])
        else:
            st["acc"] = torch.min(st["acc"], pred.to(torch.uint8))
            improved = loss > st["loss_best"]
            st["loss_best"] = torch.where(improved, loss, st["loss_best"])
            st["loss_steps"][i] = loss
            st["flags"] = (~pred).to(torch.uint8) | (improved.to(torch.uint8) << 1)
        for k, v in st.items():
            getattr(state, k).copy_(v.to(getattr(state, k).device))
    return dz.reshape(z.shape).to(z.device), loss.to(z.device)


def apgd_checkpoint(state, i, k, rho):
    """apgd.py:65-70, 194-211 with numpy, as the reference computes it."""
    L = _c(state.loss_steps).numpy()
    t = np.zeros(L.shape[1])
    for c in range(k):
        t += L[i - c] > L[i - c - 1]
    osc = t <= k * rho * np.ones(t.shape)
    reduced = _c(state.reduced_last_check).numpy().astype(bool)
    lblc, lb = _c(state.loss_best_last_check).numpy(), _c(state.loss_best).numpy()
    fl = ~(~osc * ~((~reduced) * (lblc >= lb)))
    step = _c(state.step_size)
    step[torch.from_numpy(fl)] /= 2.0
    flags = _c(state.flags) & 0xFB
    flags[torch.from_numpy(fl)] |= 4
    state.step_size.copy_(step.to(state.step_size.device))
    state.flags.copy_(flags.to(state.flags.device))
    state.reduced_last_check.copy_(torch.from_numpy(fl.astype(np.uint8)).to(state.reduced_last_check.device))
    state.loss_best_last_check.copy_(state.loss_best)


def apgd_track(x_adv, grad, x_best, grad_best, x_best_adv, flags):
    f = _c(flags)
    fooled, improved, reset = (f & 1) != 0, (f & 2) != 0, (f & 4) != 0
    xa, g, xb, gb, xba = (_c(t) for t in (x_adv, grad, x_best, grad_best, x_best_adv))
    xba[fooled] = xa[fooled]
    xb[improved] = xa[improved]
    gb[improved] = g[improved]
    xa[reset] = xb[reset]
    g[reset] = gb[reset]
    for dst, src in ((x_adv, xa), (grad, g), (x_best, xb), (grad_best, gb), (x_best_adv, xba)):
        dst.copy_(src.to(dst.device))


def apgd_linf_step(cur, prev, grad, x, step_size, eps, a, out=None):
    """apgd.py:140-149."""
    x_adv, x_adv_old, g, xc = _c(cur), _c(prev), _c(grad), _c(x)
    step = _c(step_size).reshape(-1, 1)
    grad2 = x_adv - x_adv_old
    x_adv_1 = x_adv + step * torch.sign(g)
    x_adv_1 = torch.clamp(torch.min(torch.max(x_adv_1, xc - eps), xc + eps), 0.0, 1.0)
    x_adv_1 = torch.clamp(torch.min(torch.max(x_adv + (x_adv_1 - x_adv) * a + grad2 * (1 - a), xc - eps), xc + eps), 0.0,
                          1.0)
    return _emit(x_adv_1, cur, out)


def apgd_l2_step(cur, prev, grad, x, step_size, eps, a, out=None, return_norms=False):
    """apgd.py:140-157."""
    x_adv, x_adv_old, g, xc = _c(cur), _c(prev), _c(grad), _c(x)
    step = _c(step_size).reshape(-1, 1)
    grad2 = x_adv - x_adv_old
    gn = (g ** 2).sum(dim=1, keepdim=True).sqrt()
    x_adv_1 = x_adv + step * g / (gn + 1e-12)
    n1 = ((x_adv_1 - xc) ** 2).sum(dim=1, keepdim=True).sqrt()
    x_adv_1 = torch.clamp(xc + (x_adv_1 - xc) / (n1 + 1e-12) * torch.min(eps * torch.ones(xc.shape), n1), 0.0, 1.0)
    x_adv_1 = x_adv + (x_adv_1 - x_adv) * a + grad2 * (1 - a)
    n2 = ((x_adv_1 - xc) ** 2).sum(dim=1, keepdim=True).sqrt()
    x_adv_1 = torch.clamp(xc + (x_adv_1 - xc) / (n2 + 1e-12) * torch.min(eps * torch.ones(xc.shape), n2 + 1e-12), 0.0,
                          1.0)
    res = _emit(x_adv_1, cur, out)
    if return_norms:
        return res, torch.cat([gn, n1, n2], 1).to(cur.device)
    return res


class ReferenceLoss:
    """This table with the reference's loss arithmetic in apgd_eval: the per-row loss and dz from autograd through
    CrossEntropyLoss(reduction='none') over cat([-z, z], 1), summed (apgd.py:103, 113-117), instead of the closed form the
    library uses.  Everything else is the table above: it isolates the one deliberate difference in the arithmetic."""

    def __getattr__(self, name):
        return getattr(__import__(__name__, fromlist=["_"]), name)

    @staticmethod
    def apgd_eval(z, labels, state=None, mode="grad", i=0):
        zc = _c(z).reshape(-1, 1).requires_grad_(True)
        y = _c(labels).reshape(-1)
        with torch.enable_grad():
            loss_indiv = torch.nn.CrossEntropyLoss(reduction="none")(torch.cat([-zc, zc], 1), y)
            (dz,) = torch.autograd.grad(loss_indiv.sum(), [zc])
        loss = loss_indiv.detach()
        pred = (zc.detach().reshape(-1) > 0).to(torch.int64) == y
        if mode != "grad":
            st = {k: _c(getattr(state, k)) for k in ("acc", "flags", "loss_best", "loss_best_last_check",
                                                      "reduced_last_check", "loss_steps")}
            if mode == "start":
                st.update(acc=pred.to(torch.uint8), loss_best=loss.clone(), loss_best_last_check=loss.clone(),
                          reduced_last_check=torch.ones_like(st["reduced_last_check"]), flags=torch.zeros_like(st["flags"]))
            else:
                st["acc"] = torch.min(st["acc"], pred.to(torch.uint8))
                improved = loss > st["loss_best"]
                st["loss_best"] = torch.where(improved, loss, st["loss_best"])
                st["loss_steps"][i] = loss
                st["flags"] = (~pred).to(torch.uint8) | (improved.to(torch.uint8) << 1)
            for k, v in st.items():
                getattr(state, k).copy_(v.to(getattr(state, k).device))
        return dz.reshape(z.shape).to(z.device), loss.to(z.device)
