"""TEST INFRASTRUCTURE — the three entry points of include/advstep_smoothadv.h restated on the CPU, built on
tests.smooth_cpu_ops.normals_np: each in a float32 form (the kernel's expressions in its rounding order, libm where the device has
its own transcendentals: not bit-identical) and a float64 form (the float32 inputs taken exactly, everything after them in
float64: what the device's error is measured against).  The module is also an op table: `smoothadv_fill`, `smoothadv_loss_grad`,
`smoothadv_step`, `smooth_noise` and `smooth_tally` take and return torch tensors like hip_ops', so it can stand in for hip_ops
inside SmoothAdvPGD, Smoothing and the trainer on a box without a GPU; every other op is oracle.torch_ops'."""
import numpy as np
import torch

from tests import smooth_cpu_ops as S
from tests.apgd_cpu_ops import _c, _emit

NAME = "smoothadv_cpu"


def __getattr__(name):  # every op this table does not restate (the random starts)
    from oracle import torch_ops
    return getattr(torch_ops, name)


def _f32(a):
    return np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float32)


# ---- a. the noised copies of the iterate ---------------------------------------------------------------------------------------------

def fill_np(adv, sigma, seed, offset=0, s0=0, ns=1, scale=None, shift=None, dtype=np.float32):
    """(ns, B, T): out[s - s0] = v + sigma * z(offset + s), v = fl(shift_b + fl(scale_b * adv)) or adv when scale / shift are None.
    v is float32 arithmetic on float32 inputs in BOTH forms (IEEE: the device's bits); float32: fl(v + fl(sigma * z)) as the
    kernel rounds; float64: v and sigma taken exactly, the normals, the product and the sum in float64."""
    adv = _f32(adv)
    B = adv.shape[0]
    v = adv.reshape(B, -1)
    if scale is not None:
        v = _f32(shift).reshape(B, 1) + _f32(scale).reshape(B, 1) * v
    assert v.dtype == np.float32
    T = v.shape[1]
    sig = np.float32(sigma)
    out = np.empty((ns, B, T), dtype=dtype)
    for i in range(ns):
        z = S.normals_np(B, T, seed, int(offset) + int(s0) + i, dtype)
        out[i] = v + sig * z if dtype == np.float32 else v.astype(np.float64) + np.float64(sig) * z
    return out


# ---- b. the soft vote and its gradient -----------------------------------------------------------------------------------------------

def loss_grad_np(z, labels, scale=1.0, dtype=np.float64):
    """(dz (m, B), cost (B)) in `dtype`, in the order the header writes: t = s z, l = -sp(-t), M = max l, e = exp(l - M), S = the
    slot-order sum, cost = (log m - M) - log S, dz = ((scale * -s) * (e / S)) * exp(-sp(t)).  A NaN logit makes its row NaN."""
    z = _f32(z).astype(dtype)
    m = z.shape[0]
    y = np.asarray(labels.detach().cpu().numpy() if isinstance(labels, torch.Tensor) else labels)
    s = (2.0 * y - 1.0).astype(dtype).reshape(1, -1)

    def sp(u):
        return np.maximum(u, dtype(0)) + np.log1p(np.exp(-np.abs(u)))

    with np.errstate(invalid="ignore"):
        t = s * z
        l = -sp(-t)
        M = l.max(axis=0)                                                             # numpy's max propagates NaN
        e = np.exp(l - M)
        tot = e[0].copy()
        for i in range(1, m):
            tot = tot + e[i]
        cost = (np.log(dtype(m)) - M) - np.log(tot)
        dz = ((dtype(scale) * -s) * (e / tot)) * np.exp(-sp(t))
    return dz.astype(dtype), cost.astype(dtype)


# ---- the logits and the error measure of the soft vote's tolerance (tools/smoothadv_probe.py --error and the GPU tests) -----------

def probe_logits(m, B, seed):
    """(z (m, B) float32, labels (B) int64): N(0, 3^2) logits; rows 0 .. 4 are all-saturated wrong, all-saturated right, mixed at
    +-80, saturated with one slot a logit apart, and near zero."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(m, B, generator=g) * 3.0
    y = torch.randint(0, 2, (B,), generator=g)
    s = (2 * y - 1).float()
    z[:, 0] = -80.0 * s[0]
    z[:, 1] = 80.0 * s[1]
    z[:, 2] = torch.where(torch.arange(m) % 2 == 0, 80.0, -80.0)
    z[:, 3] = -80.0 * s[3]
    z[0, 3] = -79.0 * s[3]
    z[:, 4] = 1e-3
    return z, y


def loss_error(dz, cost, dz_ref, cost_ref):
    """(max |dz - ref| / the row's max |ref|, max |cost - ref| / max(|ref|, 1)) for float64 numpy arrays."""
    row = np.abs(dz_ref).max(axis=0, keepdims=True)
    return float(np.max(np.abs(dz - dz_ref) / row)), float(np.max(np.abs(cost - cost_ref) / np.maximum(np.abs(cost_ref), 1.0)))


# ---- c. the sum over the slots, and the step -----------------------------------------------------------------------------------------

def step_t(adv, orig, grads, alpha, eps, norm="L2", eps_div=1e-10, lo=0.0, hi=1.0, dtype=torch.float32):
    """(out, gsum) in `dtype` on the CPU: gsum = ((g_0 + g_1) + g_2) + ... in slot order, then pgd.py:74-76 (L-inf) or
    pgdl2.py:78-88 (L2) expression by expression.  float32 rounds every expression as the kernels do; only the order inside the two
    row norms differs (torch's sum against the tile order), which is why the GPU tests compare with the library's own PGD steps."""
    a, x, g_all = _c(adv).to(dtype), _c(orig).to(dtype), _c(grads).to(dtype)
    B = a.shape[0]
    g = g_all[0].reshape(a.shape).clone()
    for i in range(1, g_all.shape[0]):
        g = g + g_all[i].reshape(a.shape)

    def c(v):
        return torch.tensor(v, dtype=torch.float32).to(dtype)                        # the launch scalars are float32

    cols = [B] + [1] * (a.dim() - 1)
    if norm == "Linf":
        moved = a + c(alpha) * g.sign()
        delta = torch.clamp(moved - x, min=-float(c(eps)), max=float(c(eps)))
        return torch.clamp(x + delta, min=lo, max=hi), g
    if norm != "L2":
        raise ValueError(f"norm must be 'L2' or 'Linf', got {norm!r}")
    gn = torch.sqrt((g * g).reshape(B, -1).sum(dim=1)).reshape(cols) + c(eps_div)
    d = (a + c(alpha) * (g / gn)) - x
    dn = torch.sqrt((d * d).reshape(B, -1).sum(dim=1)).reshape(cols)
    f = torch.minimum((1.0 / dn) * c(eps), torch.ones_like(dn))
    return torch.clamp(x + d * f, min=lo, max=hi), g


# ---- the analytic case ---------------------------------------------------------------------------------------------------------------

def unit_box_linear_case(T):
    """smooth_cpu_ops.linear_case moved into [0, 1]: (model, x01 = x + 0.5 in [0.25, 0.75], labels, k, sigma), the bias recomputed
    from x01 in float64 so that the clean logit of row b is again k_b sigma ||w||_2 exactly.  The perturbations tested here are
    below 0.005: no sample reaches the box."""
    model, x, y, k, sigma = S.linear_case(T)
    x01 = x + 0.5
    w = model.w.detach()
    bias = k * float(np.float32(sigma)) * w.norm() - x01.double() @ w
    return S.SlotLinearDetector(w.float(), bias), x01, y, k, sigma


def check_linear_attack(adv, x01, model, y, k, sigma, eps, steps, alpha):
    """What SmoothAdvPGD (L2, random_start=False) must return on the linear detector: every slot gradient is a multiple of w, so
    adv - x is -s min(steps alpha, eps) w / ||w||, up to one rounding of a sample below 1 per step and sample (2^-24), with a
    factor 2 of slack: the component along w and the L2 norm of the rest are each within steps sqrt(T) 2^-23.  Rows with
    |k| >= 0.5 lie further than eps = 0.45 sigma from the boundary and keep their float64 class; rows with 0 < |k| <= 0.25 cross it
    when the attack went the whole radius."""
    adv, x01 = adv.detach().cpu(), x01.detach().cpu()
    T = x01.shape[1]
    assert abs(eps - 0.45 * sigma) < 1e-12
    w = model.w.detach().cpu().double()
    unit = w / w.norm()
    d = adv.double() - x01.double()
    s = (2 * y.cpu() - 1).double()
    reach = min(steps * alpha, eps)
    along = d @ unit
    rest = (d - along[:, None] * unit[None]).norm(dim=1)
    bound = steps * np.sqrt(T) * 2.0 ** -23
    print(f"T = {T}: max |along + s reach| = {float((along + s * reach).abs().max()):.3e}, max ||rest|| = {float(rest.max()):.3e}, "
          f"bound {bound:.3e}")
    assert float((along + s * reach).abs().max()) <= bound and float(rest.max()) <= bound
    bias = model.bias.detach().cpu()
    clean = (x01.double() @ w + bias) > 0
    after = (adv.double() @ w + bias) > 0
    strong = k.abs() >= 0.5
    assert bool((after[strong] == clean[strong]).all())
    weak = (k.abs() > 0) & (k.abs() <= 0.25)
    if steps * alpha >= eps:
        assert bool(weak.any()) and bool((after[weak] != clean[weak]).all())
    return strong, clean


# ---- the op table ----------------------------------------------------------------------------------------------------------------------

def smoothadv_fill(adv, sigma, seed, offset=0, s0=0, ns=1, scale=None, shift=None, out=None):
    res = torch.from_numpy(fill_np(adv, sigma, seed, offset, s0, ns, scale, shift)).reshape((ns,) + tuple(adv.shape))
    return _emit(res, res, out)


def smoothadv_loss_grad(z, labels, scale=1.0):
    dz, cost = loss_grad_np(z, labels, scale, dtype=np.float32)
    return torch.from_numpy(dz).to(z.device), torch.from_numpy(cost).to(z.device)


def smoothadv_step(adv, orig, grads, alpha, eps, norm="L2", eps_div=1e-10, lo=0.0, hi=1.0, out=None, gsum=None):
    res, g = step_t(adv, orig, grads, alpha, eps, norm, eps_div, lo, hi)
    res = _emit(res, adv, out)
    return res if gsum is None else (res, _emit(g, adv, gsum))


def smooth_noise(x, sigma, seed, offset=0, s0=0, ns=1, out=None):
    res = torch.from_numpy(S.smooth_noise_np(x, sigma, seed, offset, s0, ns)).reshape((ns,) + tuple(x.shape))
    return _emit(res, res, out)


def smooth_tally(z, counts):
    with torch.no_grad():
        counts.copy_(torch.from_numpy(S.smooth_tally_np(z, counts)))
    return counts
