"""TEST INFRASTRUCTURE — the minimal-radius entry points of hip_ops (row_pgd_linf_step, row_pgd_l2_step, radius_begin,
radius_round) restated in float32 torch eager on the CPU, expression by expression (include/advstep_radius.h); every other op is
oracle.torch_ops'.  Inputs may live on any device: they are copied to the CPU, and results go back to the input's device (into
`out` / `state` / `best_adv` when given), so the table can stand in for hip_ops inside MinRadiusPGD and can recompute a GPU launch
from its own inputs.  Also here: the analytic linear detector both test files run the search on."""
import math

import torch

from oracle import torch_ops as _base
from tests.apgd_cpu_ops import _c, _emit

NAME = "radius_cpu"
PLANES = ("lo", "hi", "eps", "best")


def __getattr__(name):  # every op this table does not restate
    return getattr(_base, name)


def _row_scalars(eps_rows, alpha_abs, alpha_rel, like):
    """e and a = alpha_abs + alpha_rel * e as float32 columns that broadcast over the rows of `like`."""
    e = _c(eps_rows).reshape([like.shape[0]] + [1] * (like.dim() - 1))
    a = torch.tensor(alpha_abs, dtype=torch.float32) + torch.tensor(alpha_rel, dtype=torch.float32) * e
    return e, a


def row_pgd_linf_step(adv, grad, orig, eps_rows, alpha_abs, alpha_rel, lo=0.0, hi=1.0, out=None):
    a_c, g, x = _c(adv), _c(grad), _c(orig)
    e, a = _row_scalars(eps_rows, alpha_abs, alpha_rel, a_c)
    x1 = a_c + a * g.sign()
    delta = torch.clamp(x1 - x, min=-e, max=e)
    return _emit(torch.clamp(x + delta, min=lo, max=hi), adv, out)


def l2_delta(adv, grad, orig, a, gn_raw, eps_div=1e-10):
    """d of the L2 step from a given ||g|| (B) — the kernel's own, or this table's."""
    gn = gn_raw.reshape(a.shape) + torch.tensor(eps_div, dtype=torch.float32)
    return (adv + a * (grad / gn)) - orig


def l2_tail(orig, d, e, dn, lo=0.0, hi=1.0):
    """The part of the L2 step without re-association: out from d and a given ||d|| (B)."""
    dn = dn.reshape(e.shape)
    f = torch.where(dn == 0, torch.ones_like(dn), torch.minimum((1.0 / dn) * e, torch.ones_like(dn)))
    return torch.clamp(orig + d * f, min=lo, max=hi)


def row_pgd_l2_step(adv, grad, orig, eps_rows, alpha_abs, alpha_rel, eps_div=1e-10, lo=0.0, hi=1.0, out=None,
                    return_norms=False):
    a_c, g, x = _c(adv), _c(grad), _c(orig)
    B = a_c.shape[0]
    e, a = _row_scalars(eps_rows, alpha_abs, alpha_rel, a_c)
    gn_raw = torch.sqrt((g * g).reshape(B, -1).sum(dim=1))
    d = l2_delta(a_c, g, x, a, gn_raw, eps_div)
    dn = torch.sqrt((d * d).reshape(B, -1).sum(dim=1))
    res = _emit(l2_tail(x, d, e, dn, lo, hi), adv, out)
    return (res, gn_raw.to(adv.device), dn.to(adv.device)) if return_norms else res


def judged_wrong(z, labels):
    """(int64)(z > 0) != y: the first maximal index of cat([-z, z], 1), so +-0 and NaN give class 0."""
    return (_c(z).reshape(-1) > 0).to(torch.int64) != _c(labels).reshape(-1)


def radius_begin(z0, labels, eps_max, state=None):
    wrong = judged_wrong(z0, labels)
    B = wrong.numel()
    zero = torch.zeros(B, dtype=torch.float32)
    hi = torch.where(wrong, zero, torch.full((B,), eps_max, dtype=torch.float32))
    best = torch.where(wrong, zero, torch.full((B,), math.inf, dtype=torch.float32))
    new = torch.stack([zero, hi, hi, best])
    if state is None:
        return new.to(z0.device)
    with torch.no_grad():
        state.copy_(new.to(state.device))
    return state


def round_decision(z, labels, first, state):
    """(copy (B) bool, new state (4, B)) of one search round, on the CPU."""
    lo, hi, eps, best = (p.clone() for p in _c(state))
    flipped = judged_wrong(z, labels)
    better = flipped & (eps < best)
    held = ~flipped
    best = torch.where(better, eps, best)
    hi = torch.where(better, eps, hi)
    lo = torch.where(held, eps, lo)
    copy = better | (held & bool(first))
    return copy, torch.stack([lo, hi, 0.5 * (lo + hi), best])


def radius_round(adv, z, labels, first, state, best_adv, out=None):
    copy, new = round_decision(z, labels, first, state)
    with torch.no_grad():
        rows = copy.nonzero().reshape(-1)
        if rows.numel():
            best_adv[rows.to(best_adv.device)] = adv.detach()[rows.to(adv.device)].to(best_adv.device)
        if out is None:
            return new.to(state.device)
        out.copy_(new.to(out.device))
    return out


# ---- the analytic search: a linear one-logit detector whose minimal radii are known in closed form ----------------------------

class LinearDetector(torch.nn.Module):
    """z_b = x_b . w + bias_b, accumulated in float64 (the logit a test reasons about is then the exact one, rounded once).
    PGD moves every sample by the whole radius against sign(w) (L-inf) or along w / ||w||_2 (L2), so the smallest radius that
    flips row b is |z_b(x)| / ||w||_1 resp. |z_b(x)| / ||w||_2."""

    def __init__(self, w, bias):
        super().__init__()
        self.w = torch.nn.Parameter(w.clone().double())
        self.register_buffer("bias", bias.clone().double())

    def forward(self, x):
        return (x.double() @ self.w + self.bias).float().unsqueeze(1)


def analytic_case(B, T, norm, eps_max, search_steps, seed=0):
    """(model, x, y, true radii (float64), expected `last_radius` (float32)) for a batch that holds, in turn, a row the model
    already gets wrong, rows that flip inside eps_max and a row that cannot.  No true radius lies within 0.1 % of eps_max of a
    grid point k * eps_max / 2^(search_steps - 1) (asserted: a condition on the inputs, not on the code under test)."""
    g = torch.Generator().manual_seed(seed)
    w = (torch.rand(T, generator=g) + 0.5) * (torch.randint(0, 2, (T,), generator=g) * 2 - 1).float()   # no zeros
    x = torch.rand(B, T, generator=g) * 0.5 + 0.25                                                       # the [0, 1] clamp never binds
    y = torch.randint(0, 2, (B,), generator=g)
    grid = eps_max / 2 ** (search_steps - 1)
    # ||w|| = 64 in the attack's norm, so |z(x)| = 64 * (the row's true radius) <= 64 * (1 + 0.29 * (1 + (B - 1) // 5)) * eps_max:
    # 1.58 at eps_max = 2^-6 and B = 8.  The loss gradient's sigmoid(-2 |z|) is then >= e^-3.2, far from float32 underflow
    # (|z| ~ 44), so no row loses its gradient
    w = (w.double() * (64.0 / (w.double().abs().sum() if norm == "Linf" else w.double().norm()))).float()
    wnorm = w.double().abs().sum() if norm == "Linf" else w.double().norm()
    # the kind of a row by its index (B >= 3 holds every kind); radii in units of the grid, fractional parts away from 0 and 1
    cells = 2 ** (search_steps - 1)
    true = torch.empty(B, dtype=torch.float64)
    wrong = torch.zeros(B, dtype=torch.bool)
    for b in range(B):
        if b % 5 == 0:
            wrong[b], true[b] = True, 0.37 * eps_max                 # already wrong, by a margin
        elif b % 5 == 2:
            true[b] = (1.0 + 0.29 * (1 + b // 5)) * eps_max          # out of reach
        else:
            true[b] = (((5 * b + 3) % cells) + 0.23 + 0.11 * (b % 5)) * grid
    frac = (true / grid) - torch.floor(true / grid)
    assert ((frac * grid > 1e-3 * eps_max) & ((1 - frac) * grid > 1e-3 * eps_max)).all()
    side = torch.where(y == 1, 1.0, -1.0).double() * torch.where(wrong, -1.0, 1.0).double()     # the sign of z(x)
    bias = side * true * wnorm - x.double() @ w.double()
    expected = torch.where(wrong, torch.zeros(B, dtype=torch.float64),
                           torch.where(true > eps_max, torch.full((B,), math.inf, dtype=torch.float64),
                                       torch.ceil(true / grid) * grid)).float()
    return LinearDetector(w, bias), x, y, torch.where(wrong, torch.zeros_like(true), true), expected


U = 2.0 ** -24


def chain(T):
    """Additions on the longest chain of a row sum of squares (csrc/radius.hip): 24 + ceil(C / 256), C = ceil(T / 4096)."""
    return 24 + math.ceil(math.ceil(T / 4096) / 256)


def norm_rel_bound(T):
    """|norm - norm64| / norm64 of the device's row norms, to first order: every square rounds once and the chain adds
    chain(T) times over non-negative terms ((chain + 1) u on the sum), the square root halves that and rounds once more."""
    return ((chain(T) + 1) / 2 + 1) * U


def l2_ball_bound(e, T):
    """||out - orig||_2 of an L2 step at radius e: f <= (e / dn)(1 + 2u) (the reciprocal and the product round), dn >= ||d||
    (1 - norm_rel_bound), d * f rounds once per sample, and orig + d * f rounds to within u of a value in [0, 1] per sample
    (u sqrt(T) in the norm); the clamp only moves a sample towards orig, which lies in [0, 1]."""
    return e * (1 + norm_rel_bound(T) + 3 * U) + U * math.sqrt(T)
