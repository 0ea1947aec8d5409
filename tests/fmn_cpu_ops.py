"""TEST INFRASTRUCTURE — the FMN entry points of hip_ops (fmn_begin, fmn_norms, fmn_step, with fmn_workspace / fmn_partials)
restated in float32 torch eager on the CPU, expression by expression (include/advstep_fmn.h); every other op is
oracle.torch_ops'.  Inputs may live on any device: they are copied to the CPU, and results go back to the input's device (into
`out` / `state_out` / `best_adv` when given), so the table can stand in for hip_ops inside torchattacks.FMN and can recompute a
GPU launch from its own inputs and the kernel's own row norms.  Also here: float64 row norms, the bounds on the device's sums
derived from their summation order, and the linear detectors both test files run the attack on.

PAPER_RULE switches the never-found rule to the paper's unwidened eps' = dn + |z| / gq; only the test that documents the
departure sets it.

Bounds.  tests/test_gpu_minradius.py's docstring derives the summation order of a row sum (csrc/radius.hip's, which
csrc/fmn.hip keeps): n = 24 + ceil(C / 256) additions on the longest chain, C = ceil(T / 4096), all over non-negative terms.
With u = 2^-24 and gamma(k) = k u / (1 - k u) (Higham's bound on k roundings of non-negative terms), against the float64 sum
of the SAME float32 operands:
    sum |g|   n additions                                     |err| <= gamma(n) sum64
    sum g^2   every square rounds once, then n additions      |err| <= gamma(n + 1) sum64
    sum d^2   d = fl(adv - orig) is the float32 operand both sides square: as sum g^2
    max |d|   no rounding: bit for bit
and a square root halves the relative error and rounds once more (radius_cpu_ops.norm_rel_bound).  No constant was measured."""
import math

import torch

from oracle import torch_ops as _base
from tests.apgd_cpu_ops import _c, _emit
from tests.radius_cpu_ops import LinearDetector, U, chain, judged_wrong, l2_ball_bound, l2_tail, norm_rel_bound  # noqa: F401

NAME = "fmn_cpu"
FMN_PLANES = ("eps", "best", "found", "dnorm")
FMN_NORMS = ("dsq", "dmax", "gsq", "gabs")
FMN_TILE = 4096
PAPER_RULE = False
INF = math.inf


def __getattr__(name):  # every op this table does not restate
    return getattr(_base, name)


def _f(v):
    return torch.tensor(v, dtype=torch.float32)


def _sqrt32(t):
    """The correctly rounded float32 square root (the device's sqrtf): through float64, whose 53 bits make the second rounding
    innocuous.  The vectorised float32 square root of a CPU tensor can be one ulp off (seen on sum g^2 = 9.391747: 3.0645959
    for 3.0645957), which a bit-for-bit comparison with the device cannot carry."""
    return t.double().sqrt().float()


def tiles(T):
    return -(-T // FMN_TILE)


def _plane(B, T):
    return ((B * tiles(T) * 4 + 15) // 16 * 16) // 4       # floats of one 16-byte aligned plane


def fmn_workspace(B, T, device="cpu"):
    return torch.zeros(max(5 * _plane(B, T), 4), dtype=torch.float32, device=device)


def fmn_partials(ws, B, T):
    plane = ws.numel() // 5
    return ws[:4 * plane].view(4, plane)[:, :B * tiles(T)].view(4, B, tiles(T))


def fmn_begin(state=None, B=None, device="cpu"):
    n = state.shape[1] if state is not None else int(B)
    new = torch.stack([torch.full((n,), INF), torch.full((n,), INF), torch.zeros(n), torch.zeros(n)])
    if state is None:
        return new.to(device)
    with torch.no_grad():
        state.copy_(new.to(state.device))
    return state


def tile_partials(adv, grad, orig):
    """(4, B, C) float32 partials of sum d^2, max |d|, sum g^2, sum |g| per 4096-sample tile (torch's own summation order)."""
    a, x = _c(adv), _c(orig)
    B = a.shape[0]
    d = (a - x).reshape(B, -1)
    T = d.shape[1]
    g = torch.zeros_like(d) if grad is None else _c(grad).reshape(B, -1)
    C = tiles(T)
    out = torch.zeros(4, B, C)
    for c in range(C):
        dd, gg = d[:, c * FMN_TILE:(c + 1) * FMN_TILE], g[:, c * FMN_TILE:(c + 1) * FMN_TILE]
        out[0, :, c] = (dd * dd).sum(dim=1)
        out[1, :, c] = dd.abs().amax(dim=1)
        out[2, :, c] = (gg * gg).sum(dim=1)
        out[3, :, c] = gg.abs().sum(dim=1)
    return out


def fmn_norms(adv, grad, orig, ws=None):
    B = adv.shape[0]
    T = adv.numel() // B
    if ws is None:
        ws = fmn_workspace(B, T, adv.device)
    with torch.no_grad():
        fmn_partials(ws, B, T).copy_(tile_partials(adv, grad, orig).to(ws.device))
    return ws


def row_norms_of(partials):
    """(4, B): the re-reduction of the partials (sum, max, sum, sum over the tiles; amax propagates NaN as max_nan does)."""
    p = _c(partials)
    return torch.stack([p[0].sum(dim=1), p[1].amax(dim=1), p[2].sum(dim=1), p[3].sum(dim=1)])


def decide(norms4, z, labels, state, gamma, norm):
    """(copy (B) bool, new state (4, B)) of one step from the row norms (4, B) = sum d^2, max |d|, sum g^2, sum |g|."""
    n4, st = _c(norms4), _c(state)
    zb = _c(z).reshape(-1)
    dn = _sqrt32(n4[0]) if norm == "L2" else n4[1]
    gq = _sqrt32(n4[2]) if norm == "L2" else n4[3]
    e, best, found = st[0], st[1], st[2] != 0
    is_adv = judged_wrong(zb, labels)
    better = is_adv & (dn < best)
    best1 = torch.where(better, dn, best)
    g = _f(gamma)
    shrink, grow = _f(1.0) - g, _f(1.0) + g
    reach = dn + torch.where(gq > 0, zb.abs() / gq, torch.full_like(gq, INF))
    never = reach if PAPER_RULE else reach * grow
    eps1 = torch.where(is_adv, torch.minimum(e, best1) * shrink, torch.where(found, e * grow, never))
    found1 = (found | is_adv).to(torch.float32)
    return better, torch.stack([eps1, best1, found1, dn])


def _clampf(v, lo, hi):
    """csrc/advstep_common.h's clampf: v < lo ? lo : v, then v > hi ? hi : v (a NaN bound leaves v alone)."""
    v = torch.where(v < lo, lo.expand_as(v), v)
    return torch.where(v > hi, hi.expand_as(v), v)


def move_delta(adv, grad, orig, alpha, gsq, eps_div=1e-10):
    """d' = (adv + alpha * (g / (sqrt(sum g^2) + eps_div))) - orig from a given sum g^2 (B)."""
    a = _c(adv)
    gn = (_sqrt32(_c(gsq)) + _f(eps_div)).reshape([a.shape[0]] + [1] * (a.dim() - 1))
    return (a + _f(alpha) * (_c(grad) / gn)) - _c(orig)


def fmn_step(adv, grad, orig, z, labels, state, best_adv, ws, alpha, gamma, norm="Linf", move=True, eps_div=1e-10, lo=0.0, hi=1.0,
             state_out=None, out=None, row_norms=None, given_norms=None):
    """hip_ops.fmn_step.  given_norms: a (5, B) tensor of row norms to use INSTEAD of re-reducing `ws` — the kernel's own, so
    that everything after the sums can be compared bit for bit (plane 4 = the L2 move's ||d'||, NaN to recompute it)."""
    if norm not in ("Linf", "L2"):
        raise ValueError(f"FMN norm must be 'Linf' or 'L2', got {norm!r}")
    B = adv.shape[0]
    T = adv.numel() // B
    n4 = _c(given_norms)[:4] if given_norms is not None else row_norms_of(fmn_partials(ws, B, T))
    copy, new = decide(n4, z, labels, state, gamma, norm)
    dn1 = torch.zeros(B)
    with torch.no_grad():
        rows = copy.nonzero().reshape(-1)
        if rows.numel():
            best_adv[rows.to(best_adv.device)] = adv.detach()[rows.to(adv.device)].to(best_adv.device)
        if state_out is None:
            state_out = new.to(state.device)
        else:
            state_out.copy_(new.to(state_out.device))
    res = None
    if move:
        x = _c(orig)
        d = move_delta(adv, grad, orig, alpha, n4[2], eps_div)
        e = new[0].reshape([B] + [1] * (x.dim() - 1))
        if norm == "Linf":
            res = _clampf(x + _clampf(d, -e, e), _f(lo), _f(hi))
        else:
            dn1 = _sqrt32((d * d).reshape(B, -1).sum(dim=1))
            if given_norms is not None and not torch.isnan(_c(given_norms)[4]).all():
                dn1 = _c(given_norms)[4]
            res = l2_tail(x, d, e, dn1, lo, hi)
        res = _emit(res, adv, out)
    if row_norms is not None:
        with torch.no_grad():
            row_norms[:4].copy_(n4.to(row_norms.device))
            if move and norm == "L2":
                row_norms[4].copy_(dn1.to(row_norms.device))
    return state_out, res


# ---- float64 and the derived bounds ----------------------------------------------------------------------------------------------

def row_norms64(adv, grad, orig):
    """(4, B) float64: sum d^2, max |d|, sum g^2, sum |g| over the float32 operands d = fl(adv - orig) and g."""
    B = adv.shape[0]
    d = (_c(adv) - _c(orig)).reshape(B, -1).double()
    g = torch.zeros_like(d) if grad is None else _c(grad).reshape(B, -1).double()
    return torch.stack([(d * d).sum(dim=1), d.abs().amax(dim=1), (g * g).sum(dim=1), g.abs().sum(dim=1)])


def gamma_k(k):
    return k * U / (1 - k * U)


def sum_rel_bound(T, squares):
    """|sum - sum64| / sum64 of a device row sum over non-negative terms: chain(T) additions, plus one rounding per square."""
    return gamma_k(chain(T) + (1 if squares else 0))


# ---- the analytic attack: linear one-logit detectors whose minimal norms are known in closed form ---------------------------------

def linear_case(T, norm, seed=0):
    """(model, zero-weight model, x, y, true radii (float64)) — ten rows of both classes on z = x . w + bias_row, x in [0.3, 0.7]
    (the box never binds), true radii r = |z(x)| / ||w||_q (q = 1 for L-inf, 2 for L2) log-spaced over 1e-4 .. 0.03 (L-inf) or
    1e-3 .. 0.3 (L2); row 0 is already wrong (radius 0).  The second model has w = 0: no row of it can flip."""
    g = torch.Generator().manual_seed(seed)
    B = 10
    w = (torch.rand(T, generator=g) + 0.5) * (torch.randint(0, 2, (T,), generator=g) * 2 - 1).float()   # no zeros
    x = torch.rand(B, T, generator=g) * 0.4 + 0.3
    y = (torch.arange(B) % 2).to(torch.int64)
    lo, hi = (1e-4, 0.03) if norm == "Linf" else (1e-3, 0.3)
    true = torch.tensor([lo * (hi / lo) ** (b / (B - 1)) for b in range(B)], dtype=torch.float64)
    wnorm = w.double().abs().sum() if norm == "Linf" else w.double().norm()
    wrong = torch.zeros(B, dtype=torch.bool)
    wrong[0] = True
    side = torch.where(y == 1, 1.0, -1.0).double() * torch.where(wrong, -1.0, 1.0).double()             # the sign of z(x)
    bias = side * true * wnorm - x.double() @ w.double()
    flat = LinearDetector(torch.zeros(T), torch.where(y == 1, 1.0, -1.0).double())                      # every row right, no gradient
    return LinearDetector(w, bias), flat, x, y, torch.where(wrong, torch.zeros_like(true), true)
