"""TEST INFRASTRUCTURE — hip_ops.fmn_sparse_step (include/advstep_fmn_sparse.h) restated in float32 torch eager on the CPU,
expression by expression: tests/fmn_cpu_ops.py's decision pattern with the L1 and the L0 radius rules, its `move_delta`, and
the two sort-/bisection-based projections of tests/apgdl1_cpu_ops.py and tests/l0_cpu_ops.py applied row by row, each row with
its own radius.  Every other op is tests/fmn_cpu_ops.py's (fmn_begin among them).  Inputs may live on any device: they are
copied to the CPU, and results go back to the input's device (into `out` / `state_out` / `best_adv` when given), so the table
can stand in for hip_ops inside torchattacks.FMNSparse and can recompute a GPU launch from its own inputs and the kernel's own
row norms (`given_norms=`).  Also here: float64 row norms, the bound on the device's sums derived from their summation order,
and the linear detectors both test files run the attack on.

Bounds.  include/advstep_fmn_sparse.h states the summation order of a row sum: n = 4 ceil(T / 4096) + 21 additions on the
longest chain (a thread's samples one after the other, 6 shuffle levels, 15 waves), all over non-negative terms.  With
u = 2^-24 and gamma(k) = k u / (1 - k u) (Higham), against the float64 sum of the SAME float32 operands:
    sum |d|   d = fl(adv - orig) is the float32 operand both sides add: n additions      |err| <= gamma(n) sum64
    sum g^2   every square rounds once, then n additions                                 |err| <= gamma(n + 1) sum64
    #{d != 0} and max |g|: no rounding (T < 2^24), bit for bit
No constant was measured."""
import math

import torch

from tests import apgdl1_cpu_ops as _l1
from tests import fmn_cpu_ops as _base
from tests import l0_cpu_ops as _l0
from tests.apgd_cpu_ops import _c, _emit
from tests.fmn_cpu_ops import _clampf, _f, gamma_k, move_delta
from tests.radius_cpu_ops import LinearDetector, U, judged_wrong  # noqa: F401

NAME = "fmn_sparse_cpu"
FMN_SPARSE_NORMS = ("dabs", "dcnt", "gsq", "gmax")
INF = math.inf


def __getattr__(name):  # every op this table does not restate
    return getattr(_base, name)


def chain(T):
    """Additions on the longest chain of a row sum of csrc/fmn_sparse.hip: 4 ceil(T / 4096) + 21."""
    return 4 * math.ceil(T / 4096) + 21


def sum_rel_bound(T, squares):
    """|sum - sum64| / sum64 of a device row sum over non-negative terms: chain(T) additions, plus one rounding per square."""
    return gamma_k(chain(T) + (1 if squares else 0))


def sparse_norms(adv, grad, orig):
    """(4, B) float32: sum |d|, #{d != 0}, sum g^2, max |g| in torch's own summation order (grad None: the g rows are 0)."""
    B = adv.shape[0]
    d = (_c(adv) - _c(orig)).reshape(B, -1)
    g = torch.zeros_like(d) if grad is None else _c(grad).reshape(B, -1)
    return torch.stack([d.abs().sum(dim=1), (d != 0).sum(dim=1).to(torch.float32), (g * g).sum(dim=1), g.abs().amax(dim=1)])


def row_norms64(adv, grad, orig):
    """(4, B) float64 over the float32 operands d = fl(adv - orig) and g."""
    B = adv.shape[0]
    d = (_c(adv) - _c(orig)).reshape(B, -1).double()
    g = torch.zeros_like(d) if grad is None else _c(grad).reshape(B, -1).double()
    return torch.stack([d.abs().sum(dim=1), (d != 0).sum(dim=1).double(), (g * g).sum(dim=1), g.abs().amax(dim=1)])


def decide(norms4, z, labels, state, gamma, norm, T):
    """(copy (B) bool, new state (4, B)) of one step from the row norms (4, B) = sum |d|, #{d != 0}, sum g^2, max |g|."""
    n4, st = _c(norms4), _c(state)
    zb = _c(z).reshape(-1)
    dn = n4[0] if norm == "L1" else n4[1]
    e, best, found = st[0], st[1], st[2] != 0
    is_adv = judged_wrong(zb, labels)
    better = is_adv & (dn < best)
    best1 = torch.where(better, dn, best)
    g = _f(gamma)
    shrink, grow = _f(1.0) - g, _f(1.0) + g
    if norm == "L1":
        gq = n4[3]
        reach = dn + torch.where(gq > 0, zb.abs() / gq, torch.full_like(gq, INF))
        eps1 = torch.where(is_adv, torch.minimum(e, best1) * shrink, torch.where(found, e * grow, reach * grow))
    else:
        e1 = torch.where(e == INF, torch.ones_like(e), e)
        down = torch.minimum(torch.minimum(e1 - _f(1.0), torch.floor(e1 * shrink)), best1)
        up = torch.maximum(e1 + _f(1.0), torch.floor(e1 * grow))
        eps1 = _clampf(torch.where(is_adv, down, up), _f(0.0), _f(float(T)))
    found1 = (found | is_adv).to(torch.float32)
    return better, torch.stack([eps1, best1, found1, dn])


def project_rows(x, u, eps_rows, norm):
    """Each row of u (B, T) projected about x into ITS radius: apgdl1_cpu_ops.project (L1) or l0_cpu_ops.project (L0: kk < 1
    gives the x row, a NaN radius keeps every sample, as the kernel's failed comparisons do)."""
    B, T = x.shape
    rows = []
    for b in range(B):
        e = float(eps_rows[b])
        xb, ub = x[b:b + 1], u[b:b + 1]
        if norm == "L1":
            rows.append(_l1.project(xb, ub, e))
        elif e < 1:
            rows.append(xb.clone())
        else:
            rows.append(_l0.project(xb, ub, T if math.isnan(e) else int(min(e, T))))
    return torch.cat(rows)


def fmn_sparse_step(adv, grad, orig, z, labels, state, best_adv, alpha, gamma, norm, move=True, eps_div=1e-10, state_out=None,
                    out=None, row_norms=None, given_norms=None):
    """hip_ops.fmn_sparse_step.  given_norms: a (4, B) tensor of row norms to use INSTEAD of this table's own sums — the
    kernel's, so that everything after the sums can be compared bit for bit."""
    if norm not in ("L1", "L0"):
        raise ValueError(f"fmn_sparse_step norm must be 'L1' or 'L0', got {norm!r}")
    B = adv.shape[0]
    T = adv.numel() // B
    n4 = _c(given_norms) if given_norms is not None else sparse_norms(adv, grad if move else None, orig)
    copy, new = decide(n4, z, labels, state, gamma, norm, T)
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
        x = _c(orig).reshape(B, -1)
        u = move_point(adv, grad, alpha, n4[2], eps_div)
        res = _emit(project_rows(x, u, new[0], norm), adv, out)
    if row_norms is not None:
        with torch.no_grad():
            row_norms.copy_(n4.to(row_norms.device))
    return state_out, res


def move_point(adv, grad, alpha, gsq, eps_div=1e-10):
    """u = adv + alpha * (g / (sqrt(sum g^2) + eps_div)) on the CPU, (B, T), from a given sum g^2 (B): fmn_cpu_ops.move_delta
    about 0 (u - 0 rounds nothing)."""
    B = adv.shape[0]
    return move_delta(adv, grad, torch.zeros_like(_c(adv)), alpha, gsq, eps_div).reshape(B, -1)


# ---- the analytic attack: linear one-logit detectors whose minimal norms are known in closed form ---------------------------------

L0_TRUE_K = (1, 1, 2, 3, 5, 8, 12, 20, 30, 45)


def _linear_parts(T, seed):
    g = torch.Generator().manual_seed(seed)
    B = 10
    w = (torch.rand(T, generator=g) + 0.5) * (torch.randint(0, 2, (T,), generator=g) * 2 - 1).float()   # no zeros
    x = torch.rand(B, T, generator=g) * 0.4 + 0.3
    y = (torch.arange(B) % 2).to(torch.int64)
    wrong = torch.zeros(B, dtype=torch.bool)
    wrong[0] = True
    side = torch.where(y == 1, 1.0, -1.0).double() * torch.where(wrong, -1.0, 1.0).double()             # the sign of z(x)
    flat = LinearDetector(torch.zeros(T), torch.where(y == 1, 1.0, -1.0).double())                      # every row right, no gradient
    return w, x, y, wrong, side, flat


def l0_gains(w, x, side):
    """(B, T) float64, descending per row: what each sample can move z towards the other class, |w_i| cap_i, cap_i the headroom
    of x_i inside [0, 1] in the flipping direction (z has to move by -side |z|)."""
    up = (-side[:, None] * w.double()[None, :]) > 0                                                     # the sample has to rise
    cap = torch.where(up, 1.0 - x.double(), x.double())
    return (w.double().abs()[None, :] * cap).sort(dim=1, descending=True)[0]


def linear_case(T, norm, seed=0):
    """(model, zero-weight model, x, y, true minima (float64)) — ten rows of both classes on z = x . w + bias_row, x in
    [0.3, 0.7]; row 0 is already wrong (minimum 0).  The second model has w = 0: no row of it can flip.
    L1: the minimal L1 norm is |z| / max |w| (all of it on the heaviest sample), log-spaced over 0.01 .. 0.25 — below the 0.3 of
        headroom every sample has, so the box never binds.
    L0: the minimal count is the smallest k whose k largest gains |w_i| cap_i sum to at least |z|; |z| is placed half-way
        between the cumulative sums of k - 1 and k gains for k = L0_TRUE_K."""
    w, x, y, wrong, side, flat = _linear_parts(T, seed)
    B = x.shape[0]
    if norm == "L1":
        lo, hi = 0.01, 0.25
        true = torch.tensor([lo * (hi / lo) ** (b / (B - 1)) for b in range(B)], dtype=torch.float64)
        zabs = true * w.double().abs().max()
    elif norm == "L0":
        cum = torch.cat([torch.zeros(B, 1, dtype=torch.float64), l0_gains(w, x, side).cumsum(dim=1)], dim=1)
        k = torch.tensor(L0_TRUE_K)
        zabs = 0.5 * (cum.gather(1, (k - 1)[:, None]) + cum.gather(1, k[:, None])).reshape(-1)
        true = k.double()
    else:
        raise ValueError(norm)
    bias = side * zabs - x.double() @ w.double()
    return LinearDetector(w, bias), flat, x, y, torch.where(wrong, torch.zeros_like(true), true)


def l0_margins(model, x, y):
    """(below, above) per row, float64: how far |z(x)| lies above the k - 1 and below the k largest gains' sums, k = L0_TRUE_K
    (both must be positive for the true count to be k: a condition on the inputs)."""
    with torch.no_grad():
        z = model(x).reshape(-1).double()
    side = torch.where(z > 0, 1.0, -1.0).double()
    cum = torch.cat([torch.zeros(x.shape[0], 1, dtype=torch.float64), l0_gains(model.w.detach().float(), x, side).cumsum(dim=1)], dim=1)
    k = torch.tensor(L0_TRUE_K)
    return z.abs() - cum.gather(1, (k - 1)[:, None]).reshape(-1), cum.gather(1, k[:, None]).reshape(-1) - z.abs()
