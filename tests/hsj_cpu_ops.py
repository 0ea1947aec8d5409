"""TEST INFRASTRUCTURE — the HopSkipJump entry points of hip_ops (hsj_search_open / _next / _close, hsj_probe, hsj_candidates,
hsj_take; include/advstep_hsj.h) restated on the CPU in numpy float32 / int32 WITH THE KERNELS' OPERATION ORDER, the direction
bits being tests.spsa_cpu_ops'; plane 0 of perturbation_stats restated too (the maximum of |fl(adv - x)|: exact); every other op
is tests.spsa_cpu_ops'.  Inputs may live on any device; results go back to the input's device, so the table can stand in for hip_ops
inside torchattacks.HopSkipJump.

Every op is single rounded float32 operations or integers: point(r) is one subtraction, two clamps and one addition; a probe sample
one addition and a clamp; the step's sign an integer expression of population counts; a candidate two exact products, one addition
and a clamp.  numpy float32 rounds each the same way, so the GPU tests compare BYTES with this table, with no tolerance."""
import numpy as np
import torch

from tests import spsa_cpu_ops as _base
from tests.apgd_cpu_ops import _c, _emit
from tests.spsa_cpu_ops import LinearDetector, direction_bits  # noqa: F401  (re-exported)

NAME = "hsj_cpu"
PLANES = ("lo", "hi", "mid", "dist0")          # hip_ops.HSJ_PLANES
MAX_DIRECTIONS = 1024                          # ADVSTEP_HSJ_MAX_DIRECTIONS
MAX_TRIALS = 8                                 # ADVSTEP_HSJ_MAX_TRIALS
F = np.float32


def __getattr__(name):  # every op this table does not restate
    return getattr(_base, name)


# ---- float32 helpers with the kernels' semantics ------------------------------------------------------------------------------------

def _clamp(v, lo, hi):
    """clampf of csrc/advstep_common.h with scalar or per-row bounds: v < lo ? lo : v, then v > hi ? hi : v — a NaN stays."""
    lo, hi = np.asarray(lo, F), np.asarray(hi, F)
    v = np.where(v < lo, lo, v)
    return np.where(v > hi, hi, v).astype(F)


def adversarial(z, labels):
    """(z > 0) != (labels == 1): +-0 and NaN are class 0."""
    with np.errstate(invalid="ignore"):
        return (z > 0) != (labels == 1)


def point_np(cur, orig, r, lo=0.0, hi=1.0):
    """point(r) per row: clamp(orig + clamp(cur - orig, -r, r), lo, hi); r (B,)."""
    r = np.asarray(r, F)[:, None]
    d = _clamp((cur - orig).astype(F), -r, r)
    return _clamp((orig + d).astype(F), lo, hi)


def linf_np(x, adv):
    """Plane 0 of perturbation_stats: max_t |fl(adv - x)| per row (0 for rows of no samples)."""
    d = np.abs((adv - x).astype(F))
    return d.max(axis=1).astype(F) if d.shape[1] else np.zeros(d.shape[0], F)


# ---- the boundary search --------------------------------------------------------------------------------------------------------------

def search_open_np(cur, orig, dist, active, lo=0.0, hi=1.0):
    """(out (B, T), state (4, B))."""
    act = active != 0
    dist = dist.astype(F)
    mid = ((F(0.0) + dist) * F(0.5)).astype(F)
    state = np.stack([np.where(act, F(0.0), dist), dist, np.where(act, mid, dist), dist]).astype(F)
    out = point_np(cur, orig, mid, lo, hi)
    out[~act] = cur[~act]
    return out, state


def _decide(z, labels, state):
    blo, bhi, mid, d0 = (p.copy() for p in state)
    adv = adversarial(z, labels)
    return np.where(adv, blo, mid).astype(F), np.where(adv, mid, bhi).astype(F), d0


def search_next_np(cur, orig, z, labels, active, state, lo=0.0, hi=1.0):
    """(out (B, T), state_out (4, B))."""
    act = active != 0
    blo, bhi, d0 = _decide(z, labels, state)
    mid = ((blo + bhi) * F(0.5)).astype(F)
    new = np.stack([blo, bhi, mid, d0]).astype(F)
    new[:, ~act] = state[:, ~act]
    out = point_np(cur, orig, mid, lo, hi)
    out[~act] = cur[~act]
    return out, new


def search_close_np(cur, orig, z, labels, active, state, queries, rounds, lo=0.0, hi=1.0):
    """(out (B, T), queries (B,) int32)."""
    act = active != 0
    _, bhi, d0 = _decide(z, labels, state)
    move = act & (bhi < d0)
    out = point_np(cur, orig, bhi, lo, hi)
    out[~move] = cur[~move]
    return out, (queries + np.where(act, rounds, 0)).astype(np.int32)


# ---- the probes -------------------------------------------------------------------------------------------------------------------------

def probe_np(cur, mag, active, seed, offset=0, s0=0, ns=1, lo=0.0, hi=1.0):
    """(ns, B, T) float32."""
    B, T = cur.shape
    act = active != 0
    m = mag.astype(F)[:, None]
    out = np.empty((ns, B, T), F)
    for i, j in enumerate(range(s0, s0 + ns)):
        out[i] = _clamp((cur + np.where(direction_bits(B, T, j, seed, offset), -m, m)).astype(F), lo, hi)
        out[i][~act] = cur[~act]
    return out


# ---- the step -------------------------------------------------------------------------------------------------------------------------------

def vote_np(z, labels, T, seed, offset=0):
    """(B, T) int64: the integer form of the estimate for every row, active or not — with c the adversarial probes of the row, a the
    adversarial probes whose bit is set at the sample and e the other probes whose bit is set there: c e - (n - c) a where
    0 < c < n, n - 2 a where c == n, 2 e - n where c == 0."""
    n, B = z.shape
    phi = np.stack([adversarial(z[j], labels) for j in range(n)]) if n else np.zeros((0, B), bool)
    c = phi.sum(axis=0).astype(np.int64)[:, None]
    a = np.zeros((B, T), np.int64)
    e = np.zeros((B, T), np.int64)
    for j in range(n):
        bit = direction_bits(B, T, j, seed, offset)
        a += bit & phi[j][:, None]
        e += bit & ~phi[j][:, None]
    return np.where(c == n, n - 2 * a, np.where(c == 0, 2 * e - n, c * e - (n - c) * a))


def candidates_np(cur, z, labels, dist, active, xi_rel, trials, seed, offset=0, lo=0.0, hi=1.0):
    """(trials, B, T) float32."""
    B, T = cur.shape
    act = active != 0
    s = np.sign(vote_np(z, labels, T, seed, offset)).astype(F)
    xi = (dist.astype(F) * F(xi_rel)).astype(F)
    out = np.empty((trials, B, T), F)
    scale = F(1.0)
    for k in range(trials):
        step = (xi * scale).astype(F)[:, None]
        with np.errstate(invalid="ignore"):
            out[k] = _clamp((cur + (step * s).astype(F)).astype(F), lo, hi)
        out[k][~act] = cur[~act]
        scale = F(scale * F(0.5))
    return out


def take_np(cur, cand, zc, labels, active, queries, n):
    """(out (B, T), queries (B,) int32, used (B,) — k + 1 of the slot taken, trials where none was, 0 for inactive rows)."""
    K, B = zc.shape
    act = active != 0
    adv = np.stack([adversarial(zc[k], labels) for k in range(K)]) if K else np.zeros((0, B), bool)
    any_adv = adv.any(axis=0) if K else np.zeros(B, bool)
    first = adv.argmax(axis=0) if K else np.zeros(B, np.int64)
    used = np.where(act, np.where(any_adv, first + 1, K), 0)
    out = cur.copy()
    for b in range(B):
        if act[b] and any_adv[b]:
            out[b] = cand[first[b], b]
    return out, (queries + np.where(act, n + used, 0)).astype(np.int32), used


# ---- the table's ops ----------------------------------------------------------------------------------------------------------------------

def _np2(t):
    a = _c(t).numpy()
    return a.reshape(a.shape[0], -1)


def _np1(t):
    return _c(t).numpy().reshape(-1)


def _put(dst, arr):
    with torch.no_grad():
        dst.copy_(torch.from_numpy(np.ascontiguousarray(arr)).reshape(dst.shape).to(dst.device))
    return dst


def perturbation_stats(x, adv, out=None):
    """(6, B): plane 0 exact, the other planes NaN (HopSkipJump reads plane 0 alone)."""
    res = np.full((6, x.shape[0]), np.nan, F)
    res[0] = linf_np(_np2(x), _np2(adv))
    res = torch.from_numpy(res)
    return _put(out, res.numpy()) if out is not None else res.to(x.device)


def hsj_search_open(cur, orig, dist, active, out, state=None, lo=0.0, hi=1.0):
    res, st = search_open_np(_np2(cur), _np2(orig), _np1(dist), _np1(active), lo, hi)
    _put(out, res)
    return torch.from_numpy(st).to(cur.device) if state is None else _put(state, st)


def hsj_search_next(cur, orig, z, labels, active, state, out, state_out=None, lo=0.0, hi=1.0):
    res, st = search_next_np(_np2(cur), _np2(orig), _np1(z), _np1(labels), _np1(active), _c(state).numpy(), lo, hi)
    _put(out, res)
    return torch.from_numpy(st).to(cur.device) if state_out is None else _put(state_out, st)


def hsj_search_close(cur, orig, z, labels, active, state, queries, rounds, out=None, lo=0.0, hi=1.0):
    res, q = search_close_np(_np2(cur), _np2(orig), _np1(z), _np1(labels), _np1(active), _c(state).numpy(), _np1(queries),
                             int(rounds), lo, hi)
    _put(queries, q)
    return _emit(torch.from_numpy(res), cur, out)


def hsj_probe(cur, mag, active, seed, offset=0, s0=0, ns=1, lo=0.0, hi=1.0, out=None):
    res = probe_np(_np2(cur), _np1(mag), _np1(active), seed, offset, s0, ns, lo, hi)
    if out is not None:
        return _put(out, res)
    return torch.from_numpy(res).reshape((ns,) + tuple(cur.shape)).to(cur.device)


def hsj_candidates(cur, z, labels, dist, active, xi_rel, trials, seed, offset=0, lo=0.0, hi=1.0, out=None):
    res = candidates_np(_np2(cur), _c(z).numpy(), _np1(labels), _np1(dist), _np1(active), xi_rel, int(trials), seed, offset, lo, hi)
    if out is not None:
        return _put(out, res)
    return torch.from_numpy(res).reshape((int(trials),) + tuple(cur.shape)).to(cur.device)


def hsj_take(cur, cand, zc, labels, active, queries, n, out=None):
    K = zc.shape[0]
    res, q, _ = take_np(_np2(cur), _c(cand).numpy().reshape(K, cur.shape[0], -1), _c(zc).numpy(), _np1(labels), _np1(active),
                        _np1(queries), int(n))
    _put(queries, q)
    return _emit(torch.from_numpy(res), cur, out)


# ---- the exact end-to-end case ---------------------------------------------------------------------------------------------------------

X_BITS = 6
DYADIC = {"eps": 2.0 ** -4, "steps": 3, "init_evals": 6, "max_evals": 8, "search_steps": 3, "step_trials": 2, "delta_rel": 2.0 ** -2,
          "delta_min": 2.0 ** -12, "step_schedule": (0.5, 0.5, 0.5), "init_trials": 2}
# the deepest fractional bit of a forwarded sample (derived in dyadic_case's docstring)
G = X_BITS + DYADIC["search_steps"] + DYADIC["steps"] * (DYADIC["search_steps"] + 1 + DYADIC["step_trials"] - 1)
assert G == 24 and G + 6 + 4 <= 52


class GridChecked(torch.nn.Module):
    """A detector that asserts, at run time, that every sample it is shown is a multiple of 2^-G inside [0, 1]."""

    def __init__(self, inner, bits=G):
        super().__init__()
        self.inner, self.bits, self.rows = inner, bits, 0

    def forward(self, x):
        scaled = x.detach().double() * 2.0 ** self.bits
        assert bool((scaled == scaled.round()).all()) and float(x.min()) >= 0.0 and float(x.max()) <= 1.0
        self.rows += x.shape[0]
        return self.inner(x)


def dyadic_case(B=8, T=200, seed=1, checked=True):
    """(model, x, y) on which every forwarded sample and every logit is exact, so a float32 device and this table must agree to
    the byte.  x lies on the grid 2^-6 inside [0, 1], weights are small integer multiples of 2^-6 and the scalar bias lies on the
    grid 2^-16 (the median of the rows' logits: rows on both sides, so every row has a donor); delta_rel, delta_min and the step
    schedule are powers of two (DYADIC).  With R = search_steps, K = step_trials, xi_rel = 2^-1:

      * a donor is a row of x: grid 2^-6, and dist = max |cur - x| lies on cur's grid;
      * a boundary search halves [0, dist] R times: its probes and the cur it leaves lie R bits deeper than the cur it began with;
      * the probes of an estimate are cur +- max(dist 2^-2, 2^-12): 2 bits deeper than cur (at least 12), never kept;
      * a candidate is cur +- dist 2^-1 2^-k, k < K: 1 + (K - 1) bits deeper than cur.

    So cur lies on 2^-(6 + R) after the opening search and each iteration adds R + 1 + (K - 1) bits: the deepest bit of anything
    forwarded is G = 6 + R + steps (R + K) = 24 at R = 3, K = 2, steps = 3 (the last iteration's probes, at G - R - K + 2,
    are shallower than its search).  Every sample lies in [0, 1], so 24 fractional bits fit float32's significand: NO sample
    arithmetic rounds, and sums like lo + hi < 2 of radii on the grid 2^-23 fit too.  A product with a weight has at most G + 6
    fractional bits and magnitude < 2^-4, and a logit sums T <= 256 of them: below 2^4 with 30 fractional bits, G + 6 + 4 = 34
    <= 52 — exact in the detector's float64 in ANY order of summation, then rounded once to float32, the same way everywhere.
    `checked` wraps the detector in GridChecked, which asserts the grid for every forwarded row at run time.  The labels are the clean
    classes except row 0's, which is wrong from the start."""
    assert T <= 256
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 2 ** X_BITS + 1, (B, T), generator=g).float() / 2.0 ** X_BITS
    w = (torch.randint(1, 4, (T,), generator=g) * (torch.randint(0, 2, (T,), generator=g) * 2 - 1)).float() / 64.0
    z = x.double() @ w.double()
    bias = -(torch.round(z.median() * 65536.0) / 65536.0).reshape(1)
    model = LinearDetector(w, bias)
    y = (model(x).reshape(-1) > 0).long()
    y[0] = 1 - y[0]
    return (GridChecked(model) if checked else model), x, y
