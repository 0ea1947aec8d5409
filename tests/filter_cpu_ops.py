"""TEST INFRASTRUCTURE — the universal-filter entry points of hip_ops (filter_apply, filter_tap_grad, filter_tap_update;
include/advstep_filter.h) restated on the CPU: the float32 twin of filter_apply in the ABI's order (its BYTES are the reference),
the float64 twins of the tap gradient and of the Adam step from the float32 operands, the bound the tap gradient is held to, the
inputs the CPU and the GPU tests share, and the fit on a linear detector restated in either precision.

THE BOUND OF THE TAP GRADIENT (u = 2^-24; no constant here was measured).

The operands are float32: gm (the model's gradient or 0) and xc = fl(x - c), the centred sample AS THE ABI DEFINES IT (one float32
subtraction; the float64 twin takes that float32 value, so xc is an operand, not an error source).  gm xc is exact in float64.  The
kernels add the terms of dh[i] in the order the header documents, with one rounding per term (fmaf: the product is not rounded
on its own) and additions of an exact +0 at the start of every partial, which round nothing:
    thread      a chain of at most 16 CPS fused multiply-adds over its segment of a tile, CPS = ceil(ceil(n / 16) / NS) chunks of 16
                samples, NS = floor(256 / TL) segments, TL = ceil(L / 16) tap lanes, n = min(T, 4096) the samples of a full tile;
    workgroup   NS additions of the segments' sums;
    tile, row   C = ceil(T / 4096) additions of a row's tiles;
    row group   at most min(B, 16) additions of a group's rows, then ceil(B / 16) additions of the groups.
A term therefore passes through at most
    D = 16 CPS + NS + C + min(B, 16) + ceil(B / 16)
rounded additions, each of which errs by at most u times the magnitude of its result, itself at most the sum of the |terms| below
it.  To first order |dh - dh64| <= D u sum |gm xc|; the second-order remainder is below (D u)^2 / 2 of the same sum, which is less
than the one u that
    tap_grad_tolerance = (D + 1) u sum_b sum_t |gm xc|
leaves for it while D^2 u < 2, i.e. D < 5 792: the thread and workgroup part is at most 16 * 17 + 256, so only a batch of tens
of thousands of rows or rows of millions of samples gets there (the tests' largest D is 312; test_filter_host.py asserts the
condition for every shape they use).  The bound is per tap and uses no property of the data.  (The test's operands are of normal size: nothing
underflows.)  At (3, 4100, 17) D = 16 * 2 + 128 + 2 + 3 + 1 = 166; at (128, 64 600, 255) D = 256 + 16 + 16 + 16 + 8 = 312.

filter_apply rounds every product and sum on its own in the ABI's order; numpy float32 does the same, so the twin gives the
kernel's bytes and the GPU test allows no tolerance.  Against exact arithmetic it errs by at most (L + 2) u (|c| + sum_i |h_i xc|)
to first order (L products, L additions of the accumulator and the one of c; the clamp is 1-Lipschitz): `apply_tolerance`, which
the host test holds the twin to, with the same +1 for the second order.
"""
import numpy as np
import torch

U = 2.0 ** -24
MAX_TAPS = 1025       # ADVSTEP_FILTER_MAX_TAPS
GROUP_ROWS = 16       # ADVSTEP_FILTER_GROUP_ROWS
TILE = 4096


def _np32(t):
    return np.ascontiguousarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t, dtype=np.float32)


def _window(x, center, P, dtype):
    """xc padded with P zeros (silence) at either end, (B, T + 2 P): xc = fl32(x - c), then `dtype`."""
    x, c = _np32(x), _np32(center).reshape(-1, 1)
    xp = np.zeros((x.shape[0], x.shape[1] + 2 * P), dtype=dtype)
    xp[:, P:P + x.shape[1]] = (x - c).astype(dtype)
    return xp


def _mask(row_mask, B):
    return np.ones(B, dtype=bool) if row_mask is None else (_np32(row_mask).reshape(-1) != 0)


# ---- filter_apply ------------------------------------------------------------------------------------------------------------------

def filter_apply_np(x, center, taps, row_mask=None, lo=0.0, hi=1.0):
    """The float32 twin, in the ABI's order: acc = 0; acc = acc + h[i] * xc[t + P - i] for i = 0 .. L-1; clamp(c + acc)."""
    x, h = _np32(x), _np32(taps).reshape(-1)
    B, T = x.shape
    L = h.size
    P = (L - 1) // 2
    xp = _window(x, center, P, np.float32)
    acc = np.zeros((B, T), dtype=np.float32)
    for i in range(L):
        acc = acc + h[i] * xp[:, 2 * P - i:2 * P - i + T]
    c = _np32(center).reshape(-1, 1)
    out = np.minimum(np.maximum(c + acc, np.float32(lo)), np.float32(hi)).astype(np.float32)
    keep = ~_mask(row_mask, B)
    out[keep] = x[keep]
    return out


def filter_apply_ref64(x, center, taps, row_mask=None, lo=0.0, hi=1.0, parts=False):
    """The same in float64 from the float32 operands; with parts also |c| + sum_i |h_i xc| per sample."""
    x, h = _np32(x), _np32(taps).reshape(-1).astype(np.float64)
    B, T = x.shape
    P = (h.size - 1) // 2
    xp = _window(x, center, P, np.float64)
    acc, mag = np.zeros((B, T)), np.zeros((B, T))
    for i in range(h.size):
        term = h[i] * xp[:, 2 * P - i:2 * P - i + T]
        acc += term
        mag += np.abs(term)
    c = _np32(center).reshape(-1, 1).astype(np.float64)
    out = np.clip(c + acc, lo, hi)
    keep = ~_mask(row_mask, B)
    out[keep] = x[keep]
    return (out, np.abs(c) + mag) if parts else out


def apply_tolerance(L, mag):
    return (L + 3) * U * mag


# ---- the tap gradient --------------------------------------------------------------------------------------------------------------

def tap_grad_ref64(x, center, grad, out_adv, L, row_mask=None, lo=0.0, hi=1.0, parts=False, drop=None):
    """(L,) float64: dh[i] = sum_b sum_t gm[b, t] xc[b, t + P - i] with gm = grad where the row is unmasked and lo < out_adv < hi
    (STRICT), else 0; with parts also sum |gm xc|.  drop = (tile, row): that workgroup's partial is left out."""
    x, g, y = _np32(x), _np32(grad).astype(np.float64), _np32(out_adv)
    B, T = x.shape
    P = (L - 1) // 2
    xp = _window(x, center, P, np.float64)
    live = (y > np.float32(lo)) & (y < np.float32(hi)) & _mask(row_mask, B).reshape(-1, 1)
    gm = np.where(live, g.reshape(B, T), 0.0)
    if drop is not None:
        gm[drop[1], drop[0] * TILE:(drop[0] + 1) * TILE] = 0.0
    dh, mag = np.zeros(L), np.zeros(L)
    for i in range(L):
        term = gm * xp[:, 2 * P - i:2 * P - i + T]
        dh[i] = term.sum()
        mag[i] = np.abs(term).sum()
    return (dh, mag) if parts else dh


def chain_length(B, T, L):
    """D of the module docstring: the most rounded additions a term of dh passes through."""
    n = min(T, TILE)
    TL = -(-L // 16)
    NS = 256 // TL
    CPS = -(-(-(-n // 16)) // NS)
    return 16 * CPS + NS + -(-T // TILE) + min(B, GROUP_ROWS) + -(-B // GROUP_ROWS)


def tap_grad_tolerance(B, T, L, abs_sum):
    return (chain_length(B, T, L) + 1) * U * abs_sum


# ---- the Adam step -----------------------------------------------------------------------------------------------------------------

def adam_step(h, m, v, dh, step, lr, beta1=0.9, beta2=0.999, adam_eps=1e-8, ascend=True, dtype=np.float64):
    """One step in `dtype`, expression by expression as include/advstep_filter.h states it: the bias corrections formed in double
    and applied as `dtype` scalars.  Returns (h, m, v)."""
    f = dtype
    h, m, v, dh = (np.asarray(a, dtype=f) for a in (h, m, v, dh))
    g = -dh if ascend else dh
    w1, b2, omb2 = f(1.0 - beta1), f(beta2), f(1.0 - beta2)
    neg_step, bc2_sqrt, eps = f(-(lr / (1.0 - beta1 ** step))), f(np.sqrt(1.0 - beta2 ** step)), f(adam_eps)
    m = m + w1 * (g - m)
    v = v * b2 + (omb2 * g) * g
    h = h + neg_step * (m / (np.sqrt(v) / bc2_sqrt + eps))
    return h.astype(f), m.astype(f), v.astype(f)


# ---- the inputs the CPU and the GPU tests share ------------------------------------------------------------------------------------

T_SWEEP, L_SWEEP, B_SWEEP = (1, 16, 255, 4095, 4096, 4097, 4100), (1, 3, 17, 255, 257, 1025), (1, 3, 17)


def shapes():
    """Every T at L = 17 and 255, every L at T = 255 and 4100 (T < L included), B cycling through 1, 3, 17, and one production row."""
    seen, out = set(), []
    for T, L in [(T, L) for T in T_SWEEP for L in (17, 255)] + [(T, L) for L in L_SWEEP for T in (255, 4100)]:
        if (T, L) not in seen:
            seen.add((T, L))
            out.append((B_SWEEP[len(out) % 3], T, L))
    return out + [(4, 64_600, 255)]


def case(B, T, L, seed=None):
    """x in [0, 1] with exact 0s and 1s, centres inside the range, a filter of gain > 1 (so some outputs clip at either end), a row
    mask that keeps row 0 and drops the odd rows, and a gradient with zeros.  Float32 CPU tensors."""
    g = torch.Generator().manual_seed(1000 * B + 7 * T + L if seed is None else seed)
    x = torch.rand(B, T, generator=g)
    x[:, ::17] = 0.0
    x[:, 5::19] = 1.0
    center = torch.rand(B, generator=g) * 0.4 + 0.3
    taps = torch.randn(L, generator=g) * (0.5 / np.sqrt(L))
    taps[(L - 1) // 2] = 1.25 + 0.1 * taps[(L - 1) // 2]        # a centre tap > 1: the rows' exact 0s and 1s leave [0, 1] even at L = 1
    mask = torch.tensor([1.0 if b % 2 == 0 else 0.0 for b in range(B)])
    grad = torch.randn(B, T, generator=g)
    grad[:, ::11] = 0.0
    return x, center, taps, mask, grad


# ---- the attack on a linear detector ------------------------------------------------------------------------------------------------

FIT = {"taps": 17, "lr": 0.02, "steps": 40}


class RevertedLinear(torch.nn.Module):
    """z_b = <v, x01_b (mx_b - mn_b) + mn_b>: a linear detector of the WAVEFORM, given the min-max domain's rows like every attacked
    model (the loop reverts before the detector; here the model does, with the mn, mx of `set_minmax`), accumulated in float64."""

    def __init__(self, v):
        super().__init__()
        self.v = torch.nn.Parameter(v.clone().double())
        self.mn = self.mx = None

    def set_minmax(self, mn, mx):
        self.mn, self.mx = mn.double().reshape(-1, 1), mx.double().reshape(-1, 1)

    def forward(self, x01):
        wave = x01.double() * (self.mx - self.mn) + self.mn
        return (wave @ self.v).float().unsqueeze(1)


def linear_case(T, seed, rows=8, spoof_only=False):
    """(waveform (rows, T), labels, v): 0.3 randn + (2 y - 1) 0.2 sin(2 pi 0.11 t), labels alternating spoof (0) / bonafide (1) or all
    spoof; v = (8 / T) sin(2 pi 0.11 t), so z = <v, waveform> is about -0.8 for a spoof row and +0.8 for a bonafide one."""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(T, dtype=torch.float64)
    tone = torch.sin(2 * np.pi * 0.11 * t)
    y = torch.zeros(rows, dtype=torch.int64) if spoof_only else torch.tensor([b % 2 for b in range(rows)])
    wave = 0.3 * torch.randn(rows, T, generator=g, dtype=torch.float64) + (2.0 * y.double().reshape(-1, 1) - 1.0) * 0.2 * tone
    return wave.float(), y, ((8.0 / T) * tone).float()


def minmax(wave):
    """(x01, mn, mx) as to_minmax forms them, float32."""
    mn, mx = wave.min(dim=1, keepdim=True).values, wave.max(dim=1, keepdim=True).values
    return (wave - mn) / (mx - mn), mn, mx


def fit_restated(x01, y, mn, mx, v, taps, lr, steps, dtype, source_label=0):
    """torchattacks.UniversalFilter's fit on RevertedLinear(v), restated in numpy `dtype`: per step the filter, the logit, the
    closed-form gradient of the mean cross-entropy of cat([-z, z]) (dz_b = (2 / B)(sigmoid(2 z_b) - y_b)), the masked correlation
    and the Adam ascent.  Returns the taps (L,)."""
    f = dtype
    x, yv, v = _np32(x01).astype(f), np.asarray(y).astype(f), _np32(v).astype(f)
    mn, mx = _np32(mn).reshape(-1, 1).astype(f), _np32(mx).reshape(-1, 1).astype(f)
    B, T = x.shape
    L, P = taps, (taps - 1) // 2
    c = (-mn / (mx - mn)).astype(f)
    live_row = (np.asarray(y) == source_label).reshape(-1, 1)
    xp = np.zeros((B, T + 2 * P), dtype=f)
    xp[:, P:P + T] = x - c
    h, m, s = np.zeros(L, dtype=f), np.zeros(L, dtype=f), np.zeros(L, dtype=f)
    h[P] = 1.0
    for step in range(1, steps + 1):
        acc = np.zeros((B, T), dtype=f)
        for i in range(L):
            acc = acc + h[i] * xp[:, 2 * P - i:2 * P - i + T]
        adv = np.where(live_row, np.clip(c + acc, f(0), f(1)), x).astype(f)
        z = (adv * (mx - mn) + mn) @ v
        dz = (f(2.0) / f(B)) * (f(1.0) / (f(1.0) + np.exp(-f(2.0) * z)) - yv)
        grad = dz.reshape(-1, 1) * v.reshape(1, -1) * (mx - mn)
        gm = np.where(live_row & (adv > 0) & (adv < 1), grad, f(0)).astype(f)
        dh = np.array([(gm * xp[:, 2 * P - i:2 * P - i + T]).sum() for i in range(L)], dtype=f)
        h, m, s = adam_step(h, m, s, dh, step, lr, dtype=f)
    return h
