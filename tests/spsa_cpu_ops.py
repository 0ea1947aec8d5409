"""TEST INFRASTRUCTURE — the SPSA entry points of hip_ops (spsa_probe, spsa_step; include/advstep_spsa.h) restated on the CPU in
numpy float32 WITH THE KERNELS' OPERATION ORDER, and the direction bits restated with tests.apgd_cpu_ops' Philox; every other
op is tests.radius_cpu_ops' (whose LinearDetector the end-to-end tests run on).  Inputs may live on any device; results go back to
the input's device, so the table can stand in for hip_ops inside torchattacks.SPSA.

Everything in both kernels is an exact-order float32 computation: a probe sample is ONE rounded addition of +-delta and a clamp;
the step's d_j is one rounded subtraction, g its left-to-right float32 sum of +-d_j, and the move is the three roundings of the
PGD L-inf step.  numpy float32 arithmetic rounds each of these the same way, so the GPU tests compare BYTES with this table, with
no tolerance."""
import numpy as np
import torch

from tests import radius_cpu_ops as _base
from tests.apgd_cpu_ops import _c, _emit, philox4x32_10
from tests.radius_cpu_ops import LinearDetector  # noqa: F401  (re-exported)

NAME = "spsa_cpu"
MAX_DIRECTIONS = 1024      # ADVSTEP_SPSA_MAX_DIRECTIONS of include/advstep_spsa.h


def __getattr__(name):  # every op this table does not restate
    return getattr(_base, name)


# ---- the directions --------------------------------------------------------------------------------------------------------------

def direction_bits(B, T, j, seed, offset=0):
    """(B, T) bool: True where v_j[b, t] = -1.  q = t >> 2, k = t & 3, O = offset + (j >> 5);
    R = philox4x32_10(lo32(q), b, lo32(O), hi32(O), lo32(seed), hi32(seed)); bit i = 4 (j & 31) + k of R is word i >> 5, bit i & 31."""
    O = (int(offset) + (int(j) >> 5)) & 0xFFFFFFFFFFFFFFFF
    Q = (T + 3) // 4
    q, b = np.meshgrid(np.arange(Q, dtype=np.uint32), np.arange(B, dtype=np.uint32))
    r = philox4x32_10(q, b, np.full(q.shape, O & 0xFFFFFFFF, np.uint32), np.full(q.shape, O >> 32, np.uint32),
                      seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    i0 = 4 * (int(j) & 31)
    word = r[i0 >> 5]                                                # the 4 bits of a quad never straddle a word
    bits = np.stack([(word >> np.uint32((i0 & 31) + k)) & np.uint32(1) for k in range(4)], axis=-1)
    return np.ascontiguousarray(bits.reshape(B, Q * 4)[:, :T]).astype(bool)


def directions(B, T, j, seed, offset=0):
    """(B, T) float32 of +1 / -1: v_j."""
    return np.where(direction_bits(B, T, j, seed, offset), np.float32(-1.0), np.float32(1.0))


# ---- float32 helpers with the kernels' semantics ------------------------------------------------------------------------------------

def _clamp(v, lo, hi):
    """clampf of csrc/advstep_common.h: v < lo ? lo : v, then v > hi ? hi : v — a NaN stays."""
    v = np.where(v < np.float32(lo), np.float32(lo), v)
    return np.where(v > np.float32(hi), np.float32(hi), v).astype(np.float32)


def _sgn(g):
    """torch.sign: NaN and +-0 give 0."""
    return (g > 0).astype(np.float32) - (g < 0).astype(np.float32)


def pgd_linf_step_np(adv, g, orig, alpha, eps, lo=0.0, hi=1.0):
    a = (adv + np.float32(alpha) * _sgn(g)).astype(np.float32)
    d = _clamp((a - orig).astype(np.float32), -np.float32(eps), np.float32(eps))
    return _clamp((orig + d).astype(np.float32), lo, hi)


# ---- the two ops in numpy ------------------------------------------------------------------------------------------------------------

def spsa_probe_np(adv, delta, seed, offset=0, s0=0, ns=1, lo=0.0, hi=1.0):
    """(ns, B, T) float32 from adv (B, T) float32."""
    B, T = adv.shape
    out = np.empty((ns, B, T), np.float32)
    for i, s in enumerate(range(s0, s0 + ns)):
        if s == 0:
            out[i] = adv
            continue
        m = np.float32(delta) if s & 1 else -np.float32(delta)
        out[i] = _clamp((adv + np.where(direction_bits(B, T, (s - 1) >> 1, seed, offset), -m, m)).astype(np.float32), lo, hi)
    return out


def fooled_rows(z0, labels):
    """(B,) bool: (z[0, b] > 0) != (labels[b] == 1)."""
    return (z0 > 0) != (labels == 1)


def spsa_gradient_np(z, labels, T, seed, offset=0):
    """(B, T) float32: g = ((+-d_0) +- d_1) +- ... for every row, fooled or not; zeros for n = 0."""
    S, B = z.shape
    n = (S - 1) // 2
    g = np.zeros((B, T), np.float32)
    with np.errstate(invalid="ignore"):
        for j in range(n):
            diff = (z[1 + 2 * j] - z[2 + 2 * j]).astype(np.float32)
            d = np.where(labels == 1, -diff, diff).astype(np.float32)[:, None]
            t = np.where(direction_bits(B, T, j, seed, offset), -d, d).astype(np.float32)
            g = t if j == 0 else (g + t).astype(np.float32)
    return g


def spsa_step_np(adv, orig, z, labels, queries, alpha, eps, seed, offset=0, lo=0.0, hi=1.0):
    """(out (B, T) float32, queries (B,) int32)."""
    S, B = z.shape
    fooled = fooled_rows(z[0], labels)
    g = spsa_gradient_np(z, labels, adv.shape[1], seed, offset)
    with np.errstate(invalid="ignore"):
        moved = pgd_linf_step_np(adv, g, orig, alpha, eps, lo, hi)
    out = moved.copy()
    out[fooled] = adv[fooled]                                         # byte for byte
    return out, (queries + np.where(fooled, 0, S)).astype(np.int32)


# ---- the table's ops -----------------------------------------------------------------------------------------------------------------

def _np2(t):
    a = _c(t).numpy()
    return a.reshape(a.shape[0], -1)


def spsa_probe(adv, delta, seed, offset=0, s0=0, ns=1, lo=0.0, hi=1.0, out=None):
    res = torch.from_numpy(spsa_probe_np(_np2(adv), delta, seed, offset, s0, ns, lo, hi))
    if out is not None:
        with torch.no_grad():
            out.copy_(res.reshape(out.shape).to(out.device))
        return out
    return res.reshape((ns,) + tuple(adv.shape)).to(adv.device)


def spsa_step(adv, orig, z, labels, queries, alpha, eps, seed, offset=0, lo=0.0, hi=1.0, out=None):
    res, q = spsa_step_np(_np2(adv), _np2(orig), _c(z).numpy(), _c(labels).numpy().reshape(-1), _c(queries).numpy().reshape(-1),
                          alpha, eps, seed, offset, lo, hi)
    with torch.no_grad():
        queries.copy_(torch.from_numpy(q).reshape(queries.shape).to(queries.device))
    return _emit(torch.from_numpy(res), adv, out)


# ---- the exact end-to-end case -----------------------------------------------------------------------------------------------------

DYADIC = {"eps": 2.0 ** -6, "alpha": 2.0 ** -8, "delta": 2.0 ** -7, "steps": 6, "nb_sample": 4}


def dyadic_case(B=8, T=200, seed=1):
    """(model, x, y) on which every logit and every step is exact, so a float32 device and this table must agree to the byte:
    x on the grid 2^-10 inside [0, 1], weights small integer multiples of 2^-6, a scalar bias on the grid 2^-16 (the median of
    the rows' logits, so that rows lie on both sides and at every distance), eps, alpha and delta powers of two (DYADIC).
    Samples then stay on the grid 2^-10, products on 2^-16, and a logit is a sum of T <= 256 such products of magnitude
    < 2^-4 each: below 2^4 with 16 fractional bits — exact in the detector's float64 in ANY order of summation, and then
    rounded once to float32, the same way everywhere.  The labels are the clean classes except row 0's, which is wrong from the
    start."""
    assert T <= 256
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 1025, (B, T), generator=g).float() / 1024.0
    w = (torch.randint(1, 4, (T,), generator=g) * (torch.randint(0, 2, (T,), generator=g) * 2 - 1)).float() / 64.0
    z = x.double() @ w.double()
    bias = -(torch.round(z.median() * 65536.0) / 65536.0).reshape(1)
    model = LinearDetector(w, bias)
    y = (model(x).reshape(-1) > 0).long()
    y[0] = 1 - y[0]
    return model, x, y
