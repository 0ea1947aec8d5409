"""TEST INFRASTRUCTURE — the two entry points of include/advstep_smooth.h restated in numpy on the CPU, from tests.apgd_cpu_ops'
Philox: the noisy copies in a float32 form (the kernel's expressions, libm where the device has hardware transcendentals: not
bit-identical, ~1e-6) and a float64 form (the exact uniforms, then Box-Muller and the sum in float64: what the device's error is
measured against), and the vote count.  Also here: the analytic linear case whose true L2 radii are known in closed form."""
import numpy as np
import torch

from tests.apgd_cpu_ops import _u01, philox4x32_10
from tests.radius_cpu_ops import LinearDetector

NAME = "smooth_cpu"
MASK32 = 0xFFFFFFFF


def normals_np(B, T, seed, counter, dtype=np.float32):
    """(B, T) standard normals of one slot: the mapping of philox_draw's L2 branch (quad q = t >> 2 and row b in the counter's low
    words, Box-Muller on two uniform pairs) at the 64-bit counter `counter` = offset + s, which carries into the high word."""
    counter = int(counter) & 0xFFFFFFFFFFFFFFFF
    Q = (T + 3) // 4
    q, b = np.meshgrid(np.arange(Q, dtype=np.uint32), np.arange(B, dtype=np.uint32))
    r = philox4x32_10(q, b, np.full(q.shape, counter & MASK32, np.uint32), np.full(q.shape, counter >> 32, np.uint32),
                      seed & MASK32, (seed >> 32) & MASK32)
    u0, u1, u2, u3 = _u01(r[0], True), _u01(r[1]), _u01(r[2], True), _u01(r[3])       # float32, exact (24-bit)
    if dtype == np.float32:
        two, tau = np.float32(-2.0), np.float32(6.283185307179586)
    else:
        u0, u1, u2, u3 = (u.astype(np.float64) for u in (u0, u1, u2, u3))
        two, tau = -2.0, 2.0 * np.pi
    r0, r1 = np.sqrt(two * np.log(u0)), np.sqrt(two * np.log(u2))
    t0, t1 = tau * u1, tau * u3
    n = np.stack([r0 * np.cos(t0), r0 * np.sin(t0), r1 * np.cos(t1), r1 * np.sin(t1)], axis=-1).astype(dtype)
    return np.ascontiguousarray(n.reshape(B, Q * 4)[:, :T])


def smooth_noise_np(x, sigma, seed, offset=0, s0=0, ns=1, dtype=np.float32):
    """(ns, B, T): out[s - s0] = x + sigma * z(offset + s).  float32: fl(x + fl(sigma * z)) as the kernel rounds; float64: the
    float32 inputs (x, sigma) taken exactly, everything after them in float64."""
    x = np.asarray(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x, dtype=np.float32)
    B = x.shape[0]
    flat = x.reshape(B, -1)
    T = flat.shape[1]
    sig = np.float32(sigma)
    out = np.empty((ns, B, T), dtype=dtype)
    for i in range(ns):
        z = normals_np(B, T, seed, int(offset) + int(s0) + i, dtype)
        out[i] = flat + sig * z if dtype == np.float32 else flat.astype(np.float64) + np.float64(sig) * z
    return out


def smooth_tally_np(z, counts):
    """counts + #{s : z[s, b] > 0} (int32); NaN, +-0 and negatives are class 0."""
    z = np.asarray(z.detach().cpu().numpy() if isinstance(z, torch.Tensor) else z, dtype=np.float32)
    counts = np.asarray(counts.detach().cpu().numpy() if isinstance(counts, torch.Tensor) else counts, dtype=np.int32)
    with np.errstate(invalid="ignore"):
        return (counts + (z > 0).sum(axis=0).astype(np.int32)).astype(np.int32)


# ---- the analytic case ---------------------------------------------------------------------------------------------------------------

LINEAR_K = (0.0, 0.25, 0.5, 1.0, 1.5, 2.0, 3.0, -1.0)
LINEAR_SIGMA = 0.01


class SlotLinearDetector(LinearDetector):
    """radius_cpu_ops.LinearDetector (z = x . w + bias in float64, rounded once) with its per-row bias repeated over the slots
    of a slot-major (S * B, T) batch: row i of a forward is utterance i % B."""

    def forward(self, x):
        B = self.bias.numel()
        return (x.double() @ self.w + self.bias.repeat(x.shape[0] // B)).float().unsqueeze(1)


def linear_case(T, sigma=LINEAR_SIGMA):
    """(model, x (8, T), labels, k, sigma): w as in radius_cpu_ops.analytic_case at seed 0 (no zeros, ||w||_2 = 64), x = rand *
    0.5 - 0.25 from the same generator, and a bias per row that puts the clean logit at k * sigma * ||w||_2 for k = LINEAR_K.  The
    detector is linear, so row b's decision changes exactly at L2 distance |k_b| * sigma: its TRUE radius.  Labels are the clean
    classes (k > 0 is class 1; the k = 0 row, on the boundary, is labelled 0)."""
    g = torch.Generator().manual_seed(0)
    w = (torch.rand(T, generator=g) + 0.5) * (torch.randint(0, 2, (T,), generator=g) * 2 - 1).float()
    w = (w.double() * (64.0 / w.double().norm())).float()
    B = len(LINEAR_K)
    x = torch.rand(B, T, generator=g) * 0.5 - 0.25
    k = torch.tensor(LINEAR_K, dtype=torch.float64)
    bias = k * float(np.float32(sigma)) * w.double().norm() - x.double() @ w.double()
    return SlotLinearDetector(w, bias), x, (k > 0).long(), k, sigma
