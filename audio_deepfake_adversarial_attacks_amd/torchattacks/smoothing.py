"""Randomized smoothing (Cohen, Rosenfeld and Kolter, ICML 2019): the one procedure here that is not an attack.  An attack
witnesses an UPPER bound on an utterance's minimal adversarial radius; smoothing certifies a LOWER bound, for the detector
g(x) = the majority class of f(x + N(0, sigma^2 I)), without retraining f.  It sits beside `Channel` and `MaskingModel`: the
evaluation loop uses it through `generate_attacks(..., certify=sigma)`, and the statistics that turn its counts into a radius
are host-side float64 in `metrics` (`clopper_pearson_lower`, `certified_radius`, `smoothed_prediction`)."""
import math

import torch


class Smoothing:
    r"""Votes of a one-logit detector over Gaussian-noised copies of a batch, counted on the device.

    The copies of a (B, ...) batch are SLOTS, slot-major (S, B, ...) like SPSA's probes: copy s is x + sigma * z with z the
    standard normals `hip_ops.smooth_noise` regenerates from Philox at counter `offset + s` under the key `seed`
    (include/advstep_smooth.h has the mapping).  Nothing is stored but the chunk being forwarded:

        1. `ops.smooth_noise` fills whole slots, in chunks of at most `max_rows` forward rows;
        2. the model scores each chunk under `torch.no_grad()`;
        3. `ops.smooth_tally` adds the chunk's class-1 votes (logit > 0; NaN is class 0) to a (B,) int32 counter.

    There is no host read anywhere.  `sigma` is in the unit of the tensors passed in and is the same for every input: the
    smoothed detector is ONE function, so its noise level cannot depend on the utterance.  The noise is float32 (Box-Muller on
    24-bit uniforms, |z| <= 5.77), as in every float32 implementation of smoothing.

    A caller owns the offsets: copies are independent as long as no two votes of a run share (seed, offset + s).  `certify`
    consumes `n0 + n` offsets from `offset`, `predict` consumes `n0` (the `slots_*` properties).

    Arguments:
        sigma (float): noise level, > 0.
        n (int): estimation copies of CERTIFY. (Default: 1000)
        n0 (int): selection copies of CERTIFY, and the copies of PREDICT. (Default: 100)
        alpha (float): failure probability of a certificate, in (0, 1). (Default: 0.001)
        max_rows (int): forward rows per model call. (Default: 1024, SPSA's)
        seed (int): the Philox key. (Default: 0)

    Examples::
        >>> smooth = torchattacks.Smoothing(sigma=0.05)
        >>> rows = smooth.certify(model, waveforms, offset=0)                  # (B, 2) int32: class, kA
        >>> radius = metrics.certified_radius(rows[:, 1].cpu().numpy(), smooth.n, smooth.alpha, smooth.sigma)
    """

    def __init__(self, sigma, n=1000, n0=100, alpha=0.001, max_rows=1024, seed=0):
        if not (float(sigma) > 0.0 and math.isfinite(float(sigma))):       # (a NaN sigma fails the comparison)
            raise ValueError(f"sigma must be a finite noise level > 0, got {sigma}")
        if int(n) < 1 or int(n0) < 1 or int(max_rows) < 1:
            raise ValueError(f"n, n0 and max_rows must be at least 1, got {n}, {n0} and {max_rows}")
        if not 0.0 < float(alpha) < 1.0:
            raise ValueError(f"alpha must lie inside (0, 1), got {alpha}")
        self.sigma, self.n, self.n0, self.alpha = float(sigma), int(n), int(n0), float(alpha)
        self.max_rows, self.seed = int(max_rows), int(seed)
        self._ops = None

    @property
    def ops(self):
        """Waveform op table; the HIP kernels, bound at the first use (as `Attack.ops`)."""
        if self._ops is None:
            from .. import hip_ops
            hip_ops._lib.load()
            self._ops = hip_ops
        return self._ops

    @ops.setter
    def ops(self, table):
        self._ops = table

    @property
    def slots_certify(self):
        """n0 + n: the offsets (and model queries per utterance) of one `certify` call."""
        return self.n0 + self.n

    @property
    def slots_predict(self):
        """n0: the offsets of one `predict` call."""
        return self.n0

    @staticmethod
    def _score(model, x):
        z = model(x)
        if z.dim() != 2 or z.shape[1] != 1:
            raise ValueError(f"the smoothed model must emit one logit per utterance, got {tuple(z.shape)}")
        return z.reshape(-1)

    def votes(self, model, x, m, offset, post=None):
        """(B,) int32 on the device: how many of the `m` copies at offsets `offset .. offset + m - 1` the model puts in class 1.
        `post`: a transformation between the noisy waveform and the model (the loop's preprocessing), or None."""
        ops, m = self.ops, int(m)
        B = x.shape[0]
        T = x.numel() // B if B else 0
        flat = x.reshape(B, T).contiguous()
        counts = torch.zeros(B, dtype=torch.int32, device=x.device)
        if B == 0 or m == 0:
            return counts
        max_rows = self.max_rows
        per_chunk = max(1, min(m, max_rows // B))                    # slots per fill
        copies = torch.empty((per_chunk, B) + tuple(x.shape[1:]), dtype=torch.float32, device=x.device)
        z = torch.empty(per_chunk * B, dtype=torch.float32, device=x.device)
        with torch.no_grad():
            for s0 in range(0, m, per_chunk):
                ns = min(per_chunk, m - s0)
                chunk = copies[:ns]
                ops.smooth_noise(flat, self.sigma, self.seed, offset, s0=s0, ns=ns, out=chunk)
                rows = chunk.reshape((ns * B,) + tuple(x.shape[1:]))
                for r0 in range(0, ns * B, max_rows):                # one piece unless a single slot exceeds max_rows
                    piece = rows[r0:r0 + max_rows]
                    z[r0:r0 + piece.shape[0]] = self._score(model, post(piece) if post is not None else piece)
                ops.smooth_tally(z[:ns * B].reshape(ns, B), counts)
        return counts

    def certify(self, model, x, offset, post=None):
        """Cohen's CERTIFY up to its statistics: (B, 2) int32 on the device, (class, kA).  `n0` copies pick the class — class 1
        when 2 * c0 > n0, a tie goes to class 0 — and `n` FRESH copies at offsets `offset + n0 .. offset + n0 + n - 1` give kA,
        the count of that class.  `metrics.certified_radius(kA, n, alpha, sigma)` is the radius, or the abstention."""
        c0 = self.votes(model, x, self.n0, offset, post)
        c1 = self.votes(model, x, self.n, offset + self.n0, post)
        cls = (2 * c0 > self.n0).to(torch.int32)
        return torch.stack([cls, torch.where(cls == 1, c1, self.n - c1)], dim=1)

    def predict(self, model, x, offset, post=None):
        """Cohen's PREDICT up to its test: (B, 2) int32 on the device, (c1, n0), the class-1 votes among `n0` copies at offsets
        `offset .. offset + n0 - 1`.  `metrics.smoothed_prediction(c1, n0, alpha)` is the class, or the abstention."""
        c1 = self.votes(model, x, self.n0, offset, post)
        return torch.stack([c1, torch.full_like(c1, self.n0)], dim=1)
