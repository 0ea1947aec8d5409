"""SmoothAdvPGD: PGD on the smoothed detector (no counterpart in the reference)."""
import math

import torch

from ..attack import Attack


class SmoothAdvPGD(Attack):
    r"""SmoothAdv, 'Provably Robust Deep Learning via Adversarially Trained Smoothed Classifiers' (Salman et al., NeurIPS 2019)
    [https://arxiv.org/abs/1906.04584]: PGD against g(x) = the majority class of f(x + N(0, sigma^2 I)), the detector that
    `torchattacks.Smoothing` certifies.  A gradient of f at one point mostly ignores g; this attack differentiates the
    Monte-Carlo estimate of g's soft score over `samples` noise draws,

        J(x') = -log( (1 / m) sum_i sigmoid(s f(x' + sigma z_i)) ),   s = 2 y - 1.

    Arguments:
        model (nn.Module): model to attack.
        eps (float): maximum perturbation, in the attack's domain. (Default: 0.1)
        alpha (float or None): step size; None is 2 * eps / steps, the paper's choice. (Default: None)
        steps (int): number of steps. (Default: 10)
        sigma (float): noise level of the smoothed detector, in the WAVEFORM's units, > 0. (Default: 0.05)
        samples (int): noise draws m per step. (Default: 8)
        norm (str): "L2" or "Linf". (Default: "L2")
        random_start (bool): using random initialization of delta, as PGDL2 / PGD draw it. (Default: True)
        fresh_noise (bool): new draws at every step instead of the paper's fixed ones. (Default: False)
        max_rows (int): forward rows per model call. (Default: 1024, Smoothing's)

    Per step:

        1. `ops.smoothadv_fill` writes the `samples` noised copies of the iterate, slot-major (m, B, T);
        2. the model scores them in whole-slot chunks formed exactly as `Smoothing.votes` forms them — the frontends' dB floor
           is batch-wide, so the attacked function is the detector as the certifier's chunks make it — giving z (m, B);
        3. `ops.smoothadv_loss_grad` gives J per row and dJ / dz, and autograd carries it back through each chunk into a
           (m, B, T) buffer;
        4. `ops.smoothadv_step` sums the slots in order and takes PGD's step in the same launch(es).

    The iterate lives in the min-max domain the loop attacks in, sigma and the certified detector in the waveform's.  The caller
    that normalised the utterance hands mn and mx over with `set_minmax(mn, mx)` before the call (`evaluation.attack_batch` does:
    `wants_minmax`); copy i is then revert(adv) + sigma z_i, what `Smoothing.votes` feeds the model, and the model is given
    waveform-domain rows.  Without them the copies are adv + sigma z_i.  The fill's Jacobian (mx - mn) I is a positive factor
    per row, and so is the cost's scale: the step normalises per row or takes signs, so both are dropped.

    The noise key is one `_fresh_seed()` per call; offsets 0 .. m - 1 are reused at every step (the paper's fixed draws; nothing
    is stored, they are regenerated), `fresh_noise=True` uses offsets step * m .. step * m + m - 1.  The key is never the
    certifier's: a perturbation computed from the certification noise would void the certificate's 1 - alpha statement.

    Out of scope: `replays_from_graph` stays False (the loop is eager, one batch in flight); momentum and APGD variants
    (`ops.smoothadv_step` returns the summed gradient they would start from); MultiAttack membership.

    Examples::
        >>> attack = torchattacks.SmoothAdvPGD(model, eps=0.1, steps=10, sigma=0.05, samples=8)
        >>> attack.set_minmax(mn, mx)
        >>> adv_images = attack(images, labels)
    """

    replays_from_graph = False
    wants_minmax = True

    def __init__(self, model, eps=0.1, alpha=None, steps=10, sigma=0.05, samples=8, norm="L2", random_start=True, fresh_noise=False,
                 max_rows=1024):
        super().__init__("SmoothAdvPGD", model)
        if not (float(sigma) > 0.0 and math.isfinite(float(sigma))):       # (a NaN sigma fails the comparison)
            raise ValueError(f"sigma must be a finite noise level > 0, got {sigma}")
        if int(steps) < 1 or int(samples) < 1 or int(max_rows) < 1:
            raise ValueError(f"steps, samples and max_rows must be at least 1, got {steps}, {samples} and {max_rows}")
        if norm not in ("L2", "Linf"):
            raise ValueError(f"norm must be 'L2' or 'Linf', got {norm!r}")
        if not (float(eps) >= 0.0 and math.isfinite(float(eps))):
            raise ValueError(f"eps must be a finite radius >= 0, got {eps}")
        if alpha is not None and not (float(alpha) >= 0.0 and math.isfinite(float(alpha))):
            raise ValueError(f"alpha must be a finite step size >= 0 or None, got {alpha}")
        self.eps = eps
        self.alpha = 2.0 * eps / int(steps) if alpha is None else alpha
        self.steps = int(steps)
        self.sigma = float(sigma)
        self.samples = int(samples)
        self.norm = norm
        self.random_start = random_start
        self.fresh_noise = bool(fresh_noise)
        self.max_rows = int(max_rows)
        self._supported_mode = ["default", "targeted"]
        self._minmax = None

    def set_minmax(self, mn, mx) -> None:
        """The per-utterance minimum and maximum `to_minmax` returned, (B,) or (B, 1), for the NEXT call only."""
        self._minmax = (mn, mx)

    def _affine(self, B, device):
        """(scale, shift) = (mx - mn, mn) per row on the device, or (None, None) when no min-max was handed over; consumes it."""
        minmax, self._minmax = self._minmax, None
        if minmax is None:
            return None, None
        mn, mx = (t.detach().to(device=device, dtype=torch.float32).reshape(-1) for t in minmax)
        if mn.numel() != B or mx.numel() != B:
            raise ValueError(f"set_minmax: mn / mx must hold one value per utterance ({B}), got {mn.numel()} / {mx.numel()}")
        return (mx - mn).contiguous(), mn.contiguous()

    def _start(self, images):
        ops = self.ops
        if not self.random_start:
            return images.clone()
        if self.norm == "L2":                                        # pgdl2.py:55-62, as PGDL2 draws it
            if self._init_noise is not None:
                normal, r = self._init_noise
                return ops.pgd_l2_init(images, self.eps, draws=(normal.to(self.device).contiguous(),
                                                                r.to(self.device).reshape(-1).contiguous()))
            return ops.pgd_l2_init(images, self.eps, seed=self._fresh_seed())
        if self._init_noise is not None:                             # pgd.py:54-57, as PGD draws it
            return ops.pgd_linf_init(images, self.eps, noise=self._init_noise.to(self.device).contiguous())
        return ops.pgd_linf_init(images, self.eps, seed=self._fresh_seed())

    def forward(self, images, labels):
        r"""
        Overridden.
        """
        ops = self.ops
        images, labels, target = self._prepare(images, labels)
        B, m, max_rows = images.shape[0], self.samples, self.max_rows
        scale, shift = self._affine(B, images.device)
        wanted = (target if self._targeted else labels).to(torch.int64).contiguous()
        sign = -1.0 if self._targeted else 1.0

        adv = self._start(images)
        bufs = (adv, torch.empty_like(adv))
        cur = 0
        if B == 0:
            return adv
        seed = self._fresh_seed()                                    # the noise key of this call: never the certifier's
        tail = tuple(images.shape[1:])
        copies = torch.empty((m, B) + tail, dtype=torch.float32, device=images.device)
        grads = torch.empty_like(copies)
        rows, grad_rows = copies.view((m * B,) + tail), grads.view((m * B,) + tail)
        per_chunk = max(1, min(m, max_rows // B))                    # slots per chunk: Smoothing.votes' formation
        pieces = [(r0, min(r0 + max_rows, (s0 + min(per_chunk, m - s0)) * B))
                  for s0 in range(0, m, per_chunk) for r0 in range(s0 * B, (s0 + min(per_chunk, m - s0)) * B, max_rows)]
        z = torch.empty(m * B, dtype=torch.float32, device=images.device)

        for it in range(self.steps):
            adv = bufs[cur]
            ops.smoothadv_fill(adv, self.sigma, seed, it * m if self.fresh_noise else 0, s0=0, ns=m, scale=scale, shift=shift,
                               out=copies)
            graphs = []
            for r0, r1 in pieces:
                piece = rows[r0:r1].detach().requires_grad_(True)
                zp = self.model(piece)
                if zp.dim() != 2 or zp.shape[1] != 1:
                    raise ValueError(f"the attacked model must emit one logit per utterance, got {tuple(zp.shape)}")
                z[r0:r1] = zp.detach().reshape(-1)
                graphs.append((piece, zp))
            dz, _ = ops.smoothadv_loss_grad(z.view(m, B), wanted, sign)
            dz = dz.reshape(-1)
            for (r0, r1), (piece, zp) in zip(pieces, graphs):
                (g,) = torch.autograd.grad(zp, piece, grad_outputs=dz[r0:r1].view_as(zp), retain_graph=False, create_graph=False)
                grad_rows[r0:r1].copy_(g)
            del graphs
            ops.smoothadv_step(adv, images, grads, self.alpha, self.eps, norm=self.norm, out=bufs[1 - cur])
            cur = 1 - cur
        return bufs[cur]
