"""PsyPGD: PGD under a psychoacoustic masking threshold (no counterpart in the reference tree; the definitions of
include/advstep_masking.h and torchattacks/masking.py are the specification)."""
import torch

from .. import graphed
from ..attack import Attack
from ..masking import MaskingModel


class PsyPGD(Attack):
    r"""PGD whose second phase pulls the perturbation under the frequency-masking threshold of the clean utterance, the
    two-stage recipe of 'Imperceptible, Robust, and Targeted Adversarial Examples for Automatic Speech Recognition' (Qin et
    al., ICML 2019) [https://arxiv.org/abs/1903.10346] on (B, T) waveforms, with the dense-spreading threshold of
    `torchattacks.masking.MaskingModel` (a departure from the paper's masker selection, stated there).

    Phase 1: `steps` iterations of PGD inside the L-inf ball (`ops.psy_step` with lambda = 0: PGD's arithmetic, bit for bit).
    Phase 2: `mask_steps` iterations of one model forward + input-backward, one `ops.masking_hinge_grad` launch (the hinge
    loss  s sum max(|STFT(adv - x)|^2 - theta, 0)  and its exact gradient) and one `ops.psy_step` launch along
    sign(g_ce / mean|g_ce| - mask_weight * g_mask / mean|g_mask|), still inside the ball and the box.
    Then one forward of the model: a row keeps phase 2's result where that still fools the model, phase 1's otherwise.
    Both phases go through `graphed.run_iterations`; nothing reads the host.

    Arguments:
        model (nn.Module): model to attack.
        eps (float): maximum perturbation. (Default: 0.001)
        alpha (float): step size of both phases. (Default: eps / 10)
        steps (int): phase 1's steps. (Default: 10)
        mask_steps (int): phase 2's steps; 0 skips the phase. (Default: 20)
        mask_weight (float): the weight of the masking gradient against the classifier's, both normalised to mean |.| = 1 per
            utterance; a choice of scale that nobody has measured. (Default: 1.0)
        hop (int): hop of the threshold's STFT (n_fft 512). (Default: 128)
        random_start (bool): PGD's random start. (Default: False)

    After a call `last_masking` holds the (B, 3) statistics of the returned rows on the device: the hinge loss, the number of
    time-frequency cells over the threshold, and the largest ratio of perturbation power to threshold.

    Examples::
        >>> attack = torchattacks.PsyPGD(model, eps=0.001, alpha=0.0001, steps=10, mask_steps=20, mask_weight=1.0)
        >>> adv_images = attack(images, labels)
        >>> loss, cells_over, worst = attack.last_masking.unbind(dim=1)
    """

    replays_from_graph = True

    def __init__(self, model, eps=0.001, alpha=None, steps=10, mask_steps=20, mask_weight=1.0, hop=128, random_start=False):
        super().__init__("PsyPGD", model)
        if not eps > 0:
            raise ValueError(f"eps must be positive, got {eps!r}")
        alpha = eps / 10 if alpha is None else alpha
        if not alpha > 0:
            raise ValueError(f"alpha must be positive, got {alpha!r}")
        if int(steps) < 0 or int(mask_steps) < 0 or int(steps) + int(mask_steps) < 1:
            raise ValueError(f"steps and mask_steps must be non-negative and not both 0, got {steps!r}, {mask_steps!r}")
        if not mask_weight >= 0:
            raise ValueError(f"mask_weight must be non-negative, got {mask_weight!r}")
        self.eps = eps
        self.alpha = alpha
        self.steps = int(steps)
        self.mask_steps = int(mask_steps)
        self.mask_weight = float(mask_weight)
        self.hop = int(hop)
        self.random_start = random_start
        self._supported_mode = ["default", "targeted"]
        self._masking = MaskingModel(hop=self.hop)
        self._last_masking = None

    @property
    def last_masking(self):
        """(B, 3) float32 on the device: (hinge loss, cells over the threshold, max P / theta) of the rows the last call
        returned (None before the first call)."""
        return self._last_masking

    @property
    def masking(self):
        return self._masking

    def forward(self, images, labels):
        ops = self.ops
        images, labels, target = self._prepare(images, labels)
        B = images.shape[0]
        rows = images.reshape(B, -1)
        hop, eps, alpha, lam = self.hop, float(self.eps), float(self.alpha), self.mask_weight

        if self.random_start:
            if self._init_noise is not None:
                adv = ops.pgd_linf_init(images, self.eps, noise=self._init_noise.to(self.device).contiguous())
            else:
                adv = ops.pgd_linf_init(images, self.eps, seed=self._fresh_seed())
        else:
            adv = images.clone()

        def pgd_step(cur, grad, orig, out):
            ops.psy_step(cur, grad, None, orig, 0.0, alpha, eps, out=out)

        hyper = (self.eps, self.alpha, self.mask_weight, self.hop)
        if self.steps:
            adv = graphed.run_iterations(self, adv, images, labels, target, self.steps, pgd_step, hyper)

        # once per call, not on the hot path: the clean utterance's threshold and scale
        theta, scale = self._masking.threshold(rows, ops)
        window = self._masking.window(images.device)
        stats = torch.empty((B, 3), dtype=torch.float32, device=images.device)
        result = adv
        if self.mask_steps:
            g_mask = torch.empty_like(rows)

            def masked_step(cur, grad, orig, out):
                ops.masking_hinge_grad(cur.reshape(B, -1), orig.reshape(B, -1), window, theta, scale, hop, out=g_mask, stats=stats)
                ops.psy_step(cur, grad, g_mask.view_as(cur), orig, lam, alpha, eps, out=out)

            # the closure owns g_mask and stats: a step with state (never warmed up or baked into a fused graph); the split
            # form's graphs hold the model part only, so both phases replay the same capture
            adv2 = graphed.run_iterations(self, adv, images, labels, target, self.mask_steps, masked_step, hyper,
                                          step_has_state=True)
            with torch.no_grad():
                z = self.model(adv2)
            pred = (z.reshape(B) > 0).to(labels.dtype)
            fooled = (pred == target) if self._targeted else (pred != labels)
            result = torch.where(fooled.view(B, *([1] * (images.dim() - 1))), adv2, adv)
        ops.masking_hinge_grad(result.reshape(B, -1).contiguous(), rows, window, theta, scale, hop, stats=stats)
        self._last_masking = stats
        return result.detach()
