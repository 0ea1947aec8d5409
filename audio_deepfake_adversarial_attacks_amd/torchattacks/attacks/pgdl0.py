"""PGDL0: the sparse (L0) threat model (no counterpart in the reference tree, whose sparsefool.py / onepixel.py are other
algorithms; the definitions of include/advstep_l0.h are the specification)."""
import math

import torch

from .. import graphed
from ..attack import Attack


class PGDL0(Attack):
    r"""PGD0 of 'Sparse and Imperceivable Adversarial Attacks' (Croce & Hein, ICCV 2019) [https://arxiv.org/abs/1909.05040]
    on (B, T) waveforms: the attacker changes at most `k` samples of an utterance, each as far as the box [0, 1] allows (or,
    with `eps_inf`, by at most that much: the paper's "sparse and bounded" variant) - a handful of clicks.

    An iteration is one forward + input-backward of the model and one launch (`ops.pgdl0_step`): the gradient step scaled by
    the row's ||grad||_1, then the exact projection onto the L0 ball intersected with the box, which keeps the k samples whose
    keeping saves most squared distance and breaks ties towards the lower index (the paper's random jitter is dropped: the
    index rule is reproducible).  The iterations run through `graphed.run_iterations` exactly as PGD's do: the step owns no
    per-call state and writes where the model is not reading, so it is a plain launch between graph replays.  The final
    iterate is returned, as PGD does.

    Arguments:
        model (nn.Module): model to attack.
        k (int): samples of an utterance that may change; k >= T means all. (Default: 64, about 0.1 % of 64 600)
        alpha (float): step per dimension: the step handed to the kernel is alpha * T.  The paper's 120000 / 255 on 3 072
            dimensions is 0.153 per dimension; a choice of scale carried over, not measured on audio. (Default: 0.15)
        steps (int): number of steps. (Default: 20)
        eps_inf (float): optional per-sample cap |adv - x| <= eps_inf. (Default: None, no cap)
        random_start (bool): start from the projection of x + U(-1, 1). (Default: True)

    After a call `last_changed` holds #{adv != x} per utterance, a (B,) int64 tensor on the device.

    Shape:
        - images: (B, T) float32 in [0, 1] (any (B, ...) is treated as B rows).
        - labels: (B) class indices in {0, 1}.
        - output: (B, T).

    Examples::
        >>> attack = torchattacks.PGDL0(model, k=64, alpha=0.15, steps=20)
        >>> adv_images = attack(images, labels)
        >>> changed = attack.last_changed
    """

    replays_from_graph = True

    def __init__(self, model, k=64, alpha=0.15, steps=20, eps_inf=None, random_start=True):
        super().__init__("PGDL0", model)
        if isinstance(k, bool) or int(k) != k or k < 1:
            raise ValueError(f"k must be an integer >= 1, got {k!r}")
        if int(steps) < 1:
            raise ValueError(f"steps must be at least 1, got {steps!r}")
        if not alpha > 0:                                            # (a NaN fails the comparison)
            raise ValueError(f"alpha must be positive, got {alpha!r}")
        if eps_inf is not None and not eps_inf > 0:
            raise ValueError(f"eps_inf must be positive (None: no cap), got {eps_inf!r}")
        self.k = int(k)
        self.alpha = alpha
        self.steps = int(steps)
        self.eps_inf = eps_inf
        self.random_start = random_start
        self._supported_mode = ["default", "targeted"]
        self._last_changed = None

    @property
    def last_changed(self):
        """#{adv != x} per utterance of the last call, (B,) int64 on the device (None before the first call)."""
        return self._last_changed

    def forward(self, images, labels):
        ops = self.ops
        images, labels, target = self._prepare(images, labels)
        B = images.shape[0]
        T = images.numel() // B if B else 0
        k, cap = self.k, (math.inf if self.eps_inf is None else float(self.eps_inf))
        step = float(self.alpha) * T

        if self.random_start:
            # once per call, not on the hot path: one U(-1, 1) draw (or the one installed with set_init_noise), projected
            if self._init_noise is not None:
                noise = self._init_noise.to(self.device).contiguous()
            else:
                noise = torch.rand(images.shape, dtype=torch.float32, device=images.device) * 2.0 - 1.0
            u = images + noise
            adv = ops.l0_box_project(images, u, k, cap, out=u)
        else:
            adv = images.clone()

        def one_step(cur, grad, orig, out):
            ops.pgdl0_step(cur, grad, orig, step, k, cap, out=out)

        adv = graphed.run_iterations(self, adv, images, labels, target, self.steps, one_step, (k, self.alpha, cap))
        self._last_changed = (adv != images).reshape(B, -1).sum(dim=1)
        return adv
