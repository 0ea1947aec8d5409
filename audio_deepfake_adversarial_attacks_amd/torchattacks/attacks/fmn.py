"""FMN: Fast Minimum-Norm attack (Pintor, Roli, Brendel, Biggio, "Fast Minimum-norm Adversarial Attacks through Adaptive Norm
Constraints", NeurIPS 2021) for waveform detectors with one logit; no counterpart in the reference, whose AttackEnum asks for
the radius at which an utterance breaks with one whole evaluation per radius."""
import math

import torch

from ..attack import Attack

_NORMS = ("Linf", "L2")


def cosine_schedule(v0: float, vK: float, k: int, K: int) -> float:
    """v_K + (v_0 - v_K)(1 + cos(pi k / K)) / 2 in float64: v_0 at k = 0, v_K at k = K."""
    return float(vK) + 0.5 * (float(v0) - float(vK)) * (1.0 + math.cos(math.pi * k / K))


class FMN(Attack):
    r"""For every utterance, the smallest perturbation (in L-inf or L2) that flips the attacked model, found in ONE run of
    `steps` gradient passes: every row carries its own radius eps, which shrinks by (1 - gamma) while the iterate is adversarial
    and grows by (1 + gamma) while it is not, and the iterate takes a normalised gradient step of size alpha on the logit margin
    and is projected into the row's ball.  There is no largest radius and no outer search, and the radii are continuous.

    Per step k (`hip_ops.fmn_norms`, `hip_ops.fmn_step`; include/advstep_fmn.h has the expressions), with z the logit of the
    iterate, d = adv - x and g = dz / d adv from the same pass:

        dn = ||d||_p,  gq = ||g||_q (q dual to p),  is_adv = (z > 0) != label
        best = min(best, dn) and best_adv = adv when is_adv
        eps  = min(eps, best) (1 - gamma_k)           if is_adv
             = eps (1 + gamma_k)                      elif the row was adversarial before
             = (dn + |z| / gq) (1 + gamma_k)          else: the boundary of the local linear model
        adv  = clamp(x + project_eps((adv + alpha_k g' / (||g'||_2 + 1e-10)) - x), 0, 1),   g' = g turned towards the other class

    alpha_k and gamma_k are cosine-annealed from their `_init` to their `_final` value, computed on the host in float64 and
    passed as float32 launch scalars.  The loss is the logit margin, not cross-entropy.  After the last step one forward-only
    pass judges the final iterate.  Radii, norms and decisions never leave the device: the call makes no host read.

    DEPARTURE FROM THE PAPER: its never-found rule is eps = dn + |z| / gq, without the factor (1 + gamma_k).  On a locally linear
    detector that rule puts the iterate exactly on the boundary, where the rounding of z decides and a row can stall unfound
    (tests/test_fmn_host.py's linear detectors, K = 100: 2 and 4 of ten rows in L2, none with the widened rule).

    Arguments:
        model (nn.Module): model to attack.
        norm (str): "Linf" or "L2". (Default: "Linf")
        steps (int): gradient passes. (Default: 60)
        alpha_init, alpha_final (float): the step size's schedule. (Default: 1.0, 1e-3)
        gamma_init, gamma_final (float): the radius' relative change per step, in (0, 1). (Default: 0.05, 1e-3)
        report_at (tuple): radii at which `evaluation.generate_attacks` reports the robust accuracy. (Default: ())

    Returns each row's smallest adversarial iterate: the clean input for a row the model already gets wrong and for a row
    that never flipped.  `last_radius` holds the norms of the last call, a (B,) float32 tensor on the device: 0 for the former,
    +inf for the latter.  The radius is in the attack's domain (the min-max-normalised waveform) and is a WITNESSED UPPER BOUND
    on the true minimal norm.  The model is judged in the mode the attack runs it in (`set_training_mode`).

    The defaults are the paper's and are choices of scale: nobody has measured what they achieve against a trained detector.

    Out of scope here: L1 and L0 (torchattacks.FMNSparse runs this recurrence with the projections of csrc/apgdl1.hip and
    csrc/l0.hip), targeted mode, restarts, and hipGraph replay (a captured graph returns only the gradient, and the step also
    needs the pass's logit).

    Examples::
        >>> attack = torchattacks.FMN(model, norm="L2", steps=60)
        >>> adv_images = attack(images, labels)
        >>> radii = attack.last_radius
    """

    replays_from_graph = False

    def __init__(self, model, norm="Linf", steps=60, alpha_init=1.0, alpha_final=1e-3, gamma_init=0.05, gamma_final=1e-3,
                 report_at=()):
        super().__init__("FMN", model)
        if norm not in _NORMS:
            raise ValueError(f"FMN norm must be 'Linf' or 'L2', got {norm!r}")
        if int(steps) < 1:
            raise ValueError(f"steps must be at least 1, got {steps}")
        for name, v in (("gamma_init", gamma_init), ("gamma_final", gamma_final)):
            if not 0.0 < float(v) < 1.0:
                raise ValueError(f"{name} must lie in (0, 1), got {v}")
        for name, v in (("alpha_init", alpha_init), ("alpha_final", alpha_final)):
            if not float(v) >= 0.0:
                raise ValueError(f"{name} must be a step size >= 0, got {v}")
        self.norm = norm
        self.steps = steps
        self.alpha_init = alpha_init
        self.alpha_final = alpha_final
        self.gamma_init = gamma_init
        self.gamma_final = gamma_final
        self.report_at = tuple(report_at)
        self._supported_mode = ["default"]
        self._eps_for_division = 1e-10                      # PGDL2's default
        self._last_radius = None

    @property
    def last_radius(self):
        """The norms of the last call, (B,) float32 on the device (None before the first call); not a hyper-parameter."""
        return self._last_radius

    def schedule(self, k):
        """(alpha_k, gamma_k) of step k = 0 .. steps (k = steps: the last, forward-only decision)."""
        K = int(self.steps)
        return (cosine_schedule(self.alpha_init, self.alpha_final, k, K), cosine_schedule(self.gamma_init, self.gamma_final, k, K))

    def _logits(self, z):
        if z.dim() != 2 or z.shape[1] != 1:
            raise ValueError(f"the attacked model must emit one logit per utterance, got {tuple(z.shape)}")
        return z.detach().reshape(-1).contiguous()

    def _margin_gradient(self, adv, towards):
        """One forward + input-backward of the logit margin: (g' = towards_b * dz_b / d adv, z (B)) from ONE pass.  `towards` (B, 1)
        is -1 for label 1 and +1 for label 0, so g' points to the other class and ||g'|| = ||dz / d adv||."""
        adv.requires_grad_(True)
        z = self.model(adv)
        zb = self._logits(z)
        (grad,) = torch.autograd.grad(z, adv, grad_outputs=towards.view_as(z), retain_graph=False, create_graph=False)
        adv.requires_grad_(False)
        return grad.contiguous(), zb

    def forward(self, images, labels):
        r"""
        Overridden.
        """
        ops = self.ops
        images, labels, _ = self._prepare(images, labels)
        y = labels.to(torch.int64).contiguous()
        B = images.shape[0]
        towards = torch.where(y == 1, -1.0, 1.0).to(torch.float32).reshape(B, 1)

        # two (4, B) states, ping-pong: a step reads one and writes the other (include/advstep_fmn.h)
        states = torch.empty((2, 4, B), dtype=torch.float32, device=images.device)
        cur = 0
        ops.fmn_begin(states[cur])
        best_adv = images.clone()
        adv = images.clone()
        ws = None
        for k in range(int(self.steps)):
            alpha, gamma = self.schedule(k)
            grad, z = self._margin_gradient(adv, towards)
            ws = ops.fmn_norms(adv, grad, images, ws=ws)
            _, adv = ops.fmn_step(adv, grad, images, z, y, states[cur], best_adv, ws, alpha, gamma, self.norm, move=True,
                                  eps_div=self._eps_for_division, state_out=states[1 - cur])
            cur = 1 - cur
        with torch.no_grad():                                # the last iterate's decision: forward only, in the attack's mode
            z = self._logits(self.model(adv))
        ws = ops.fmn_norms(adv, None, images, ws=ws)
        ops.fmn_step(adv, None, images, z, y, states[cur], best_adv, ws, 0.0, self.schedule(int(self.steps))[1], self.norm,
                     move=False, state_out=states[1 - cur])
        self._last_radius = states[1 - cur][1]
        return best_adv
