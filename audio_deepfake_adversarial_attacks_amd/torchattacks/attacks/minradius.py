"""MinRadiusPGD: per-utterance minimal radius by bisection on the device (no counterpart in the reference, whose AttackEnum
asks the same question with one whole evaluation per radius: PGD, PGD_eps00075, PGD_eps001 ...)."""
import torch

from .. import graphed
from ..attack import Attack

_NORMS = ("Linf", "L2")


class MinRadiusPGD(Attack):
    r"""For every utterance, the smallest radius at which PGD flips the attacked model, found in ONE call by bisection on
    [0, eps_max], and the adversarial example witnessed at that radius.

    A round attacks the whole batch from the clean input, every row within its OWN radius (`hip_ops.row_pgd_linf_step` /
    `row_pgd_l2_step` read it from the search state on the device), judges the result with the model in eval mode and
    halves every row's bracket (`hip_ops.radius_round`).  The radii are device data, so the batch shape never changes: one
    captured hipGraph pair (torchattacks/graphed.py, the split form: the model part replays, the step is launched with the
    round's radii; ADVSTEP_ATTACK_GRAPH=fused stays eager) serves every round, two batches can be in flight, and the call
    makes no host read at all.

    Arguments:
        model (nn.Module): model to attack.
        norm (str): "Linf" or "L2". (Default: "Linf")
        eps_max (float): the largest radius tried; the first round attacks every row at it. (Default: 0.001)
        search_steps (int): rounds; a radius is resolved to eps_max / 2^(search_steps - 1). (Default: 6)
        steps (int): PGD steps per round. (Default: 10)
        alpha (float): absolute step size, as in PGD / PGDL2. (Default: None)
        rel_alpha (float): step size as a fraction of the row's radius.  Neither given: 2.5 / steps; both: ValueError.
        report_at (tuple): radii at which `evaluation.generate_attacks` reports the robust accuracy. (Default: ())

    Returns each row's smallest witnessed adversarial example: the clean input for a row the model already gets wrong, the
    attempt at eps_max for a row no round flipped.  `last_radius` holds the radii of the last call, a (B,) float32 tensor on
    the device: 0 for the former, +inf for the latter.

    The radius is in the attack's domain — the min-max-normalised waveform the attacked model is given, the unit of every
    `eps` of AttackEnum — and it is a WITNESSED UPPER BOUND on the true minimal radius: the bisection assumes that PGD's
    success is monotone in the radius, which it need not be.

    There is no random start: a row's outcome at a radius must be a function of the radius alone, or the brackets of two
    rounds would not describe the same attack.  Only the default (untargeted) mode is supported.

    Examples::
        >>> attack = torchattacks.MinRadiusPGD(model, norm="Linf", eps_max=0.001, search_steps=6, steps=10)
        >>> adv_images = attack(images, labels)
        >>> radii = attack.last_radius
    """

    replays_from_graph = True

    def __init__(self, model, norm="Linf", eps_max=0.001, search_steps=6, steps=10, alpha=None, rel_alpha=None, report_at=()):
        super().__init__("MinRadiusPGD", model)
        if norm not in _NORMS:
            raise ValueError(f"MinRadiusPGD norm must be 'Linf' or 'L2', got {norm!r}")
        if alpha is not None and rel_alpha is not None:
            raise ValueError("MinRadiusPGD takes `alpha` (absolute) or `rel_alpha` (a fraction of the row's radius), not both")
        if not float(eps_max) >= 0.0:
            raise ValueError(f"eps_max must be a radius >= 0, got {eps_max}")
        if int(search_steps) < 1 or int(steps) < 1:
            raise ValueError(f"search_steps and steps must be at least 1, got {search_steps} and {steps}")
        if alpha is None and rel_alpha is None:
            rel_alpha = 2.5 / steps
        self.norm = norm
        self.eps_max = eps_max
        self.search_steps = search_steps
        self.steps = steps
        self.alpha = alpha
        self.rel_alpha = rel_alpha
        self.report_at = tuple(report_at)
        self._supported_mode = ["default"]
        self._eps_for_division = 1e-10                      # PGDL2's default
        self._last_radius = None

    @property
    def last_radius(self):
        """The radii of the last call, (B,) float32 on the device (None before the first call); not a hyper-parameter."""
        return self._last_radius

    def _judge(self, x, modules, flags):
        """The logits of the model as it is deployed (eval mode, no_grad), (B,).  Every module's `training` flag is put back
        exactly: the flags are part of the captured graph's key (graphed._state_signature)."""
        self.model.eval()
        try:
            with torch.no_grad():
                z = self.model(x)
        finally:
            for module, flag in zip(modules, flags):
                module.training = flag
        if z.dim() != 2 or z.shape[1] != 1:
            raise ValueError(f"the attacked model must emit one logit per utterance, got {tuple(z.shape)}")
        return z.detach().reshape(-1).contiguous()

    def forward(self, images, labels):
        r"""
        Overridden.
        """
        ops = self.ops
        images, labels, _ = self._prepare(images, labels)
        y = labels.to(torch.int64).contiguous()
        B = images.shape[0]
        modules = list(self.model.modules())
        flags = [module.training for module in modules]
        alpha_abs = float(self.alpha) if self.alpha is not None else 0.0
        alpha_rel = float(self.rel_alpha) if self.rel_alpha is not None else 0.0
        hyper = (self.norm, alpha_abs, alpha_rel)           # no radius: the radii are device data, one capture serves every round

        # two (4, B) states, ping-pong: a round reads one and writes the other (include/advstep_radius.h)
        states = torch.empty((2, 4, B), dtype=torch.float32, device=images.device)
        cur = 0
        ops.radius_begin(self._judge(images, modules, flags), y, self.eps_max, states[cur])
        best_adv = images.clone()

        for rnd in range(self.search_steps):
            state = states[cur]
            eps_rows = state[2]

            if self.norm == "Linf":
                def step(adv, grad, orig, out, eps_rows=eps_rows):
                    ops.row_pgd_linf_step(adv, grad, orig, eps_rows, alpha_abs, alpha_rel, out=out)
            else:
                def step(adv, grad, orig, out, eps_rows=eps_rows):
                    ops.row_pgd_l2_step(adv, grad, orig, eps_rows, alpha_abs, alpha_rel, self._eps_for_division, out=out)

            # step_has_state: the closure reads THIS call's, THIS round's radii; only the split form, whose steps are plain
            # launches of the current closure, may replay (the legacy fused form would bake one round's plane into its graph)
            adv = graphed.run_iterations(self, images.clone(), images, labels, None, self.steps, step, hyper,
                                         step_has_state=True)
            z = self._judge(adv, modules, flags)
            ops.radius_round(adv, z, y, rnd == 0, state, best_adv, out=states[1 - cur])
            cur = 1 - cur

        self._last_radius = states[cur][3]
        return best_adv
