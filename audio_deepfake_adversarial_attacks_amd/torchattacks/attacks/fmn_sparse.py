"""FMNSparse: the L1 and L0 forms of the Fast Minimum-Norm attack (Pintor, Roli, Brendel, Biggio, "Fast Minimum-norm Adversarial
Attacks through Adaptive Norm Constraints", NeurIPS 2021) for waveform detectors with one logit; no counterpart in the reference.
FMN (fmn.py) answers "at which radius does this utterance break" in L-inf and L2; this class answers it for the two sparse threat
models, which APGDL1 and PGDL0 only attack at fixed budgets."""
import torch

from .fmn import FMN

_NORMS = ("L1", "L0")


class FMNSparse(FMN):
    r"""For every utterance, the smallest L1 norm ("L1") or the smallest number of changed samples ("L0") that flips the attacked
    model, found in ONE run of `steps` gradient passes.  The recurrence, the cosine schedules, the one-pass margin gradient and
    the forward-only last decision are FMN's; the step is one fused launch per pass (`hip_ops.fmn_sparse_step`;
    include/advstep_fmn_sparse.h has the expressions): one workgroup owns a row's norms, its decision, the copy of an improved
    iterate, the move and the projection into the row's NEW radius.

        L1:  dn = ||adv - x||_1, gq = max |g|, FMN's three-way radius rule; the projection is l1-APGD's EXACT projection onto the
             L1 ball intersected with the box [0, 1] (Croce & Hein, ICML 2021), with a radius per row.
        L0:  dn = #{adv != x}, the paper's integer rule: eps = min(eps - 1, floor(eps (1 - gamma_k)), best) while adversarial,
             max(eps + 1, floor(eps (1 + gamma_k))) while not, from a starting radius of 1 and inside [0, T]; the projection
             keeps the eps samples whose keeping saves most squared distance (PGD0's exact-k projection) and resets the rest.

    DEPARTURES FROM THE PAPER: its L1 projection is the simplex projection followed by a clamp to the box, which leaves the ball's
    surface wherever the clamp bites; this one is exact for the intersection.  Its L0 projection takes the top-k of a sort, whose
    choice among equal scores is the sort's; this one keeps the LOWEST indices among samples that tie at the threshold, so a call
    is a function of its inputs.  The widened never-found rule of FMN (its own departure) applies to L1 as it stands.

    Arguments:
        model (nn.Module): model to attack.
        norm (str): "L1" or "L0". (Default: "L1")
        steps (int): gradient passes. (Default: 100)
        alpha_init, alpha_final (float): the step size's schedule. (Default: 1.0, 1e-3)
        gamma_init, gamma_final (float): the radius' relative change per step, in (0, 1). (Default: 0.05, 1e-3)
        report_at (tuple): radii at which `evaluation.generate_attacks` reports the robust accuracy. (Default: ())

    Returns each row's smallest adversarial iterate: the clean input for a row the model already gets wrong and for a row that
    never flipped.  `last_radius` holds the L1 norms, or the numbers of changed samples, of the last call, a (B,) float32 tensor
    on the device: 0 for the former, +inf for the latter.  It is a WITNESSED UPPER BOUND on the true minimum, in the attack's
    domain (the min-max-normalised waveform, box [0, 1]).  The call makes no host read.

    The defaults are choices of scale: nobody has measured what they achieve against a trained detector.  With gamma_init = 0.05
    an L0 radius grows by one sample per step (101 samples after 100 steps); the registry's FMN_L0 therefore starts at 0.3.

    Out of scope, as for FMN: targeted mode, restarts, hipGraph replay; also a per-sample cap in the L0 form.

    Examples::
        >>> attack = torchattacks.FMNSparse(model, norm="L0", steps=100, gamma_init=0.3)
        >>> adv_images = attack(images, labels)
        >>> changed_samples = attack.last_radius
    """

    def __init__(self, model, norm="L1", steps=100, alpha_init=1.0, alpha_final=1e-3, gamma_init=0.05, gamma_final=1e-3,
                 report_at=()):
        if norm not in _NORMS:
            raise ValueError(f"FMNSparse norm must be 'L1' or 'L0', got {norm!r}")
        super().__init__(model, norm="Linf", steps=steps, alpha_init=alpha_init, alpha_final=alpha_final, gamma_init=gamma_init,
                         gamma_final=gamma_final, report_at=report_at)
        self.attack = "FMNSparse"
        self.norm = norm

    def forward(self, images, labels):
        r"""
        Overridden.
        """
        ops = self.ops
        images, labels, _ = self._prepare(images, labels)
        y = labels.to(torch.int64).contiguous()
        B = images.shape[0]
        towards = torch.where(y == 1, -1.0, 1.0).to(torch.float32).reshape(B, 1)

        # two (4, B) states, ping-pong: a step reads one and writes the other (include/advstep_fmn_sparse.h)
        states = torch.empty((2, 4, B), dtype=torch.float32, device=images.device)
        cur = 0
        ops.fmn_begin(states[cur])
        best_adv = images.clone()
        adv = images.clone()
        for k in range(int(self.steps)):
            alpha, gamma = self.schedule(k)
            grad, z = self._margin_gradient(adv, towards)
            _, adv = ops.fmn_sparse_step(adv, grad, images, z, y, states[cur], best_adv, alpha, gamma, self.norm, move=True,
                                         eps_div=self._eps_for_division, state_out=states[1 - cur])
            cur = 1 - cur
        with torch.no_grad():                                # the last iterate's decision: forward only, in the attack's mode
            z = self._logits(self.model(adv))
        ops.fmn_sparse_step(adv, None, images, z, y, states[cur], best_adv, 0.0, self.schedule(int(self.steps))[1], self.norm,
                            move=False, state_out=states[1 - cur])
        self._last_radius = states[1 - cur][1]
        return best_adv
