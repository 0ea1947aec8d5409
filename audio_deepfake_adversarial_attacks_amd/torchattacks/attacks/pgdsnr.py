"""PGDSNR: PGD under a budget stated in dB of SNR, per utterance or per 256-sample segment (no counterpart in the reference,
whose every radius is an `eps` in the per-utterance min-max domain)."""
import math

import torch

from .. import graphed
from ..attack import Attack


class PGDSNR(Attack):
    r"""PGD whose budget is a signal-to-noise ratio of the WAVEFORM, in dB.

    The attack sees the min-max-normalised utterance x01 = (x - mn) / (mx - mn).  The waveform is (mx - mn) (x01 + c) with
    c = mn / (mx - mn), and a perturbation scales by (mx - mn), so the waveform's SNR is sum (x01 + c)^2 / sum delta^2 whatever
    the scale.  With rho = 10^(-snr_db / 20):

    * global (segmental=False): ||delta_b||_2 <= rho sqrt(sum_t (x01 + c_b)^2) — an L2 ball with a radius per utterance.  The
      radii come from `ops.snr_row_radius`, the step is `ops.row_pgd_l2_step` with them.
    * segmental (segmental=True): the same inequality for every segment [256 s, 256 s + 256) on its own (the last, partial segment
      included) — a product of L2 balls.  `ops.seg_pgd_step` normalises each segment's gradient by its own norm, steps by
      rel_alpha times the segment's radius and projects the segment onto its own ball, in one launch.  A silent segment has
      radius 0 and is not touched; there is no energy floor, so EVERY segment's SNR is >= snr_db, hence the report's
      snr_db >= snr_db and seg_snr_db >= min(snr_db, 35), up to float32 rounding.

    The caller that normalised the utterance hands mn and mx over with `set_minmax(mn, mx)` before the call
    (`evaluation.attack_batch` and the trainer do: `wants_minmax`); they are used by the next call and then forgotten.  WITHOUT
    them c = 0: the budget is then relative to x01 itself, whose energy includes the offset the normalisation added — a much
    looser budget for a typical, zero-mean utterance.  A constant utterance (mx == mn) gives NaN, as `to_minmax` already does.

    Arguments:
        model (nn.Module): model to attack.
        snr_db (float): the budget; larger is quieter. (Default: 30.0)
        segmental (bool): per segment instead of per utterance. (Default: False)
        steps (int): number of steps. (Default: 10)
        rel_alpha (float): step size as a fraction of the radius (the row's or the segment's). (Default: 2.5 / steps)
        eps_for_division (float): added to the gradient's norm. (Default: 1e-10)

    The start is the clean input (no random start).  Only the default (untargeted) mode is supported.

    Examples::
        >>> attack = torchattacks.PGDSNR(model, snr_db=30.0, segmental=True, steps=10)
        >>> attack.set_minmax(mn, mx)
        >>> adv_images = attack(images, labels)
    """

    replays_from_graph = True
    wants_minmax = True

    def __init__(self, model, snr_db=30.0, segmental=False, steps=10, rel_alpha=None, eps_for_division=1e-10):
        super().__init__("PGDSNR", model)
        if math.isnan(float(snr_db)):
            raise ValueError("snr_db must be a number of dB, got NaN")
        if int(steps) < 1:
            raise ValueError(f"steps must be at least 1, got {steps}")
        self.snr_db = snr_db
        self.segmental = bool(segmental)
        self.steps = steps
        self.rel_alpha = 2.5 / steps if rel_alpha is None else rel_alpha
        self.eps_for_division = eps_for_division
        self._supported_mode = ["default"]
        self._minmax = None

    @property
    def rho(self):
        """10^(-snr_db / 20), in double: ||delta|| / ||signal|| at the budget."""
        return 10.0 ** (-float(self.snr_db) / 20.0)

    def set_minmax(self, mn, mx) -> None:
        """The per-utterance minimum and maximum `to_minmax` returned, (B,) or (B, 1), for the NEXT call only."""
        self._minmax = (mn, mx)

    def _offsets(self, B, device):
        """c = mn / (mx - mn) per row on the device, or None (c = 0) when no min-max was handed over; consumes it."""
        minmax, self._minmax = self._minmax, None
        if minmax is None:
            return None
        mn, mx = (t.detach().to(device=device, dtype=torch.float32).reshape(-1) for t in minmax)
        if mn.numel() != B or mx.numel() != B:
            raise ValueError(f"set_minmax: mn / mx must hold one value per utterance ({B}), got {mn.numel()} / {mx.numel()}")
        return (mn / (mx - mn)).contiguous()

    def forward(self, images, labels):
        r"""
        Overridden.
        """
        ops = self.ops
        images, labels, _ = self._prepare(images, labels)
        c = self._offsets(images.shape[0], images.device)
        rho, alpha_rel, eps_div = float(self.rho), float(self.rel_alpha), float(self.eps_for_division)
        hyper = ("segmental" if self.segmental else "global", alpha_rel, rho)   # c is device data: one capture serves every call

        if self.segmental:
            def step(adv, grad, orig, out):
                ops.seg_pgd_step(adv, grad, orig, c, rho, alpha_rel, eps_div, out=out)
        else:
            eps_rows = ops.snr_row_radius(images, c, rho)

            def step(adv, grad, orig, out):
                ops.row_pgd_l2_step(adv, grad, orig, eps_rows, 0.0, alpha_rel, eps_div, out=out)

        # step_has_state: the closure reads THIS call's offsets / radii; only the split form, whose steps are plain launches of
        # the current closure, may replay (the legacy fused form would bake one call's into its graph)
        return graphed.run_iterations(self, images.clone(), images, labels, None, self.steps, step, hyper, step_has_state=True)
