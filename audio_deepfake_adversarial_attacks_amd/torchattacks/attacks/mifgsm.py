"""MI-FGSM (reference: adversarial_attacks/torchattacks/attacks/mifgsm.py:7-78)."""
import torch

from .. import graphed
from ..attack import Attack


class MIFGSM(Attack):
    r"""MI-FGSM in the paper 'Boosting Adversarial Attacks with Momentum' [https://arxiv.org/abs/1710.06081]

    Distance Measure : Linf

    Arguments:
        model (nn.Module): model to attack.
        eps (float): maximum perturbation. (Default: 8/255)
        alpha (float): step size. (Default: 2/255)
        decay (float): momentum factor. (Default: 1.0)
        steps (int): number of iterations. (Default: 5)

    Adaptations to (B, T) waveform detectors with one logit: a row of (B, T) takes the place of an image (the mean of |grad|
    over dims (1, 2, 3) is the mean over T); the gradient comes from `Attack._input_gradient` as for PGD.  One iteration's
    whole update — normalisation, momentum, sign step, eps-ball and [0, 1] projection — is one fused call
    (hip_ops.mi_step); the momentum is per-call state, zero-filled at the start of every call.

    Examples::
        >>> attack = torchattacks.MIFGSM(model, eps=8/255, steps=5, decay=1.0)
        >>> adv_images = attack(images, labels)
    """

    replays_from_graph = True
    _nesterov = False       # NIFGSM: the model reads the look-ahead point adv + decay * alpha * momentum

    def __init__(self, model, eps=8 / 255, alpha=2 / 255, steps=5, decay=1.0):
        super().__init__("MIFGSM", model)
        self.eps = eps
        self.steps = steps
        self.decay = decay
        self.alpha = alpha
        self._supported_mode = ["default", "targeted"]

    def forward(self, images, labels):
        ops = self.ops
        images, labels, target = self._prepare(images, labels)
        momentum = torch.zeros_like(images)     # mifgsm.py:50: state of THIS call, on the current stream
        hyper = (self.eps, self.alpha, self.decay)

        if not self._nesterov:
            # mifgsm.py:56-76, `steps` times: the ping-pong buffers hold adv
            def step(cur, grad, orig, out):
                ops.mi_step(cur, grad, orig, momentum, self.alpha, self.eps, self.decay, out=out)

            return graphed.run_iterations(self, images.clone(), images, labels, target, self.steps, step, hyper,
                                          step_has_state=True)

        # nifgsm.py:54-71: the ping-pong buffers hold the look-ahead point the model reads (the first equals the images: the
        # momentum is zero); the true adv is updated in place and the next look-ahead point written where the model is not
        # reading.  The gradient w.r.t. the look-ahead point is the reference's gradient w.r.t. adv (identity Jacobian).
        adv = images.clone()

        def nes_step(cur, grad, orig, out):
            ops.mi_step(adv, grad, orig, momentum, self.alpha, self.eps, self.decay, nes_out=out,
                        nes_scale=self.decay * self.alpha, out=adv)

        graphed.run_iterations(self, images.clone(), images, labels, target, self.steps, nes_step, hyper, step_has_state=True)
        return adv
