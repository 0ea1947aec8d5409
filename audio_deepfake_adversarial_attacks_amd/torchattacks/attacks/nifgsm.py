"""NI-FGSM (reference: adversarial_attacks/torchattacks/attacks/nifgsm.py:7-73)."""
from ..attack import Attack
from .mifgsm import MIFGSM


class NIFGSM(MIFGSM):
    r"""NI-FGSM in the paper 'NESTEROV ACCELERATED GRADIENT AND SCALEINVARIANCE FOR ADVERSARIAL ATTACKS'
    [https://arxiv.org/abs/1908.06281], Published as a conference paper at ICLR 2020

    Distance Measure : Linf

    Arguments:
        model (nn.Module): model to attack.
        eps (float): maximum perturbation. (Default: 8/255)
        alpha (float): step size. (Default: 2/255)
        decay (float): momentum factor. (Default: 1.0)
        steps (int): number of iterations. (Default: 5)

    MI-FGSM's update (see MIFGSM) with the model evaluated at the look-ahead point adv + decay * alpha * momentum, which
    the fused update writes for the next iteration.

    Examples::
        >>> attack = torchattacks.NIFGSM(model, eps=8/255, alpha=2/255, steps=5, decay=1.0)
        >>> adv_images = attack(images, labels)
    """

    _nesterov = True

    def __init__(self, model, eps=8 / 255, alpha=2 / 255, steps=5, decay=1.0):
        Attack.__init__(self, "NIFGSM", model)
        self.eps = eps
        self.steps = steps
        self.decay = decay
        self.alpha = alpha
        self._supported_mode = ["default", "targeted"]
