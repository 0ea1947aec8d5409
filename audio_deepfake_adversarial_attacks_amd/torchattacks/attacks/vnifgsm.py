"""VNI-FGSM (reference: adversarial_attacks/torchattacks/attacks/vnifgsm.py:7-104)."""
from ..attack import Attack
from .vmifgsm import VMIFGSM


class VNIFGSM(VMIFGSM):
    r"""VNI-FGSM in the paper 'Enhancing the Transferability of Adversarial Attacks through Variance Tuning'
    [https://arxiv.org/abs/2103.15571], Published as a conference paper at CVPR 2021

    Distance Measure : Linf

    Arguments:
        model (nn.Module): model to attack.
        eps (float): maximum perturbation. (Default: 8/255)
        alpha (float): step size. (Default: 2/255)
        steps (int): number of iterations. (Default: 5)
        decay (float): momentum factor. (Default: 1.0)
        N (int): the number of sampled examples in the neighborhood. (Default: 20)
        beta (float): the upper bound of neighborhood. (Default: 3/2)

    VMI-FGSM (see VMIFGSM) with the model evaluated at the look-ahead point adv + decay * alpha * momentum; the neighbours
    stay around adv itself, as in the reference.

    Examples::
        >>> attack = torchattacks.VNIFGSM(model, eps=8/255, steps=5, decay=1.0, N=20, beta=3/2)
        >>> adv_images = attack(images, labels)
    """

    _nesterov = True

    def __init__(self, model, eps=8 / 255, alpha=2 / 255, steps=5, decay=1.0, N=20, beta=3 / 2):
        Attack.__init__(self, "VNIFGSM", model)
        self.eps = eps
        self.steps = steps
        self.decay = decay
        self.alpha = alpha
        self.N = N
        self.beta = beta
        self._supported_mode = ["default", "targeted"]
