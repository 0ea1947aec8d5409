"""VMI-FGSM (reference: adversarial_attacks/torchattacks/attacks/vmifgsm.py:7-103)."""
import torch

from ..attack import Attack


class VMIFGSM(Attack):
    r"""VMI-FGSM in the paper 'Enhancing the Transferability of Adversarial Attacks through Variance Tuning'
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

    Adaptations to (B, T) waveform detectors with one logit: as MIFGSM.  The N neighbours of an iteration are
    adv + U(-eps * beta, eps * beta) with the draw made in the kernel from a fresh Philox key per call (neighbour j of
    iteration i at offset i * N + j); `set_init_noise(draws)` installs explicit draws instead, draws[i][j] a tensor shaped
    like the images.  The loop is a fixed launch sequence that never synchronises with the host; it always runs eagerly.

    Examples::
        >>> attack = torchattacks.VMIFGSM(model, eps=8/255, steps=5, decay=1.0, N=20, beta=3/2)
        >>> adv_images = attack(images, labels)
    """

    _nesterov = False       # VNIFGSM: the model reads the look-ahead point adv + decay * alpha * momentum

    def __init__(self, model, eps=8 / 255, alpha=2 / 255, steps=5, decay=1.0, N=20, beta=3 / 2):
        super().__init__("VMIFGSM", model)
        self.eps = eps
        self.steps = steps
        self.decay = decay
        self.alpha = alpha
        self.N = N
        self.beta = beta
        self._supported_mode = ["default", "targeted"]

    def _explicit_draws(self, images):
        """The draws of set_init_noise as device tensors, checked against this call: steps x N tensors shaped like images."""
        draws = self._init_noise
        if draws is None:
            return None
        if len(draws) < self.steps or any(len(row) < self.N for row in draws[:self.steps]):
            raise ValueError(f"set_init_noise: {self.attack} needs draws[i][j] for {self.steps} iterations x {self.N} neighbours")
        out = []
        for i in range(self.steps):
            for j in range(self.N):
                d = draws[i][j]
                if tuple(d.shape) != tuple(images.shape):
                    raise ValueError(f"set_init_noise: draws[{i}][{j}] has shape {tuple(d.shape)}, the images "
                                     f"{tuple(images.shape)}")
            out.append([draws[i][j].to(self.device, torch.float32).contiguous() for j in range(self.N)])
        return out

    def forward(self, images, labels):
        ops = self.ops
        images, labels, target = self._prepare(images, labels)
        draws = self._explicit_draws(images)
        seed = self._fresh_seed() if draws is None else None
        bound = self.eps * self.beta
        # vmifgsm.py:55-61: state of THIS call
        momentum = torch.zeros_like(images)
        v, v_next = torch.zeros_like(images), torch.empty_like(images)
        gv, neighbor = torch.empty_like(images), torch.empty_like(images)
        adv = images.clone()
        nes = images.clone() if self._nesterov else None    # vnifgsm.py:65: the first look-ahead point is adv (zero momentum)

        for i in range(self.steps):
            adv_grad, _ = self._input_gradient(nes if self._nesterov else adv, labels, target)
            # vmifgsm.py:82-97 first: the neighbours lie around the adv this iteration started from
            for j in range(self.N):
                if draws is not None:
                    ops.vt_neighbor(adv.detach(), bound, draw=draws[i][j], out=neighbor.detach())
                else:
                    ops.vt_neighbor(adv.detach(), bound, seed=seed, offset=i * self.N + j, out=neighbor.detach())
                g, _ = self._input_gradient(neighbor, labels, target)
                ops.vt_accumulate(gv, g, first=(j == 0))
            ops.vt_variance(gv, adv_grad, self.N, out=v_next)
            # vmifgsm.py:77-79, 99-101 with this iteration's v
            ops.mi_step(adv.detach(), adv_grad, images, momentum, self.alpha, self.eps, self.decay, v=v,
                        nes_out=nes.detach() if self._nesterov else None,
                        nes_scale=self.decay * self.alpha if self._nesterov else 0.0, out=adv.detach())
            v, v_next = v_next, v
        return adv.detach()
