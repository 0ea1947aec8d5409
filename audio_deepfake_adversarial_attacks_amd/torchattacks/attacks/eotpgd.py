"""EOTPGD (reference: adversarial_attacks/torchattacks/attacks/eotpgd.py:7-83), and its expectation over a simulated audio
channel (no counterpart in the reference)."""
import torch

from ..attack import Attack
from ..channel import resolve


class EOTPGD(Attack):
    r"""PGD on a gradient summed over `eot_iter` passes, 'Comment on "Adv-BNN: Improved Adversarial Defense through Robust Bayesian
    Neural Network"' [https://arxiv.org/abs/1907.00895].

    Arguments:
        model (nn.Module): model to attack.
        eps (float): maximum perturbation. (Default: 0.3)
        alpha (float): step size. (Default: 2/255)
        steps (int): number of steps. (Default: 40)
        eot_iter (int): number of passes (draws of the channel) per step. (Default: 10)
        random_start (bool): using random initialization of delta. (Default: True)
        channel (Channel, str or None): the channel the expectation is taken over: a `torchattacks.Channel`, the name of a
            preset in `torchattacks.CHANNELS`, or None. (Default: None)

    `channel=None` is the reference's algorithm: `eot_iter` forward + input-backward passes at `adv` (eotpgd.py:64-76), their
    gradients summed in pass order, then PGD's step (eotpgd.py:79-81; the sum's sign is the mean's).  On a deterministic
    detector every pass returns the same gradient: the attack is PGD done `eot_iter` times over.

    With a channel the expectation is over what happens to the audio between the attacker and the detector.  `steps * eot_iter`
    draws (`Channel.draw`) are made once per call.  Per step:

        1. `ops.channel_apply` writes the `eot_iter` channelled copies of `adv` (Philox offset = step * eot_iter);
        2. the model is differentiated at each copy, B rows per call — the cross-entropy's mean then has the same scale in every
           draw and LFCC's batch-wide dB floor sees the rows PGD's would — and each gradient goes into its slot of a
           (eot_iter, B, T) buffer;
        3. `ops.channel_eot_step` applies the channel's adjoint, sums over the draws and takes PGD's step in one launch.

    The channel works in the utterance's own units around its CENTRE, the value that means silence: -mn / (mx - mn) in the
    min-max domain the attack sees.  The caller that normalised the utterance hands mn and mx over with `set_minmax(mn, mx)`
    before the call (`evaluation.attack_batch` does: `wants_minmax`); without them the centre is 0.5.

    Out of scope: `replays_from_graph` stays False (the loop is eager, no graph capture, one batch in flight); L2 and momentum
    variants (`ops.channel_adjoint` returns the summed gradient they would start from); the adversarial trainer.

    Examples::
        >>> attack = torchattacks.EOTPGD(model, eps=0.0005, alpha=0.000125, steps=10, eot_iter=4, channel="mild")
        >>> attack.set_minmax(mn, mx)
        >>> adv_images = attack(images, labels)
    """

    replays_from_graph = False

    def __init__(self, model, eps=0.3, alpha=2 / 255, steps=40, eot_iter=10, random_start=True, channel=None):
        super().__init__("EOTPGD", model)
        if int(steps) < 1 or int(eot_iter) < 1:
            raise ValueError(f"steps and eot_iter must be at least 1, got {steps} and {eot_iter}")
        self._channel = resolve(channel)
        if self._channel is not None and int(eot_iter) > 64:
            raise ValueError(f"at most 64 draws of a channel per step (hip_ops.CHANNEL_MAX_DRAWS), got eot_iter={eot_iter}")
        self.eps = eps
        self.alpha = alpha
        self.steps = steps
        self.eot_iter = eot_iter
        self.random_start = random_start
        self._supported_mode = ["default", "targeted"]
        self._minmax = None

    @property
    def channel(self):
        """The `Channel` the expectation is taken over, or None (a property: `__str__` stays the reference's)."""
        return self._channel

    @property
    def wants_minmax(self):
        """Only a channel needs the utterance's mn and mx (for its centre)."""
        return self._channel is not None

    def set_minmax(self, mn, mx) -> None:
        """The per-utterance minimum and maximum `to_minmax` returned, (B,) or (B, 1), for the NEXT call only."""
        self._minmax = (mn, mx)

    def _center(self, B, device):
        """-mn / (mx - mn) per row on the device, or 0.5 when no min-max was handed over; consumes it."""
        minmax, self._minmax = self._minmax, None
        if minmax is None:
            return torch.full((B,), 0.5, dtype=torch.float32, device=device)
        mn, mx = (t.detach().to(device=device, dtype=torch.float32).reshape(-1) for t in minmax)
        if mn.numel() != B or mx.numel() != B:
            raise ValueError(f"set_minmax: mn / mx must hold one value per utterance ({B}), got {mn.numel()} / {mx.numel()}")
        return (-mn / (mx - mn)).contiguous()

    def forward(self, images, labels):
        r"""
        Overridden.
        """
        ops = self.ops
        images, labels, target = self._prepare(images, labels)
        K, steps = int(self.eot_iter), int(self.steps)

        if self.random_start:                                        # eotpgd.py:55-58, as PGD draws it
            if self._init_noise is not None:
                adv = ops.pgd_linf_init(images, self.eps, noise=self._init_noise.to(self.device).contiguous())
            else:
                adv = ops.pgd_linf_init(images, self.eps, seed=self._fresh_seed())
        else:
            adv = images.clone()
        bufs = (adv, torch.empty_like(adv))
        cur = 0

        if self._channel is None:
            for _ in range(steps):
                adv = bufs[cur].detach()
                grad = None
                for _ in range(K):                                   # eotpgd.py:64-76: grad += d cost / d adv
                    g, _ = self._input_gradient(adv, labels, target)
                    grad = g if grad is None else grad + g
                ops.pgd_linf_step(adv, grad, images, self.alpha, self.eps, out=bufs[1 - cur])
                cur = 1 - cur
            return bufs[cur]

        B = images.shape[0]
        center = self._center(B, images.device)
        taps, shift, gain, noise = self._channel.draw(steps * K, images, center)
        seed = self._fresh_seed()
        through = torch.empty((K,) + tuple(images.shape), dtype=torch.float32, device=images.device)
        grads = torch.empty_like(through)
        for it in range(steps):
            adv = bufs[cur]
            d = slice(it * K, (it + 1) * K)
            ops.channel_apply(adv, center, taps[d], shift[d], gain[d], noise[d], seed, it * K, out=through)
            for j in range(K):
                g, _ = self._input_gradient(through[j].detach(), labels, target)
                grads[j].copy_(g)
            ops.channel_eot_step(adv, images, grads, taps[d], shift[d], gain[d], self.alpha, self.eps, out=bufs[1 - cur])
            cur = 1 - cur
        return bufs[cur]
