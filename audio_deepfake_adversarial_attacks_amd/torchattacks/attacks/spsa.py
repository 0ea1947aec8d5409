"""SPSA: the score-based black-box counterpart of PGD (no counterpart in the reference, whose every attack differentiates the
attacked detector)."""
import torch

from ..attack import Attack


class SPSA(Attack):
    r"""Simultaneous-perturbation gradient estimation (Spall 1992; as an attack: Uesato et al., ICML 2018) with the sign step of
    ZO-signSGD (Liu et al., ICLR 2019), inside PGD's L-inf ball.  The attacker only submits waveforms and reads the detector's
    logit: no gradient of the model is taken, and the figure the attack adds beside the robust accuracy is QUERIES per utterance.

    An iteration draws `nb_sample` Rademacher directions v_j per utterance, queries the model at adv (slot 0) and at
    clamp(adv +- delta v_j, 0, 1) (S = 1 + 2 nb_sample slots), estimates the sign of the margin loss's gradient from the paired
    differences and takes PGD's step and projection along it:

        1. `ops.spsa_probe` fills the slots, in chunks of at most `max_rows` forward rows;
        2. the model scores each chunk under `torch.no_grad()`;
        3. the logits go into one (S, B) buffer;
        4. `ops.spsa_step` moves every row that slot 0 does not already show fooled, and adds S to its query count.

    The directions are regenerated from Philox inside both kernels (one `_fresh_seed()` per call, a fresh offset per iteration)
    and never stored.  There is no host read inside the loop.

    A row that slot 0 shows fooled is frozen by the step kernel: it keeps its bytes and stops counting queries (it is still
    forwarded with the batch, whose shape never changes; the count is what an attacker who stops at success would have spent).
    `early_stop=False` overwrites the slot-0 row of the logit buffer with a logit of the row's own class before the step
    (+1 for label 1, -1 for label 0), so that no row counts as fooled and every row spends steps * S queries.

    Arguments:
        model (nn.Module): model to attack.
        eps (float): maximum perturbation. (Default: 0.0005)
        alpha (float): step size. (Default: 2.5 * eps / steps)
        steps (int): iterations. (Default: 10)
        nb_sample (int): direction pairs per iteration, at most `hip_ops.SPSA_MAX_DIRECTIONS`. (Default: 8)
        delta (float): probe size. (Default: eps)
        max_rows (int): forward rows per model call. (Default: 1024)
        early_stop (bool): freeze rows that are already fooled. (Default: True)

    After a call `last_queries` holds the model queries each utterance spent, a (B,) int32 tensor on the device.

    Only the default (untargeted) mode is supported and there is no random start.  The loop is eager: graph capture of the
    forward and two batches in flight (`replays_from_graph`) are out of scope.

    Examples::
        >>> attack = torchattacks.SPSA(model, eps=0.0005, steps=20, nb_sample=8)
        >>> adv_images = attack(images, labels)
        >>> queries = attack.last_queries
    """

    replays_from_graph = False

    def __init__(self, model, eps=0.0005, alpha=None, steps=10, nb_sample=8, delta=None, max_rows=1024, early_stop=True):
        super().__init__("SPSA", model)
        if not float(eps) >= 0.0:                                   # (a NaN eps fails the comparison)
            raise ValueError(f"eps must be a radius >= 0, got {eps}")
        if int(steps) < 1 or int(nb_sample) < 1 or int(max_rows) < 1:
            raise ValueError(f"steps, nb_sample and max_rows must be at least 1, got {steps}, {nb_sample} and {max_rows}")
        self.eps = eps
        self.alpha = 2.5 * eps / steps if alpha is None else alpha
        self.steps = steps
        self.nb_sample = nb_sample
        self.delta = eps if delta is None else delta
        self.max_rows = max_rows
        self.early_stop = early_stop
        self._supported_mode = ["default"]
        self._last_queries = None

    @property
    def slots(self):
        """S = 1 + 2 nb_sample: model queries per utterance and iteration."""
        return 1 + 2 * int(self.nb_sample)

    @property
    def budget(self):
        """steps * S: the queries of an utterance that is never fooled."""
        return int(self.steps) * self.slots

    @property
    def last_queries(self):
        """The queries of the last call, (B,) int32 on the device (None before the first call); not a hyper-parameter."""
        return self._last_queries

    def _score(self, x):
        z = self.model(x)
        if z.dim() != 2 or z.shape[1] != 1:
            raise ValueError(f"the attacked model must emit one logit per utterance, got {tuple(z.shape)}")
        return z.reshape(-1)

    def forward(self, images, labels):
        r"""
        Overridden.
        """
        ops = self.ops
        images, labels, _ = self._prepare(images, labels)
        y = labels.to(torch.int64).reshape(-1).contiguous()
        B = images.shape[0]
        T = images.numel() // B if B else 0
        n, S = int(self.nb_sample), self.slots
        eps, alpha, delta = float(self.eps), float(self.alpha), float(self.delta)
        seed = self._fresh_seed()
        calls = (n + 31) // 32                                      # Philox offsets an iteration consumes
        max_rows = int(self.max_rows)
        per_chunk = max(1, min(S, max_rows // max(B, 1)))           # slots per probe fill

        orig = images.reshape(B, T)
        bufs = (orig.clone(), torch.empty_like(orig))
        probes = torch.empty((per_chunk, B) + tuple(images.shape[1:]), dtype=torch.float32, device=images.device)
        z = torch.empty((S, B), dtype=torch.float32, device=images.device)
        z_flat = z.reshape(-1)                                      # slot-major, like the probe rows
        queries = torch.zeros(B, dtype=torch.int32, device=images.device)
        own_class = None if self.early_stop else (2.0 * y.to(torch.float32) - 1.0)
        cur = 0
        for it in range(int(self.steps)):
            adv, offset = bufs[cur], it * calls
            with torch.no_grad():
                for s0 in range(0, S, per_chunk):
                    ns = min(per_chunk, S - s0)
                    chunk = probes[:ns]
                    ops.spsa_probe(adv, delta, seed, offset, s0=s0, ns=ns, out=chunk)
                    rows = chunk.reshape((ns * B,) + tuple(images.shape[1:]))
                    for r0 in range(0, ns * B, max_rows):            # one piece unless a single slot exceeds max_rows
                        z_flat[s0 * B + r0:s0 * B + min(r0 + max_rows, ns * B)] = self._score(rows[r0:r0 + max_rows])
                if own_class is not None:
                    z[0] = own_class
            ops.spsa_step(adv, orig, z, y, queries, alpha, eps, seed, offset, out=bufs[1 - cur])
            cur = 1 - cur
        self._last_queries = queries
        return bufs[cur].reshape(images.shape)
