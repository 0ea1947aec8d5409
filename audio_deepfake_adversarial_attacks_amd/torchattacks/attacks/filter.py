"""UniversalFilter: one short FIR filter, fitted once, that every utterance of the source class is run through (no counterpart in
the reference, whose every attack is additive and optimises each utterance on its own)."""
import numpy as np
import torch

from ..attack import Attack

MAX_TAPS = 1025       # ADVSTEP_FILTER_MAX_TAPS of include/advstep_filter.h


class UniversalFilter(Attack):
    r"""A universal adversarial linear time-invariant filter (Malafide: Panariello et al., Interspeech 2023): ONE centred FIR `h`
    of `taps` samples, fitted on some utterances and then applied unchanged to any other, of any length.  The attack is
    CONVOLUTIVE, adv = h * x, where every other attack of this package is additive; its budget is the filter's length, not a norm
    of a perturbation.  Applying it needs no gradient and no model: `forward` is one launch.

    Per row, in the attacks' min-max domain, adv_b = clamp(c_b + h * (x_b - c_b), 0, 1) with c_b = -mn_b / (mx_b - mn_b), the
    value that means silence in the row: filtering is linear and c_b maps to waveform 0, so before the clamp the waveform the
    detector sees is h * waveform — the same physical filter for every utterance, whatever its minimum and maximum.  The caller
    hands mn and mx over with `set_minmax(mn, mx)` before EVERY call (`evaluation.attack_batch` does: `wants_minmax`); they are
    used by the next call and then forgotten.  The clamp clips to the utterance's own original range, which the paper does not do.
    With a source label only the rows of that class are filtered (label 0 = spoof: the filter an attacker runs any fake through);
    the others come back bit for bit.

    The taps start as the unit impulse (the identity) and climb the cross-entropy of the source rows by Adam: per batch one
    `ops.filter_apply`, the model's input gradient, `ops.filter_tap_grad` (the correlation of that gradient, masked where the
    clamp is active, with the centred input) and `ops.filter_tap_update` (its fold over tiles and rows and the Adam step).  No
    step reads the device; there is no random start, so a fit is reproducible.  Fitting is eager (no hipGraph replay).

    Arguments:
        model (nn.Module): model to attack.
        taps (int): the filter's length, odd, 1 .. 1025. (Default: 129 — 8 ms at 16 kHz)
        lr (float): Adam's step size. (Default: 0.02 — a choice of scale, not a measured optimum)
        epochs (int): passes `fit` makes over its batches. (Default: 5)
        source_label (int): None, 0 or 1. (Default: 0)
        betas (tuple): Adam's decay rates. (Default: (0.9, 0.999))

    Examples::
        >>> attack = torchattacks.UniversalFilter(model, taps=129, source_label=0)
        >>> attack.fit([(images, labels, mn, mx), ...])
        >>> attack.set_minmax(other_mn, other_mx)
        >>> adv_images = attack(other_images, other_labels)
        >>> attack.save_delta("filter.npz")
    """

    replays_from_graph = False
    is_universal = True
    is_filter = True
    wants_minmax = True
    _ADAM_EPS = 1e-8

    def __init__(self, model, taps=129, lr=0.02, epochs=5, source_label=0, betas=(0.9, 0.999)):
        super().__init__("UniversalFilter", model)
        if isinstance(taps, bool) or int(taps) != taps or not 1 <= int(taps) <= MAX_TAPS or int(taps) % 2 == 0:
            raise ValueError(f"taps must be an odd number between 1 and {MAX_TAPS}, got {taps!r}")
        if not float(lr) > 0.0:                                     # (a NaN lr fails the comparison)
            raise ValueError(f"lr must be a step size > 0, got {lr}")
        if int(epochs) < 1:
            raise ValueError(f"epochs must be at least 1, got {epochs}")
        if source_label not in (None, 0, 1) or isinstance(source_label, bool):
            raise ValueError(f"source_label must be None, 0 or 1, got {source_label!r}")
        if len(betas) != 2 or not all(0.0 <= float(b) < 1.0 for b in betas):
            raise ValueError(f"betas must be two decay rates in [0, 1), got {betas!r}")
        self.taps = int(taps)
        self.lr = lr
        self.epochs = epochs
        self.source_label = source_label
        self.betas = (float(betas[0]), float(betas[1]))
        self._supported_mode = ["default"]
        self._minmax = None
        self._h = None              # (L,) on the device, or None before fit / load
        self._m = self._v = None    # Adam's moments of the taps
        self._fit_steps = 0
        self._fitting = False

    # ---- state ------------------------------------------------------------------------------------------------------------

    @property
    def delta(self):
        """The taps, (L,) on the device (the attack's own buffer), or None before `fit` / `load_delta`."""
        return self._h

    @property
    def fit_steps(self):
        """`partial_fit` calls since construction, `reset` or `load_delta`."""
        return self._fit_steps

    def reset(self) -> None:
        self._h = self._m = self._v = self._minmax = None
        self._fit_steps = 0

    def set_minmax(self, mn, mx) -> None:
        """The per-utterance minimum and maximum `to_minmax` returned, (B,) or (B, 1), for the NEXT call only."""
        self._minmax = (mn, mx)

    def _rows(self, images, labels):
        """(images, labels, c, m) on the device: c_b = -mn_b / (mx_b - mn_b), m_b = [y_b == source] or None; consumes the min-max."""
        minmax, self._minmax = self._minmax, None
        images = images.detach().to(self.device)
        labels = labels.detach().to(self.device)
        if images.dtype != torch.float32:
            raise TypeError(f"images must be float32 waveforms, got {images.dtype}")
        if images.dim() < 2:
            raise ValueError(f"images must be (B, T), got {tuple(images.shape)}")
        B = images.shape[0]
        if minmax is None:
            raise ValueError("call set_minmax(mn, mx) before every call: the filter acts around each utterance's silence")
        mn, mx = (t.detach().to(device=images.device, dtype=torch.float32).reshape(-1) for t in minmax)
        if mn.numel() != B or mx.numel() != B:
            raise ValueError(f"set_minmax: mn / mx must hold one value per utterance ({B}), got {mn.numel()} / {mx.numel()}")
        c = (-mn / (mx - mn)).contiguous()
        m = None if self.source_label is None else (labels.reshape(-1) == self.source_label).to(torch.float32).contiguous()
        return images.contiguous(), labels, c, m

    # ---- fitting ----------------------------------------------------------------------------------------------------------

    def partial_fit(self, images, labels):
        """One step on one batch: adv = filter_apply(x, h); g = d loss / d adv; the taps take one Adam step up the gradient
        filter_tap_grad and filter_tap_update form.  The model's mode and parameters are handled as in an attack call."""
        self._fitting = True
        try:
            Attack.__call__(self, images, labels)
        finally:
            self._fitting = False
        return self

    def fit(self, batches):
        """`epochs` passes over `batches`, an iterable of (images, labels, mn, mx), in the given order."""
        batches = list(batches)
        for _ in range(int(self.epochs)):
            for batch in batches:
                if len(batch) == 4:
                    self.set_minmax(batch[2], batch[3])
                self.partial_fit(batch[0], batch[1])
        return self

    def _fit_step(self, images, labels):
        ops = self.ops
        images, labels, c, m = self._rows(images, labels)
        B = images.shape[0]
        T = images.numel() // B if B else 0
        if self._h is None:
            self._h = torch.zeros(self.taps, dtype=torch.float32, device=images.device)
            self._h[(self.taps - 1) // 2] = 1.0                     # the unit impulse at P: the identity
            self._m, self._v = torch.zeros_like(self._h), torch.zeros_like(self._h)
        adv = ops.filter_apply(images, c, self._h, m)
        grad, _ = self._input_gradient(adv, labels, None)
        adv = adv.detach()
        ops.filter_tap_grad(images, c, grad.reshape(B, T), adv, self.taps, m)
        self._fit_steps += 1
        ops.filter_tap_update(self._h, self._m, self._v, B, T, self._fit_steps, float(self.lr), self.betas[0], self.betas[1],
                              self._ADAM_EPS, ascend=True)
        return adv

    # ---- applying ---------------------------------------------------------------------------------------------------------

    def forward(self, images, labels):
        r"""
        Overridden.  Applies the frozen filter: no model call, no host read.
        """
        if self._fitting:
            return self._fit_step(images, labels)
        if self._h is None:
            self._minmax = None
            raise RuntimeError("fit or load a perturbation first")
        images, labels, c, m = self._rows(images, labels)
        return self.ops.filter_apply(images, c, self._h, m)

    # ---- persistence ------------------------------------------------------------------------------------------------------

    def save_delta(self, path) -> None:
        """The taps (float32) with their number L and the attack's source_label (-1: none), as an .npz at exactly `path`."""
        if self._h is None:
            raise RuntimeError("fit or load a perturbation first")
        with open(path, "wb") as f:
            np.savez(f, taps=self._h.detach().cpu().numpy().astype(np.float32), L=np.array(self.taps, dtype=np.int64),
                     source_label=np.array(-1 if self.source_label is None else int(self.source_label), dtype=np.int64))

    def load_delta(self, path) -> None:
        """Take the taps from a file `save_delta` wrote; refuses one whose L or source label differ from this attack's."""
        with np.load(path, allow_pickle=False) as z:
            if "taps" not in z.files:
                raise ValueError(f"{path}: not a filter file (no taps; an additive perturbation belongs to UniversalPGD)")
            L, source = int(z["L"]), int(z["source_label"])
            taps = np.ascontiguousarray(z["taps"], dtype=np.float32).reshape(-1)
        mine = -1 if self.source_label is None else int(self.source_label)
        if L != self.taps or taps.size != L or source != mine:
            raise ValueError(f"{path}: fitted for L={L} ({taps.size} taps), source_label={source}; this attack has L={self.taps}, "
                             f"source_label={mine}")
        self.reset()
        self._h = torch.from_numpy(taps).to(self.device).contiguous()
        self._m, self._v = torch.zeros_like(self._h), torch.zeros_like(self._h)
