"""UniversalPGD: one perturbation, fitted once, that is added to every utterance (no counterpart in the reference, whose every
attack optimises each utterance on its own)."""
import math

import numpy as np
import torch

from ..attack import Attack

_NORMS = ("Linf", "L2")
_DOMAINS = ("normalized", "waveform")


class UniversalPGD(Attack):
    r"""A universal adversarial perturbation by projected gradient ascent over batches (Moosavi-Dezfooli et al., CVPR 2017, in
    the mini-batch form of Shafahi et al., AAAI 2020): ONE `delta` of T samples with ||delta|| <= eps, fitted on some
    utterances and then added unchanged to any other.  Applying it needs no gradient and no model: `forward` is one launch.

    Per row, adv_b = clamp(x_b + w_b delta, 0, 1) with the row weight w_b = m_b s_b:

    * m_b = 1, or [y_b == source_label] with a source label: in binary detection the gradients of bonafide and spoof rows point
      in opposite directions and their sum cancels, so a useful universal perturbation has a source class (label 0 = spoof: the
      noise an attacker adds to any fake).  Rows of the other class pass through unchanged.
    * s_b = 1 (domain="normalized": delta and eps live in the per-utterance min-max domain, like every `eps` of the other
      attacks), or 1 / (mx_b - mn_b) (domain="waveform": delta and eps are in the waveform's units, so the signal added to the
      waveform, (mx_b - mn_b) w_b delta = delta, is literally the same for every utterance).  The caller hands mn and mx over
      with `set_minmax(mn, mx)` before EVERY call in that domain (`evaluation.attack_batch` and the trainer do:
      `wants_minmax`); they are used by the next call and then forgotten.

    The gradient of the batch's loss with respect to delta is sum_b w_b g_b (`ops.universal_colsum`); delta then takes the PGD
    step of a (1, T) row whose original is the zero row — `ops.pgd_linf_step` resp. `ops.pgd_l2_step` with lo, hi = -eps, eps.
    delta starts at zero and there is no random start, so a fit is reproducible.  Fitting is eager (no hipGraph replay).

    Arguments:
        model (nn.Module): model to attack.
        norm (str): "Linf" or "L2". (Default: "Linf")
        eps (float): radius of delta's ball, in the units of `domain`. (Default: 0.0005)
        alpha (float): step size. (Default: eps / 8 for Linf, eps / 4 for L2 — a choice of scale, not a measured optimum)
        epochs (int): passes `fit` makes over its batches. (Default: 5)
        source_label (int): None, 0 or 1. (Default: None)
        domain (str): "normalized" or "waveform". (Default: "normalized")
        eps_for_division (float): added to the gradient's norm (L2). (Default: 1e-10)

    Examples::
        >>> attack = torchattacks.UniversalPGD(model, eps=0.0005, source_label=0)
        >>> attack.fit([(images, labels), ...])
        >>> adv_images = attack(other_images, other_labels)
        >>> attack.save_delta("uap.npz")
    """

    replays_from_graph = False
    is_universal = True

    def __init__(self, model, norm="Linf", eps=0.0005, alpha=None, epochs=5, source_label=None, domain="normalized",
                 eps_for_division=1e-10):
        super().__init__("UniversalPGD", model)
        if norm not in _NORMS:
            raise ValueError(f"norm must be one of {_NORMS}, got {norm!r}")
        if domain not in _DOMAINS:
            raise ValueError(f"domain must be one of {_DOMAINS}, got {domain!r}")
        if not float(eps) > 0.0:                                    # (a NaN eps fails the comparison)
            raise ValueError(f"eps must be a radius > 0, got {eps}")
        if int(epochs) < 1:
            raise ValueError(f"epochs must be at least 1, got {epochs}")
        if source_label not in (None, 0, 1) or isinstance(source_label, bool):
            raise ValueError(f"source_label must be None, 0 or 1, got {source_label!r}")
        self.norm = norm
        self.eps = eps
        self.alpha = (eps / 8 if norm == "Linf" else eps / 4) if alpha is None else alpha
        self.epochs = epochs
        self.source_label = source_label
        self.domain = domain
        self.eps_for_division = eps_for_division
        self._supported_mode = ["default"]
        self._minmax = None
        self._delta = None          # (1, T) on the device, or None before fit / load
        self._zero = None           # the (1, T) zero row that is `orig` of delta's PGD step
        self._fit_steps = 0
        self._fitting = False

    # ---- state ------------------------------------------------------------------------------------------------------------

    @property
    def wants_minmax(self):
        return self.domain == "waveform"

    @property
    def delta(self):
        """The perturbation, (T,) on the device (a view of the attack's own buffer), or None before `fit` / `load_delta`."""
        return None if self._delta is None else self._delta.reshape(-1)

    @property
    def fit_steps(self):
        """`partial_fit` calls since construction, `reset` or `load_delta`."""
        return self._fit_steps

    def reset(self) -> None:
        self._delta = self._zero = self._minmax = None
        self._fit_steps = 0

    def set_minmax(self, mn, mx) -> None:
        """The per-utterance minimum and maximum `to_minmax` returned, (B,) or (B, 1), for the NEXT call only."""
        self._minmax = (mn, mx)

    def _row_weight(self, labels, B, device):
        """w_b = m_b s_b on the device, (B,), or None when every w_b is 1; consumes the min-max."""
        minmax, self._minmax = self._minmax, None
        w = None
        if self.wants_minmax:
            if minmax is None:
                raise ValueError("domain='waveform': call set_minmax(mn, mx) before every call")
            mn, mx = (t.detach().to(device=device, dtype=torch.float32).reshape(-1) for t in minmax)
            if mn.numel() != B or mx.numel() != B:
                raise ValueError(f"set_minmax: mn / mx must hold one value per utterance ({B}), got {mn.numel()} / {mx.numel()}")
            w = 1.0 / (mx - mn)
        if self.source_label is not None:
            m = (labels.reshape(-1) == self.source_label).to(torch.float32)
            w = m if w is None else m * w
        return None if w is None else w.contiguous()

    def _inputs(self, images, labels):
        images = images.detach().to(self.device)
        labels = labels.detach().to(self.device)
        if images.dtype != torch.float32:
            raise TypeError(f"images must be float32 waveforms, got {images.dtype}")
        if images.dim() < 2:
            raise ValueError(f"images must be (B, T), got {tuple(images.shape)}")
        return images.contiguous(), labels

    # ---- fitting ----------------------------------------------------------------------------------------------------------

    def partial_fit(self, images, labels):
        """One step on one batch: adv = apply(x, delta, w); g = d loss / d adv; s = colsum(g, w); delta takes the PGD step of a
        (1, T) row along s.  The model's mode and parameters are handled as in an attack call."""
        self._fitting = True
        try:
            Attack.__call__(self, images, labels)
        finally:
            self._fitting = False
        return self

    def fit(self, batches):
        """`epochs` passes over `batches`, an iterable of (images, labels) or (images, labels, mn, mx), in the given order."""
        batches = list(batches)
        for _ in range(int(self.epochs)):
            for batch in batches:
                if len(batch) == 4:
                    self.set_minmax(batch[2], batch[3])
                self.partial_fit(batch[0], batch[1])
        return self

    def _fit_step(self, images, labels):
        ops = self.ops
        images, labels = self._inputs(images, labels)
        B = images.shape[0]
        T = images.numel() // B if B else 0
        w = self._row_weight(labels, B, images.device)
        if self._delta is None:
            self._delta = torch.zeros((1, T), dtype=torch.float32, device=images.device)
        self._check_T(T)
        if self._zero is None:
            self._zero = torch.zeros_like(self._delta)
        eps, alpha = float(self.eps), float(self.alpha)
        adv = ops.universal_apply(images, self._delta, w)
        grad, _ = self._input_gradient(adv, labels, None)
        s = ops.universal_colsum(grad.reshape(B, T), w)
        if self.norm == "Linf":
            ops.pgd_linf_step(self._delta, s, self._zero, alpha, eps, lo=-eps, hi=eps, out=self._delta)
        else:
            ops.pgd_l2_step(self._delta, s, self._zero, alpha, eps, float(self.eps_for_division), lo=-eps, hi=eps,
                            out=self._delta)
        self._fit_steps += 1
        return adv.detach()

    def _check_T(self, T):
        if self._delta.numel() != T:
            raise ValueError(f"the perturbation holds {self._delta.numel()} samples, the utterances {T}")

    # ---- applying ---------------------------------------------------------------------------------------------------------

    def forward(self, images, labels):
        r"""
        Overridden.  Applies the frozen delta: no model call, no host read.
        """
        if self._fitting:
            return self._fit_step(images, labels)
        if self._delta is None:
            self._minmax = None
            raise RuntimeError("fit or load a perturbation first")
        images, labels = self._inputs(images, labels)
        B = images.shape[0]
        w = self._row_weight(labels, B, images.device)
        self._check_T(images.numel() // B if B else 0)
        return self.ops.universal_apply(images, self._delta, w)

    # ---- persistence ------------------------------------------------------------------------------------------------------

    def save_delta(self, path) -> None:
        """delta (float32) with the attack's norm, eps, domain and source_label (-1: none), as an .npz at exactly `path`."""
        if self._delta is None:
            raise RuntimeError("fit or load a perturbation first")
        with open(path, "wb") as f:
            np.savez(f, delta=self._delta.detach().reshape(-1).cpu().numpy().astype(np.float32), norm=np.array(self.norm),
                     eps=np.array(float(self.eps), dtype=np.float64), domain=np.array(self.domain),
                     source_label=np.array(-1 if self.source_label is None else int(self.source_label), dtype=np.int64))

    def load_delta(self, path) -> None:
        """Take delta from a file `save_delta` wrote; refuses one whose norm, eps or domain differ from this attack's."""
        with np.load(path, allow_pickle=False) as z:
            norm, eps, domain = str(z["norm"]), float(z["eps"]), str(z["domain"])
            delta = np.ascontiguousarray(z["delta"], dtype=np.float32).reshape(-1)
        if norm != self.norm or domain != self.domain or not math.isclose(eps, float(self.eps), rel_tol=1e-12, abs_tol=0.0):
            raise ValueError(f"{path}: fitted for norm={norm}, eps={eps}, domain={domain}; this attack has norm={self.norm}, "
                             f"eps={self.eps}, domain={self.domain}")
        self.reset()
        self._delta = torch.from_numpy(delta).reshape(1, -1).to(self.device).contiguous()
