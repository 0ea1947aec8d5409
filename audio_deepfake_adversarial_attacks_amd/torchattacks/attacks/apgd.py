"""APGD, L-inf and L2 (reference: adversarial_attacks/torchattacks/attacks/apgd.py:11-265)."""
import time
from dataclasses import dataclass

import torch

from ..attack import Attack


@dataclass
class ApgdState:
    """Per-row state of one `attack_single_run` (apgd.py:96-135), on the attack's device: nothing in it is read back to the
    host inside the iteration loop."""

    acc: torch.Tensor                   # (B) uint8: still classified correctly
    flags: torch.Tensor                 # (B) uint8: fooled | improved << 1 | reset << 2 (include/advstep_apgd.h)
    loss_best: torch.Tensor             # (B) float32
    loss_best_last_check: torch.Tensor  # (B) float32
    reduced_last_check: torch.Tensor    # (B) uint8
    step_size: torch.Tensor             # (B) float32
    loss_steps: torch.Tensor            # (steps, B) float32

    @classmethod
    def new(cls, B: int, steps: int, eps: float, device) -> "ApgdState":
        u8 = dict(dtype=torch.uint8, device=device)
        f32 = dict(dtype=torch.float32, device=device)
        return cls(acc=torch.zeros(B, **u8), flags=torch.zeros(B, **u8), loss_best=torch.zeros(B, **f32),
                   loss_best_last_check=torch.zeros(B, **f32), reduced_last_check=torch.ones(B, **u8),
                   # apgd.py:126: eps * ones * 2.0, all in float32
                   step_size=torch.full((B,), eps, **f32) * 2.0, loss_steps=torch.zeros((steps, B), **f32))


def checkpoint_schedule(steps: int):
    """The iterations i after which apgd.py:194 checks the step size, with the window k of each check (host-known: the
    schedule depends on `steps` only)."""
    steps_2, steps_min, size_decr = max(int(0.22 * steps), 1), max(int(0.06 * steps), 1), max(int(0.03 * steps), 1)
    k, counter3, out = steps_2, 0, []
    for i in range(steps):
        counter3 += 1
        if counter3 == k:
            out.append((i, k))
            counter3 = 0
            k = max(k - size_decr, steps_min)
    return out


class APGD(Attack):
    r"""APGD in the paper 'Reliable evaluation of adversarial robustness with an ensemble of diverse parameter-free attacks'
    [https://arxiv.org/abs/2003.01690] [https://github.com/fra31/auto-attack]

    Distance Measure : Linf, L2

    Arguments:
        model (nn.Module): model to attack.
        norm (str): Lp-norm of the attack. ['Linf', 'L2'] (Default: 'Linf')
        eps (float): maximum perturbation. (Default: 8/255)
        steps (int): number of steps. (Default: 100)
        n_restarts (int): number of random restarts. (Default: 1)
        seed (int): random seed for the starting point. (Default: 0)
        loss (str): loss function optimized. ['ce'] (Default: 'ce')
        eot_iter (int): number of iteration for EOT. (Default: 1)
        rho (float): parameter for step-size update (Default: 0.75)
        verbose (bool): print progress. (Default: False)

    Adaptations to (B, T) waveform detectors with one logit (everything else follows the reference's arithmetic):
      * shapes: a row of (B, T) takes the place of an image; the sums over dims (1, 2, 3) are sums over T and the
        (B, 1, 1, 1) per-row tensors are (B).
      * logits: the attack scores cat([-z, z], 1).  The per-row loss is softplus((1 - 2y) 2z) and the gradient is that of
        the SUMMED loss, dz = 2 (1 - 2y) sigmoid((1 - 2y) 2z), in closed form; the predicted class is 1 iff z > 0 (a tie
        and NaN give 0).
      * loss='dlr' needs at least three classes and raises ValueError; a norm other than 'Linf' / 'L2' raises ValueError.
      * randomness: the call begins with torch.manual_seed(self.seed) as the reference's perturb does (a side effect on
        the caller's generator, kept on purpose); each restart then draws a fresh Philox key from `_fresh_seed()`, so two
        calls with the same seed start from identical points.  `set_init_noise(t)` installs an explicit full-batch (B, T)
        draw instead (U[0, 1) for Linf, N(0, 1) for L2); a restart uses its rows t[ind_to_fool].  A list of such draws
        gives restart r its own draw t[r] (the reference draws afresh at every restart).
      * the per-row update after each model evaluation, the step-size checkpoints and the best-point tracking run on the
        device (hip_ops.apgd_*): the loop never synchronises with the host; each restart does once when it gathers the
        rows still classified correctly and once when it scatters its result back.

    Examples::
        >>> attack = torchattacks.APGD(model, norm='Linf', eps=8/255, steps=100, n_restarts=1, seed=0, loss='ce', eot_iter=1, rho=.75, verbose=False)
        >>> adv_images = attack(images, labels)
    """

    def __init__(self, model, norm="Linf", eps=8 / 255, steps=100, n_restarts=1, seed=0, loss="ce", eot_iter=1, rho=.75,
                 verbose=False):
        super().__init__("APGD", model)
        self.eps = eps
        self.steps = steps
        self.norm = norm
        self.n_restarts = n_restarts
        self.seed = seed
        self.loss = loss
        self.eot_iter = eot_iter
        self.thr_decr = rho
        self.verbose = verbose
        self._supported_mode = ["default"]
        if norm not in ("Linf", "L2"):
            raise ValueError(f"APGD norm must be 'Linf' or 'L2', got {norm!r}")
        if loss == "dlr":
            raise ValueError("APGD loss='dlr' needs at least three classes (it reads the third-largest logit); the "
                             "detectors emit one logit, scored as two classes: use loss='ce'")
        if loss != "ce":
            raise ValueError("unknowkn loss")   # apgd.py:107

    # ---- one model evaluation (apgd.py:109-124, 162-175) ------------------------------------------------------------

    def _evaluate(self, x_adv, y, state, mode, i=0):
        """eot_iter forward + input-backward passes at x_adv; the state update (mode 'start' / 'step') uses the last
        pass's logits, as the reference does.  Returns the gradient (the mean over the passes)."""
        grads = []
        for e in range(self.eot_iter):
            leaf = x_adv.detach().requires_grad_(True)
            with torch.enable_grad():
                z = self.model(leaf)
            if z.dim() != 2 or z.shape[1] != 1:
                raise ValueError(f"the attacked model must emit one logit per utterance, got {tuple(z.shape)}")
            last = e == self.eot_iter - 1
            dz, _ = self.ops.apgd_eval(z.detach().contiguous(), y, state, mode if last else "grad", i)
            (g,) = torch.autograd.grad(z, leaf, grad_outputs=dz.view_as(z), retain_graph=False, create_graph=False)
            grads.append(g)
        if self.eot_iter == 1:
            return grads[0].contiguous()
        grad = torch.zeros_like(x_adv)
        for g in grads:
            grad += g
        grad /= float(self.eot_iter)
        return grad

    # ---- attack_single_run (apgd.py:81-213) ----------------------------------------------------------------------------

    def _single_run(self, x, y, draw=None, seed=None):
        """One restart over the rows (x, y).  Returns (acc (B) uint8, x_best_adv (B, T))."""
        ops = self.ops
        B = x.shape[0]
        self.steps_2, self.steps_min, self.size_decr = (max(int(0.22 * self.steps), 1), max(int(0.06 * self.steps), 1),
                                                        max(int(0.03 * self.steps), 1))
        if self.verbose:
            print("parameters: ", self.steps, self.steps_2, self.steps_min, self.size_decr)
        x_adv = ops.apgd_init(x, self.eps, self.norm, draw=draw, seed=seed)
        x_best = x_adv.clone()
        x_best_adv = x_adv.clone()
        state = ApgdState.new(B, self.steps, self.eps, x.device)
        grad = self._evaluate(x_adv, y, state, "start")
        grad_best = grad.clone()

        checks = dict(checkpoint_schedule(self.steps))
        step = ops.apgd_linf_step if self.norm == "Linf" else ops.apgd_l2_step
        cur, prev = x_adv, x_adv.clone()                          # x_adv, x_adv_old
        for i in range(self.steps):
            a = 0.75 if i > 0 else 1.0
            # the new point is written over x_adv_old's buffer: x_adv_old of the next step is this step's x_adv
            cur, prev = step(cur, prev, grad, x, state.step_size, self.eps, a, out=prev), cur
            grad = self._evaluate(cur, y, state, "step", i)
            if i in checks:
                ops.apgd_checkpoint(state, i, checks[i], self.thr_decr)
            ops.apgd_track(cur, grad, x_best, grad_best, x_best_adv, state.flags)
        return state.acc, x_best_adv

    # ---- perturb(cheap=True) (apgd.py:216-251) -------------------------------------------------------------------------

    def forward(self, images, labels):
        x, y, _ = self._prepare(images, labels)
        y = y.to(torch.int64).contiguous()
        adv = x.clone()
        with torch.no_grad():
            z = self.model(x)
        acc = (z.reshape(-1) > 0).to(torch.int64) == y           # argmax(cat([-z, z], 1)) == y
        if self.verbose:
            print("-------------------------- running {}-attack with epsilon {:.4f} --------------------------".format(
                self.norm, self.eps))
            print("initial accuracy: {:.2%}".format(acc.float().mean()))
        startt = time.time()
        torch.manual_seed(self.seed)
        draws = self._init_noise
        for counter in range(self.n_restarts):
            ind_to_fool = acc.nonzero().reshape(-1)              # host synchronisation: gather the rows still correct
            if ind_to_fool.numel() == 0:
                continue
            x_to_fool, y_to_fool = x[ind_to_fool].contiguous(), y[ind_to_fool].contiguous()
            draw = draws[counter] if isinstance(draws, (list, tuple)) else draws
            if draw is not None:
                acc_curr, adv_curr = self._single_run(x_to_fool, y_to_fool,
                                                      draw=draw.to(self.device)[ind_to_fool].contiguous())
            else:
                acc_curr, adv_curr = self._single_run(x_to_fool, y_to_fool, seed=self._fresh_seed())
            fooled = acc_curr == 0
            rows = ind_to_fool[fooled]                           # host synchronisation: scatter the fooled rows back
            acc[rows] = False
            adv[rows] = adv_curr[fooled]
            if self.verbose:
                print("restart {} - robust accuracy: {:.2%} - cum. time: {:.1f} s".format(
                    counter, acc.float().mean(), time.time() - startt))
        return adv
