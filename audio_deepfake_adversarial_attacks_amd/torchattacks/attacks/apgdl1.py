"""l1-APGD: APGD for the L1 threat model (no counterpart in the reference tree, whose apgd.py has no L1 branch)."""
from dataclasses import dataclass

import torch

from ..attack import Attack
from .apgd import APGD, ApgdState


@dataclass
class ApgdL1State(ApgdState):
    """ApgdState plus the two per-row quantities of the sparsity schedule."""

    topk: torch.Tensor = None      # (B) float32: the fraction of coordinates the next step moves
    sp_old: torch.Tensor = None    # (B) float32: non-zeros of the best perturbation at the last checkpoint

    @classmethod
    def new(cls, B: int, steps: int, eps: float, device, T: int) -> "ApgdL1State":
        st = super().new(B, steps, eps, device)
        f32 = dict(dtype=torch.float32, device=device)
        st.step_size = torch.full((B,), eps, **f32)                      # alpha = 1: the first step may cross the whole ball
        st.topk = torch.full((B,), 0.2, **f32)
        st.sp_old = torch.full((B,), float(T), **f32)
        return st


class APGDL1(APGD):
    r"""l1-APGD in the paper 'Mind the box: l1-APGD for sparse adversarial attacks on image classifiers' (Croce & Hein,
    ICML 2021) [https://arxiv.org/abs/2103.01208] [https://github.com/fra31/auto-attack]: the L1 member of AutoAttack.

    Distance Measure : L1

    Arguments:
        model (nn.Module): model to attack.
        eps (float): maximum L1 norm of the perturbation. (Default: 20.0)
        steps (int): number of steps. (Default: 100)
        n_restarts (int): number of random restarts. (Default: 1)
        seed (int): random seed for the starting point. (Default: 0)
        eot_iter (int): number of iteration for EOT. (Default: 1)
        verbose (bool): print progress. (Default: False)

    Each iteration moves only the coordinates whose |gradient| is among the row's top-k, by sign, with the step spread over
    their number, and projects exactly onto the intersection of the L1 ball with the box [0, 1] (not onto the ball and then
    the box, which shrinks the perturbation: the paper's point).  Every k = max(int(0.04 steps), 1) iterations the sparsity
    of the best point sets the next top-k fraction; the step size restarts at eps when the sparsity fell by more than 5 %
    (with a reset to the best point) and otherwise decays by 1.5, within [eps / 10, eps].  No momentum.

    Untargeted, cross-entropy of cat([-z, z], 1) only.  The restart / gather / scatter logic, the evaluation (EOT included),
    the randomness and `set_init_noise` (a full-batch (B, T) draw of N(0, 1), or a list with one per restart) are APGD's.
    Both per-iteration operations run on the device without sorting (hip_ops.apgdl1_step); the loop never synchronises
    with the host.

    Examples::
        >>> attack = torchattacks.APGDL1(model, eps=20.0, steps=100, n_restarts=1, seed=0, eot_iter=1, verbose=False)
        >>> adv_images = attack(images, labels)
    """

    def __init__(self, model, eps=20.0, steps=100, n_restarts=1, seed=0, eot_iter=1, verbose=False):
        Attack.__init__(self, "APGDL1", model)
        self.eps = eps
        self.steps = steps
        self.norm = "L1"
        self.n_restarts = n_restarts
        self.seed = seed
        self.eot_iter = eot_iter
        self.verbose = verbose
        self._supported_mode = ["default"]
        if not eps > 0:
            raise ValueError(f"APGDL1 eps must be positive, got {eps!r}")

    def _single_run(self, x, y, draw=None, seed=None):
        """One restart over the rows (x, y).  Returns (acc (B) uint8, x_best_adv (B, T))."""
        ops = self.ops
        B, T = x.shape[0], x[0].numel()
        k = max(int(0.04 * self.steps), 1)
        x_adv = ops.apgdl1_init(x, self.eps, draw=draw, seed=seed)
        x_best = x_adv.clone()
        x_best_adv = x_adv.clone()
        state = ApgdL1State.new(B, self.steps, self.eps, x.device, T)
        grad = self._evaluate(x_adv, y, state, "start")
        grad_best = grad.clone()
        for i in range(self.steps):
            ops.apgdl1_step(x_adv, grad, x, state.step_size, state.topk, self.eps, out=x_adv)
            grad = self._evaluate(x_adv, y, state, "step", i)
            if (i + 1) % k == 0:
                ops.apgdl1_checkpoint(x_adv, x_best, x, state, self.eps)
            ops.apgd_track(x_adv, grad, x_best, grad_best, x_best_adv, state.flags)
        return state.acc, x_best_adv
