"""TEST INFRASTRUCTURE — hip_ops.multi_route (include/advstep_multi.h) restated in torch by plain indexing, on whatever device
its inputs live; every other op is tests/momentum_cpu_ops'.  The table can stand in for hip_ops inside MultiAttack and can
recompute a GPU launch from its own inputs."""
import torch

from tests import momentum_cpu_ops as _base

NAME = "multiattack_cpu"


def __getattr__(name):  # every op this table does not restate
    return getattr(_base, name)


def multi_route(adv, x, z, labels, rows, final, next_x=None, next_y=None, next_rows=None):
    """multiattack.py:55-66 for one stage: pre = z > 0 (the first maximal index of cat([-z, z], 1)); wrong rows of adv go to
    final[rows], the others are compacted in order.  Rows past counts[1] of the next_* buffers are left as they were."""
    n = adv.shape[0]
    pre = (z.reshape(-1) > 0).to(torch.int64)
    wrong = pre != labels.reshape(-1)
    keep = ~wrong
    k = int(keep.sum())
    next_x = torch.empty_like(x) if next_x is None else next_x
    next_y = torch.empty(n, dtype=torch.int64, device=x.device) if next_y is None else next_y
    next_rows = torch.empty(n, dtype=torch.int32, device=x.device) if next_rows is None else next_rows
    with torch.no_grad():
        final[rows[wrong].long()] = adv[wrong]
        next_x[:k] = x[keep]
        next_y[:k] = labels[keep]
        next_rows[:k] = rows[keep]
    counts = torch.tensor([n - k, k], dtype=torch.int32, device=x.device)
    return next_x, next_y, next_rows, counts


class ReferenceLoss(_base.ReferenceLoss):
    """momentum_cpu_ops.ReferenceLoss (the reference's loss arithmetic) over this table."""

    def __getattr__(self, name):
        return getattr(__import__(__name__, fromlist=["_"]), name)
