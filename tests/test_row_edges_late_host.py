"""CPU: the inputs of tests/test_gpu_row_edges_late.py and the conditions its assertions rely on, at every (B, T) that module
runs.  The generators of tests/test_gpu_fmn.py and tests/test_gpu_l0.py do not survive tests/test_gpu_row_edges.py's LENGTHS:
    step_inputs (L0)   pokes samples 1, 2, 3, 4, 6 of its feasible row: an IndexError at T = 1, 3, 4, 5.  l0_step_rows takes
                       the first min(k, 5, T) interior samples of that row instead (x >= 0.01 there; at T = 1 the one sample is
                       an exact 0, so the row is x itself) and zeroes grad[:, ::13] only where T > 1, as
                       test_gpu_row_edges.gradient does (at T = 1 that slice is the whole gradient).
    wave_inputs (FMN)  zeroes grad[:, ::13] (the whole gradient at T = 1) and, with orig from ball_rows (sample 0 is an exact 0),
                       leaves adv == orig in most rows at T = 1, so that step_case's branch table no longer matches its
                       want_copy.  fmn_rows builds orig in the interior at T = 1 and keeps the zeros for T > 1.
Everything asserted here is a condition on the inputs alone: the CPU twins (tests/fmn_cpu_ops.py, tests/l0_cpu_ops.py,
tests/multiattack_cpu_ops.py) run on them, no kernel does.  Where a length cannot hold an ingredient (a tie row with k >= T has
no tie left out; one row cannot go to both destinations) that is asserted here, and the GPU module skips that one assertion,
never the launch."""
import itertools

import pytest
import torch

from tests import fmn_cpu_ops as CF
from tests import l0_cpu_ops as CL0
from tests import multiattack_cpu_ops as CMA
from tests.test_gpu_apgd import same
from tests.test_gpu_apgdl1 import box_rows
from tests.test_gpu_fmn import step_case
from tests.test_gpu_l0 import ALPHA, INF, projection_inputs, tie_row
from tests.test_gpu_multiattack import PATTERNS, route_inputs
from tests.test_gpu_row_edges import LENGTHS, NAN, ball_rows, gen, gradient

FMN_BATCHES = (1, 8)                          # eight rows hold every branch of step_case
FMN_ALPHA, FMN_GAMMA = 0.37, 0.05
FMN_FILL = -2.5                               # best_adv before a launch: no sample of [0, 1]
L0_BATCHES = (1, 3)
L0_PROJECTION_SEED, L0_STEP_SEED = 10, 20
MULTI_ROUTE_N = (1, 5)
MULTI_SELECT_N = (63, 64, 65, 128, 129)       # either side of the select kernel's one and two 64-lane ballots
MULTI_SELECT_T = 5


# ---- FMN ---------------------------------------------------------------------------------------------------------------------------

def fmn_rows(B, T):
    """(adv, grad, orig) of tests/test_gpu_fmn.py's wave_inputs at any length.  By b % 8: 1 an all-zero gradient row, 5 a
    delta = 0 row, 6 a NaN in the gradient (at T // 2); every other row has a gradient that is not zero and max |delta| >= 1e-3,
    the floor below which step_case stops scaling its radii with the row's norm (short rows hold few samples to reach it: the
    first seed that does is taken, a condition on the inputs alone)."""
    scale = torch.tensor([0.003 * (1 + b % 3) for b in range(B)])[:, None]
    for seed in itertools.count(3200 + B + T):
        g = gen(seed)
        if T == 1:
            orig = 0.25 + 0.5 * torch.rand(B, T, generator=g)
            adv = (orig + (torch.rand(B, T, generator=g) * 2 - 1) * scale).clamp(0, 1)
        else:
            orig, adv = ball_rows(B, T, g, scale)
        if all((adv[b] - orig[b]).abs().max() >= 1e-3 for b in range(B) if b % 8 != 5):
            break
    grad = gradient(B, T, g, 0.05, nan=False)                           # zeros only where T > 1
    for b in range(B):
        if b % 8 == 1:
            grad[b] = 0.0
        if b % 8 == 5:
            adv[b] = orig[b]
        if b % 8 == 6:
            grad[b, T // 2] = NAN
    return adv, grad, orig


@pytest.mark.parametrize("norm", ["Linf", "L2"])
@pytest.mark.parametrize("T", LENGTHS)
@pytest.mark.parametrize("B", FMN_BATCHES)
def test_fmn_rows_keep_the_branch_table(B, T, norm):
    adv, grad, orig = fmn_rows(B, T)
    rows = torch.arange(B) % 8
    assert ((adv - orig) == 0).all(dim=1).tolist() == (rows == 5).tolist()          # exactly the b % 8 == 5 row has no delta
    assert ((adv - orig).abs().amax(dim=1)[rows != 5] >= 1e-3).all()
    assert torch.isnan(grad).any(dim=1).tolist() == (rows == 6).tolist()
    assert (grad == 0).all(dim=1).tolist() == (rows == 1).tolist()
    assert adv.min() >= 0 and adv.max() <= 1 and orig.min() >= 0 and orig.max() <= 1
    state, z, y, want_copy = step_case(adv, orig, norm)
    for move in (True, False):
        best = torch.full((B, T), FMN_FILL)
        new, out = CF.fmn_step(adv, grad, orig, z, y, state, best, CF.fmn_norms(adv, grad, orig), FMN_ALPHA, FMN_GAMMA, norm,
                               move=move)
        copied = (best != FMN_FILL).any(dim=1)
        assert copied.tolist() == want_copy                                         # the twin's copied rows
        assert same(best[copied], adv[copied]) and (best[~copied] == FMN_FILL).all()
        assert not torch.isnan(new[0][rows != 6]).any()                             # eps': finite or +inf, never NaN
        assert (new[0][rows == 5] == 0).all() and torch.isinf(new[0][rows == 1]).all()
        if move:
            assert same(out[rows == 5], orig[rows == 5])                            # eps' = 0: the clean row
            assert torch.isnan(out[rows == 6]).all() and not torch.isnan(out[rows != 6]).any()


# ---- L0 ----------------------------------------------------------------------------------------------------------------------------

def l0_cases(T):
    """(k, eps_inf): k in {1, min(16, T), T} x eps_inf in {inf, 0.05}, and k = T + 5 with inf only (test_gpu_l0.cases)."""
    return [(k, e) for k in sorted({1, min(16, T), T}) for e in (INF, 0.05)] + [(T + 5, INF)]


def l0_projection_rows(B, T):
    """test_gpu_l0.projection_inputs, which holds at every length: the tie row is row 2 (x = 0.5 off the exact 0s and 1s)."""
    return projection_inputs(B, T, L0_PROJECTION_SEED)


def l0_step_rows(B, T, k):
    """test_gpu_l0.step_inputs at any length (the module docstring has the two differences): (x, cur, grad); row 1 (B > 1) has
    no gradient and a feasible current point, the last row (B > 2) is the tie row."""
    x, g = box_rows(B, T, L0_STEP_SEED)
    cur = (x + torch.randn(B, T, generator=g) * (torch.rand(B, T, generator=g) < 0.1) * 1e-3).clamp(0.0, 1.0)
    grad = torch.randn(B, T, generator=g) * 1e-3
    if T > 1:
        grad[:, ::13] = 0.0
    if B > 1:
        grad[1] = 0.0
        cur[1] = x[1]
        off = ((x[1] != 0.0) & (x[1] != 1.0)).nonzero().reshape(-1)[:min(k, 5, T)]   # interior samples: x >= 0.01
        cur[1, off] = x[1, off] + 1e-3
        assert (cur[1] <= 1).all() and ((x[1] + (cur[1] - x[1])) == cur[1]).all()
    if B > 2:
        x[-1] = tie_row(x[-1])
        cur[-1] = x[-1]
        grad[-1] = 1e-3 * torch.sign(torch.randn(T, generator=g))
    return x, cur, grad


def ties_left_out(s, k):
    """(samples of the one row s that score exactly the k-th largest score, how many of them are kept)."""
    keep, order = CL0.kept_mask(s, k)
    thr = s[0, order[0, min(k, s.shape[1]) - 1]]
    return int((s == thr).sum()), int((keep & (s == thr)).sum())


@pytest.mark.parametrize("T", LENGTHS)
@pytest.mark.parametrize("B", L0_BATCHES)
def test_l0_rows_keep_their_ingredients(B, T):
    x, u = l0_projection_rows(B, T)
    assert x.min() >= 0 and x.max() <= 1 and torch.isfinite(u).all()
    for k, eps_inf in l0_cases(T):
        if B > 2 and k < T:                                                         # the projection's tie row: the cut decides
            ties, kept = ties_left_out(CL0.scores(x[2:3], u[2:3], eps_inf)[1], k)
            assert ties > kept >= 1
            assert (CL0.l0_box_project(x, u, k, eps_inf)[2] != x[2]).sum() == k
        xs, cur, grad = l0_step_rows(B, T, k)
        assert torch.isfinite(grad).all() and cur.min() >= 0 and cur.max() <= 1
        want, stats = CL0.pgdl0_step(cur, grad, xs, ALPHA * T, k, eps_inf, return_stats=True)
        assert (stats[:, 2] < k).all()                                              # fewer scores above the threshold than places
        assert stats[0, 0] > 0                                                      # row 0 has a gradient at every length
        if B > 1:
            assert stats[1, 0] == 0 and same(want[1], cur[1])                       # the feasible row comes back bit for bit
            assert (cur[1] != xs[1]).sum() == min(k, 5, T, int(((xs[1] != 0) & (xs[1] != 1)).sum()))
        if B > 2 and k < T:                                                         # the step's tie row: the second search runs
            s = CL0.scores(xs[-1:], CL0.step_point(cur[-1:], grad[-1:], ALPHA * T, stats[-1:, 0]), eps_inf)[1]
            ties, kept = ties_left_out(s, k)
            assert ties > kept >= 1 and stats[-1, 2] + kept == k
    assert [k for k, _ in l0_cases(T) if k < T] == ([] if T == 1 else [1, 1] if T <= 16 else [1, 1, 16, 16])


# ---- MultiAttack -------------------------------------------------------------------------------------------------------------------

def multi_rows(n, T, pattern):
    """test_gpu_multiattack.route_inputs from the first seed that sends rows to both destinations (n >= 2; a condition on
    the inputs alone): (adv, x, z, labels, rows, wrong, B)."""
    for seed in itertools.count(100 + n + T + PATTERNS.index(pattern)):
        got = route_inputs(n, T, pattern, seed)
        wrong = got[5]
        if n < 2 or (wrong.any() and not wrong.all()):
            return got


def multi_cases():
    """(n, T, pattern) of the copy kernel's grid and of the select kernel's wave seam."""
    r = [(n, T, p) for n in MULTI_ROUTE_N for T in LENGTHS for p in (("alternating", "random") if n > 1 else ("alternating",))]
    return r + [(n, MULTI_SELECT_T, p) for n in MULTI_SELECT_N for p in ("alternating", "random")]


@pytest.mark.parametrize("n,T,pattern", multi_cases())
def test_multi_rows_reach_both_destinations(n, T, pattern):
    adv, x, z, labels, rows, wrong, B = multi_rows(n, T, pattern)
    final = torch.zeros(B, T)
    *_, counts = CMA.multi_route(adv, x, z, labels, rows, final)
    assert counts.tolist() == [int(wrong.sum()), n - int(wrong.sum())]
    assert n < 2 or (counts[0] > 0 and counts[1] > 0)
    assert rows.dtype == torch.int32 and (rows[1:] > rows[:-1]).all() and 0 <= rows.min() and rows.max() < B
