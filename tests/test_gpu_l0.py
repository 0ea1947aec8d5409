"""`-m gpu`: the L0 kernels (include/advstep_l0.h) against the CPU table tests/l0_cpu_ops.py on identical inputs, and whole PGDL0
attacks on the detectors with every launch recomputed on the CPU table from its own inputs.

What is bit-exact: everything.  The scores are elementwise IEEE arithmetic without contraction, the selection (threshold, count
above it, tie cut) is exact, and the one reduced quantity, gnorm = sum |g|, is handed to the table as the device computed it.
No tolerance appears below except the two derived ones:
    gnorm      a float32 sum of T non-negative terms in any order is within gamma_(T-1) = (T - 1) u / (1 - (T - 1) u), u = 2^-24,
               of the exact sum, relative (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2).
    float64    test_projection_against_float64: per-sample value bound u (|d_i| + 1) (one rounding of d, one of x + c), per-score
               bound E_i = 1.01 u (5 d_i^2 + 4 r_i^2 + 2 |r_i|) (the roundings of d, of 1 - x, of r, of the two squares and of
               their difference, first order, 1 % for the higher orders).

Measured on gfx950 by test_projection_against_float64 ((3, 64 600): x + N(0, 1), a 10 %-sparse 1e-3 step, the tie row
x = 0.5, u = x +- 0.25), k in {64, 1024} x eps_inf in {inf, 0.05}:
    swapped indices per row: 0, 0, 0 in all four cases (the float32 and the float64 kept sets are the same sets; the tie row's
    scores are exactly equal in both precisions, so the index rule picks the same samples)
    max |device - f64| on the kept samples: 0 without the cap (x + (u - x) is exact on these rows), 1.1e-8 (k = 64) and
    1.9e-8 (k = 1024) with eps_inf = 0.05, against a bound of u (|d| + 1) >= 6.0e-8."""
import copy
import functools
import math

import pytest
import torch

from tests import l0_cpu_ops as C
from tests.test_gpu_apgd import atk_call_context, detector, hip, same
from tests.test_gpu_apgdl1 import _evaluate_synthetic, attack_inputs, box_rows, with_canary
from tests.test_gpu_row_edges import NAN, identical, on_routes

pytestmark = pytest.mark.gpu

SHAPES = [(1, 257), (5, 4099), (3, 64_600)]
T_FULL = 64_600
U = 2.0 ** -24
INF = math.inf
ALPHA = 0.15                                   # the attack's step per dimension: the kernel's step is ALPHA * T


def cases(T):
    """(k, eps_inf): k in {1, 16, T} x eps_inf in {inf, 0.05}, and k = T + 5 once."""
    return [(k, e) for k in (1, 16, T) for e in (INF, 0.05)] + [(T + 5, INF)]


def gnorm_bound(grad):
    """|float32 sum in any order - exact sum| for the rows of |grad|, from the module docstring."""
    T = grad.shape[1]
    return (T - 1) * U / (1 - (T - 1) * U) * grad.double().abs().sum(dim=1)


def tie_row(x_row):
    """x = 0.5 away from the exact 0s and 1s: every interior sample then moves by one of two amounts."""
    return torch.where((x_row == 0.0) | (x_row == 1.0), x_row, torch.full_like(x_row, 0.5))


def projection_inputs(B, T, seed):
    """(x, u): rows cycle through x + N(0, 1); a 10 %-sparse step of 1e-3 N(0, 1); the tie input x = 0.5, u = x +- 0.25."""
    x, g = box_rows(B, T, seed)
    u = torch.empty(B, T)
    for r in range(B):
        noise = torch.randn(T, generator=g)
        if r % 3 == 0:
            u[r] = x[r] + noise
        elif r % 3 == 1:
            u[r] = x[r] + 1e-3 * noise * (torch.rand(T, generator=g) < 0.1)
        else:
            x[r] = tie_row(x[r])
            u[r] = x[r] + 0.25 * torch.sign(noise)
    return x, u


def step_inputs(B, T, k, seed):
    """x with exact 0s and 1s, a sparse current point in the box, gradients with zeros; row 1 (B > 1): a zero gradient and a
    current point with min(k, 5) samples off x (feasible: it must come back bit for bit); the last row (B > 2): the tie row,
    cur = x = 0.5 off the edges, g = 1e-3 sign(noise)."""
    x, g = box_rows(B, T, seed)
    cur = (x + torch.randn(B, T, generator=g) * (torch.rand(B, T, generator=g) < 0.1) * 1e-3).clamp(0.0, 1.0)
    grad = torch.randn(B, T, generator=g) * 1e-3
    grad[:, ::13] = 0.0
    if B > 1:
        grad[1] = 0.0
        cur[1] = x[1]
        off = torch.tensor([1, 2, 3, 4, 6])[:min(k, 5)]                      # interior samples of box_rows: x >= 0.01
        cur[1, off] = x[1, off] + 1e-3
        assert (cur[1] <= 1).all() and ((x[1] + (cur[1] - x[1])) == cur[1]).all()
    if B > 2:
        x[-1] = tie_row(x[-1])
        cur[-1] = x[-1]
        grad[-1] = 1e-3 * torch.sign(torch.randn(T, generator=g))
    return x, cur, grad


def check_ball(out, x, k, eps_inf):
    """#{out != x} <= k per row, the box and the cap as float32 forms their bounds."""
    out, x = out.cpu(), x.cpu()
    assert ((out != x).sum(dim=1) <= k).all()
    assert out.min() >= 0 and out.max() <= 1 and torch.isfinite(out).all()
    if eps_inf != INF:
        e = torch.tensor(eps_inf, dtype=torch.float32)
        assert (out <= x + e).all() and (out >= x - e).all()


@pytest.mark.parametrize("B,T", SHAPES)
def test_projection_kernel(cuda, B, T):
    ops = hip()
    x, u = projection_inputs(B, T, 10)
    xd, ud = x.to(cuda), u.to(cuda)
    for k, eps_inf in cases(T):
        out, canary = with_canary(torch.full((B, T), NAN), cuda)
        got = ops.l0_box_project(xd, ud, k, eps_inf, out=out)
        assert got.data_ptr() == out.data_ptr() and (canary == 7.0).all()
        assert same(got, C.l0_box_project(x, u, k, eps_inf)), (k, eps_inf)   # bit for bit
        assert same(got, ops.l0_box_project(xd, ud, k, eps_inf))            # a rerun is bit-identical
        alias = ud.clone()
        ops.l0_box_project(xd, alias, k, eps_inf, out=alias)                # out aliasing u
        assert same(alias, got)
        check_ball(got, x, k, eps_inf)
        if B > 2 and k < T:                                                 # the tie row: more equal scores than places
            _, s = C.scores(x[2:3], u[2:3], eps_inf)
            keep, order = C.kept_mask(s, k)
            thr = s[0, order[0, k - 1]]
            assert (s == thr).sum() > (keep & (s == thr)).sum() >= 1
            assert (got[2].cpu() != x[2]).sum() == k


def short_tie_rows(T, layout):
    """(x, u, ties) for B = 2, x = 0.5.  "all": u = x +- 0.25, every sample ties.  "odd": u = x + 0.25 (row 1: - 0.25) on odd i
    and x + 0.125 on even i, so only the odd indices tie at the threshold of every k <= T // 2 and the kept ties are not a prefix
    of the row.  ties: how many samples share the largest score."""
    x = torch.full((2, T), 0.5)
    if layout == "all":
        sign = torch.sign(torch.randn(2, T, generator=torch.Generator().manual_seed(70 + T)))
        return x, x + 0.25 * sign, T
    u = x + 0.125
    u[0, 1::2] = 0.75
    u[1, 1::2] = 0.25
    return x, u, T // 2


@pytest.mark.parametrize("layout", ["all", "odd"])
@pytest.mark.parametrize("T", [2, 3, 8, 9, 64, 65])
def test_projection_short_rows_index_cut(cuda, T, layout):
    """Rows whose index has 1, 2, 3, 3 + 1, 6 and 6 + 1 bits: the cut search with fewer bits than one digit, exactly one digit,
    whole digits and a one-bit last digit.  Bit for bit against the table, whose kept set is written out here as well: the
    lowest-index min(k, ties) samples of the top score, then (k = T) everything."""
    ops = hip()
    x, u, ties = short_tie_rows(T, layout)
    top = torch.arange(T) if layout == "all" else torch.arange(1, T, 2)
    xd, ud = x.to(cuda), u.to(cuda)
    for k in sorted({1, ties - 1, T} - {0}):
        for eps_inf in (INF, 0.05):
            want = C.l0_box_project(x, u, k, eps_inf)
            kept = torch.zeros(T, dtype=torch.bool)
            kept[top[:k]] = True
            if k == T:
                kept[:] = True
            assert ((want != x) == kept).all(), (k, eps_inf)                    # the table keeps the set described above
            out, canary = with_canary(torch.full((2, T), NAN), cuda)
            got = ops.l0_box_project(xd, ud, k, eps_inf, out=out)
            assert (canary == 7.0).all()
            assert same(got, want), (k, eps_inf, got.cpu(), want)               # bit for bit
            alias = ud.clone()
            ops.l0_box_project(xd, alias, k, eps_inf, out=alias)                # out aliasing u
            assert same(alias, got)


@pytest.mark.parametrize("B,T", SHAPES)
def test_step_kernel(cuda, B, T):
    ops = hip()
    step = ALPHA * T
    for k, eps_inf in cases(T):
        kk = min(k, T)
        x, cur, grad = step_inputs(B, T, k, 20)
        xd, cd, gd = x.to(cuda), cur.to(cuda), grad.to(cuda)
        out, canary = with_canary(torch.full((B, T), NAN), cuda)
        got, stats = ops.pgdl0_step(cd, gd, xd, step, k, eps_inf, out=out, return_stats=True)
        assert got.data_ptr() == out.data_ptr() and (canary == 7.0).all()
        stats = stats.cpu()
        gn = stats[:, 0]
        assert ((gn.double() - grad.double().abs().sum(dim=1)).abs() <= gnorm_bound(grad)).all()
        want, wstats = C.pgdl0_step(cur, grad, x, step, k, eps_inf, return_stats=True, gnorm=gn)
        assert same(stats, wstats), (k, eps_inf, stats, wstats)             # gnorm, threshold, count above, last kept tie
        assert same(got, want), (k, eps_inf)                                # bit for bit
        check_ball(got, x, k, eps_inf)
        if B > 1:
            assert gn[1] == 0 and same(got[1], cur[1])                      # the zero-gradient row: cur itself
        if B > 2:                                                           # the tie row: the cut decides
            _, s = C.scores(x[-1:], C.step_point(cur[-1:], grad[-1:], step, gn[-1:]), eps_inf)
            keep, _ = C.kept_mask(s, k)
            thr, gt = stats[-1, 1], stats[-1, 2]
            kept_ties = (keep & (s == thr)).sum()
            assert gt + kept_ties == kk and gt < k
            if k < T:
                assert (s == thr).sum() > kept_ties                         # ties were left out: the second search ran
        again, stats2 = ops.pgdl0_step(cd, gd, xd, step, k, eps_inf, return_stats=True)
        assert same(again, got) and same(stats2, stats)                     # a rerun is bit-identical
        alias = cd.clone()
        ops.pgdl0_step(alias, gd, xd, step, k, eps_inf, out=alias)          # out aliasing cur
        assert same(alias, got)
        assert same(ops.pgdl0_step(cd, gd, xd, step, k, eps_inf), got)      # without stats


@pytest.mark.parametrize("B,T", SHAPES)
def test_nan_gradient_terminates_and_writes_every_sample(cuda, B, T):
    ops = hip()
    x, cur, grad = step_inputs(B, T, 16, 21)
    clean = ops.pgdl0_step(cur.to(cuda), grad.to(cuda), x.to(cuda), ALPHA * T, 16)
    grad[0, 7] = NAN
    out, canary = with_canary(torch.full((B, T), 7.0), cuda)
    got, stats = ops.pgdl0_step(cur.to(cuda), grad.to(cuda), x.to(cuda), ALPHA * T, 16, out=out, return_stats=True)
    torch.cuda.synchronize()                                                # it terminated
    assert (canary == 7.0).all() and not (got == 7.0).any()                 # every in-row sample written, nothing past them
    assert torch.isnan(stats[0, 0]) and same(got[1:], clean[1:])            # the other rows never see it


def test_unaligned_views_take_the_scalar_route_with_equal_bits(cuda):
    """T % 4 == 0 with a row base one float past a 16-byte boundary: the sample route.  The projection has no reduced
    quantity, so every route gives the same bytes; the step is compared with the table under each route's own gnorm."""
    ops = hip()
    B, T, k, step = 3, 4100, 16, ALPHA * 4100
    for eps_inf in (INF, 0.05):
        x, u = projection_inputs(B, T, 30)
        want = C.l0_box_project(x, u, k, eps_inf)

        def project(p, alias=False):
            xd, ud = p("x", x), p("u", u)
            return (ops.l0_box_project(xd, ud, k, eps_inf, out=ud if alias else p("out", x.shape)),)

        res = on_routes(cuda, T, ("x", "u", "out"), project)
        identical(res)
        assert same(res["aligned"][0], want) and len(res) == 5
        for label, (got,) in on_routes(cuda, T, ("x", "u"), functools.partial(project, alias=True), single=False).items():
            assert same(got, want), label

        x, cur, grad = step_inputs(B, T, k, 31)

        def launch(p, alias=False):
            c, g, xd = p("cur", cur), p("grad", grad), p("x", x)
            return ops.pgdl0_step(c, g, xd, step, k, eps_inf, out=c if alias else p("out", x.shape), return_stats=True)

        res = on_routes(cuda, T, ("cur", "grad", "x", "out"), launch)
        res.update({f"alias {label}": v for label, v in
                    on_routes(cuda, T, ("cur", "grad", "x"), functools.partial(launch, alias=True), single=False).items()})
        assert len(res) == 8
        for label, (got, stats) in res.items():
            assert ((stats[:, 0].double() - grad.double().abs().sum(dim=1)).abs() <= gnorm_bound(grad)).all(), label
            want, wstats = C.pgdl0_step(cur, grad, x, step, k, eps_inf, return_stats=True, gnorm=stats[:, 0])
            assert same(got, want) and same(stats, wstats), label
            check_ball(got, x, k, eps_inf)


@pytest.mark.parametrize("T", [4, 5])
def test_rows_beyond_one_grid(cuda, T):
    """65 537 rows: the grid holds 65 535 workgroups, so the last two rows are the second trip of `row += gridDim.x`.  T = 4 is
    the float4 route, T = 5 the scalar one.  Every output starts as NaN and must equal the table's on every row."""
    ops = hip()
    R, k = 65537, 2
    g = torch.Generator().manual_seed(60 + T)
    x = torch.rand(R, T, generator=g)
    x[:, 0] = 0.0
    x[1::5, 1] = 1.0
    kind = torch.arange(R) % 3
    kind[R - 2:] = torch.tensor([0, 2])
    noise = torch.randn(R, T, generator=g)
    x = torch.where((kind == 2)[:, None], torch.full_like(x, 0.5), x)
    u = torch.where((kind == 0)[:, None], x + noise, torch.where((kind == 1)[:, None], x, x + 0.25 * torch.sign(noise)))
    grad = torch.where((kind == 2)[:, None], 1e-3 * torch.sign(noise), 1e-3 * torch.randn(R, T, generator=g))
    grad[1::7] = 0.0
    cur = torch.where((kind == 0)[:, None], (x + 1e-3 * noise).clamp(0.0, 1.0), x)
    xd = x.to(cuda)
    for eps_inf in (INF, 0.05):
        got = ops.l0_box_project(xd, u.to(cuda), k, eps_inf, out=torch.full((R, T), NAN, device=cuda))
        assert same(got, C.l0_box_project(x, u, k, eps_inf))
        check_ball(got, x, k, eps_inf)
        got, stats = ops.pgdl0_step(cur.to(cuda), grad.to(cuda), xd, ALPHA * T, k, eps_inf,
                                    out=torch.full((R, T), NAN, device=cuda), return_stats=True)
        want, wstats = C.pgdl0_step(cur, grad, x, ALPHA * T, k, eps_inf, return_stats=True, gnorm=stats[:, 0])
        assert same(got, want) and same(stats, wstats)
        assert ((stats[:, 0].cpu().double() - grad.double().abs().sum(dim=1)).abs() <= gnorm_bound(grad)).all()
        check_ball(got, x, k, eps_inf)


def test_projection_against_float64(cuda):
    """The device's float32 projection against the same definitions in float64 on the real row length.  Where the kept sets
    agree the values agree to float32 rounding; where they differ, every swapped pair's float64 scores lie within the float32
    rounding of a score of each other (bounds: module docstring)."""
    ops = hip()
    B, T = 3, T_FULL
    x, u = projection_inputs(B, T, 50)
    x64, u64 = x.double(), u.double()
    d = u64 - x64
    for k in (64, 1024):
        for eps_inf in (INF, 0.05):
            got = ops.l0_box_project(x.to(cuda), u.to(cuda), k, eps_inf).cpu()
            cap = torch.tensor(eps_inf, dtype=torch.float32).item()         # the cap as the kernel receives it
            ref = C.project(x64, u64, k, cap)
            c64, s64 = C.scores(x64, u64, cap)
            keep64, _ = C.kept_mask(s64, k)
            keep32 = got != x                                               # every kept sample of these rows moves
            assert (keep32.sum(dim=1) == k).all()
            r = d - c64
            E = 1.01 * U * (5 * d * d + 4 * r * r + 2 * r.abs())
            agree = keep32 & keep64
            assert ((got.double() - ref).abs()[agree] <= (U * (d.abs() + 1))[agree]).all()
            assert same(got[~keep32], x[~keep32])
            swapped = []
            for b in range(B):
                only32, only64 = keep32[b] & ~keep64[b], keep64[b] & ~keep32[b]
                assert only32.sum() == only64.sum()
                swapped.append(int(only32.sum()))
                if swapped[-1]:
                    assert (s64[b] - E[b])[only64].max() <= (s64[b] + E[b])[only32].min()
            print(f"L0 projection vs float64, k = {k}, eps_inf = {eps_inf}: swapped per row {swapped}, "
                  f"max |device - f64| on the agreed set {(got.double() - ref).abs()[agree].max().item():.3e}")


# ---- whole attacks ---------------------------------------------------------------------------------------------------------

class Recording:
    """hip_ops with every L0 launch recomputed by the CPU table from copies of the launch's own inputs (the step under the
    device's gnorm, which is held to its derived bound)."""

    def __init__(self):
        self.ops, self.calls = hip(), {}

    def __getattr__(self, name):
        fn = getattr(self.ops, name)
        if name not in ("pgdl0_step", "l0_box_project"):
            return fn

        def run(*args, **kw):
            self.calls[name] = self.calls.get(name, 0) + 1
            snap = [a.clone() if isinstance(a, torch.Tensor) else copy.deepcopy(a) for a in args]
            kw_in = {k: v for k, v in kw.items() if k != "out"}
            if name == "l0_box_project":
                res = fn(*args, **kw)
                assert same(res, C.l0_box_project(*snap, **kw_in))
                return res
            res, stats = fn(*args, **kw, return_stats=True)
            grad = snap[1].cpu()
            assert ((stats[:, 0].cpu().double() - grad.double().abs().sum(dim=1)).abs() <= gnorm_bound(grad)).all()
            want, wstats = C.pgdl0_step(*snap, **kw_in, return_stats=True, gnorm=stats[:, 0])
            assert same(res, want) and same(stats, wstats)
            return res
        return run


def l0_attack(model, k, steps, eps_inf=None, draw=None):
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    atk = torchattacks.PGDL0(model, k=k, steps=steps, eps_inf=eps_inf)
    atk.set_training_mode(model_training=True, batchnorm_training=False)
    if draw is not None:
        atk.set_init_noise(draw)
    return atk


def differing(a, b):
    """(samples that differ per row, the largest difference): what a failed comparison prints."""
    return (a != b).sum(dim=1).tolist(), (a - b).abs().max().item()


@pytest.fixture()
def fresh_graphs():
    from audio_deepfake_adversarial_attacks_amd.torchattacks import graphed
    graphed.clear()
    yield graphed
    graphed.clear()


@pytest.mark.parametrize("model_name", ["lcnn", "specrnet"])
def test_pgdl0_on_detectors_every_launch_checked(cuda, fresh_graphs, monkeypatch, model_name):
    """Every launch of a PGDL0 run recomputed on the table, then eager against graph replay (eager, captured, replayed).

    The replayed calls are compared ON THE DEVICE (`torch.equal`, as every graph test of the suite compares), not through
    `same()`: a device-to-host copy of a whole (B, T) result between two calls makes the later, replayed calls on SpecRNet
    differ from the eager loop - for every graph-replayed attack, the unchanged PGD included, and with nothing of this attack
    involved.  Measured on gfx950 (B = 3 and 4, 5 steps, two repetitions each): with `result.cpu()` after every call the calls
    under replay read = = X X X for PGD and for PGDL0 alike (the replayed model graph hands step 0 a gradient that differs
    from the eager one in 2 510 samples per row, values up to 3e28, although its input is the eager input bit for bit; the
    step kernel still equals the table on what it is given); with `torch.cuda.synchronize()` instead, or with nothing, they
    read = = = = =.  LCNN reads = = = = = either way.  The cause lies below this attack, in how a captured graph is replayed
    after such a copy, and was not found."""
    model = detector(model_name, cuda)
    x01, y = attack_inputs(model, cuda, 33)
    x01, y = x01[:4].contiguous(), y[:4].contiguous()
    draw = torch.rand(x01.shape, generator=torch.Generator().manual_seed(7)) * 2 - 1
    for k, eps_inf in ((64, None), (1024, 0.05)):
        rec = Recording()
        atk = l0_attack(model, k, 3, eps_inf, draw)
        atk.ops = rec
        adv = atk(x01, y)
        assert rec.calls == {"l0_box_project": 1, "pgdl0_step": 3}
        assert atk.last_changed.dtype == torch.int64 and atk.last_changed.device == x01.device
        assert same(atk.last_changed, (adv != x01).sum(dim=1)) and (atk.last_changed <= k).all() and atk.last_changed.max() > 0
        check_ball(adv, x01, k, INF if eps_inf is None else eps_inf)
        assert adv.data_ptr() != x01.data_ptr()
    # eager and graph replay: 5 steps = two replayed pairs and one eager step
    monkeypatch.setenv("ADVSTEP_ATTACK_GRAPH", "0")
    eager = l0_attack(model, 64, 5, None, draw)(x01, y)
    again = l0_attack(model, 64, 5, None, draw)(x01, y)
    assert torch.equal(again, eager), "the eager loop itself is not reproducible"
    assert len(fresh_graphs._GRAPHS) == 0
    changed = (eager != x01).sum(dim=1)
    monkeypatch.setenv("ADVSTEP_ATTACK_GRAPH", "1")
    atk = l0_attack(model, 64, 5, None, draw)
    for call, held in enumerate((0, 1, 1)):                                 # eager, captured + replayed, replayed
        got = atk(x01, y)
        assert torch.equal(got, eager), (call, differing(got, eager))
        assert torch.equal(atk.last_changed, changed) and len(fresh_graphs._GRAPHS) == held
    other = l0_attack(model, 64, 5, None, draw)                             # another object, the first one's capture
    assert torch.equal(other(x01, y), eager) and len(fresh_graphs._GRAPHS) == 1


def test_pgdl0_iteration_loop_never_synchronises(cuda, monkeypatch):
    monkeypatch.setenv("ADVSTEP_ATTACK_GRAPH", "0")
    model = detector("lcnn", cuda)
    x01, y = attack_inputs(model, cuda, 34)
    x01, y = x01[:4].contiguous(), y[:4].contiguous()
    atk = l0_attack(model, 64, 3)
    atk(x01, y)                                                             # warm-up: plans, kernels loaded
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            torch.ones(1, device=cuda).item()                               # the mode works on this build
        with atk_call_context(atk):
            adv = atk.forward(x01, y)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert adv.shape == x01.shape and atk.last_changed.shape == (4,) and atk.last_changed.is_cuda


def test_evaluation_loop_reports_sparsity(cuda):
    rep = _evaluate_synthetic(cuda, "PGDL0")
    assert rep["num_total"] == 16 and 0.0 <= rep["adv_eval/accuracy"] <= 100.0
    assert {k for k in rep if k.startswith("sparse/")} == {"sparse/changed_mean", "sparse/changed_median", "sparse/changed_max",
                                                           "sparse/k"}
    assert rep["sparse/k"] == 64 and 0 < rep["sparse/changed_max"] <= 64
    assert 0 < rep["sparse/changed_mean"] <= rep["sparse/changed_max"]
    assert not any(k.startswith("sparse/") for k in _evaluate_synthetic(cuda, "PGD"))
