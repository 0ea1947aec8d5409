"""`-m gpu`: the row kernels of apgd.hip, apgdl1.hip, momentum.hip, radius.hip and fab.hip at the seams of their two
geometries (csrc/row_tiles.h: 256 threads, 4096-sample tiles; csrc/row_workgroup.h: one 1024-thread workgroup per row, trips of
1024 samples or quads) and of their two load routes (float4 when T % 4 == 0 and every row base is 16-byte aligned, sample by
sample otherwise): LENGTHS holds the first and the last quad of a row, tiles and trips that are exactly full or hold one quad or
one sample, apgdl1.hip's prefetch not taken (4096), taken by thread 0 only (4100) and taken twice (8196).

Every length that is a multiple of four runs on the float4 route (all bases aligned), on the sample route (every row tensor,
the output included, one float past a 16-byte boundary) and, at T = 4, 4096 and 4100, with each row tensor shifted in turn.
Every device tensor lies between canary elements, inputs included.  No tolerance is new: each comes from the module that
measured or derived it at T = 64 600 (they grow with T).

What is bit-identical across the routes: everything in the row_tiles.h kernels (the sample route loads the same quad into the
same thread, the reductions have a fixed order, -ffp-contract=off); in the row_workgroup.h kernels, whose threads accumulate
in another order on the sample route, the selection results (the step's threshold and count, the checkpoint, fab_combine,
x1 / adv of fab_backward_step).  Everything else is held to its module's tolerance on each route.

The ball of apgd_l2_step.  tests/test_gpu_apgd.py asks ||out - x||_2 <= eps (1 + 1e-6) at T >= 257; at short rows that is not
a property of float32.  Measured on gfx950 at (3, 4096), a = 1.0, eps = 0.1, on the row without a gradient (d = cur - x, 373
samples on the ball's face): ||out - x||_2 / eps - 1 = 1.282e-6 for the device AND for the CPU table, -1.0e-11 for the float64
chain, while |device - f64| = |cpu table - f64| = 5.0e-8 per sample (L2_ATOL allows 4.8e-7 for the two together).  Neither side
is wrong: x = k 2^-24 (torch.rand) and the face samples all move by the same p = 0.003 eps / ||d||, so fl(x + p) - (x + p)
is one constant per binade of x instead of a zero-mean error, the norm grows by (sum e_i p_i) / eps^2 = 1.4e-6 in the first
projection, and the second projection's correction of 1.4e-6 * |p| = 3.6e-9 per sample is below half an ulp of x: it rounds
away.  So the invariant is asserted with the bound DERIVED from the format for the same arithmetic and the same summation
order (row_tiles.h's sum of squares), radius_cpu_ops.l2_ball_bound: eps (1 + ((n + 1) / 2 + 1) u + 3 u) + u sqrt(T),
u = 2^-24, n = 24 + ceil(ceil(T / 4096) / 256).  No constant in it was measured."""
import functools
import itertools

import numpy as np
import pytest
import torch

from oracle import fab as OF
from oracle import torch_ops as O
from tests import apgd_cpu_ops as CA
from tests import apgdl1_cpu_ops as CL
from tests import momentum_cpu_ops as CM
from tests import radius_cpu_ops as CR
from tests.test_gpu_apgd import L2_ATOL, hip, l2_step_f64, same, same_state
from tests.test_gpu_apgdl1 import L1_ATOL, L1_SLACK, check_box, eps_for, l1_excess
from tests.test_gpu_fab import TOL
from tests.test_gpu_minradius import RADII, check_l2_launch, round_case
from tests.test_gpu_momentum import U, chain, check_mi_launch

pytestmark = pytest.mark.gpu

LENGTHS = (1, 3, 4, 5, 255, 256, 1023, 1024, 1025, 4092, 4095, 4096, 4097, 4100, 8196)
BATCHES = (1, 3)
SINGLE = (4, 4096, 4100)                     # lengths at which each row tensor is shifted in turn
CANARY, PAD = -7.25, 64                      # PAD floats = 256 bytes: the view of a slot keeps its buffer's alignment
NAN = float("nan")


def grid(fn):
    return pytest.mark.parametrize("B", BATCHES)(pytest.mark.parametrize("T", LENGTHS)(fn))


# ---- placement: aligned or shifted bases, canaries on both sides -------------------------------------------------------------

class Slot:
    """A float32 device tensor inside a canary-filled allocation, its base on a 16-byte boundary (shift 0) or one float past it
    (shift 1: torch.empty(n + 1)[1:], as tests/test_gpu_universal.py builds its unaligned rows)."""

    def __init__(self, src, cuda, shift, fill=CANARY):
        shape = tuple(src.shape) if isinstance(src, torch.Tensor) else tuple(src)
        self.n, self.lo, self.fill = int(np.prod(shape)), PAD + shift, fill
        self.buf = torch.full((PAD + self.n + PAD + 1,), fill, dtype=torch.float32, device=cuda)
        self.t = self.buf[self.lo:self.lo + self.n].view(shape)
        assert self.t.data_ptr() % 16 == 4 * shift
        if isinstance(src, torch.Tensor):
            self.t.copy_(src)

    def intact(self):
        return bool((self.buf[:self.lo] == self.fill).all() and (self.buf[self.lo + self.n:] == self.fill).all())


class Placer:
    """place(name, src) -> the device tensor of a launch's row tensor `name`: a copy of the CPU tensor `src`, or for a shape an
    output left filled with the canary, at the shift the route gives that name."""

    def __init__(self, cuda, shifts):
        self.cuda, self.shifts, self.slots = cuda, shifts, []

    def __call__(self, name, src, fill=CANARY):
        self.slots.append(Slot(src, self.cuda, self.shifts[name], fill))
        return self.slots[-1].t

    def intact(self):
        return all(s.intact() for s in self.slots)


def routes(T, names, single=True):
    """(label, shift by name): all aligned; at T % 4 == 0 also all shifted and, at the SINGLE lengths, each name alone."""
    r = [("aligned", dict.fromkeys(names, 0))]
    if T % 4 == 0:
        r.append(("shifted", dict.fromkeys(names, 1)))
        if single and T in SINGLE:
            r += [(f"only {n}", {m: int(m == n) for m in names}) for n in names]
    return r


def on_routes(cuda, T, names, launch, single=True):
    """launch(place) -> a tuple of device tensors (or None), once per route; {label: CPU copies}.  No canary may change."""
    res = {}
    for label, shifts in routes(T, names, single):
        place = Placer(cuda, shifts)
        got = launch(place)
        torch.cuda.synchronize()
        assert place.intact(), label
        res[label] = tuple(None if t is None else t.cpu() for t in got)
    return res


def identical(res, fields=None):
    """Every route gives the bytes of the aligned one (in the listed fields), NaN where it has NaN."""
    first = res["aligned"]
    for label, got in res.items():
        for k, (a, b) in enumerate(zip(got, first)):
            if fields is None or k in fields:
                assert (a is None and b is None) or same(a, b), (label, k)


# ---- inputs that keep their ingredients at every length -----------------------------------------------------------------------

def gen(seed):
    return torch.Generator().manual_seed(seed)


def box(B, T, g, lo=0.0, span=1.0):
    """Rows in [lo, lo + span] with exact 0s and 1s (sample 0 is a 0 at every length, sample 1 a 1 in rows too short for 5::19)."""
    x = lo + span * torch.rand(B, T, generator=g)
    x[:, ::17] = 0.0
    x[:, 5::19] = 1.0
    if 1 < T <= 5:
        x[:, 1] = 1.0
    if T == 1 and B > 1:
        x[1, 0] = 1.0
    return x


def faces(T, start=3, stride=11):
    """The samples put on the ball's face: start::stride, or sample 0 where the row is too short to reach `start`."""
    return list(range(start, T, stride)) or [0]


def gradient(B, T, g, scale, nan=True):
    """N(0, scale^2) with zeros (T > 1), one NaN at T - 1 of row 0 (T > 1), an all-zero row 1 and a tie row 2 (equal |g|)."""
    grad = torch.randn(B, T, generator=g) * scale
    if T > 1:
        grad[:, ::13] = 0.0
        if nan:
            grad[0, T - 1] = NAN
    if B > 1:
        grad[1] = 0.0
    if B > 2:
        grad[2] = scale * torch.sign(torch.randn(T, generator=g))
    return grad


def ball_rows(B, T, g, e):
    """(orig, adv): orig from box(), adv inside each row's L-inf ball of radius e (a float or a (B, 1) column), on its faces."""
    orig = box(B, T, g)
    adv = (orig + (torch.rand(B, T, generator=g) * 2 - 1) * e).clamp(0, 1)
    f = faces(T)
    adv[:, f] = (orig[:, f] + e).clamp(0, 1)
    f = faces(T, 4, 23)
    adv[:, f] = (orig[:, f] - e).clamp(0, 1)
    return orig, adv


def apgd_rows(B, T, seed, nan=True):
    """tests/test_gpu_apgd.py's waves() at any length: (x, cur, prev, grad) on the CPU, eps = 0.003."""
    g = gen(seed)
    x, cur = ball_rows(B, T, g, 0.003)
    prev = (x + (torch.rand(B, T, generator=g) * 2 - 1) * 0.003).clamp(0, 1)
    return x, cur, prev, gradient(B, T, g, 1e-3, nan)


# ---- apgd.hip ---------------------------------------------------------------------------------------------------------------------

@grid
@pytest.mark.parametrize("norm", ["Linf", "L2"])
def test_apgd_init(cuda, B, T, norm):
    ops, eps = hip(), 0.003
    x = apgd_rows(B, T, 1)[0]
    draw = torch.rand(B, T, generator=gen(2)) if norm == "Linf" else torch.randn(B, T, generator=gen(2))
    if B > 1:
        draw[0] = 0.5 if norm == "Linf" else 0.0                        # an all-zero t: 0 / 0 as in the reference
    res = on_routes(cuda, T, ("x", "draw", "out"),
                    lambda p: (ops.apgd_init(p("x", x), eps, norm, draw=p("draw", draw), out=p("out", x.shape)),))
    identical(res)
    got, want = res["aligned"][0], CA.apgd_init(x, eps, norm, draw=draw)
    if norm == "Linf":
        assert same(got, want) and (B == 1 or torch.isnan(got[0]).all())
    else:
        assert same(torch.isnan(got), torch.isnan(want)) and not torch.isnan(got).any()
        torch.testing.assert_close(got, want, atol=L2_ATOL, rtol=0)
    res = on_routes(cuda, T, ("x", "out"),
                    lambda p: (ops.apgd_init(p("x", x), eps, norm, seed=1234, offset=3, out=p("out", x.shape)),))
    identical(res)
    got, want = res["aligned"][0], CA.apgd_init(x, eps, norm, seed=1234, offset=3)
    if norm == "Linf":
        assert same(got, want)
    else:
        torch.testing.assert_close(got, want, atol=1e-6 * eps + L2_ATOL, rtol=0)    # the module's Philox allowance


TRACK = ("x_adv", "grad", "x_best", "grad_best", "x_best_adv")


@grid
def test_apgd_track(cuda, B, T):
    ops = hip()
    _, cur, _, grad = apgd_rows(B, T, 3)
    sentinels = (7.0, -7.0, 9.0)
    src = [cur, grad] + [torch.full((B, T), v) for v in sentinels]
    for f0 in range(8):                                                 # all eight flag values in every row position
        flags = torch.tensor([(f0 + r) % 8 for r in range(B)], dtype=torch.uint8)
        ref = [t.clone() for t in src]
        CA.apgd_track(*ref, flags)

        def launch(p):
            bufs = [p(n, t) for n, t in zip(TRACK, src)]
            ops.apgd_track(*bufs, flags.to(cuda))
            return bufs

        res = on_routes(cuda, T, TRACK, launch)
        identical(res)
        for a, b in zip(res["aligned"], ref):
            assert same(a, b), f0
        none = flags == 0
        for t, v in zip(res["aligned"][2:], sentinels):
            assert (t[none] == v).all()                                 # unflagged rows keep their bytes


STEP = ("cur", "prev", "grad", "x", "out")


def apgd_step_launch(fn, rows, step, eps, a, cuda, **kw):
    """launch(place, alias): the APGD step `fn` on the CPU rows (cur, prev, grad, x); alias: `out` is `prev` (ping-pong)."""
    def launch(p, alias=False):
        c, pv, g, x = (p(n, t) for n, t in zip(STEP, rows))
        res = fn(c, pv, g, x, step.to(cuda), eps, a, out=pv if alias else p("out", x.shape), **kw)
        return res if isinstance(res, tuple) else (res,)
    return launch


@grid
@pytest.mark.parametrize("a", [1.0, 0.75])
def test_apgd_linf_step(cuda, B, T, a):
    ops, eps = hip(), 0.003
    x, cur, prev, grad = apgd_rows(B, T, 4)
    step = torch.rand(B, generator=gen(5)) * 2 * eps
    want = CA.apgd_linf_step(cur, prev, grad, x, step, eps, a)
    launch = apgd_step_launch(ops.apgd_linf_step, (cur, prev, grad, x), step, eps, a, cuda)
    for res in (on_routes(cuda, T, STEP, launch), on_routes(cuda, T, STEP[:4], functools.partial(launch, alias=True))):
        identical(res)
        assert same(res["aligned"][0], want)                            # bit for bit, NaN where the table has NaN


@grid
@pytest.mark.parametrize("a", [1.0, 0.75])
def test_apgd_l2_step(cuda, B, T, a):
    ops, eps = hip(), 0.1
    ball = CR.l2_ball_bound(torch.tensor(eps, dtype=torch.float32).item(), T)      # see the module's docstring
    x, cur, prev, grad = apgd_rows(B, T, 6)
    step = torch.rand(B, generator=gen(7)) * 2 * eps
    want, wn = CA.apgd_l2_step(cur, prev, grad, x, step, eps, a, return_norms=True)
    launch = apgd_step_launch(ops.apgd_l2_step, (cur, prev, grad, x), step, eps, a, cuda, return_norms=True)
    res = on_routes(cuda, T, STEP, launch)
    identical(res)
    got, norms = res["aligned"]
    assert same(torch.isnan(got), torch.isnan(want))
    torch.testing.assert_close(got, want, atol=L2_ATOL, rtol=0, equal_nan=True)
    torch.testing.assert_close(norms, wn, rtol=1e-5, atol=0, equal_nan=True)
    d = (got - x).double()
    ok = torch.isfinite(d).all(dim=1)
    assert (d[ok].norm(dim=1) <= ball).all()
    ali = on_routes(cuda, T, STEP[:4], functools.partial(launch, alias=True))
    identical(ali)
    assert same(ali["aligned"][0], got) and same(ali["aligned"][1], norms)
    # against float64, without the NaN (with it row 0 is NaN from end to end, and B = 1 would compare nothing)
    x, cur, prev, grad = apgd_rows(B, T, 8, nan=False)
    launch = apgd_step_launch(ops.apgd_l2_step, (cur, prev, grad, x), step, eps, a, cuda)
    res = on_routes(cuda, T, STEP, launch, single=False)
    identical(res)
    got = res["aligned"][0].double()
    ref = l2_step_f64(cur, prev, grad, x, step, eps, a)
    cpu = CA.apgd_l2_step(cur, prev, grad, x, step, eps, a).double()
    assert torch.isfinite(ref).all() and torch.isfinite(got).all()
    err_dev, err_cpu = (got - ref).abs().max().item(), (cpu - ref).abs().max().item()
    print(f"L2 step ({B}, {T}) |device - f64| max {err_dev:.3e}, |cpu table - f64| max {err_cpu:.3e}")
    assert err_dev + err_cpu <= L2_ATOL
    # the ball, in float64
    size, size_cpu = (got - x.double()).norm(dim=1), (cpu - x.double()).norm(dim=1)
    print(f"        ||out - x||_2 / eps - 1: device {(size / eps - 1).max().item():.3e}, cpu table "
          f"{(size_cpu / eps - 1).max().item():.3e}, f64 {((ref - x.double()).norm(dim=1) / eps - 1).max().item():.3e}")
    assert (size <= ball).all()


# ---- apgdl1.hip ----------------------------------------------------------------------------------------------------------------

def l1_box(B, T, g):
    """tests/test_gpu_apgdl1.py's box_rows(): away from its exact 0s and 1s x >= 0.01, so x + (u - x) == u for a small u - x."""
    return box(B, T, g, 0.01, 0.98)


def l1_projection_inputs(B, T, seed, first_case=0):
    """test_gpu_apgdl1.projection_inputs at any length (the sparse step keeps at least one coordinate): (x, u, case per row),
    0 = x + N(0, 1); 1 = a 20 %-sparse sign step of size eps plus 3e-4 noise; 2 = a point of the box within 1e-4 N(0, 1) of x
    (phi(0) < eps: the projection is the identity); 3 = x +- 0.01 everywhere, the tie input."""
    g = gen(seed)
    x = l1_box(B, T, g)
    eps = eps_for(T)
    u = torch.empty(B, T)
    cases = [(first_case + r) % 4 for r in range(B)]
    for r, case in enumerate(cases):
        noise = torch.randn(T, generator=g)
        if case == 0:
            u[r] = x[r] + noise
        elif case == 1:
            sel = torch.rand(T, generator=g) < 0.2
            if not sel.any():
                sel[T // 2] = True
            step = torch.where(sel, torch.sign(torch.randn(T, generator=g)), torch.zeros(T)) * (eps / sel.sum())
            u[r] = x[r] + step + 3e-4 * noise
        elif case == 2:
            u[r] = (x[r] + 1e-4 * noise).clamp(0.0, 1.0)
        else:
            u[r] = x[r] + 0.01 * torch.sign(noise)
    return x, u, cases


def l1_step_inputs(B, T, seed):
    """test_gpu_apgdl1.step_inputs at any length: the NaN of row 0 sits at T - 1, which at T = 3, 4, 5 is the threshold rank
    of topk = 0.2 (thr = NaN, count = 0, a finite output); row 1 has no gradient, row 2 is the tie row with cur = x."""
    g = gen(seed)
    x = l1_box(B, T, g)
    eps = eps_for(T)
    cur = (x + torch.randn(B, T, generator=g) * (torch.rand(B, T, generator=g) < 0.1) * 1e-3).clamp(0.0, 1.0)
    grad = gradient(B, T, g, 1e-3)
    if B > 2:
        cur[2] = x[2]
    topk = torch.tensor([0.2, 0.0, 0.2])[:B].contiguous()
    step = (torch.tensor([1.0, 0.5, 2.0])[:B] * eps).contiguous()
    return x, cur, grad, step, topk, eps


def check_l1_rows(got, want, x, eps, allow=None):
    """The module's assertions on an output of the projection: the box, the table within L1_ATOL (+ allow), the L1 excess."""
    check_box(got)
    if allow is None:
        torch.testing.assert_close(got, want, atol=L1_ATOL, rtol=0)
    else:
        assert ((got - want).abs() <= allow).all(), (got - want).abs().max().item()
    assert l1_excess(got, x, eps) <= L1_SLACK, l1_excess(got, x, eps)


@grid
def test_l1_box_project(cuda, B, T):
    ops, eps = hip(), eps_for(T)
    for first_case in range(4):
        x, u, cases = l1_projection_inputs(B, T, 10 + first_case, first_case)
        want = CL.l1_box_project(x, u, eps)

        def launch(p, alias=False):
            xd, ud = p("x", x), p("u", u)
            return (ops.l1_box_project(xd, ud, eps, out=ud if alias else p("out", x.shape)),)

        res = on_routes(cuda, T, ("x", "u", "out"), launch)
        for label, (got,) in res.items():
            check_l1_rows(got, want, x, eps)
            for r, case in enumerate(cases):
                if case == 2:
                    assert same(got[r], u[r]), label                    # already feasible: untouched
        for label, (got,) in on_routes(cuda, T, ("x", "u"), functools.partial(launch, alias=True), single=False).items():
            assert same(got, res[label][0]), label                      # out aliasing u


@grid
def test_apgdl1_step(cuda, B, T):
    ops = hip()
    x, cur, grad, step, topk, eps = l1_step_inputs(B, T, 20)
    want, wstats = CL.apgdl1_step(cur, grad, x, step, topk, eps, return_stats=True)
    if T in (3, 4, 5):
        assert torch.isnan(wstats[0, 0]) and wstats[0, 1] == 0           # the NaN is the threshold: a condition on the inputs
    else:
        assert wstats[0, 1] > 0
    assert (B < 2 or wstats[1, 1] == 0) and (B < 3 or wstats[2, 1] == T)  # the zero row, the all-equal row

    def launch(p, alias=False):
        c, g, xd = p("cur", cur), p("grad", grad), p("x", x)
        return ops.apgdl1_step(c, g, xd, step.to(cuda), topk.to(cuda), eps, out=c if alias else p("out", x.shape),
                               return_stats=True)

    res = on_routes(cuda, T, ("cur", "grad", "x", "out"), launch)
    identical(res, fields=(1,))                                         # threshold and count: the same on every route
    for label, (got, stats) in res.items():
        assert same(stats, wstats), label                               # bit-exact, NaN threshold included
        check_l1_rows(got, want, x, eps)
        if B > 1:
            assert same(got[1], cur[1]), label                          # cnt = 0: the projection of cur, feasible already
    for label, (got, stats) in on_routes(cuda, T, ("cur", "grad", "x"), functools.partial(launch, alias=True),
                                         single=False).items():
        assert same(got, res[label][0]) and same(stats, wstats), label  # out aliasing cur: the attack's form


@grid
def test_apgdl1_init(cuda, B, T):
    ops, eps = hip(), eps_for(T)
    g = gen(30)
    x = l1_box(B, T, g)
    draw = torch.randn(B, T, generator=g)
    want = CL.apgdl1_init(x, eps, draw=draw)

    def launch(p, alias=False):
        xd, dd = p("x", x), p("draw", draw)
        return (ops.apgdl1_init(xd, eps, draw=dd, out=dd if alias else p("out", x.shape)),)

    res = on_routes(cuda, T, ("x", "draw", "out"), launch)
    for label, (got,) in res.items():
        check_l1_rows(got, want, x, eps)
    for label, (got,) in on_routes(cuda, T, ("x", "draw"), functools.partial(launch, alias=True), single=False).items():
        assert same(got, res[label][0]), label                          # out aliasing the draw
    # Philox: the module's allowance for libm against the device's transcendentals
    t = CL.philox_draw(B, T, "L2", 1234, 3)
    want = CL.apgdl1_init(x, eps, seed=1234, offset=3)
    allow = L1_ATOL + 1e-6 * (t.abs() + t.abs().max(dim=1, keepdim=True)[0])
    res = on_routes(cuda, T, ("x", "out"),
                    lambda p: (ops.apgdl1_init(p("x", x), eps, seed=1234, offset=3, out=p("out", x.shape)),))
    for label, (got,) in res.items():
        check_l1_rows(got, want, x, eps, allow)
    if T >= 255:                                                        # (a short row can project two draws onto one point)
        assert not same(ops.apgdl1_init(x.to(cuda), eps, seed=1234, offset=4).cpu(), res["aligned"][0])


@grid
def test_apgdl1_checkpoint(cuda, B, T):
    from audio_deepfake_adversarial_attacks_amd.torchattacks.attacks.apgdl1 import ApgdL1State
    ops, eps = hip(), eps_for(T)
    g = gen(40)
    x = l1_box(B, T, g)
    cur = torch.where(torch.rand(B, T, generator=g) < 0.3, torch.rand(B, T, generator=g), x)
    best = torch.where(torch.rand(B, T, generator=g) < 0.1, torch.rand(B, T, generator=g), x)
    if T > 1:
        cur[0, min(3, T - 1)] = NAN
    for variant in range(4):
        st = ApgdL1State.new(B, 4, eps, "cpu", T)
        st.flags.copy_((torch.arange(B) + 2 * variant) % 8)              # every flag combination
        sp = torch.where(((st.flags & 2) != 0)[:, None], cur, best).sub(x).ne(0).sum(dim=1).float()
        st.sp_old.copy_([sp / 0.94, sp / 0.96, sp, torch.full((B,), float(T))][variant])   # either side of 0.95
        st.step_size.copy_(torch.tensor([1.0, 0.12, 2.0, 0.5])[(torch.arange(B) + variant) % 4] * eps)
        before = {k: v.clone() for k, v in st.__dict__.items()}
        CL.apgdl1_checkpoint(cur, best, x, st, eps)
        assert same(st.sp_old, sp)
        if T >= 255:
            assert ((st.flags & 4) != 0).tolist() == [variant in (0, 3)] * B

        def launch(p):
            padded = {k: torch.cat([v, torch.full_like(v[:1], 7)]).to(cuda) for k, v in before.items() if v.dim() == 1}
            dev = type(st)(**{k: (padded[k][:-1] if k in padded else v.to(cuda)) for k, v in before.items()})
            ops.apgdl1_checkpoint(p("cur", cur), p("x_best", best), p("x", x), dev, eps)
            assert all(v[-1] == 7 for v in padded.values())              # the element after each (B) array: untouched
            return tuple(getattr(dev, k) for k in sorted(before))

        res = on_routes(cuda, T, ("cur", "x_best", "x"), launch)
        identical(res)
        for k, got in zip(sorted(before), res["aligned"]):
            assert same(got, getattr(st, k)), (variant, k)               # every field, bit for bit


def many_l1_rows(T, seed):
    """65 537 rows for the four l1-APGD kernels: x, the projection's u (by row: N(0, 1) away, feasible already, the tie input),
    the step's (cur, grad, step, topk).  The last two rows are the second trip of `row += gridDim.x`: there u = x + N(0, 1) and
    the step moves x = 0.5 by 2 eps over all T coordinates, so phi(0) > eps in both."""
    R = 65537
    g = gen(seed)
    x = l1_box(R, T, g)
    eps = eps_for(T)
    noise = torch.randn(R, T, generator=g)
    case = torch.arange(R) % 3
    case[R - 2:] = 0
    u = torch.where((case == 0)[:, None], x + noise,
                    torch.where((case == 1)[:, None], (x + 1e-4 * noise).clamp(0.0, 1.0), x + 0.01 * torch.sign(noise)))
    cur = (x + torch.randn(R, T, generator=g) * (torch.rand(R, T, generator=g) < 0.1) * 1e-3).clamp(0.0, 1.0)
    grad = torch.randn(R, T, generator=g) * 1e-3
    grad[:, 0] = 0.0
    grad[1::7] = 0.0
    topk = torch.tensor([0.2, 0.0, 1.0, 0.05])[torch.arange(R) % 4].contiguous()
    step = (torch.tensor([1.0, 0.5, 2.0, 0.1, 1.0])[torch.arange(R) % 5] * eps).contiguous()
    x[R - 2:], cur[R - 2:] = 0.5, 0.5
    u[R - 2:] = 0.5 + noise[R - 2:]
    grad[R - 2:] = 1e-3 * torch.sign(noise[R - 2:])
    topk[R - 2:], step[R - 2:] = 1.0, 2 * eps
    return x, u, cur, grad, step, topk, eps


def phi0(x, u):
    """phi(0) of the projection in float64: how far the rows of u are from x in L1 once clipped to the box."""
    d = u.double() - x.double()
    return torch.minimum(d.abs(), torch.where(d > 0, 1.0 - x.double(), x.double())).sum(dim=1)


@pytest.mark.parametrize("T", [4, 5])
def test_l1_rows_beyond_one_grid(cuda, T):
    """65 537 rows: the grid holds 65 535 workgroups, so the last two rows are the second trip of each kernel's
    `row += gridDim.x` loop (tests/test_gpu_fab.py::test_rows_beyond_one_grid for FAB).  T = 4 is the float4 path, T = 5 the
    scalar one.  Every output starts as NaN and must end without one."""
    from audio_deepfake_adversarial_attacks_amd.torchattacks.attacks.apgdl1 import ApgdL1State
    ops = hip()
    x, u, cur, grad, step, topk, eps = many_l1_rows(T, 60 + T)
    R = x.shape[0]
    ends = [0, 1, R - 3, R - 2, R - 1]
    xd = x.to(cuda)

    def check(got, want_ends, what, allow=None):
        got = got.cpu()
        assert not torch.isnan(got).any(), (what, torch.isnan(got).any(dim=1).nonzero().reshape(-1))
        check_l1_rows(got[ends], want_ends, x[ends], eps, allow)
        assert l1_excess(got, x, eps) <= L1_SLACK, (what, l1_excess(got, x, eps))   # every row
        check_box(got)

    def nan_rows():
        return torch.full((R, T), NAN, device=cuda)

    assert (phi0(x, u)[R - 2:] > eps).all()                              # the rows of the second trip do real work
    check(ops.l1_box_project(xd, u.to(cuda), eps, out=nan_rows()), CL.l1_box_project(x[ends], u[ends], eps), "project")

    want, wstats = CL.apgdl1_step(cur, grad, x, step, topk, eps, return_stats=True)
    u_step = cur + step[:, None] * torch.where(grad.abs() >= wstats[:, :1], torch.sign(grad), torch.zeros(())) \
        / (wstats[:, 1:] + 1e-10)
    assert (phi0(x, u_step)[R - 2:] > eps).all()
    got, stats = ops.apgdl1_step(cur.to(cuda), grad.to(cuda), xd, step.to(cuda), topk.to(cuda), eps, out=nan_rows(),
                                 return_stats=True)
    assert same(stats, wstats)                                           # every row's threshold and count
    check(got, want[ends], "step")

    draw = torch.randn(R, T, generator=gen(70 + T))
    assert (phi0(x, x + draw)[R - 2:] > eps).all()
    check(ops.apgdl1_init(xd, eps, draw=draw.to(cuda), out=nan_rows()), CL.apgdl1_init(x[ends], eps, draw=draw[ends]), "init")
    t = CL.philox_draw(R, T, "L2", 1234, 3)
    assert (phi0(x, x + t)[R - 2:] > eps).all()
    allow = (L1_ATOL + 1e-6 * (t.abs() + t.abs().max(dim=1, keepdim=True)[0]))[ends]
    check(ops.apgdl1_init(xd, eps, seed=1234, offset=3, out=nan_rows()), CL.project(x[ends], x[ends] + t[ends], eps),
          "init (Philox)", allow)

    best = torch.where(torch.rand(R, T, generator=gen(80 + T)) < 0.5, cur, x)
    st = ApgdL1State.new(R, 4, eps, "cpu", T)
    st.flags.copy_(torch.arange(R) % 8)
    st.flags[R - 2:] = torch.tensor([2, 5], dtype=torch.uint8)
    st.sp_old.copy_(torch.tensor([1.0, 2.0, 4.0, 5.0])[torch.arange(R) % 4])
    st.step_size.copy_(step)
    st.topk.fill_(NAN)                                                   # written by every row, read by none
    dev = type(st)(**{k: v.to(cuda) for k, v in st.__dict__.items()})
    ops.apgdl1_checkpoint(cur.to(cuda), best.to(cuda), xd, dev, eps)
    CL.apgdl1_checkpoint(cur, best, x, st, eps)
    assert same_state(dev, st)                                           # every field of every row, bit for bit
    assert not torch.isnan(dev.topk).any()


def test_row_count_limit_is_refused_at_the_entry_point(cuda):
    """The (tile, row) grid carries the row in 16 bits: the entry points of apgd.hip, momentum.hip and radius.hip document
    B <= 65 535.  One row more raises the wrapper's error, and nothing is written."""
    from audio_deepfake_adversarial_attacks_amd._lib import AdvstepError
    ops = hip()
    B, T = 65536, 1
    g = gen(90)
    rows = [torch.rand(B, T, generator=g).to(cuda) for _ in range(4)]
    per_row = torch.full((B,), 0.001, device=cuda)
    y = torch.zeros(B, dtype=torch.int64, device=cuda)
    flags = torch.full((B,), 7, dtype=torch.uint8, device=cuda)
    state = torch.rand(4, B, generator=g).to(cuda)

    def canary(shape=(B, T)):
        return Slot(shape, cuda, 0)

    def refused(call, *slots):
        with pytest.raises(AdvstepError):
            call()
        torch.cuda.synchronize()
        for s in slots:
            assert s.intact() and (s.t == CANARY).all()

    a, b, c, d = rows
    out = canary()
    refused(lambda: ops.apgd_init(a, 0.003, "Linf", draw=b, out=out.t), out)
    refused(lambda: ops.apgd_init(a, 0.003, "L2", seed=1, out=out.t), out)
    track = [canary() for _ in range(5)]
    refused(lambda: ops.apgd_track(*(s.t for s in track), flags), *track)
    refused(lambda: ops.apgd_linf_step(a, b, c, d, per_row, 0.003, 0.75, out=out.t), out)
    refused(lambda: ops.apgd_l2_step(a, b, c, d, per_row, 0.1, 0.75, out=out.t), out)
    m, nes = canary(), canary()
    refused(lambda: ops.mi_step(a, b, c, m.t, 0.0004, 0.003, 1.0, nes_out=nes.t, nes_scale=0.0004, out=out.t), out, m, nes)
    refused(lambda: ops.row_pgd_linf_step(a, b, c, per_row, 0.0004, 0.0, out=out.t), out)
    refused(lambda: ops.row_pgd_l2_step(a, b, c, per_row, 0.01, 0.0, out=out.t), out)
    new = canary((4, B))
    refused(lambda: ops.radius_round(a, per_row, y, True, state, out.t, out=new.t), out, new)
    # one row fewer is served (the canaries of the output stay, its rows do not)
    ok = Slot((B - 1, T), cuda, 0)
    ops.apgd_linf_step(a[:-1], b[:-1], c[:-1], d[:-1], per_row[:-1], 0.003, 0.75, out=ok.t)
    torch.cuda.synchronize()
    assert ok.intact() and (ok.t != CANARY).all()


# ---- momentum.hip ----------------------------------------------------------------------------------------------------------------

def mi_near64(adv, grad, orig, m, v, decay):
    """check_mi_launch's count of samples whose float64 momentum lies inside the rounding bound of zero, from the inputs."""
    B, T = adv.shape
    a = (grad if v is None else grad + v).double()
    mu = a.abs().sum(dim=1, keepdim=True) / T
    zero = mu == 0
    with np.errstate(all="ignore"):
        m64 = a / mu + m.double() * decay
    bound = (chain(T) + 3) * U * (a / mu).abs() + 2 * U * (m.double() * decay).abs()
    return int(((m64.abs() <= bound) & ~zero).sum())


def near_limit(B, T):
    return 0 if B * T < 10_000 else 1e-4 * B * T


def mi_rows(B, T, with_v, decay):
    """tests/test_gpu_momentum.py's mi_inputs at any length, from the first seed whose float64 momentum keeps clear of zero
    (a condition on the inputs alone: the float64 path does not depend on the kernel)."""
    for seed in itertools.count(1000 + B + T):
        g = gen(seed)
        orig, adv = ball_rows(B, T, g, 0.003)
        grad = gradient(B, T, g, 1.0, nan=False)
        m = torch.randn(B, T, generator=g)
        v = torch.randn(B, T, generator=g) * 0.5 if with_v else None
        if with_v and B > 1:
            v[1] = 0.0
        if mi_near64(adv, grad, orig, m, v, decay) <= near_limit(B, T):
            return adv, grad, orig, m, v, 0.003


@grid
@pytest.mark.parametrize("with_v,with_nes,alias,decay", [(False, False, False, 1.0), (True, True, True, 0.5),
                                                         (True, False, False, 1.0), (False, True, True, 1.0)])
def test_mi_step(cuda, B, T, with_v, with_nes, alias, decay):
    ops = hip()
    adv, grad, orig, m, v, eps = mi_rows(B, T, with_v, decay)
    alpha, nes_scale = 0.0004, decay * 0.0004
    names = ("adv", "grad", "orig", "momentum") + (() if alias else ("out",)) + (("v",) if with_v else ()) + \
        (("nes_out",) if with_nes else ())

    def launch(p):
        a, g, x, md = p("adv", adv), p("grad", grad), p("orig", orig), p("momentum", m)
        nes = p("nes_out", adv.shape, 9.125) if with_nes else None
        out, gmean = ops.mi_step(a, g, x, md, alpha, eps, decay, v=p("v", v) if with_v else None, nes_out=nes,
                                 nes_scale=nes_scale, out=a if alias else p("out", adv.shape), return_mean=True)
        return out, md, nes, gmean

    res = on_routes(cuda, T, names, launch)
    identical(res)
    out, m_out, nes, gmean = res["aligned"]
    near = check_mi_launch(adv, grad, orig, m, v, alpha, eps, decay, nes_scale, out, m_out, nes, gmean)
    assert near <= near_limit(B, T)


@grid
def test_variance_tuning_on_flat_lengths(cuda, B, T):
    """n = B * T samples as one flat row of the (tile, row) grid."""
    ops, n = hip(), B * T
    g = gen(n)
    adv = torch.rand(B, T, generator=g)
    bound = 0.005 * 1.5
    for o in (0, 20 * 7 + 3):
        res = on_routes(cuda, n, ("adv", "out"), lambda p: (ops.vt_neighbor(p("adv", adv), bound, seed=0x1234_5678_9ABC, offset=o,
                                                                            out=p("out", adv.shape)),))
        identical(res)
        got = res["aligned"][0]
        assert same(got, CM.vt_neighbor(adv, bound, seed=0x1234_5678_9ABC, offset=o))       # the Philox restatement
        assert ((got - adv).abs() <= bound).all()
    draw = (torch.rand(B, T, generator=g) * 2 - 1) * bound
    res = on_routes(cuda, n, ("adv", "draw", "out"),
                    lambda p: (ops.vt_neighbor(p("adv", adv), bound, draw=p("draw", draw), out=p("out", adv.shape)),))
    identical(res)
    assert same(res["aligned"][0], adv + draw) and same(res["aligned"][0], CM.vt_neighbor(adv, bound, draw=draw))
    g1, g2, ag = (torch.randn(B, T, generator=g) for _ in range(3))
    g1[0, :5] = -0.0
    for first in (True, False):
        start = torch.full((B, T), NAN) if first else g2
        want = start.clone()
        CM.vt_accumulate(want, g1, first)

        def launch(p):
            gv = p("gv", start)
            ops.vt_accumulate(gv, p("g", g1), first=first)
            return (gv,)

        res = on_routes(cuda, n, ("gv", "g"), launch)
        identical(res)
        assert same(res["aligned"][0], want) and same(want, (torch.zeros_like(g1) if first else g2) + g1)
    for N in (2, 20):
        res = on_routes(cuda, n, ("gv", "adv_grad", "out"),
                        lambda p: (ops.vt_variance(p("gv", g1), p("adv_grad", ag), N, out=p("out", g1.shape)),))
        identical(res)
        assert same(res["aligned"][0], CM.vt_variance(g1, ag, N))


# ---- radius.hip --------------------------------------------------------------------------------------------------------------------

def radius_rows(B, T, seed, nan=True, scale=1.0):
    """tests/test_gpu_minradius.py's step_inputs at any length: radii with 0 and 1e-7 within the batch of three."""
    g = gen(seed)
    e = torch.tensor([RADII[b % len(RADII)] for b in range(B)], dtype=torch.float32)
    orig, adv = ball_rows(B, T, g, e[:, None])
    return adv, gradient(B, T, g, 1.0, nan), orig, e * scale


ROWSTEP = ("adv", "grad", "orig", "out")


def row_step_launch(fn, rows, e, alpha_abs, alpha_rel, cuda, **kw):
    """launch(place, alias): the per-row step `fn` on the CPU rows (adv, grad, orig); alias: `out` is `adv`."""
    def launch(p, alias=False):
        a, g, x = (p(n, t) for n, t in zip(ROWSTEP, rows))
        res = fn(a, g, x, e.to(cuda), alpha_abs, alpha_rel, out=a if alias else p("out", x.shape), **kw)
        return res if isinstance(res, tuple) else (res,)
    return launch


@grid
@pytest.mark.parametrize("alpha_abs,alpha_rel,alias", [(0.0, 0.25, False), (0.0004, 0.0, True), (0.0002, 0.5, False)])
def test_row_pgd_linf_step(cuda, B, T, alpha_abs, alpha_rel, alias):
    ops = hip()
    adv, grad, orig, e = radius_rows(B, T, 2000 + B + T)
    want = CR.row_pgd_linf_step(adv, grad, orig, e, alpha_abs, alpha_rel)
    launch = row_step_launch(ops.row_pgd_linf_step, (adv, grad, orig), e, alpha_abs, alpha_rel, cuda)
    res = on_routes(cuda, T, ROWSTEP[:3] if alias else ROWSTEP, functools.partial(launch, alias=alias))
    identical(res)
    got = res["aligned"][0]
    assert same(got, want)                                              # bit for bit
    d = (got - orig).double().abs()
    ok = ~torch.isnan(d)
    assert (d[ok] <= (e[:, None].double() + 2.0 ** -24).expand_as(d)[ok]).all()
    if alpha_abs == 0.0:
        assert same(got[e == 0], orig[e == 0])                          # a radius-0 row is the clean row


@grid
def test_row_pgd_linf_step_equals_the_fixed_radius_kernel(cuda, B, T):
    ops = hip()
    adv, grad, orig, _ = radius_rows(B, T, 2100 + B + T)
    eps, alpha = 0.003, 0.0004
    adv = (orig + (adv - orig).clamp(-eps, eps)).clamp(0, 1)
    want = ops.pgd_linf_step(adv.to(cuda), grad.to(cuda), orig.to(cuda), alpha, eps).cpu()
    launch = row_step_launch(ops.row_pgd_linf_step, (adv, grad, orig), torch.full((B,), eps), alpha, 0.0, cuda)
    for label, (got,) in on_routes(cuda, T, ROWSTEP, launch, single=False).items():
        assert same(got, want), label


@grid
@pytest.mark.parametrize("alpha_abs,alpha_rel,alias", [(0.0, 0.25, False), (0.01, 0.0, True), (0.001, 0.5, False)])
def test_row_pgd_l2_step(cuda, B, T, alpha_abs, alpha_rel, alias):
    ops = hip()
    adv, grad, orig, e = radius_rows(B, T, 2200 + B + T, nan=False, scale=10)   # L2 radii: 0 .. 2.5
    launch = row_step_launch(ops.row_pgd_l2_step, (adv, grad, orig), e, alpha_abs, alpha_rel, cuda, return_norms=True)
    res = on_routes(cuda, T, ROWSTEP[:3] if alias else ROWSTEP, functools.partial(launch, alias=alias))
    identical(res)
    out, gn, dn = res["aligned"]
    check_l2_launch(adv, grad, orig, e, alpha_abs, alpha_rel, out, gn, dn)
    if B > 1:
        assert gn[1] == 0                                               # the all-zero gradient row
    plain = row_step_launch(ops.row_pgd_l2_step, (adv, grad, orig), e, alpha_abs, alpha_rel, cuda)
    for label, (got,) in on_routes(cuda, T, ROWSTEP, plain, single=False).items():
        assert same(got, out), label                                    # without the norm outputs: the same bytes


@grid
def test_row_pgd_l2_step_equals_the_fixed_radius_kernel(cuda, B, T, monkeypatch):
    monkeypatch.setenv("ADVSTEP_L2_SINGLE_PASS", "0")                   # the three-launch form
    ops = hip()
    adv, grad, orig, _ = radius_rows(B, T, 2300 + B + T, nan=False)
    eps, alpha = 0.1, 0.02
    want = [t.cpu() for t in ops.pgd_l2_step(adv.to(cuda), grad.to(cuda), orig.to(cuda), alpha, eps, return_norms=True)]
    launch = row_step_launch(ops.row_pgd_l2_step, (adv, grad, orig), torch.full((B,), eps), alpha, 0.0, cuda, return_norms=True)
    for label, got in on_routes(cuda, T, ROWSTEP, launch, single=False).items():
        for p, q in zip(got, want):
            assert same(p, q), label


@grid
@pytest.mark.parametrize("first", [True, False])
def test_radius_round(cuda, B, T, first):
    ops = hip()
    copied = []
    for k0 in range(0, 8, B):                                           # every kind of round_case's rows, B at a time
        state, z, y, adv = (t[..., k0:] if i < 3 else t[k0:] for i, t in enumerate(round_case(B + k0, T, seed=B * T + k0)))
        state, z, y = state.contiguous(), z.contiguous(), y.contiguous()
        copy, want_state = CR.round_decision(z, y, first, state)
        copied += copy.tolist()
        want_best = torch.full((B, T), -2.5)
        CR.radius_round(adv, z, y, first, state, want_best)

        def launch(p):
            best = p("best_adv", want_best.shape, -2.5)
            sbuf = torch.full((64 + 4 * B + 64,), 9.5, device=cuda)
            new = sbuf[64:64 + 4 * B].view(4, B)
            state_dev = state.to(cuda)
            got = ops.radius_round(p("adv", adv), z.to(cuda), y.to(cuda), first, state_dev, best, out=new)
            assert got.data_ptr() == new.data_ptr() and (sbuf[:64] == 9.5).all() and (sbuf[64 + 4 * B:] == 9.5).all()
            assert same(state_dev, state)                               # the launch only reads the old state
            return new, best

        res = on_routes(cuda, T, ("adv", "best_adv"), launch)
        identical(res)
        new, best = res["aligned"]
        assert same(new, want_state) and same(best, want_best)
        assert (best[~copy] == -2.5).all() and same(best[copy], adv[copy])   # only rows whose decision is "copy" change
    assert True in copied and False in copied


# ---- fab.hip ------------------------------------------------------------------------------------------------------------------------

NORMS = ("Linf", "L2", "L1")
OFFSETS = torch.tensor([1e-4, -1e-3, 0.05, -0.2, 0.45, 5.0])             # tests/helpers.py's fab_projection_inputs


def fab_points(R, T, g):
    t = torch.rand(R, T, generator=g)
    t[:, ::7] = 0.0
    t[:, 3::11] = 1.0
    if 1 < T <= 3:
        t[:, 1] = 1.0
    return t


def fab_normals(R, T, g, scale=0.01):
    w = torch.randn(R, T, generator=g) * scale
    if T > 1:
        w[:, ::13] = 0.0
    return w


def norm_of(d, norm):
    return OF.row_norm(d.double(), norm)


def check_projection(got, dn, want, t, w, b, norm):
    """tests/test_gpu_fab.py's assertions on one fab_projection launch (CPU tensors; w = the effective normals)."""
    want = torch.from_numpy(want)
    err = (got - want).abs().max().item()
    assert err <= TOL[norm], (norm, err)
    assert np.allclose(dn.numpy(), norm_of(want, norm).numpy(), rtol=1e-4, atol=TOL[norm])
    assert (got[w == 0] == 0).all()                                     # a zero normal never moves its coordinate
    assert ((t + got) >= -1e-6).all() and ((t + got) <= 1 + 1e-6).all()

    def resid(d):
        return ((w.double() * (t.double() + d.double())).sum(1) - b.double()).abs()
    scale = w.abs().sum(1).double()
    bound = 2e-5 * scale + TOL[norm] * w.abs().max().item()
    on = resid(want) <= 1e-6 * scale + 1e-9                             # rows whose hyperplane the box lets the oracle reach
    assert (resid(got)[on] <= bound[on]).all(), (norm, resid(got), bound)


@grid
@pytest.mark.parametrize("norm", NORMS)
def test_fab_hyperplane(cuda, B, T, norm):
    ops = hip()
    g = gen(4)
    gz = torch.randn(B, T, generator=g) * 1e-3
    x = torch.rand(B, T, generator=g)
    z = torch.tensor([2.5, 0.0, float("inf")])[:B].contiguous()
    la = torch.tensor([1, 0, 1])[:B].contiguous()
    want = O.fab_hyperplane(gz, x, z, la, norm)
    res = on_routes(cuda, T, ("gz", "x"), lambda p: ops.fab_hyperplane(p("gz", gz), p("x", x), z.to(cuda), la.to(cuda), norm))
    for label, got in res.items():
        for name, a, c in zip(("wscale", "b", "gnorm", "gdot"), got, want):
            a, c = a.numpy(), c.numpy()
            if name == "wscale":
                assert np.array_equal(a, c), (label, name)
            else:
                fin = np.isfinite(c)
                assert np.allclose(a[fin], c[fin], rtol=2e-5, atol=2e-5), (label, name, a, c)
                assert np.array_equal(np.isfinite(a), fin), (label, name)
    gzd, xd = gz.to(cuda), x.to(cuda)
    _, _, gn, gd = ops.fab_hyperplane(gzd, xd, None, None, norm)        # statistics only
    assert same(gn, res["aligned"][2]) and same(gd, res["aligned"][3])


@grid
@pytest.mark.parametrize("norm", NORMS)
def test_fab_projection(cuda, B, T, norm):
    ops = hip()
    for k0 in range(0, 6, B):                                           # every hyperplane offset, B at a time
        g = gen(100 + T + k0)
        t, w = fab_points(B, T, g), fab_normals(B, T, g)
        b = (w * t).sum(1) + OFFSETS[(torch.arange(B) + k0) % 6] * w.abs().sum(1)
        want = OF.PROJECTIONS[norm](t.numpy(), w.numpy(), b.numpy())
        res = on_routes(cuda, T, ("points", "w", "out"),
                        lambda p: ops.fab_projection(p("points", t), p("w", w), b.to(cuda), norm, out=p("out", t.shape)))
        for label, (d, dn) in res.items():
            check_projection(d, dn, want, t, w, b, norm)


@grid
@pytest.mark.parametrize("norm", NORMS)
def test_fab_projection_shared_normals_and_scale(cuda, B, T, norm):
    """R = 2 * B rows read w[r % B] * wscale[r % B]."""
    ops = hip()
    g = gen(3 + T)
    pts, gz = fab_points(2 * B, T, g), fab_normals(B, T, g, 0.02)
    wscale = torch.tensor([2.0, -2.0, 0.0])[:B].contiguous()
    w_full = (gz * wscale[:, None]).repeat(2, 1)
    b = (w_full * pts).sum(1) + torch.tensor([0.05, -0.2, 0.3, -1e-3, 0.45, 0.1])[:2 * B] * w_full.abs().sum(1)
    want = OF.PROJECTIONS[norm](pts.numpy(), w_full.numpy(), b.numpy())
    res = on_routes(cuda, T, ("points", "w", "out"),
                    lambda p: ops.fab_projection(p("points", pts), p("w", gz), b.to(cuda), norm, wscale.to(cuda),
                                                 out=p("out", pts.shape)))
    for label, (d, dn) in res.items():
        check_projection(d, dn, want, pts, w_full, b, norm)
        if B > 2:
            assert (d[[2, 5]] == 0).all() and (dn[[2, 5]] == 0).all()   # zero normal: no move


@pytest.mark.parametrize("T", [4, 1024, 4096, 4100])
def test_fab_l1_tie_rows(cuda, T):
    """w = +-0.03 everywhere: L1's tie group is the whole row, walked in index order by contiguous chunks, another sample ->
    thread map than the pass before it.  Row 0 crosses the hyperplane half way along the row, row 1 inside its last sample.
    With equal |w| the optimum is not unique coordinate-wise: the size of the move and the hyperplane residual are compared."""
    ops = hip()
    g = gen(9 + T)
    t = torch.rand(2, T, generator=g)
    w = torch.sign(torch.randn(2, T, generator=g)) * 0.03
    t[1, -1] = 0.9 if w[1, -1] > 0 else 0.1                             # the last sample has room 0.9, and uses 0.81 of it
    gain = (w.abs() * torch.where(w > 0, t, 1 - t)).double()            # the residual a full move of each coordinate takes off
    cum = gain.cumsum(1)
    c = torch.stack([0.5 * cum[0, -1], cum[1, -1] - 0.1 * gain[1, -1]])
    b = ((w.double() * t.double()).sum(1) - c).float()                  # the point lies on the positive side, c away
    want = torch.from_numpy(OF.projection_l1(t.numpy(), w.numpy(), b.numpy()))
    assert want[1, -1] != 0 and (want[0, -1] == 0 or T == 4)            # where each row crosses: a condition on the inputs
    res = on_routes(cuda, T, ("points", "w", "out"),
                    lambda p: ops.fab_projection(p("points", t), p("w", w), b.to(cuda), "L1", out=p("out", t.shape)))
    for label, (d, dn) in res.items():
        assert np.allclose(d.abs().sum(1).numpy(), want.abs().sum(1).numpy(), rtol=1e-4, atol=1e-4), label
        assert np.allclose(dn.numpy(), d.double().abs().sum(1).numpy(), rtol=1e-5, atol=0), label
        resid = ((w.double() * (t.double() + d.double())).sum(1) - b.double()).abs()
        assert (resid <= 2e-5 * w.abs().sum(1).double() + TOL["L1"] * 0.03).all(), (label, resid)
        assert ((t + d) >= -1e-6).all() and ((t + d) <= 1 + 1e-6).all()


@grid
def test_fab_combine(cuda, B, T):
    ops = hip()
    g = gen(6)
    x1, x0 = torch.rand(B, T, generator=g), torch.rand(B, T, generator=g)
    d1, d2 = torch.randn(B, T, generator=g) * 0.1, torch.randn(B, T, generator=g) * 0.1
    n1, n2 = torch.tensor([0.3, 0.0, 1e-9])[:B].contiguous(), torch.tensor([0.1, 0.0, 2.0])[:B].contiguous()
    names = ("x1", "x0", "d1", "d2", "out")
    for eta, amax in ((1.05, 0.1), (10.0, 0.1), (20.0, 0.5)):
        want = O.fab_combine(x1, x0, d1, d2, n1, n2, eta, amax)

        def launch(p, alias=False):
            a = p("x1", x1)
            return (ops.fab_combine(a, p("x0", x0), p("d1", d1), p("d2", d2), n1.to(cuda), n2.to(cuda), eta, amax,
                                    out=a if alias else p("out", x1.shape)),)

        for res in (on_routes(cuda, T, names, launch), on_routes(cuda, T, names[:4], functools.partial(launch, alias=True))):
            identical(res)
            assert torch.equal(res["aligned"][0], want)


@grid
@pytest.mark.parametrize("norm", NORMS)
def test_fab_backward_step(cuda, B, T, norm):
    ops = hip()
    g = gen(8)
    x0 = torch.rand(B, T, generator=g)
    x1 = (x0 + torch.randn(B, T, generator=g) * 0.01).clamp(0, 1)
    adv = torch.rand(B, T, generator=g)
    big = float(OF.row_norm(x1 - x0, norm).max()) * 2
    for k0 in range(0, 6, B):                                           # every (best so far, flag) pair, B at a time
        idx = (torch.arange(B) + k0) % 6
        res2 = torch.tensor([1e10, 1e-6, big, 1e10, 1e-6, big])[idx].contiguous()
        flags = torch.tensor([1, 1, 1, 0, 0, 1], dtype=torch.uint8)[idx].contiguous()
        c1, ca, cr = x1.clone(), adv.clone(), res2.clone()
        O.fab_backward_step(c1, x0, ca, cr, flags, 0.9, norm)

        def launch(p):
            g1, ga, gr = p("x1", x1), p("adv", adv), res2.to(cuda)
            ops.fab_backward_step(g1, p("x0", x0), ga, gr, flags.to(cuda).bool(), 0.9, norm)
            return g1, ga, gr

        res = on_routes(cuda, T, ("x1", "x0", "adv"), launch)
        identical(res, fields=(0, 1))
        for label, (g1, ga, gr) in res.items():
            assert torch.equal(g1, c1) and torch.equal(ga, ca), label
            assert torch.allclose(gr, cr, rtol=1e-5), label
            off = flags == 0
            assert torch.equal(g1[off], x1[off]) and torch.equal(ga[off], adv[off])   # rows that were not adversarial
