"""`-m gpu`: the row kernels of fmn.hip, l0.hip and multiattack.hip at the seams of their geometries and load routes, with the
harness and the lengths of tests/test_gpu_row_edges.py (its docstring has the routes and the canaries) and the inputs of
tests/test_row_edges_late_host.py, which asserts on the CPU what these inputs must hold at every length.

LENGTHS, by geometry.
    row_tiles.h (fmn.hip, multiattack.hip's copy: 256 threads, four quad rows of 256 quads per 4096-sample tile)
        1, 3            less than one quad: the sample route only, out-of-row lanes of the first quad filled
        4, 5            the first whole quad, and one sample into the second
        255, 256        the quad row's 64th quad short by one sample and whole
        1023 .. 1025    the end of the tile's first quad row (j = 0) and the first sample of its second
        4092, 4095      the tile's last quad missing, its last sample missing
        4096            the tile exactly full: one partial per row, nothing out of row
        4097, 4100      one sample and one quad into a second tile: C = 2, the second partial sums one thread's samples
        8196            two full tiles and one quad: C = 3
    row_workgroup.h (l0.hip: 1024 threads, trips of 1024 samples or 1024 quads)
        1023 .. 1025    the sample route's trip one short, full, and one sample into a second trip
        4092 .. 4100    the float4 route's trip one quad short, full (visit_rows_ahead's prefetch not taken) and one quad past
                        it (taken by thread 0 only); 4095 and 4097: the sample route's fourth trip short, fifth begun
        8196            the prefetch taken twice by thread 0
      and the index-cut search of l0.hip over 32 - clz(T - 1) bits, three per digit: 2 bits (T = 3, 4: less than one digit),
      3 (5: one digit), 8 (255, 256: 2 + a two-bit digit), 10 (1023, 1024: 3 + one bit), 11 (1025: 3 + two bits), 12 (4092 ..
      4096: four whole digits), 13 (4097, 4100: 4 + one bit), 14 (8196: 4 + two bits).

What is bit-identical across the routes.  fmn.hip and multiattack.hip: everything (row_tiles.h's sample route loads the same
quad into the same thread, the reductions have a fixed order).  fmn_step is launched on partials that an ALIGNED fmn_norms
left, so a route that shifts only best_adv or only out runs a float4 norms launch and a sample-route step over the same
partials.  l0.hip: the projection (no reduced quantity).  The step's gnorm is summed in another order on the sample route and
the threshold depends on it through u, so the step is NOT asked to be identical across routes: on every route it equals the
table bit for bit under that route's own gnorm, which is held to its derived bound.

No tolerance is new: the FMN row sums are held to fmn_cpu_ops.sum_rel_bound / norm_rel_bound, L0's gnorm to
test_gpu_l0.gnorm_bound, both derived from the summation order at any T (chain(T) = 24 + ceil(C / 256) is an upper bound of
the longest chain of a short row as well: a thread adds its 4 x 4 samples, the wave butterfly adds 6 times, the four waves 3
times, the row's C <= 3 partials once more).  Everything else is bit for bit.

What a slip at a seam would change, reasoned from the code.
    load4<true>'s bound q < (T >> 2) read as <=: the float4 route loads the quad after the row (the next row's first quad, or
        the canary after the last row) wherever that quad falls into a launched tile, T = 4, 256, 1024, 4092, 4100, 8196.
        test_fmn_norms then sums four foreign samples on the float4 route only: the partials differ between the aligned and
        the shifted route, and at B = 1 sum g^2 gains 4 x 7.25^2 against float64.  (The stores keep their own bound.)
    multi_select_kernel without its i < n guard: the lanes past n of the last ballot judge whatever follows z, labels and
        rows, so wrong + kept is a multiple of 64: counts != [n - k, k] at n = 1, 5, 63, 65, 129.
    fmn.hip's rows_vec list of the moving forms without best_adv: the routes "only best_adv" (T = 4, 4096, 4100) store
        float4 through a base one float past a 16-byte boundary.  The comparisons see that only if the device does not
        serve such a store byte for byte; they cannot tell a device that does from the right route.
    visit_rows_ahead's prefetch guard e + kRow < n read as <=: at T = 4096 (float4) and 1024 (samples) thread 0 loads the
        element after the row and never uses it.  No value changes; only a row that ends with its allocation could show it,
        and no test here builds one.

Findings.  None: no comparison below failed on gfx950 at any (T, route), so no kernel or route decision was changed."""
import functools

import pytest
import torch

from tests import fmn_cpu_ops as CF
from tests import l0_cpu_ops as CL0
from tests import multiattack_cpu_ops as CMA
from tests.test_gpu_apgd import hip, same
from tests.test_gpu_fmn import step_case
from tests.test_gpu_l0 import ALPHA, check_ball, gnorm_bound
from tests.test_gpu_multiattack import padded, same_bits, untouched
from tests.test_gpu_row_edges import CANARY, LENGTHS, NAN, Slot, gen, identical, on_routes, routes
from tests.test_row_edges_late_host import (FMN_ALPHA, FMN_BATCHES, FMN_FILL, FMN_GAMMA, L0_BATCHES, MULTI_ROUTE_N,
                                            MULTI_SELECT_N, MULTI_SELECT_T, fmn_rows, l0_cases, l0_projection_rows,
                                            l0_step_rows, multi_rows)

pytestmark = pytest.mark.gpu


def grid(batches):
    return lambda fn: pytest.mark.parametrize("B", batches)(pytest.mark.parametrize("T", LENGTHS)(fn))


def extra(place, shape, cuda, fill):
    """A canary-framed aligned output that no route shifts (a workspace, a state), watched by on_routes like a placed one."""
    place.slots.append(Slot(shape, cuda, 0, fill))
    return place.slots[-1].t


# ---- fmn.hip ------------------------------------------------------------------------------------------------------------------------

@grid(FMN_BATCHES)
def test_fmn_norms(cuda, B, T):
    """rows_vec(T, {adv, grad, orig}).  Across the routes the per-tile partials and the row norms re-reduced from them are
    identical; max |d| is the twin's bit for bit; the three sums lie within the derived bound of float64."""
    ops = hip()
    adv, grad, orig = fmn_rows(B, T)
    need = ops.fmn_workspace(B, T, cuda).numel()
    ones, y1 = torch.ones(B, device=cuda), torch.ones(B, dtype=torch.int64, device=cuda)   # no row adversarial: no copy

    def launch(p):
        a, g, x = p("adv", adv), p("grad", grad), p("orig", orig)
        ws = extra(p, (need,), cuda, -3.25)
        assert ops.fmn_norms(a, g, x, ws=ws).data_ptr() == ws.data_ptr()
        parts = ops.fmn_partials(ws, B, T).clone()
        rn = torch.full((5, B), -9.5, device=cuda)
        best = torch.full((B, T), FMN_FILL, device=cuda)
        _, out = ops.fmn_step(a, None, x, ones, y1, ops.fmn_begin(B=B, device=cuda), best, ws, 0.0, FMN_GAMMA, "Linf",
                              move=False, row_norms=rn)                 # move = False: nothing but the re-reduction runs
        assert out is None and (best == FMN_FILL).all() and (rn[4] == -9.5).all()
        ws0 = extra(p, (need,), cuda, -3.25)
        ops.fmn_norms(a, None, x, ws=ws0)                               # without a gradient
        return parts, rn[:4], ops.fmn_partials(ws0, B, T).clone()

    res = on_routes(cuda, T, ("adv", "grad", "orig"), launch)
    assert len(res) == len(routes(T, ("adv", "grad", "orig")))
    identical(res)
    parts, rn, parts0 = res["aligned"]
    assert parts.shape == (4, B, CF.tiles(T)) and same(parts[1], CF.tile_partials(adv, grad, orig)[1])
    want = CF.row_norms64(adv, grad, orig)
    got = rn.double()
    assert same(rn[1], want[1].float())                                 # max |d|: bit for bit
    rows = torch.arange(B) % 8
    assert torch.isnan(got[2:, rows == 6]).all() and not torch.isnan(got[2:, rows != 6]).any()
    assert not torch.isnan(got[:2]).any()                               # the NaN stays in its row and in the g planes
    for plane, squares in ((0, True), (2, True), (3, False)):
        ok = ~torch.isnan(want[plane])
        err, bound = (got[plane] - want[plane]).abs()[ok], CF.sum_rel_bound(T, squares) * want[plane][ok]
        print(f"  {CF.FMN_NORMS[plane]} ({B}, {T}): max err / bound = {(err / bound.clamp_min(1e-300)).max().item():.3f}")
        assert (err <= bound).all()
    assert (got[2:, rows == 1] == 0).all() and (got[:2, rows == 5] == 0).all()          # zero rows: exact 0
    assert same(parts0[:2], parts[:2]) and (parts0[2:] == 0).all()


@grid(FMN_BATCHES)
@pytest.mark.parametrize("norm", ["Linf", "L2"])
@pytest.mark.parametrize("move", [True, False])
def test_fmn_step(cuda, B, T, norm, move):
    """rows_vec(T, {adv, grad, orig, best_adv, out}) for the moving forms, rows_vec(T, {adv, best_adv}) for move = False,
    over partials of an aligned norms launch.  state_out, best_adv, out and row_norms are identical across the routes and
    equal the twin under the kernel's own row norms bit for bit."""
    ops = hip()
    adv, grad, orig = fmn_rows(B, T)
    state, z, y, want_copy = step_case(adv, orig, norm)
    copy, rows = torch.tensor(want_copy), torch.arange(B) % 8
    dev = lambda t: t.to(cuda)                                          # noqa: E731
    names = ("adv", "grad", "orig", "best_adv", "out") if move else ("adv", "best_adv")

    def launch(p, alias=False):
        ws = ops.fmn_norms(dev(adv), dev(grad), dev(orig))              # aligned, whatever the step's route
        a = p("adv", adv)
        g, x = (p("grad", grad), p("orig", orig)) if move else (None, dev(orig))
        best = p("best_adv", adv.shape, FMN_FILL)
        out = (a if alias else p("out", adv.shape)) if move else None
        new = extra(p, (4, B), cuda, 9.5)
        rn = torch.full((5, B), NAN, device=cuda)
        state_dev = dev(state)
        got_state, got_out = ops.fmn_step(a, g, x, dev(z), dev(y), state_dev, best, ws, FMN_ALPHA, FMN_GAMMA, norm, move=move,
                                          state_out=new, out=out, row_norms=rn)
        assert got_state.data_ptr() == new.data_ptr() and same(state_dev, state)   # the launch only reads the old state
        assert (got_out is None) if not move else (got_out.data_ptr() == out.data_ptr())
        return new, best, got_out, rn

    res = on_routes(cuda, T, names, launch)
    assert len(res) == len(routes(T, names))
    identical(res)
    new, best, out, rn = res["aligned"]
    want_best = torch.full((B, T), FMN_FILL)
    want_state, want_out = CF.fmn_step(adv, grad, orig, z, y, state, want_best, None, FMN_ALPHA, FMN_GAMMA, norm, move=move,
                                       given_norms=rn)
    assert same(new, want_state) and same(best, want_best)
    assert (best[~copy] == FMN_FILL).all() and same(best[copy], adv[copy])   # unimproved rows keep their fill
    assert not torch.isnan(new[:, rows != 6]).any()
    assert (new[0, rows == 5] == 0).all() and (new[1, rows == 5] == 0).all() and torch.isinf(new[0, rows == 1]).all()
    n64 = CF.row_norms64(adv, grad, orig)
    dn64 = n64[0].sqrt() if norm == "L2" else n64[1]
    assert ((new[3].double() - dn64).abs() <= CF.norm_rel_bound(T) * dn64).all()         # dnorm is the row's norm
    if not move:
        return
    assert same(out, want_out)
    assert same(out[rows == 5], orig[rows == 5])                        # eps' = 0: the clean row
    assert torch.isnan(out[rows == 6]).all() and not torch.isnan(out[rows != 6]).any()   # the NaN row stays NaN, and alone
    ali = on_routes(cuda, T, names[:4], functools.partial(launch, alias=True))           # out = adv
    identical(ali)
    for a, b in zip(ali["aligned"], res["aligned"]):
        assert same(a, b)
    st0, _ = ops.fmn_step(dev(adv), None, dev(orig), dev(z), dev(y), dev(state), torch.empty(B, T, device=cuda),
                          ops.fmn_norms(dev(adv), dev(grad), dev(orig)), 0.0, FMN_GAMMA, norm, move=False)
    assert same(st0, new)                                               # the move = False decision is the moving form's


# ---- l0.hip -------------------------------------------------------------------------------------------------------------------------

@grid(L0_BATCHES)
def test_l0_box_project(cuda, B, T):
    """rows_vec(T, {x, u, out}): identical across the routes and the table's bit for bit, also with out = u."""
    ops = hip()
    x, u = l0_projection_rows(B, T)
    for k, eps_inf in l0_cases(T):
        def launch(p, alias=False):
            xd, ud = p("x", x), p("u", u)
            return (ops.l0_box_project(xd, ud, k, eps_inf, out=ud if alias else p("out", x.shape)),)

        res = on_routes(cuda, T, ("x", "u", "out"), launch)
        identical(res)
        got = res["aligned"][0]
        assert same(got, CL0.l0_box_project(x, u, k, eps_inf)), (k, eps_inf)
        check_ball(got, x, k, eps_inf)
        for label, (a,) in on_routes(cuda, T, ("x", "u"), functools.partial(launch, alias=True)).items():
            assert same(a, got), (k, eps_inf, label)
        if B > 2 and k < T:                                             # the tie row: more equal scores than places (host test)
            assert (got[2] != x[2]).sum() == k


STEP = ("cur", "grad", "x", "out")


@grid(L0_BATCHES)
def test_pgdl0_step(cuda, B, T):
    """rows_vec(T, {cur, grad, x, out}).  On every route separately: gnorm within its derived bound, output and the four stats
    the table's under that gnorm bit for bit, out = cur the same bytes."""
    ops, step = hip(), ALPHA * T
    for k, eps_inf in l0_cases(T):
        x, cur, grad = l0_step_rows(B, T, k)

        def launch(p, alias=False):
            c, g, xd = p("cur", cur), p("grad", grad), p("x", x)
            return ops.pgdl0_step(c, g, xd, step, k, eps_inf, out=c if alias else p("out", x.shape), return_stats=True)

        res = on_routes(cuda, T, STEP, launch)
        ali = on_routes(cuda, T, STEP[:3], functools.partial(launch, alias=True))
        assert len(res) == len(routes(T, STEP))
        for label, (got, stats) in res.items():
            where = (k, eps_inf, label)
            assert ((stats[:, 0].double() - grad.double().abs().sum(dim=1)).abs() <= gnorm_bound(grad)).all(), where
            want, wstats = CL0.pgdl0_step(cur, grad, x, step, k, eps_inf, return_stats=True, gnorm=stats[:, 0])
            assert same(stats, wstats), (where, stats, wstats)          # gnorm, threshold, count above, last kept tie
            assert same(got, want), where
            check_ball(got, x, k, eps_inf)
            if B > 1:
                assert stats[1, 0] == 0 and same(got[1], cur[1]), where  # the zero-gradient row: cur itself
            if label in ali:
                assert same(ali[label][0], got) and same(ali[label][1], stats), where


@grid(L0_BATCHES)
def test_pgdl0_step_nan_gradient(cuda, B, T):
    """A NaN in grad[0]: the launch terminates, every in-row sample is written and no other row sees it."""
    ops, step, k = hip(), ALPHA * T, min(16, T)
    x, cur, grad = l0_step_rows(B, T, k)
    bad = grad.clone()
    bad[0, min(7, T - 1)] = NAN

    def launch(p):
        c, xd = p("cur", cur), p("x", x)
        clean = ops.pgdl0_step(c, p("grad", grad), xd, step, k, out=p("out", x.shape))
        got, stats = ops.pgdl0_step(c, p("grad", bad), xd, step, k, out=p("out", x.shape), return_stats=True)
        return clean, got, stats

    for label, (clean, got, stats) in on_routes(cuda, T, STEP, launch, single=False).items():   # synchronised: it terminated
        assert not (got == CANARY).any() and not (clean == CANARY).any(), label
        assert torch.isnan(stats[0, 0]) and same(got[1:], clean[1:]), label


# ---- multiattack.hip ----------------------------------------------------------------------------------------------------------------

ROUTE = ("adv", "x", "final", "next_x")


def multi_launch_and_check(cuda, n, T, pattern, names=ROUTE):
    """One multi_route launch per route of `names`, every output between canaries, against the restatement bit for bit."""
    ops = hip()
    adv, x, z, labels, rows, wrong, B = multi_rows(n, T, pattern)
    final0 = torch.rand(B, T, generator=gen(n + T))
    k = int((~wrong).sum())
    w_final, w_x = final0.clone(), torch.full((n, T), 9.125)
    w_y, w_rows = torch.full((n,), -5, dtype=torch.int64), torch.full((n,), -6, dtype=torch.int32)
    *_, w_counts = CMA.multi_route(adv, x, z, labels, rows, w_final, next_x=w_x, next_y=w_y, next_rows=w_rows)
    assert w_counts.tolist() == [n - k, k]

    def launch(p):
        final, next_x = p("final", final0), p("next_x", (n, T), 9.125)
        ybuf, next_y = padded((n,), -5, torch.int64, cuda)
        rbuf, next_rows = padded((n,), -6, torch.int32, cuda)
        out = ops.multi_route(p("adv", adv), p("x", x), z.to(cuda), labels.to(cuda), rows.to(cuda), final, next_x=next_x,
                              next_y=next_y, next_rows=next_rows)
        torch.cuda.synchronize()
        assert untouched(ybuf, -5, n) and untouched(rbuf, -6, n)
        return final, next_x, next_y, next_rows, out[3]

    res = on_routes(cuda, T, names, launch)
    for label, (final, next_x, next_y, next_rows, counts) in res.items():
        assert counts.dtype == torch.int32 and counts.tolist() == [n - k, k], label
        assert torch.equal(next_y, w_y) and torch.equal(next_rows, w_rows), label
        assert same_bits(final, w_final) and same_bits(next_x, w_x), label
        named = torch.zeros(B, dtype=torch.bool)
        named[rows[wrong].long()] = True
        assert same_bits(final[~named], final0[~named]) and same_bits(final[named], adv[wrong]), label
        assert (next_x[k:] == 9.125).all() and (next_y[k:] == -5).all() and (next_rows[k:] == -6).all(), label
    return res


@pytest.mark.parametrize("T", LENGTHS)
@pytest.mark.parametrize("n,pattern", [(n, p) for n in MULTI_ROUTE_N for p in (("alternating", "random") if n > 1
                                                                               else ("alternating",))])
def test_multi_route(cuda, n, T, pattern):
    """rows_vec(T, {adv, x, final, next_x}): aligned, all four shifted and, at T = 4, 4096 and 4100, each one alone."""
    res = multi_launch_and_check(cuda, n, T, pattern)
    assert len(res) == len(routes(T, ROUTE))


@pytest.mark.parametrize("pattern", ["alternating", "random"])
@pytest.mark.parametrize("n", MULTI_SELECT_N)
def test_multi_select_wave_seam(cuda, n, pattern):
    """The one-wave select kernel either side of one and of two 64-lane ballots: counts, next_y and next_rows exactly (the
    lanes past n of the last ballot judge nothing and write nothing)."""
    multi_launch_and_check(cuda, n, MULTI_SELECT_T, pattern)


# ---- the row-count limit ------------------------------------------------------------------------------------------------------------

def test_row_count_limit_is_refused_at_the_late_entry_points(cuda):
    """tests/test_gpu_row_edges.py::test_row_count_limit_is_refused_at_the_entry_point for the entry points of fmn.hip,
    multiattack.hip, smooth.hip and smoothadv.hip that document B <= 65 535: one row more raises the wrapper's error and
    nothing is written; 65 535 rows are served."""
    from audio_deepfake_adversarial_attacks_amd._lib import AdvstepError
    ops = hip()
    B, T = 65536, 1
    g = gen(91)
    a, b, c = (torch.rand(B, T, generator=g).to(cuda) for _ in range(3))
    z = torch.randn(B, generator=g).to(cuda)
    y = torch.zeros(B, dtype=torch.int64, device=cuda)

    def canary(shape=(B, T)):
        return Slot(shape, cuda, 0)

    def refused(call, *slots):
        with pytest.raises(AdvstepError):
            call()
        torch.cuda.synchronize()
        for s in slots:
            assert s.intact() and (s.t == CANARY).all()

    state = canary((4, B))
    refused(lambda: ops.fmn_begin(state.t), state)
    ws = canary((ops.fmn_workspace(B, T, cuda).numel(),))
    refused(lambda: ops.fmn_norms(a, b, c, ws=ws.t), ws)
    old = torch.rand(4, B, generator=g).to(cuda)
    best, out, rn = canary(), canary(), canary((5, B))
    for norm in ("Linf", "L2"):
        refused(lambda: ops.fmn_step(a, b, c, z, y, old, best.t, ws.t, 0.37, 0.05, norm, state_out=state.t, out=out.t,
                                     row_norms=rn.t), state, best, out, rn, ws)
    refused(lambda: ops.fmn_step(a, None, c, z, y, old, best.t, ws.t, 0.0, 0.05, "Linf", move=False, state_out=state.t),
            state, best, ws)
    rows = torch.arange(B, dtype=torch.int32, device=cuda)
    final, next_x = canary(), canary()
    ybuf, next_y = padded((B,), -5, torch.int64, cuda)
    rbuf, next_rows = padded((B,), -6, torch.int32, cuda)
    refused(lambda: ops.multi_route(a, b, z, y, rows, final.t, next_x=next_x.t, next_y=next_y, next_rows=next_rows),
            final, next_x)
    assert untouched(ybuf, -5, B) and untouched(rbuf, -6, B) and (next_y == -5).all() and (next_rows == -6).all()
    copies = canary((2, B, T))
    refused(lambda: ops.smooth_noise(a, 0.25, 1234, ns=2, out=copies.t), copies)
    refused(lambda: ops.smoothadv_fill(a, 0.25, 1234, ns=2, out=copies.t), copies)
    grads = torch.randn(2, B, T, generator=g).to(cuda)
    gsum = canary()
    for norm in ("Linf", "L2"):
        refused(lambda: ops.smoothadv_step(a, b, grads, 0.02, 0.05, norm=norm, out=out.t, gsum=gsum.t), out, gsum)
    # one row fewer is served (the canaries of the outputs stay, their rows do not)
    n = B - 1
    ok, ok_state = Slot((n, T), cuda, 0), Slot((4, n), cuda, 0)
    a, b, c = a[:n], b[:n], c[:n]
    ops.fmn_step(a, b, c, z[:n], y[:n], old[:, :n].contiguous(), best.t[:n], ops.fmn_norms(a, b, c), 0.37, 0.05, "Linf",
                 state_out=ok_state.t, out=ok.t)
    torch.cuda.synchronize()
    assert ok.intact() and ok_state.intact() and (ok.t != CANARY).all() and (ok_state.t != CANARY).all()
