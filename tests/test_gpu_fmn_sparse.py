"""`-m gpu`: the kernel of include/advstep_fmn_sparse.h against float64, against the CPU table tests/fmn_sparse_cpu_ops.py and
against the existing device projections, the attack on a device LinearDetector with the host test's bounds, on the real
detector, host reads and the evaluation loop.

The bounds on the row sums are DERIVED from the kernel's summation order (include/advstep_fmn_sparse.h; the table's docstring):
gamma(n) resp. gamma(n + 1) relative to the float64 sum of the same float32 operands, n = 4 ceil(T / 4096) + 21; the count and
the maximum are exact.  Everything after the sums is compared bit for bit: the twin recomputes a launch from the launch's inputs
and the kernel's own row norms, and the projected rows are those of hip_ops.l1_box_project / l0_box_project applied row by row to
the twin's u with the row's own new radius (one row body, one traversal order: no tolerance).  No constant here was measured."""
import math

import pytest
import torch

from tests import fmn_sparse_cpu_ops as C
from tests.test_fmn_sparse_host import ATTACK_KW, check_attack_result
from tests.test_gpu_apgd import atk_call_context, detector, same
from tests.test_gpu_apgdl1 import L1_SLACK
from tests.test_gpu_fmn import detector_batch, wave_inputs
from tests.test_gpu_momentum import padded, untouched

pytestmark = pytest.mark.gpu

INF, NAN = math.inf, float("nan")
SHAPES = [(1, 257), (5, 4099), (8, 4100), (16, 8192), (2, 64_600)]     # 64 600: the L0 cut search walks 16 index bits
ALPHA, GAMMA = 0.37, 0.05


def hip():
    from audio_deepfake_adversarial_attacks_amd import hip_ops
    return hip_ops


def sparse_inputs(B, T, seed, norm):
    """tests/test_gpu_fmn.wave_inputs (by b % 8: 1 an all-zero gradient row, 5 a delta = 0 row, 6 a NaN in the gradient).  In L0
    the zero-gradient row is row 7, and row 1 — which every shape with two rows holds, (2, 64 600) among them — is the tie row:
    adv = orig = 0.5 and a gradient of one magnitude, so the scores take two values (one per sign: 0.5 + t and 0.5 - t round in
    different binades) and the row's radius of 10 cuts through a class of equal scores."""
    adv, grad, orig = wave_inputs(B, T, seed)
    if norm == "L0":
        for b in range(B):
            if b % 8 == 1:
                orig[b] = 0.5
                adv[b] = 0.5
                grad[b] = torch.where(torch.arange(T) % 3 == 0, -0.05, 0.05)
            if b % 8 == 7:
                grad[b] = 0.0
    return adv, grad, orig


def step_case(adv, orig, norm):
    """A state, logits and labels whose rows walk through every branch of the step, by b % 8.
    L1 (eps and best as multiples of the row's sum |d|):
      0 adversarial and better (found)          1 never found, zero gradient: eps' = inf  2 adversarial, not better
      3 not adversarial, found: eps grows       4 never found, eps = inf: the reach rule  5 delta = 0, already wrong: best' = eps' = 0
      6 never found, NaN in the gradient        7 NaN logit, y = 1: adversarial, first find
    L0 (eps and best in samples; dcnt is nearly T):
      0 adversarial and better: 40 shrinks      1 the tie row, never found: 9 -> 10        2 NaN logit, y = 1: adversarial, not better: 12 -> best = 5
      3 not adversarial, found: 100 grows       4 eps = T grows: eps' >= T, clamped to T   5 delta = 0, already wrong: best' = eps' = 0
      6 begin row, NaN in the gradient: 2       7 begin row, zero gradient: inf -> 1 -> 2"""
    B, T = adv.shape
    if norm == "L1":
        dn = (adv - orig).double().abs().sum(dim=1).float().clamp_min(1e-3)
        kinds = [(1.5, 2.0, 1.0, -1.5, 1), (INF, INF, 0.0, 2.0, 1), (1.0, 0.5, 1.0, 0.7, 0), (0.8, 0.7, 1.0, -0.4, 0),
                 (INF, INF, 0.0, 0.3, 1), (INF, INF, 0.0, -3.0, 1), (INF, INF, 0.0, -0.0, 0), (INF, INF, 0.0, NAN, 1)]
        want_copy = [True, False, False, False, False, True, False, True]
    else:
        dn = torch.ones(B)
        kinds = [(40.0, INF, 1.0, -1.5, 1), (9.0, INF, 0.0, 0.3, 1), (12.0, 5.0, 1.0, NAN, 1), (100.0, 90.0, 1.0, -0.4, 0),
                 (float(T), INF, 0.0, 0.3, 1), (INF, INF, 0.0, -3.0, 1), (INF, INF, 0.0, -0.0, 0), (INF, INF, 0.0, 2.0, 1)]
        want_copy = [True, False, False, False, False, True, False, False]
    rows = [kinds[b % 8] for b in range(B)]
    state = torch.stack([torch.tensor([r[0] for r in rows]) * dn, torch.tensor([r[1] for r in rows]) * dn,
                         torch.tensor([r[2] for r in rows]), torch.full((B,), 0.125)]).float()
    z = torch.tensor([r[3] for r in rows], dtype=torch.float32)
    y = torch.tensor([r[4] for r in rows], dtype=torch.int64)
    return state, z, y, [want_copy[b % 8] for b in range(B)]


def shifted(t, cuda, shift):
    """A device copy of `t` whose base lies `shift` floats past a 16-byte boundary (tests/test_gpu_row_edges.py's Slot)."""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=cuda)
    view = buf[shift:shift + t.numel()].view(t.shape)
    assert view.data_ptr() % 16 == 4 * shift
    view.copy_(t)
    return view


@pytest.mark.parametrize("B,T", SHAPES)
def test_row_norms_against_float64(cuda, B, T):
    ops = hip()
    adv, grad, orig = wave_inputs(B, T, seed=4000 + B + T)
    st = ops.fmn_begin(B=B, device=cuda)
    z, y = torch.ones(B, device=cuda), torch.ones(B, dtype=torch.int64, device=cuda)   # no row adversarial: no copy
    want = C.row_norms64(adv, grad, orig)
    nan_rows = torch.tensor([b % 8 == 6 for b in range(B)])
    zero_g = torch.tensor([b % 8 == 1 for b in range(B)])
    zero_d = torch.tensor([b % 8 == 5 for b in range(B)])
    for norm in ("L1", "L0"):
        # move = False reads no gradient: the g planes are 0, the d planes the move form's
        rbuf, rn0 = padded((4, B), -9.5, cuda, pad=64)
        best = torch.full((B, T), -2.5, device=cuda)
        new0, out0 = ops.fmn_sparse_step(adv.to(cuda), grad.to(cuda), orig.to(cuda), z, y, st, best, 0.0, GAMMA, norm, move=False,
                                         row_norms=rn0)
        torch.cuda.synchronize()
        assert out0 is None and (best == -2.5).all() and untouched(rbuf, -9.5, 4 * B, pad=64)
        rn = torch.full((4, B), -9.5, device=cuda)
        new, _ = ops.fmn_sparse_step(adv.to(cuda), grad.to(cuda), orig.to(cuda), z, y, st, best, 0.0, GAMMA, norm, move=True,
                                     row_norms=rn)
        got0, got = rn0.cpu().double(), rn.cpu().double()
        assert same(got0[:2], got[:2]) and (got0[2:] == 0).all() and (best == -2.5).all()
        assert same(got[1], want[1]) and same(got[3], want[3])                         # the count and max |g|: bit for bit
        assert torch.isnan(got[2])[nan_rows].all() and torch.isnan(got[3])[nan_rows].all()
        assert not torch.isnan(got[:, ~nan_rows]).any() and not torch.isnan(got[:2]).any()   # the NaN stays in its row and planes
        for plane, squares in ((0, False), (2, True)):
            ok = ~torch.isnan(want[plane])
            err = (got[plane] - want[plane]).abs()[ok]
            bound = C.sum_rel_bound(T, squares) * want[plane][ok]
            print(f"  {norm} {C.FMN_SPARSE_NORMS[plane]}: max err / bound = {(err / bound.clamp_min(1e-300)).max().item():.3f} (n = {C.chain(T)})")
            assert (err <= bound).all()
        assert (got[2][zero_g] == 0).all() and (got[3][zero_g] == 0).all() and (got[:2][:, zero_d] == 0).all()
        assert same(new[3].cpu(), rn.cpu()[0 if norm == "L1" else 1])                  # dnorm
        assert same(new0[1:], new[1:]) and (norm == "L1" or same(new0, new))           # one decision body (L1's reach rule reads gmax)


def reference_rows(ops, cuda, x, u, eps_rows, norm):
    """The existing device projections applied row by row, each row with its own radius: hip_ops.l1_box_project(x, u, eps'_b) /
    hip_ops.l0_box_project(x, u, int(eps'_b)).  They refuse a radius of 0, for which the kernel returns the x row."""
    rows = []
    for b in range(x.shape[0]):
        e = float(eps_rows[b])
        xb, ub = x[b:b + 1].to(cuda).contiguous(), u[b:b + 1].to(cuda).contiguous()
        if norm == "L1":
            rows.append(ops.l1_box_project(xb, ub, e).cpu() if e > 0 else x[b:b + 1].clone())
        else:
            rows.append(ops.l0_box_project(xb, ub, int(e)).cpu() if e >= 1 else x[b:b + 1].clone())
    return torch.cat(rows)


def launch_step(ops, cuda, tensors, norm, move, shift=0, alias=False):
    """One launch between canaries; returns CPU copies of (state_out, out, best_adv, row_norms)."""
    adv, grad, orig, state, z, y = tensors
    B, T = adv.shape
    dev = lambda t: shifted(t, cuda, shift) if t.dtype == torch.float32 and t.dim() == 2 and t.shape[1] == T else t.to(cuda)   # noqa: E731
    obuf, o_dev = padded((B, T), -7.25, cuda, pad=1024 + shift)
    bbuf, best = padded((B, T), -2.5, cuda, pad=1024 + shift)
    sbuf, new = padded((4, B), 9.5, cuda, pad=64)
    rn = torch.full((4, B), NAN, device=cuda)
    assert o_dev.data_ptr() % 16 == 4 * shift and best.data_ptr() % 16 == 4 * shift
    state_dev, adv_dev = state.to(cuda), dev(adv)
    if alias and move:
        o_dev.copy_(adv)
        adv_dev = o_dev
    got_state, out = ops.fmn_sparse_step(adv_dev, dev(grad), dev(orig), z.to(cuda), y.to(cuda), state_dev, best, ALPHA, GAMMA, norm,
                                         move=move, state_out=new, out=o_dev if move else None, row_norms=rn)
    torch.cuda.synchronize()
    assert got_state.data_ptr() == new.data_ptr() and untouched(bbuf, -2.5, B * T, pad=1024 + shift)
    assert untouched(sbuf, 9.5, 4 * B, pad=64) and untouched(obuf, -7.25, B * T, pad=1024 + shift)
    assert same(state_dev, state)                                                       # the launch only reads the old state
    if move:
        assert out.data_ptr() == o_dev.data_ptr()
    else:
        assert out is None and (o_dev == -7.25).all()                                   # the last call writes no `out`
    return new.cpu(), (out.cpu() if move else None), best.cpu(), rn.cpu()


@pytest.mark.parametrize("B,T", SHAPES)
@pytest.mark.parametrize("norm", ["L1", "L0"])
@pytest.mark.parametrize("move", [True, False])
def test_step_kernel_bit_for_bit(cuda, B, T, norm, move):
    ops = hip()
    adv, grad, orig = sparse_inputs(B, T, seed=4100 + B + T, norm=norm)
    state, z, y, want_copy = step_case(adv, orig, norm)
    tensors = (adv, grad, orig, state, z, y)
    new, out, best, rn = launch_step(ops, cuda, tensors, norm, move)
    want_best = torch.full((B, T), -2.5)
    want_state, want_out = C.fmn_sparse_step(adv, grad, orig, z, y, state, want_best, ALPHA, GAMMA, norm, move=move, given_norms=rn)
    assert same(new, want_state)
    assert same(best, want_best)
    copy = torch.tensor(want_copy)
    assert (best[~copy] == -2.5).all() and same(best[copy], adv[copy])                  # unimproved rows keep their bytes
    rows = lambda k: [b for b in range(B) if b % 8 == k]                                # noqa: E731
    eps1 = new[0]
    if norm == "L0":                                                                    # the radii step_case's docstring promises
        want_eps = {1: 10.0, 2: 5.0, 4: float(T), 5: 0.0, 6: 2.0, 7: 2.0}
        assert all(eps1[b] == want_eps[b % 8] for b in range(B) if b % 8 in want_eps)
        assert all(eps1[b] < 40 for b in rows(0)) and all(eps1[b] > 100 for b in rows(3))
    else:
        assert all(math.isinf(eps1[b].item()) for b in rows(1) + rows(6)) and all(eps1[b] == 0 and new[1, b] == 0 for b in rows(5))
    if move:
        u = C.move_point(adv, grad, ALPHA, rn[2])
        ref = reference_rows(ops, cuda, orig, u, eps1, norm)
        assert same(out, ref)                                                           # the existing device kernels' bits
        assert all(same(out[b], orig[b]) for b in rows(5))                              # already wrong: eps' = 0, the clean row
        nan_rows = torch.tensor([b % 8 == 6 for b in range(B)])
        assert not torch.isnan(out[~nan_rows]).any()                                    # a NaN never reaches another row
        fin = ~nan_rows
        assert out[fin].min() >= 0 and out[fin].max() <= 1
        if norm == "L0":
            assert same(out, want_out)                                                  # ... and the sort-based CPU table's
            changed = (out != orig).sum(dim=1)
            assert (changed[fin] <= eps1[fin]).all()
            for b in rows(1):                                                           # the tie row: exactly 10 samples, of ONE score class,
                idx = (out[b] != orig[b]).nonzero().reshape(-1)                         # the lowest indices of it
                assert idx.numel() == 10
                d = (u[b] - orig[b])
                score = d * d
                top = score.max()
                assert (score[idx] == top).all() and (score == top).sum() > 10
                assert same(idx, (score == top).nonzero().reshape(-1)[:10])
            for b in rows(4):                                                           # eps' >= T keeps every sample: as radius T + 1000 does
                assert same(out[b], C.project_rows(orig[b:b + 1], u[b:b + 1], torch.tensor([T + 1000.0]), "L0")[0])
        else:
            l1 = (out.double() - orig.double()).abs().sum(dim=1)
            ok = fin & (eps1 > 0) & ~torch.isinf(eps1)
            assert (l1[ok] <= eps1[ok].double() * (1 + L1_SLACK)).all()
            for b in rows(1):                                                           # zero gradient: u is the iterate itself
                assert same(u[b], adv[b])
    assert not torch.isnan(new[:, [b for b in range(B) if b % 8 not in (6,)]]).any()
    # the norms behind the decision against float64 (the norms' test has the bounds): dnorm is the row's norm
    n64 = C.row_norms64(adv, grad, orig)
    if norm == "L0":
        assert same(new[3].double(), n64[1])
    else:
        assert ((new[3].double() - n64[0]).abs() <= C.sum_rel_bound(T, False) * n64[0]).all()
    again = launch_step(ops, cuda, tensors, norm, move, alias=True)                     # out = adv, and a rerun: the same bytes
    assert same(again[0], new) and same(again[2], best) and same(again[3], rn)
    if move:
        assert same(again[1], out)
    if T % 4 == 0:      # every row tensor one float past a 16-byte boundary: 4-byte accesses in the quads' order, the same bytes
        for alias in (False, True):
            off = launch_step(ops, cuda, tensors, norm, move, shift=1, alias=alias)
            assert same(off[0], new) and same(off[2], best)
            assert same(off[3][:2], rn[:2]) and (not move or (same(off[3], rn) and same(off[1], out)))
    if move:            # the decision of the move = 0 form equals the move form's (one body)
        st0, _ = ops.fmn_sparse_step(adv.to(cuda), None, orig.to(cuda), z.to(cuda), y.to(cuda), state.to(cuda),
                                     torch.empty(B, T, device=cuda), 0.0, GAMMA, norm, move=False)
        if norm == "L0":
            assert same(st0, new)
        else:   # without the gradient gmax = 0: only the never-found rows' reach rule differs (eps' = inf)
            reach = torch.tensor([b % 8 in (4,) for b in range(B)])
            assert same(st0.cpu()[1:], new[1:]) and same(st0.cpu()[0][~reach], new[0][~reach]) and torch.isinf(st0.cpu()[0][reach]).all()


def nan_radius_case(T, norm):
    """Three rows whose middle one gets eps' = NaN.  L1: never found, a NaN logit with y = 0 (class 0: not adversarial) and a
    gradient, so the reach rule adds |NaN| / gmax.  L0, whose rule reads no logit: a NaN radius in the caller's state (found, not
    adversarial).  Rows 0 and 2 are ordinary: adversarial and better, and found and growing."""
    adv, grad, orig = wave_inputs(3, T, seed=4300 + T)
    grad[1] = grad[0].flip(0)                                                           # wave_inputs' row 1 has no gradient
    dn = (adv - orig).double().abs().sum(dim=1).float() if norm == "L1" else torch.ones(3)
    if norm == "L1":
        rows = [(1.5, 2.0, 1.0, -1.5, 1), (INF, INF, 0.0, NAN, 0), (0.8, 0.7, 1.0, -0.4, 0)]
    else:
        rows = [(40.0, INF, 1.0, -1.5, 1), (NAN, INF, 1.0, 0.3, 1), (100.0, 90.0, 1.0, -0.4, 0)]
    state = torch.stack([torch.tensor([r[0] for r in rows]) * dn, torch.tensor([r[1] for r in rows]) * dn,
                         torch.tensor([r[2] for r in rows]), torch.full((3,), 0.125)]).float()
    return adv, grad, orig, state, torch.tensor([r[3] for r in rows], dtype=torch.float32), torch.tensor([r[4] for r in rows])


@pytest.mark.parametrize("T", [4099, 4100])
@pytest.mark.parametrize("norm", ["L1", "L0"])
def test_a_nan_radius_stays_in_its_row_and_every_sample_is_written(cuda, norm, T):
    """The header's edge row: a NaN eps' fails phi(0) > eps' in L1 (lambda = 0: the move clamped to the box) and every
    comparison of the L0 search (every sample kept); the kernel terminates, writes the whole row and leaves its neighbours alone."""
    ops = hip()
    tensors = nan_radius_case(T, norm)
    adv, grad, orig, state, z, y = tensors
    new, out, best, rn = launch_step(ops, cuda, tensors, norm, True)                    # (its canaries are checked inside)
    want_best = torch.full((3, T), -2.5)
    want_state, want_out = C.fmn_sparse_step(adv, grad, orig, z, y, state, want_best, ALPHA, GAMMA, norm, move=True, given_norms=rn)
    assert same(new, want_state) and same(best, want_best)
    assert torch.isnan(new[0, 1]) and not torch.isnan(new[0, [0, 2]]).any() and not torch.isnan(rn).any()
    assert new[1, 1] == INF and (best[1] == -2.5).all() and same(best[0], adv[0])      # the NaN row is no find; row 0 is copied
    u = C.move_point(adv, grad, ALPHA, rn[2])
    x1, u1 = orig[1:2], u[1:2]
    assert same(out[1], C.project_rows(x1, u1, torch.tensor([NAN]), norm)[0])
    if norm == "L1":                                                                    # lambda = 0: every coordinate moves as far as the box lets it
        d1 = u1 - x1
        assert same(out[1], (x1 + torch.sign(d1) * torch.minimum(d1.abs(), torch.where(d1 > 0, 1.0 - x1, x1))).clamp(0.0, 1.0)[0])
    else:                                                                               # every sample kept: as a radius past T keeps them
        assert same(out[1], C.project_rows(x1, u1, torch.tensor([T + 1000.0]), "L0")[0])
    assert torch.isfinite(out).all() and out.min() >= 0 and out.max() <= 1              # every in-row sample written, none NaN
    others = [0, 2]                                                                     # the neighbours: the existing device kernels' bits
    assert same(out[others], reference_rows(ops, cuda, orig[others], u[others], new[0][others], norm))
    assert not torch.isnan(new[0][others]).any() and (new[0][others] > 0).all()
    for shift, alias in ((0, True),) + (((1, False), (1, True)) if T % 4 == 0 else ()):   # out = adv; bases off the 16-byte grid
        again = launch_step(ops, cuda, tensors, norm, True, shift=shift, alias=alias)
        assert same(again[0], new) and same(again[1], out) and same(again[2], best) and same(again[3], rn)
    last = launch_step(ops, cuda, tensors, norm, False)                                 # the decision-only form writes no `out`
    e_last = last[0][0, 1]                       # L0: the same NaN; L1: without the gradient gmax = 0 and the reach rule gives +inf
    assert (torch.isnan(e_last) if norm == "L0" else e_last == INF) and same(last[0][1:], new[1:]) and same(last[2], best)


def test_empty_work_and_wrapper_checks(cuda):
    ops = hip()
    st = ops.fmn_begin(B=3, device=cuda)
    out = torch.full((4, 3), 9.5, device=cuda)
    y = torch.zeros(3, dtype=torch.int64, device=cuda)
    e = torch.empty(3, 0, device=cuda)
    got, _ = ops.fmn_sparse_step(e, e.clone(), e.clone(), torch.zeros(3, device=cuda), y, st, e.clone(), 0.5, 0.05, "L0", state_out=out)
    assert got.data_ptr() == out.data_ptr() and (out == 9.5).all()       # rows of no samples: nothing launched, nothing written
    x = torch.rand(3, 8, device=cuda)
    with pytest.raises(ValueError, match="'L1' or 'L0'"):
        ops.fmn_sparse_step(x, x.clone(), x.clone(), torch.zeros(3, device=cuda), y, st, x.clone(), 0.5, 0.05, "L2")
    with pytest.raises(ValueError, match=r"\(0, 1\)"):
        ops.fmn_sparse_step(x, x.clone(), x.clone(), torch.zeros(3, device=cuda), y, st, x.clone(), 0.5, 1.0, "L1")
    with pytest.raises(ValueError, match="needs the gradient"):
        ops.fmn_sparse_step(x, None, x.clone(), torch.zeros(3, device=cuda), y, st, x.clone(), 0.5, 0.05, "L1")
    with pytest.raises(Exception):                                       # the library refuses state_out = state (EINVAL)
        ops.fmn_sparse_step(x, x.clone(), x.clone(), torch.zeros(3, device=cuda), y, st, x.clone(), 0.5, 0.05, "L1", state_out=st)


# ---- the attack ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T", [257, 4099])
@pytest.mark.parametrize("norm", ["L1", "L0"])
def test_attack_on_a_device_linear_detector(cuda, norm, T):
    """The attack of tests/test_fmn_sparse_host.py through hip_ops, with that test's bounds (check_attack_result)."""
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    model, flat, x, y, true = C.linear_case(T, norm, seed=T)
    model, flat, x, y = model.to(cuda), flat.to(cuda), x.to(cuda), y.to(cuda)
    atk = torchattacks.FMNSparse(model, norm=norm, steps=100, **ATTACK_KW[norm])
    adv = atk(x, y)
    assert atk.last_radius.is_cuda and adv.data_ptr() != x.data_ptr()
    check_attack_result(atk, model, x, y, adv, true, norm)
    radius = atk.last_radius.clone()
    assert same(atk(x, y), adv) and same(atk.last_radius, radius)                       # same call, same bytes
    atk0 = torchattacks.FMNSparse(flat, norm=norm, steps=5, **ATTACK_KW[norm])          # w = 0: the clean input with +inf
    adv0 = atk0(x, y)
    assert torch.isinf(atk0.last_radius).all() and (atk0.last_radius > 0).all() and same(adv0, x)


@pytest.mark.parametrize("norm", ["L1", "L0"])
def test_attack_on_the_detector_and_no_host_read(cuda, norm):
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    model = detector("lcnn", cuda)
    x01, y = detector_batch(cuda, model)
    T = x01.shape[1]
    # L0 takes the registry's 100 steps: its radius starts at one sample, and this detector's rows flip at thousands of them
    atk = torchattacks.FMNSparse(model, norm=norm, steps=12 if norm == "L1" else 100, **ATTACK_KW[norm])
    atk.set_training_mode(model_training=True, batchnorm_training=False)
    best_adv = atk(x01, y)                                              # warm-up as well: plans, kernels loaded
    radius = atk.last_radius.cpu()
    print("  radii:", radius.tolist())
    assert best_adv.min() >= 0 and best_adv.max() <= 1 and best_adv.data_ptr() != x01.data_ptr()
    finite = ~torch.isinf(radius)
    with atk_call_context(atk), torch.no_grad():                        # the mode the attack ran (and judged) the model in
        wrong_clean = C.judged_wrong(model(x01).reshape(-1), y)
        flipped = C.judged_wrong(model(best_adv).reshape(-1), y)
    assert same(radius == 0, wrong_clean.cpu())                          # radius 0: exactly the rows the clean input gets wrong
    assert flipped.cpu()[finite].all()                                   # every finite-radius row is misclassified
    d = (best_adv - x01).cpu()
    if norm == "L0":
        assert same((d != 0).sum(dim=1)[finite].float(), radius[finite])                # the count of changed samples IS the radius
    else:
        dn = d.double().abs().sum(dim=1)
        assert ((dn - radius.double()).abs()[finite] <= C.gamma_k(C.chain(T) + 1) * dn[finite]).all()
    still = (radius == 0) | ~finite
    assert same(best_adv.cpu()[still], x01.cpu()[still])                # 0 and +inf rows are the clean input
    assert (radius[finite] >= 0).all()
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            torch.ones(1, device=cuda).item()                           # the mode works on this build
        with atk_call_context(atk):
            again = atk.forward(x01, y)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert same(again, best_adv) and same(atk.last_radius, radius)      # no random start: same call, same bytes


@pytest.mark.parametrize("member", ["FMN_L1", "FMN_L0"])
def test_evaluation_loop_reports_the_radii(cuda, member):
    """generate_attacks() with the registry's members (8 steps instead of 100: the report, not the attack's strength, is under
    test) on 16 synthetic utterances: min_radius/* with the robust accuracies at report_at."""
    from audio_deepfake_adversarial_attacks_amd.aa.aa_types import AttackEnum
    from audio_deepfake_adversarial_attacks_amd.datasets.synthetic import SyntheticDetectionDataset
    from audio_deepfake_adversarial_attacks_amd.evaluation import generate_attacks
    from audio_deepfake_adversarial_attacks_amd.metrics import radius_summary
    from audio_deepfake_adversarial_attacks_amd.utils import set_seed
    cfg = {"data": {"seed": 42}, "checkpoint": {"path": ""},
           "model": {"name": "lcnn", "parameters": {"frontend_algorithm": ["lfcc"], "input_channels": 1}}}
    cls, params = AttackEnum[member].value
    params = dict(params, steps=8)
    loader = dict(batch_size=8, shuffle=False, num_workers=0)        # in-process loading: no worker start-up inside a long suite
    set_seed(42)
    rep = generate_attacks([None, None, None], cfg, str(cuda), attack_model_config=cfg, attack_method=cls, attack_params=params,
                           dataset=SyntheticDetectionDataset(16), share_weights=True, return_scores=True, **loader)
    torch.cuda.synchronize()
    report_at = params["report_at"]
    keys = ["min_radius/median", "min_radius/p10", "min_radius/p90", "min_radius/unflipped_share",
            "min_radius/already_wrong_share"] + [f"min_radius/robust_acc@{e:g}" for e in report_at]
    assert [k for k in rep if k.startswith("min_radius/")] == keys
    radii = rep["scores"]["min_radius"]
    assert radii.shape == (16,) and radii.dtype.name == "float32" and rep["num_total"] == 16
    assert {k: rep[k] for k in keys} == radius_summary(radii, report_at)
    assert "changed" not in rep["scores"]                                               # no last_changed report: the radius is per row
    set_seed(42)
    clean = generate_attacks([None, None, None], cfg, str(cuda), attack_model_config=None, attack_method=None,
                             dataset=SyntheticDetectionDataset(16), **loader)
    assert clean["num_total"] == 16 and 0.0 <= rep["adv_eval/accuracy"] <= clean["adv_eval/accuracy"] + 1e-9
