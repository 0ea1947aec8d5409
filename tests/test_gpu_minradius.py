"""`-m gpu`: the minimal-radius kernels (include/advstep_radius.h) against the CPU table tests/radius_cpu_ops.py and against
float64, the analytic search on the device, MinRadiusPGD on the detectors, hipGraph replay, host reads and the evaluation loop.

The bound on the L2 step's row norms is DERIVED from the kernels' summation order (csrc/radius.hip, which is advstep.hip's):
with u = 2^-24, every square rounds once; a thread adds its 4 quads, each as (x^2 + y^2) + (z^2 + w^2), one after the other
(2 + 4 additions deep), a wave adds in 6 shuffle levels, the 4 waves in 3, and the re-reduction adds ceil(C / 256) partials per
thread (C = ceil(T / 4096) tiles), then 6 + 3 again: n = 24 + ceil(C / 256) additions on the longest chain, all over
non-negative terms.  To first order the sum is within (n + 1) u of the float64 sum of the same float32 operands, relatively; the
square root halves that and rounds once:
    |norm - norm64| <= ((n + 1) / 2 + 1) u norm64                               (radius_cpu_ops.norm_rel_bound)
and a row leaves the step within
    ||out - orig||_2 <= e (1 + ((n + 1) / 2 + 1) u + 3 u) + u sqrt(T)           (radius_cpu_ops.l2_ball_bound)
of orig: f <= (e / dn)(1 + 2u), dn >= ||d|| (1 - the bound above), d * f rounds once, and orig + d * f rounds to within u of a
value in [0, 1] per sample.  No constant here was measured."""
import math

import pytest
import torch

from tests import radius_cpu_ops as C
from tests.test_gpu_apgd import atk_call_context, detector, same
from tests.test_gpu_momentum import padded, untouched

pytestmark = pytest.mark.gpu

# one tile scalar, two tiles with unaligned rows, two exact vector tiles, four tiles with an odd T
SHAPES = [(1, 257), (5, 4099), (3, 8192), (7, 12_289)]
RADII = (0.003, 0.0, 1e-7, 0.25, 0.0005, 0.0, 0.02)          # by row: 0, tiny and large within one batch


def hip():
    from audio_deepfake_adversarial_attacks_amd import hip_ops
    return hip_ops


def step_inputs(B, T, seed, nan=True):
    """orig in [0, 1] with exact 0s and 1s, adv inside each row's ball with samples on its faces, gradients with zeros, a NaN
    and (B > 1) an all-zero row."""
    g = torch.Generator().manual_seed(seed)
    e = torch.tensor([RADII[b % len(RADII)] for b in range(B)], dtype=torch.float32)
    orig = torch.rand(B, T, generator=g)
    orig[:, ::17] = 0.0
    orig[:, 5::19] = 1.0
    adv = (orig + (torch.rand(B, T, generator=g) * 2 - 1) * e[:, None]).clamp(0, 1)
    adv[:, 3::11] = (orig[:, 3::11] + e[:, None]).clamp(0, 1)                        # on the ball's face
    adv[:, 4::23] = (orig[:, 4::23] - e[:, None]).clamp(0, 1)
    grad = torch.randn(B, T, generator=g)
    grad[:, ::13] = 0.0
    if nan:
        grad[0, 7] = float("nan")
    if B > 1:
        grad[1] = 0.0                                                               # one all-zero gradient row
    return adv, grad, orig, e


@pytest.mark.parametrize("B,T", SHAPES)
@pytest.mark.parametrize("alpha_abs,alpha_rel,alias", [(0.0, 0.25, False), (0.0004, 0.0, True), (0.0002, 0.5, False)])
def test_row_linf_step_kernel(cuda, B, T, alpha_abs, alpha_rel, alias):
    ops = hip()
    adv, grad, orig, e = step_inputs(B, T, seed=2000 + B + T)
    want = C.row_pgd_linf_step(adv, grad, orig, e, alpha_abs, alpha_rel)

    def launch():
        obuf, o_dev = padded((B, T), -7.25, cuda)
        adv_dev = adv.to(cuda)
        if alias:
            o_dev.copy_(adv)
            adv_dev = o_dev
        out = ops.row_pgd_linf_step(adv_dev, grad.to(cuda), orig.to(cuda), e.to(cuda), alpha_abs, alpha_rel, out=o_dev)
        torch.cuda.synchronize()
        assert out.data_ptr() == o_dev.data_ptr() and untouched(obuf, -7.25, B * T)
        return out.cpu()

    got = launch()
    assert same(got, want)                                                          # bit for bit
    assert same(got, launch())
    d = (got - orig).double().abs()
    ok = ~torch.isnan(d)
    assert (d[ok] <= (e[:, None].double() + 2.0 ** -24).expand_as(d)[ok]).all()
    zero = e == 0
    if alpha_abs == 0.0:
        assert same(got[zero], orig[zero])                                          # a radius-0 row is the clean row


@pytest.mark.parametrize("B,T", SHAPES)
def test_row_linf_step_equals_the_fixed_radius_kernel(cuda, B, T):
    ops = hip()
    adv, grad, orig, _ = step_inputs(B, T, seed=2100 + B + T)
    eps, alpha = 0.003, 0.0004
    adv = (orig + (adv - orig).clamp(-eps, eps)).clamp(0, 1)
    a, g, x = adv.to(cuda), grad.to(cuda), orig.to(cuda)
    rows = torch.full((B,), eps, device=cuda)
    assert same(ops.row_pgd_linf_step(a, g, x, rows, alpha, 0.0), ops.pgd_linf_step(a, g, x, alpha, eps))


def check_l2_launch(adv, grad, orig, e, alpha_abs, alpha_rel, out, gnorm, dnorm, eps_div=1e-10):
    """One row_pgd_l2_step launch (CPU copies) against float64 within the derived bound, and its elementwise tail bit for bit
    from the kernel's own norms."""
    B, T = adv.shape
    bound = C.norm_rel_bound(T)
    gn64 = grad.double().norm(dim=1)
    err = (gnorm.double() - gn64).abs()
    print(f"  ||g||: max err / bound = {(err / (bound * gn64).clamp_min(1e-300)).max().item():.3f} (n = {C.chain(T)})")
    assert (err <= bound * gn64).all()
    ecol, a = C._row_scalars(e, alpha_abs, alpha_rel, adv)
    d = C.l2_delta(adv, grad, orig, a, gnorm, eps_div)                               # the kernel's own d, bit for bit
    dn64 = d.double().norm(dim=1)
    err = (dnorm.double() - dn64).abs()
    print(f"  ||d||: max err / bound = {(err / (bound * dn64).clamp_min(1e-300)).max().item():.3f}")
    assert (err <= bound * dn64).all()
    assert same(out, C.l2_tail(orig, d, ecol, dnorm))
    assert not torch.isnan(out).any()
    for b in range(B):
        assert (out[b] - orig[b]).double().norm().item() <= C.l2_ball_bound(e[b].item(), T)


@pytest.mark.parametrize("B,T", SHAPES)
@pytest.mark.parametrize("alpha_abs,alpha_rel,alias", [(0.0, 0.25, False), (0.01, 0.0, True), (0.001, 0.5, False)])
def test_row_l2_step_kernel(cuda, B, T, alpha_abs, alpha_rel, alias):
    ops = hip()
    adv, grad, orig, e = step_inputs(B, T, seed=2200 + B + T, nan=False)
    e = e * 10                                                                      # L2 radii: 0 .. 2.5

    def launch():
        obuf, o_dev = padded((B, T), -7.25, cuda)
        adv_dev = adv.to(cuda)
        if alias:
            o_dev.copy_(adv)
            adv_dev = o_dev
        out, gn, dn = ops.row_pgd_l2_step(adv_dev, grad.to(cuda), orig.to(cuda), e.to(cuda), alpha_abs, alpha_rel, out=o_dev,
                                          return_norms=True)
        torch.cuda.synchronize()
        assert out.data_ptr() == o_dev.data_ptr() and untouched(obuf, -7.25, B * T)
        return out.cpu(), gn.cpu(), dn.cpu()

    out, gn, dn = launch()
    check_l2_launch(adv, grad, orig, e, alpha_abs, alpha_rel, out, gn, dn)
    if B > 1:
        assert gn[1] == 0                                                           # the all-zero gradient row
    for a, b in zip((out, gn, dn), launch()):                                       # no atomics: reruns are bit-identical
        assert same(a, b)
    # without the norm outputs: the same bytes
    assert same(ops.row_pgd_l2_step(adv.to(cuda), grad.to(cuda), orig.to(cuda), e.to(cuda), alpha_abs, alpha_rel), out)


def test_row_l2_step_keeps_a_radius_zero_row_where_it_is(cuda):
    """e = 0 under a relative step: d = 0, ||d|| = 0, and the row comes back as orig (the fixed-radius expression's
    (1 / 0) * 0 would be NaN)."""
    ops = hip()
    _, grad, orig, _ = step_inputs(3, 4099, seed=5, nan=False)
    e = torch.tensor([0.0, 0.0, 0.1])                                  # row 1 has no gradient either
    out, gn, dn = ops.row_pgd_l2_step(orig.to(cuda), grad.to(cuda), orig.to(cuda), e.to(cuda), 0.0, 0.25, return_norms=True)
    assert same(out[0], orig[0]) and same(out[1], orig[1]) and dn[0] == 0 and dn[1] == 0 and dn[2] > 0
    check_l2_launch(orig, grad, orig, e, 0.0, 0.25, out.cpu(), gn.cpu(), dn.cpu())


@pytest.mark.parametrize("B,T", SHAPES)
def test_row_l2_step_equals_the_fixed_radius_kernel(cuda, B, T, monkeypatch):
    monkeypatch.setenv("ADVSTEP_L2_SINGLE_PASS", "0")                               # the three-launch form
    ops = hip()
    adv, grad, orig, _ = step_inputs(B, T, seed=2300 + B + T, nan=False)
    eps, alpha = 0.1, 0.02
    a, g, x = adv.to(cuda), grad.to(cuda), orig.to(cuda)
    rows = torch.full((B,), eps, device=cuda)
    got = ops.row_pgd_l2_step(a, g, x, rows, alpha, 0.0, return_norms=True)
    want = ops.pgd_l2_step(a, g, x, alpha, eps, return_norms=True)
    for p, q in zip(got, want):
        assert same(p, q)


# ---- begin and round -----------------------------------------------------------------------------------------------------------

def round_case(B, T, seed):
    """A state, logits and labels whose rows walk through every branch of the round, by b % 8:
    0 flipped, eps < best = inf (copy)      1 held (copy iff first)               2 radius-0 row, flipped (nothing)
    3 NaN logit, y = 1: flipped (copy)      4 NaN logit, y = 0: held              5 flipped, eps == best (nothing)
    6 flipped, eps < finite best (copy)     7 z = -0.0, y = 0: held"""
    g = torch.Generator().manual_seed(seed)
    inf, nan = math.inf, float("nan")
    kinds = [  # lo, hi, eps, best, z, y
        (0.0, 0.25, 0.25, inf, -1.5, 1), (0.0, 0.25, 0.125, 0.25, 2.0, 1), (0.0, 0.0, 0.0, 0.0, -3.0, 1),
        (0.0625, 0.125, 0.09375, 0.125, nan, 1), (0.0, 0.25, 0.25, inf, nan, 0), (0.0, 0.125, 0.125, 0.125, 0.5, 0),
        (0.03125, 0.0625, 0.046875, 0.0625, 1.0, 0), (0.125, 0.25, 0.1875, 0.25, -0.0, 0)]
    rows = [kinds[b % 8] for b in range(B)]
    state = torch.tensor([[r[p] for r in rows] for p in range(4)], dtype=torch.float32)
    z = torch.tensor([r[4] for r in rows], dtype=torch.float32)
    y = torch.tensor([r[5] for r in rows], dtype=torch.int64)
    adv = torch.rand(B, T, generator=g)
    adv[:, 1::29] = float("nan")                                                    # a copy moves bits, NaN payloads included
    return state, z, y, adv


@pytest.mark.parametrize("B,T", SHAPES + [(8, 4099), (16, 8192)])
@pytest.mark.parametrize("first", [True, False])
def test_radius_round_kernel(cuda, B, T, first):
    ops = hip()
    state, z, y, adv = round_case(B, T, seed=B * T)
    copy, want_state = C.round_decision(z, y, first, state)
    want_best = torch.full((B, T), -2.5)
    C.radius_round(adv, z, y, first, state, want_best)
    bbuf, best = padded((B, T), -2.5, cuda)
    sbuf, new = padded((4, B), 9.5, cuda, pad=64)
    state_dev = state.to(cuda)
    got = ops.radius_round(adv.to(cuda), z.to(cuda), y.to(cuda), first, state_dev, best, out=new)
    torch.cuda.synchronize()
    assert got.data_ptr() == new.data_ptr() and untouched(bbuf, -2.5, B * T) and untouched(sbuf, 9.5, 4 * B, pad=64)
    assert same(state_dev, state)                                                   # the launch only reads the old state
    assert same(new, want_state)
    assert same(best, want_best)
    assert (best.cpu()[~copy] == -2.5).all()                                        # only rows whose decision is "copy" change
    assert same(best.cpu()[copy], adv[copy])
    if B >= 8:
        assert copy.tolist()[:8] == [True, first, False, True, first, False, True, first]
    again = ops.radius_round(adv.to(cuda), z.to(cuda), y.to(cuda), first, state_dev, torch.full((B, T), -2.5, device=cuda))
    assert same(again, new)


@pytest.mark.parametrize("B", [1, 5, 257, 1000])
def test_radius_begin_kernel(cuda, B):
    ops = hip()
    g = torch.Generator().manual_seed(B)
    z0 = torch.randn(B, generator=g)
    z0[::5] = 0.0
    z0[1::7] = float("nan")
    z0[2::11] = -0.0
    y = torch.randint(0, 2, (B,), generator=g)
    sbuf, st = padded((4, B), 9.5, cuda, pad=64)
    got = ops.radius_begin(z0.to(cuda), y.to(cuda), 0.001, st)
    torch.cuda.synchronize()
    assert got.data_ptr() == st.data_ptr() and untouched(sbuf, 9.5, 4 * B, pad=64)
    assert same(st, C.radius_begin(z0, y, 0.001))
    fresh = ops.radius_begin(z0.to(cuda).reshape(B, 1), y.to(cuda), 0.001)         # the model's (B, 1) logits, an own state
    assert same(fresh, st)


# ---- the search ----------------------------------------------------------------------------------------------------------------

def check_search_result(model, x, y, best_adv, radius, norm, expected=None):
    """Exact radii where they are known, and the invariants of best_adv: every finite row is flipped when judged in eval mode
    and lies within its radius of x, radius-0 rows equal x bit for bit, inf rows are not flipped."""
    radius_c = radius.cpu()
    print("  radii:", radius_c.tolist())
    if expected is not None:
        assert same(radius_c, expected)
    model.eval()
    with torch.no_grad():
        flipped = C.judged_wrong(model(best_adv).reshape(-1), y)
    finite = ~torch.isinf(radius_c)
    assert flipped[finite].all() and not flipped[~finite].any()
    d = (best_adv - x).double().cpu()
    T = x.shape[1]
    for b in torch.nonzero(finite).reshape(-1).tolist():
        if norm == "Linf":
            assert d[b].abs().max().item() <= radius_c[b].item() + 2.0 ** -23
        else:
            assert d[b].norm().item() <= C.l2_ball_bound(radius_c[b].item(), T)
    zero = (radius_c == 0).to(x.device)
    assert same(best_adv[zero], x[zero])
    assert best_adv.min() >= 0 and best_adv.max() <= 1 and best_adv.data_ptr() != x.data_ptr()


@pytest.mark.parametrize("B,T", [(5, 4099), (3, 8192)])
@pytest.mark.parametrize("norm", ["Linf", "L2"])
def test_analytic_search_on_the_device(cuda, B, T, norm, monkeypatch):
    """The search of tests/test_minradius_host.py through hip_ops: the same exact radii (0, the smallest grid point above
    |z(x)| / ||w||, inf)."""
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    monkeypatch.setenv("ADVSTEP_ATTACK_GRAPH", "0")          # the float64 surrogate is not a capture workload (replay: below)
    eps_max, S, steps = 2.0 ** -6, 5, 4
    model, x, y, true, expected = C.analytic_case(B, T, norm, eps_max, S, seed=B + T)
    model, x, y = model.to(cuda), x.to(cuda), y.to(cuda)
    atk = torchattacks.MinRadiusPGD(model, norm=norm, eps_max=eps_max, search_steps=S, steps=steps)
    best_adv = atk(x, y)
    print("  true :", [f"{v:.6g}" for v in true.tolist()])
    check_search_result(model, x, y, best_adv, atk.last_radius, norm, expected)
    assert atk.last_radius.is_cuda and atk.last_radius.shape == (B,)


# eps_max per norm and the seed of the four synthetic utterances: chosen so that at least one row of the untrained detector
# breaks strictly inside (0, eps_max]; the test requires it.  L-inf: the rows of this seed break near 0.002.  L2: an L-inf
# perturbation of radius r lies inside the L2 ball of r sqrt(T) = 0.002 * 254, so a flip exists within about 0.5; 2.0 leaves
# four PGD steps room to find one
DETECTOR_CASE = {"Linf": 0.003, "L2": 2.0}
DETECTOR_SEED = 41


def detector_batch(cuda, model):
    from audio_deepfake_adversarial_attacks_amd.datasets.synthetic import synthetic_waveforms
    x, _ = synthetic_waveforms(4, seed=DETECTOR_SEED)
    x01, _, _ = hip().to_minmax(x.to(cuda))
    with torch.no_grad():
        y = (model(x01).reshape(-1) > 0).long()                                     # every row starts classified correctly ...
    y[0] = 1 - y[0]                                                                 # ... but one: radius 0
    return x01, y


@pytest.mark.parametrize("norm", ["Linf", "L2"])
def test_whole_attack_on_the_detector(cuda, norm, monkeypatch):
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    monkeypatch.setenv("ADVSTEP_ATTACK_GRAPH", "0")
    model = detector("lcnn", cuda)
    x01, y = detector_batch(cuda, model)
    atk = torchattacks.MinRadiusPGD(model, norm=norm, eps_max=DETECTOR_CASE[norm], search_steps=4, steps=4)
    atk.set_training_mode(model_training=True, batchnorm_training=False)
    with atk_call_context(atk):
        before = [m.training for m in model.modules()]
        best_adv = atk.forward(x01, y)
        assert [m.training for m in model.modules()] == before and any(before)
    radius = atk.last_radius.cpu()
    check_search_result(model, x01, y, best_adv, atk.last_radius, norm)
    assert radius[0] == 0 and (radius[1:] > 0).all() and (radius[~torch.isinf(radius)] <= DETECTOR_CASE[norm]).all()
    inside = (radius > 0) & ~torch.isinf(radius)
    assert inside.any()                                                             # see DETECTOR_CASE
    again = atk(x01, y)                                                             # no random start: same call, same bytes
    assert same(again, best_adv) and same(atk.last_radius, radius)


@pytest.fixture()
def fresh_graphs():
    from audio_deepfake_adversarial_attacks_amd.torchattacks import graphed
    graphed.clear()
    yield graphed
    graphed.clear()


@pytest.mark.parametrize("norm", ["Linf", "L2"])
def test_graph_replay_is_bit_identical(cuda, fresh_graphs, monkeypatch, norm):
    """ADVSTEP_ATTACK_GRAPH = 0, 1 and fused give the same bytes.  The radii are device data, so in the split form ONE capture
    of the model part serves every round of every call: it is taken in the first call's second round (the judge puts every
    training flag back, so the key repeats) and the step is launched between the replays with the round's own radii.  The
    fused form would bake one round's radius plane into its graph: the attack stays eager under it.  The rows of this case
    break at different radii, so every round steps with other radii than the round before."""
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    model = detector("lcnn", cuda)
    x01, y = detector_batch(cuda, model)

    def make():
        atk = torchattacks.MinRadiusPGD(model, norm=norm, eps_max=DETECTOR_CASE[norm], search_steps=4, steps=4)
        atk.set_training_mode(model_training=True, batchnorm_training=False)
        return atk

    atk = make()
    monkeypatch.setenv("ADVSTEP_ATTACK_GRAPH", "0")
    want = atk(x01, y)
    want_radius = atk.last_radius.clone()
    finite = want_radius[~torch.isinf(want_radius)]
    assert len(fresh_graphs._GRAPHS) == 0 and finite.unique().numel() >= 2 and not torch.equal(want, x01)
    monkeypatch.setenv("ADVSTEP_ATTACK_GRAPH", "1")
    for call in range(3):
        got = atk(x01, y)
        assert len(fresh_graphs._GRAPHS) == 1                 # one capture, whatever the round and the call
        assert torch.equal(got, want) and same(atk.last_radius, want_radius), call
    other = make()
    assert torch.equal(other(x01, y), want) and len(fresh_graphs._GRAPHS) == 1      # same family: the first object's capture
    assert same(other.last_radius, want_radius)
    monkeypatch.setenv("ADVSTEP_ATTACK_GRAPH", "fused")
    for call in range(3):
        fused = make()
        assert torch.equal(fused(x01, y), want) and same(fused.last_radius, want_radius), call
        assert len(fresh_graphs._GRAPHS) == 1                 # no fused capture was added


def test_radius_round_passes_empty_work_through(cuda):
    """Rows of no samples (and no rows): OK from the library, nothing launched, nothing written — `out` included."""
    ops = hip()
    st = torch.zeros(4, 3, device=cuda)
    out = torch.full((4, 3), 9.5, device=cuda)
    y = torch.zeros(3, dtype=torch.int64, device=cuda)
    got = ops.radius_round(torch.empty(3, 0, device=cuda), torch.zeros(3, device=cuda), y, True, st, torch.empty(3, 0, device=cuda),
                           out=out)
    assert got.data_ptr() == out.data_ptr() and (out == 9.5).all()
    empty = ops.radius_round(torch.empty(0, 8, device=cuda), torch.empty(0, device=cuda), y[:0], True, st[:, :0].contiguous(),
                             torch.empty(0, 8, device=cuda))
    assert empty.shape == (4, 0)


@pytest.mark.parametrize("norm", ["Linf", "L2"])
def test_forward_makes_no_host_read(cuda, monkeypatch, norm):
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    monkeypatch.setenv("ADVSTEP_ATTACK_GRAPH", "0")
    model = detector("lcnn", cuda)
    x01, y = detector_batch(cuda, model)
    atk = torchattacks.MinRadiusPGD(model, norm=norm, eps_max=DETECTOR_CASE[norm], search_steps=2, steps=4)
    atk.set_training_mode(model_training=True, batchnorm_training=False)
    atk(x01, y)                                                         # warm-up: workspaces, plans, kernels loaded
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            torch.ones(1, device=cuda).item()                           # the mode works on this build
        with atk_call_context(atk):
            adv = atk.forward(x01, y)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert adv.shape == x01.shape and atk.last_radius.shape == (4,)


def test_evaluation_loop_reports_the_radii(cuda, fresh_graphs):
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    from audio_deepfake_adversarial_attacks_amd.datasets.synthetic import SyntheticDetectionDataset
    from audio_deepfake_adversarial_attacks_amd.evaluation import generate_attacks
    cfg = {"data": {"seed": 42}, "checkpoint": {"path": ""},
           "model": {"name": "lcnn", "parameters": {"frontend_algorithm": ["lfcc"], "input_channels": 1}}}
    report_at = (0.00075, 0.0015, 0.003)

    def evaluate(in_flight, method=None, params=None):
        torch.manual_seed(5)
        fresh_graphs.clear()
        made, per_batch = [], []

        def build(model, **kw):
            made.append((method or torchattacks.MinRadiusPGD)(model, **kw))
            return made[0]

        def queued(i):                                        # under the batch's stream: what the attack left for THIS batch
            r = getattr(made[0], "last_radius", None)
            if r is not None:
                per_batch.append(r.clone())

        rep = generate_attacks([None, None, None], cfg, str(cuda), attack_model_config=cfg, attack_method=build,
                               attack_params=params or {"norm": "Linf", "eps_max": 0.003, "search_steps": 3, "steps": 4,
                                                        "report_at": report_at},
                               batch_size=4, dataset=SyntheticDetectionDataset(16), share_weights=True, shuffle=False,
                               num_workers=0, return_scores=True, in_flight=in_flight, on_batch_queued=queued)
        torch.cuda.synchronize()
        return rep, per_batch

    one, batches = evaluate(1)
    keys = ["min_radius/median", "min_radius/p10", "min_radius/p90", "min_radius/unflipped_share",
            "min_radius/already_wrong_share"] + [f"min_radius/robust_acc@{e:g}" for e in report_at]
    assert [k for k in one if k.startswith("min_radius/")] == keys
    radii = one["scores"]["min_radius"]
    assert radii.shape == (16,) and radii.dtype.name == "float32" and one["num_total"] == 16
    assert len(batches) == 4 and same(torch.as_tensor(radii), torch.cat(batches).cpu())          # utterance order
    from audio_deepfake_adversarial_attacks_amd.metrics import radius_summary
    assert {k: one[k] for k in keys} == radius_summary(radii, report_at)
    assert 0.0 <= one["min_radius/robust_acc@0.003"] <= one["min_radius/robust_acc@0.00075"] <= 100.0
    two, _ = evaluate(2)
    assert same(torch.as_tensor(two["scores"]["min_radius"]), torch.as_tensor(radii))
    for k in ("y_pred", "y_pred_label", "y"):
        assert torch.equal(torch.as_tensor(one["scores"][k]), torch.as_tensor(two["scores"][k])), k
    assert {k: two[k] for k in keys} == {k: one[k] for k in keys}
    pgd, _ = evaluate(1, torchattacks.PGD, {"eps": 0.003, "steps": 4})
    assert not [k for k in pgd if k.startswith("min_radius")] and "min_radius" not in pgd["scores"]
