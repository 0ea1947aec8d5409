"""`-m gpu`: the SNR-budget kernels (include/advstep_snr.h) against the float64 restatement tests/snr_cpu_ops.py, the budget
recomputed from their outputs, PGDSNR on the detector, hipGraph replay, host reads and the evaluation loop.

Every bound is DERIVED (tests/snr_cpu_ops.py's docstring has the derivation, DESIGN.md section 4v repeats it); u = 2^-24:
    step          |out - out64| <= (32 M_t + 25 ||M||_seg) u,  M_t = |adv_t| + |a g_t / gn| + |x_t|        (C.step_tolerance)
    budget        ||out - x||_seg <= r64 (1 + (16 + sqrt(n)) u) + u sqrt(n)                                (C.seg_ball_bound)
    global radii  |e - e64| <= ((chain(T) + 3) / 2 + 2) u e64                                              (C.radius_rel_bound)
No constant here was measured.

The loop's slack (test_loop_meets_the_budget_in_the_waveform_domain) is derived per row in `waveform_bounds`."""
import math

import numpy as np
import pytest
import torch

from tests import radius_cpu_ops as R
from tests import snr_cpu_ops as C
from tests.test_gpu_apgd import atk_call_context, detector, same
from tests.test_gpu_momentum import padded, untouched

pytestmark = pytest.mark.gpu

U = C.U
STEP_SHAPES = [(B, T) for T in (1, 255, 256, 257, 1023, 1025, 4095, 4096, 4097, 4100) for B in (1, 3)] + [(2, 64_600)]
RHO = C.rho_of(30.0)
OFFSET = -0.25                                               # exact in float32: x = 0.25 is silent under it


def hip():
    from audio_deepfake_adversarial_attacks_amd import hip_ops
    return hip_ops


def step_inputs(B, T, with_offset, seed):
    """orig in [0, 1] with exact 0s and 1s, adv mostly OUTSIDE its segments' balls (f < 1), and by segment index, where the row
    has it: 1 a zero gradient, 2 silence (x + c = 0 throughout) under a moved adv, 3 d = 0 (no gradient, adv = orig), 4 an adv
    just beside orig (inside the ball: f = 1).  B > 1: one NaN in row 1's gradient, in its last segment (the planted segments are
    checked on row 0)."""
    g = torch.Generator().manual_seed(seed)
    orig = torch.rand(B, T, generator=g)
    orig[:, ::17] = 0.0
    orig[:, 5::19] = 1.0
    c = torch.tensor([OFFSET, 0.125, -0.5][:B]) if with_offset else None
    grad = torch.randn(B, T, generator=g) * 1e-3
    grad[:, ::13] = 0.0
    adv = (orig + (torch.rand(B, T, generator=g) * 2 - 1) * 0.05).clamp(0, 1)
    S = -(-T // 256)
    seg = lambda s: slice(256 * s, min(256 * s + 256, T))    # noqa: E731
    planted = []
    if S > 1:
        grad[:, seg(1)] = 0.0
        planted.append("zero_grad")
    if S > 2:
        orig[0, seg(2)] = -OFFSET if with_offset else 0.0
        planted.append("silent")
    if S > 3:
        grad[:, seg(3)] = 0.0
        adv[:, seg(3)] = orig[:, seg(3)]
        planted.append("d_zero")
    if S > 4:
        adv[:, seg(4)] = (orig[:, seg(4)] + 1e-4).clamp(0, 1)
        planted.append("inside")
    if B > 1:
        grad[1, T - 1] = float("nan")
    return adv, grad, orig, c, planted, seg


@pytest.mark.parametrize("B,T", STEP_SHAPES)
@pytest.mark.parametrize("alias,with_offset", [(False, False), (True, False), (False, True), (True, True)])
def test_seg_step_kernel_against_float64(cuda, B, T, alias, with_offset):
    """The step within (32 M_t + 25 ||M||_seg) u of the float64 restatement, per sample (first order in u = 2^-24; every
    operation is correctly rounded, segment sums are 2 + 6 additions deep: tests/snr_cpu_ops.py), and every segment's budget
    recomputed in float64 from the float32 output: ||out - x||_seg <= r64 (1 + (16 + sqrt(n)) u) + u sqrt(n), which is
    sum (out - x)^2 <= rho^2 sum (x + c)^2 (1 + k u) with k = 2 (16 + sqrt(n) (1 + 1 / r64))."""
    ops = hip()
    adv, grad, orig, c, planted, seg = step_inputs(B, T, with_offset, seed=3000 + 7 * B + T)
    alpha_rel, eps_div = 0.25, 1e-10
    want, M, Mn, r = C.seg_pgd_step_ref64(adv, grad, orig, c, RHO, alpha_rel, eps_div, parts=True)
    if T >= 4095:
        assert planted == ["zero_grad", "silent", "d_zero", "inside"]
    c_dev = None if c is None else c.to(cuda)

    def launch():
        obuf, o_dev = padded((B, T), -7.25, cuda)
        adv_dev = adv.to(cuda)
        if alias:
            o_dev.copy_(adv)
            adv_dev = o_dev
        out = ops.seg_pgd_step(adv_dev, grad.to(cuda), orig.to(cuda), c_dev, RHO, alpha_rel, eps_div, out=o_dev)
        torch.cuda.synchronize()
        assert out.data_ptr() == o_dev.data_ptr() and untouched(obuf, -7.25, B * T)
        return out.cpu()

    got = launch()
    assert same(got, launch())                                                      # reruns are bit-identical
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan)                                       # NaN exactly where the restatement has it
    if B > 1:
        last = torch.zeros_like(nan)
        last[1, seg(-(-T // 256) - 1)] = True
        assert torch.equal(nan, last)                                               # the NaN's own segment, no neighbour, no other row
    else:
        assert not nan.any()
    err = (got.double() - want).abs()
    tol = C.step_tolerance(M, Mn)
    ok = ~nan
    print(f"  max err / tol = {(err[ok] / tol[ok].clamp_min(1e-300)).max().item():.3f}")
    assert (err[ok] <= tol[ok]).all()
    # the budget, from the float32 output
    d = torch.where(nan, torch.zeros_like(want), got.double() - orig.double())
    dn = (C.segments(d) ** 2).sum(-1).sqrt()
    n = C.segment_sizes(T)
    bound = C.seg_ball_bound(r, n)
    clean = ~C.segments(nan.double()).sum(-1).bool()
    print(f"  max ||out - x|| / bound = {(dn[clean] / bound[clean].clamp_min(1e-300)).max().item():.6f}")
    assert (dn[clean] <= bound[clean]).all()
    assert got[ok].min() >= 0 and got[ok].max() <= 1
    if "silent" in planted:
        assert r[0, 2] == 0 and same(got[0, seg(2)], orig[0, seg(2)]) and not same(adv[0, seg(2)], orig[0, seg(2)])
    if "d_zero" in planted:
        assert same(got[0, seg(3)], orig[0, seg(3)])
    if "inside" in planted:                                                         # f = 1 there (the step as taken), f < 1 in segment 0
        assert 0 < dn[0, 4] < 0.5 * r[0, 4] and dn[0, 0] > 0.9 * r[0, 0]


def test_seg_step_takes_a_2d_offset_and_refuses_bad_arguments(cuda):
    ops = hip()
    adv, grad, orig, c, _, _ = step_inputs(3, 1025, True, seed=1)
    a, g, x = adv.to(cuda), grad.to(cuda), orig.to(cuda)
    want = ops.seg_pgd_step(a, g, x, c.to(cuda), RHO, 0.25, 1e-10)
    assert same(ops.seg_pgd_step(a, g, x, c.to(cuda).reshape(3, 1), RHO, 0.25, 1e-10), want)
    with pytest.raises(ValueError, match="one value per row"):
        ops.seg_pgd_step(a, g, x, c.to(cuda)[:2].contiguous(), RHO, 0.25, 1e-10)
    with pytest.raises(ValueError, match="rho"):
        ops.seg_pgd_step(a, g, x, None, float("nan"), 0.25, 1e-10)
    with pytest.raises(ValueError, match="rho"):
        ops.snr_row_radius(x, None, -1.0)
    assert ops.seg_pgd_step(a[:0], g[:0], x[:0], None, RHO, 0.25, 1e-10).shape == (0, 1025)
    assert ops.snr_row_radius(x[:0], None, RHO).shape == (0,)


# ---- the global budget's radii ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,T", STEP_SHAPES)
@pytest.mark.parametrize("with_offset", [False, True])
def test_row_radius_kernel(cuda, B, T, with_offset):
    """|e - e64| <= ((chain(T) + 3) / 2 + 2) u e64: the squares of x + c carry 3u, the chain adds chain(T) times, the square
    root halves and rounds, the product by rho rounds.  Bit-identical on a side stream."""
    ops = hip()
    _, _, orig, c, _, _ = step_inputs(B, T, with_offset, seed=3100 + 7 * B + T)
    if B > 1:
        orig[1] = -c[1] if with_offset else 0.0                                     # a silent row: radius 0
    want = C.snr_row_radius_ref64(orig, c, RHO)
    c_dev = None if c is None else c.to(cuda)
    ebuf, e_dev = padded((B,), 9.5, cuda, pad=64)
    got = ops.snr_row_radius(orig.to(cuda), c_dev, RHO, out=e_dev)
    torch.cuda.synchronize()
    assert got.data_ptr() == e_dev.data_ptr() and untouched(ebuf, 9.5, B, pad=64)
    err = (got.cpu().double() - want).abs()
    print(f"  max err / bound = {(err / (C.radius_rel_bound(T) * want).clamp_min(1e-300)).max().item():.3f} (n = {C.chain(T)})")
    assert (err <= C.radius_rel_bound(T) * want).all()
    if B > 1:
        assert got[1] == 0
    side = torch.cuda.Stream(device=cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):
        again = ops.snr_row_radius(orig.to(cuda), c_dev, RHO)
    side.synchronize()
    assert same(again, got)


@pytest.mark.parametrize("B,T", [(3, 4097), (3, 4100), (2, 64_600)])
def test_global_step_is_the_row_l2_step_at_these_radii(cuda, B, T, monkeypatch):
    """PGDSNR's global mode restates nothing: one step of it from `adv` is hip_ops.row_pgd_l2_step at snr_row_radius' radii
    with alpha_abs = 0, byte for byte."""
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    monkeypatch.setenv("ADVSTEP_ATTACK_GRAPH", "0")
    ops = hip()
    g = torch.Generator().manual_seed(B + T)
    w = torch.randn(T, generator=g) * 0.01
    model = C.LinearDetector(w, torch.zeros(1)).to(cuda)
    x = (torch.rand(B, T, generator=g) * 0.5 + 0.25).to(cuda)
    y = torch.randint(0, 2, (B,), generator=g).to(cuda)
    mn = -torch.rand(B, 1, generator=g).to(cuda)
    mx = torch.rand(B, 1, generator=g).to(cuda) + 0.5
    calls = []

    class Recording:                                                                # hip_ops, with the step's arguments kept
        def __getattr__(self, name):
            return getattr(ops, name)

        def row_pgd_l2_step(self, adv, grad, orig, eps_rows, alpha_abs, alpha_rel, eps_div, out=None):
            calls.append((adv.clone(), grad.clone(), orig.clone(), eps_rows.clone(), alpha_abs, alpha_rel, eps_div))
            return ops.row_pgd_l2_step(adv, grad, orig, eps_rows, alpha_abs, alpha_rel, eps_div, out=out)

    atk = torchattacks.PGDSNR(model, snr_db=30.0, segmental=False, steps=2, rel_alpha=0.6)
    atk.ops = Recording()
    atk.set_minmax(mn, mx)
    got = atk(x, y)
    c = (mn / (mx - mn)).reshape(-1).contiguous()
    e = ops.snr_row_radius(x, c, atk.rho)
    assert len(calls) == 2
    for adv_in, grad, orig, eps_rows, alpha_abs, alpha_rel, eps_div in calls:
        assert same(eps_rows, e) and same(orig, x) and (alpha_abs, alpha_rel, eps_div) == (0.0, 0.6, 1e-10)
    adv_in, grad = calls[1][:2]
    want = ops.row_pgd_l2_step(adv_in, grad, x, e, 0.0, 0.6, 1e-10)
    assert same(got, want) and not same(got, x) and not same(adv_in, x)
    rel = ((e.cpu().double() - C.snr_row_radius_ref64(x, c, atk.rho)).abs() / C.snr_row_radius_ref64(x, c, atk.rho)).max().item()
    assert rel <= C.radius_rel_bound(T)


# ---- on the detector: graph replay, host reads -------------------------------------------------------------------------------------

DETECTOR_SEED = 41


def detector_batch(cuda, model, seed=DETECTOR_SEED):
    from audio_deepfake_adversarial_attacks_amd.datasets.synthetic import synthetic_waveforms
    x, _ = synthetic_waveforms(4, seed=seed)
    x01, mn, mx = hip().to_minmax(x.to(cuda))
    with torch.no_grad():
        y = (model(x01).reshape(-1) > 0).long()
    return x01, y, mn, mx


@pytest.fixture()
def fresh_graphs():
    from audio_deepfake_adversarial_attacks_amd.torchattacks import graphed
    graphed.clear()
    yield graphed
    graphed.clear()


@pytest.mark.parametrize("segmental", [True, False])
def test_graph_replay_is_bit_identical(cuda, fresh_graphs, monkeypatch, segmental):
    """ADVSTEP_ATTACK_GRAPH = 0, 1 and fused give the same bytes.  The offsets (and the global radii) are device data of the
    call, so in the split form ONE capture of the model part serves calls with different mn / mx; the fused form would bake
    one call's into its graph: the attack stays eager under it."""
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    model = detector("lcnn", cuda)
    x01, y, mn, mx = detector_batch(cuda, model)
    other = (mn * 0.5 - 0.01, mx * 2.0)                                             # another pair: other offsets, other radii

    def make():
        atk = torchattacks.PGDSNR(model, snr_db=30.0, segmental=segmental, steps=4)
        atk.set_training_mode(model_training=True, batchnorm_training=False)
        return atk

    def run(atk, pair):
        atk.set_minmax(*pair)
        return atk(x01, y)

    atk = make()
    monkeypatch.setenv("ADVSTEP_ATTACK_GRAPH", "0")
    want = [run(atk, (mn, mx)), run(atk, other)]
    assert len(fresh_graphs._GRAPHS) == 0 and not torch.equal(want[0], want[1]) and not torch.equal(want[0], x01)
    monkeypatch.setenv("ADVSTEP_ATTACK_GRAPH", "1")
    for call in range(3):
        for pair, w in zip(((mn, mx), other), want):
            assert torch.equal(run(atk, pair), w), call
    assert len(fresh_graphs._GRAPHS) == 1                                           # one capture served both pairs
    assert torch.equal(run(make(), other), want[1]) and len(fresh_graphs._GRAPHS) == 1
    monkeypatch.setenv("ADVSTEP_ATTACK_GRAPH", "fused")
    for pair, w in zip(((mn, mx), other, (mn, mx)), want + want[:1]):
        assert torch.equal(run(make(), pair), w)
    assert len(fresh_graphs._GRAPHS) == 1                                           # no fused capture was added


@pytest.mark.parametrize("segmental", [True, False])
def test_forward_makes_no_host_read(cuda, monkeypatch, segmental):
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    monkeypatch.setenv("ADVSTEP_ATTACK_GRAPH", "0")
    model = detector("lcnn", cuda)
    x01, y, mn, mx = detector_batch(cuda, model)
    atk = torchattacks.PGDSNR(model, snr_db=30.0, segmental=segmental, steps=4)
    atk.set_training_mode(model_training=True, batchnorm_training=False)
    atk.set_minmax(mn, mx)
    atk(x01, y)                                                         # warm-up: workspaces, plans, kernels loaded
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            torch.ones(1, device=cuda).item()                           # the mode works on this build
        atk.set_minmax(mn, mx)
        with atk_call_context(atk):
            adv = atk.forward(x01, y)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert adv.shape == x01.shape and atk._minmax is None


# ---- through the loop --------------------------------------------------------------------------------------------------------------

CFG = {"data": {"seed": 42}, "checkpoint": {"path": ""},
       "model": {"name": "lcnn", "parameters": {"frontend_algorithm": ["lfcc"], "input_channels": 1}}}
K_DB = 10.0 / math.log(10.0)
LOG10F_DB = 6.8e-6                                           # DESIGN 4q's allowance for the report's log10f stage


def waveform_bounds(x, segmental, snr_db):
    """Per row of the float32 batch `x` (N, T), in float64: lower bounds on the report's snr_db and seg_snr_db after PGDSNR at
    `snr_db`, from the row's mn, mx, T and budget alone.  With range = fl(mx - mn), A = max(|mn|, |mx|), and over a set of n
    samples whose signal norm is X (a segment, or the row):

      the budget in the attack's domain.  x01 = fl(fl(x - mn) / range) and c = fl(mn / range) give range (x01 + c) = x +
        (x - mn)(e3 + e4) + mn e5, |e| <= u: range ||x01 + c|| <= X + u (2 range + A) sqrt(n), so the radius is
        r <= fl(rho) (X + u (2 range + A) sqrt(n)) / range, and the kernels leave ||delta01|| <= ball(r): C.seg_ball_bound(r, n)
        per segment; R.l2_ball_bound(e, T) with e <= r (1 + C.radius_rel_bound(T)) for the row.
      the way back.  adv_w = fl(fl(adv01 range) + mn) = x + delta01 range (1 + e1) + (x - mn)(e1 + e3 + e4) + e2 (<= A) — the
        samples the attack did not move are not returned bit-exactly — and the report's d = fl(adv_w - x):
        ||d|| <= range ball (1 + 3u) + u (3 range + A) sqrt(n).
      the report.  Its sums and log10f: K (2 (chain(T) + 1) + 1) u + 6.8e-6 dB on snr_db; K 19 u + 6.8e-6 dB on a segment's term
        and (17 + ceil(C / 256) + 1) u 35 dB on their mean.

    snr_db >= 20 log10(X / ||d||bound) - its error; seg_snr_db >= the mean over the FULL segments of that figure clamped to
    [-10, 35] - its error.  For the segmental attack the row's ||d||^2 bound is the sum of its segments' (the partial one
    included)."""
    x = x.double()
    N, T = x.shape
    rho32 = C._f32(C.rho_of(snr_db))
    mn, mx = x.min(dim=1).values, x.max(dim=1).values
    rng = (mx.float() - mn.float()).double()
    A = torch.maximum(mn.abs(), mx.abs())

    def back(X, n, ball):
        r = rho32 * (X + U * (2 * rng.reshape(-1, 1) + A.reshape(-1, 1)) * n ** 0.5) / rng.reshape(-1, 1)
        return rng.reshape(-1, 1) * ball(r) * (1 + 3 * U) + U * (3 * rng.reshape(-1, 1) + A.reshape(-1, 1)) * n ** 0.5

    Xrow = x.norm(dim=1, keepdim=True)
    n_seg = C.segment_sizes(T).reshape(1, -1)
    Xseg = (C.segments(x) ** 2).sum(-1).sqrt()
    if segmental:
        dseg = back(Xseg, n_seg, lambda r: C.seg_ball_bound(r, n_seg))
        drow = (dseg ** 2).sum(-1, keepdim=True).sqrt()
    else:
        drow = back(Xrow, torch.tensor(float(T), dtype=torch.float64),
                    lambda r: r * (1 + C.radius_rel_bound(T)) * (1 + R.norm_rel_bound(T) + 3 * U) + U * math.sqrt(T))
    snr_lb = 20 * torch.log10(Xrow / drow).reshape(-1) - (K_DB * (2 * (R.chain(T) + 1) + 1) * U + LOG10F_DB)
    seg_lb = None
    if segmental:
        S = T // 256
        term = (20 * torch.log10(Xseg[:, :S] / dseg[:, :S]) - (K_DB * 19 * U + LOG10F_DB)).clamp(-10.0, 35.0)
        seg_lb = term.mean(dim=1) - (17 + math.ceil(math.ceil(T / 4096) / 256) + 1) * U * 35.0
    return snr_lb, seg_lb


@pytest.mark.parametrize("member", ["PGDSEGSNR_30dB", "PGDSNR_30dB"])
def test_loop_meets_the_budget_in_the_waveform_domain(cuda, fresh_graphs, member):
    """generate_attacks with the enum member over 8 synthetic utterances, perturbation_stats on, one and two lanes: every
    utterance's snr_db >= 30 - slack and, for the segmental member, seg_snr_db >= 30 - slack, slack derived per row in
    `waveform_bounds` (float32 rounding only: the kernel's k u and the min-max round trip).  One-sided: how many utterances
    flip is not asserted."""
    from audio_deepfake_adversarial_attacks_amd.aa.aa_types import AttackEnum
    from audio_deepfake_adversarial_attacks_amd.datasets.synthetic import SyntheticDetectionDataset
    from audio_deepfake_adversarial_attacks_amd.evaluation import generate_attacks
    method, params = AttackEnum[member].value
    segmental = params["segmental"]

    def evaluate(in_flight):
        torch.manual_seed(5)
        fresh_graphs.clear()
        pairs = []

        def keep(batch_x, batch_x_attacked, **_):
            pairs.append((batch_x.cpu(), batch_x_attacked.cpu()))

        rep = generate_attacks([None, None, None], CFG, str(cuda), attack_model_config=CFG, attack_method=method,
                               attack_params=params, batch_size=4, dataset=SyntheticDetectionDataset(8), share_weights=True,
                               shuffle=False, num_workers=0, return_scores=True, in_flight=in_flight, perturbation_stats=True,
                               on_attack_end_callback=keep)
        torch.cuda.synchronize()
        return rep, pairs

    one, pairs = evaluate(1)
    x = torch.cat([p[0] for p in pairs]).reshape(8, -1)
    adv = torch.cat([p[1] for p in pairs]).reshape(8, -1)
    planes = one["scores"]["perturbation"]
    snr_lb, seg_lb = waveform_bounds(x, segmental, 30.0)
    snr, seg = torch.as_tensor(planes["snr_db"]).double(), torch.as_tensor(planes["seg_snr_db"]).double()
    print("  snr_db      :", snr.tolist(), "\n  30 - slack  :", snr_lb.tolist())
    assert not torch.equal(adv, x) and torch.isfinite(snr).all()
    assert (snr_lb > 29.9).all() and (snr >= snr_lb).all()                          # the slack is rounding, not a loophole
    if segmental:
        print("  seg_snr_db  :", seg.tolist(), "\n  30 - slack  :", seg_lb.tolist())
        assert (seg >= seg_lb).all()
    two, _ = evaluate(2)
    for k in ("snr_db", "seg_snr_db", "l2"):
        assert np.array_equal(planes[k].view(np.int32), two["scores"]["perturbation"][k].view(np.int32)), k
