"""GPU: the universal perturbation — universal_colsum against its float64 restatement within the derived bound and
universal_apply against the bits of float32 eager on the CPU, on every shape at which a path changes (tests/universal_cpu_ops.py
derives the bounds); the update of delta is the existing PGD row step, byte for byte; UniversalPGD on LCNN; the loop."""

import numpy as np
import pytest
import torch

from tests import radius_cpu_ops as R
from tests import universal_cpu_ops as C
from tests.test_gpu_apgd import atk_call_context, detector, same
from tests.test_gpu_momentum import padded, untouched

pytestmark = pytest.mark.gpu

U = C.U
G = C.GROUP_ROWS
# one sample; below, at and above the 1024-column tile of the sum and the 4096-sample tile of the broadcast; T % 4 != 0 (sample by
# sample, unaligned later rows) and T % 4 == 0 (16-byte accesses); one row, fewer rows than a group, a whole group, one more (the
# second launch), two groups and a partial third; the production row
SHAPES = [(B, T) for T in (1, 255, 1023, 1025, 4095, 4096, 4097, 4100) for B in (1, 2, 3, G - 1, G, G + 1, 2 * G + 1)] + [(4, 64_600)]
FILL = 3.5


def hip():
    from audio_deepfake_adversarial_attacks_amd import hip_ops
    return hip_ops


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def weights(B, seed):
    """Row weights of both signs with an exact zero in row 0."""
    w = torch.rand(B, generator=torch.Generator().manual_seed(seed)) * 2.0 - 0.5
    w[0] = 0.0
    return w


# ---- the column sum -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("B,T", SHAPES)
def test_colsum_kernel_against_float64(cuda, B, T, weighted):
    """|out - out64| <= (B + 1) u sum_b |w_b g_bt| per column (C.colsum_tolerance: any summation order); a NaN planted in row 0
    — whose weight is 0 in the weighted case: 0 * NaN = NaN — reaches its own column and no other; the guard round `out` is
    untouched; a rerun and a run on a side stream give the same bits."""
    ops = hip()
    g = torch.Generator().manual_seed(7 * B + T)
    grad = torch.randn(B, T, generator=g)
    grad[:, ::11] = 0.0
    col = T // 2
    grad[0, col] = float("nan")
    w = weights(B, B + T) if weighted else None
    grad_d = grad.to(cuda)
    w_d = None if w is None else w.to(cuda)
    buf, out = padded((1, T), FILL, cuda)
    assert ops.universal_colsum(grad_d, w_d, out=out) is out
    torch.cuda.synchronize()
    assert untouched(buf, FILL, T)
    got = out.cpu().double().reshape(-1)
    want, abs_sum = C.universal_colsum_ref64(grad, w, parts=True)
    finite = torch.ones(T, dtype=torch.bool)
    finite[col] = False
    assert torch.isnan(got[col]) and torch.isfinite(got[finite]).all()
    err, tol = (got - want)[finite].abs(), C.colsum_tolerance(B, abs_sum)[finite]
    if finite.any():
        print(f"  B {B} T {T}: max err / tol = {(err / tol.clamp_min(1e-300)).max().item():.3f}")
    assert (err <= tol).all()
    if weighted and B == 1:
        assert (got[finite] == 0).all()                                 # the only row has weight 0
    fresh = ops.universal_colsum(grad_d, w_d)
    assert fresh.shape == (1, T) and same(fresh, out)
    side = torch.cuda.Stream(cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):
        other = ops.universal_colsum(grad_d, w_d)
    side.synchronize()
    assert same(other, out)


def test_colsum_gives_the_same_bits_from_unaligned_rows_and_takes_a_2d_weight(cuda):
    """T % 4 == 0 from a base one float off a 16-byte boundary takes the sample-by-sample path: the same order, the same bits."""
    ops = hip()
    B, T = 2 * G + 1, 4096
    g = torch.Generator().manual_seed(3)
    grad, w = torch.randn(B, T, generator=g), weights(B, 4)
    aligned = ops.universal_colsum(grad.to(cuda), w.to(cuda))
    shifted = torch.empty(B * T + 1, device=cuda)[1:].view(B, T)
    assert shifted.data_ptr() % 16 == 4
    shifted.copy_(grad)
    assert same(ops.universal_colsum(shifted, w.reshape(B, 1).to(cuda)), aligned)
    buf = torch.full((T + 9,), FILL, device=cuda)
    out = buf[5:5 + T]                                                  # an unaligned `out`, and (T,) instead of (1, T)
    ops.universal_colsum(grad.to(cuda), w.to(cuda), out=out)
    assert same(out.reshape(1, T), aligned) and bool((buf[:5] == FILL).all() and (buf[5 + T:] == FILL).all())


def test_wrappers_refuse_bad_arguments(cuda):
    ops = hip()
    x, d, w = torch.zeros(3, 8, device=cuda), torch.zeros(8, device=cuda), torch.zeros(3, device=cuda)
    with pytest.raises(TypeError, match="float32"):
        ops.universal_colsum(x.double())
    with pytest.raises(ValueError, match="one value per row"):
        ops.universal_colsum(x, w[:2])
    with pytest.raises(ValueError, match="one value per column"):
        ops.universal_colsum(x, w, out=torch.zeros(1, 7, device=cuda))
    with pytest.raises(RuntimeError, match="no CPU fallback"):                       # a weight that is not on the device
        ops.universal_colsum(x, torch.zeros(3))
    with pytest.raises(ValueError, match="one value per sample"):
        ops.universal_apply(x, d[:7])
    with pytest.raises(ValueError, match="one value per row"):
        ops.universal_apply(x, d, torch.zeros(4, device=cuda))
    with pytest.raises(ValueError, match="contiguous"):
        ops.universal_apply(x.t(), d)
    assert ops.universal_colsum(torch.zeros(0, 8, device=cuda)).shape == (1, 0)      # B = 0: rows of no samples, nothing launched


# ---- the broadcast ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("alias", [False, True])
@pytest.mark.parametrize("B,T", SHAPES)
def test_apply_kernel_bit_identical_to_float32_eager(cuda, B, T, alias):
    """out == torch.clamp(x + w[:, None] * delta, 0, 1) in float32 on the CPU, bit for bit (both round the product and the sum
    once each), with and without weights, in place and not; a weight-0 row comes back unchanged; the guard is untouched."""
    ops = hip()
    g = torch.Generator().manual_seed(13 * B + T)
    x = torch.rand(B, T, generator=g)
    x[:, ::17] = 0.0
    x[:, 5::19] = 1.0
    delta = torch.randn(T, generator=g) * 0.05                          # large enough to reach both clamps
    delta[::7] = 0.0
    if B > 1:
        x[B - 1, T // 3] = float("nan")
    for w in (None, weights(B, B * T)):
        buf, x_d = padded((B, T), FILL, cuda)
        x_d.copy_(x)
        d_d = delta.to(cuda)
        w_d = None if w is None else w.to(cuda)
        if alias:
            out, obuf = ops.universal_apply(x_d, d_d, w_d, out=x_d), buf
            assert out is x_d
        else:
            obuf, out = padded((B, T), FILL, cuda)
            assert ops.universal_apply(x_d, d_d, w_d, out=out) is out
            assert same(x_d, x)
        torch.cuda.synchronize()
        assert untouched(obuf, FILL, B * T)
        want = C.universal_apply_f32(x, delta, w)
        assert same(out, want)
        finite = ~torch.isnan(want)
        assert torch.equal(bits(out)[finite], bits(want)[finite])
        if w is not None:
            assert same(out[0], x[0])                                   # w_0 = 0: the row itself
    lo_hi = ops.universal_apply(x.to(cuda), delta.to(cuda), None, lo=0.25, hi=0.5)
    assert same(lo_hi, torch.clamp(x + delta.reshape(1, -1), 0.25, 0.5))


# ---- the update of delta is the PGD row step ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("norm,eps", [("Linf", 0.001), ("L2", 0.05)])
def test_delta_update_is_the_row_step_on_a_zero_orig(cuda, norm, eps):
    """UniversalPGD restates nothing: partial_fit's new delta is hip_ops.pgd_linf_step / pgd_l2_step on the (1, T) row, byte for
    byte, with universal_colsum's output as the gradient, a zero row as orig and lo, hi = -eps, eps."""
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    ops = hip()
    B, T = G + 1, 4100
    g = torch.Generator().manual_seed(T)
    model = C.LinearDetector(torch.randn(T, generator=g) * 0.01, torch.zeros(1)).to(cuda)
    x = (torch.rand(B, T, generator=g) * 0.5 + 0.25).to(cuda)
    y = torch.tensor([b % 2 for b in range(B)]).to(cuda)
    sums, steps = [], []

    class Recording:                                                                # hip_ops, with the steps' arguments kept
        def __getattr__(self, name):
            return getattr(ops, name)

        def universal_colsum(self, grad, row_weight=None, out=None):
            sums.append(ops.universal_colsum(grad, row_weight, out=out))
            return sums[-1]

        def pgd_linf_step(self, adv, grad, orig, alpha, eps, lo=0.0, hi=1.0, out=None):
            steps.append(("Linf", adv.clone(), grad.clone(), orig.clone(), (alpha, eps, lo, hi), out))
            return ops.pgd_linf_step(adv, grad, orig, alpha, eps, lo, hi, out=out)

        def pgd_l2_step(self, adv, grad, orig, alpha, eps, eps_div=1e-10, lo=0.0, hi=1.0, out=None):
            steps.append(("L2", adv.clone(), grad.clone(), orig.clone(), (alpha, eps, eps_div, lo, hi), out))
            return ops.pgd_l2_step(adv, grad, orig, alpha, eps, eps_div, lo, hi, out=out)

    atk = torchattacks.UniversalPGD(model, norm=norm, eps=eps, source_label=0)
    atk.ops = Recording()
    for k in range(3):
        atk.partial_fit(x, y)
        kind, delta_in, grad, orig, scalars, out = steps[k]
        assert kind == norm and delta_in.shape == (1, T) and out.data_ptr() == atk.delta.data_ptr()
        assert same(grad, sums[k]) and grad.shape == (1, T) and not bool(orig.any())
        if norm == "Linf":
            assert scalars == (eps / 8, eps, -eps, eps)
            want = ops.pgd_linf_step(delta_in, grad, orig, *scalars)
        else:
            assert scalars == (eps / 4, eps, 1e-10, -eps, eps)
            want = ops.pgd_l2_step(delta_in, grad, orig, *scalars)
        assert torch.equal(bits(atk.delta), bits(want.reshape(-1)))
        assert same(delta_in.reshape(-1), torch.zeros(T)) == (k == 0)               # from zero, then from where it was
    assert atk.fit_steps == 3 and bool(atk.delta.any())


# ---- on the detector --------------------------------------------------------------------------------------------------------------

DETECTOR_SEED = 43


def detector_batch(cuda, model):
    from audio_deepfake_adversarial_attacks_amd.datasets.synthetic import synthetic_waveforms
    x, _ = synthetic_waveforms(4, seed=DETECTOR_SEED)
    x01, mn, mx = hip().to_minmax(x.to(cuda))
    y = torch.tensor([0, 1, 0, 0], device=cuda)
    return x01, y, mn, mx


def fitted(model, batch, **kw):
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    x01, y, mn, mx = batch
    atk = torchattacks.UniversalPGD(model, epochs=2, **kw)
    atk.set_training_mode(model_training=True, batchnorm_training=False)
    atk.fit([(x01, y, mn, mx)])
    return atk


@pytest.mark.parametrize("kw", [{"norm": "Linf", "eps": 0.0005, "source_label": 0},
                                {"norm": "L2", "eps": 0.1},
                                {"norm": "Linf", "eps": 0.001, "source_label": 0, "domain": "waveform"}],
                         ids=["linf_spoof", "l2", "wave_spoof"])
def test_fit_on_lcnn_is_reproducible_and_inside_the_ball(cuda, monkeypatch, kw):
    """Two fits give equal bytes; |delta|_inf <= eps, or ||delta||_2 <= eps (1 + R.norm_rel_bound(T) + 3u): f <= (eps / dn)(1 +
    2u) with dn within norm_rel_bound of ||d||, d f rounds once per sample, and orig = 0 adds no rounding of its own; the clamp
    to [-eps, eps] only shrinks a sample."""
    monkeypatch.setenv("ADVSTEP_ATTACK_GRAPH", "0")
    model = detector("lcnn", cuda)
    batch = detector_batch(cuda, model)
    a, b = fitted(model, batch, **kw), fitted(model, batch, **kw)
    assert a.fit_steps == 2 and a.delta.shape == (batch[0].shape[1],) and a.delta.is_cuda
    assert torch.equal(bits(a.delta), bits(b.delta)) and bool(a.delta.any())
    d = a.delta.cpu().double()
    T = d.numel()
    eps32 = float(np.float32(kw["eps"]))
    if kw["norm"] == "Linf":
        assert d.abs().max().item() <= eps32
    else:
        print(f"  ||delta|| / eps - 1 = {d.norm().item() / eps32 - 1:.3e}, bound {R.norm_rel_bound(T) + 3 * U:.3e}")
        assert d.norm().item() <= eps32 * (1 + R.norm_rel_bound(T) + 3 * U)
        assert d.abs().max().item() <= eps32


def test_forward_makes_no_host_read_and_no_model_call(cuda, monkeypatch):
    monkeypatch.setenv("ADVSTEP_ATTACK_GRAPH", "0")
    model = detector("lcnn", cuda)
    x01, y, mn, mx = detector_batch(cuda, model)
    atk = fitted(model, (x01, y, mn, mx), norm="Linf", eps=0.001, source_label=0, domain="waveform")
    atk.set_minmax(mn, mx)
    warm = atk(x01, y)                                                  # warm-up: kernels loaded
    torch.cuda.synchronize()
    calls = []
    hook = model.register_forward_pre_hook(lambda *a: calls.append(1))
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
        hook.remove()
    assert calls == [] and atk._minmax is None and atk.fit_steps == 2
    assert torch.equal(adv, warm) and torch.equal(adv[1], x01[1]) and not torch.equal(adv[0], x01[0])
    w = (y == 0).float() / (mx - mn).reshape(-1)
    assert same(adv, C.universal_apply_f32(x01, atk.delta, w))


# ---- through the loop --------------------------------------------------------------------------------------------------------------

CFG = {"data": {"seed": 42}, "checkpoint": {"path": ""},
       "model": {"name": "lcnn", "parameters": {"frontend_algorithm": ["lfcc"], "input_channels": 1}}}
KEYS = ["universal/fit_utterances", "universal/heldout_utterances", "universal/accuracy_fit", "universal/accuracy_heldout",
        "universal/source_flipped_fit", "universal/source_flipped_heldout", "universal/delta_linf", "universal/delta_l2"]


@pytest.mark.parametrize("member", ["UAP_SPOOF", "UAP_WAVE_SPOOF"])
def test_loop_fits_on_the_first_batch_and_applies_to_all(cuda, tmp_path, monkeypatch, member):
    """generate_attacks with the enum member over 8 synthetic utterances, batch 4, universal_fit = 1: the universal/* keys, one
    and two lanes with the same bits, and save -> load reproducing the scores with no fit step.  How many utterances flip is not
    asserted.

    For the waveform member every utterance's reported linf <= eps (1 + 5u) + u (3 range + A), range = fl(mx - mn), A = max(|mn|,
    |mx|) — the per-sample form of the way back of test_gpu_snr.waveform_bounds.  The attack moves a source row by delta01 =
    fl(fl(1 / range) delta_t), |delta01| <= (eps / range)(1 + 2u), which is eps (1 + 2u) once multiplied by range again.  Around
    it, in the waveform's units: fl(x - mn) errs by <= u range; x01 = fl(. / range) lies in [0, 1], where float32's grid is u, so
    the division errs by <= u / 2, i.e. range u / 2; adv01 = fl(x01 + delta01) likewise by range u / 2 (a sum above 1 is clamped
    towards x01); fl(adv01 range) by <= u range; the addition of mn by <= u A.  That is u (3 range + A), also for the rows the
    attack does not move.  The report's d = fl(adv_w - x) rounds once more: (1 + u) on everything, inside eps (1 + 5u)."""
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    from audio_deepfake_adversarial_attacks_amd.aa.aa_types import AttackEnum
    from audio_deepfake_adversarial_attacks_amd.datasets.synthetic import SyntheticDetectionDataset
    from audio_deepfake_adversarial_attacks_amd.evaluation import generate_attacks
    method, params = AttackEnum[member].value
    wave = member == "UAP_WAVE_SPOOF"
    data = SyntheticDetectionDataset(8)
    fit_calls = []
    real_fit = torchattacks.UniversalPGD.partial_fit
    monkeypatch.setattr(torchattacks.UniversalPGD, "partial_fit", lambda self, *a: (fit_calls.append(1), real_fit(self, *a))[1])

    def evaluate(in_flight, **kw):
        torch.manual_seed(5)
        fit_calls.clear()
        rep = generate_attacks([None, None, None], CFG, str(cuda), attack_model_config=CFG, attack_method=method,
                               attack_params=params, batch_size=4, dataset=data, share_weights=True, shuffle=False,
                               num_workers=0, return_scores=True, in_flight=in_flight, perturbation_stats=wave, **kw)
        torch.cuda.synchronize()
        return rep, len(fit_calls)

    path = tmp_path / "uap.npz"
    one, n_fit = evaluate(1, universal_fit=1, universal_save=path)
    assert n_fit == 5                                                   # epochs x one batch
    assert [k for k in one if k.startswith("universal/")] == KEYS
    assert one["universal/fit_utterances"] == 4 and one["universal/heldout_utterances"] == 4 and one["num_total"] == 8
    delta = one["scores"]["universal_delta"]
    eps32 = float(np.float32(params["eps"]))
    assert delta.dtype == np.float32 and delta.shape == (data.x.shape[1],)
    assert one["universal/delta_linf"] == float(np.abs(delta).max()) <= eps32
    if (data.y[:4] == 0).any():                                         # a spoof row in the fitted batch: the fit moved delta
        assert one["universal/delta_linf"] > 0
    for k in ("accuracy_fit", "accuracy_heldout"):
        assert 0.0 <= one["universal/" + k] <= 100.0
    if wave:
        x = data.x.double()
        mn, mx = data.x.min(dim=1).values, data.x.max(dim=1).values
        rng, A = (mx - mn).double(), torch.maximum(mn.abs(), mx.abs()).double()
        bound = eps32 * (1 + 5 * U) + U * (3 * rng + A)
        linf = torch.as_tensor(one["scores"]["perturbation"]["linf"]).double()
        print("  linf :", linf.tolist(), "\n  bound:", bound.tolist())
        assert x.shape[0] == 8 and (linf <= bound).all()
    two, n_fit = evaluate(2, universal_fit=1)
    assert n_fit == 5
    loaded, n_fit = evaluate(1, universal_load=path)
    assert n_fit == 0                                                   # zero fit steps
    assert loaded["universal/fit_utterances"] == 0 and loaded["universal/heldout_utterances"] == 8
    for rep in (two, loaded):
        assert np.array_equal(rep["scores"]["universal_delta"].view(np.int32), delta.view(np.int32))
        for k in ("y_pred", "y_pred_label", "y"):
            assert np.array_equal(rep["scores"][k], one["scores"][k]), k
        assert np.array_equal(rep["scores"]["y_pred"].view(np.int32), one["scores"]["y_pred"].view(np.int32))


def test_loop_refuses_the_keywords_for_another_attack(cuda):
    from audio_deepfake_adversarial_attacks_amd.aa.aa_types import AttackEnum
    from audio_deepfake_adversarial_attacks_amd.datasets.synthetic import SyntheticDetectionDataset
    from audio_deepfake_adversarial_attacks_amd.evaluation import generate_attacks
    method, params = AttackEnum["FGSM"].value
    with pytest.raises(ValueError, match="need a universal attack"):
        generate_attacks([None, None, None], CFG, str(cuda), attack_model_config=CFG, attack_method=method, attack_params=params,
                         batch_size=4, dataset=SyntheticDetectionDataset(4), share_weights=True, shuffle=False, num_workers=0,
                         universal_fit=1)
