"""GPU: the universal adversarial filter — filter_apply against the BYTES of its float32 twin and the values of the channel's K = 1
forward, filter_tap_grad + the fold against the float64 twin within the derived bound (tests/filter_cpu_ops.py derives it),
filter_tap_update against the float64 Adam twin, on every shape at which a path changes; UniversalFilter on a linear detector
whose outcome was computed beforehand in float64; the loop."""
import numpy as np
import pytest
import torch

from tests import filter_cpu_ops as C
from tests.test_gpu_apgd import hip, same

pytestmark = pytest.mark.gpu

U = C.U
FILL = 3.5
PAD = 1024
SHAPES = C.shapes()


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def off_padded(shape, fill, cuda):
    """(buffer, view): `shape` floats one float off a 16-byte boundary, with PAD guard floats of `fill` on either side."""
    n = int(np.prod(shape))
    buf = torch.full((PAD + 1 + n + PAD,), fill, device=cuda)
    view = buf[PAD + 1:PAD + 1 + n].view(shape)
    assert view.data_ptr() % 16 == 4
    return buf, view


def untouched(buf, fill, n):
    return bool((buf[:PAD + 1] == fill).all() and (buf[PAD + 1 + n:] == fill).all())


def off(t, cuda):
    """A copy of `t` on the device, one float off a 16-byte boundary."""
    _, view = off_padded(tuple(t.shape), FILL, cuda)
    view.copy_(t)
    return view


def on_side_stream(cuda, fn):
    side = torch.cuda.Stream(cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):
        res = fn()
    side.synchronize()
    return res


# ---- filter_apply ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,T,L", SHAPES)
def test_apply_kernel_is_the_float32_twin_bit_for_bit(cuda, B, T, L):
    """out == the numpy float32 restatement in the ABI's order, bit for bit, with and without a row mask, from bases one float off
    16-byte alignment; a masked row is x's bits; the guard round `out` is untouched; a rerun, a run on a side stream and a run in
    place (`out` is `x`) give the same bits; for L <= 255 the values are those of clamp(channel_apply(K = 1, the taps replicated
    per row, shift = -P, gain 1, noise 0)).  Some samples clip at either end."""
    ops = hip()
    x, center, taps, mask, _ = C.case(B, T, L)
    x_d, c_d, h_d = off(x, cuda), off(center, cuda), off(taps, cuda)
    for m in (None, mask):
        m_d = None if m is None else off(m, cuda)
        want = torch.from_numpy(C.filter_apply_np(x, center, taps, m))
        if T >= 255:
            assert bool((want[0] == 0).any()) and bool((want[0] == 1).any())
        buf, out = off_padded((B, T), FILL, cuda)
        assert ops.filter_apply(x_d, c_d, h_d, m_d, out=out) is out
        torch.cuda.synchronize()
        assert untouched(buf, FILL, B * T) and same(x_d, x)
        assert torch.equal(bits(out), bits(want))
        if m is not None:
            for b in range(1, B, 2):
                assert torch.equal(bits(out[b]), bits(x[b]))                        # the masked row: x's bits
        fresh = ops.filter_apply(x_d, c_d, h_d, m_d)
        assert torch.equal(bits(fresh), bits(want))
        other = on_side_stream(cuda, lambda: ops.filter_apply(x_d, c_d, h_d, m_d))
        assert torch.equal(bits(other), bits(want))
        abuf, alias = off_padded((B, T), FILL, cuda)
        alias.copy_(x)
        assert ops.filter_apply(alias, c_d, h_d, m_d, out=alias) is alias
        torch.cuda.synchronize()
        assert untouched(abuf, FILL, B * T) and torch.equal(bits(alias), bits(want))
    if L <= 255:
        P = (L - 1) // 2
        through = ops.channel_apply(x_d, c_d, h_d.reshape(1, 1, L).repeat(1, B, 1).contiguous(),
                                    torch.full((1, B), -P, dtype=torch.int32, device=cuda), torch.ones(1, B, device=cuda),
                                    torch.zeros(1, B, device=cuda), seed=1)
        assert torch.equal(torch.clamp(through[0], 0.0, 1.0), ops.filter_apply(x_d, c_d, h_d))
    lo_hi = ops.filter_apply(x_d, c_d, h_d, None, lo=0.25, hi=0.5)
    assert torch.equal(bits(lo_hi), bits(torch.from_numpy(C.filter_apply_np(x, center, taps, None, 0.25, 0.5))))


def test_wrappers_refuse_bad_arguments(cuda):
    ops = hip()
    x, c, h = torch.zeros(3, 8, device=cuda), torch.zeros(3, device=cuda), torch.zeros(5, device=cuda)
    with pytest.raises(TypeError, match="float32"):
        ops.filter_apply(x.double(), c, h)
    with pytest.raises(ValueError, match="one value per row"):
        ops.filter_apply(x, c[:2], h)
    with pytest.raises(ValueError, match="one value per row"):
        ops.filter_apply(x, c, h, torch.zeros(4, device=cuda))
    with pytest.raises(ValueError, match="contiguous"):
        ops.filter_apply(x.t(), c, h)
    with pytest.raises(RuntimeError, match="no CPU fallback"):                       # taps that are not on the device
        ops.filter_apply(x, c, torch.zeros(5))
    for bad in (4, 0, 1027):
        with pytest.raises(ValueError, match="odd number of taps"):
            ops.filter_apply(x, c, torch.zeros(bad, device=cuda))
        with pytest.raises(ValueError, match="odd number of taps"):
            ops.filter_tap_grad(x, c, x, x, bad)
    with pytest.raises(ValueError, match=r"grad must hold \(3, 8\)"):
        ops.filter_tap_grad(x, c, x[:2], x, 5)
    with pytest.raises(ValueError, match="one value per tap"):
        ops.filter_tap_update(h, h[:3].clone(), h.clone(), 3, 8, 1, 0.02)
    with pytest.raises(ValueError, match="1-based"):
        ops.filter_tap_update(h, h.clone(), h.clone(), 3, 8, 0, 0.02)
    assert ops.filter_apply(torch.zeros(0, 8, device=cuda), torch.zeros(0, device=cuda), h).shape == (0, 8)


# ---- the tap gradient ---------------------------------------------------------------------------------------------------------------

def device_gradient(ops, cuda, x_d, c_d, m_d, g_d, y_d, L, lr=0.02):
    """(dh, taps after one Adam step from zero taps and moments) of one filter_tap_grad + filter_tap_update; dh sits in a guarded,
    unaligned buffer whose guard is checked."""
    B, T = x_d.shape
    buf, dh = off_padded((L,), FILL, cuda)
    h, m, v = off(torch.zeros(L), cuda), off(torch.zeros(L), cuda), off(torch.zeros(L), cuda)
    ops.filter_tap_grad(x_d, c_d, g_d, y_d, L, m_d)
    assert ops.filter_tap_update(h, m, v, B, T, 1, lr, dh_out=dh) is dh
    torch.cuda.synchronize()
    assert untouched(buf, FILL, L)
    return dh.clone(), h


@pytest.mark.parametrize("B,T,L", SHAPES)
def test_tap_gradient_against_float64(cuda, B, T, L):
    """|dh - dh64| <= (D + 1) u sum |gm xc| per tap (C.tap_grad_tolerance: the documented order's chain length D); the twin masks
    the dropped rows and the samples ON or beyond lo / hi (at least 1 % of them); a rerun and a run on a side stream give the same
    bits.  The adjoint identity, in float64 of the device's outputs: sum_i h_i dh_i = sum gm (y - c) within sum_i |h_i| tol_i (dh's
    bound) + sum |gm| (L + 3) u (|c| + sum_i |h_i xc|) (the float32 forward's, C.apply_tolerance: y - c is the rounded filter
    sum) + u sum |gm| (|y| + |c|) (nothing: y - c is formed in float64)."""
    ops = hip()
    x, center, taps, mask, grad = C.case(B, T, L)
    y = torch.from_numpy(C.filter_apply_np(x, center, taps, mask))
    x_d, c_d, m_d, g_d, y_d = (off(t, cuda) for t in (x, center, mask, grad, y))
    assert torch.equal(bits(ops.filter_apply(x_d, c_d, off(taps, cuda), m_d)), bits(y))
    live = mask.reshape(-1, 1).bool() & (y > 0) & (y < 1)
    if T >= 255:
        assert 0.01 <= 1.0 - live[0].float().mean().item() < 0.9
    dh, stepped = device_gradient(ops, cuda, x_d, c_d, m_d, g_d, y_d, L)
    got = dh.cpu().double().numpy()
    want, abs_sum = C.tap_grad_ref64(x, center, grad, y, L, mask, parts=True)
    tol = C.tap_grad_tolerance(B, T, L, abs_sum)
    err = np.abs(got - want)
    print(f"  B {B} T {T} L {L}: D = {C.chain_length(B, T, L)}, max err / tol = {(err / np.maximum(tol, 1e-300)).max():.3f}")
    assert (err <= tol).all()
    assert np.isfinite(got).all() and (T < 64 or np.abs(got).max() > 0)
    # the first Adam ascent step from zero: lr * sign(dh) up to the eps in its denominator
    moved = stepped.cpu().double().numpy()
    big = np.abs(got) > 1e-3
    assert np.allclose(moved[big], 0.02 * np.sign(got[big]), rtol=1e-4)
    # adjoint identity
    gm = np.where(live.numpy(), grad.double().numpy(), 0.0)
    _, mag = C.filter_apply_ref64(x, center, taps, mask, parts=True)
    h64 = taps.double().numpy()
    lhs, rhs = float(h64 @ got), float((gm * (y.double().numpy() - center.double().numpy().reshape(-1, 1))).sum())
    bound = float(np.abs(h64) @ tol + (np.abs(gm) * C.apply_tolerance(L, mag)).sum())
    print(f"    adjoint: |lhs - rhs| / bound = {abs(lhs - rhs) / max(bound, 1e-300):.3f}")
    assert abs(lhs - rhs) <= bound
    again, _ = device_gradient(ops, cuda, x_d, c_d, m_d, g_d, y_d, L)
    assert torch.equal(bits(again), bits(dh))
    other, _ = on_side_stream(cuda, lambda: device_gradient(ops, cuda, x_d, c_d, m_d, g_d, y_d, L))
    assert torch.equal(bits(other), bits(dh))
    if B > 1:                                                                        # without a mask every row counts
        all_rows, _ = device_gradient(ops, cuda, x_d, c_d, None, g_d, y_d, L)
        want_all, abs_all = C.tap_grad_ref64(x, center, grad, y, L, None, parts=True)
        assert (np.abs(all_rows.cpu().double().numpy() - want_all) <= C.tap_grad_tolerance(B, T, L, abs_all)).all()


# ---- the Adam step -----------------------------------------------------------------------------------------------------------------

def test_tap_update_three_steps_against_the_float64_adam_twin(cuda):
    """Three steps, each on a new gradient, descent and ascent: the device's taps against the float64 twin fed the device's own dh,
    within TWICE the distance between the float32 and the float64 CPU twin on the same inputs.  The kernel is the float32 twin's
    arithmetic expression by expression.  Measured on gfx950: the device's taps ARE the float32 twin's — |device - f64| = |f32 twin
    - f64| = 1.905e-08, 3.295e-08, 7.996e-08 after steps 1, 2, 3, ascending and descending alike."""
    ops = hip()
    B, T, L = 3, 4100, 17
    x, center, taps, mask, _ = C.case(B, T, L)
    y = torch.from_numpy(C.filter_apply_np(x, center, taps, mask))
    x_d, c_d, m_d, y_d = (t.to(cuda) for t in (x, center, mask, y))
    for ascend in (True, False):
        h_d, am, av = taps.to(cuda), torch.zeros(L, device=cuda), torch.zeros(L, device=cuda)
        dh_d = torch.empty(L, device=cuda)
        h32 = h64 = taps.numpy()
        m32 = m64 = v32 = v64 = np.zeros(L)
        for step in (1, 2, 3):
            grad = torch.randn(B, T, generator=torch.Generator().manual_seed(step))
            ops.filter_tap_grad(x_d, c_d, grad.to(cuda), y_d, L, m_d)
            ops.filter_tap_update(h_d, am, av, B, T, step, 0.02, ascend=ascend, dh_out=dh_d)
            dh = dh_d.cpu().numpy()
            h32, m32, v32 = C.adam_step(h32, m32, v32, dh, step, 0.02, ascend=ascend, dtype=np.float32)
            h64, m64, v64 = C.adam_step(h64, m64, v64, dh, step, 0.02, ascend=ascend, dtype=np.float64)
            twin = np.abs(h32.astype(np.float64) - h64).max()
            err = np.abs(h_d.cpu().double().numpy() - h64).max()
            print(f"  ascend {ascend} step {step}: |device - f64| = {err:.3e}, |f32 twin - f64| = {twin:.3e}")
            assert err <= 2 * twin
            assert np.abs(am.cpu().double().numpy() - m64).max() <= 2 * max(np.abs(m32 - m64).max(), 1e-300)
            assert np.abs(av.cpu().double().numpy() - v64).max() <= 2 * max(np.abs(v32 - v64).max(), 1e-300)
        assert np.abs(h64 - taps.numpy()).max() > 0.01                              # the taps moved


# ---- the attack on a linear detector ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T", [700, 4100])
def test_fit_on_a_linear_detector(cuda, T):
    """The recipe whose outcome was computed beforehand in float64 on the CPU (tests/test_filter_host.py repeats it at T = 700):
    8 rows, spoof / bonafide alternating, 17 taps, lr 0.02, 40 steps on all 8 rows.  Every fitted spoof row and four held-out
    spoof rows of another seed end with z > 0 (on the CPU: z > 3, from about -0.8); every bonafide row is bit-identical to its
    input; the taps are within TWICE the distance between the float32 and the float64 CPU restatement of the same fit.  Measured
    on gfx950, max over the taps: T = 700: |device - f64| = 1.694e-07 against |f32 restatement - f64| = 1.273e-07; T = 4100:
    1.345e-07 against 1.154e-07.  Fitted spoof rows end at z = 3.26 .. 4.32, held-out ones at 3.19 .. 4.58; ||h - impulse|| = 2.9."""
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    ops = hip()
    wave, y, v = C.linear_case(T, seed=0)
    model = C.RevertedLinear(v).to(cuda)
    x01, mn, mx = ops.to_minmax(wave.to(cuda))
    atk = torchattacks.UniversalFilter(model, taps=C.FIT["taps"], lr=C.FIT["lr"], epochs=C.FIT["steps"], source_label=0)
    model.set_minmax(mn, mx)
    atk.fit([(x01, y.to(cuda), mn, mx)])
    assert atk.fit_steps == 40 and atk.delta.shape == (17,) and atk.delta.is_cuda
    h = atk.delta.cpu().double().numpy()
    args = (x01.cpu(), y, mn.cpu(), mx.cpu(), v)
    h64 = C.fit_restated(*args, dtype=np.float64, **C.FIT)
    h32 = C.fit_restated(*args, dtype=np.float32, **C.FIT)
    twin, err = np.abs(h32.astype(np.float64) - h64).max(), np.abs(h - h64).max()
    print(f"  T {T}: |device - f64| = {err:.3e}, |f32 restatement - f64| = {twin:.3e}, ||h - impulse|| = {np.linalg.norm(h64 - np.eye(17)[8]):.3f}")
    held, y_h, _ = C.linear_case(T, seed=1, rows=4, spoof_only=True)
    for w, labels in ((wave, y), (held, y_h)):
        a01, a_mn, a_mx = ops.to_minmax(w.to(cuda))
        model.set_minmax(a_mn, a_mx)
        atk.set_minmax(a_mn, a_mx)
        adv = atk(a01, labels.to(cuda))
        with torch.no_grad():
            z0, z = model(a01).reshape(-1).cpu(), model(adv).reshape(-1).cpu()
        print("  z before:", [round(t, 2) for t in z0.tolist()], "\n  z after: ", [round(t, 2) for t in z.tolist()])
        assert bool((z0[labels == 0] < 0).all()) and bool((z[labels == 0] > 0).all())
        assert torch.equal(bits(adv[labels == 1]), bits(a01[labels == 1]))         # bonafide rows: unchanged
        assert atk.fit_steps == 40
    assert err <= 2 * twin


# ---- through the loop --------------------------------------------------------------------------------------------------------------

CFG = {"data": {"seed": 42}, "checkpoint": {"path": ""},
       "model": {"name": "lcnn", "parameters": {"frontend_algorithm": ["lfcc"], "input_channels": 1}}}
KEYS = ["universal/fit_utterances", "universal/heldout_utterances", "universal/accuracy_fit", "universal/accuracy_heldout",
        "universal/source_flipped_fit", "universal/source_flipped_heldout"]
FILTER_KEYS = ["filter/taps", "filter/gain_db_max", "filter/gain_db_min", "filter/dc_gain_db", "filter/identity_distance"]


def test_loop_fits_on_the_first_batch_and_applies_to_all(cuda, tmp_path, monkeypatch):
    """generate_attacks with FILTER_SPOOF over 8 synthetic utterances of 4100 samples, batch 4, universal_fit = 1: the universal/*
    group keys without the two delta_* norms, the filter/* keys, the taps under scores["universal_delta"], and save -> load
    reproducing the scores bit for bit with no fit step.  How many utterances flip is not asserted."""
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    from audio_deepfake_adversarial_attacks_amd.aa.aa_types import AttackEnum
    from audio_deepfake_adversarial_attacks_amd.datasets.synthetic import SyntheticDetectionDataset
    from audio_deepfake_adversarial_attacks_amd.evaluation import generate_attacks
    from audio_deepfake_adversarial_attacks_amd.metrics import filter_summary
    monkeypatch.setenv("ADVSTEP_ATTACK_GRAPH", "0")
    method, params = AttackEnum["FILTER_SPOOF"].value
    data = SyntheticDetectionDataset(8, num_samples=4100)
    fit_calls = []
    real_fit = torchattacks.UniversalFilter.partial_fit
    monkeypatch.setattr(torchattacks.UniversalFilter, "partial_fit", lambda self, *a: (fit_calls.append(1), real_fit(self, *a))[1])

    def evaluate(**kw):
        torch.manual_seed(5)
        fit_calls.clear()
        rep = generate_attacks([None, None, None], CFG, str(cuda), attack_model_config=CFG, attack_method=method,
                               attack_params=params, batch_size=4, dataset=data, share_weights=True, shuffle=False,
                               num_workers=0, return_scores=True, in_flight=1, perturbation_stats=True, **kw)
        torch.cuda.synchronize()
        return rep, len(fit_calls)

    path = tmp_path / "filter.npz"
    one, n_fit = evaluate(universal_fit=1, universal_save=path)
    assert n_fit == 5                                                   # epochs x one batch
    assert [k for k in one if k.startswith("universal/")] == KEYS and [k for k in one if k.startswith("filter/")] == FILTER_KEYS
    assert not any("delta_" in k for k in one)
    assert one["universal/fit_utterances"] == 4 and one["universal/heldout_utterances"] == 4 and one["num_total"] == 8
    taps = one["scores"]["universal_delta"]
    assert taps.dtype == np.float32 and taps.shape == (129,) and one["filter/taps"] == 129
    assert {k: one[k] for k in FILTER_KEYS} == filter_summary(taps)
    if (data.y[:4] == 0).any():                                         # a spoof row in the fitted batch: the fit moved the taps
        assert one["filter/identity_distance"] > 0
    assert any(k.startswith("perturbation/") for k in one)
    loaded, n_fit = evaluate(universal_load=path)
    assert n_fit == 0                                                   # zero fit steps
    assert loaded["universal/fit_utterances"] == 0 and loaded["universal/heldout_utterances"] == 8
    assert np.array_equal(loaded["scores"]["universal_delta"].view(np.int32), taps.view(np.int32))
    for k in ("y_pred", "y_pred_label", "y"):
        assert np.array_equal(loaded["scores"][k], one["scores"][k]), k
    assert np.array_equal(loaded["scores"]["y_pred"].view(np.int32), one["scores"]["y_pred"].view(np.int32))


def test_loop_still_refuses_the_keywords_for_another_attack(cuda):
    from audio_deepfake_adversarial_attacks_amd.aa.aa_types import AttackEnum
    from audio_deepfake_adversarial_attacks_amd.datasets.synthetic import SyntheticDetectionDataset
    from audio_deepfake_adversarial_attacks_amd.evaluation import generate_attacks
    method, params = AttackEnum["FGSM"].value
    with pytest.raises(ValueError, match="need a universal attack"):
        generate_attacks([None, None, None], CFG, str(cuda), attack_model_config=CFG, attack_method=method, attack_params=params,
                         batch_size=4, dataset=SyntheticDetectionDataset(4, num_samples=4100), share_weights=True, shuffle=False,
                         num_workers=0, universal_fit=1)
