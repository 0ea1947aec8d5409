"""CPU: host logic of UniversalFilter — constructor surface, the registry, `metrics.filter_summary` against hand-computed
responses, the .npz round trip, the CPU twins of tests/filter_cpu_ops.py against each other, the sensitivity of the tap
gradient's bound to a dropped (tile, row) partial, and argument validation of the entry points of include/advstep_filter.h
without a device."""
import ctypes

import numpy as np
import pytest
import torch

from tests import filter_cpu_ops as C
from tests.radius_cpu_ops import LinearDetector


@pytest.fixture(scope="module")
def lib():
    from audio_deepfake_adversarial_attacks_amd import build
    build.build()
    from audio_deepfake_adversarial_attacks_amd import _lib
    return _lib.load()


def stub(T=8):
    return LinearDetector(torch.ones(T), torch.zeros(1))


# ---- surface -------------------------------------------------------------------------------------------------------------------------

def test_class_is_exported_and_prints_public_hyper_parameters_only():
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    assert "UniversalFilter" in torchattacks.__all__
    atk = torchattacks.UniversalFilter(stub())
    assert str(atk) == ("UniversalFilter(model_name=LinearDetector, device=cpu, taps=129, lr=0.02, epochs=5, source_label=0, "
                        "betas=(0.9, 0.999), attack_mode=default, return_type=float)")
    assert atk.is_universal is True and atk.is_filter is True and atk.replays_from_graph is False
    assert atk.wants_minmax is True and atk.delta is None and atk.fit_steps == 0 and atk._supported_mode == ["default"]
    assert not getattr(torchattacks.UniversalPGD(stub()), "is_filter", False)
    with pytest.raises(ValueError, match="Targeted mode is not supported"):
        atk.set_mode_targeted_by_function(lambda images, labels: 1 - labels)
    with pytest.raises(RuntimeError, match="fit or load a perturbation first"):
        atk(torch.zeros(2, 8), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="fit or load a perturbation first"):
        atk.save_delta("unused.npz")
    custom = torchattacks.UniversalFilter(stub(), taps=1025, lr=0.1, epochs=2, source_label=None, betas=(0.5, 0.9))
    assert (custom.taps, custom.lr, custom.epochs, custom.source_label, custom.betas) == (1025, 0.1, 2, None, (0.5, 0.9))


def test_constructor_refusals():
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    for kw, match in (({"taps": 128}, "odd number"), ({"taps": 0}, "odd number"), ({"taps": -3}, "odd number"),
                      ({"taps": 1027}, "odd number"), ({"taps": 3.5}, "odd number"), ({"taps": True}, "odd number"),
                      ({"lr": 0.0}, "step size > 0"), ({"lr": -1.0}, "step size > 0"), ({"lr": float("nan")}, "step size > 0"),
                      ({"epochs": 0}, "at least 1"), ({"source_label": 2}, "None, 0 or 1"), ({"source_label": -1}, "None, 0 or 1"),
                      ({"source_label": "spoof"}, "None, 0 or 1"), ({"source_label": False}, "None, 0 or 1"),
                      ({"betas": (0.9,)}, "two decay rates"), ({"betas": (0.9, 1.0)}, "two decay rates")):
        with pytest.raises(ValueError, match=match):
            torchattacks.UniversalFilter(stub(), **kw)
    assert torchattacks.UniversalFilter(stub(), taps=1).taps == 1 and torchattacks.UniversalFilter(stub(), taps=1025).taps == 1025


def test_registry_members_and_cli_flags():
    import evaluate_models_on_adversarial_attacks as cli
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    from audio_deepfake_adversarial_attacks_amd.aa.aa_types import AttackEnum
    want = {"FILTER_SPOOF": {"taps": 129, "source_label": 0}, "FILTER_SPOOF_L257": {"taps": 257, "source_label": 0},
            "FILTER_SPOOF_L1025": {"taps": 1025, "source_label": 0}}
    for name, kw in want.items():
        method, params = AttackEnum[name].value
        assert method is torchattacks.UniversalFilter and params == kw
        atk = method(stub(), **params)
        assert atk.is_universal and atk.is_filter and atk.wants_minmax and atk.epochs == 5 and atk.lr == 0.02
        assert cli.parse_arguments(["--attack", name]).attack == name
    assert len({e.name for e in AttackEnum}) == len(AttackEnum.__members__)        # no member became an alias of another
    for name, (method, params) in ((e.name, e.value) for e in AttackEnum if e.name.startswith("WORSTCASE")):
        assert all(member != "UniversalFilter" for member, _ in params["members"]), name
    b = cli.parse_arguments(["--attack", "FILTER_SPOOF", "--universal_fit", "3", "--universal_save", "out.npz"])
    assert (b.universal_fit, b.universal_load, b.universal_save) == (3, None, "out.npz")


# ---- the summary ---------------------------------------------------------------------------------------------------------------------

def test_filter_summary_against_hand_computed_responses():
    """The unit impulse: |H| = 1 at every frequency, distance 0.  [0.5, 0, 0.5]: H(w) = e^{-jw} cos(w), so |H| = 1 (0 dB) at DC
    and at half the sampling rate and a null at a quarter of it (bin 1024 of 4096: cos(pi / 2), -inf or far below -300 dB);
    the distance from the impulse [0, 1, 0] is sqrt(0.25 + 1 + 0.25)."""
    from audio_deepfake_adversarial_attacks_amd.metrics import filter_summary
    for L in (1, 17, 129):
        h = np.zeros(L)
        h[(L - 1) // 2] = 1.0
        s = filter_summary(h)
        assert list(s) == ["filter/taps", "filter/gain_db_max", "filter/gain_db_min", "filter/dc_gain_db", "filter/identity_distance"]
        assert s["filter/taps"] == L and s["filter/identity_distance"] == 0.0
        assert max(abs(s[k]) for k in ("filter/gain_db_max", "filter/gain_db_min", "filter/dc_gain_db")) < 1e-12
    s = filter_summary(np.array([0.5, 0.0, 0.5], dtype=np.float32))
    assert s["filter/taps"] == 3 and abs(s["filter/dc_gain_db"]) < 1e-12 and abs(s["filter/gain_db_max"]) < 1e-12
    assert s["filter/gain_db_min"] < -300.0
    assert s["filter/identity_distance"] == pytest.approx(np.sqrt(1.5), rel=1e-15)
    assert filter_summary([2.0])["filter/dc_gain_db"] == pytest.approx(20 * np.log10(2.0), rel=1e-15)
    with pytest.raises(ValueError, match="odd number"):
        filter_summary([1.0, 0.0])


# ---- persistence ---------------------------------------------------------------------------------------------------------------------

def test_npz_round_trip_and_refusals(tmp_path):
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    atk = torchattacks.UniversalFilter(stub(), taps=5, source_label=0)
    taps = torch.tensor([0.1, -0.2, 0.9, 0.3, -0.05])
    atk._h = taps.clone()
    atk._fit_steps = 7
    path = tmp_path / "filter.npz"
    atk.save_delta(path)
    with np.load(path) as z:
        assert sorted(z.files) == ["L", "source_label", "taps"] and int(z["L"]) == 5 and int(z["source_label"]) == 0
        assert z["taps"].dtype == np.float32
    other = torchattacks.UniversalFilter(stub(), taps=5, source_label=0)
    other.load_delta(path)
    assert torch.equal(other.delta, taps) and other.fit_steps == 0 and other.delta.dtype == torch.float32
    with pytest.raises(ValueError, match="fitted for L=5"):
        torchattacks.UniversalFilter(stub(), taps=7, source_label=0).load_delta(path)
    with pytest.raises(ValueError, match="source_label=0"):
        torchattacks.UniversalFilter(stub(), taps=5, source_label=None).load_delta(path)
    uap = tmp_path / "uap.npz"
    pgd = torchattacks.UniversalPGD(stub())
    pgd._delta = torch.zeros(1, 8)
    pgd.save_delta(uap)
    with pytest.raises(ValueError, match="not a filter file"):
        other.load_delta(uap)
    assert torch.equal(other.delta, taps)                                          # a refused file changes nothing


# ---- the twins -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,T,L", [(3, 255, 17), (2, 300, 257), (3, 4100, 3)])
def test_float32_twin_within_the_bound_of_the_float64_twin(B, T, L):
    """|out32 - out64| <= (L + 3) u (|c| + sum_i |h_i xc|) per sample (C.apply_tolerance); masked rows are x's bits; some samples
    clip at either end."""
    x, center, taps, mask, _ = C.case(B, T, L)
    out32 = C.filter_apply_np(x, center, taps, mask)
    out64, mag = C.filter_apply_ref64(x, center, taps, mask, parts=True)
    err, tol = np.abs(out32.astype(np.float64) - out64), C.apply_tolerance(L, mag)
    print(f"  ({B}, {T}, {L}): max err / tol = {(err / tol).max():.3f}")
    assert (err <= tol).all()
    assert np.array_equal(out32[1].view(np.int32), x[1].numpy().view(np.int32)) if B > 1 else True
    assert (out32[0] == 0.0).any() and (out32[0] == 1.0).any()
    same_all = C.filter_apply_np(x, center, taps, None)
    assert np.array_equal(same_all[0], out32[0]) and not np.array_equal(same_all[1], x[1].numpy())


def test_identity_filter_returns_the_row_and_masks_its_two_extremes():
    """h = the impulse: out = c + (x - c), x up to two roundings; the samples 0 and 1 of a min-max row sit ON the bounds and
    contribute nothing to the tap gradient under the strict rule, clipped or not."""
    x, center, _, _, grad = C.case(2, 64, 5)
    x = torch.rand(2, 64, generator=torch.Generator().manual_seed(1)) * 0.8 + 0.1
    x[:, 3], x[:, 9] = 0.0, 1.0
    taps = torch.tensor([0.0, 0.0, 1.0, 0.0, 0.0])
    out = C.filter_apply_np(x, center, taps)
    assert np.abs(out - x.numpy()).max() <= 2 * C.U and (out[:, 3] == 0).all() and (out[:, 9] == 1).all()
    full = C.tap_grad_ref64(x, center, grad, out, 5)
    g2 = grad.clone()
    g2[:, 3] = g2[:, 9] = 0.0
    assert np.array_equal(full, C.tap_grad_ref64(x, center, g2, out, 5))
    g2[:, 4] += 1.0
    assert not np.array_equal(full, C.tap_grad_ref64(x, center, g2, out, 5))


def test_tap_gradient_twin_is_the_derivative_of_the_filter():
    """Away from the clamp, sum(w * out) is linear in the taps: its derivative along tap i is dh[i] with grad = w."""
    x, center, taps, mask, grad = C.case(3, 200, 17)
    wide = {"lo": -10.0, "hi": 10.0}                                                # no sample is clamped
    out = C.filter_apply_ref64(x, center, taps, mask, **wide)
    dh = C.tap_grad_ref64(x, center, grad, out.astype(np.float32), 17, mask, **wide)
    for i in (0, 8, 16):
        moved = taps.clone()
        moved[i] += 0.25
        step = float(moved[i]) - float(taps[i])
        other = C.filter_apply_ref64(x, center, moved, mask, **wide)
        slope = ((other - out) * grad.double().numpy()).sum() / step
        assert slope == pytest.approx(dh[i], rel=1e-9, abs=1e-9)
    assert np.array_equal(out[1], x[1].double().numpy())                            # the masked row: no derivative at all


@pytest.mark.parametrize("B,T,L", [s for s in C.shapes() if s[1] >= 255 and s[2] <= 257 and s[1] <= 4100])
def test_the_bound_cannot_hide_a_dropped_tile(B, T, L):
    """SENSITIVITY: on the GPU test's inputs, the float64 gradient with ONE (tile, row) partial left out — tile 0 of row 0 — misses
    the exact one by more than the bound, at some tap.  (No bound on rounding can see a partial smaller than itself: the one- and
    four-sample last tiles of T = 4097 and 4100 stay under it for most taps — measured here: 1 of 17 and 0 of 255 taps over the
    bound at T = 4097 — so it is the full tile that is dropped.)"""
    x, center, taps, mask, grad = C.case(B, T, L)
    out = C.filter_apply_np(x, center, taps, mask)
    clipped = ((out[0] <= 0) | (out[0] >= 1)).mean()
    assert clipped >= 0.01                                                          # at least 1 % of the samples clip
    dh, mag = C.tap_grad_ref64(x, center, grad, out, L, mask, parts=True)
    dropped = C.tap_grad_ref64(x, center, grad, out, L, mask, drop=(0, 0))
    tol = C.tap_grad_tolerance(B, T, L, mag)
    over = np.abs(dropped - dh) > tol
    print(f"  ({B}, {T}, {L}): D = {C.chain_length(B, T, L)}, taps over the bound {over.sum()} / {L}, clipped {clipped:.3f}")
    assert over.any()


def test_chain_length_of_the_documented_order():
    assert C.chain_length(3, 4100, 17) == 32 + 128 + 2 + 3 + 1
    assert C.chain_length(128, 64_600, 255) == 256 + 16 + 16 + 16 + 8
    assert C.chain_length(1, 1, 1) == 16 + 256 + 1 + 1 + 1
    assert max(C.chain_length(*s) for s in C.shapes()) < 5792                      # the second-order condition of the bound


def test_adam_twin_float32_against_float64():
    g = np.random.default_rng(0)
    h32 = h64 = np.zeros(9)
    m32 = m64 = v32 = v64 = np.zeros(9)
    for step in (1, 2, 3):
        dh = g.standard_normal(9).astype(np.float32)
        h32, m32, v32 = C.adam_step(h32, m32, v32, dh, step, 0.02, dtype=np.float32)
        h64, m64, v64 = C.adam_step(h64, m64, v64, dh, step, 0.02, dtype=np.float64)
    assert h32.dtype == np.float32 and np.abs(h32 - h64).max() < 1e-6 and np.abs(h64).max() > 0.01
    first, _, _ = C.adam_step(np.zeros(3), np.zeros(3), np.zeros(3), np.array([1.0, -2.0, 0.5]), 1, 0.02)
    assert np.allclose(first, [0.02, -0.02, 0.02], rtol=1e-6)                      # ascent: the first step is lr * sign(dh)
    down, _, _ = C.adam_step(np.zeros(3), np.zeros(3), np.zeros(3), np.array([1.0, -2.0, 0.5]), 1, 0.02, ascend=False)
    assert np.array_equal(down, -first)


def test_fit_restated_moves_every_spoof_row_across_the_boundary():
    """The issue's recipe in float64 on the CPU: every fitted and held-out spoof row ends with z > 3 (from about -0.8)."""
    T = 700
    wave, y, v = C.linear_case(T, seed=0)
    x01, mn, mx = C.minmax(wave)
    h = C.fit_restated(x01, y, mn, mx, v, dtype=np.float64, **C.FIT)
    held, y_h, _ = C.linear_case(T, seed=1, rows=4, spoof_only=True)
    for w, labels in ((wave, y), (held, y_h)):
        a01, a_mn, a_mx = C.minmax(w)
        adv = C.filter_apply_ref64(a01, (-a_mn / (a_mx - a_mn)).reshape(-1), h.astype(np.float32), (labels == 0).float())
        z = (adv * (a_mx - a_mn).double().numpy() + a_mn.double().numpy()) @ v.double().numpy()
        z0 = w.double().numpy() @ v.double().numpy()
        print("  z before:", np.round(z0, 2), "\n  z after: ", np.round(z, 2))
        assert (z0[labels.numpy() == 0] < -0.5).all() and (z[labels.numpy() == 0] > 3.0).all()
        assert np.array_equal(adv[labels.numpy() == 1], a01.numpy().astype(np.float64)[labels.numpy() == 1])


# ---- the C ABI without a device ------------------------------------------------------------------------------------------------------

def test_argument_validation_needs_no_device(lib):
    """Invalid arguments are rejected before any launch (so this is safe without a device); no call here is valid as a whole."""
    EINVAL, EWORKSPACE = 1, 2
    P = [ctypes.c_void_p(0x10000000 * (k + 1)) for k in range(9)]     # never dereferenced: validation fails first
    x, center, mask, taps, out, grad, adv, ws, extra = P
    B, T, L = 3, 5000, 17

    assert lib.advstep_filter_workspace_bytes(B, T, L) == 3 * 2 * 17 * 4
    assert lib.advstep_filter_workspace_bytes(128, 64_600, 255) == 128 * 16 * 255 * 4
    for bad in ((0, T, L), (B, 0, L), (-1, T, L), (B, -1, L), (B, T, 0), (B, T, 16), (B, T, 1027), (65536, T, L)):
        assert lib.advstep_filter_workspace_bytes(*bad) == 0
    need = lib.advstep_filter_workspace_bytes(B, T, L)

    def apply(x=x, center=center, mask=mask, taps=taps, out=out, B=B, T=T, L=L):
        return lib.advstep_filter_apply_f32(x, center, mask, taps, out, B, T, L, 0.0, 1.0, None)

    for missing in ("x", "center", "taps", "out"):
        assert apply(**{missing: None}) == EINVAL
        assert apply(**{missing: None}, mask=None) == EINVAL           # a null mask is no excuse for another
    assert apply(B=-1) == EINVAL and apply(T=-1) == EINVAL and apply(B=65536) == EINVAL
    assert apply(L=0) == EINVAL and apply(L=16) == EINVAL and apply(L=1027) == EINVAL and apply(L=-1) == EINVAL
    assert apply(out=center) == EINVAL and apply(out=mask) == EINVAL and apply(out=taps) == EINVAL
    assert apply(out=ctypes.c_void_p(x.value + 4)) == EINVAL          # overlaps x without being x
    assert apply(out=x) == EINVAL                                     # in place across tiles: a halo is a neighbour's output
    assert apply(B=0, x=None, center=None, taps=None, out=None, mask=None) == 0 and apply(T=0) == 0

    def tap_grad(x=x, center=center, mask=mask, grad=grad, adv=adv, ws=ws, ws_bytes=need, B=B, T=T, L=L):
        return lib.advstep_filter_tap_grad_f32(x, center, mask, grad, adv, ws, ws_bytes, B, T, L, 0.0, 1.0, None)

    for missing in ("x", "center", "grad", "adv"):
        assert tap_grad(**{missing: None}) == EINVAL
    assert tap_grad(B=-1) == EINVAL and tap_grad(T=-1) == EINVAL and tap_grad(B=65536) == EINVAL
    assert tap_grad(L=0) == EINVAL and tap_grad(L=2) == EINVAL and tap_grad(L=1027) == EINVAL
    assert tap_grad(ws=None) == EWORKSPACE and tap_grad(ws_bytes=need - 1) == EWORKSPACE
    assert tap_grad(mask=None, ws=None) == EWORKSPACE                  # a null mask is valid: the workspace is what fails
    assert tap_grad(ws=x) == EINVAL and tap_grad(ws=grad) == EINVAL and tap_grad(ws=adv) == EINVAL
    assert tap_grad(ws=center) == EINVAL and tap_grad(ws=mask) == EINVAL
    assert tap_grad(B=0, ws=None, ws_bytes=0) == 0 and tap_grad(T=0, ws=None, ws_bytes=0) == 0

    m, v, dh = extra, grad, adv

    def update(ws=ws, taps=taps, m=m, v=v, dh=dh, B=B, T=T, L=L, step=1):
        return lib.advstep_filter_tap_update_f32(ws, taps, m, v, dh, B, T, L, step, 0.02, 0.9, 0.999, 1e-8, 1, None)

    for missing in ("ws", "taps", "m", "v"):
        assert update(**{missing: None}) == EINVAL
    assert update(step=0) == EINVAL and update(step=-1) == EINVAL     # step is 1-based
    assert update(B=-1) == EINVAL and update(L=4) == EINVAL and update(L=1027) == EINVAL and update(B=65536) == EINVAL
    assert update(m=taps) == EINVAL and update(v=taps) == EINVAL and update(m=v) == EINVAL
    assert update(dh=taps) == EINVAL and update(dh=m) == EINVAL and update(taps=ws) == EINVAL and update(dh=ws) == EINVAL
    assert update(B=0) == 0 and update(T=0, dh=None) == 0


def test_wrappers_refuse_cpu_tensors_and_bad_taps():
    from audio_deepfake_adversarial_attacks_amd import _lib, hip_ops
    x, c, h = torch.zeros(2, 8), torch.zeros(2), torch.zeros(3)
    with pytest.raises(_lib.AdvstepError, match="no CPU fallback"):
        hip_ops.filter_apply(x, c, h)
    with pytest.raises(_lib.AdvstepError, match="no CPU fallback"):
        hip_ops.filter_tap_grad(x, c, x, x, 3)
    with pytest.raises(_lib.AdvstepError, match="no CPU fallback"):
        hip_ops.filter_tap_update(h, h.clone(), h.clone(), 2, 8, 1, 0.02)
    with pytest.raises(TypeError, match="torch.Tensor"):
        hip_ops.filter_apply(x.numpy(), c, h)
