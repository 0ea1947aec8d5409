"""CPU: host logic of UniversalPGD — constructor surface, the registry and the CLI flags, argument validation of the three entry
points of include/advstep_universal.h without a device, the run-level summary, the loop's preparation step, and the attack on
an analytic linear detector through the CPU table tests/universal_cpu_ops.py, where the fitted perturbation and the movement of
every logit are known in closed form."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import universal_cpu_ops as C

U = C.U


@pytest.fixture(scope="module")
def lib():
    from audio_deepfake_adversarial_attacks_amd import build
    build.build()
    from audio_deepfake_adversarial_attacks_amd import _lib
    return _lib.load()


def stub(T=8):
    return C.LinearDetector(torch.ones(T), torch.zeros(1))


# ---- surface -------------------------------------------------------------------------------------------------------------------------

def test_class_is_exported_and_prints_public_hyper_parameters_only():
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    assert "UniversalPGD" in torchattacks.__all__
    atk = torchattacks.UniversalPGD(stub())
    assert str(atk) == ("UniversalPGD(model_name=LinearDetector, device=cpu, norm=Linf, eps=0.0005, alpha=6.25e-05, epochs=5, "
                        "source_label=None, domain=normalized, eps_for_division=1e-10, attack_mode=default, return_type=float)")
    assert atk.is_universal is True and atk.replays_from_graph is False and atk._supported_mode == ["default"]
    assert atk.wants_minmax is False and atk.delta is None and atk.fit_steps == 0
    assert not getattr(torchattacks.PGD(stub()), "is_universal", False)
    with pytest.raises(ValueError, match="Targeted mode is not supported"):
        atk.set_mode_targeted_by_function(lambda images, labels: 1 - labels)
    l2 = torchattacks.UniversalPGD(stub(), norm="L2", eps=0.1)
    assert l2.alpha == 0.1 / 4 and torchattacks.UniversalPGD(stub(), eps=0.001).alpha == 0.001 / 8
    custom = torchattacks.UniversalPGD(stub(), norm="L2", eps=0.2, alpha=0.01, epochs=2, source_label=1, domain="waveform",
                                       eps_for_division=1e-12)
    assert (custom.norm, custom.eps, custom.alpha, custom.epochs, custom.source_label, custom.domain,
            custom.eps_for_division) == ("L2", 0.2, 0.01, 2, 1, "waveform", 1e-12)
    assert custom.wants_minmax is True


def test_constructor_refusals():
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    for kw, match in (({"norm": "L1"}, "norm must be"), ({"domain": "db"}, "domain must be"), ({"eps": 0.0}, "radius > 0"),
                      ({"eps": -0.1}, "radius > 0"), ({"eps": float("nan")}, "radius > 0"), ({"epochs": 0}, "at least 1"),
                      ({"source_label": 2}, "None, 0 or 1"), ({"source_label": -1}, "None, 0 or 1"),
                      ({"source_label": "spoof"}, "None, 0 or 1")):
        with pytest.raises(ValueError, match=match):
            torchattacks.UniversalPGD(stub(), **kw)


def test_registry_members_and_cli_flags():
    import evaluate_models_on_adversarial_attacks as cli
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    from audio_deepfake_adversarial_attacks_amd.aa.aa_types import AttackEnum
    want = {"UAP": {"norm": "Linf", "eps": 0.0005}, "UAP_eps00075": {"norm": "Linf", "eps": 0.00075},
            "UAP_eps001": {"norm": "Linf", "eps": 0.001}, "UAP_L2": {"norm": "L2", "eps": 0.1},
            "UAP_SPOOF": {"norm": "Linf", "eps": 0.0005, "source_label": 0},
            "UAP_SPOOF_eps001": {"norm": "Linf", "eps": 0.001, "source_label": 0},
            "UAP_WAVE_SPOOF": {"norm": "Linf", "eps": 0.001, "source_label": 0, "domain": "waveform"}}
    for name, kw in want.items():
        method, params = AttackEnum[name].value
        assert method is torchattacks.UniversalPGD and params == kw
        atk = method(stub(), **params)
        assert atk.is_universal and atk.wants_minmax is (name == "UAP_WAVE_SPOOF") and atk.epochs == 5
        assert cli.parse_arguments(["--attack", name]).attack == name
    assert len({e.name for e in AttackEnum}) == len(AttackEnum.__members__)
    assert AttackEnum["PGD"].value == (torchattacks.PGD, {"eps": 0.0005, "steps": 10})
    for name, (method, params) in ((e.name, e.value) for e in AttackEnum if e.name.startswith("WORSTCASE")):
        assert all(member != "UniversalPGD" for member, _ in params["members"]), name
    a = cli.parse_arguments([])
    assert (a.universal_fit, a.universal_load, a.universal_save) == (None, None, None)
    b = cli.parse_arguments(["--attack", "UAP_SPOOF", "--universal_fit", "3", "--universal_load", "in.npz", "--universal_save",
                             "out.npz"])
    assert (b.universal_fit, b.universal_load, b.universal_save) == (3, "in.npz", "out.npz")


# ---- the C ABI without a device --------------------------------------------------------------------------------------------------------

def test_argument_validation_needs_no_device(lib):
    """Invalid arguments are rejected before any launch (so this is safe without a device); no call here is valid as a whole."""
    EINVAL, EWORKSPACE = 1, 2
    P = [ctypes.c_void_p(0x1000000 * (k + 1)) for k in range(6)]     # never dereferenced: validation fails first
    grad, wgt, out, ws, x, delta = P
    R = C.GROUP_ROWS
    B, Tn = R + 1, 10                                               # two groups: the workspace is needed

    assert lib.advstep_universal_workspace_bytes(B, Tn) == 2 * 12 * 4             # planes padded to a multiple of 4 floats
    assert lib.advstep_universal_workspace_bytes(128, 64_600) == 8 * 64_600 * 4
    assert lib.advstep_universal_workspace_bytes(R, 64_600) == 0 and lib.advstep_universal_workspace_bytes(1, 5) == 0
    assert lib.advstep_universal_workspace_bytes(0, 5) == 0 and lib.advstep_universal_workspace_bytes(5, 0) == 0
    assert lib.advstep_universal_workspace_bytes(-1, 5) == 0
    need = lib.advstep_universal_workspace_bytes(B, Tn)

    def colsum(grad=grad, wgt=wgt, out=out, B=B, Tn=Tn, ws=ws, ws_bytes=need):
        return lib.advstep_universal_colsum_f32(grad, wgt, out, B, Tn, ws, ws_bytes, None)

    assert colsum(grad=None) == EINVAL and colsum(out=None) == EINVAL and colsum(grad=None, wgt=None) == EINVAL
    assert colsum(B=-1) == EINVAL and colsum(Tn=-1) == EINVAL and colsum(B=65536) == EINVAL
    assert colsum(out=grad) == EINVAL and colsum(out=ctypes.c_void_p(grad.value + 4 * B * Tn - 4)) == EINVAL
    assert colsum(out=wgt) == EINVAL and colsum(out=ctypes.c_void_p(wgt.value - 4 * Tn + 4)) == EINVAL
    assert colsum(ws=None) == EWORKSPACE and colsum(ws_bytes=need - 1) == EWORKSPACE
    assert colsum(ws=ctypes.c_void_p(ws.value + 4)) == EWORKSPACE
    assert colsum(wgt=None, ws=None) == EWORKSPACE                  # a null weight is valid: the workspace is what fails
    assert colsum(ws=out) == EINVAL and colsum(ws=grad) == EINVAL   # a workspace over an operand
    assert colsum(B=0, grad=None, out=None, ws=None, ws_bytes=0) == 0 and colsum(Tn=0, ws=None, ws_bytes=0) == 0

    def apply(x=x, delta=delta, wgt=wgt, out=out, B=B, Tn=Tn):
        return lib.advstep_universal_apply_f32(x, delta, wgt, out, B, Tn, 0.0, 1.0, None)

    for missing in ("x", "delta", "out"):
        assert apply(**{missing: None}) == EINVAL
        assert apply(**{missing: None}, wgt=None) == EINVAL          # a null weight is no excuse for another
    assert apply(B=-1) == EINVAL and apply(Tn=-1) == EINVAL and apply(B=65536) == EINVAL
    assert apply(out=delta) == EINVAL and apply(out=wgt) == EINVAL
    assert apply(out=ctypes.c_void_p(x.value + 4)) == EINVAL         # overlaps x without being x
    assert apply(delta=ctypes.c_void_p(out.value + 4 * B * Tn - 4)) == EINVAL
    assert apply(B=0, x=None, delta=None, out=None, wgt=None) == 0 and apply(Tn=0) == 0


def test_wrappers_refuse_cpu_tensors():
    from audio_deepfake_adversarial_attacks_amd import _lib, hip_ops
    x, d, w = torch.zeros(2, 8), torch.zeros(8), torch.zeros(2)
    with pytest.raises(_lib.AdvstepError, match="no CPU fallback"):
        hip_ops.universal_colsum(x, w)
    with pytest.raises(_lib.AdvstepError, match="no CPU fallback"):
        hip_ops.universal_colsum(x)
    with pytest.raises(_lib.AdvstepError, match="no CPU fallback"):
        hip_ops.universal_apply(x, d, w)
    with pytest.raises(TypeError, match="torch.Tensor"):
        hip_ops.universal_apply(x.numpy(), d)
    assert hip_ops.UNIVERSAL_GROUP_ROWS == C.GROUP_ROWS


# ---- the CPU table on hand-checkable numbers --------------------------------------------------------------------------------------

def test_cpu_table_on_hand_checkable_numbers():
    g = torch.tensor([[1.0, 2.0, float("nan")], [10.0, 20.0, 30.0], [100.0, 200.0, 300.0]])
    assert torch.equal(C.universal_colsum(g)[0, :2], torch.tensor([111.0, 222.0])) and torch.isnan(C.universal_colsum(g)[0, 2])
    out = C.universal_colsum(g, torch.tensor([0.0, 0.5, 2.0]))
    assert out.shape == (1, 3) and torch.equal(out[0, :2], torch.tensor([205.0, 410.0]))
    assert torch.isnan(out[0, 2])                                     # 0 * NaN = NaN: a zero weight multiplies
    x = torch.tensor([[0.25, 0.5, 0.999], [0.25, 0.5, 0.001]])
    d = torch.tensor([0.125, -0.25, 0.5])
    got = C.universal_apply(x, d, torch.tensor([1.0, 0.0]))
    assert torch.equal(got, torch.tensor([[0.375, 0.25, 1.0], [0.25, 0.5, 0.001]]))
    assert torch.equal(C.universal_apply(x, d, torch.tensor([[-2.0], [1.0]]))[0], torch.tensor([0.0, 1.0, 0.0]))
    assert torch.equal(C.universal_apply_f32(x, d, torch.tensor([1.0, 0.0])), got)
    into = torch.empty(3)
    assert C.universal_colsum(g[1:], None, out=into) is into and torch.equal(into, torch.tensor([110.0, 220.0, 330.0]))


def test_universal_summary():
    from audio_deepfake_adversarial_attacks_amd import metrics
    y = np.array([0, 0, 1, 1, 0, 0, 0, 1])
    lab = np.array([1, 0, 1, 0, 1, 1, 0, 1])
    fitted = np.arange(8) < 4
    delta = np.array([3e-4, -4e-4, 0.0], dtype=np.float32)
    rep = metrics.universal_summary(y, lab, fitted, delta, source_label=0)
    assert list(rep) == ["universal/fit_utterances", "universal/heldout_utterances", "universal/accuracy_fit",
                         "universal/accuracy_heldout", "universal/source_flipped_fit", "universal/source_flipped_heldout",
                         "universal/delta_linf", "universal/delta_l2"]
    assert rep["universal/fit_utterances"] == 4 and rep["universal/heldout_utterances"] == 4
    assert rep["universal/accuracy_fit"] == 50.0 and rep["universal/accuracy_heldout"] == 50.0
    assert rep["universal/source_flipped_fit"] == 50.0                               # spoof rows 0, 1: one flipped
    assert rep["universal/source_flipped_heldout"] == pytest.approx(200.0 / 3.0)     # spoof rows 4, 5, 6: two flipped
    assert rep["universal/delta_linf"] == float(np.float32(4e-4))
    assert rep["universal/delta_l2"] == pytest.approx(5e-4, rel=1e-6)
    plain = metrics.universal_summary(y, lab, np.zeros(8, bool), delta)
    assert "universal/source_flipped_fit" not in plain and math.isnan(plain["universal/accuracy_fit"])
    assert plain["universal/heldout_utterances"] == 8 and plain["universal/accuracy_heldout"] == 50.0
    with pytest.raises(ValueError, match="one value per utterance"):
        metrics.universal_summary(y, lab[:-1], fitted, delta)


# ---- closed form on the linear detector --------------------------------------------------------------------------------------------

T_CASE = 300
EPS = 0.0005
# |z(x)| of the held-out spoof rows as a multiple of the movement eps ||w||_1: < 1 flips, > 1 does not
FACTORS = (0.5, 1.5, 0.8, 1.25, 0.25, 3.0)


def linear_case(seed=5, n_batches=4, B=6):
    """(model, fit batches, held-out (x, y), w).  The detector's bias is one number, so the rows' logits are set through the
    rows themselves: x in [0.25, 0.75] (no clamp acts at eps = 0.0005) plus a multiple of sign(w) that keeps them there.  Every
    fit batch holds both classes; the logits stay small (|z| < 1), far from the saturation of the loss's sigmoid."""
    g = torch.Generator().manual_seed(seed)
    w = 0.01 * (torch.rand(T_CASE, generator=g) + 0.5) * (torch.randint(0, 2, (T_CASE,), generator=g) * 2 - 1).float()
    model = C.LinearDetector(w, torch.zeros(1))
    batches = []
    for k in range(n_batches):
        x = torch.rand(B, T_CASE, generator=g) * 0.5 + 0.25
        y = torch.tensor([(b + k) % 2 for b in range(B)])
        batches.append((x, y))
    # held-out rows: z(x) = -f * move for the spoof rows (labelled 0, judged spoof: z <= 0), set through the bias of a detector
    # per test row (the model's forward adds one bias to every row, so each held-out row is judged by its own model)
    x = torch.rand(len(FACTORS), T_CASE, generator=g) * 0.5 + 0.25
    return model, batches, x, w


def fitted_attack(model, batches, epochs=3, **kw):
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    atk = torchattacks.UniversalPGD(model, eps=EPS, epochs=epochs, source_label=0, **kw)
    atk.ops = C
    atk.fit(batches)
    return atk


def test_linf_fit_reaches_eps_sign_w_exactly_and_is_reproducible():
    """L-inf, source_label = 0, 3 epochs x 4 batches = 12 steps of eps / 8: the spoof rows' loss grows with z, so every s_t has
    the sign of w_t (the other class has weight 0 and contributes 0 * g = 0), delta_t grows by alpha sign(w_t) per step and the
    step's clamp holds it at fl32(eps) from the ninth step on: delta == fl32(eps) sign(w), exactly."""
    model, batches, _, w = linear_case()
    atk = fitted_attack(model, batches)
    assert atk.fit_steps == 12 and atk.delta.shape == (T_CASE,) and atk.delta.dtype == torch.float32
    want = torch.tensor(EPS, dtype=torch.float32) * torch.sign(w)
    assert torch.equal(atk.delta, want)
    again = fitted_attack(model, batches)
    assert again.delta.numpy().tobytes() == atk.delta.numpy().tobytes()                # fit twice: the same bytes
    atk.reset()
    assert atk.delta is None and atk.fit_steps == 0
    atk.fit(batches)
    assert torch.equal(atk.delta, want)
    few = fitted_attack(model, batches[:1], epochs=2)                                  # 2 steps: a quarter of the way
    assert torch.allclose(few.delta.double(), 0.25 * want.double(), rtol=4 * U, atol=0)


def test_heldout_rows_move_by_the_closed_form_and_the_other_class_is_untouched():
    """A held-out spoof row with x in [0.25, 0.75]: adv = fl(x + delta), so z(adv) = z(x) + eps ||w||_1 up to the one rounding
    of each sample and of the float32 logit (C.logit_tolerance); it flips exactly when that is positive.  Rows labelled 1 come
    back bit for bit."""
    model, batches, x, w = linear_case()
    atk = fitted_attack(model, batches)
    move = float(np.float32(EPS)) * float(w.double().abs().sum())
    y = torch.tensor([0, 0, 1, 0, 1, 0])
    before = x.clone()
    adv = atk(x, y)
    assert torch.equal(x, before) and adv.dtype == torch.float32 and adv.shape == x.shape
    assert torch.equal(adv[y == 1], x[y == 1])                                        # bit for bit
    assert adv.min() > 0.2 and adv.max() < 0.8                                        # no clamp acted
    wd = w.double()
    for b, f in enumerate(FACTORS):
        if y[b] != 0:
            continue
        bias = -f * move - float(x[b].double() @ wd)                                  # z(x_b) = -f * move under this bias
        row_model = C.LinearDetector(w, torch.tensor([bias]))
        z0, z1 = row_model(x[b:b + 1]).double().item(), row_model(adv[b:b + 1]).double().item()
        tol = float(C.logit_tolerance(w, adv[b], torch.tensor(z1))) + U * abs(z0) + 1e-12 * move
        print(f"  row {b}: z0 {z0:.6e} z1 {z1:.6e} move {move:.6e} err {z1 - z0 - move:.3e} tol {tol:.3e}")
        assert abs((z1 - z0) - move) <= tol
        assert tol < 0.05 * move                                                      # the cases are decided, not marginal
        assert (z1 > 0) == ((1 - f) * move > 0) and (z0 <= 0)
    assert atk.fit_steps == 12                                                         # applying fits nothing


def test_l2_fit_stays_in_its_ball_along_w():
    """L2: s is a positive multiple of w at every step, so delta is along w / ||w||_2 and reaches the sphere after 4 steps of
    eps / 4: ||delta||_2 = eps and delta / eps = w / ||w|| up to float32 rounding (the CPU table rounds each step once)."""
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    model, batches, _, w = linear_case()
    atk = torchattacks.UniversalPGD(model, norm="L2", eps=0.01, epochs=2, source_label=0)
    atk.ops = C
    atk.fit(batches)
    d = atk.delta.double()
    assert abs(d.norm().item() - 0.01) <= 0.01 * (C.norm_rel_bound(T_CASE) + 3 * U) + U * math.sqrt(T_CASE) * 0.01
    assert torch.allclose(d / 0.01, w.double() / w.double().norm(), rtol=0, atol=16 * U)
    assert (d.abs() <= float(np.float32(0.01))).all()


# ---- state, persistence, refusals ---------------------------------------------------------------------------------------------------

def test_forward_before_fit_raises_and_a_wrong_length_is_refused():
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    model, batches, x, _ = linear_case()
    atk = torchattacks.UniversalPGD(model, source_label=0)
    atk.ops = C
    y = torch.zeros(x.shape[0], dtype=torch.int64)
    with pytest.raises(RuntimeError, match="fit or load a perturbation first"):
        atk(x, y)
    with pytest.raises(RuntimeError, match="fit or load a perturbation first"):
        atk.save_delta("unused.npz")
    atk.partial_fit(*batches[0])
    assert atk.fit_steps == 1
    with pytest.raises(ValueError, match="samples"):
        atk(x[:, :-1].contiguous(), y)
    with pytest.raises(ValueError, match="samples"):
        atk.partial_fit(x[:, :-1].contiguous(), y)
    with pytest.raises(TypeError, match="float32"):
        atk(x.double(), y)
    assert all(p.requires_grad for p in model.parameters())                            # a refused call leaves the model as it was


def test_save_load_round_trip_and_refusals(tmp_path):
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    model, batches, x, _ = linear_case()
    atk = fitted_attack(model, batches[:2], epochs=1)
    path = tmp_path / "uap.npz"
    atk.save_delta(path)
    assert path.exists() and not (tmp_path / "uap.npz.npz").exists()
    with np.load(path) as z:
        assert set(z.files) == {"delta", "norm", "eps", "domain", "source_label"}
        assert z["delta"].dtype == np.float32 and z["delta"].shape == (T_CASE,)
        assert str(z["norm"]) == "Linf" and float(z["eps"]) == EPS and str(z["domain"]) == "normalized" and int(z["source_label"]) == 0
    other = torchattacks.UniversalPGD(model, eps=EPS, source_label=0)
    other.ops = C
    other.load_delta(path)
    assert other.fit_steps == 0 and other.delta.numpy().tobytes() == atk.delta.numpy().tobytes()
    y = torch.tensor([0, 1, 0, 1, 0, 0])
    assert torch.equal(other(x, y), atk(x, y))
    for kw in ({"eps": 0.001}, {"norm": "L2"}, {"domain": "waveform"}):
        refused = torchattacks.UniversalPGD(model, **{"eps": EPS, **kw})
        with pytest.raises(ValueError, match="fitted for"):
            refused.load_delta(path)
        assert refused.delta is None
    free = torchattacks.UniversalPGD(model, eps=EPS)                                  # the source label is the attack's own
    free.load_delta(path)
    assert free.source_label is None and free.delta is not None


class Recorder:
    """An op table that records the row weights universal_apply and universal_colsum are given."""

    def __init__(self, base):
        self.base, self.weights = base, []

    def __getattr__(self, name):
        fn = getattr(self.base, name)
        if name not in ("universal_apply", "universal_colsum"):
            return fn

        def wrapped(*args, **kw):
            w = args[2] if name == "universal_apply" and len(args) > 2 else (args[1] if name == "universal_colsum" and len(args) > 1
                                                                               else kw.get("row_weight"))
            self.weights.append((name, None if w is None else w.clone()))
            return fn(*args, **kw)
        return wrapped


def test_waveform_domain_weights_are_one_over_the_range_and_the_minmax_is_consumed():
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    model, batches, x, _ = linear_case()
    B = x.shape[0]
    mn = -0.2 - 0.05 * torch.arange(B, dtype=torch.float32).reshape(B, 1)              # (B, 1) and (B,) are both taken
    mx = 0.9 + 0.1 * torch.arange(B, dtype=torch.float32)
    y = torch.tensor([0, 1, 0, 0, 1, 0])
    atk = torchattacks.UniversalPGD(model, eps=0.001, source_label=0, domain="waveform")
    rec = Recorder(C)
    atk.ops = rec
    with pytest.raises(ValueError, match="set_minmax"):
        atk.partial_fit(x, y)
    atk.set_minmax(mn, mx)
    atk.partial_fit(x, y)
    want = (y == 0).float() * (1.0 / (mx - mn.reshape(-1)))
    assert [n for n, _ in rec.weights] == ["universal_apply", "universal_colsum"]
    assert all(torch.equal(w, want) for _, w in rec.weights)
    with pytest.raises(ValueError, match="set_minmax"):                                # consumed by ONE call
        atk(x, y)
    atk.set_minmax(mn, mx)
    adv = atk(x, y)
    assert torch.equal(rec.weights[-1][1], want) and torch.equal(adv[y == 1], x[y == 1])
    # in the waveform's units the added signal is the same for every source row: (mx - mn) (adv - x) = delta
    added = (adv.double() - x.double()) * (mx.double() - mn.double().reshape(-1)).reshape(B, 1)
    src = (y == 0).nonzero().reshape(-1)
    tol = (mx.double() - mn.double().reshape(-1)).reshape(B, 1) * U * 1.0 + 2 * U * atk.delta.double().abs().max()
    assert ((added[src] - atk.delta.double().reshape(1, -1)).abs() <= tol[src]).all()
    atk.set_minmax(mn[:-1], mx[:-1])
    with pytest.raises(ValueError, match="one value per utterance"):
        atk(x, y)
    fit4 = torchattacks.UniversalPGD(model, eps=0.001, epochs=2, source_label=0, domain="waveform")
    fit4.ops = C
    fit4.fit([(x, y, mn, mx)])                                                         # fit hands the 4-tuple's mn, mx over
    assert fit4.fit_steps == 2 and fit4.delta.abs().max() > 0
    plain = torchattacks.UniversalPGD(model, eps=0.001)                                # no source, normalised: every weight is 1
    rec2 = Recorder(C)
    plain.ops = rec2
    plain.partial_fit(x, y)
    assert all(w is None for _, w in rec2.weights)


# ---- the loop's preparation ---------------------------------------------------------------------------------------------------------

class StubUniversal:
    is_universal = True

    def __init__(self):
        self.log = []

    def reset(self):
        self.log.append("reset")

    def fit(self, batches):
        self.log.append(("fit", [tuple(t.shape for t in b) for b in batches]))

    def load_delta(self, path):
        self.log.append(("load", path))

    def save_delta(self, path):
        self.log.append(("save", path))


def loader(n, B=4, T=8):
    return [(torch.rand(B, T), 16_000, torch.zeros(B, dtype=torch.int64), {}) for _ in range(n)]


def test_prepare_universal_fits_on_the_first_batches_or_loads(monkeypatch):
    from audio_deepfake_adversarial_attacks_amd import evaluation
    monkeypatch.setattr(evaluation.aa_utils, "to_minmax", lambda x: (x * 0.5, x.amin(1, keepdim=True), x.amax(1, keepdim=True)))
    shapes = [(torch.Size([4, 8]), torch.Size([4]), torch.Size([4, 1]), torch.Size([4, 1]))]
    atk = StubUniversal()
    assert evaluation.prepare_universal(atk, loader(9), "cpu", 9) == 8                 # default: 9 // 4 = 2 batches
    assert atk.log == ["reset", ("fit", shapes * 2)]
    atk = StubUniversal()
    assert evaluation.prepare_universal(atk, loader(3), "cpu", 3, save="o.npz") == 4   # max(1, 3 // 4)
    assert atk.log == ["reset", ("fit", shapes), ("save", "o.npz")]
    atk = StubUniversal()
    assert evaluation.prepare_universal(atk, loader(5), "cpu", 5, fit=5) == 20
    for bad in (0, 6, -1):
        with pytest.raises(ValueError, match="universal_fit"):
            evaluation.prepare_universal(StubUniversal(), loader(5), "cpu", 5, fit=bad)
    atk = StubUniversal()
    assert evaluation.prepare_universal(atk, loader(5), "cpu", 5, fit=2, load="i.npz", save="o.npz") == 0
    assert atk.log == [("load", "i.npz"), ("save", "o.npz")]                           # a loaded perturbation fits nothing
    monkeypatch.setattr(evaluation, "rank_and_world", lambda: (1, 2))
    with pytest.raises(ValueError, match="fitted by one process"):
        evaluation.prepare_universal(StubUniversal(), loader(5), "cpu", 5)
    atk = StubUniversal()
    assert evaluation.prepare_universal(atk, loader(5), "cpu", 5, load="i.npz", save="o.npz") == 0
    assert atk.log == [("load", "i.npz")]                                              # only rank 0 writes
