"""CPU: host logic of PGDSNR — constructor surface, the registry, argument validation of the two entry points of
include/advstep_snr.h without a device, the callers that hand the utterance's min and max over, and the attack on an analytic
linear detector through the CPU table tests/snr_cpu_ops.py, where the logit's movement is known in closed form."""
import ctypes
import math

import pytest
import torch

from tests import snr_cpu_ops as C

U = C.U


@pytest.fixture(scope="module")
def lib():
    from audio_deepfake_adversarial_attacks_amd import build
    build.build()
    from audio_deepfake_adversarial_attacks_amd import _lib
    return _lib.load()


def stub(T=8):
    return C.LinearDetector(torch.ones(T), torch.zeros(1))


def test_class_is_exported_and_prints_public_hyper_parameters_only():
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    assert "PGDSNR" in torchattacks.__all__
    atk = torchattacks.PGDSNR(stub())
    assert str(atk) == ("PGDSNR(model_name=LinearDetector, device=cpu, snr_db=30.0, segmental=False, steps=10, rel_alpha=0.25, "
                        "eps_for_division=1e-10, attack_mode=default, return_type=float)")
    assert atk.replays_from_graph is True and atk.wants_minmax is True and atk._supported_mode == ["default"]
    assert atk.rho == pytest.approx(10.0 ** -1.5, rel=1e-15)
    with pytest.raises(ValueError, match="Targeted mode is not supported"):
        atk.set_mode_targeted_by_function(lambda images, labels: 1 - labels)
    custom = torchattacks.PGDSNR(stub(), snr_db=20, segmental=True, steps=4, rel_alpha=0.5, eps_for_division=1e-12)
    assert (custom.snr_db, custom.segmental, custom.steps, custom.rel_alpha, custom.eps_for_division) == (20, True, 4, 0.5, 1e-12)
    assert torchattacks.PGDSNR(stub(), steps=5).rel_alpha == 0.5
    assert not getattr(torchattacks.PGD(stub()), "wants_minmax", False)


def test_constructor_refusals():
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    with pytest.raises(ValueError, match="NaN"):
        torchattacks.PGDSNR(stub(), snr_db=float("nan"))
    with pytest.raises(ValueError, match="at least 1"):
        torchattacks.PGDSNR(stub(), steps=0)


def test_registry_members():
    import evaluate_models_on_adversarial_attacks as cli
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    from audio_deepfake_adversarial_attacks_amd.aa.aa_types import AttackEnum
    want = {f"PGD{'SEG' if seg else ''}SNR_{db}dB": {"snr_db": float(db), "segmental": seg, "steps": 10}
            for seg in (False, True) for db in (40, 30, 20)}
    assert len(want) == 6
    for name, kw in want.items():
        method, params = AttackEnum[name].value
        assert method is torchattacks.PGDSNR and params == kw
        atk = method(stub(), **params)
        assert atk.rel_alpha == 0.25 and atk.segmental is kw["segmental"] and atk.snr_db == kw["snr_db"]
        assert cli.parse_arguments(["--attack", name]).attack == name
    assert len({e.name for e in AttackEnum}) == len(AttackEnum.__members__)
    assert AttackEnum["PGD"].value == (torchattacks.PGD, {"eps": 0.0005, "steps": 10})


def test_argument_validation_needs_no_device(lib):
    """Invalid arguments are rejected before any launch (so this is safe without a device); no call here is valid as a whole."""
    EINVAL, EWORKSPACE = 1, 2
    P = [ctypes.c_void_p(0x100000 * (k + 1)) for k in range(7)]     # never dereferenced: validation fails first
    adv, grad, orig, off, out, eps, ws = P
    B, Tn = 2, 8
    nan = float("nan")

    def seg(adv=adv, grad=grad, orig=orig, off=off, out=out, rho=0.03, B=B, Tn=Tn):
        return lib.advstep_seg_pgd_step_f32(adv, grad, orig, off, rho, 0.25, 1e-10, 0.0, 1.0, out, B, Tn, None)

    for missing in ("adv", "grad", "orig", "out"):
        assert seg(**{missing: None}) == EINVAL
        assert seg(**{missing: None}, off=None) == EINVAL            # a null offset is no excuse for another
    assert seg(B=-1) == EINVAL and seg(Tn=-1) == EINVAL and seg(B=65536) == EINVAL
    assert seg(rho=nan) == EINVAL and seg(rho=-0.01) == EINVAL and seg(rho=nan, B=0) == EINVAL
    assert seg(out=grad) == EINVAL and seg(out=orig) == EINVAL and seg(out=off) == EINVAL
    assert seg(out=ctypes.c_void_p(adv.value + 4)) == EINVAL        # overlaps adv without being adv
    assert seg(off=ctypes.c_void_p(out.value + 4 * B * Tn - 4)) == EINVAL
    assert seg(B=0, adv=None, grad=None, orig=None, off=None, out=None) == 0 and seg(Tn=0) == 0

    need = lib.advstep_row_workspace_bytes(B, Tn)

    def rad(x=orig, off=off, eps=eps, rho=0.03, B=B, Tn=Tn, ws=ws, ws_bytes=need):
        return lib.advstep_snr_row_radius_f32(x, off, rho, eps, B, Tn, ws, ws_bytes, None)

    assert rad(x=None) == EINVAL and rad(eps=None) == EINVAL
    assert rad(B=-1) == EINVAL and rad(Tn=-1) == EINVAL and rad(B=65536) == EINVAL
    assert rad(rho=nan) == EINVAL and rad(rho=-1.0) == EINVAL
    assert rad(eps=orig) == EINVAL and rad(eps=ctypes.c_void_p(orig.value + 4 * B * Tn - 4)) == EINVAL and rad(eps=off) == EINVAL
    assert rad(ws=None) == EWORKSPACE and rad(ws_bytes=need - 1) == EWORKSPACE and rad(ws=ctypes.c_void_p(ws.value + 4)) == EWORKSPACE
    assert rad(off=None, ws=None) == EWORKSPACE                     # a null offset is valid: the workspace is what fails
    assert rad(B=0, x=None, eps=None, ws=None, ws_bytes=0) == 0 and rad(Tn=0, ws=None, ws_bytes=0) == 0


def test_wrappers_refuse_cpu_tensors_and_bad_scalars():
    from audio_deepfake_adversarial_attacks_amd import _lib, hip_ops
    x, c = torch.zeros(2, 8), torch.zeros(2)
    with pytest.raises(_lib.AdvstepError, match="no CPU fallback"):
        hip_ops.seg_pgd_step(x, x.clone(), x.clone(), c, 0.03, 0.25, 1e-10)
    with pytest.raises(_lib.AdvstepError, match="no CPU fallback"):
        hip_ops.seg_pgd_step(x, x.clone(), x.clone(), None, 0.03, 0.25, 1e-10)
    with pytest.raises(_lib.AdvstepError, match="no CPU fallback"):
        hip_ops.snr_row_radius(x, c, 0.03)


# ---- the callers hand mn and mx over ---------------------------------------------------------------------------------------------

class StubAttack:
    def __init__(self, wants, ops=None):
        if wants is not None:
            self.wants_minmax = wants
        self.ops, self.got, self.calls = ops, [], 0

    def set_minmax(self, mn, mx):
        self.got.append((mn, mx))

    def __call__(self, x01, y):
        self.calls += 1
        self.seen_minmax_first = len(self.got)
        return x01


class StubOps:
    def __init__(self):
        self.mn, self.mx = torch.tensor([[-1.0], [-2.0]]), torch.tensor([[1.0], [3.0]])

    def to_minmax(self, x):
        return x * 0.5, self.mn, self.mx

    def revert_minmax(self, x01, mn, mx):
        assert mn is self.mn and mx is self.mx
        return x01 * 2.0


@pytest.mark.parametrize("wants", [True, False, None])
def test_attack_batch_and_the_trainer_helper_call_set_minmax(monkeypatch, wants):
    from audio_deepfake_adversarial_attacks_amd import evaluation
    from audio_deepfake_adversarial_attacks_amd.trainer import AdversarialGDTrainer
    ops = StubOps()
    monkeypatch.setattr(evaluation.aa_utils, "to_minmax", ops.to_minmax)
    monkeypatch.setattr(evaluation.aa_utils, "revert_minmax", ops.revert_minmax)
    x, y = torch.rand(2, 8), torch.zeros(2)
    for run in (lambda atk: evaluation.attack_batch(atk, x, y), lambda atk: AdversarialGDTrainer._attack_batch(atk, x, y)):
        atk = StubAttack(wants, ops)
        out = run(atk)
        assert torch.equal(out, x) and atk.calls == 1
        if wants:
            assert len(atk.got) == 1 and atk.got[0][0] is ops.mn and atk.got[0][1] is ops.mx    # the tensors to_minmax returned
            assert atk.seen_minmax_first == 1                                                    # before the attack ran
        else:
            assert atk.got == []


def test_multiattack_refuses_a_member_that_wants_minmax():
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    with pytest.raises(ValueError, match="cannot be a member"):
        torchattacks.MultiAttack.on_model(stub(), [("PGD", {"eps": 0.001, "steps": 2}), ("PGDSNR", {"snr_db": 30.0})])
    assert len(torchattacks.MultiAttack.on_model(stub(), [("PGD", {"eps": 0.001, "steps": 2})]).attacks) == 1


def test_set_minmax_is_consumed_and_checked():
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    model, x, y, _ = linear_case(segmental=True, with_minmax=False)
    atk = torchattacks.PGDSNR(model, segmental=True, steps=1, rel_alpha=1.0)
    atk.ops = C
    plain = atk(x, y)
    B = x.shape[0]
    mn, mx = torch.full((B, 1), -0.4), torch.full((B,), 0.6)         # (B, 1) and (B,) are both taken
    atk.set_minmax(mn, mx)
    shifted = atk(x, y)
    assert not torch.equal(shifted, plain)
    assert torch.equal(atk(x, y), plain)                              # consumed by ONE call
    atk.set_minmax(mn[:-1], mx[:-1])
    with pytest.raises(ValueError, match="one value per utterance"):
        atk(x, y)
    assert torch.equal(atk(x, y), plain)                              # ... and cleared by the refused call too
    atk.set_minmax(torch.zeros(B), torch.zeros(B))                    # a constant utterance: NaN, as to_minmax gives
    assert torch.isnan(atk(x, y)).all()


# ---- closed form on the linear detector --------------------------------------------------------------------------------------------

T_CASE = 700                                                        # segments of 256, 256 and 188 samples
FACTORS = (0.5, 1.5, 0.8, 1.25, 0.25, 3.0)                          # |z0| as a multiple of the movement: < 1 flips, > 1 does not


def linear_case(segmental, with_minmax, snr_db=30.0, seed=11):
    """(model, x, y, the movement of each row's logit in float64): rows strictly inside the box — x in [0.3, 0.7], and a
    sample moves by at most r max|w| / ||w|| < 0.08 — so no clamp acts; |z0| = FACTORS[b] * movement, on the label's side."""
    g = torch.Generator().manual_seed(seed)
    B = len(FACTORS)
    w = 0.1 * (torch.rand(T_CASE, generator=g) + 0.5) * (torch.randint(0, 2, (T_CASE,), generator=g) * 2 - 1).float()
    x = torch.rand(B, T_CASE, generator=g) * 0.4 + 0.3
    y = torch.randint(0, 2, (B,), generator=g)
    c = minmax_case(B)[2] if with_minmax else None
    rho = C.rho_of(snr_db)
    if segmental:
        r = C.segment_radii_ref64(x, c, rho)                                                    # (B, S)
        wn = (C.segments(w.double().reshape(1, -1)) ** 2).sum(-1).sqrt()                         # (1, S)
        move = (r * wn).sum(-1)
    else:
        move = C.snr_row_radius_ref64(x, c, rho) * w.double().norm()
    side = torch.where(y == 1, 1.0, -1.0).double()
    bias = side * torch.tensor(FACTORS, dtype=torch.float64) * move - x.double() @ w.double()
    return C.LinearDetector(w, bias), x, y, move


def minmax_case(B):
    mn = -0.2 - 0.05 * torch.arange(B, dtype=torch.float32)
    mx = 0.9 + 0.1 * torch.arange(B, dtype=torch.float32)
    return mn, mx, mn / (mx - mn)


@pytest.mark.parametrize("with_minmax", [False, True])
@pytest.mark.parametrize("segmental", [True, False])
def test_one_full_step_moves_the_logit_by_the_closed_form(segmental, with_minmax):
    """rel_alpha = 1, steps = 1 from the clean input: every segment (row) moves by its whole radius along its own w / ||w||, so
    the logit moves by sum_s r_s ||w_s|| (e_b ||w||) against the label, every budget is met with equality, and a row flips iff
    |z0| is below that sum.

    Tolerance: the restatement computes in float64 (1e-12 relative covers it); what is left is float32 at the table's boundary.
    The gradient reaches the step as float32 — each w_t dz rounds once, which moves the normalised direction by at most 2u —
    and the global radius is rounded to float32 once: 4u of the movement covers both.  The result is rounded to float32 once per
    sample: sum_t |w_t| u |adv_t| on the logit, and u ||adv||_seg on a segment's norm."""
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    model, x, y, move = linear_case(segmental, with_minmax)
    B = x.shape[0]
    atk = torchattacks.PGDSNR(model, snr_db=30.0, segmental=segmental, steps=1, rel_alpha=1.0)
    atk.ops = C
    c = None
    if with_minmax:
        mn, mx, c = minmax_case(B)
        atk.set_minmax(mn, mx)
    adv = atk(x, y)
    assert adv.dtype == torch.float32 and adv.min() > 0.2 and adv.max() < 0.8                    # no clamp acted
    w, bias = model.w.detach(), model.bias
    z0, z1 = x.double() @ w + bias, adv.double() @ w + bias
    side = torch.where(y == 1, 1.0, -1.0).double()
    got = (z0 - z1) * side                                                                      # against the label
    tol = 4 * U * move + U * (adv.double().abs() @ w.abs()) + 1e-12 * move
    print("  movement:", move.tolist(), "\n  got - want:", (got - move).tolist(), "\n  tol:", tol.tolist())
    assert ((got - move).abs() <= tol).all()
    d = adv.double() - x.double()
    if segmental:
        r = C.segment_radii_ref64(x, c, C.rho_of(30.0))
        dn = (C.segments(d) ** 2).sum(-1).sqrt()
        an = (C.segments(adv.double()) ** 2).sum(-1).sqrt()
    else:
        r = C.snr_row_radius_ref64(x, c, C.rho_of(30.0))
        dn, an = d.norm(dim=1), adv.double().norm(dim=1)
    assert (r > 0).all() and ((dn - r).abs() <= 4 * U * r + U * an).all()                       # every budget met with equality
    flipped = C.judged_wrong(z1.float(), y)
    want = torch.tensor([f < 1 for f in FACTORS])
    assert not C.judged_wrong(z0.float(), y).any() and torch.equal(flipped, want) and want.any() and not want.all()
    if with_minmax:                                                                             # the offset changed the budget
        plain = torchattacks.PGDSNR(model, snr_db=30.0, segmental=segmental, steps=1, rel_alpha=1.0)
        plain.ops = C
        assert not torch.equal(plain(x, y), adv)


@pytest.mark.parametrize("segmental", [True, False])
def test_ten_steps_stay_inside_the_budget(segmental):
    """The default step size over ten steps: the projection holds every segment (row) inside its ball."""
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    model, x, y, _ = linear_case(segmental, True)
    mn, mx, c = minmax_case(x.shape[0])
    atk = torchattacks.PGDSNR(model, snr_db=30.0, segmental=segmental)
    atk.ops = C
    atk.set_minmax(mn, mx)
    adv = atk(x, y)
    d = adv.double() - x.double()
    if segmental:
        r, dn = C.segment_radii_ref64(x, c, C.rho_of(30.0)), (C.segments(d) ** 2).sum(-1).sqrt()
        an = (C.segments(adv.double()) ** 2).sum(-1).sqrt()
    else:
        r, dn, an = C.snr_row_radius_ref64(x, c, C.rho_of(30.0)), d.norm(dim=1), adv.double().norm(dim=1)
    assert (dn <= r * (1 + 4 * U) + U * an).all() and (dn >= 0.99 * r).all()                    # 2.5 radii of steps fill the ball


def test_cpu_table_on_hand_checkable_segments():
    """One row of three segments (256, 256, 3): a silent one, one with no gradient, one that is scaled back."""
    T = 515
    x = torch.zeros(1, T)
    x[0, 256:512] = 0.5
    x[0, 512:] = torch.tensor([0.3, 0.4, 0.0])                       # ||.|| = 0.5
    g = torch.ones(1, T)
    g[0, 256:512] = 0.0
    adv = x.clone()
    adv[0, :256] = 0.25                                              # moved where nothing may move
    adv[0, 300] = 0.75                                               # inside its ball: r = 0.1 * 0.5 * 16 = 0.8
    out = C.seg_pgd_step(adv, g, x, None, 0.1, 1.0, 1e-10)
    assert torch.equal(out[0, :256], x[0, :256])                     # radius 0: back to orig
    assert torch.equal(out[0, 256:512], adv[0, 256:512])             # no gradient, inside: f = 1
    want = x[0, 512:].double() + 0.1 * 0.5 / math.sqrt(3.0)          # r = 0.05 along (1, 1, 1) / sqrt(3)
    assert torch.allclose(out[0, 512:].double(), want, rtol=0, atol=2 * U)
    assert C.snr_row_radius(x, None, 0.1).item() == pytest.approx(0.1 * math.sqrt(256 * 0.25 + 0.25), rel=2 * U)
    c = torch.tensor([-0.5])
    assert C.snr_row_radius(x, c, 1.0).item() == pytest.approx(math.sqrt(256 * 0.25 + 0.04 + 0.01 + 0.25), rel=2 * U)
    assert C.segment_radii_ref64(x, c, 1.0)[0, 1].item() == 0.0       # x + c = 0 throughout: silent under the offset
