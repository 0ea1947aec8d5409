"""GPU: the attack on the smoothed detector — smoothadv_fill against the float64 twin (tests/smoothadv_cpu_ops.py) within
test_gpu_smooth's measured bound, against smooth_noise and against itself bit for bit; smoothadv_loss_grad against the float64 twin
within a measured bound; smoothadv_step bit for bit against the slot-order device sum followed by the library's own PGD steps; the
edges and EINVAL cases of the three entry points through the C ABI; SmoothAdvPGD on the analytic linear case; SMOOTHADV through the
evaluation loop with a certificate; Gaussian-noise and SmoothAdv training."""
import random

import numpy as np
import pytest
import torch

from tests import smoothadv_cpu_ops as A
from tests.test_gpu_momentum import padded, untouched
from tests.test_gpu_smooth import CERT_KEYS, CERTIFY, MEASURED_OVER_SIGMA, certified_part, loop, same_certificates, shifted
from tests.test_gpu_spsa import bits, on_side_stream

pytestmark = pytest.mark.gpu

SEED = (0x01234567 << 32) | 0x89ABCDEF            # non-zero high words
OFFSET = (5 << 32) | 0x00000100
SIGMA = 0.05
FILL = 3.5
SHAPES = [(3, 4099), (2, 4100), (1, 1), (2, 5), (2, 8193)]
SLOTS = [1, 2, 5]
# max |dz - twin64| over the row's max |twin64|, and max |cost - twin64| / max(|cost|, 1), measured on (8, 4096) logits with
# saturated, mixed and near-zero rows at scale +-1 (tools/smoothadv_probe.py --error; profiles/smoothadv_timing.txt): the device
# library's expf, log1pf and logf; 3.10e-7 for dz and 3.78e-7 for the cost, the larger kept for both.  The tests assert twice that.  The measurement had to come out at most 1e-5.
MEASURED_LOSS_REL = 3.8e-7
assert 0.0 < MEASURED_LOSS_REL <= 1e-5


def hip():
    from audio_deepfake_adversarial_attacks_amd import hip_ops
    return hip_ops


def raw():
    from audio_deepfake_adversarial_attacks_amd import _lib
    return _lib.load()


def stream(cuda):
    return torch.cuda.current_stream(cuda).cuda_stream


def wave01(B, T, seed):
    return torch.rand(B, T, generator=torch.Generator().manual_seed(seed))


def affine(B, seed):
    """(scale, shift) = (mx - mn, mn) of utterances with spans 0.5 .. 2.5 around negative minima."""
    g = torch.Generator().manual_seed(seed)
    mn = -torch.rand(B, generator=g) - 0.1
    mx = mn + 0.5 + 2.0 * torch.rand(B, generator=g)
    return mx - mn, mn


# ---- the fill ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,T,off_by_one", [(B, T, False) for B, T in SHAPES] + [(2, 4096, True)])
def test_fill_against_the_float64_twin(cuda, B, T, off_by_one):
    ops, ns, s0 = hip(), 3, 2
    x = wave01(B, T, 100 + T)
    scale, shift = affine(B, T)
    x_d = shifted(x, cuda) if off_by_one else x.to(cuda)
    buf, out = padded((ns, B, T), FILL, cuda)
    assert ops.smoothadv_fill(x_d, SIGMA, SEED, OFFSET, s0=s0, ns=ns, scale=scale.to(cuda), shift=shift.to(cuda), out=out) is out
    torch.cuda.synchronize()
    assert untouched(buf, FILL, ns * B * T)                                          # a canary either side of `out`
    got = out.cpu().numpy().astype(np.float64)
    twin = A.fill_np(x, SIGMA, SEED, OFFSET, s0, ns, scale, shift, dtype=np.float64)
    err = np.abs(got - twin)
    bound = 2.0 * MEASURED_OVER_SIGMA * float(np.float32(SIGMA)) + np.spacing(np.abs(twin).astype(np.float32)).astype(np.float64)
    print(f"({B}, {T}): max |out - twin64| / sigma = {err.max() / SIGMA:.3e}, largest share of the bound {np.max(err / bound):.3f}")
    assert (err <= bound).all()
    assert torch.equal(bits(x_d), bits(x))                                            # the input is read only


@pytest.mark.parametrize("B,T", SHAPES)
def test_fill_without_scale_has_smooth_noises_bits(cuda, B, T):
    ops = hip()
    x_d = wave01(B, T, 7 + T).to(cuda)
    want = ops.smooth_noise(x_d, SIGMA, SEED, OFFSET, s0=1, ns=3)
    assert torch.equal(bits(ops.smoothadv_fill(x_d, SIGMA, SEED, OFFSET, s0=1, ns=3)), bits(want))
    one, zero = torch.ones(B, device=cuda), torch.zeros(B, device=cuda)               # x * 1 + 0 is x: the affine kernel, same values
    assert bool((ops.smoothadv_fill(x_d, SIGMA, SEED, OFFSET, s0=1, ns=3, scale=one, shift=zero) == want).all())


@pytest.mark.parametrize("T", [4100, 4099])
def test_fill_chunks_routes_and_streams_give_the_same_bits(cuda, T):
    ops, B, ns = hip(), 3, 5
    x = wave01(B, T, 7)
    scale, shift = (t.to(cuda) for t in affine(B, 3))
    x_d = x.to(cuda)
    kw = {"scale": scale, "shift": shift}
    whole = ops.smoothadv_fill(x_d, SIGMA, SEED, OFFSET, s0=1, ns=ns, **kw)
    assert whole.shape == (ns, B, T)
    parts = torch.cat([ops.smoothadv_fill(x_d, SIGMA, SEED, OFFSET, s0=1, ns=2, **kw), ops.smoothadv_fill(x_d, SIGMA, SEED, OFFSET, s0=3, ns=3, **kw)])
    assert torch.equal(bits(parts), bits(whole))                                      # a fill in chunks, 2 + 3
    assert torch.equal(bits(ops.smoothadv_fill(shifted(x, cuda), SIGMA, SEED, OFFSET, s0=1, ns=ns, **kw)), bits(whole))   # the scalar route
    other = on_side_stream(cuda, lambda: ops.smoothadv_fill(x_d, SIGMA, SEED, OFFSET, s0=1, ns=ns, **kw))
    assert torch.equal(bits(other), bits(whole))                                      # a rerun, on a second stream
    x[1, 5] = float("nan")                                                            # a NaN stays where it is
    got = ops.smoothadv_fill(x.to(cuda), SIGMA, SEED, OFFSET, s0=1, ns=ns, **kw).cpu()
    assert bool(torch.isnan(got[:, 1, 5]).all()) and int(torch.isnan(got).sum()) == ns


def test_fill_is_the_reverted_iterates_noise(cuda):
    """With scale = mx - mn and shift = mn as to_minmax returns them, the copies are smooth_noise's of revert_minmax(adv): bit for bit."""
    ops = hip()
    wave = (torch.rand(3, 4100, generator=torch.Generator().manual_seed(1)) * 2 - 1).to(cuda) * torch.tensor([[0.3], [1.0], [2.5]], device=cuda)
    x01, mn, mx = ops.to_minmax(wave)
    adv = (x01 + 0.001).clamp(0, 1)
    got = ops.smoothadv_fill(adv, SIGMA, SEED, OFFSET, ns=2, scale=(mx - mn).reshape(-1).contiguous(), shift=mn.reshape(-1).contiguous())
    want = ops.smooth_noise(ops.revert_minmax(adv, mn, mx), SIGMA, SEED, OFFSET, ns=2)
    assert torch.equal(bits(got), bits(want))


# ---- the soft vote ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [6, 7, 130])
@pytest.mark.parametrize("m", [1, 2, 5, 8])
@pytest.mark.parametrize("scale", [1.0, -1.0])
def test_loss_and_gradient_against_the_float64_twin(cuda, B, m, scale):
    ops = hip()
    z, y = A.probe_logits(m, B, 100 * B + m)
    z_d = z.to(cuda)
    dz, cost = ops.smoothadv_loss_grad(z_d, y.to(cuda), scale)
    assert dz.shape == (m, B) and cost.shape == (B,) and torch.equal(bits(z_d), bits(z))
    ref_dz, ref_cost = A.loss_grad_np(z, y, scale, dtype=np.float64)
    e_dz, e_cost = A.loss_error(dz.cpu().numpy().astype(np.float64), cost.cpu().numpy().astype(np.float64), ref_dz, ref_cost)
    print(f"(m {m}, B {B}, scale {scale}): dz {e_dz:.3e}, cost {e_cost:.3e} against the asserted {2 * MEASURED_LOSS_REL:.1e}")
    assert e_dz <= 2.0 * MEASURED_LOSS_REL and e_cost <= 2.0 * MEASURED_LOSS_REL
    assert bool(torch.isfinite(dz).all()) and bool(torch.isfinite(cost).all())         # |z| = 80 included
    assert bool((dz[:, 0].abs().cpu() == 1.0 / m).all())                               # all-saturated: w = 1 / m exactly


def test_nan_logit_poisons_only_its_row(cuda):
    ops = hip()
    z, y = A.probe_logits(5, 70, 3)
    clean = ops.smoothadv_loss_grad(z.to(cuda), y.to(cuda))
    z[2, 66] = float("nan")
    dz, cost = ops.smoothadv_loss_grad(z.to(cuda), y.to(cuda))
    assert bool(torch.isnan(dz[:, 66]).all()) and bool(torch.isnan(cost[66]))
    keep = torch.arange(70) != 66
    assert torch.equal(bits(dz[:, keep]), bits(clean[0][:, keep])) and torch.equal(bits(cost[keep]), bits(clean[1][keep]))


# ---- the step --------------------------------------------------------------------------------------------------------------------------

def step_inputs(B, T, m, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, T, generator=g)
    adv = (x + (torch.rand(B, T, generator=g) - 0.5) * 0.02).clamp(0, 1)
    grads = torch.randn(m, B, T, generator=g)
    grads[:, B - 1] = 0.0                                                             # a row without a gradient
    if T > 8:
        grads[:, 0, 3] = 0.0                                                          # and a sample without one: sign(0) = 0
    return adv, x, grads


@pytest.mark.parametrize("norm", ["L2", "Linf"])
@pytest.mark.parametrize("m", SLOTS)
@pytest.mark.parametrize("B,T,off_by_one", [(B, T, False) for B, T in SHAPES] + [(2, 4096, True)])
def test_step_has_the_bits_of_the_sum_then_the_librarys_pgd_step(cuda, B, T, off_by_one, m, norm):
    ops = hip()
    adv, x, grads = step_inputs(B, T, m, 1000 * m + T)
    put = (lambda t: shifted(t, cuda)) if off_by_one else (lambda t: t.to(cuda))
    adv_d, x_d, grads_d = put(adv), put(x), put(grads)
    eps, alpha = (0.05, 0.02) if norm == "L2" else (0.004, 0.001)
    total = grads_d[0].clone()
    for i in range(1, m):
        total = total + grads_d[i]                                                    # the slot-order device sum
    plain = ops.pgd_l2_step if norm == "L2" else ops.pgd_linf_step
    want = plain(adv.to(cuda), total, x.to(cuda), alpha, eps)
    obuf, out = padded((B, T), FILL, cuda)
    gbuf, gsum = padded((B, T), FILL, cuda)
    res = ops.smoothadv_step(adv_d, x_d, grads_d, alpha, eps, norm=norm, out=out, gsum=gsum)
    torch.cuda.synchronize()
    assert res[0] is out and res[1] is gsum
    assert untouched(obuf, FILL, B * T) and untouched(gbuf, FILL, B * T)
    assert torch.equal(bits(gsum), bits(total)) and torch.equal(bits(out), bits(want))
    assert torch.equal(bits(adv_d), bits(adv)) and torch.equal(bits(x_d), bits(x)) and torch.equal(bits(grads_d), bits(grads))
    if m == 1:
        assert torch.equal(bits(gsum), bits(grads[0]))
    alias = adv_d.clone() if not off_by_one else put(adv)
    assert ops.smoothadv_step(alias, x_d, grads_d, alpha, eps, norm=norm, out=alias) is alias   # out is adv
    assert torch.equal(bits(alias), bits(want))
    other = on_side_stream(cuda, lambda: ops.smoothadv_step(adv_d, x_d, grads_d, alpha, eps, norm=norm))
    assert torch.equal(bits(other), bits(want))


@pytest.mark.parametrize("norm", ["L2", "Linf"])
def test_step_keeps_a_nan_in_its_row(cuda, norm):
    ops = hip()
    adv, x, grads = step_inputs(3, 4100, 2, 5)
    clean = ops.smoothadv_step(adv.to(cuda), x.to(cuda), grads.to(cuda), 0.02, 0.05, norm=norm)
    grads[1, 1, 7] = float("nan")
    got, gsum = ops.smoothadv_step(adv.to(cuda), x.to(cuda), grads.to(cuda), 0.02, 0.05, norm=norm, gsum=torch.empty(3, 4100, device=cuda))
    assert bool(torch.isnan(gsum[1, 7])) and int(torch.isnan(gsum).sum()) == 1
    assert torch.equal(bits(got[[0, 2]]), bits(clean[[0, 2]]))


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------

def test_every_einval_case_of_the_header(cuda):
    lib, EINVAL, EWORKSPACE = raw(), 1, 2
    st = stream(cuda)
    x = torch.zeros(2, 8, device=cuda)
    row = torch.ones(2, device=cuda)
    out = torch.full((3, 2, 8), FILL, device=cuda)

    def fill(ap=x.data_ptr(), sc=row.data_ptr(), sh=row.data_ptr(), op=out.data_ptr(), B=2, T=8, s0=0, ns=3, sigma=SIGMA):
        return lib.advstep_smoothadv_fill_f32(ap, sc, sh, op, B, T, s0, ns, sigma, 1, 0, st)

    assert fill(B=-1) == EINVAL and fill(T=-1) == EINVAL and fill(ns=-1) == EINVAL and fill(s0=-1) == EINVAL
    assert fill(B=65_536) == EINVAL
    assert fill(ap=None) == EINVAL and fill(op=None) == EINVAL
    assert fill(sc=None) == EINVAL and fill(sh=None) == EINVAL                          # one of the two alone
    assert fill(op=x.data_ptr()) == EINVAL and fill(ap=out.data_ptr() + 4 * 40) == EINVAL   # out overlaps adv
    assert fill(sc=out.data_ptr() + 4) == EINVAL and fill(sh=out.data_ptr() + 4 * 46) == EINVAL   # out overlaps scale / shift
    for sigma in (-0.01, float("nan"), float("inf"), -float("inf")):
        assert fill(sigma=sigma) == EINVAL
    assert fill(B=0) == 0 and fill(T=0) == 0 and fill(ns=0) == 0
    assert fill(ap=None, sc=None, sh=None, op=None, ns=0) == 0 and fill(ap=None, sc=None, sh=None, op=None, B=0) == 0

    z = torch.zeros(3, 2, device=cuda)
    y = torch.zeros(2, dtype=torch.int64, device=cuda)
    dz = torch.full((3, 2), FILL, device=cuda)
    cost = torch.full((2,), FILL, device=cuda)

    def loss(zp=z.data_ptr(), yp=y.data_ptr(), dp=dz.data_ptr(), cp=cost.data_ptr(), B=2, m=3):
        return lib.advstep_smoothadv_loss_grad_f32(zp, yp, dp, cp, B, m, 1.0, st)

    assert loss(B=-1) == EINVAL and loss(m=-1) == EINVAL
    assert loss(zp=None) == EINVAL and loss(yp=None) == EINVAL and loss(dp=None) == EINVAL and loss(cp=None) == EINVAL
    assert loss(dp=z.data_ptr()) == EINVAL and loss(dp=y.data_ptr()) == EINVAL and loss(cp=z.data_ptr() + 8) == EINVAL
    assert loss(cp=y.data_ptr()) == EINVAL and loss(cp=dz.data_ptr() + 4) == EINVAL
    assert loss(B=0) == 0 and loss(m=0) == 0 and loss(zp=None, yp=None, dp=None, cp=None, m=0) == 0

    adv, orig = torch.zeros(2, 8, device=cuda), torch.zeros(2, 8, device=cuda)
    grads = torch.zeros(3, 2, 8, device=cuda)
    gsum, res = torch.full((2, 8), FILL, device=cuda), torch.full((2, 8), FILL, device=cuda)
    ws = torch.zeros(4096, dtype=torch.uint8, device=cuda)
    need = lib.advstep_row_workspace_bytes(2, 8)
    assert 0 < need <= ws.numel()

    def step(ap=adv.data_ptr(), xp=orig.data_ptr(), gp=grads.data_ptr(), sp=gsum.data_ptr(), op=res.data_ptr(), B=2, T=8, m=3, norm=1,
             wp=ws.data_ptr(), wb=ws.numel()):
        return lib.advstep_smoothadv_step_f32(ap, xp, gp, sp, op, B, T, m, norm, 0.02, 0.05, 1e-10, 0.0, 1.0, wp, wb, st)

    for norm in (0, 1):
        assert step(B=-1, norm=norm) == EINVAL and step(T=-1, norm=norm) == EINVAL and step(m=-1, norm=norm) == EINVAL
        assert step(B=65_536, norm=norm) == EINVAL
        for name in ("ap", "xp", "gp", "sp", "op"):
            assert step(norm=norm, **{name: None}) == EINVAL
        assert step(sp=grads.data_ptr() + 4 * 16, norm=norm) == EINVAL and step(op=grads.data_ptr() + 4 * 40, norm=norm) == EINVAL
        assert step(sp=orig.data_ptr(), norm=norm) == EINVAL and step(op=orig.data_ptr(), norm=norm) == EINVAL
        assert step(sp=adv.data_ptr(), norm=norm) == EINVAL and step(sp=res.data_ptr() + 4, norm=norm) == EINVAL
        assert step(op=adv.data_ptr() + 4, norm=norm) == EINVAL                         # out overlaps adv without being adv
        assert step(B=0, norm=norm) == 0 and step(T=0, norm=norm) == 0 and step(m=0, norm=norm) == 0
        assert step(ap=None, xp=None, gp=None, sp=None, op=None, wp=None, wb=0, m=0, norm=norm) == 0
    assert step(norm=2) == EINVAL and step(norm=-1) == EINVAL
    assert step(wp=None) == EWORKSPACE and step(wb=need - 1) == EWORKSPACE and step(wp=ws.data_ptr() + 4) == EWORKSPACE
    assert step(norm=0, wp=None, wb=0) == 0                                             # L-inf needs no workspace (this one launches)
    torch.cuda.synchronize()
    assert bool((out == FILL).all()) and bool((dz == FILL).all()) and bool((cost == FILL).all())   # nothing else was launched
    assert bool((gsum == 0).all()) and bool((res == 0).all())                          # the one L-inf launch: zeros in, zeros out

    ops = hip()
    with pytest.raises(ValueError, match="sigma"):
        ops.smoothadv_fill(x, -1.0, 1)
    with pytest.raises(ValueError, match="s0 and ns"):
        ops.smoothadv_fill(x, 0.1, 1, s0=-1)
    with pytest.raises(ValueError, match="together"):
        ops.smoothadv_fill(x, 0.1, 1, scale=row)
    with pytest.raises(ValueError, match="one value per row"):
        ops.smoothadv_fill(x, 0.1, 1, scale=torch.ones(3, device=cuda), shift=torch.ones(3, device=cuda))
    with pytest.raises(ValueError, match="out must hold"):
        ops.smoothadv_fill(x, 0.1, 1, ns=2, out=torch.zeros(3, 2, 8, device=cuda))
    with pytest.raises(TypeError, match="int64"):
        ops.smoothadv_loss_grad(z, y.int())
    with pytest.raises(ValueError, match=r"\(m, B\)"):
        ops.smoothadv_loss_grad(z.reshape(-1), y)
    with pytest.raises(ValueError, match="norm"):
        ops.smoothadv_step(adv, orig, grads, 0.02, 0.05, norm="L1")
    with pytest.raises(ValueError, match="grads must hold"):
        ops.smoothadv_step(adv, orig, torch.zeros(3, 2, 7, device=cuda), 0.02, 0.05)


# ---- the attack on the analytic case ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T,steps,alpha", [(1028, 4, None), (1030, 3, None), (1028, 2, 0.1 * 0.45 * 0.01)],
                         ids=["whole_radius", "odd_length", "short_of_the_radius"])
def test_attack_on_the_linear_detector(cuda, T, steps, alpha):
    """The CPU properties (tests/smoothadv_cpu_ops.check_linear_attack) through the HIP kernels, and the smoothed detector's own
    answer: after the whole radius eps = 0.45 sigma the k = 0.5 row keeps a margin of 0.05 sigma, so its class wins a vote with
    probability Phi(0.05) = 0.520; 40 000 votes put the majority 8 standard deviations from a tie."""
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    model, x01, y, k, sigma = A.unit_box_linear_case(T)
    eps = 0.45 * sigma
    model = model.to(cuda)
    atk = torchattacks.SmoothAdvPGD(model, eps=eps, alpha=alpha, steps=steps, sigma=sigma, samples=4, random_start=False)
    torch.manual_seed(11)
    adv = atk(x01.to(cuda), y.to(cuda))
    torch.cuda.synchronize()
    strong, clean = A.check_linear_attack(adv, x01, model, y, k, sigma, eps, steps, atk.alpha)
    if T == 1028 and alpha is None:
        n0 = 40_000
        sm = torchattacks.Smoothing(sigma, n=1, n0=n0, max_rows=8192, seed=99)
        votes = sm.predict(model, adv, 0).cpu()
        assert bool((votes[:, 1] == n0).all())
        kept = (2 * votes[:, 0] > n0) == clean
        print(f"class-1 votes of {n0}: {votes[:, 0].tolist()}")
        assert bool(kept[strong].all())


# ---- through the loop -------------------------------------------------------------------------------------------------------------------

def test_loop_with_smoothadv(cuda):
    """8 synthetic utterances, batch 4, LCNN + LFCC at random initialisation, SMOOTHADV at 2 steps of 2 draws with test_gpu_smooth's
    CERTIFY settings.  (The scorer's noise offsets advance by the PREDICT votes too, so the second batch's certificate is drawn at
    other offsets than in the NO_ATTACK run; the clean keys are compared all the same, as the figures of one detector.)"""
    from audio_deepfake_adversarial_attacks_amd.aa.aa_types import AttackEnum
    method, params = AttackEnum["SMOOTHADV"].value
    params = {**params, "steps": 2, "samples": 2}
    plain = loop(None, {}, **CERTIFY)
    rep = loop(method, params, **CERTIFY)
    assert [k for k in rep if k.startswith("certified/")] == CERT_KEYS + ["certified/attacked_accuracy", "certified/attacked_abstained",
                                                                         "certified/violations"]
    assert isinstance(rep["certified/violations"], int) and rep["certified/violations"] >= 0
    assert 0.0 <= rep["certified/attacked_accuracy"] <= 100.0
    clean_rep, clean_plain = certified_part(rep)[0], certified_part(plain)[0]
    np.testing.assert_equal({k: clean_rep[k] for k in CERT_KEYS}, {k: clean_plain[k] for k in CERT_KEYS})
    assert (rep["scores"]["certified"]["l2"] > 0).all()
    again = loop(method, params, **CERTIFY)
    same_certificates(rep, again)
    assert np.array_equal(rep["scores"]["y_pred"].view(np.int32), again["scores"]["y_pred"].view(np.int32))
    assert {k: v for k, v in rep.items() if k.startswith("adv_eval/")} == {k: v for k, v in again.items() if k.startswith("adv_eval/")}


# ---- the trainer -----------------------------------------------------------------------------------------------------------------------

def _lcnn(cuda):
    from audio_deepfake_adversarial_attacks_amd.models.models import get_model
    torch.manual_seed(0)
    return get_model("lcnn", {"frontend_algorithm": ["lfcc"], "input_channels": 1}, str(cuda)).to(cuda)


def _train(cuda, noise_sigma, attacks, set_attribute=True, linear=False):
    from audio_deepfake_adversarial_attacks_amd import trainer as T
    from audio_deepfake_adversarial_attacks_amd.datasets.synthetic import SyntheticDetectionDataset
    random.seed(1)
    torch.manual_seed(1)
    model = torch.nn.Linear(64_600, 1).to(cuda) if linear else _lcnn(cuda)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    tr = T.EqualAdversarialGDTrainer(epochs=1, batch_size=4, device=str(cuda), optimizer_kwargs={"lr": 1e-4})
    if set_attribute:
        tr.noise_sigma = noise_sigma
    real = tr.init_adv_attacks

    def small(attack_model, names):                                                    # the enum's attack at 2 steps of 2 draws
        made = real(attack_model, names)
        for _, atk in made:
            atk.steps, atk.samples = 2, 2
        return made
    tr.init_adv_attacks = small
    inner = tr._attack_batch
    tr._attack_batch = staticmethod(lambda atk, bx, by: (calls.append(type(atk).__name__), inner(atk, bx, by))[1])
    records, calls = [], []
    import logging
    handler = logging.Handler()
    handler.emit = lambda rec: records.append(rec.getMessage())
    T.LOGGER.setLevel(logging.INFO)
    T.LOGGER.addHandler(handler)
    try:
        if attacks:
            out = tr.train(dataset=SyntheticDetectionDataset(8, return_meta=False), model=model, attack_model=model,
                           adversarial_attacks=attacks, test_dataset=SyntheticDetectionDataset(4, seed=99, return_meta=False))
        else:
            plain = T.GDTrainer(epochs=1, batch_size=4, device=str(cuda), optimizer_kwargs={"lr": 1e-4})
            if set_attribute:
                plain.noise_sigma = noise_sigma
            out = plain.train(SyntheticDetectionDataset(8, return_meta=False), model,
                              test_dataset=SyntheticDetectionDataset(4, seed=99, return_meta=False))
    finally:
        T.LOGGER.removeHandler(handler)
    torch.cuda.synchronize()
    losses = [float(m.split("train/loss: ")[1].split(",")[0]) for m in records if "train/loss: " in m]
    return before, {k: v.detach().clone() for k, v in out.state_dict().items()}, (losses, calls), torch.get_rng_state()


@pytest.mark.parametrize("attacks", [[], ["SMOOTHADV"]], ids=["gaussian_noise_training", "smoothadv_training"])
def test_training_under_noise(cuda, attacks):
    before, after, (losses, calls), _ = _train(cuda, 0.05, attacks)
    assert losses and all(np.isfinite(v) for v in losses)
    assert calls == (["SmoothAdvPGD"] * 3 if attacks else [])                         # two training steps and the attacked validation
    changed = [k for k, v in after.items() if v.dtype.is_floating_point and not torch.equal(v, before[k])]
    assert len(changed) > 10 and all(torch.isfinite(v).all() for v in after.values() if v.dtype.is_floating_point)


def test_training_without_noise_is_the_run_it_was(cuda, monkeypatch):
    """noise_sigma=None: the weights are, bit for bit, those of a run on which the noise path cannot have been taken (the class
    attribute untouched and hip_ops.smooth_noise made to raise), under the same seed; torch's CPU generator ends in the same state:
    no key was drawn.

    The detector here is one linear layer over the 64 600 samples, not LCNN: a comparison bit for bit needs a training run that
    the device repeats bit for bit, and LCNN's does not, with or without this attribute.  Measured on the unchanged path (three
    seeded runs of GDTrainer, one epoch, synthetic 8 / 4, batch 4): 40 and 39 of LCNN's 57 tensors differ between runs, by up to
    4.5e-5 (`m_transform.16.bias`; the first step's loss agrees, the second's differs in the seventh digit), and the convolutional
    Surrogate of tests/helpers.py differed once in two comparisons (conv.weight, 1.2e-10): the weight gradients of the
    convolutions are accumulated in an order that varies.  On the CPU, where training repeats, tests/test_trainer.py's golden runs
    and tests/test_smoothadv_host.py pin the same property bit for bit."""
    ops = hip()
    _, want, _, rng_want = _train(cuda, None, [], set_attribute=False, linear=True)

    def boom(*args, **kw):
        raise AssertionError("smooth_noise was called with noise_sigma=None")
    monkeypatch.setattr(ops, "smooth_noise", boom)
    before, got, _, rng_got = _train(cuda, None, [], linear=True)
    assert list(got) == list(want) and all(torch.equal(got[k], want[k]) for k in want)
    assert any(not torch.equal(got[k], before[k]) for k in got)                        # it did train
    assert torch.equal(rng_got, rng_want)
