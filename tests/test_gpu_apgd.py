"""`-m gpu`: the APGD kernels (include/advstep_apgd.h) against the CPU table tests/apgd_cpu_ops.py on identical inputs, and
whole APGD attacks on the detectors with every APGD launch recomputed on the CPU table from its own inputs."""
import copy

import numpy as np
import pytest
import torch

from tests import apgd_cpu_ops as C

pytestmark = pytest.mark.gpu

SHAPES = [(1, 257), (5, 4099), (128, 64_600)]
# L2 outputs: the device re-associates the row sums of squares (4096-sample tiles, wave64 trees) where torch's CPU kernels
# sum in their own order.  Bound on |out - CPU table| per sample, derived from a float64 restatement of the same chain
# (test_l2_step_error_against_float64: 6.0e-8 for each side on gfx950, 1.2e-7 together; the bound is 4x that)
L2_ATOL = 4 * 1.2e-7


def same(a, b):
    """Equal values, NaN where the other has NaN (the NaN payloads of the CPU and of gfx950 differ)."""
    return a.shape == b.shape and np.array_equal(a.detach().cpu().numpy(), b.detach().cpu().numpy(), equal_nan=True)


def hip():
    from audio_deepfake_adversarial_attacks_amd import hip_ops
    return hip_ops


def state(B, steps, eps, device, seed):
    from audio_deepfake_adversarial_attacks_amd.torchattacks.attacks.apgd import ApgdState
    g = torch.Generator().manual_seed(seed)
    st = ApgdState.new(B, steps, eps, device)
    st.acc.copy_(torch.randint(0, 2, (B,), generator=g, dtype=torch.uint8))
    st.loss_best.copy_(torch.rand(B, generator=g))
    st.loss_best_last_check.copy_(torch.rand(B, generator=g))
    st.reduced_last_check.copy_(torch.randint(0, 2, (B,), generator=g, dtype=torch.uint8))
    st.loss_steps.copy_(torch.rand(steps, B, generator=g))
    st.step_size.copy_(torch.rand(B, generator=g) * 0.01)
    return st


def cpu_copy(st):
    return type(st)(**{k: v.cpu().clone() for k, v in st.__dict__.items()})


def same_state(a, b):
    return all(same(getattr(a, k).cpu(), getattr(b, k).cpu()) for k in a.__dict__)


def waves(B, T, seed, cuda):
    """x in [0, 1] with exact 0s and 1s, a current point on the eps-ball faces, gradients with zeros and NaNs."""
    g = torch.Generator().manual_seed(seed)
    eps = 0.003
    x = torch.rand(B, T, generator=g)
    x[:, ::17] = 0.0
    x[:, 5::19] = 1.0
    cur = (x + (torch.rand(B, T, generator=g) * 2 - 1) * eps).clamp(0, 1)
    cur[:, 3::11] = (x[:, 3::11] + eps).clamp(0, 1)
    prev = (x + (torch.rand(B, T, generator=g) * 2 - 1) * eps).clamp(0, 1)
    grad = torch.randn(B, T, generator=g) * 1e-3
    grad[:, ::13] = 0.0
    grad[0, 7] = float("nan")
    if B > 1:
        grad[1] = 0.0                                                   # a whole row with g = 0
    return [t.to(cuda).contiguous() for t in (x, cur, prev, grad)], eps


@pytest.mark.parametrize("B,T", SHAPES)
@pytest.mark.parametrize("norm", ["Linf", "L2"])
def test_init_kernels(cuda, B, T, norm):
    ops = hip()
    (x, *_), eps = waves(B, T, 1, cuda)
    g = torch.Generator().manual_seed(2)
    draw = torch.rand(B, T, generator=g) if norm == "Linf" else torch.randn(B, T, generator=g)
    draw[0] = 0.5 if norm == "Linf" else 0.0                            # an all-zero t: 0 / 0 as in the reference
    draw = draw.to(cuda)
    got = ops.apgd_init(x, eps, norm, draw=draw)
    want = C.apgd_init(x, eps, norm, draw=draw).cpu()
    again = ops.apgd_init(x, eps, norm, draw=draw)
    assert same(got, again)
    if norm == "Linf":
        assert same(got, want)
        assert torch.isnan(got[0]).all()
    else:
        assert same(torch.isnan(got.cpu()), torch.isnan(want))
        torch.testing.assert_close(got.cpu(), want, atol=L2_ATOL, rtol=0, equal_nan=True)
    seeded = ops.apgd_init(x, eps, norm, seed=1234, offset=3)
    want = C.apgd_init(x, eps, norm, seed=1234, offset=3).cpu()
    assert same(seeded, ops.apgd_init(x, eps, norm, seed=1234, offset=3))
    if norm == "Linf":
        assert same(seeded.cpu(), want)
    else:
        torch.testing.assert_close(seeded.cpu(), want, atol=1e-6 * eps + L2_ATOL, rtol=0)


@pytest.mark.parametrize("B", [1, 5, 128])
def test_eval_and_checkpoint_kernels(cuda, B):
    ops = hip()
    g = torch.Generator().manual_seed(B)
    z = (torch.randn(B, 1, generator=g) * 3).to(cuda)
    z[0, 0] = 0.0
    if B > 2:
        z[1, 0], z[2, 0] = float("nan"), 40.0
    y = torch.randint(0, 2, (B,), generator=g).to(cuda)
    steps = 7
    for mode, i in (("grad", 0), ("start", 0), ("step", 3)):
        st = state(B, steps, 0.003, cuda, B)
        ref = cpu_copy(st)
        dz, loss = ops.apgd_eval(z, y, st, mode, i)
        dz_c, loss_c = C.apgd_eval(z.cpu(), y.cpu(), ref, mode, i)
        # transcendental functions: the device's expf / log1pf against torch's CPU kernels, a few ulp
        torch.testing.assert_close(dz.cpu(), dz_c, rtol=4.8e-7, atol=0, equal_nan=True)
        torch.testing.assert_close(loss.cpu(), loss_c, rtol=4.8e-7, atol=0, equal_nan=True)
        if mode != "grad":
            # the state transition, recomputed on the CPU from the device's own losses, is bit-exact
            ref2 = cpu_copy(state(B, steps, 0.003, "cpu", B))
            if mode == "start":
                C_loss = loss.cpu()
                ref2.acc.copy_(((z.cpu().reshape(-1) > 0).long() == y.cpu()).to(torch.uint8))
                ref2.loss_best.copy_(C_loss), ref2.loss_best_last_check.copy_(C_loss)
                ref2.reduced_last_check.fill_(1), ref2.flags.fill_(0)
            else:
                lv = loss.cpu()
                pred = (z.cpu().reshape(-1) > 0).long() == y.cpu()
                improved = lv > ref2.loss_best
                ref2.acc.copy_(torch.min(ref2.acc, pred.to(torch.uint8)))
                ref2.loss_best.copy_(torch.where(improved, lv, ref2.loss_best))
                ref2.loss_steps[i] = lv
                ref2.flags.copy_((~pred).to(torch.uint8) | (improved.to(torch.uint8) << 1))
            assert same_state(st, ref2), mode
    for i, k in ((0, 1), (3, 4), (6, 3), (6, 7)):
        st = state(B, steps, 0.003, cuda, 100 + i)
        st.loss_steps[2, :] = float("nan")
        ref = cpu_copy(st)
        ops.apgd_checkpoint(st, i, k, 0.75)
        C.apgd_checkpoint(ref, i, k, 0.75)
        assert same_state(st, ref), (i, k)
        again = state(B, steps, 0.003, cuda, 100 + i)
        again.loss_steps[2, :] = float("nan")
        ops.apgd_checkpoint(again, i, k, 0.75)
        assert same_state(st, again)


@pytest.mark.parametrize("B,T", SHAPES)
def test_track_kernel_touches_flagged_rows_only(cuda, B, T):
    ops = hip()
    (x, cur, prev, grad), _ = waves(B, T, 3, cuda)
    sentinel = [torch.full((B, T), v, device=cuda) for v in (7.0, -7.0, 9.0)]
    flags = torch.tensor([f % 8 for f in range(B)], dtype=torch.uint8, device=cuda)   # every flag combination, and none
    bufs = [cur.clone(), grad.clone()] + [s.clone() for s in sentinel]
    ref = [t.clone() for t in bufs]
    ops.apgd_track(*bufs, flags)
    C.apgd_track(*ref, flags)
    for a, b in zip(bufs, ref):
        assert same(a, b)
    none = (flags == 0).cpu()
    for t, s in zip(bufs[2:], sentinel):
        assert same(t.cpu()[none], s.cpu()[none])                # untouched rows keep their bytes


@pytest.mark.parametrize("B,T", SHAPES)
@pytest.mark.parametrize("a", [1.0, 0.75])
def test_linf_step_kernel(cuda, B, T, a):
    ops = hip()
    (x, cur, prev, grad), eps = waves(B, T, 4, cuda)
    step = (torch.rand(B, generator=torch.Generator().manual_seed(5)) * 2 * eps).to(cuda)
    want = C.apgd_linf_step(cur, prev, grad, x, step, eps, a).cpu()
    got = ops.apgd_linf_step(cur, prev, grad, x, step, eps, a)
    assert same(got.cpu(), want)
    p2 = prev.clone()
    ops.apgd_linf_step(cur, p2, grad, x, step, eps, a, out=p2)          # out aliasing prev: the ping-pong form
    assert same(p2, got)
    assert same(got, ops.apgd_linf_step(cur, prev, grad, x, step, eps, a))


@pytest.mark.parametrize("B,T", SHAPES)
@pytest.mark.parametrize("a", [1.0, 0.75])
def test_l2_step_kernel(cuda, B, T, a):
    ops = hip()
    (x, cur, prev, grad), _ = waves(B, T, 6, cuda)
    eps = 0.1
    step = (torch.rand(B, generator=torch.Generator().manual_seed(7)) * 2 * eps).to(cuda)
    got, norms = ops.apgd_l2_step(cur, prev, grad, x, step, eps, a, return_norms=True)
    want, wn = C.apgd_l2_step(cur, prev, grad, x, step, eps, a, return_norms=True)
    assert same(torch.isnan(got.cpu()), torch.isnan(want.cpu()))
    torch.testing.assert_close(got.cpu(), want.cpu(), atol=L2_ATOL, rtol=0, equal_nan=True)
    torch.testing.assert_close(norms.cpu(), wn.cpu(), rtol=1e-5, atol=0, equal_nan=True)
    p2 = prev.clone()
    ops.apgd_l2_step(cur, p2, grad, x, step, eps, a, out=p2)
    assert np.array_equal(p2.cpu().numpy(), got.cpu().numpy(), equal_nan=True)
    d = (got - x).double()
    ok = torch.isfinite(d).all(dim=1)
    assert (d[ok].norm(dim=1) <= eps * (1 + 1e-6)).all()


def l2_step_f64(cur, prev, grad, x, step, eps, a):
    """The L2 step's chain (apgd.py:140-157) in float64 from the float32 inputs, on the CPU."""
    X, Cu, P, G = (t.cpu().double() for t in (x, cur, prev, grad))
    x1 = Cu + step.cpu().double()[:, None] * G / (G.norm(dim=1, keepdim=True) + 1e-12)
    n1 = (x1 - X).norm(dim=1, keepdim=True)
    x1 = (X + (x1 - X) / (n1 + 1e-12) * torch.clamp(n1, max=eps)).clamp(0, 1)
    x2 = Cu + (x1 - Cu) * a + (Cu - P) * (1 - a)
    n2 = (x2 - X).norm(dim=1, keepdim=True)
    return (X + (x2 - X) / (n2 + 1e-12) * torch.clamp(n2 + 1e-12, max=eps)).clamp(0, 1)


def test_l2_step_error_against_float64(cuda):
    """The bound L2_ATOL: the device's and the CPU table's distance from a float64 evaluation of the same chain."""
    ops = hip()
    B, T = 128, 64_600
    (x, cur, prev, grad), _ = waves(B, T, 8, cuda)
    grad[0] = torch.randn(T, device=cuda) * 1e-3                       # keep NaN out of this one
    eps, a = 0.1, 0.75
    step = torch.full((B,), 2 * eps, device=cuda)
    got = ops.apgd_l2_step(cur, prev, grad, x, step, eps, a).cpu().double()
    ref = l2_step_f64(cur, prev, grad, x, step, eps, a)
    cpu = C.apgd_l2_step(cur, prev, grad, x, step, eps, a).cpu().double()
    ok = torch.isfinite(ref)
    err_dev, err_cpu = (got - ref)[ok].abs().max().item(), (cpu - ref)[ok].abs().max().item()
    print(f"L2 step |device - f64| max {err_dev:.3e}, |cpu table - f64| max {err_cpu:.3e}")
    assert err_dev + err_cpu <= L2_ATOL


# ---- whole attacks ---------------------------------------------------------------------------------------------------------

class Recording:
    """hip_ops with every APGD launch recomputed by the CPU table from copies of the launch's own inputs."""

    L2_NAMES = {"apgd_l2_step"}

    def __init__(self, norm):
        self.ops, self.norm, self.calls = hip(), norm, {}

    def __getattr__(self, name):
        fn = getattr(self.ops, name)
        if not name.startswith("apgd_"):
            return fn
        cpu_fn = getattr(C, name)

        def run(*args, **kw):
            self.calls[name] = self.calls.get(name, 0) + 1
            snap_args = [copy.deepcopy(a) if not isinstance(a, torch.Tensor) else a.clone() for a in args]
            snap_kw = {k: (v.clone() if isinstance(v, torch.Tensor) else copy.deepcopy(v)) for k, v in kw.items()}
            res = fn(*args, **kw)
            want = cpu_fn(*snap_args, **snap_kw)
            tol = 0.0
            if name in self.L2_NAMES or (name == "apgd_init" and self.norm == "L2"):
                tol = L2_ATOL
            if name == "apgd_init" and self.norm == "L2" and kw.get("draw") is None:
                # the Philox normals: libm's log / cos / sin here, the device's hardware transcendentals there (~1e-6
                # relative on a normal, scaled by eps / ||t||: below 1e-6 * eps per sample, as test_init_kernels checks)
                tol += 1e-6 * kw.get("eps", args[1] if len(args) > 1 else 0.0)
            if name == "apgd_eval":
                torch.testing.assert_close(res[0], want[0], rtol=4.8e-7, atol=0)
                acc_dev = args[2].acc if len(args) > 2 and args[2] is not None else None
                if acc_dev is not None:
                    assert same(acc_dev.cpu(), snap_args[2].acc.cpu())
            elif name in ("apgd_checkpoint", "apgd_track"):
                for a, b in zip(args, snap_args):
                    if isinstance(a, torch.Tensor):
                        assert same(a, b), name
                    elif hasattr(a, "step_size"):
                        assert same_state(a, b), name
            else:
                if tol:
                    torch.testing.assert_close(res, want, atol=tol, rtol=0)
                else:
                    assert same(res, want), name
            return res
        return run


def detector(name, cuda):
    from audio_deepfake_adversarial_attacks_amd.models.models import get_model
    torch.manual_seed(0)
    if name == "lcnn":
        return get_model("lcnn", {"frontend_algorithm": ["lfcc"], "input_channels": 1}, str(cuda)).to(cuda).eval()
    return get_model("specrnet", {"frontend_algorithm": ["mel_spec"], "input_channels": 2}, str(cuda)).to(cuda).eval()


@pytest.mark.parametrize("model_name", ["lcnn", "specrnet"])
@pytest.mark.parametrize("norm,eps", [("Linf", 0.003), ("L2", 0.1)])
def test_apgd_on_detectors_every_launch_checked(cuda, model_name, norm, eps):
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    from audio_deepfake_adversarial_attacks_amd.datasets.synthetic import synthetic_waveforms
    model = detector(model_name, cuda)
    x, y = synthetic_waveforms(8, seed=31)
    x, y = x.to(cuda), y.to(cuda)
    ops = hip()
    x01, mn, mx = ops.to_minmax(x)
    with torch.no_grad():
        y = (model(x01).reshape(-1) > 0).long()                         # every row starts classified correctly ...
    y[0] = 1 - y[0]                                                     # ... but one
    rec = Recording(norm)
    atk = torchattacks.APGD(model, norm=norm, eps=eps, steps=10)
    atk.set_training_mode(model_training=True, batchnorm_training=False)
    atk.ops = rec
    adv = atk(x01, y)
    assert rec.calls["apgd_linf_step" if norm == "Linf" else "apgd_l2_step"] == 10
    assert rec.calls["apgd_track"] == 10 and rec.calls["apgd_checkpoint"] == 9 and rec.calls["apgd_init"] == 1
    d = (adv - x01).double()
    if norm == "Linf":
        assert d.abs().max().item() <= eps + 2.0 ** -24                  # x +- eps rounds to float32 (half an ulp at 1)
    else:
        assert (d.norm(dim=1) <= eps * (1 + 1e-6)).all()
    assert adv.min() >= 0 and adv.max() <= 1 and adv.data_ptr() != x01.data_ptr()
    with torch.no_grad():
        fooled = (model(adv).reshape(-1) > 0).long() != y
    unchanged = (adv == x01).all(dim=1)
    assert unchanged[0] and (fooled | unchanged).all()                  # rows never fooled equal x bit for bit
    atk2 = torchattacks.APGD(model, norm=norm, eps=eps, steps=10)
    atk2.set_training_mode(model_training=True, batchnorm_training=False)
    assert same(atk2(x01, y), adv)                               # same seed, same bytes


def test_apgd_iteration_loop_never_synchronises(cuda):
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    from audio_deepfake_adversarial_attacks_amd.datasets.synthetic import synthetic_waveforms
    model = detector("lcnn", cuda)
    x, y = synthetic_waveforms(8, seed=32)
    x01, _, _ = hip().to_minmax(x.to(cuda))
    y = y.to(cuda)
    atk = torchattacks.APGD(model, norm="Linf", eps=0.003, steps=6)
    atk.set_training_mode(model_training=True, batchnorm_training=False)
    atk(x01, y)                                                         # warm-up: workspaces, plans, kernels loaded
    seed = atk._fresh_seed()
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            torch.ones(1, device=cuda).item()                           # the mode works on this build
        with atk_call_context(atk):
            acc, adv = atk._single_run(x01, y.long(), seed=seed)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert adv.shape == x01.shape and acc.shape == (8,)


class atk_call_context:
    """What Attack.__call__ does around forward(): train mode with frozen BatchNorm, parameters frozen."""

    def __init__(self, atk):
        self.atk = atk

    def __enter__(self):
        m = self.atk.model
        m.train()
        for mod in m.modules():
            if "BatchNorm" in mod.__class__.__name__ or "Dropout" in mod.__class__.__name__:
                mod.eval()
        self.frozen = [p for p in m.parameters() if p.requires_grad]
        for p in self.frozen:
            p.requires_grad_(False)

    def __exit__(self, *exc):
        for p in self.frozen:
            p.requires_grad_(True)
        self.atk.model.eval()


def test_evaluation_loop_with_apgd(cuda):
    """generate_attacks() with AttackEnum.APGD on synthetic data, as test_evaluation_loop_end_to_end does for PGD."""
    from audio_deepfake_adversarial_attacks_amd.aa.aa_types import AttackEnum
    from audio_deepfake_adversarial_attacks_amd.datasets.synthetic import SyntheticDetectionDataset
    from audio_deepfake_adversarial_attacks_amd.evaluation import generate_attacks
    from audio_deepfake_adversarial_attacks_amd.utils import set_seed
    import yaml
    from tests.conftest import ROOT
    cfg = yaml.safe_load((ROOT / "configs" / "aa_evaluation" / "lcnn.yaml").read_text())
    set_seed(42)
    cls, params = AttackEnum.APGD.value
    rep = generate_attacks([None, None, None], cfg, str(cuda), attack_model_config=cfg, attack_method=cls,
                           attack_params=params, batch_size=8, dataset=SyntheticDetectionDataset(20), share_weights=True)
    assert rep["num_total"] == 16 and 0.0 <= rep["adv_eval/accuracy"] <= 100.0
    set_seed(42)
    clean = generate_attacks([None, None, None], cfg, str(cuda), attack_model_config=None, attack_method=None,
                             batch_size=8, dataset=SyntheticDetectionDataset(20))
    assert rep["adv_eval/accuracy"] <= clean["adv_eval/accuracy"] + 1e-9
