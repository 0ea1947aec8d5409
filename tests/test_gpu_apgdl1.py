"""`-m gpu`: the l1-APGD kernels (include/advstep_apgdl1.h) against the CPU table tests/apgdl1_cpu_ops.py on identical inputs,
and whole APGDL1 attacks on the detectors with every launch recomputed on the CPU table from its own inputs.

What is bit-exact and what is not.  The top-k threshold, the count, the selected set and every field of the checkpoint are
integer or selection results: bit-exact.  The projection's multiplier lambda* is the smallest float32 with phi(lambda*) <= eps
where phi is a float32 sum of T terms, which the device (1024 per-thread partial sums, wave64 trees) and torch's CPU kernels
associate differently; the two lambda* differ by the rounding of that sum spread over the active coordinates.

Measured on gfx950 by test_error_against_float64 (float64 restatement of the same definitions, (3, 64 600) rows):
    projection   |device - f64| max 1.46e-7, |cpu table - f64| max 1.46e-7   (the rounding of |d| - lambda at |d| ~ 4)
    step         |device - f64| max 4.2e-8,  |cpu table - f64| max 4.2e-8
    ||out - x||_1 / eps - 1 in float64: device 1.63e-5, cpu table 1.62e-5 there; the table's largest over the inputs of these
    tests and of tests/test_apgdl1_host.py is 3.7e-5, on the tie input: every sample moves by the SAME m, so x + m rounds to
    float32 the same way 64 600 times (at most 2^-25 T / eps = 9.6e-5 for x in [0.5, 1)) - a property of the output format
    that any implementation shares, the float64 solution rounded to float32 included.
    |device - cpu table| seen: 3.7e-9.
L1_ATOL is 4x the larger sum of a device and a table figure (both sides re-associate a 64 600-term sum in their own order:
hence the factor).  L1_SLACK is 4x the table's excess, capped at 1e-4: past that the search would be wrong, not the rounding."""
import copy

import pytest
import torch

from tests import apgdl1_cpu_ops as C
from tests.test_gpu_apgd import atk_call_context, detector, hip, same, same_state

pytestmark = pytest.mark.gpu

SHAPES = [(1, 257), (5, 4099), (3, 64_600)]
T_FULL = 64_600
L1_ATOL = 4 * (1.46e-7 + 1.46e-7)          # per sample, |device - cpu table|
L1_SLACK = min(4 * 3.7e-5, 1e-4)           # on ||out - x||_1 / eps - 1


def eps_for(T):
    """The registry's radius at the repo's row length, scaled to the row: the same mean |delta| per sample."""
    return 20.0 * T / T_FULL


def box_rows(B, T, seed):
    """x in [0, 1] with exact 0s and 1s; away from them x >= 0.01, so x + (u - x) == u bit for bit when |u - x| is small."""
    g = torch.Generator().manual_seed(seed)
    x = 0.01 + 0.98 * torch.rand(B, T, generator=g)
    x[:, ::17] = 0.0
    x[:, 5::19] = 1.0
    return x, g


def projection_inputs(B, T, seed, first_case=0):
    """(x, u, case per row): 0 = x + N(0, 1); 1 = a 20 %-sparse sign step of size eps plus 3e-4 noise; 2 = a point of the box
    within 1e-4 N(0, 1) of x (phi(0) < eps: the projection is the identity); 3 = x +- 0.01 everywhere, the tie input that
    defeats a Newton iteration from lambda = 0."""
    x, g = box_rows(B, T, seed)
    eps = eps_for(T)
    u = torch.empty(B, T)
    cases = [(first_case + r) % 4 for r in range(B)]
    for r, case in enumerate(cases):
        noise = torch.randn(T, generator=g)
        if case == 0:
            u[r] = x[r] + noise
        elif case == 1:
            sel = torch.rand(T, generator=g) < 0.2
            step = torch.where(sel, torch.sign(torch.randn(T, generator=g)), torch.zeros(T)) * (eps / sel.sum())
            u[r] = x[r] + step + 3e-4 * noise
        elif case == 2:
            u[r] = (x[r] + 1e-4 * noise).clamp(0.0, 1.0)
        else:
            u[r] = x[r] + 0.01 * torch.sign(noise)
    return x, u, cases


def step_inputs(B, T, seed):
    """x with exact 0s and 1s, a current point in the box, gradients with zeros and a NaN, a whole zero-gradient row (row 1)
    and a tie row (the last of B > 2: equal |g| everywhere, cur = x), per-row step sizes and top-k fractions."""
    x, g = box_rows(B, T, seed)
    eps = eps_for(T)
    cur = (x + torch.randn(B, T, generator=g) * (torch.rand(B, T, generator=g) < 0.1) * 1e-3).clamp(0.0, 1.0)
    grad = torch.randn(B, T, generator=g) * 1e-3
    grad[:, ::13] = 0.0
    grad[0, 7] = float("nan")
    if B > 1:
        grad[1] = 0.0
    if B > 2:
        grad[-1] = 1e-3 * torch.sign(torch.randn(T, generator=g))
        cur[-1] = x[-1]
    topk = torch.tensor([0.2, 0.0, 1.0, 1.0 / 1.5 / T, 0.05])[torch.arange(B) % 5]
    step = torch.tensor([1.0, 0.5, 2.0, 0.1, 1.0])[torch.arange(B) % 5] * eps
    if B > 2:
        topk[-1], step[-1] = 0.2, 2 * eps
    return x, cur, grad, step.contiguous(), topk.contiguous(), eps


def with_canary(t, cuda):
    """A device copy of t followed in the same allocation by a canary row."""
    buf = torch.full((t.shape[0] + 1, t.shape[1]), 7.0, device=cuda)
    buf[:-1] = t.to(cuda)
    return buf[:-1], buf[-1]


def l1_excess(out, x, eps):
    """max over the rows of ||out - x||_1 / eps - 1, in float64."""
    return ((out.double().cpu() - x.double().cpu()).abs().sum(dim=1) / eps - 1).max().item()


def check_box(out):
    assert out.min() >= 0 and out.max() <= 1 and torch.isfinite(out).all()


@pytest.mark.parametrize("B,T", SHAPES)
def test_projection_kernel(cuda, B, T):
    ops, eps = hip(), eps_for(T)
    for first_case in range(4):
        x, u, cases = projection_inputs(B, T, 10 + first_case, first_case)
        xd, ud = x.to(cuda), u.to(cuda)
        out, canary = with_canary(torch.zeros(B, T), cuda)
        got = ops.l1_box_project(xd, ud, eps, out=out)
        assert got.data_ptr() == out.data_ptr() and (canary == 7.0).all()
        want = C.l1_box_project(x, u, eps)
        assert same(got, ops.l1_box_project(xd, ud, eps))                       # a rerun is bit-identical
        alias = ud.clone()
        ops.l1_box_project(xd, alias, eps, out=alias)                           # out aliasing u
        assert same(alias, got)
        check_box(got)
        torch.testing.assert_close(got.cpu(), want, atol=L1_ATOL, rtol=0)
        assert l1_excess(got, x, eps) <= L1_SLACK
        for r, case in enumerate(cases):
            if case == 2:
                assert same(got[r], u[r])                                       # already feasible: untouched


@pytest.mark.parametrize("B,T", SHAPES)
def test_step_kernel(cuda, B, T):
    ops = hip()
    x, cur, grad, step, topk, eps = step_inputs(B, T, 20)
    xd, cd, gd, sd, td = (t.to(cuda) for t in (x, cur, grad, step, topk))
    out, canary = with_canary(torch.zeros(B, T), cuda)
    got, stats = ops.apgdl1_step(cd, gd, xd, sd, td, eps, out=out, return_stats=True)
    assert (canary == 7.0).all()
    want, wstats = C.apgdl1_step(cur, grad, x, step, topk, eps, return_stats=True)
    assert same(stats, wstats)                                                  # threshold and count: bit-exact
    cnt = wstats[:, 1]
    assert cnt[0] > 0 and (B < 2 or cnt[1] == 0) and (B < 3 or cnt[-1] == T)    # the zero row, the all-equal row
    check_box(got)
    torch.testing.assert_close(got.cpu(), want, atol=L1_ATOL, rtol=0)
    assert l1_excess(got, x, eps) <= L1_SLACK
    if B > 1:
        assert same(got[1], cur[1])                     # cnt = 0: the projection of cur itself, which is feasible already
    assert same(got, ops.apgdl1_step(cd, gd, xd, sd, td, eps))                  # a rerun is bit-identical
    alias = cd.clone()
    ops.apgdl1_step(alias, gd, xd, sd, td, eps, out=alias)                      # out aliasing cur: the attack's form
    assert same(alias, got)


@pytest.mark.parametrize("B,T", SHAPES)
def test_init_kernel(cuda, B, T):
    ops, eps = hip(), eps_for(T)
    x, g = box_rows(B, T, 30)
    draw = torch.randn(B, T, generator=g)
    xd, dd = x.to(cuda), draw.to(cuda)
    out, canary = with_canary(torch.zeros(B, T), cuda)
    got = ops.apgdl1_init(xd, eps, draw=dd, out=out)
    assert (canary == 7.0).all()
    want = C.apgdl1_init(x, eps, draw=draw)
    check_box(got)
    torch.testing.assert_close(got.cpu(), want, atol=L1_ATOL, rtol=0)
    assert l1_excess(got, x, eps) <= L1_SLACK
    assert same(got, ops.apgdl1_init(xd, eps, draw=dd))
    alias = dd.clone()
    ops.apgdl1_init(xd, eps, draw=alias, out=alias)                             # out aliasing the draw
    assert same(alias, got)
    # the Philox normals: libm's log / cos / sin in the table, the device's hardware transcendentals (~1e-6 relative on a
    # normal t, tests/test_gpu_apgd.py).  A sample moves by its own 1e-6 |t_i| and by lambda*'s shift, which is at most the
    # largest shift of an active coordinate, 1e-6 max_row |t|
    out, canary = with_canary(torch.zeros(B, T), cuda)
    seeded = ops.apgdl1_init(xd, eps, seed=1234, offset=3, out=out)
    assert (canary == 7.0).all()
    t = C.philox_draw(B, T, "L2", 1234, 3)
    want = C.apgdl1_init(x, eps, seed=1234, offset=3)
    allow = L1_ATOL + 1e-6 * (t.abs() + t.abs().max(dim=1, keepdim=True)[0])
    assert ((seeded.cpu() - want).abs() <= allow).all()
    check_box(seeded)
    assert same(seeded, ops.apgdl1_init(xd, eps, seed=1234, offset=3))
    assert not same(seeded, ops.apgdl1_init(xd, eps, seed=1234, offset=4))


def l1_state(B, T, eps, device):
    from audio_deepfake_adversarial_attacks_amd.torchattacks.attacks.apgdl1 import ApgdL1State
    return ApgdL1State.new(B, 4, eps, device, T)


@pytest.mark.parametrize("B,T", SHAPES)
def test_checkpoint_kernel(cuda, B, T):
    ops, eps = hip(), eps_for(T)
    x, g = box_rows(B, T, 40)
    cur = torch.where(torch.rand(B, T, generator=g) < 0.3, torch.rand(B, T, generator=g), x)
    best = torch.where(torch.rand(B, T, generator=g) < 0.1, torch.rand(B, T, generator=g), x)
    cur[0, 3] = float("nan")
    for variant in range(4):
        st = l1_state(B, T, eps, "cpu")
        st.flags.copy_((torch.arange(B) + 2 * variant) % 8)                      # every flag combination
        sp = torch.where(((st.flags & 2) != 0)[:, None], cur, best).sub(x).ne(0).sum(dim=1).float()
        st.sp_old.copy_([sp / 0.94, sp / 0.96, sp, torch.full((B,), float(T))][variant])   # either side of 0.95
        st.step_size.copy_(torch.tensor([1.0, 0.12, 2.0, 0.5])[(torch.arange(B) + variant) % 4] * eps)   # 2.0 / 1.5 and 0.12 / 1.5: both clamps
        padded = {k: torch.cat([v, torch.full_like(v[:1], 7)]).to(cuda) for k, v in st.__dict__.items() if v.dim() == 1}
        dev = type(st)(**{k: (padded[k][:-1] if k in padded else v.to(cuda)) for k, v in st.__dict__.items()})
        again = type(st)(**{k: v.to(cuda) for k, v in st.__dict__.items()})
        ops.apgdl1_checkpoint(cur.to(cuda), best.to(cuda), x.to(cuda), dev, eps)
        C.apgdl1_checkpoint(cur, best, x, st, eps)
        assert same_state(dev, st), variant                                      # every field, bit for bit
        assert all(v[-1] == 7 for v in padded.values())                          # the element after each (B) array: untouched
        assert same(st.sp_old, sp) and ((st.flags & 4) != 0).tolist() == [variant in (0, 3)] * B
        ops.apgdl1_checkpoint(cur.to(cuda), best.to(cuda), x.to(cuda), again, eps)
        assert same_state(dev, again)


def project_f64(x, u, eps):
    """The projection's definition in float64 with a real-valued lambda (interval halving to machine precision)."""
    x, u = x.double(), u.double()
    d = u - x
    ad, cap = d.abs(), torch.where(d > 0, 1.0 - x, x)

    def moves(lam):
        return torch.minimum(torch.clamp(ad - lam[:, None], min=0.0), cap)
    lo, hi = torch.zeros(x.shape[0], dtype=torch.float64), ad.max(dim=1)[0]
    feasible = moves(lo).sum(dim=1) <= eps
    for _ in range(100):
        mid = (lo + hi) / 2
        over = moves(mid).sum(dim=1) > eps
        lo, hi = torch.where(over, mid, lo), torch.where(over, hi, mid)
    lam = torch.where(feasible, torch.zeros_like(hi), hi)
    return (x + torch.sign(d) * moves(lam)).clamp(0.0, 1.0)


def test_error_against_float64(cuda):
    """The bounds L1_ATOL and L1_SLACK: the device's and the CPU table's distance from a float64 evaluation of the same
    definitions, on the real row length."""
    ops = hip()
    B, T = 3, T_FULL
    eps = eps_for(T)
    x, u, _ = projection_inputs(B, T, 50, first_case=0)
    u[2] = x[2] + 0.01 * torch.sign(torch.randn(T, generator=torch.Generator().manual_seed(52)))   # rows: N(0, 1), sparse step, tie
    ref = project_f64(x, u, eps)
    dev, cpu = ops.l1_box_project(x.to(cuda), u.to(cuda), eps).cpu(), C.l1_box_project(x, u, eps)
    p_dev, p_cpu = (dev.double() - ref).abs().max().item(), (cpu.double() - ref).abs().max().item()
    e_dev, e_cpu = l1_excess(dev, x, eps), l1_excess(cpu, x, eps)
    print(f"L1 projection |device - f64| max {p_dev:.3e}, |cpu table - f64| max {p_cpu:.3e}; "
          f"L1 / eps - 1: device {e_dev:.3e}, cpu table {e_cpu:.3e}, f64 {l1_excess(ref, x, eps):.3e}")
    x, cur, grad, step, topk, eps = step_inputs(B, T, 51)
    _, _, s, cnt = C.topk_threshold(grad, topk)
    u64 = cur.double() + step.double()[:, None] * s.double() / (cnt.double()[:, None] + 1e-10)
    ref = project_f64(x, u64, eps)
    dev = ops.apgdl1_step(*(t.to(cuda) for t in (cur, grad, x, step, topk)), eps).cpu()
    cpu = C.apgdl1_step(cur, grad, x, step, topk, eps)
    s_dev, s_cpu = (dev.double() - ref).abs().max().item(), (cpu.double() - ref).abs().max().item()
    e_dev, e_cpu = max(e_dev, l1_excess(dev, x, eps)), max(e_cpu, l1_excess(cpu, x, eps))
    print(f"L1 step |device - f64| max {s_dev:.3e}, |cpu table - f64| max {s_cpu:.3e}; "
          f"L1 / eps - 1 over both: device {e_dev:.3e}, cpu table {e_cpu:.3e}")
    assert max(p_dev + p_cpu, s_dev + s_cpu) <= L1_ATOL
    assert e_dev <= L1_SLACK and e_cpu <= L1_SLACK
    assert L1_SLACK <= 1e-4                                                      # looser would mean a wrong search, not rounding


# ---- whole attacks ---------------------------------------------------------------------------------------------------------

class Recording:
    """hip_ops with every l1-APGD launch (apgdl1_*, apgd_eval, apgd_track) recomputed by the CPU table from copies of the
    launch's own inputs."""

    def __init__(self):
        self.ops, self.calls = hip(), {}

    def __getattr__(self, name):
        fn = getattr(self.ops, name)
        if not name.startswith("apgd"):
            return fn
        cpu_fn = getattr(C, name)

        def run(*args, **kw):
            self.calls[name] = self.calls.get(name, 0) + 1
            snap_args = [a.clone() if isinstance(a, torch.Tensor) else copy.deepcopy(a) for a in args]
            snap_kw = {k: (v.clone() if isinstance(v, torch.Tensor) else copy.deepcopy(v)) for k, v in kw.items()}
            res = fn(*args, **kw)
            want = cpu_fn(*snap_args, **snap_kw)
            if name == "apgd_eval":
                torch.testing.assert_close(res[0], want[0], rtol=4.8e-7, atol=0)
                if len(args) > 2 and args[2] is not None:
                    assert same(args[2].acc, snap_args[2].acc)
            elif name in ("apgdl1_checkpoint", "apgd_track"):
                for a, b in zip(args, snap_args):
                    if isinstance(a, torch.Tensor):
                        assert same(a, b), name
                    elif hasattr(a, "step_size"):
                        assert same_state(a, b), name
            else:
                tol = L1_ATOL
                if name == "apgdl1_init" and kw.get("draw") is None:
                    t = C.philox_draw(args[0].shape[0], args[0].shape[1], "L2", kw["seed"], kw.get("offset", 0))
                    tol = tol + 1e-6 * 2 * t.abs().max().item()                  # the Philox allowance of test_init_kernel
                torch.testing.assert_close(res, want, atol=tol, rtol=0)
            return res
        return run


def attack_inputs(model, cuda, seed):
    from audio_deepfake_adversarial_attacks_amd.datasets.synthetic import synthetic_waveforms
    x, y = synthetic_waveforms(8, seed=seed)
    x01, _, _ = hip().to_minmax(x.to(cuda))
    with torch.no_grad():
        y = (model(x01).reshape(-1) > 0).long()                                 # every row starts classified correctly ...
    y[0] = 1 - y[0]                                                             # ... but one
    return x01, y


@pytest.mark.parametrize("model_name", ["lcnn", "specrnet"])
def test_apgdl1_on_detectors_every_launch_checked(cuda, model_name):
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    model = detector(model_name, cuda)
    x01, y = attack_inputs(model, cuda, 33)
    eps = 20.0
    rec = Recording()
    atk = torchattacks.APGDL1(model, eps=eps, steps=10)
    atk.set_training_mode(model_training=True, batchnorm_training=False)
    atk.ops = rec
    adv = atk(x01, y)
    assert rec.calls == {"apgdl1_init": 1, "apgd_eval": 11, "apgdl1_step": 10, "apgdl1_checkpoint": 10, "apgd_track": 10}
    assert l1_excess(adv, x01, eps) <= L1_SLACK
    assert adv.min() >= 0 and adv.max() <= 1 and adv.data_ptr() != x01.data_ptr()
    with torch.no_grad():
        fooled = (model(adv).reshape(-1) > 0).long() != y
    unchanged = (adv == x01).all(dim=1)
    assert unchanged[0] and (fooled | unchanged).all()                          # rows never fooled equal x bit for bit
    atk2 = torchattacks.APGDL1(model, eps=eps, steps=10)
    atk2.set_training_mode(model_training=True, batchnorm_training=False)
    assert same(atk2(x01, y), adv)                                              # same seed, same bytes


def test_apgdl1_iteration_loop_never_synchronises(cuda):
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    model = detector("lcnn", cuda)
    x01, y = attack_inputs(model, cuda, 34)
    atk = torchattacks.APGDL1(model, eps=20.0, steps=6)
    atk.set_training_mode(model_training=True, batchnorm_training=False)
    atk(x01, y)                                                                 # warm-up: plans, kernels loaded
    seed = atk._fresh_seed()
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            torch.ones(1, device=cuda).item()                                   # the mode works on this build
        with atk_call_context(atk):
            acc, adv = atk._single_run(x01, y.long(), seed=seed)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert adv.shape == x01.shape and acc.shape == (8,)


def _evaluate_synthetic(cuda, member):
    """generate_attacks() on SyntheticDetectionDataset(20) with an AttackEnum member (None: no attack), as
    test_evaluation_loop_with_apgd runs it for APGD."""
    import yaml

    from audio_deepfake_adversarial_attacks_amd.aa.aa_types import AttackEnum
    from audio_deepfake_adversarial_attacks_amd.datasets.synthetic import SyntheticDetectionDataset
    from audio_deepfake_adversarial_attacks_amd.evaluation import generate_attacks
    from audio_deepfake_adversarial_attacks_amd.utils import set_seed
    from tests.conftest import ROOT
    cfg = yaml.safe_load((ROOT / "configs" / "aa_evaluation" / "lcnn.yaml").read_text())
    set_seed(42)
    if member is None:
        return generate_attacks([None, None, None], cfg, str(cuda), attack_model_config=None, attack_method=None,
                                batch_size=8, dataset=SyntheticDetectionDataset(20))
    cls, params = AttackEnum[member].value
    return generate_attacks([None, None, None], cfg, str(cuda), attack_model_config=cfg, attack_method=cls,
                            attack_params=params, batch_size=8, dataset=SyntheticDetectionDataset(20), share_weights=True)


@pytest.fixture(scope="module")
def clean_report(cuda):
    """The unattacked run, once for both members."""
    return _evaluate_synthetic(cuda, None)


@pytest.mark.parametrize("member", ["APGDL1", "WORSTCASE_L1"])
def test_evaluation_loop_with_l1_members(cuda, clean_report, member):
    rep = _evaluate_synthetic(cuda, member)
    assert rep["num_total"] == 16 and 0.0 <= rep["adv_eval/accuracy"] <= 100.0
    assert rep["adv_eval/accuracy"] <= clean_report["adv_eval/accuracy"] + 1e-9
