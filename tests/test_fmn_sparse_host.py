"""CPU: host logic of FMNSparse — constructor surface, the registry, argument validation of the entry point of
include/advstep_fmn_sparse.h without a device, every branch of both decisions against hand-written values, and the whole attack
on analytic linear detectors through the CPU table tests/fmn_sparse_cpu_ops.py, where every utterance's minimal L1 norm and
minimal number of changed samples are known in closed form.

Lower bounds are derived.  L0: counts are exact, so last_radius >= the true count and equals #{adv != x}.  L1: LinearDetector
accumulates z in float64, so no flipped iterate lies inside the true radius; what remains is the float32 error of the reported
norm itself: d = fl(adv - x) is within u of adv - x per sample, and the device adds chain(T) = 4 ceil(T / 4096) + 21 times over
non-negative terms (include/advstep_fmn_sparse.h): s = gamma(chain(T) + 1).

Upper bounds are NOT derivable: the dense L2-normalised step projected on a sparse ball does not land on a linear model's
boundary.  MEASURED on these seeds (T = 257 and 4099, K = 100, ten rows, the CPU table): the worst last_radius / true is
1.0035882 for L1 (defaults; per T: 1.0035882, 1.0027282) and 1.4166667 for L0 (gamma_init = 0.3; 7 samples for 5 at T = 257,
17 for 12 at T = 4099).  The tests assert 1 + 2 (worst - 1): 1.0071764 and 1.8333334."""
import ctypes
import math

import pytest
import torch

from tests import fmn_sparse_cpu_ops as C

INF, NAN = math.inf, float("nan")
WORST = {"L1": 1.0035882, "L0": 1.4166667}                      # measured: the docstring
ATTACK_KW = {"L1": {}, "L0": {"gamma_init": 0.3}}                # L1: the defaults; L0: the registry member's gamma_init


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
    assert "FMNSparse" in torchattacks.__all__ and len(set(torchattacks.__all__)) == len(torchattacks.__all__)
    atk = torchattacks.FMNSparse(stub())
    assert str(atk) == ("FMNSparse(model_name=LinearDetector, device=cpu, norm=L1, steps=100, alpha_init=1.0, alpha_final=0.001, "
                        "gamma_init=0.05, gamma_final=0.001, report_at=(), attack_mode=default, return_type=float)")
    assert isinstance(atk, torchattacks.FMN)                      # the schedule, the margin gradient and last_radius are FMN's
    assert atk.replays_from_graph is False and atk._supported_mode == ["default"] and atk.last_radius is None
    assert "last_radius" not in vars(atk) and not hasattr(atk, "last_changed")
    assert atk.schedule(0) == (1.0, 0.05)
    with pytest.raises(ValueError, match="Targeted mode is not supported"):
        atk.set_mode_targeted_by_function(lambda images, labels: 1 - labels)
    custom = torchattacks.FMNSparse(stub(), norm="L0", steps=7, gamma_init=0.3, report_at=[64, 256])
    assert (custom.norm, custom.steps, custom.gamma_init, custom.report_at) == ("L0", 7, 0.3, (64, 256))
    for word in ("DEPARTURES", "exact", "LOWEST", "nobody has measured", "targeted", "restarts", "replay"):
        assert word in torchattacks.FMNSparse.__doc__, word
    # FMN itself: unchanged behaviour, its docstring now points here
    assert str(torchattacks.FMN(stub())).startswith("FMN(model_name=LinearDetector, device=cpu, norm=Linf, steps=60,")
    assert "L1 and L0" in torchattacks.FMN.__doc__ and "FMNSparse" in torchattacks.FMN.__doc__


def test_constructor_refusals():
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    for norm in ("Linf", "L2", "l1", None):
        with pytest.raises(ValueError, match="'L1' or 'L0'"):
            torchattacks.FMNSparse(stub(), norm=norm)
    with pytest.raises(ValueError, match="'Linf' or 'L2'"):      # FMN keeps refusing the sparse norms, with its present message
        torchattacks.FMN(stub(), norm="L1")
    with pytest.raises(ValueError, match="'Linf' or 'L2'"):
        torchattacks.FMN(stub(), norm="L0")
    with pytest.raises(ValueError, match="at least 1"):
        torchattacks.FMNSparse(stub(), steps=0)
    for kw in ({"gamma_init": 0.0}, {"gamma_init": 1.0}, {"gamma_final": -0.1}, {"gamma_init": NAN}):
        with pytest.raises(ValueError, match=r"\(0, 1\)"):
            torchattacks.FMNSparse(stub(), **kw)
    with pytest.raises(ValueError, match="alpha_init"):
        torchattacks.FMNSparse(stub(), alpha_init=-1.0)


def test_registry_members_and_cli():
    import evaluate_models_on_adversarial_attacks as cli
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    from audio_deepfake_adversarial_attacks_amd.aa.aa_types import AttackEnum
    want = {"FMN_L1": {"norm": "L1", "steps": 100, "report_at": (20.0, 30.0, 40.0)},
            "FMN_L0": {"norm": "L0", "steps": 100, "gamma_init": 0.3, "report_at": (64, 256, 1024)}}
    for name, kw in want.items():
        method, params = AttackEnum[name].value
        assert method is torchattacks.FMNSparse and params == kw
        atk = method(stub(), **params)
        assert (atk.norm, atk.steps, atk.report_at, atk.gamma_init) == (kw["norm"], 100, kw["report_at"], kw.get("gamma_init", 0.05))
        assert (atk.alpha_init, atk.alpha_final, atk.gamma_final) == (1.0, 1e-3, 1e-3)
        assert hasattr(atk, "last_radius")                        # what switches the loop's min_radius report on
        assert cli.parse_arguments(["--attack", name]).attack == name
    assert want["FMN_L1"]["report_at"] == tuple(AttackEnum[n].value[1]["eps"] for n in ("APGDL1", "APGDL1_eps30", "APGDL1_eps40"))
    assert want["FMN_L0"]["report_at"] == tuple(AttackEnum[n].value[1]["k"] for n in ("PGDL0", "PGDL0_k256", "PGDL0_k1024"))
    assert len({e.name for e in AttackEnum}) == len(AttackEnum.__members__)        # no member became an alias of another


def test_argument_validation_needs_no_device(lib):
    """Invalid arguments are rejected before any launch (so this is safe without a device)."""
    EINVAL = 1
    P = [ctypes.c_void_p(0x1000000 * (k + 1)) for k in range(10)]    # never dereferenced: validation fails first
    adv, grad, orig, z, y, st_in, st_out, best, out, rn = P
    B, Tn = 2, 8

    def step(adv=adv, grad=grad, orig=orig, z=z, y=y, st_in=st_in, st_out=st_out, best=best, out=out, rn=rn, alpha=0.5, gamma=0.05,
             norm=2, move=1, eps_div=1e-10, B=B, Tn=Tn):
        return lib.advstep_fmn_sparse_step_f32(adv, grad, orig, z, y, st_in, st_out, best, out, rn, alpha, gamma, norm, move, eps_div,
                                               B, Tn, None)

    for missing in ("adv", "grad", "orig", "z", "y", "st_in", "st_out", "best", "out"):
        assert step(**{missing: None}) == EINVAL, missing
    for missing in ("adv", "orig", "z", "y", "st_in", "st_out", "best"):
        assert step(move=0, grad=None, out=None, **{missing: None}) == EINVAL, missing
    assert step(B=-1) == EINVAL and step(Tn=-1) == EINVAL and step(B=65536) == EINVAL and step(Tn=1 << 24) == EINVAL
    for norm in (0, 1, 4, -1):
        assert step(norm=norm) == EINVAL, norm
    for gamma in (0.0, 1.0, -0.5, NAN):
        assert step(gamma=gamma) == EINVAL
    assert step(alpha=-1.0) == EINVAL and step(alpha=NAN) == EINVAL and step(eps_div=-1.0) == EINVAL and step(eps_div=NAN) == EINVAL
    assert step(st_out=st_in) == EINVAL                              # ping-pong: never in place
    assert step(st_out=ctypes.c_void_p(st_in.value + 4 * 4 * B - 4)) == EINVAL
    assert step(best=adv) == EINVAL and step(best=orig) == EINVAL and step(best=grad) == EINVAL and step(best=out) == EINVAL
    assert step(best=st_in) == EINVAL and step(best=st_out) == EINVAL and step(best=z) == EINVAL and step(best=y) == EINVAL
    assert step(st_out=z) == EINVAL and step(st_out=y) == EINVAL and step(st_out=adv) == EINVAL and step(st_out=orig) == EINVAL
    assert step(st_out=grad) == EINVAL
    assert step(out=grad) == EINVAL and step(out=orig) == EINVAL and step(out=st_in) == EINVAL and step(out=st_out) == EINVAL
    assert step(out=z) == EINVAL and step(out=y) == EINVAL and step(out=rn) == EINVAL
    assert step(out=ctypes.c_void_p(adv.value + 4)) == EINVAL        # overlaps adv without being adv
    for clash in (st_in, st_out, z, y, best, adv, orig, grad):
        assert step(rn=clash) == EINVAL
    # The valid forms (out = adv, no row_norms, the last call without gradient and out, whose alpha and eps_div are ignored) pass
    # validation and reach the launch, which has no workspace to fail on first.  These pointers are dummies, so that is only
    # tried where no device can run the launch (it then fails as ELAUNCH = 3); tests/test_gpu_fmn_sparse.py launches every one
    # of these forms on real buffers.
    if lib.advstep_device_count() == 0:
        for status in (step(), step(out=adv), step(rn=None), step(norm=3), step(move=0, grad=None, out=None),
                       step(move=0, grad=None, out=None, alpha=-1.0, eps_div=-1.0)):
            assert status == 3
    assert step(B=0) == 0 and step(Tn=0) == 0 and step(B=0, adv=None, best=None) == 0 and step(Tn=0, adv=None, out=None) == 0
    # FMN's own step keeps refusing the sparse norms
    assert lib.advstep_fmn_step_f32(adv, grad, orig, z, y, st_in, st_out, best, out, rn, 0.5, 0.05, 2, 1, 1e-10, 0.0, 1.0, B, Tn,
                                    ctypes.c_void_p(0x20000000), 1 << 20, None) == EINVAL


def test_wrapper_refuses_cpu_tensors_and_bad_scalars():
    from audio_deepfake_adversarial_attacks_amd import _lib, hip_ops
    x, z = torch.zeros(2, 8), torch.zeros(2)
    y, st = torch.zeros(2, dtype=torch.int64), torch.zeros(4, 2)
    with pytest.raises(_lib.AdvstepError, match="no CPU fallback"):
        hip_ops.fmn_sparse_step(x, x.clone(), x.clone(), z, y, st, x.clone(), 0.5, 0.05, "L1")
    assert hip_ops.FMN_SPARSE_NORMS == C.FMN_SPARSE_NORMS == ("dabs", "dcnt", "gsq", "gmax")
    assert "advstep_fmn_sparse_step_f32" in _lib.SIGNATURES


def table(rows, norm, gamma=0.25, T=100):
    """decide() on hand-written rows (eps, best, found, z, y, dabs, dcnt, gmax)."""
    st = torch.tensor([[r[p] for r in rows] for p in range(3)] + [[0.0] * len(rows)], dtype=torch.float32)
    z = torch.tensor([r[3] for r in rows], dtype=torch.float32)
    y = torch.tensor([r[4] for r in rows])
    n4 = torch.tensor([[r[5] for r in rows], [r[6] for r in rows], [0.0] * len(rows), [r[7] for r in rows]], dtype=torch.float32)
    return C.decide(n4, z, y, st, gamma, norm, T)


def test_cpu_table_covers_every_branch_of_the_l0_decision():
    """gamma = 0.25, T = 100.  begin: inf is read as 1 and grows to 2 | grows by the factor | shrinks to best' | shrinks by the
    factor | shrinks by one | already wrong at begin: 0 | stays 0 (clamped from -1) | clamped at T | NaN logit, y = 1:
    adversarial | NaN logit, y = 0: not adversarial, never found (no reach rule: it grows)."""
    #         eps  best found   z  y dabs dcnt gmax
    rows = [(INF, INF, 0.0, 1.0, 1, 0.0, 0.0, 2.0), (20.0, 30.0, 1.0, 1.0, 1, 0.5, 9.0, 2.0), (20.0, 30.0, 1.0, -1.0, 1, 0.5, 8.0, 2.0),
            (20.0, 17.0, 1.0, -1.0, 1, 0.5, 18.0, 2.0), (2.0, 10.0, 1.0, -1.0, 1, 0.5, 2.0, 2.0), (INF, INF, 0.0, -3.0, 1, 0.0, 0.0, 2.0),
            (0.0, 0.0, 1.0, -3.0, 1, 0.0, 0.0, 2.0), (90.0, 40.0, 1.0, 1.0, 1, 0.5, 90.0, 2.0), (10.0, INF, 0.0, NAN, 1, 0.5, 4.0, 2.0),
            (10.0, INF, 0.0, NAN, 0, 0.5, 4.0, 0.0)]
    copy, new = table(rows, "L0")
    assert copy.tolist() == [False, False, True, False, True, True, False, False, True, False]
    f = torch.float32
    assert torch.equal(new[0], torch.tensor([2.0, 25.0, 8.0, 15.0, 1.0, 0.0, 0.0, 100.0, 4.0, 12.0], dtype=f))
    assert torch.equal(new[1], torch.tensor([INF, 30.0, 8.0, 17.0, 2.0, 0.0, 0.0, 40.0, 4.0, INF], dtype=f))
    assert torch.equal(new[2], torch.tensor([0.0, 1, 1, 1, 1, 1, 1, 1, 1, 0]))
    assert torch.equal(new[3], torch.tensor([r[6] for r in rows], dtype=f))          # dnorm = the count
    # the begin row's next step: 2 -> 3 (2 + 1 beats floor(2.5)); a clamp to a short row
    _, again = table([(2.0, INF, 0.0, 1.0, 1, 0.1, 2.0, 2.0)], "L0")
    assert again[0].tolist() == [3.0]
    _, short = table([(5.0, INF, 0.0, 1.0, 1, 0.1, 5.0, 2.0)], "L0", T=5)
    assert short[0].tolist() == [5.0]


def test_cpu_table_covers_every_branch_of_the_l1_decision():
    """gamma = 0.25.  adversarial and better: shrink | adversarial, not better | found, not adversarial: grow | never found: the
    reach rule with the dual norm max |g| | already wrong at begin | zero gradient: +inf | NaN logit, y = 0 | NaN logit, y = 1."""
    rows = [(0.5, 0.4, 1.0, -1.0, 1, 0.3, 7.0, 2.0), (0.5, 0.2, 1.0, -1.0, 1, 0.3, 7.0, 2.0), (0.5, 0.2, 1.0, 1.0, 1, 0.3, 7.0, 2.0),
            (INF, INF, 0.0, 1.0, 1, 0.25, 7.0, 2.0), (INF, INF, 0.0, -2.0, 1, 0.0, 0.0, 2.0), (INF, INF, 0.0, 1.0, 1, 0.0, 0.0, 0.0),
            (0.5, INF, 0.0, NAN, 0, 0.1, 7.0, 2.0), (0.5, INF, 0.0, NAN, 1, 0.1, 7.0, 2.0)]
    copy, new = table(rows, "L1")
    assert copy.tolist() == [True, False, False, False, True, False, False, True]
    f = torch.float32
    assert torch.equal(new[1], torch.tensor([0.3, 0.2, 0.2, INF, 0.0, INF, INF, 0.1], dtype=f))
    assert torch.equal(new[2], torch.tensor([1.0, 1, 1, 0, 1, 0, 0, 1]))
    want_eps = torch.tensor([0.3 * 0.75, 0.2 * 0.75, 0.5 * 1.25, (0.25 + 0.5) * 1.25, 0.0, INF, NAN, 0.1 * 0.75], dtype=torch.float64)
    torch.testing.assert_close(new[0].double(), want_eps, rtol=2e-7, atol=0, equal_nan=True)
    assert torch.equal(new[3], torch.tensor([r[5] for r in rows], dtype=f))          # dnorm = sum |d|


def test_cpu_table_projects_every_row_into_its_own_radius():
    g = torch.Generator().manual_seed(11)
    x = torch.rand(4, 64, generator=g) * 0.6 + 0.2
    u = x + torch.randn(4, 64, generator=g) * 0.05
    l1 = C.project_rows(x, u, torch.tensor([0.0, 0.1, INF, NAN]), "L1")
    assert torch.equal(l1[0], x[0]) and torch.equal(l1[2], u[2].clamp(0, 1)) and torch.equal(l1[3], u[3].clamp(0, 1))
    assert abs((l1[1] - x[1]).double().abs().sum().item() - 0.1) < 1e-5
    l0 = C.project_rows(x, u, torch.tensor([0.0, 3.0, 64.0, 1000.0]), "L0")
    assert torch.equal(l0[0], x[0]) and (l0[1] != x[1]).sum() == 3 and torch.equal(l0[2], u[2].clamp(0, 1)) and torch.equal(l0[3], l0[3].clamp(0, 1))
    top3 = (u[1] - x[1]).abs().topk(3)[1]
    assert torch.equal(l0[1][top3], u[1][top3])                  # away from the box the score is d^2: the three largest moves


def run_attack(model, x, y, norm, K=100):
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    atk = torchattacks.FMNSparse(model, norm=norm, steps=K, **ATTACK_KW[norm])
    atk.ops = C
    adv = atk(x, y)
    return atk, adv


def check_attack_result(atk, model, x, y, adv, true, norm):
    """Every property asserted of a result on a linear detector; shared with tests/test_gpu_fmn_sparse.py (any device)."""
    radius, adv_c, x_c = atk.last_radius.cpu(), adv.cpu(), x.cpu()
    B, T = x_c.shape
    assert radius.shape == (B,) and radius.dtype == torch.float32
    ratio = radius.double() / true
    print("  true :", [f"{v:.6g}" for v in true.tolist()], "\n  found:", radius.tolist(), "\n  ratio:", [f"{v:.7f}" for v in ratio[1:].tolist()])
    assert not torch.isinf(radius).any() and not torch.isnan(radius).any()     # every row is found
    with torch.no_grad():
        flipped = C.judged_wrong(model(adv).reshape(-1).cpu(), y.cpu())
    assert flipped.all()                                              # every row with a finite radius is flipped by the detector
    assert radius[0] == 0 and torch.equal(adv_c[0], x_c[0])           # the already-wrong row: the clean input, radius 0
    assert adv_c.min() >= 0 and adv_c.max() <= 1
    if norm == "L0":
        assert torch.equal((adv_c != x_c).sum(dim=1).float(), radius)                  # the count is exact
        assert (radius[1:].double() >= true[1:]).all()
    else:
        s = C.gamma_k(C.chain(T) + 1)
        dn = (adv_c.double() - x_c.double()).abs().sum(dim=1)
        assert ((dn - radius.double()).abs() <= s * dn).all()
        assert (radius[1:].double() >= true[1:] * (1 - s)).all()
    bound = 1 + 2 * (WORST[norm] - 1)
    print(f"  worst ratio {ratio[1:].max().item():.7f} (asserted <= {bound:.7f})")
    assert (ratio[1:] <= bound).all()


@pytest.mark.parametrize("T", [257, 4099])
@pytest.mark.parametrize("norm", ["L1", "L0"])
def test_attack_on_linear_detectors_finds_the_closed_form_minima(norm, T):
    """z = x . w + bias_row: the minimal L1 norm of row b is |z_b(x)| / max |w|; its minimal count is the smallest k whose k
    largest gains |w_i| cap_i reach |z_b(x)|.  K = 100."""
    model, flat, x, y, true = C.linear_case(T, norm, seed=T)
    if norm == "L0":                                                  # a condition on the inputs: |z| sits between two sums
        below, above = C.l0_margins(model, x, y)
        assert (below > 0.1 * (below + above)).all() and (above > 0.1 * (below + above)).all()
        assert true.tolist() == [0.0] + [float(k) for k in C.L0_TRUE_K[1:]]
    else:
        assert true[0] == 0 and true[1] > 0.01 and true[-1] == pytest.approx(0.25) and (x >= 0.3).all() and (x <= 0.7).all()
    atk, adv = run_attack(model, x, y, norm)
    check_attack_result(atk, model, x, y, adv, true, norm)
    radius = atk.last_radius.clone()
    again = atk(x, y)                                                 # no random start: the call is a function of its inputs
    assert torch.equal(again, adv) and torch.equal(atk.last_radius, radius)
    # w = 0: no gradient, no move, nothing found — the clean input with +inf
    atk0, adv0 = run_attack(flat, x, y, norm, K=5)
    assert torch.isinf(atk0.last_radius).all() and (atk0.last_radius > 0).all() and torch.equal(adv0, x)
    assert adv0.data_ptr() != x.data_ptr()


def test_the_papers_gamma_reaches_64_late_and_cannot_reach_256_or_1024_in_100_steps():
    """Why FMN_L0 sets gamma_init itself: from the starting radius 1 the integer rule grows by +1 per step while
    floor(eps (1 + gamma)) <= eps + 1, i.e. below eps = 20 at gamma = 0.05, and the cosine schedule lowers gamma as eps grows: 100
    never-adversarial steps end at 101 samples, so a row whose minimum is 64 is first met after 63 of the 100 steps and the
    budgets 256 and 1024 of report_at are out of reach.  gamma_init = 0.3 meets 64 at step 16, 256 at 21 and 1024 at 28."""
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    for gamma_init, want_end, want_reached in ((0.05, 101.0, {64: 63}), (0.3, 64_600.0, {64: 16, 256: 21, 1024: 28})):
        atk = torchattacks.FMNSparse(stub(), norm="L0", steps=100, gamma_init=gamma_init)
        state = C.fmn_begin(B=1)
        reached = {}
        for k in range(100):
            _, state = C.decide(torch.zeros(4, 1), torch.ones(1), torch.ones(1, dtype=torch.int64), state, atk.schedule(k)[1], "L0", 64_600)
            for budget in (64, 256, 1024):
                if state[0].item() >= budget:
                    reached.setdefault(budget, k + 1)
        print(f"  gamma_init {gamma_init}: eps after 100 never-adversarial steps = {state[0].item():g}, budgets first reached at step {reached}")
        assert state[0].item() == want_end and reached == want_reached
