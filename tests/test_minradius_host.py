"""CPU: host logic of MinRadiusPGD — constructor surface, the registry, the run-level digest, argument validation of the four
entry points of include/advstep_radius.h without a device, and the whole search on an analytic linear detector through the
CPU table tests/radius_cpu_ops.py, where every utterance's minimal radius is known in closed form."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import radius_cpu_ops as C

INF = math.inf


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
    assert "MinRadiusPGD" in torchattacks.__all__
    atk = torchattacks.MinRadiusPGD(stub())
    assert str(atk) == ("MinRadiusPGD(model_name=LinearDetector, device=cpu, norm=Linf, eps_max=0.001, search_steps=6, steps=10, "
                        "alpha=None, rel_alpha=0.25, report_at=(), attack_mode=default, return_type=float)")
    assert atk.replays_from_graph is True and atk._supported_mode == ["default"] and atk.last_radius is None
    assert "last_radius" not in vars(atk)                        # a result, not a hyper-parameter
    with pytest.raises(ValueError, match="Targeted mode is not supported"):
        atk.set_mode_targeted_by_function(lambda images, labels: 1 - labels)
    custom = torchattacks.MinRadiusPGD(stub(), norm="L2", eps_max=0.2, search_steps=3, steps=5, alpha=0.01, report_at=[0.1, 0.2])
    assert (custom.alpha, custom.rel_alpha, custom.report_at) == (0.01, None, (0.1, 0.2))
    assert torchattacks.MinRadiusPGD(stub(), rel_alpha=0.5).alpha is None


def test_constructor_refuses_both_step_sizes_and_unknown_norms():
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    with pytest.raises(ValueError, match="not both"):
        torchattacks.MinRadiusPGD(stub(), alpha=0.001, rel_alpha=0.25)
    with pytest.raises(ValueError, match="'Linf' or 'L2'"):
        torchattacks.MinRadiusPGD(stub(), norm="L1")
    with pytest.raises(ValueError, match="eps_max"):
        torchattacks.MinRadiusPGD(stub(), eps_max=-1.0)
    with pytest.raises(ValueError, match="at least 1"):
        torchattacks.MinRadiusPGD(stub(), search_steps=0)


def test_registry_members():
    import evaluate_models_on_adversarial_attacks as cli
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    from audio_deepfake_adversarial_attacks_amd.aa.aa_types import AttackEnum
    want = {"MINRADIUS": {"norm": "Linf", "eps_max": 0.001, "search_steps": 6, "steps": 10, "report_at": (0.0005, 0.00075, 0.001)},
            "MINRADIUS_L2": {"norm": "L2", "eps_max": 0.2, "search_steps": 6, "steps": 10, "report_at": (0.1, 0.15, 0.2)},
            "MINRADIUS40_eps003": {"norm": "Linf", "eps_max": 0.003, "search_steps": 8, "steps": 40}}
    for name, kw in want.items():
        method, params = AttackEnum[name].value
        assert method is torchattacks.MinRadiusPGD and params == kw
        atk = method(stub(), **params)
        assert atk.rel_alpha == 2.5 / kw["steps"] and atk.alpha is None and atk.report_at == kw.get("report_at", ())
        assert cli.parse_arguments(["--attack", name]).attack == name
    # the radii reported are those of the fixed-radius members the search replaces
    assert want["MINRADIUS"]["report_at"] == tuple(AttackEnum[n].value[1]["eps"] for n in ("PGD", "PGD_eps00075", "PGD_eps001"))
    assert want["MINRADIUS_L2"]["report_at"] == tuple(AttackEnum[n].value[1]["eps"] for n in ("PGDL2", "PGDL2_eps15", "PGDL2_eps20"))
    assert len({e.name for e in AttackEnum}) == len(AttackEnum.__members__)
    assert AttackEnum["PGD"].value == (torchattacks.PGD, {"eps": 0.0005, "steps": 10})


def test_radius_summary_on_a_hand_made_vector():
    from audio_deepfake_adversarial_attacks_amd.metrics import radius_summary
    r = np.array([0.0, 0.0, 0.0005, INF, 0.00075, 0.001, INF, 0.00025, 0.0005, INF], dtype=np.float32)
    got = radius_summary(r, (0.0005, 0.00075, 0.001))
    # ascending: 0, 0, .00025, .0005, .0005, .00075, .001, inf, inf, inf; positions 0.9, 4.5, 8.1 of 0 .. 9
    assert got["min_radius/p10"] == pytest.approx(0.0)
    assert got["min_radius/median"] == pytest.approx((0.0005 + 0.00075) / 2, rel=1e-6)
    assert got["min_radius/p90"] == INF
    assert got["min_radius/unflipped_share"] == pytest.approx(0.3) and got["min_radius/already_wrong_share"] == pytest.approx(0.2)
    # strictly above eps, in float32: the three rows AT 0.0005 / 0.00075 / 0.001 are broken at their own radius
    assert got["min_radius/robust_acc@0.0005"] == 50.0       # .00075, .001, inf, inf, inf of ten
    assert got["min_radius/robust_acc@0.00075"] == 40.0      # .001, inf, inf, inf
    assert got["min_radius/robust_acc@0.001"] == pytest.approx(30.0) == pytest.approx(100.0 * got["min_radius/unflipped_share"])
    assert list(got) == ["min_radius/median", "min_radius/p10", "min_radius/p90", "min_radius/unflipped_share",
                         "min_radius/already_wrong_share", "min_radius/robust_acc@0.0005", "min_radius/robust_acc@0.00075",
                         "min_radius/robust_acc@0.001"]
    exact = radius_summary([0.0, 0.25, 0.5, INF, INF], (0.25, 0.5))
    assert exact == {"min_radius/median": 0.5, "min_radius/p10": 0.1, "min_radius/p90": INF, "min_radius/unflipped_share": 0.4,
                     "min_radius/already_wrong_share": 0.2, "min_radius/robust_acc@0.25": 60.0, "min_radius/robust_acc@0.5": 40.0}
    mostly_inf = radius_summary([0.125, INF, INF, INF], ())
    assert mostly_inf["min_radius/median"] == INF and mostly_inf["min_radius/p10"] == INF and mostly_inf["min_radius/p90"] == INF
    assert radius_summary([INF, INF], (1.0,)) == {"min_radius/median": INF, "min_radius/p10": INF, "min_radius/p90": INF,
                                                  "min_radius/unflipped_share": 1.0, "min_radius/already_wrong_share": 0.0,
                                                  "min_radius/robust_acc@1": 100.0}
    assert all(math.isnan(v) for v in radius_summary([], (0.5,)).values())


@pytest.mark.parametrize("member", ["MINRADIUS", "MINRADIUS_L2"])
def test_robust_accuracy_at_the_grid_points_the_search_itself_produces(member):
    """Every default report_at radius is a point of the bisection grid, formed in float32 by the midpoint rule
    0.5f * (lo + hi) from float32(eps_max): eps_max / 2, 3/4 eps_max, eps_max.  Those float32 values lie just above the float64
    literals (float32(0.001) = 0.0010000000475), and a row that flipped AT a radius is not robust at it."""
    from audio_deepfake_adversarial_attacks_amd.aa.aa_types import AttackEnum
    from audio_deepfake_adversarial_attacks_amd.metrics import radius_summary
    kw = AttackEnum[member].value[1]
    top = np.float32(kw["eps_max"])
    half = np.float32(0.5) * (np.float32(0.0) + top)                 # round 1 of a row that flipped at eps_max
    three_q = np.float32(0.5) * (half + top)                         # round 2 of a row that held at eps_max / 2
    eighth5 = np.float32(0.5) * (half + three_q)                     # between the first two report points
    at = kw["report_at"]
    assert float(top) > kw["eps_max"]                                # the float32 point lies above the float64 literal ...
    assert (half, three_q, top) == tuple(np.float32(e) for e in at)   # ... but it IS the float32 of it
    radii = np.array([half, three_q, top], dtype=np.float32)
    got = radius_summary(radii, at)
    assert [got[f"min_radius/robust_acc@{e:g}"] for e in at] == [pytest.approx(200 / 3), pytest.approx(100 / 3), 0.0]
    more = np.array([0.0, half, eighth5, three_q, top, top, math.inf, math.inf], dtype=np.float32)
    got = radius_summary(more, at)
    assert [got[f"min_radius/robust_acc@{e:g}"] for e in at] == [75.0, 50.0, 25.0]
    assert got[f"min_radius/robust_acc@{at[2]:g}"] == 100.0 * got["min_radius/unflipped_share"]   # nothing is robust AT eps_max but the unflipped


def test_cpu_table_agrees_with_the_fixed_radius_steps():
    """With every radius equal and alpha_rel = 0 the per-row steps are the oracle's PGD steps: bit for bit for L-inf, to the
    summation order of the norms for L2."""
    from oracle import torch_ops
    g = torch.Generator().manual_seed(4)
    x = torch.rand(3, 301, generator=g)
    adv = (x + (torch.rand(3, 301, generator=g) * 2 - 1) * 0.01).clamp(0, 1)
    grad = torch.randn(3, 301, generator=g)
    e = torch.full((3,), 0.01)
    assert torch.equal(C.row_pgd_linf_step(adv, grad, x, e, 0.004, 0.0), torch_ops.pgd_linf_step(adv, grad, x, 0.004, 0.01))
    e2 = torch.full((3,), 0.05)
    torch.testing.assert_close(C.row_pgd_l2_step(adv, grad, x, e2, 0.03, 0.0), torch_ops.pgd_l2_step(adv, grad, x, 0.03, 0.05),
                               atol=1e-6, rtol=0)
    # a radius-0 row under a relative step stays where it is (||d|| = 0: no 0 * inf)
    out = C.row_pgd_l2_step(x.clone(), grad, x, torch.tensor([0.0, 0.05, 0.0]), 0.0, 0.25)
    assert torch.equal(out[0], x[0]) and torch.equal(out[2], x[2]) and not torch.isnan(out).any() and not torch.equal(out[1], x[1])


def test_begin_and_round_on_the_cpu_table_cover_every_branch():
    z0 = torch.tensor([0.5, -0.5, 0.0, float("nan"), 2.0])
    y = torch.tensor([1, 1, 0, 1, 0])
    st = C.radius_begin(z0, y, 0.25)
    assert torch.equal(st, torch.tensor([[0.0] * 5, [0.25, 0, 0.25, 0, 0], [0.25, 0, 0.25, 0, 0], [INF, 0, INF, 0, 0]]))
    adv, best_adv = torch.arange(10.0).reshape(5, 2), torch.full((5, 2), -1.0)
    # row 0 flips (z <= 0 against y = 1), row 2 holds, the radius-0 rows 1, 3, 4 stay wrong: nothing
    z = torch.tensor([-1.0, -1.0, -0.0, float("nan"), 1.0])
    st1 = C.radius_round(adv, z, y, True, st, best_adv)
    assert torch.equal(st1, torch.tensor([[0, 0, 0.25, 0, 0], [0.25, 0, 0.25, 0, 0], [0.125, 0, 0.25, 0, 0], [0.25, 0, INF, 0, 0]]))
    assert torch.equal(best_adv, torch.tensor([[0.0, 1.0], [-1, -1], [4.0, 5.0], [-1, -1], [-1, -1]]))
    # second round: row 0 holds at 0.125 (no copy: not first), row 2 flips at eps_max
    adv2 = adv + 100
    st2 = C.radius_round(adv2, torch.tensor([1.0, -1.0, 3.0, float("nan"), 1.0]), y, False, st1, best_adv)
    assert torch.equal(st2, torch.tensor([[0.125, 0, 0.25, 0, 0], [0.25, 0, 0.25, 0, 0], [0.1875, 0, 0.25, 0, 0], [0.25, 0, 0.25, 0, 0]]))
    assert torch.equal(best_adv, torch.tensor([[0.0, 1.0], [-1, -1], [104.0, 105.0], [-1, -1], [-1, -1]]))
    # flipped again at the same radius: eps < best fails, nothing moves
    st3 = C.radius_round(adv, torch.tensor([1.0, -1.0, 3.0, float("nan"), 1.0]), y, False, st2, best_adv)
    assert torch.equal(st3[3], st2[3]) and torch.equal(best_adv[2], torch.tensor([104.0, 105.0]))


def check_search_result(atk, model, x, y, best_adv, radius, expected, true, norm):
    """What the issue asks of a search result: the exact radii, and the invariants of best_adv."""
    radius, best_adv = radius.cpu(), best_adv.cpu()
    print("  true radii:", [f"{v:.6g}" for v in true.tolist()], "\n  found     :", radius.tolist(), "\n  expected  :", expected.tolist())
    assert torch.equal(radius, expected)                            # exactly 0, the grid point above the true radius, or inf
    assert set(torch.isinf(expected).tolist()) == {True, False} and (expected == 0).any() and ((expected > 0) & ~torch.isinf(expected)).any()
    model = model.cpu().eval()
    with torch.no_grad():
        flipped = C.judged_wrong(model(best_adv).reshape(-1), y.cpu())
    finite = ~torch.isinf(radius)
    assert flipped[finite].all() and not flipped[~finite].any()
    d = (best_adv - x.cpu()).double()
    T = x.shape[1]
    for b in torch.nonzero(finite).reshape(-1).tolist():
        if norm == "Linf":
            assert d[b].abs().max().item() <= radius[b].item() + 2.0 ** -23
        else:
            assert d[b].norm().item() <= C.l2_ball_bound(radius[b].item(), T)
    assert torch.equal(best_adv[radius == 0], x.cpu()[radius == 0])  # bit for bit
    assert best_adv.min() >= 0 and best_adv.max() <= 1


@pytest.mark.parametrize("norm", ["Linf", "L2"])
def test_analytic_search_finds_the_exact_grid_points(norm):
    """z = x . w + b_row: the minimal radius of row b is |z_b(x)| / ||w||_1 (L-inf) or / ||w||_2 (L2); with eps_max = 2^-6 every
    midpoint of the bisection is exact in float32, so `last_radius` is 0, the smallest grid point above the true radius, or inf."""
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    eps_max, S, steps = 2.0 ** -6, 5, 4
    model, x, y, true, expected = C.analytic_case(8, 37, norm, eps_max, S, seed=7)
    atk = torchattacks.MinRadiusPGD(model, norm=norm, eps_max=eps_max, search_steps=S, steps=steps)
    assert atk.rel_alpha * steps >= 1
    atk.ops = C
    best_adv = atk(x, y)
    check_search_result(atk, model, x, y, best_adv, atk.last_radius, expected, true, norm)
    again = atk(x, y)                                                # no random start: the call is a function of its inputs
    assert torch.equal(again, best_adv) and torch.equal(atk.last_radius, expected)
    assert atk.last_radius.shape == (8,) and atk.last_radius.dtype == torch.float32


def test_absolute_step_size_also_resolves_the_radii():
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    eps_max, S = 2.0 ** -6, 4
    model, x, y, true, expected = C.analytic_case(5, 20, "Linf", eps_max, S, seed=3)
    atk = torchattacks.MinRadiusPGD(model, eps_max=eps_max, search_steps=S, steps=4, alpha=eps_max / 2)   # 4 * alpha >= every radius
    atk.ops = C
    best_adv = atk(x, y)
    check_search_result(atk, model, x, y, best_adv, atk.last_radius, expected, true, "Linf")


def test_training_flags_come_back_exactly():
    """The judge runs the model in eval mode; afterwards every module has the flag it had (they are part of the graph key)."""
    from audio_deepfake_adversarial_attacks_amd import torchattacks

    class Net(C.LinearDetector):
        def __init__(self, w, b):
            super().__init__(w, b)
            self.drop, self.norm = torch.nn.Dropout(0.0), torch.nn.BatchNorm1d(1)
            self.seen = []

        def forward(self, x):
            self.seen.append((self.training, self.drop.training, self.norm.training))
            return super().forward(x)

    model, x, y, _, _ = C.analytic_case(4, 12, "Linf", 2.0 ** -6, 3)
    net = Net(model.w.data, model.bias)
    net.train()
    net.norm.eval()                                                 # the mix Attack.__call__ leaves: BatchNorm frozen, the rest training
    before = [m.training for m in net.modules()]
    atk = torchattacks.MinRadiusPGD(net, eps_max=2.0 ** -6, search_steps=3, steps=2)
    atk.ops = C
    atk.forward(x, y)
    assert [m.training for m in net.modules()] == before == [True, True, False]
    # the clean judge, then per round: `steps` attack passes under the caller's flags and one judge pass in eval mode
    per_round = [(True, True, False)] * 2 + [(False, False, False)]
    assert net.seen == [(False, False, False)] + per_round * 3


def test_argument_validation_needs_no_device(lib):
    """Invalid arguments are rejected before any launch (so this is safe without a device)."""
    EINVAL, EWORKSPACE = 1, 2
    P = [ctypes.c_void_p(0x100000 * (k + 1)) for k in range(10)]    # never dereferenced: validation fails first
    adv, grad, orig, eps, out, gn, dn, ws, st_in, st_out = P
    B, Tn = 2, 8
    need = lib.advstep_row_workspace_bytes(B, Tn)

    def linf(adv=adv, grad=grad, orig=orig, eps=eps, out=out, B=B, Tn=Tn):
        return lib.advstep_row_pgd_linf_step_f32(adv, grad, orig, eps, 0.0, 0.25, 0.0, 1.0, out, B, Tn, None)

    for missing in ("adv", "grad", "orig", "eps", "out"):
        assert linf(**{missing: None}) == EINVAL
    assert linf(B=-1) == EINVAL and linf(Tn=-1) == EINVAL and linf(B=65536) == EINVAL
    assert linf(out=grad) == EINVAL and linf(out=orig) == EINVAL and linf(out=eps) == EINVAL
    assert linf(out=ctypes.c_void_p(adv.value + 4)) == EINVAL       # overlaps adv without being adv
    assert linf(B=0, adv=None, grad=None, orig=None, eps=None, out=None) == 0 and linf(Tn=0) == 0

    def l2(adv=adv, grad=grad, orig=orig, eps=eps, out=out, gn=gn, dn=dn, B=B, Tn=Tn, ws=ws, ws_bytes=need):
        return lib.advstep_row_pgd_l2_step_f32(adv, grad, orig, eps, 0.0, 0.25, 1e-10, 0.0, 1.0, out, gn, dn, B, Tn, ws, ws_bytes, None)

    for missing in ("adv", "grad", "orig", "eps", "out"):
        assert l2(**{missing: None}) == EINVAL
    assert l2(B=-1) == EINVAL and l2(B=65536) == EINVAL and l2(out=grad) == EINVAL and l2(out=orig) == EINVAL
    assert l2(gn=out) == EINVAL and l2(dn=out) == EINVAL
    assert l2(ws=None) == EWORKSPACE and l2(ws_bytes=need - 1) == EWORKSPACE and l2(ws=ctypes.c_void_p(ws.value + 4)) == EWORKSPACE
    assert l2(out=adv, gn=None, dn=None, ws_bytes=0) == EWORKSPACE  # out = adv and absent norms are valid: the workspace is what fails
    assert l2(B=0, ws=None, ws_bytes=0) == 0 and l2(Tn=0, ws=None, ws_bytes=0) == 0

    z, y = grad, orig
    assert lib.advstep_radius_begin_f32(None, y, 0.1, st_in, B, None) == EINVAL
    assert lib.advstep_radius_begin_f32(z, None, 0.1, st_in, B, None) == EINVAL
    assert lib.advstep_radius_begin_f32(z, y, 0.1, None, B, None) == EINVAL
    assert lib.advstep_radius_begin_f32(z, y, -0.1, st_in, B, None) == EINVAL
    assert lib.advstep_radius_begin_f32(z, y, float("nan"), st_in, B, None) == EINVAL
    assert lib.advstep_radius_begin_f32(z, y, 0.1, z, B, None) == EINVAL and lib.advstep_radius_begin_f32(z, y, 0.1, st_in, -1, None) == EINVAL
    assert lib.advstep_radius_begin_f32(None, None, 0.1, None, 0, None) == 0

    def rnd(adv=adv, z=z, y=y, st_in=st_in, st_out=st_out, best=out, B=B, Tn=Tn):
        return lib.advstep_radius_round_f32(adv, z, y, 1, st_in, st_out, best, B, Tn, None)

    for missing in ("adv", "z", "y", "st_in", "st_out", "best"):
        assert rnd(**{missing: None}) == EINVAL
    assert rnd(st_out=st_in) == EINVAL                              # ping-pong: never in place
    assert rnd(st_out=ctypes.c_void_p(st_in.value + 4 * 4 * B - 4)) == EINVAL
    assert rnd(best=adv) == EINVAL and rnd(best=st_in) == EINVAL and rnd(best=st_out) == EINVAL and rnd(st_out=z) == EINVAL
    assert rnd(B=-1) == EINVAL and rnd(Tn=-1) == EINVAL and rnd(B=65536) == EINVAL
    assert rnd(B=0) == 0 and rnd(Tn=0) == 0


def test_wrappers_refuse_cpu_tensors():
    from audio_deepfake_adversarial_attacks_amd import _lib, hip_ops
    x, e = torch.zeros(2, 8), torch.zeros(2)
    y, st = torch.zeros(2, dtype=torch.int64), torch.zeros(4, 2)
    with pytest.raises(_lib.AdvstepError, match="no CPU fallback"):
        hip_ops.row_pgd_linf_step(x, x.clone(), x.clone(), e, 0.0, 0.25)
    with pytest.raises(_lib.AdvstepError, match="no CPU fallback"):
        hip_ops.row_pgd_l2_step(x, x.clone(), x.clone(), e, 0.0, 0.25)
    with pytest.raises(_lib.AdvstepError, match="no CPU fallback"):
        hip_ops.radius_begin(e, y, 0.1)
    with pytest.raises(_lib.AdvstepError, match="no CPU fallback"):
        hip_ops.radius_round(x, e, y, True, st, x.clone())
