"""CPU: host logic of FMN — constructor surface, the registry, the schedules, argument validation of the entry points of
include/advstep_fmn.h without a device, and the whole attack on analytic linear detectors through the CPU table
tests/fmn_cpu_ops.py, where every utterance's minimal norm is known in closed form."""
import ctypes
import math

import pytest
import torch

from tests import fmn_cpu_ops as C

INF = math.inf
# The lower bound's slack.  Twice the worst shortfall of `last_radius` below the true radius that the CPU twin shows on these
# seeds would be the figure; the twin shows NONE (both norms, T = 257 and 4099, K = 100: the smallest last_radius / r is
# 1.0000144, the largest 1.000127): LinearDetector accumulates z in float64, so the sign of z is the exact one and no flipped
# iterate lies inside the true radius.  What remains is the float32 error of the reported norm itself: ||d||_2 within
# norm_rel_bound(T) <= 14 u of the exact norm of d = fl(adv - x), which is within u of adv - x per sample, and max |d| within u:
# s = 16 u = 2^-20.
S = 2.0 ** -20


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
    assert "FMN" in torchattacks.__all__ and len(set(torchattacks.__all__)) == len(torchattacks.__all__)
    atk = torchattacks.FMN(stub())
    assert str(atk) == ("FMN(model_name=LinearDetector, device=cpu, norm=Linf, steps=60, alpha_init=1.0, alpha_final=0.001, "
                        "gamma_init=0.05, gamma_final=0.001, report_at=(), attack_mode=default, return_type=float)")
    assert atk.replays_from_graph is False and atk._supported_mode == ["default"] and atk.last_radius is None
    assert "last_radius" not in vars(atk)                        # a result, not a hyper-parameter
    with pytest.raises(ValueError, match="Targeted mode is not supported"):
        atk.set_mode_targeted_by_function(lambda images, labels: 1 - labels)
    custom = torchattacks.FMN(stub(), norm="L2", steps=7, alpha_init=0.5, alpha_final=0.01, gamma_init=0.1, gamma_final=0.01,
                              report_at=[0.1, 0.2])
    assert (custom.norm, custom.steps, custom.report_at) == ("L2", 7, (0.1, 0.2))
    doc = torchattacks.FMN.__doc__
    for word in ("L1 and L0", "targeted", "restarts", "replay", "DEPARTURE", "nobody has measured"):
        assert word in doc, word


def test_constructor_refuses_unknown_norms_bad_steps_and_bad_gammas():
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    with pytest.raises(ValueError, match="'Linf' or 'L2'"):
        torchattacks.FMN(stub(), norm="L1")
    with pytest.raises(ValueError, match="at least 1"):
        torchattacks.FMN(stub(), steps=0)
    for kw in ({"gamma_init": 0.0}, {"gamma_init": 1.0}, {"gamma_final": -0.1}, {"gamma_final": 1.5}, {"gamma_init": float("nan")}):
        with pytest.raises(ValueError, match=r"\(0, 1\)"):
            torchattacks.FMN(stub(), **kw)
    with pytest.raises(ValueError, match="alpha_init"):
        torchattacks.FMN(stub(), alpha_init=-1.0)


def test_registry_members_and_cli():
    import evaluate_models_on_adversarial_attacks as cli
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    from audio_deepfake_adversarial_attacks_amd.aa.aa_types import AttackEnum
    want = {"FMN": {"norm": "Linf", "steps": 60, "report_at": (0.0005, 0.00075, 0.001)},
            "FMN_L2": {"norm": "L2", "steps": 60, "report_at": (0.1, 0.15, 0.2)},
            "FMN200": {"norm": "Linf", "steps": 200}}
    for name, kw in want.items():
        method, params = AttackEnum[name].value
        assert method is torchattacks.FMN and params == kw
        atk = method(stub(), **params)
        assert (atk.norm, atk.steps, atk.report_at) == (kw["norm"], kw["steps"], kw.get("report_at", ()))
        assert (atk.alpha_init, atk.alpha_final, atk.gamma_init, atk.gamma_final) == (1.0, 1e-3, 0.05, 1e-3)   # the paper's
        assert hasattr(atk, "last_radius")                        # what switches the loop's min_radius report on
        assert cli.parse_arguments(["--attack", name]).attack == name
    assert want["FMN"]["report_at"] == tuple(AttackEnum[n].value[1]["eps"] for n in ("PGD", "PGD_eps00075", "PGD_eps001"))
    assert want["FMN_L2"]["report_at"] == tuple(AttackEnum[n].value[1]["eps"] for n in ("PGDL2", "PGDL2_eps15", "PGDL2_eps20"))
    assert len({e.name for e in AttackEnum}) == len(AttackEnum.__members__)        # no member became an alias of another
    # the default budget is MINRADIUS's: search_steps * steps gradient passes
    mr = AttackEnum["MINRADIUS"].value[1]
    assert want["FMN"]["steps"] == mr["search_steps"] * mr["steps"]


def test_schedule_endpoints_and_shape():
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    from audio_deepfake_adversarial_attacks_amd.torchattacks.attacks.fmn import cosine_schedule
    atk = torchattacks.FMN(stub(), steps=20)
    assert atk.schedule(0) == (1.0, 0.05)
    a, g = atk.schedule(20)
    assert a == pytest.approx(1e-3, rel=1e-12) and g == pytest.approx(1e-3, rel=1e-12)
    mid = atk.schedule(10)
    assert mid[0] == pytest.approx(0.5 * (1.0 + 1e-3), rel=1e-12) and mid[1] == pytest.approx(0.5 * (0.05 + 1e-3), rel=1e-12)
    seq = [atk.schedule(k) for k in range(21)]
    assert all(p[0] > q[0] and p[1] > q[1] for p, q in zip(seq, seq[1:]))          # strictly annealed
    assert cosine_schedule(2.0, 1.0, 5, 10) == pytest.approx(1.0 + 0.5 * (1.0 + math.cos(math.pi / 2)))
    assert isinstance(a, float)                                                   # host float64, a launch scalar afterwards


def test_argument_validation_needs_no_device(lib):
    """Invalid arguments are rejected before any launch (so this is safe without a device)."""
    EINVAL, EWORKSPACE = 1, 2
    P = [ctypes.c_void_p(0x1000000 * (k + 1)) for k in range(12)]    # never dereferenced: validation fails first
    adv, grad, orig, z, y, st_in, st_out, best, out, rn, ws, other = P
    B, Tn = 2, 8
    need = lib.advstep_fmn_workspace_bytes(B, Tn)
    assert need == 5 * 16 and lib.advstep_fmn_workspace_bytes(128, 64_600) == 5 * 128 * 16 * 4
    assert lib.advstep_fmn_workspace_bytes(0, 5) == 0 and lib.advstep_fmn_workspace_bytes(5, 0) == 0
    assert lib.advstep_row_workspace_bytes(128, 64_600) == 16 + 2 * 128 * 16 * 8 + 2 * 128 * 4 + 2 * 128 * 16 * 4   # unchanged
    assert lib.advstep_abi_version() == 3

    assert lib.advstep_fmn_begin_f32(None, B, None) == EINVAL and lib.advstep_fmn_begin_f32(st_in, -1, None) == EINVAL
    assert lib.advstep_fmn_begin_f32(st_in, 65536, None) == EINVAL and lib.advstep_fmn_begin_f32(None, 0, None) == 0

    def norms(adv=adv, grad=grad, orig=orig, B=B, Tn=Tn, ws=ws, ws_bytes=need):
        return lib.advstep_fmn_norms_f32(adv, grad, orig, B, Tn, ws, ws_bytes, None)

    assert norms(adv=None) == EINVAL and norms(orig=None) == EINVAL
    assert norms(B=-1) == EINVAL and norms(Tn=-1) == EINVAL and norms(B=65536) == EINVAL
    assert norms(ws=None) == EWORKSPACE and norms(ws_bytes=need - 1) == EWORKSPACE
    assert norms(ws=ctypes.c_void_p(ws.value + 4)) == EWORKSPACE and norms(ws=adv) == EINVAL
    assert norms(B=0, adv=None, orig=None, ws=None, ws_bytes=0) == 0 and norms(Tn=0, ws=None, ws_bytes=0) == 0

    def step(adv=adv, grad=grad, orig=orig, z=z, y=y, st_in=st_in, st_out=st_out, best=best, out=out, rn=rn, alpha=0.5, gamma=0.05,
             norm=0, move=1, eps_div=1e-10, B=B, Tn=Tn, ws=ws, ws_bytes=need):
        return lib.advstep_fmn_step_f32(adv, grad, orig, z, y, st_in, st_out, best, out, rn, alpha, gamma, norm, move, eps_div, 0.0,
                                        1.0, B, Tn, ws, ws_bytes, None)

    for missing in ("adv", "grad", "orig", "z", "y", "st_in", "st_out", "best", "out"):
        assert step(**{missing: None}) == EINVAL, missing
    assert step(B=-1) == EINVAL and step(Tn=-1) == EINVAL and step(B=65536) == EINVAL
    assert step(norm=2) == EINVAL and step(norm=-1) == EINVAL
    for gamma in (0.0, 1.0, -0.5, float("nan")):
        assert step(gamma=gamma) == EINVAL
    assert step(alpha=-1.0) == EINVAL and step(alpha=float("nan")) == EINVAL and step(eps_div=-1.0) == EINVAL
    assert step(st_out=st_in) == EINVAL                              # ping-pong: never in place
    assert step(st_out=ctypes.c_void_p(st_in.value + 4 * 4 * B - 4)) == EINVAL
    assert step(best=adv) == EINVAL and step(best=orig) == EINVAL and step(best=grad) == EINVAL and step(best=out) == EINVAL
    assert step(best=st_in) == EINVAL and step(best=st_out) == EINVAL and step(st_out=z) == EINVAL
    assert step(out=grad) == EINVAL and step(out=orig) == EINVAL and step(out=st_out) == EINVAL and step(out=rn) == EINVAL
    assert step(out=ctypes.c_void_p(adv.value + 4)) == EINVAL       # overlaps adv without being adv
    assert step(rn=st_out) == EINVAL and step(rn=best) == EINVAL
    assert step(ws=None) == EWORKSPACE and step(ws_bytes=need - 1) == EWORKSPACE and step(ws=ctypes.c_void_p(ws.value + 4)) == EWORKSPACE
    assert step(out=adv, rn=None, ws_bytes=0) == EWORKSPACE         # out = adv and no row_norms are valid: the workspace is what fails
    assert step(move=0, grad=None, out=None, ws_bytes=0) == EWORKSPACE   # the last call needs neither gradient nor out
    assert step(ws=best) == EINVAL
    assert step(B=0) == 0 and step(Tn=0) == 0 and step(B=0, adv=None, ws=None, ws_bytes=0) == 0


def test_wrappers_refuse_cpu_tensors_and_bad_scalars():
    from audio_deepfake_adversarial_attacks_amd import _lib, hip_ops
    x, z = torch.zeros(2, 8), torch.zeros(2)
    y, st = torch.zeros(2, dtype=torch.int64), torch.zeros(4, 2)
    with pytest.raises(_lib.AdvstepError, match="no CPU fallback"):
        hip_ops.fmn_begin(st)
    with pytest.raises(_lib.AdvstepError, match="no CPU fallback"):
        hip_ops.fmn_norms(x, x.clone(), x.clone())
    with pytest.raises(_lib.AdvstepError, match="no CPU fallback"):
        hip_ops.fmn_step(x, x.clone(), x.clone(), z, y, st, x.clone(), torch.zeros(20), 0.5, 0.05)
    assert hip_ops.FMN_PLANES == C.FMN_PLANES and hip_ops.FMN_NORMS == C.FMN_NORMS and hip_ops.FMN_TILE == C.FMN_TILE


def test_cpu_table_covers_every_branch_of_the_decision():
    """adversarial and better | adversarial, not better | not adversarial, found | never found | eps = inf | zero gradient | NaN z."""
    nan = float("nan")
    #                     eps   best  found                z     y   dn    gq
    rows = [(0.5, 0.4, 1.0, -1.0, 1, 0.3, 2.0), (0.5, 0.2, 1.0, -1.0, 1, 0.3, 2.0), (0.5, 0.2, 1.0, 1.0, 1, 0.3, 2.0),
            (INF, INF, 0.0, 1.0, 1, 0.25, 2.0), (INF, INF, 0.0, -2.0, 1, 0.0, 2.0), (INF, INF, 0.0, 1.0, 1, 0.0, 0.0),
            (0.5, INF, 0.0, nan, 0, 0.1, 2.0), (0.5, INF, 0.0, nan, 1, 0.1, 2.0)]
    st = torch.tensor([[r[p] for r in rows] for p in range(3)] + [[0.0] * len(rows)], dtype=torch.float32)
    z = torch.tensor([r[3] for r in rows])
    y = torch.tensor([r[4] for r in rows])
    n4 = torch.tensor([[0.0] * len(rows), [r[5] for r in rows], [0.0] * len(rows), [r[6] for r in rows]])
    copy, new = C.decide(n4, z, y, st, 0.25, "Linf")
    assert copy.tolist() == [True, False, False, False, True, False, False, True]
    f = torch.float32
    assert torch.equal(new[1], torch.tensor([0.3, 0.2, 0.2, INF, 0.0, INF, INF, 0.1], dtype=f))
    assert torch.equal(new[2], torch.tensor([1.0, 1, 1, 0, 1, 0, 0, 1]))
    want_eps = torch.tensor([0.3 * 0.75, 0.2 * 0.75, 0.5 * 1.25, (0.25 + 0.5) * 1.25, 0.0, INF, nan, 0.1 * 0.75], dtype=torch.float64)
    torch.testing.assert_close(new[0].double(), want_eps, rtol=2e-7, atol=0, equal_nan=True)
    assert torch.equal(new[3], n4[1])
    try:
        C.PAPER_RULE = True
        _, paper = C.decide(n4, z, y, st, 0.25, "Linf")
    finally:
        C.PAPER_RULE = False
    assert paper[0, 3] == 0.75 and torch.equal(paper[0, :3], new[0, :3])            # only the never-found rule differs


def run_attack(model, x, y, norm, K=100):
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    atk = torchattacks.FMN(model, norm=norm, steps=K)
    atk.ops = C
    adv = atk(x, y)
    return atk, adv


def check_attack_result(atk, model, x, y, adv, true, norm, s=S):
    """What the issue asks of a result on a linear detector; shared with tests/test_gpu_fmn.py (any device)."""
    radius, adv_c, x_c = atk.last_radius.cpu(), adv.cpu(), x.cpu()
    B, T = x_c.shape
    assert radius.shape == (B,) and radius.dtype == torch.float32
    ratio = radius.double() / true
    print("  true :", [f"{v:.6g}" for v in true.tolist()], "\n  found:", radius.tolist(), "\n  ratio:", [f"{v:.7f}" for v in ratio[1:].tolist()])
    finite = ~torch.isinf(radius)
    assert finite.all()
    with torch.no_grad():
        flipped = C.judged_wrong(model(adv).reshape(-1).cpu(), y.cpu())
    assert flipped.all()                                              # every row with a finite radius is flipped by the detector
    d = (adv_c - x_c).double()
    dn = d.abs().amax(dim=1) if norm == "Linf" else d.norm(dim=1)
    if norm == "Linf":
        assert torch.equal(dn.float(), radius)                        # max |d| is exact
    else:
        assert ((dn - radius.double()).abs() <= C.norm_rel_bound(T) * dn).all()
    assert radius[0] == 0 and torch.equal(adv_c[0], x_c[0])           # the already-wrong row: the clean input, radius 0
    r = true[1:]
    assert (radius[1:].double() <= r * (1 + float(atk.gamma_init))).all()     # the first-found bound of the recurrence
    assert (radius[1:].double() >= r * (1 - s)).all()
    assert adv_c.min() >= 0 and adv_c.max() <= 1


@pytest.mark.parametrize("T", [257, 4099])
@pytest.mark.parametrize("norm", ["Linf", "L2"])
def test_attack_on_linear_detectors_finds_the_closed_form_radii(norm, T):
    """z = x . w + bias_row: the minimal norm of row b is |z_b(x)| / ||w||_1 (L-inf) or / ||w||_2 (L2).  K = 100."""
    model, flat, x, y, true = C.linear_case(T, norm, seed=T)
    atk, adv = run_attack(model, x, y, norm)
    check_attack_result(atk, model, x, y, adv, true, norm)
    again = atk(x, y)                                                 # no random start: the call is a function of its inputs
    assert torch.equal(again, adv)
    # w = 0: no gradient, no move, nothing found — the clean input with +inf
    atk0, adv0 = run_attack(flat, x, y, norm, K=5)
    assert torch.isinf(atk0.last_radius).all() and (atk0.last_radius > 0).all() and torch.equal(adv0, x)
    assert adv0.data_ptr() != x.data_ptr()


@pytest.mark.parametrize("T", [257, 4099])
def test_the_papers_unwidened_rule_leaves_rows_unfound_in_l2(T):
    """The departure, documented: with eps' = dn + |z| / gq the iterate lands ON the boundary of a linear detector and rows stall
    there; the same inputs under the widened rule are all found (the test above)."""
    model, _, x, y, true = C.linear_case(T, "L2", seed=T)
    try:
        C.PAPER_RULE = True
        atk, adv = run_attack(model, x, y, "L2")
    finally:
        C.PAPER_RULE = False
    unfound = torch.isinf(atk.last_radius)
    print("  unfound rows:", unfound.nonzero().reshape(-1).tolist())
    assert unfound.sum() >= 1 and torch.equal(adv[unfound], x[unfound])


def test_training_flags_stay_as_the_caller_left_them():
    """FMN judges in the mode it attacks in: no pass runs under other flags."""
    from audio_deepfake_adversarial_attacks_amd import torchattacks

    class Net(C.LinearDetector):
        def __init__(self, w, b):
            super().__init__(w, b)
            self.drop, self.norm = torch.nn.Dropout(0.0), torch.nn.BatchNorm1d(1)
            self.seen = []

        def forward(self, x):
            self.seen.append((self.training, self.drop.training, self.norm.training, torch.is_grad_enabled()))
            return super().forward(x)

    model, _, x, y, _ = C.linear_case(12, "Linf", seed=1)
    net = Net(model.w.data, model.bias)
    atk = torchattacks.FMN(net, steps=3)
    atk.set_training_mode(model_training=True, batchnorm_training=False)
    atk.ops = C
    atk(x, y)
    assert net.seen == [(True, False, False, True)] * 3 + [(True, False, False, False)]   # K gradient passes + one forward-only
