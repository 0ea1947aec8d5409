"""CPU: host logic of the momentum attacks — constructor surface, the registry, argument validation of the five entry
points of include/advstep_momentum.h without a device, and per-call state."""
import ctypes

import pytest
import torch

from tests import momentum_cpu_ops as C
from tests.helpers import golden_for_this_cpu, surrogate_from

T = torch.from_numpy
NAMES = ("MIFGSM", "NIFGSM", "VMIFGSM", "VNIFGSM")


@pytest.fixture(scope="module")
def lib():
    from audio_deepfake_adversarial_attacks_amd import build
    build.build()
    from audio_deepfake_adversarial_attacks_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("name", NAMES)
def test_constructor_defaults_print_as_the_reference(golden, name):
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    assert name in torchattacks.__all__
    g = golden("momentum")
    atk = getattr(torchattacks, name)(surrogate_from(g))
    assert str(atk) == str(g[f"str_{name}"])               # attribute names, order and defaults
    assert atk._supported_mode == ["default", "targeted"]
    assert atk.replays_from_graph is (name in ("MIFGSM", "NIFGSM"))
    atk.set_mode_targeted_by_function(lambda images, labels: 1 - labels)
    assert atk._targeted and atk.get_mode() == "targeted"


def test_registry_members():
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    from audio_deepfake_adversarial_attacks_amd.aa.aa_types import AttackEnum
    for cls in ("MIFGSM", "NIFGSM"):
        for name, eps in ((cls, 0.0005), (f"{cls}_eps00075", 0.00075), (f"{cls}_eps001", 0.001)):
            got, kw = AttackEnum[name].value
            assert got is getattr(torchattacks, cls)
            assert kw == {"eps": eps, "alpha": eps / 10, "steps": 10, "decay": 1.0}
    for name in ("VMIFGSM", "VNIFGSM"):
        got, kw = AttackEnum[name].value
        assert got is getattr(torchattacks, name)
        assert kw == {"eps": 0.0005, "alpha": 0.0005 / 10, "steps": 10, "decay": 1.0, "N": 20, "beta": 1.5}
    got, kw = AttackEnum.MIFGSM40_eps003.value
    assert got is torchattacks.MIFGSM and kw == {"eps": 0.003, "alpha": 0.003 / 40, "steps": 40, "decay": 1.0}
    assert kw["eps"] == AttackEnum.PGD40_eps003.value[1]["eps"] and kw["steps"] == AttackEnum.PGD40_eps003.value[1]["steps"]
    # the reference's members stay as they were
    assert AttackEnum["PGD"].value == (torchattacks.PGD, {"eps": 0.0005, "steps": 10})
    assert AttackEnum["PGDL2_eps20"].value == (torchattacks.PGDL2, {"eps": 0.20, "steps": 10})
    assert AttackEnum["FGSM_eps001"].value == (torchattacks.FGSM, {"eps": 0.001})
    assert AttackEnum["FAB_eta30"].value == (torchattacks.FAB, {"n_classes": 2, "eta": 30})
    assert AttackEnum.NO_ATTACK.value == (None, {})


def test_cli_and_trainer_pick_the_members_up_by_name():
    import evaluate_models_on_adversarial_attacks as cli
    assert cli.parse_arguments(["--attack", "MIFGSM40_eps003"]).attack == "MIFGSM40_eps003"
    assert cli.parse_arguments(["--attack", "VNIFGSM"]).attack == "VNIFGSM"


@pytest.mark.parametrize("name", ("VMIFGSM", "VNIFGSM"))
def test_explicit_draws_must_fit_the_call(golden, name):
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    g = golden("momentum")
    x, y = T(g["x"]), T(g["y"])
    atk = getattr(torchattacks, name)(surrogate_from(g), eps=0.005, alpha=0.001, steps=2, N=3)
    atk.ops = C
    good = [[torch.zeros_like(x) for _ in range(3)] for _ in range(2)]
    atk.set_init_noise(good)
    atk(x, y)
    atk.set_init_noise(good[:1])                                             # an iteration short
    with pytest.raises(ValueError, match="2 iterations x 3 neighbours"):
        atk(x, y)
    atk.set_init_noise([row[:2] for row in good])                            # a neighbour short
    with pytest.raises(ValueError, match="2 iterations x 3 neighbours"):
        atk(x, y)
    bad = [list(row) for row in good]
    bad[1][2] = torch.zeros(x.shape[0], x.shape[1] - 1)
    atk.set_init_noise(bad)
    with pytest.raises(ValueError, match=r"draws\[1\]\[2\]"):
        atk(x, y)


@pytest.mark.parametrize("name", NAMES)
def test_state_is_per_call(golden, name):
    """Two consecutive calls of one attack object give the same result: momentum, v and NI's adv start afresh."""
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    g = golden_for_this_cpu(golden, "momentum")
    x, y = T(g["x"]), T(g["y"])
    kw = dict(N=2) if name.startswith("V") else {}
    atk = getattr(torchattacks, name)(surrogate_from(g), eps=0.005, alpha=0.001, steps=4, **kw)
    atk.ops = C
    if name.startswith("V"):
        atk.set_init_noise([[T(d) for d in row] for row in g["VMI_draws"][:, :2]] + [[T(d) for d in g["VNI_draws"][0, :2]]])
    first = atk(x, y)
    assert torch.equal(atk(x, y), first) and not torch.equal(first, x)


def test_argument_validation_needs_no_device(lib):
    """Invalid arguments are rejected before any launch (so this is safe without a device)."""
    EINVAL, EWORKSPACE = 1, 2
    P = [ctypes.c_void_p(0x100000 * (k + 1)) for k in range(8)]    # never dereferenced: validation fails first
    adv, grad, v, orig, mom, out, nes, ws = P
    B, Tn = 2, 8
    need = lib.advstep_row_workspace_bytes(B, Tn)

    def mi(adv=adv, grad=grad, v=v, orig=orig, mom=mom, out=out, nes=nes, B=B, Tn=Tn, ws=ws, ws_bytes=need):
        return lib.advstep_mi_step_f32(adv, grad, v, orig, mom, out, nes, B, Tn, 0.1, 0.2, 1.0, 0.1, 0.0, 1.0, None, ws,
                                       ws_bytes, None)

    for missing in ("adv", "grad", "orig", "mom", "out"):
        assert mi(**{missing: None}) == EINVAL
    assert mi(B=-1) == EINVAL and mi(Tn=-1) == EINVAL and mi(B=65536) == EINVAL
    assert mi(out=grad) == EINVAL and mi(out=mom) == EINVAL and mi(mom=orig) == EINVAL     # aliasing what is read
    assert mi(nes=adv) == EINVAL and mi(nes=out) == EINVAL and mi(nes=mom) == EINVAL
    assert mi(out=ctypes.c_void_p(adv.value + 4)) == EINVAL                                 # out overlaps adv without being adv
    assert mi(ws=None) == EWORKSPACE and mi(ws_bytes=need - 1) == EWORKSPACE
    assert mi(ws=ctypes.c_void_p(ws.value + 4)) == EWORKSPACE                               # misaligned
    assert mi(out=adv, ws_bytes=need - 1) == EWORKSPACE     # out = adv, v = NULL and nes_out = NULL are valid: the workspace is what fails
    assert mi(v=None, nes=None, ws_bytes=0) == EWORKSPACE
    assert mi(B=0, adv=None, grad=None, orig=None, mom=None, out=None, ws=None, ws_bytes=0) == 0
    assert mi(Tn=0, ws=None, ws_bytes=0) == 0

    assert lib.advstep_vt_neighbor_noise_f32(None, grad, out, 8, None) == EINVAL
    assert lib.advstep_vt_neighbor_noise_f32(adv, None, out, 8, None) == EINVAL
    assert lib.advstep_vt_neighbor_noise_f32(adv, grad, out, -1, None) == EINVAL
    assert lib.advstep_vt_neighbor_noise_f32(None, None, None, 0, None) == 0
    assert lib.advstep_vt_neighbor_philox_f32(adv, None, 8, 0.1, 1, 0, None) == EINVAL
    assert lib.advstep_vt_neighbor_philox_f32(adv, out, -8, 0.1, 1, 0, None) == EINVAL
    assert lib.advstep_vt_neighbor_philox_f32(None, None, 0, 0.1, 1, 0, None) == 0
    assert lib.advstep_vt_accumulate_f32(None, grad, 8, 1, None) == EINVAL
    assert lib.advstep_vt_accumulate_f32(out, out, 8, 0, None) == EINVAL                    # gv += gv is not an accumulation
    assert lib.advstep_vt_accumulate_f32(out, grad, -1, 0, None) == EINVAL
    assert lib.advstep_vt_accumulate_f32(None, None, 0, 1, None) == 0
    assert lib.advstep_vt_variance_f32(out, grad, None, 8, 4, None) == EINVAL
    assert lib.advstep_vt_variance_f32(out, grad, v, 8, 0, None) == EINVAL                  # N >= 1
    assert lib.advstep_vt_variance_f32(out, grad, v, -8, 4, None) == EINVAL
    assert lib.advstep_vt_variance_f32(None, None, None, 0, 4, None) == 0


def test_wrappers_refuse_cpu_tensors():
    from audio_deepfake_adversarial_attacks_amd import _lib, hip_ops
    x = torch.zeros(2, 8)
    with pytest.raises(_lib.AdvstepError, match="no CPU fallback"):
        hip_ops.mi_step(x, x.clone(), x.clone(), x.clone(), 0.1, 0.2, 1.0)
    with pytest.raises(_lib.AdvstepError, match="no CPU fallback"):
        hip_ops.vt_neighbor(x, 0.1, seed=1)
    with pytest.raises(_lib.AdvstepError, match="no CPU fallback"):
        hip_ops.vt_accumulate(x, x.clone(), True)
    with pytest.raises(_lib.AdvstepError, match="no CPU fallback"):
        hip_ops.vt_variance(x, x.clone(), 4)


def test_cpu_table_philox_matches_the_pgd_start_stream():
    """The neighbour draw is the uniform stream of the PGD L-inf random start (the oracle's restatement of it)."""
    from oracle import torch_ops
    x = torch.full((3, 37), 0.5)
    want = torch_ops.pgd_linf_init(x, 0.0125, seed=1234567, offset=9, lo=-10.0, hi=10.0)
    got = C.vt_neighbor(x, 0.0125, seed=1234567, offset=9)
    assert torch.equal(got, want)
