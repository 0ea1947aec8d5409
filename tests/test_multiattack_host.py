"""CPU: host logic of torchattacks.MultiAttack — constructor surface, modes, the registry and the CLI, the hipGraph off switch
around sub-batch calls — and the argument validation of include/advstep_multi.h without a device."""
import ctypes

import pytest
import torch

from tests import multiattack_cpu_ops as C
from tests.helpers import Surrogate, golden_for_this_cpu, surrogate_from

T = torch.from_numpy
WORSTCASE = ("WORSTCASE", "WORSTCASE_eps00075", "WORSTCASE_eps001", "WORSTCASE_L2", "WORSTCASE40_eps003")


@pytest.fixture(scope="module")
def lib():
    from audio_deepfake_adversarial_attacks_amd import build
    build.build()
    from audio_deepfake_adversarial_attacks_amd import _lib
    return _lib.load()


def test_constructor_errors_and_surface():
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    assert "MultiAttack" in torchattacks.__all__
    with pytest.raises(ValueError, match="At least one attack should be provided."):
        torchattacks.MultiAttack([])
    a, b = Surrogate(), Surrogate()
    with pytest.raises(ValueError, match="At least one of attacks is referencing a different model."):
        torchattacks.MultiAttack([torchattacks.FGSM(a), torchattacks.PGD(b)])
    members = [torchattacks.FGSM(a), torchattacks.PGD(a)]
    atk = torchattacks.MultiAttack(members, verbose=True)
    assert atk.attacks is members and atk.verbose is True and atk.model is a and atk.attack == "MultiAttack"
    assert atk._supported_mode == ["default"] and atk.replays_from_graph is False
    assert torchattacks.MultiAttack(members).verbose is False


def test_targeted_modes_raise():
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    m = Surrogate()
    atk = torchattacks.MultiAttack([torchattacks.FGSM(m)])
    for enter in (lambda: atk.set_mode_targeted_by_function(lambda images, labels: 1 - labels),
                  atk.set_mode_targeted_least_likely, atk.set_mode_targeted_random):
        with pytest.raises(ValueError, match="Targeted mode is not supported."):
            enter()
    assert atk.get_mode() == "default"


def test_str_lists_the_public_attributes():
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    m = Surrogate()
    members = [torchattacks.FGSM(m)]
    atk = torchattacks.MultiAttack(members)
    assert str(atk) == (f"MultiAttack(model_name=Surrogate, device=cpu, attacks={members}, verbose=False, "
                        "attack_mode=default, return_type=float)")


def test_set_training_mode_reaches_the_members():
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    m = Surrogate()
    members = [torchattacks.FGSM(m), torchattacks.MIFGSM(m)]
    atk = torchattacks.MultiAttack(members)
    atk.set_training_mode(model_training=True, batchnorm_training=False, dropout_training=True)
    for a in members + [atk]:
        assert (a._model_training, a._batchnorm_training, a._dropout_training) == (True, False, True)
    atk.set_training_mode()
    for a in members + [atk]:
        assert (a._model_training, a._batchnorm_training, a._dropout_training) == (False, False, False)


@pytest.mark.parametrize("name", WORSTCASE)
def test_registry_members_construct_on_a_stub_model(name):
    import evaluate_models_on_adversarial_attacks as cli
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    from audio_deepfake_adversarial_attacks_amd.aa.aa_types import AttackEnum
    m = Surrogate()
    method, params = AttackEnum[name].value
    atk = method(m, **params)
    assert isinstance(atk, torchattacks.MultiAttack) and all(a.model is m for a in atk.attacks)
    radius = {"WORSTCASE": 0.0005, "WORSTCASE_eps00075": 0.00075, "WORSTCASE_eps001": 0.001, "WORSTCASE_L2": 0.1,
              "WORSTCASE40_eps003": 0.003}[name]
    assert all(a.eps == radius for a in atk.attacks)                               # one threat model per member
    kinds = [(a.__class__.__name__, getattr(a, "norm", None), a.steps) for a in atk.attacks]
    if name == "WORSTCASE_L2":
        assert kinds == [("PGDL2", None, 10), ("APGD", "L2", 10)]
    elif name == "WORSTCASE40_eps003":
        assert kinds == [("PGD", None, 40), ("MIFGSM", None, 40), ("APGD", "Linf", 100)]
        assert atk.attacks[1].alpha == AttackEnum.MIFGSM40_eps003.value[1]["alpha"]
    else:
        assert kinds == [("PGD", None, 10), ("MIFGSM", None, 10), ("APGD", "Linf", 10)]
        assert atk.attacks[1].alpha == radius / 10 and atk.attacks[1].decay == 1.0
    assert cli.parse_arguments(["--attack", name]).attack == name


def test_existing_registry_members_are_unchanged():
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    from audio_deepfake_adversarial_attacks_amd.aa.aa_types import AttackEnum
    assert AttackEnum["PGD"].value == (torchattacks.PGD, {"eps": 0.0005, "steps": 10})
    assert AttackEnum["APGD100_eps003"].value == (torchattacks.APGD, {"norm": "Linf", "eps": 0.003, "steps": 100})
    assert AttackEnum.NO_ATTACK.value == (None, {})
    assert len({e.name for e in AttackEnum}) == len(AttackEnum.__members__)        # no member became an alias of another


def test_graph_switch_is_off_only_during_sub_batch_calls(golden):
    """Members see _graph_off = True exactly when they are handed fewer rows than the incoming batch, and the switch is back
    afterwards — also when a member had it set by its owner, and when a member raises."""
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    g = golden_for_this_cpu(golden, "multiattack")
    model = surrogate_from(g)
    x, y = T(g["x"]), T(g["y"])
    seen = []

    class Probe(torchattacks.FGSM):
        def forward(self, images, labels):
            seen.append((images.shape[0], self._graph_off))
            return super().forward(images, labels)

    members = [Probe(model, eps=0.0) for _ in range(3)]
    atk = torchattacks.MultiAttack(members)
    for a in members + [atk]:
        a.ops = C
    assert torchattacks.Attack._graph_off is False
    atk(x, y)
    assert seen == [(6, False), (4, True), (4, True)]                               # rows 0 and 3 start misclassified
    assert all(a._graph_off is False for a in members)

    del seen[:]
    members[0]._graph_off = True                                                    # the owner's own setting survives
    atk(x, y)
    assert seen[0] == (6, True) and members[0]._graph_off is True and members[1]._graph_off is False

    class Failing(torchattacks.FGSM):
        def forward(self, images, labels):
            raise RuntimeError("member failed")

    bad = Failing(model)
    atk2 = torchattacks.MultiAttack([members[1], bad])
    atk2.ops = C
    with pytest.raises(RuntimeError, match="member failed"):
        atk2(x, y)
    assert bad._graph_off is False


def test_run_iterations_honours_the_switch(monkeypatch):
    """graphed.run_iterations takes the eager loop while the attack's switch is set, whatever else would allow a capture; with
    the switch clear the same call goes looking for one (host logic: stubs stand in for the device)."""
    from audio_deepfake_adversarial_attacks_amd import hip_ops, torchattacks
    from audio_deepfake_adversarial_attacks_amd.torchattacks import graphed

    class FakeCuda(torch.Tensor):
        is_cuda = True

    class Looked(Exception):
        pass

    def looked(device=None):
        raise Looked

    monkeypatch.setenv("ADVSTEP_ATTACK_GRAPH", "1")
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    monkeypatch.setattr(torch.cuda, "current_stream", looked)                    # the first thing the capture's key asks for
    atk = torchattacks.PGD(Surrogate())
    atk._ops = hip_ops
    atk._input_gradient = lambda adv, labels, target: (torch.ones(2, 8), None)
    steps = []

    def step(cur, grad, orig, out):
        steps.append(1)
        out.copy_(cur + grad)

    def run():
        adv = torch.zeros(2, 8).as_subclass(FakeCuda)
        return graphed.run_iterations(atk, adv, adv, torch.zeros(2, dtype=torch.int64), None, 4, step, ())

    with pytest.raises(Looked):
        run()
    atk._graph_off = True
    out = run()
    assert len(steps) == 4 and torch.equal(torch.as_tensor(out).as_subclass(torch.Tensor), torch.full((2, 8), 4.0))


def test_model_must_emit_one_logit_per_utterance(golden):
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    g = golden_for_this_cpu(golden, "multiattack")

    class Passthrough(torchattacks.Attack):
        def __init__(self, model):
            super().__init__("Passthrough", model)

        def forward(self, images, labels):
            return images.clone()

    class TwoLogits(torch.nn.Module):
        def __init__(self, body):
            super().__init__()
            self.body = body

        def forward(self, x):
            z = self.body(x)
            return torch.cat([-z, z], 1)

    m = TwoLogits(surrogate_from(g))
    atk = torchattacks.MultiAttack([Passthrough(m)])
    atk.ops = C
    with pytest.raises(ValueError, match="one logit per utterance"):
        atk(T(g["x"]), T(g["y"]))


def test_cpu_table_routes_by_plain_indexing():
    adv = torch.arange(20, dtype=torch.float32).reshape(5, 4)
    x = -adv
    z = torch.tensor([0.5, -0.0, float("nan"), float("inf"), -1.0])
    labels = torch.tensor([1, 1, 0, 0, 0])                                        # wrong: rows 1 (pre 0) and 3 (pre 1)
    rows = torch.tensor([1, 2, 4, 6, 7], dtype=torch.int32)
    final = torch.full((8, 4), 9.0)
    nx, ny, nr, counts = C.multi_route(adv, x, z, labels, rows, final)
    assert counts.tolist() == [2, 3] and counts.dtype == torch.int32
    assert torch.equal(final[2], adv[1]) and torch.equal(final[6], adv[3])
    assert all(torch.equal(final[r], torch.full((4,), 9.0)) for r in (0, 1, 3, 4, 5, 7))
    assert torch.equal(nx[:3], x[[0, 2, 4]]) and ny[:3].tolist() == [1, 0, 0] and nr[:3].tolist() == [1, 4, 7]


def test_argument_validation_needs_no_device(lib):
    """Invalid arguments are rejected before any launch (so this is safe without a device)."""
    EINVAL = 1
    P = [ctypes.c_void_p(0x10000000 * (k + 1)) for k in range(11)]   # never dereferenced: validation fails first
    names = ("adv", "x", "z", "labels", "rows", "final", "next_x", "next_y", "next_rows", "counts", "scratch")
    base = dict(zip(names, P))

    def route(n=4, B=6, Tn=8, **kw):
        a = {**base, **kw}
        return lib.advstep_multi_route_f32(*(a[k] for k in names), n, B, Tn, None)

    for missing in names:
        assert route(**{missing: None}) == EINVAL, missing
    assert route(n=-1) == EINVAL and route(B=-1) == EINVAL and route(Tn=-1) == EINVAL
    assert route(n=65536, B=65536) == EINVAL                                        # grid.y
    assert route(n=4, B=3) == EINVAL                                                # more rows than the batch has
    assert route(next_x=base["x"]) == EINVAL and route(next_x=base["adv"]) == EINVAL and route(next_x=base["final"]) == EINVAL
    assert route(next_x=ctypes.c_void_p(base["x"].value + 4 * 8)) == EINVAL         # overlaps x without being x
    assert route(final=base["adv"]) == EINVAL and route(final=base["x"]) == EINVAL
    assert route(final=ctypes.c_void_p(base["adv"].value - 4 * 8 * 5)) == EINVAL    # final's B rows reach into adv
    # empty work: OK, nothing launched, nothing read
    none = {k: None for k in names}
    assert route(n=0, B=0, **none) == 0 and route(n=0, B=6, **none) == 0 and route(Tn=0, **none) == 0
    assert route(n=0, B=-1, **none) == EINVAL                                       # a negative size is invalid even then


def test_wrapper_refuses_cpu_tensors():
    from audio_deepfake_adversarial_attacks_amd import _lib, hip_ops
    x = torch.zeros(2, 8)
    with pytest.raises(_lib.AdvstepError, match="no CPU fallback"):
        hip_ops.multi_route(x, x.clone(), torch.zeros(2), torch.zeros(2, dtype=torch.int64),
                            torch.arange(2, dtype=torch.int32), torch.zeros(3, 8))
