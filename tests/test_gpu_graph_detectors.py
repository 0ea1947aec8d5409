"""`-m gpu`: hipGraph replay (torchattacks/graphed.py) of every graph-replayed attack on RawNet3 and SpecRNet, the stale-state
hazards of a live capture on the detectors, every component of the capture key on a cheap model, and a capture's lifetime.

Every comparison is `torch.equal` against eager launches (ADVSTEP_ATTACK_GRAPH=0) of the same kernels under the same switches:
a replay that read a stale or freed cache (Winograd-prepared weights, `bn_eval_affine` pairs, RawNet3's chain plans, packed GRU
weights, residual-block plans) returns a plausible waveform with other bits.  Waveforms keep the dataset's own T = 64 600: the
detectors' fused paths are shape-gated, and every model test checks that the fused path it is about was taken.  B = 3
is the smallest batch with a first, an inner and a last row.  The pure parts of the key: tests/test_graph_keys_host.py."""
import gc
import weakref

import pytest
import torch

pytestmark = pytest.mark.gpu

T_CHEAP = 4099


def armed(cls, model, model_training=True, **kw):
    atk = cls(model, **kw)
    atk.set_training_mode(model_training=model_training, batchnorm_training=False)
    return atk


@pytest.fixture()
def fresh_graphs():
    from audio_deepfake_adversarial_attacks_amd.torchattacks import graphed
    graphed.clear()
    yield graphed
    graphed.clear()


def data(cuda, n, seed, T=None):
    from audio_deepfake_adversarial_attacks_amd.datasets.synthetic import synthetic_waveforms
    from audio_deepfake_adversarial_attacks_amd.aa import utils as aa_utils
    x, y = synthetic_waveforms(n, seed=seed)
    if T is not None:
        x = x[:, :T].contiguous()
    x01, _, _ = aa_utils.to_minmax(x.to(cuda))
    return x01, y.to(cuda)


def build(name, cuda):
    from audio_deepfake_adversarial_attacks_amd.models.models import get_model
    torch.manual_seed(0)
    cfg = {"lcnn": {"frontend_algorithm": ["lfcc"], "input_channels": 1},
           "specrnet": {"frontend_algorithm": ["mel_spec"], "input_channels": 2}, "rawnet3": {}}[name]
    return get_model(name, cfg, str(cuda)).to(cuda).eval()


_pristine = {}


@pytest.fixture()
def pristine(cuda):
    """One detector per name for the tests that leave its parameters and buffers alone (a RawNet3 has 15.5 M parameters)."""
    def get(name):
        if name not in _pristine:
            _pristine[name] = build(name, cuda)
        return _pristine[name]
    return get


def took_fused_path(name, model):
    """The marker the fused path of `name` leaves on the model: RawNet3's Res2Net chain plan (all seven branches), a SpecRNet
    residual block's matrix-core plan, an LCNN 3x3 weight's Winograd-prepared image."""
    if name == "rawnet3":
        plan = getattr(model.layer1, "_chain_val", None)
        return plan is not None and plan["nums"] == 7
    if name == "specrnet":
        return getattr(model.block0[0], "_advstep_plan", None) is not None
    return any(getattr(p, "_advstep_wino", None) is not None and len(p._advstep_wino[1]) > 0 for p in model.parameters())


def eager(monkeypatch, atk, x, y):
    monkeypatch.setenv("ADVSTEP_ATTACK_GRAPH", "0")
    try:
        return atk(x, y)
    finally:
        monkeypatch.setenv("ADVSTEP_ATTACK_GRAPH", "1")


def pgd4(model, **kw):
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    return armed(torchattacks.PGD, model, eps=kw.pop("eps", 0.003), alpha=0.001, steps=4, random_start=False, **kw)


# ---- a. the replay matrix --------------------------------------------------------------------------------------------------------

# MinRadiusPGD: the constructor arguments of test_gpu_minradius.py::test_graph_replay_is_bit_identical (eps_max per norm: its
# DETECTOR_CASE).  Odd step counts: pairs replayed + one eager iteration.
ATTACKS = {
    "PGD": ("PGD", dict(eps=0.003, alpha=0.001, steps=5, random_start=False)),
    "PGDL2": ("PGDL2", dict(eps=0.1, alpha=0.04, steps=4, random_start=False)),
    "MIFGSM": ("MIFGSM", dict(eps=0.003, alpha=0.001, steps=4, decay=1.0)),
    "NIFGSM": ("NIFGSM", dict(eps=0.003, alpha=0.001, steps=4, decay=1.0)),
    "MinRadiusLinf": ("MinRadiusPGD", dict(norm="Linf", eps_max=0.003, search_steps=4, steps=4)),
    "MinRadiusL2": ("MinRadiusPGD", dict(norm="L2", eps_max=2.0, search_steps=4, steps=4)),
}
CELLS = [("rawnet3", a) for a in ("PGD", "PGDL2", "MIFGSM", "NIFGSM", "MinRadiusLinf")] + \
        [("specrnet", a) for a in ("PGD", "MIFGSM", "MinRadiusL2")]


@pytest.mark.parametrize("name,attack", CELLS)
def test_replay_is_bit_identical(cuda, fresh_graphs, monkeypatch, pristine, name, attack):
    """Eager, captured, replayed; another batch and another attack object through the same capture.  MinRadiusPGD runs the
    loop once per search round, so its first call already sees the key twice: it holds its capture after every call."""
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    model = pristine(name)
    cls, kw = ATTACKS[attack]
    radii = cls == "MinRadiusPGD"

    def make():
        return armed(getattr(torchattacks, cls), model, **kw)

    def result(atk, x, y):
        out = atk(x, y)
        return (out, atk.last_radius.clone()) if radii else (out,)

    def same(got, want):
        return all(torch.equal(g, w) for g, w in zip(got, want))

    atk = make()
    x01, y = data(cuda, 3, 11)
    x2, y2 = data(cuda, 3, 12)
    if radii:
        # rows that start right have a radius to search for, one row starts wrong (radius 0): test_gpu_minradius.detector_batch
        with torch.no_grad():
            y, y2 = ((model(x).reshape(-1) > 0).long() for x in (x01, x2))
        y[0], y2[1] = 1 - y[0], 1 - y2[1]
    monkeypatch.setenv("ADVSTEP_ATTACK_GRAPH", "0")
    want = result(atk, x01, y)
    assert len(fresh_graphs._GRAPHS) == 0
    monkeypatch.setenv("ADVSTEP_ATTACK_GRAPH", "1")
    for call, held in enumerate((1, 1, 1) if radii else (0, 1, 1)):     # first sight, second sight (capture), replay
        got = result(atk, x01, y)
        assert len(fresh_graphs._GRAPHS) == held, call
        assert same(got, want), call
    assert took_fused_path(name, model)
    if radii:
        print("  radii:", want[1].tolist())
    assert not torch.equal(want[0], x01)
    # another batch of the same shape through the same capture
    monkeypatch.setenv("ADVSTEP_ATTACK_GRAPH", "0")
    want2 = result(atk, x2, y2)
    monkeypatch.setenv("ADVSTEP_ATTACK_GRAPH", "1")
    assert same(result(atk, x2, y2), want2) and len(fresh_graphs._GRAPHS) == 1
    assert not torch.equal(want2[0], want[0])
    # another object with equal hyper-parameters: the same family, the first object's capture, its own per-call state
    other = make()
    assert same(result(other, x01, y), want) and len(fresh_graphs._GRAPHS) == 1


# ---- b. stale-state hazards with a live capture ---------------------------------------------------------------------------------

def live_capture(graphed, monkeypatch, name, model, x01, y):
    """PGD steps 4 on `model`, captured and replayed once; returns (attack, eager result)."""
    atk = pgd4(model)
    want = eager(monkeypatch, atk, x01, y)
    for held in (0, 1, 1):
        assert torch.equal(atk(x01, y), want) and len(graphed._GRAPHS) == held
    assert took_fused_path(name, model) and not torch.equal(want, x01)
    return atk, want


def first_batchnorm(name, model):
    return model.layer1.bns[0] if name == "rawnet3" else model.block0[0].bn2


def check_moved_state(graphed, monkeypatch, atk, x01, y, want_before):
    """After a change of the model's state with a capture live: eager on the new state, then a new capture INSTEAD of the old
    one, then its replay; all equal to eager launches on the new state, which differ from the old result."""
    want = eager(monkeypatch, atk, x01, y)
    stale = set(graphed._GRAPHS)
    assert len(stale) == 1
    assert torch.equal(atk(x01, y), want) and set(graphed._GRAPHS) == stale          # first sight: eager
    assert torch.equal(atk(x01, y), want)                                            # second sight: captured
    assert len(graphed._GRAPHS) == 1 and not (set(graphed._GRAPHS) & stale)
    assert torch.equal(atk(x01, y), want)                                            # replayed
    assert len(graphed._GRAPHS) == 1
    assert not torch.equal(want, want_before)


@pytest.mark.parametrize("name", ["rawnet3", "specrnet"])
def test_in_place_parameter_change(cuda, fresh_graphs, monkeypatch, name):
    model = build(name, cuda)
    x01, y = data(cuda, 3, 21)
    atk, want = live_capture(fresh_graphs, monkeypatch, name, model, x01, y)
    with torch.no_grad():
        for p in model.parameters():
            p.mul_(1.01)
    check_moved_state(fresh_graphs, monkeypatch, atk, x01, y, want)
    assert took_fused_path(name, model)


@pytest.mark.parametrize("name", ["rawnet3", "specrnet"])
def test_buffer_only_change(cuda, fresh_graphs, monkeypatch, name):
    """A BatchNorm's running mean moves, no parameter does: only the buffers' part of the key stands between the replay and a
    stale `bn_eval_affine` pair (SpecRNet: inside the block's plan; RawNet3: inside layer1's chain plan)."""
    model = build(name, cuda)
    x01, y = data(cuda, 3, 22)
    atk, want = live_capture(fresh_graphs, monkeypatch, name, model, x01, y)
    versions = [p._version for p in model.parameters()]
    with torch.no_grad():
        first_batchnorm(name, model).running_mean.add_(0.05)
    assert [p._version for p in model.parameters()] == versions
    check_moved_state(fresh_graphs, monkeypatch, atk, x01, y, want)


@pytest.mark.parametrize("name", ["rawnet3", "specrnet"])
def test_load_state_dict_of_the_models_own_values(cuda, fresh_graphs, monkeypatch, name):
    """Versions move, values do not: the same bits as before, through a new capture that replaces the old one."""
    model = build(name, cuda)
    x01, y = data(cuda, 3, 23)
    atk, want = live_capture(fresh_graphs, monkeypatch, name, model, x01, y)
    stale = set(fresh_graphs._GRAPHS)
    model.load_state_dict(model.state_dict())
    assert torch.equal(eager(monkeypatch, atk, x01, y), want)
    assert torch.equal(atk(x01, y), want) and set(fresh_graphs._GRAPHS) == stale      # first sight: eager, old capture unused
    assert torch.equal(atk(x01, y), want)
    assert len(fresh_graphs._GRAPHS) == 1 and not (set(fresh_graphs._GRAPHS) & stale)  # one capture in the family, the new one
    assert torch.equal(atk(x01, y), want)


@pytest.mark.parametrize("name,switch", [("rawnet3", "ADVSTEP_RAWNET3_CHAIN"), ("specrnet", "ADVSTEP_SPECRNET_CONV"),
                                         ("specrnet", "ADVSTEP_RESBLOCK_FEW"), ("lcnn", "ADVSTEP_LCNN_CONV3X3")])
def test_switch_flipped_and_flipped_back_with_a_live_capture(cuda, fresh_graphs, monkeypatch, pristine, name, switch):
    """No clear() in between.  The capture under the defaults bakes the addresses of the fused path's caches; the other path
    runs (eagerly, captured, replayed) and must leave them where they are, because the first capture is replayed again once
    the switch is back.  ADVSTEP_RESBLOCK_FEW is the switch whose other value builds ANOTHER plan for the same block."""
    model = pristine(name)
    monkeypatch.delenv(switch, raising=False)
    x01, y = data(cuda, 3, 24)
    atk, want_on = live_capture(fresh_graphs, monkeypatch, name, model, x01, y)
    first = set(fresh_graphs._GRAPHS)
    monkeypatch.setenv(switch, "0")
    want_off = eager(monkeypatch, atk, x01, y)                          # eager UNDER THAT SWITCH
    for held in (1, 2, 2):
        assert torch.equal(atk(x01, y), want_off)
        assert len(fresh_graphs._GRAPHS) == held and first <= set(fresh_graphs._GRAPHS)
    monkeypatch.delenv(switch)
    assert torch.equal(atk(x01, y), want_on)                            # the first capture, replayed
    assert len(fresh_graphs._GRAPHS) == 2
    x2, y2 = data(cuda, 3, 25)                                          # ... on a batch it has not seen
    want2 = eager(monkeypatch, atk, x2, y2)
    assert torch.equal(atk(x2, y2), want2) and len(fresh_graphs._GRAPHS) == 2
    monkeypatch.setenv(switch, "0")                                     # and the second one
    assert torch.equal(atk(x01, y), want_off) and len(fresh_graphs._GRAPHS) == 2


@pytest.mark.parametrize("name", ["rawnet3", "specrnet"])
def test_partial_batch_between_replays(cuda, fresh_graphs, monkeypatch, pristine, name):
    model = pristine(name)
    x3, y3 = data(cuda, 3, 26)
    x2, y2 = x3[:2].contiguous(), y3[:2].contiguous()
    atk, want3 = live_capture(fresh_graphs, monkeypatch, name, model, x3, y3)
    want2 = eager(monkeypatch, atk, x2, y2)
    for held in (1, 2):
        assert torch.equal(atk(x2, y2), want2) and len(fresh_graphs._GRAPHS) == held
    assert torch.equal(atk(x3, y3), want3) and torch.equal(atk(x2, y2), want2)
    assert len(fresh_graphs._GRAPHS) == 2                               # one capture per shape
    assert sorted(k[4] for k in fresh_graphs._GRAPHS) == [(2, 64_600), (3, 64_600)]


# ---- c. the key's components on a cheap model ------------------------------------------------------------------------------------

class ScaledInTraining(torch.nn.Module):
    """Surrogate whose logit depends on the module's own training flag (no BatchNorm, no Dropout: nothing else does).  The factor
    is negative: the update steps see the gradient's sign or its row-normalised direction, so under a positive per-row factor
    (2.0 was tried: equal bits) the two modes give the same waveform and a replay through the other mode's capture could not
    be told from a right one."""

    def __init__(self):
        super().__init__()
        from tests.helpers import Surrogate
        self.inner = Surrogate()

    def forward(self, x):
        return self.inner(x) * (-2.0 if self.training else 1.0)


def surrogate(cuda, cls=None):
    from tests.helpers import Surrogate
    torch.manual_seed(1)
    return (cls or Surrogate)().to(cuda).eval()


def test_training_flags_are_part_of_the_key(cuda, fresh_graphs, monkeypatch):
    model = surrogate(cuda, ScaledInTraining)
    x01, y = data(cuda, 3, 5, T_CHEAP)
    a, b = pgd4(model, eps=0.01, model_training=True), pgd4(model, eps=0.01, model_training=False)
    want_a, want_b = eager(monkeypatch, a, x01, y), eager(monkeypatch, b, x01, y)
    assert not torch.equal(want_a, want_b)
    for atk, want, held in ((a, want_a, 0), (a, want_a, 1), (b, want_b, 1), (b, want_b, 2), (a, want_a, 2), (b, want_b, 2)):
        assert torch.equal(atk(x01, y), want)
        assert len(fresh_graphs._GRAPHS) == held


def test_targeted_mode_is_part_of_the_key(cuda, fresh_graphs, monkeypatch):
    """Default mode against targeted mode (another sign in the loss gradient, the targets instead of the labels): a capture
    each.  On a two-class detector the target 1 - y asks for what the default mode asks for (-CE(z, 1 - y) and CE(z, y) grow
    in the same direction of z), so those two results cannot differ; a third attack aimed at y itself walks the other way,
    and it goes through the targeted capture of the first: the targets are replay data, not part of the key."""
    model = surrogate(cuda)
    x01, y = data(cuda, 3, 5, T_CHEAP)
    plain, aimed, kept = pgd4(model, eps=0.01), pgd4(model, eps=0.01), pgd4(model, eps=0.01)
    aimed.set_mode_targeted_by_function(lambda x, y: 1 - y)
    kept.set_mode_targeted_by_function(lambda x, y: y.clone())
    want_plain, want_aimed, want_kept = (eager(monkeypatch, atk, x01, y) for atk in (plain, aimed, kept))
    assert not torch.equal(want_kept, want_plain) and not torch.equal(want_kept, want_aimed)
    for atk, want, held in ((plain, want_plain, 0), (plain, want_plain, 1), (aimed, want_aimed, 1), (aimed, want_aimed, 2),
                            (kept, want_kept, 2), (plain, want_plain, 2), (aimed, want_aimed, 2), (kept, want_kept, 2)):
        assert torch.equal(atk(x01, y), want) and len(fresh_graphs._GRAPHS) == held
    assert sorted(k[3] for k in fresh_graphs._GRAPHS) == [False, True]


def test_labels_dtype_is_part_of_the_key(cuda, fresh_graphs, monkeypatch):
    model = surrogate(cuda)
    x01, y = data(cuda, 3, 5, T_CHEAP)
    assert y.dtype == torch.int64
    y32 = y.to(torch.int32)
    atk = pgd4(model, eps=0.01)
    want = eager(monkeypatch, atk, x01, y)
    assert torch.equal(eager(monkeypatch, atk, x01, y32), want)
    for labels, held in ((y, 0), (y, 1), (y32, 1), (y32, 2), (y, 2), (y32, 2)):
        assert torch.equal(atk(x01, labels), want) and len(fresh_graphs._GRAPHS) == held
    assert sorted(str(k[6]) for k in fresh_graphs._GRAPHS) == ["torch.int32", "torch.int64"]


def test_eviction_at_the_table_bound(cuda, fresh_graphs, monkeypatch):
    model = surrogate(cuda)
    x01, y = data(cuda, 3, 5, T_CHEAP)
    bound = fresh_graphs._MAX_GRAPHS
    workloads = [pgd4(model, eps=0.004 + 0.001 * i) for i in range(bound + 1)]
    wants = [eager(monkeypatch, atk, x01, y) for atk in workloads]
    assert not torch.equal(wants[0], wants[1])
    for i, (atk, want) in enumerate(zip(workloads, wants)):
        for _ in range(2):
            assert torch.equal(atk(x01, y), want)
            assert len(fresh_graphs._GRAPHS) <= bound
        assert len(fresh_graphs._GRAPHS) == min(i + 1, bound)
    first_family = (id(model), "PGD", (workloads[0].eps, workloads[0].alpha))
    assert not [k for k in fresh_graphs._GRAPHS if k[:3] == first_family]            # the oldest capture made room
    for _ in range(2):                                                  # ... and its workload goes on, eager or captured anew
        assert torch.equal(workloads[0](x01, y), wants[0])
        assert len(fresh_graphs._GRAPHS) <= bound
    assert [k for k in fresh_graphs._GRAPHS if k[:3] == first_family]
    assert torch.equal(workloads[-1](x01, y), wants[-1])                # a surviving capture still replays right
    assert len(fresh_graphs._SEEN) <= 64


def test_weights_that_change_before_every_call_stay_eager(cuda, fresh_graphs, monkeypatch):
    """The adversarial-training pattern: no key is ever seen twice."""
    model = surrogate(cuda)
    x01, y = data(cuda, 3, 5, T_CHEAP)
    atk = pgd4(model, eps=0.01)
    for call in range(12):
        with torch.no_grad():
            for p in model.parameters():
                p.add_(1e-4)
        want = eager(monkeypatch, atk, x01, y)
        assert torch.equal(atk(x01, y), want), call
        assert len(fresh_graphs._GRAPHS) == 0 and len(fresh_graphs._SEEN) <= 64


# ---- d. a capture dies with its model ---------------------------------------------------------------------------------------------

def held_bytes(*tensors):
    """What the caching allocator accounts for these tensors: their storages, in its 512-byte granules."""
    return sum(-(-t.untyped_storage().nbytes() // 512) * 512 for t in tensors)


def capture_then_drop_the_model(graphed, make_model, x01, y):
    """Capture PGD on a fresh model, replay once, then let go of the attack and the model.  Returns a weak reference to the
    model and its id."""
    model = make_model()
    atk = pgd4(model)
    outs = [atk(x01, y) for _ in range(3)]
    assert len(graphed._GRAPHS) == 1 and torch.equal(outs[0], outs[2])
    ref, mid = weakref.ref(model), id(model)
    del atk, model, outs
    gc.collect()
    return ref, mid


def check_nothing_outlives(graphed, ref, mid):
    assert ref() is None                                                # the tables hold no strong reference to the model
    assert ref() is not None or len(graphed._GRAPHS) == 0
    leftovers = [k for table in (graphed._SEEN, graphed._FAILED) for k in table if k[0] == mid]
    assert ref() is not None or not leftovers


def test_a_capture_dies_with_its_model_surrogate(cuda, fresh_graphs):
    x01, y = data(cuda, 3, 5, T_CHEAP)
    ref, mid = capture_then_drop_the_model(fresh_graphs, lambda: surrogate(cuda), x01, y)
    check_nothing_outlives(fresh_graphs, ref, mid)


def test_a_capture_dies_with_its_model_and_returns_its_memory_specrnet(cuda, fresh_graphs):
    """... and with the capture go its static buffers, its gradient outputs and its private pool: after the model's death the
    allocator holds what it held before the model was built plus the tensors this test still holds.  The cycle runs twice and
    the second is measured: the first leaves behind what belongs to the process, not to a model or a capture (scratch and FFT
    plans of the launch stream, loaded code objects).  The BLAS workspaces that torch allocates per (handle, stream), for
    the capture's side stream among them, are torch's to keep; they are returned before both readings."""
    def settle():
        gc.collect()
        torch.cuda.synchronize()
        assert len(fresh_graphs._GRAPHS) == 0                           # no live graph has a workspace's address baked in
        torch._C._cuda_clearCublasWorkspaces()
        return torch.cuda.memory_allocated()

    ref, mid = capture_then_drop_the_model(fresh_graphs, lambda: build("specrnet", cuda), *data(cuda, 3, 27))
    check_nothing_outlives(fresh_graphs, ref, mid)
    base = settle()
    x01, y = data(cuda, 3, 28)
    ref, mid = capture_then_drop_the_model(fresh_graphs, lambda: build("specrnet", cuda), x01, y)
    check_nothing_outlives(fresh_graphs, ref, mid)
    after = settle()
    print(f"  allocated: base {base}, after {after}, held {held_bytes(x01, y)}; reserved {torch.cuda.memory_reserved()}")
    assert after <= base + held_bytes(x01, y)
