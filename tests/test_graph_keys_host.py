"""The pure parts of torchattacks/graphed.py on the CPU: what moves a capture's key (`_state_signature`, `_toggles`) and what must
not, and the bookkeeping that ties a model's table entries to its lifetime (`_watch` / `_forget_model`).  The replays
themselves are pinned on the device by tests/test_gpu_graph_detectors.py."""
import gc
import weakref

import pytest
import torch

from tests.helpers import Surrogate


@pytest.fixture()
def graphed():
    from audio_deepfake_adversarial_attacks_amd.torchattacks import graphed
    graphed.clear()
    yield graphed
    graphed.clear()


def with_batchnorm():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Conv1d(1, 4, 3), torch.nn.BatchNorm1d(4), torch.nn.Sequential(torch.nn.Dropout(0.5))).eval()


def test_signature_moves_with_an_in_place_parameter_edit(graphed):
    model = with_batchnorm()
    before = graphed._state_signature(model)
    with torch.no_grad():
        model[0].bias.mul_(1.01)
    after = graphed._state_signature(model)
    assert after != before
    assert after[0] != before[0] and after[1:] == before[1:]            # the parameters' part, and only it


def test_signature_moves_with_a_buffer_edit(graphed):
    model = with_batchnorm()
    before = graphed._state_signature(model)
    with torch.no_grad():
        model[1].running_mean.add_(0.05)
    after = graphed._state_signature(model)
    assert after[1] != before[1] and after[0] == before[0] and after[2] == before[2]


def test_signature_moves_with_one_submodules_training_flag(graphed):
    model = with_batchnorm()
    before = graphed._state_signature(model)
    model[2][0].train()                                                 # the innermost module only
    after = graphed._state_signature(model)
    assert after[2] != before[2] and after[:2] == before[:2]
    assert sum(a != b for a, b in zip(after[2], before[2])) == 1
    model[2][0].eval()
    assert graphed._state_signature(model) == before                    # flags come back; versions would not


def test_signature_moves_with_load_state_dict_of_equal_values(graphed):
    model = with_batchnorm()
    before = graphed._state_signature(model)
    values = {k: v.clone() for k, v in model.state_dict().items()}
    model.load_state_dict(model.state_dict())
    after = graphed._state_signature(model)
    assert after[0] != before[0] and after[1] != before[1]
    for k, v in model.state_dict().items():
        assert torch.equal(v, values[k])


def test_signature_stands_through_what_an_attack_call_does(graphed):
    model = with_batchnorm()
    before = graphed._state_signature(model)
    x = torch.randn(2, 1, 32, requires_grad=True)
    model(x).sum().backward()                                           # forward + input-backward, eval-mode BatchNorm
    assert graphed._state_signature(model) == before
    frozen = [p for p in model.parameters() if p.requires_grad]         # Attack.__call__ around every call
    assert frozen
    for p in frozen:
        p.requires_grad_(False)
    assert graphed._state_signature(model) == before
    for p in frozen:
        p.requires_grad_(True)
    assert graphed._state_signature(model) == before
    unrelated = torch.zeros(3)
    unrelated = unrelated.to(torch.float64)
    assert graphed._state_signature(model) == before
    assert graphed._state_signature(Surrogate()) != before              # ... and is not a constant


def test_toggles_are_sorted_and_see_only_their_prefix(graphed, monkeypatch):
    import os
    for k in [k for k in os.environ if k.startswith("ADVSTEP_")]:
        monkeypatch.delenv(k)
    assert graphed._toggles() == ()
    monkeypatch.setenv("ADVSTEP_ZED", "0")
    monkeypatch.setenv("ADVSTEP_ABLE", "1")
    one_order = graphed._toggles()
    monkeypatch.delenv("ADVSTEP_ZED")
    monkeypatch.delenv("ADVSTEP_ABLE")
    monkeypatch.setenv("ADVSTEP_ABLE", "1")
    monkeypatch.setenv("ADVSTEP_ZED", "0")
    assert graphed._toggles() == one_order == (("ADVSTEP_ABLE", "1"), ("ADVSTEP_ZED", "0"))
    monkeypatch.setenv("OTHER_ADVSTEP_SWITCH", "1")
    monkeypatch.setenv("advstep_lower", "1")
    monkeypatch.setenv("HIP_VISIBLE_DEVICES", "0")
    assert graphed._toggles() == one_order


def test_toggles_tell_unset_from_the_default_written_out(graphed, monkeypatch):
    monkeypatch.delenv("ADVSTEP_RAWNET3_CHAIN", raising=False)
    unset = graphed._toggles()
    monkeypatch.setenv("ADVSTEP_RAWNET3_CHAIN", "1")                    # the same behaviour, another key: costs a capture, never a
    written = graphed._toggles()                                        # wrong replay
    monkeypatch.setenv("ADVSTEP_RAWNET3_CHAIN", "0")
    off = graphed._toggles()
    assert len({unset, written, off}) == 3


def entries_of(graphed, model_id):
    return [k for table in (graphed._GRAPHS, graphed._SEEN, graphed._FAILED) for k in table if k[0] == model_id]


def test_a_models_entries_go_when_the_model_goes(graphed):
    """Hand-made entries under two models' ids (`_Captured` needs a device; the tables only ever look at the keys)."""
    dead, alive = Surrogate(), Surrogate()
    ids = {}
    for name, model in (("dead", dead), ("alive", alive)):
        graphed._watch(model)
        graphed._watch(model)                                           # once per model, however many calls
        mid = ids[name] = id(model)
        family = (mid, "PGD", (0.01, 0.002))
        graphed._GRAPHS[family + ("state",)] = object()
        graphed._GRAPHS[family + ("other state",)] = object()
        graphed._SEEN[family + ("state",)] = 2
        graphed._SEEN[family + ("third state",)] = 1
        graphed._FAILED.add(family + ("another shape",))
    assert set(graphed._WATCHED) == set(ids.values())
    assert len(entries_of(graphed, ids["dead"])) == 5
    ref = weakref.ref(dead)
    del dead, model
    gc.collect()
    assert ref() is None                                                # nothing here holds the model
    assert entries_of(graphed, ids["dead"]) == []
    assert len(entries_of(graphed, ids["alive"])) == 5
    assert set(graphed._WATCHED) == {ids["alive"]}
    assert (len(graphed._GRAPHS), len(graphed._SEEN), len(graphed._FAILED)) == (2, 2, 1)


def test_clear_lets_go_of_the_finalizers(graphed):
    model = Surrogate()
    graphed._watch(model)
    fin = graphed._WATCHED[id(model)]
    assert fin.alive and fin.atexit is False
    graphed.clear()
    assert not fin.alive and not graphed._WATCHED
    # an entry made under the same id afterwards (a later model at the same address) is not the dead model's to drop
    mid = id(model)
    graphed._SEEN[(mid, "PGD")] = 1
    del model
    gc.collect()
    assert (mid, "PGD") in graphed._SEEN
