"""CPU: host logic of the product package — Attack plugin API, registry, metrics, sharding — with the oracle's op
table injected where waveform arithmetic is needed (the product itself has no CPU path)."""
import numpy as np
import pytest
import torch

from audio_deepfake_adversarial_attacks_amd import metrics, torchattacks
from audio_deepfake_adversarial_attacks_amd.aa.aa_types import AttackEnum
from audio_deepfake_adversarial_attacks_amd.evaluation import ShardedBatchSampler, format_report, shard_bounds
from oracle import torch_ops
from tests.helpers import Surrogate, surrogate_from

T = torch.from_numpy


@pytest.fixture(autouse=True)
def one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def armed(cls, model, **kw):
    atk = cls(model, **kw)
    atk.ops = torch_ops
    atk.set_training_mode(model_training=True, batchnorm_training=False)
    return atk


# ---- the plugin API ----------------------------------------------------------------------------------------------

def test_constructor_signatures_and_defaults():
    m = Surrogate()
    a = torchattacks.FGSM(m)
    assert (a.eps, a.attack) == (0.007, "FGSM")
    a = torchattacks.PGD(m)
    assert (a.eps, a.alpha, a.steps, a.random_start) == (0.3, 2 / 255, 40, True)
    a = torchattacks.PGDL2(m)
    assert (a.eps, a.alpha, a.steps, a.random_start, a.eps_for_division) == (1.0, 0.2, 40, True, 1e-10)
    a = torchattacks.CW(m)
    assert (a.c, a.kappa, a.steps, a.lr) == (1e-4, 0, 1000, 0.01)
    assert a.device == next(m.parameters()).device and a.model is m and a.model_name == "Surrogate"
    assert str(torchattacks.PGD(m, eps=0.003)) == ("PGD(model_name=Surrogate, device=cpu, eps=0.003, "
                                                   "alpha=0.00784313725490196, steps=40, random_start=True, "
                                                   "attack_mode=default, return_type=float)")


def test_mode_and_return_type_errors():
    m = Surrogate()
    base = torchattacks.Attack("X", m)
    with pytest.raises(NotImplementedError):
        base.forward(None, None)
    with pytest.raises(ValueError, match="Targeted mode is not supported"):
        base.set_mode_targeted_by_function(None)
    with pytest.raises(ValueError, match="not a valid type"):
        base.set_return_type("uint8")
    a = torchattacks.PGD(m)
    a.set_mode_targeted_by_function(lambda images, labels: 1 - labels)
    assert a.get_mode() == "targeted" and a._targeted
    a.set_mode_default()
    assert a.get_mode() == "default" and not a._targeted
    a.set_return_type("int")
    assert a._return_type == "int"


def test_call_juggles_training_mode_like_the_reference():
    """attack.py:308-331: train() for the attack, BatchNorm/Dropout forced to eval, previous mode restored."""
    seen = {}

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.conv = torch.nn.Conv1d(1, 2, 5)
            self.bn = torch.nn.BatchNorm1d(2)
            self.drop = torch.nn.Dropout(0.5)
            self.rnn = torch.nn.GRU(2, 2, batch_first=True)
            self.fc = torch.nn.Linear(2, 1)

        def forward(self, x):
            seen.update(net=self.training, bn=self.bn.training, drop=self.drop.training, rnn=self.rnn.training)
            h = self.drop(self.bn(self.conv(x.unsqueeze(1))))
            o, _ = self.rnn(h.transpose(1, 2))
            return self.fc(o.mean(1))

    net = Net().eval()
    x, y = torch.rand(2, 64), torch.tensor([0, 1])
    atk = armed(torchattacks.FGSM, net, eps=0.01)
    atk(x, y)
    assert seen == {"net": True, "bn": False, "drop": False, "rnn": True}
    # reference quirk kept (attack.py:325-326 only restores TRAIN mode): a model that was in eval mode is left in
    # train mode with its BatchNorm / Dropout layers in eval
    assert net.training and not net.bn.training and not net.drop.training
    atk.set_training_mode(model_training=True, batchnorm_training=True, dropout_training=True)
    atk(x, y)
    assert seen == {"net": True, "bn": True, "drop": True, "rnn": True}
    atk.set_training_mode(model_training=False)
    net.train()
    atk(x, y)
    assert seen["net"] is False and net.training  # eval during the attack, caller's train mode restored


def test_inputs_are_not_mutated_and_output_is_detached():
    m = Surrogate()
    x, y = torch.rand(3, 256), torch.tensor([0, 1, 1])
    x0 = x.clone()
    for cls, kw in ((torchattacks.FGSM, {"eps": 0.01}), (torchattacks.PGD, {"eps": 0.01, "steps": 2}),
                    (torchattacks.PGDL2, {"eps": 0.1, "steps": 2}), (torchattacks.CW, {"c": 1.0, "steps": 3})):
        adv = armed(cls, m, **kw)(x, y)
        assert torch.equal(x, x0) and not adv.requires_grad and adv.shape == x.shape and adv.dtype == torch.float32
        assert adv.data_ptr() != x.data_ptr()
        assert adv.min() >= 0 and adv.max() <= 1


def test_return_type_int():
    m = Surrogate()
    atk = armed(torchattacks.FGSM, m, eps=0.01)
    atk.set_return_type("int")
    assert atk(torch.rand(2, 64), torch.tensor([0, 1])).dtype == torch.uint8


def test_product_attacks_with_oracle_ops_reproduce_reference(golden):
    """Host logic + oracle kernels == reference outputs: bit-exact for the sign attacks, norm tolerance for PGDL2,
    stated tolerance for CW."""
    g = golden("fgsm")
    m = surrogate_from(g)
    for e, eps in (("e0005", 0.0005), ("e001", 0.001)):
        adv = armed(torchattacks.FGSM, m, eps=eps)(T(g[f"ragged_{e}_x"]), T(g[f"ragged_{e}_y"]))
        assert torch.equal(adv, T(g[f"ragged_{e}_adv"]))  # north-star bound for FGSM: 1e-5 max-abs; we get 0
    g = golden("pgd_linf")
    m = surrogate_from(g)
    for tag in ("ragged_rs", "small_nors", "full_rs"):
        atk = armed(torchattacks.PGD, m, eps=float(g[tag + "_eps"]), steps=int(g[tag + "_steps"]),
                    random_start=tag.endswith("_rs"))
        if tag + "_noise" in g:
            atk.set_init_noise(T(g[tag + "_noise"]))
        assert torch.equal(atk(T(g[tag + "_x"]), T(g[tag + "_y"])), T(g[tag + "_adv"])), tag
    g = golden("pgd_l2")
    m = surrogate_from(g)
    for tag in ("ragged_rs", "small_nors"):
        atk = armed(torchattacks.PGDL2, m, eps=float(g[tag + "_eps"]), steps=int(g[tag + "_steps"]),
                    random_start=tag.endswith("_rs"))
        if tag + "_normal" in g:
            atk.set_init_noise((T(g[tag + "_normal"]), T(g[tag + "_r"])))
        adv = atk(T(g[tag + "_x"]), T(g[tag + "_y"]))
        assert (adv - T(g[tag + "_adv"])).abs().max() <= 3e-7, tag
    g = golden("cw")
    m = surrogate_from(g)
    best = armed(torchattacks.CW, m, c=float(g["c"]), steps=int(g["steps"]), lr=float(g["lr"]))(T(g["x"]), T(g["y"]))
    err = (best - T(g["best"])).abs()
    # CW tolerance: Adam turns rounding-level gradients into +-lr moves on a handful of coordinates
    assert err.mean() <= 1e-6 and (err > 1e-4).float().mean() <= 1e-3 and err.max() <= 0.02
    unchanged = T(g["best"]) == T(g["x"])
    assert torch.equal(best == T(g["x"]), unchanged) or (best == T(g["x"])).float().mean() > 0.2


def test_random_start_uses_global_generator_and_stays_in_ball():
    m = Surrogate()
    x, y = torch.rand(2, 500), torch.tensor([1, 0])
    atk = armed(torchattacks.PGD, m, eps=0.01, steps=1)
    torch.manual_seed(5)
    a = atk(x, y)
    torch.manual_seed(5)
    b = atk(x, y)
    c = atk(x, y)
    assert torch.equal(a, b) and not torch.equal(a, c) and (a - x).abs().max() <= 0.01 + 1e-7


def test_targeted_mode_flips_the_gradient_sign():
    m = Surrogate()
    x, y = torch.rand(2, 300) * 0.5 + 0.25, torch.tensor([1, 0])
    plain = armed(torchattacks.FGSM, m, eps=0.01)(x, y)
    atk = armed(torchattacks.FGSM, m, eps=0.01)
    atk.set_mode_targeted_by_function(lambda images, labels: labels)  # target == label -> cost = -CE -> opposite step
    tgt = atk(x, y)
    assert torch.allclose((plain - x), -(tgt - x), atol=1e-7)


def test_attack_without_library_or_gpu_fails_loudly():
    """The default op table is the HIP one: on a CPU model it must refuse, never fall back."""
    from audio_deepfake_adversarial_attacks_amd._lib import AdvstepError
    atk = torchattacks.FGSM(Surrogate(), eps=0.01)
    with pytest.raises(AdvstepError, match="no CPU fallback"):
        atk(torch.rand(2, 64), torch.tensor([0, 1]))


# ---- registry --------------------------------------------------------------------------------------------------------

def test_attack_enum_keeps_reference_members_and_adds_baseline_configs():
    ref = {  # src/aa/aa_types.py:8-24
        "PGD": ("PGD", {"eps": 0.0005, "steps": 10}), "PGD_eps00075": ("PGD", {"eps": 0.00075, "steps": 10}),
        "PGD_eps001": ("PGD", {"eps": 0.001, "steps": 10}), "PGDL2": ("PGDL2", {"eps": 0.1, "steps": 10}),
        "PGDL2_eps15": ("PGDL2", {"eps": 0.15, "steps": 10}), "PGDL2_eps20": ("PGDL2", {"eps": 0.20, "steps": 10}),
        "FGSM": ("FGSM", {"eps": 0.0005}), "FGSM_eps00075": ("FGSM", {"eps": 0.00075}),
        "FGSM_eps001": ("FGSM", {"eps": 0.001}),
        "FAB": ("FAB", {"n_classes": 2, "eta": 10}), "FAB_eta20": ("FAB", {"n_classes": 2, "eta": 20}),
        "FAB_eta30": ("FAB", {"n_classes": 2, "eta": 30}),
    }
    for name, (cls, kw) in ref.items():
        got_cls, got_kw = AttackEnum[name].value
        assert got_cls.__name__ == cls and got_kw == kw
    assert AttackEnum.NO_ATTACK.value == (None, {})
    cls, kw = AttackEnum.PGD40_eps003.value
    assert cls is torchattacks.PGD and kw == {"eps": 0.003, "steps": 40}
    assert AttackEnum.PGDL2_40.value[1]["steps"] == 40 and AttackEnum.CW.value[0] is torchattacks.CW


# ---- metrics -----------------------------------------------------------------------------------------------------------

def test_metrics_match_the_reference_calls(golden):
    g = golden("metrics")
    for tag in ("random", "separable", "tiny"):
        y, s = g[tag + "_y"], g[tag + "_score"]
        thresh, eer, fpr, tpr = metrics.calculate_eer(1 - y, s)
        assert abs(eer - g[tag + "_eer"]) <= 1e-12 and abs(thresh - g[tag + "_thresh"]) <= 1e-12
        rep = metrics.adversarial_report(y, s, (s + 0.5).astype(np.int32))
        for k in ("precision", "recall", "f1", "auc", "accuracy"):
            key = "adv_eval/" + ("f1_score" if k == "f1" else k)
            assert abs(rep[key] - g[f"{tag}_{k}"]) <= 1e-12, (tag, k)
    line = format_report(rep)
    assert line.startswith("adv_eval/eer: ") and line.count("adv_eval/") == 6 and "adv_eval/auc" in line


def test_metrics_edge_cases():
    with pytest.raises(ValueError):
        metrics.roc_auc_score(np.ones(4), np.arange(4.0))
    assert metrics.precision_recall_f1_binary([0, 0], [0, 0]) == (0.0, 0.0, 0.0)
    y = np.array([0, 0, 1, 1])
    _, eer, _, _ = metrics.calculate_eer(1 - y, np.array([0.1, 0.2, 0.8, 0.9], np.float32))
    assert eer == 0.0
    assert metrics.roc_auc_score(y, [0.1, 0.2, 0.8, 0.9]) == 1.0


# ---- sharding ------------------------------------------------------------------------------------------------------------

def test_shard_bounds_match_torch_chunk():
    for n in (1, 7, 8, 64, 128, 1000, 1024):
        for world in (1, 2, 3, 4, 8):
            chunks = torch.arange(n).chunk(world)
            for r in range(world):
                lo, hi = shard_bounds(n, r, world)
                want = chunks[r].tolist() if r < len(chunks) else []
                assert list(range(lo, hi)) == want, (n, world, r)


def test_sharded_sampler_partitions_every_global_batch():
    n, gb, world = 1000, 64, 4
    per_rank = [list(ShardedBatchSampler(n, gb, r, world, shuffle=True, seed=3)) for r in range(world)]
    assert all(len(p) == n // gb for p in per_rank)
    ref = list(ShardedBatchSampler(n, gb, 0, 1, shuffle=True, seed=3))
    for b in range(n // gb):
        glued = sum((per_rank[r][b] for r in range(world)), [])
        assert glued == ref[b] and len(set(glued)) == gb           # contiguous chunks, in rank order
    assert sorted(sum(ref, [])) != sum(ref, [])                     # shuffled
    assert len(set(sum(ref, []))) == (n // gb) * gb                 # drop_last, no repeats
    with pytest.raises(ValueError):
        ShardedBatchSampler(n, 65, 0, 4)


# ---- FAB host logic (product class, oracle op table on CPU) against the reference's own runs -------------------------------

def _fab_fixture(golden):
    g = golden("fab_attack")
    return g, surrogate_from(g), torch.from_numpy(g["x01"]), torch.from_numpy(g["labels"])


def test_fab_class_mirrors_reference_attributes():
    atk = torchattacks.FAB(Surrogate(), n_classes=2, eta=10)
    assert (atk.attack, atk.norm, atk.eps, atk.steps, atk.n_restarts) == ("FAB", "Linf", 0.3, 100, 1)
    assert (atk.alpha_max, atk.eta, atk.beta, atk.seed, atk.verbose) == (0.1, 10, 0.9, 0, False)
    assert atk.targeted is False and atk.target_class is None and atk.n_target_classes == 1   # fab.py:63,66,67
    assert torchattacks.FAB(Surrogate(), norm="L2").eps == 1.0 and torchattacks.FAB(Surrogate(), norm="L1").eps == 5.0
    assert torchattacks.FAB(Surrogate(), targeted=True).targeted is False                      # ignored, as upstream
    with pytest.raises(ValueError):
        atk.set_mode_targeted_least_likely()                                                   # _supported_mode: default only
    with pytest.raises(KeyError):
        torchattacks.FAB(Surrogate(), norm="L0")


def test_fab_whole_runs_match_reference(golden):
    """FAB.forward / attack_single_run of the product class with the CPU op table: 5e-6 max-abs against the reference's
    adversarial waveforms (eta = 1.05); untouched rows bit-identical; the eps filter of perturb() rejects like upstream."""
    g, model, x01, y = _fab_fixture(golden)
    for name, norm in (("linf", "Linf"), ("linf_tight", "Linf"), ("l2", "L2")):
        eta, steps, eps = g[f"{name}_params"]
        atk = torchattacks.FAB(model, norm=norm, n_classes=2, eta=float(eta), steps=int(steps), eps=float(eps))
        atk.ops = torch_ops
        atk.set_training_mode(True, False, False)
        adv = atk(x01, y)
        assert adv.shape == x01.shape and adv.dtype == torch.float32 and not adv.requires_grad
        assert np.abs(adv.numpy() - g[f"{name}_adv"]).max() <= 5e-6, name
        assert np.array_equal(adv[2].numpy(), g["x01"][2])
        run = atk.attack_single_run(x01, y)
        assert np.abs(run.numpy() - g[f"{name}_single_run"]).max() <= 5e-6, name
    assert np.array_equal(g["linf_tight_adv"], g["x01"])


def test_fab_l1_forward_works_where_reference_raises(golden):
    g, model, x01, y = _fab_fixture(golden)
    assert bool(g["l1_forward_raises"])                       # upstream: UnboundLocalError at fab.py:522
    atk = torchattacks.FAB(model, norm="L1", n_classes=2, eta=1.05, steps=12, eps=2000.0)
    atk.ops = torch_ops
    adv = atk(x01, y)
    n_mine, n_ref = (adv - x01).abs().sum(1).numpy(), np.abs(g["l1_single_run"] - g["x01"]).sum(axis=1)
    assert np.allclose(n_mine, n_ref, rtol=5e-4) and n_mine[2] == 0.0


def test_fab_restarts_draw_the_reference_random_start(golden):
    """perturb() re-seeds torch's generators with `seed` and the random start is drawn on the CPU generator then moved
    (fab.py:504-505,176): a second restart starts from the same points as the reference's would."""
    g, model, x01, y = _fab_fixture(golden)
    atk = torchattacks.FAB(model, n_classes=2, eta=1.05, steps=2, eps=0.05, n_restarts=2, seed=5)
    atk.ops = torch_ops
    seen = []
    orig = atk._random_start
    atk._random_start = lambda x0, res2: seen.append(orig(x0, res2)) or seen[-1]
    atk(x01, y)
    assert len(seen) == 1
    torch.manual_seed(5)
    rows = [0, 1, 3, 4, 5]
    t = 2 * torch.rand(5, x01.shape[1]) - 1
    want = (x01[rows] + 0.05 * t / t.abs().max(dim=1, keepdim=True)[0] * 0.5).clamp(0.0, 1.0)
    assert torch.equal(seen[0], want)


def test_fab_public_gradient_helpers_keep_reference_shapes(golden):
    g, model, x01, y = _fab_fixture(golden)
    atk = torchattacks.FAB(model, n_classes=2)
    df, dg = atk.get_diff_logits_grads_batch(x01, y)
    assert df.shape == (6, 2) and dg.shape == (6, 2, x01.shape[1])
    u = torch.arange(6)
    assert (df[u, y] == 1e10).all() and (dg[u, y] == 0).all()
    z = model(x01).detach().reshape(-1)
    assert torch.allclose(df[u, 1 - y], torch.where(y == 0, 2 * z, -2 * z))
    df_t, dg_t = atk.get_diff_logits_grads_batch_targeted(x01, y, 1 - y)
    assert df_t.shape == (6, 1) and dg_t.shape == (6, 1, x01.shape[1])
    assert torch.allclose(df_t[:, 0], df[u, 1 - y]) and torch.allclose(dg_t[:, 0], dg[u, 1 - y])


def test_res_block_shape_limits_mirror_the_kernels():
    """an oversize batch must take the fallback path instead of raising from inside the fused block — the
    predicate restates resconv_check / fewin_dims_ok (32-bit buffer offsets per tensor, grid.y <= 65535)."""
    from audio_deepfake_adversarial_attacks_amd import detector_ops as D
    assert D.res_block_shape_supported((128, 2, 80, 404), 20)           # BASELINE configs[2], block0
    assert D.res_block_shape_supported((128, 20, 40, 202), 64)
    assert not D.res_block_shape_supported((1024, 2, 80, 404), 20)      # 1024 x 20 x 80 x 404 x 4 B > 2 GiB
    assert not D.res_block_shape_supported((70_000, 1, 4, 4), 4)        # grid.y


def test_same_conv1d_fallback_keeps_the_modules_padding_mode():
    """the helper's fallback must run the module's own forward (reflect / circular padding), also without bias."""
    import torch.nn as nn
    from audio_deepfake_adversarial_attacks_amd.models import rawnet3 as R
    torch.manual_seed(0)
    conv = nn.Conv1d(4, 4, 3, dilation=2, padding=2, padding_mode="reflect")
    x = torch.randn(2, 4, 20)
    assert torch.equal(R._same_conv1d(x, conv, True), conv(x))
    want = conv(x) - conv.bias.view(1, -1, 1)
    assert torch.allclose(R._same_conv1d(x, conv, False), want, atol=1e-6)
    zeros = nn.Conv1d(4, 4, 3, dilation=2, padding=2)
    assert torch.equal(R._same_conv1d(x, zeros, True), zeros(x))


def test_graph_cache_key_carries_switches_and_labels(monkeypatch):
    """what a captured graph bakes in beyond the weights — the ADVSTEP_* switches read at call time — is part of
    its key; clear() also forgets failed captures."""
    from audio_deepfake_adversarial_attacks_amd.torchattacks import graphed
    monkeypatch.setenv("ADVSTEP_L2_SINGLE_PASS", "1")
    a = graphed._toggles()
    monkeypatch.setenv("ADVSTEP_L2_SINGLE_PASS", "0")
    b = graphed._toggles()
    assert a != b and ("ADVSTEP_L2_SINGLE_PASS", "0") in b
    graphed._FAILED.add(("x",))
    graphed.clear()
    assert not graphed._FAILED and not graphed._GRAPHS and not graphed._SEEN


def test_save_reproduces_the_reference_files(golden, tmp_path):
    """Attack.save (attack.py:149-233) against the REFERENCE's own run (tests/golden/attack_save.npz): the saved
    (adversarials, labels, predictions) tuple, the returned robust accuracy and mean L2, for return types 'float' and 'int' —
    including the reference's quirk of leaving the return type at 'float' afterwards."""
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    from oracle import torch_ops
    from tests.helpers import surrogate_from
    g = golden("attack_save")
    model = surrogate_from(g)
    x, y = torch.from_numpy(g["x"]), torch.from_numpy(g["y"])
    loader = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(x, y), batch_size=2, shuffle=False)
    for kind in ("float", "int"):
        atk = torchattacks.FGSM(model, eps=0.001)
        atk.set_training_mode(model_training=True, batchnorm_training=False)
        atk.ops = torch_ops
        atk.set_return_type(kind)
        path = tmp_path / f"adv_{kind}.pt"
        rob_acc, l2, _ = atk.save(loader, save_path=str(path), verbose=False, return_verbose=True, save_pred=True)
        adv, labels, preds = torch.load(path)
        assert adv.dtype == (torch.uint8 if kind == "int" else torch.float32)
        assert np.array_equal(adv.numpy(), g[f"{kind}_adv"])
        assert np.array_equal(labels.numpy(), g[f"{kind}_labels"]) and np.array_equal(preds.numpy(), g[f"{kind}_preds"])
        assert rob_acc == float(g[f"{kind}_rob_acc"]) and abs(l2 - float(g[f"{kind}_l2"])) <= 1e-9
        assert atk._return_type == str(g[f"{kind}_return_type_after"]) == "float"


def test_row_workspace_table_is_a_bounded_lru_and_graphs_take_their_buffers_out(monkeypatch):
    """one scratch buffer per (device, stream, B, T) — the C ABI's "one workspace, one stream, one shape" rule
    (include/advstep.h) — but no more than a fixed number alive, least recently used first out, and a captured graph's
    buffers leave the table so that a stream re-using the capture stream's handle never shares them.  Host logic only:
    the library and the stream handle are stubbed, buffers are CPU tensors."""
    from audio_deepfake_adversarial_attacks_amd import hip_ops

    class _Lib:
        @staticmethod
        def advstep_row_workspace_bytes(B, T):
            return 64 * B

    handle = {"v": 11}
    monkeypatch.setattr(hip_ops._lib, "load", lambda: _Lib)
    monkeypatch.setattr(hip_ops, "_stream", lambda device: handle["v"])
    monkeypatch.setattr(hip_ops, "_workspaces", {})
    monkeypatch.setattr(hip_ops, "_WORKSPACE_SLOTS", 4)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    cpu = torch.device("cpu")
    first = hip_ops._workspace(cpu, 1, 100)
    assert hip_ops._workspace(cpu, 1, 100) == first                  # same key: same buffer, nothing re-zeroed
    for B in (2, 3, 4):
        hip_ops._workspace(cpu, B, 100)
    assert len(hip_ops._workspaces) == 4
    hip_ops._workspace(cpu, 1, 100)                                  # touch: B = 1 becomes the most recent
    hip_ops._workspace(cpu, 5, 100)                                  # evicts B = 2, the least recently used
    assert [k[2] for k in hip_ops._workspaces] == [3, 4, 1, 5]
    handle["v"] = 22                                                 # another stream: its own buffers
    ptr22, _ = hip_ops._workspace(cpu, 1, 100)
    assert ptr22 != first[0]
    taken = hip_ops.release_stream_workspaces(22)
    assert len(taken) == 1 and taken[0].data_ptr() == ptr22
    assert all(k[1] == 11 for k in hip_ops._workspaces)
    fresh, _ = hip_ops._workspace(cpu, 1, 100)                       # the handle comes round again: a NEW zero-filled buffer
    assert fresh != ptr22 and int(hip_ops._workspaces[(0, 22, 1, 100)].sum()) == 0


def test_in_flight_defaults_and_cpu_lanes(monkeypatch):
    """evaluation._Lanes on a CPU device is a pass-through (the 2-rank gloo tests run the loop there); two batches in
    flight is the default only for attacks whose inner loop replays from a graph, on a HIP device, without a callback."""
    from audio_deepfake_adversarial_attacks_amd import evaluation
    lanes = evaluation._Lanes("cpu", 2)
    assert lanes.n == 1
    with lanes.batch(0, (4, 10)) as lane:
        assert lane == 0
    lanes.keep(torch.zeros(1))
    lanes.join()
    pgd = torchattacks.PGD(Surrogate(), steps=4)
    cw = torchattacks.CW(Surrogate(), steps=4)
    monkeypatch.delenv("ADVSTEP_IN_FLIGHT", raising=False)
    monkeypatch.delenv("ADVSTEP_ATTACK_GRAPH", raising=False)
    assert evaluation.default_in_flight(pgd, "cuda:0", False) == 2
    assert evaluation.default_in_flight(pgd, "cuda:0", True) == 1          # the analyser's callback reads every batch back
    assert evaluation.default_in_flight(pgd, "cpu", False) == 1
    assert evaluation.default_in_flight(cw, "cuda:0", False) == 1          # host-driven loop
    assert evaluation.default_in_flight(None, "cuda:0", False) == 1
    monkeypatch.setenv("ADVSTEP_ATTACK_GRAPH", "0")
    assert evaluation.default_in_flight(pgd, "cuda:0", False) == 1         # eager launches keep the host busy: nothing to overlap
    monkeypatch.setenv("ADVSTEP_IN_FLIGHT", "3")
    assert evaluation.default_in_flight(cw, "cuda:0", True) == 3


# ---- csrc/lcnn_wino_plan.h: which launches one Winograd convolution becomes -------------------------------------------------

_WINO_PLAN_PROBE = r"""
#include <stdio.h>
#include "lcnn_wino_plan.h"
int main() {
    int epi, src, gen, slices;
    long long N, K, H, W, Cout;
    while (scanf("%d %d %d %lld %lld %lld %lld %lld %d", &epi, &src, &gen, &N, &K, &H, &W, &Cout, &slices) == 9) {
        const WinoPlan p = plan_wino((Epi)epi, (Src)src, gen != 0, N, K, H, W, Cout, slices, read_wino_knobs());
        for (int i = 0; i < p.count; ++i) {
            const WinoLaunch &l = p.launch[i];
            printf("%d %d %d %d %d %d %d %d %zu;", l.NT, (int)l.stream, (int)l.wodd, l.halves, l.n_slices, l.slice0, l.ranges, l.xcd,
                   l.lds);
        }
        printf("\n");
    }
    return 0;
}
"""


def _wino_launches_before_the_plan(epi, src, gen, N, K, H, W, Cout, slices, env):
    """What launch_wino launched before plan_wino existed, restated from that function: (NT, stream, wodd, halves, slices of the
    launch, first slice, ranges, xcd, LDS bytes) per launch, in launch order."""
    def cdiv(a, b):
        return -(-a // b)

    def off(name):
        return env.get(name, "")[:1] == "0"
    chunks = cdiv(K, 16)
    stream = chunks > 4
    groups = cdiv(N * ((H + 1) // 2) * ((W + 1) // 2), 16)
    lds = ((4 if src == 1 else 2) if stream else chunks) * 16 * 16 * 32 * 4
    wodd = src == 0 and W % 2 == 1
    m = env.get("ADVSTEP_WINO_RANGE_MULT", "")[:1]
    mult = int(m) if m and "1" <= m <= "8" else 1
    out = []

    def go(NT, halves, n_slices, slice0):
        ranges = mult * 256 // n_slices
        if ranges * 8 > groups:
            ranges = cdiv(groups, 8)
        ranges = max(ranges, 1)
        xcd, r8 = 0, ranges & ~7
        if not off("ADVSTEP_WINO_XCD") and n_slices > 1 and r8 >= 8 and cdiv(groups, r8 * 8) == cdiv(groups, ranges * 8):
            ranges, xcd = r8, 1
        out.append((NT, int(stream), int(wodd), halves, n_slices, slice0, ranges, xcd, lds))
    full = slices
    if epi in (0, 3, 5, 6) and Cout - (slices - 1) * 32 <= 16 and not off("ADVSTEP_WINO_HALF_SLICE"):
        full = slices - 1
        go(1, 0, 1, slices - 1)
    if (epi == 0 and src == 1 and not gen and full == 1 and slices == 1 and Cout == 32 and groups <= 256 * 8 // 2
            and not off("ADVSTEP_WINO_HALVES")):
        go(1, 1, 2, 0)
        return out
    if full > 0:
        go(2, 0, full, 0)
    return out


def test_wino_launch_plan_is_what_launch_wino_used_to_decide(tmp_path):
    """plan_wino (plain host C++) against a restatement of the launch logic it replaced, for every epilogue / source pair the
    library launches, at model shapes and at shapes where the range count is capped, under every setting of the four knobs it
    reads: the half-empty last slice on its own, the two-halves launch, ranges rounded to a multiple of 8 with xcd set,
    ADVSTEP_WINO_RANGE_MULT."""
    import os
    import shutil
    import subprocess
    from audio_deepfake_adversarial_attacks_amd import build as B
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src_file, exe = tmp_path / "wino_plan_probe.cpp", tmp_path / "wino_plan_probe"
    src_file.write_text(_WINO_PLAN_PROBE)
    subprocess.run([hipcc, "--cuda-host-only", "-x", "hip", "-std=c++17", "-O0", f"-I{B.ROOT / 'include'}", f"-I{B.PKG / 'csrc'}",
                    str(src_file), "-o", str(exe)], check=True, capture_output=True)
    pairs = [(1, 0, 0), (2, 0, 0), (0, 0, 0), (0, 1, 0), (3, 0, 1), (4, 0, 1), (7, 0, 1), (0, 2, 1), (5, 2, 1), (6, 2, 1)]   # (Epi, Src, GEN)
    shapes = [  # (N, K, H, W, Cout, slices)
        (128, 32, 202, 40, 48, 3), (128, 128, 101, 20, 48, 2), (128, 64, 50, 10, 32, 1), (128, 96, 50, 10, 32, 1),
        (129, 64, 50, 10, 32, 1), (128, 24, 80, 404, 20, 1), (128, 84, 20, 101, 64, 2), (128, 64, 5, 25, 64, 2),
        (2, 64, 7, 10, 48, 2), (3, 128, 6, 9, 80, 3), (1, 8, 2, 2, 16, 1), (1, 256, 8, 6, 256, 8), (16, 20, 20, 101, 33, 2),
    ]
    cases = [(e, s, g) + sh for e, s, g in pairs for sh in shapes]
    knobs = [{}, {"ADVSTEP_WINO_HALF_SLICE": "0"}, {"ADVSTEP_WINO_HALVES": "0"}, {"ADVSTEP_WINO_XCD": "0"},
             {"ADVSTEP_WINO_RANGE_MULT": "2"}, {"ADVSTEP_WINO_RANGE_MULT": "4", "ADVSTEP_WINO_XCD": "0"},
             {"ADVSTEP_WINO_RANGE_MULT": "9"}, {"ADVSTEP_WINO_HALVES": "1", "ADVSTEP_WINO_XCD": "1"}]
    stdin = "".join(" ".join(map(str, c)) + "\n" for c in cases)
    seen = set()
    for env in knobs:
        clean = {k: v for k, v in os.environ.items() if not k.startswith("ADVSTEP_WINO_")}
        got = subprocess.run([str(exe)], input=stdin, env={**clean, **env}, check=True, capture_output=True, text=True).stdout
        lines = got.splitlines()
        assert len(lines) == len(cases)
        for c, line in zip(cases, lines):
            plan = [tuple(int(v) for v in part.split()) for part in line.split(";") if part]
            assert plan == _wino_launches_before_the_plan(*c, env), (c, env)
            seen.update((l[0], l[3], l[7]) for l in plan)
    # the branches the cases are there for: one-tile last slice, the two halves, xcd placement, and plain two-tile launches
    assert {(1, 0, 0), (1, 1, 0), (2, 0, 1), (2, 0, 0)} <= seen       # (NT, halves, xcd)
