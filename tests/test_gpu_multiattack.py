"""`-m gpu`: the MultiAttack row router (include/advstep_multi.h) against its restatement by plain torch indexing
(tests/multiattack_cpu_ops.py), whole MultiAttack calls on the detectors against a loop written here with eager indexing,
hipGraph replay of the full-batch member, and the evaluation loop.

Nothing here has a tolerance: the router only moves bytes, so every comparison is on the bit patterns (NaN payloads and signed
zeros included)."""
import numpy as np
import pytest
import torch

from tests import multiattack_cpu_ops as C
from tests.test_gpu_apgd import detector

pytestmark = pytest.mark.gpu

# one row; an odd T across two tiles; four tiles with an odd T; the aligned float4 path; more than two 64-lane ballots
SHAPES = [(1, 257), (5, 4099), (7, 12_289), (64, 1024), (130, 257)]
PATTERNS = ["none", "all", "alternating", "random"]
PAD = 1024                                   # canary elements either side of an output (4096 bytes: keeps 16-byte alignment)
SPECIAL_Z = [0.0, -0.0, float("nan"), float("inf"), float("-inf"), 0.75, -0.25, 1e-40, -1e-40]


def hip():
    from audio_deepfake_adversarial_attacks_amd import hip_ops
    return hip_ops


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def padded(shape, fill, dtype, cuda, shift=0):
    """A buffer of `fill` with the tensor of `shape` in its middle (`shift` elements further: a base that is not 16-byte
    aligned).  Returns (buffer, view)."""
    n = int(np.prod(shape))
    buf = torch.full((PAD + shift + n + PAD,), fill, dtype=dtype, device=cuda)
    return buf, buf[PAD + shift:PAD + shift + n].view(shape)


def untouched(buf, fill, n, shift=0):
    return bool((buf[:PAD + shift] == fill).all() and (buf[PAD + shift + n:] == fill).all())


def route_inputs(n, T, pattern, seed):
    g = torch.Generator().manual_seed(seed)
    B = n + 3
    adv, x = torch.rand(n, T, generator=g), torch.rand(n, T, generator=g)
    adv[:, ::29] = float("nan")
    adv[:, 1::31] = -0.0
    x[:, 2::37] = float("nan")
    x[:, ::41] = -0.0
    z = torch.randn(n, generator=g)
    for i in range(n):
        if i % 2 == 0 or n < 4:
            z[i] = SPECIAL_Z[(i // 2 + seed) % len(SPECIAL_Z)]
    pre = (z > 0).long()                                                       # NaN, +-0 and -inf: class 0
    wrong = {"none": torch.zeros(n, dtype=torch.bool), "all": torch.ones(n, dtype=torch.bool),
             "alternating": torch.arange(n) % 2 == 0, "random": torch.rand(n, generator=g) < 0.5}[pattern]
    labels = torch.where(wrong, 1 - pre, pre)
    rows = torch.randperm(B, generator=g)[:n].sort().values.to(torch.int32)    # a sorted random subset of the full batch
    return adv, x, z, labels, rows, wrong, B


def launch_and_check(cuda, n, T, pattern, seed, shift):
    adv, x, z, labels, rows, wrong, B = route_inputs(n, T, pattern, seed)
    g = torch.Generator().manual_seed(seed + 1)
    final0 = torch.rand(B, T, generator=g)

    def shifted(t):                                                            # the same values from a base off by `shift` floats
        buf = torch.empty(t.numel() + shift, dtype=t.dtype, device=cuda)
        view = buf[shift:].view(t.shape)
        view.copy_(t)
        return view

    def launch():
        fbuf, final = padded((B, T), -7.25, torch.float32, cuda, shift)
        final.copy_(final0)
        xbuf, next_x = padded((n, T), 9.125, torch.float32, cuda, shift)
        ybuf, next_y = padded((n,), -5, torch.int64, cuda)
        rbuf, next_rows = padded((n,), -6, torch.int32, cuda)
        out = hip().multi_route(shifted(adv), shifted(x), z.to(cuda), labels.to(cuda), rows.to(cuda), final, next_x=next_x,
                                next_y=next_y, next_rows=next_rows)
        torch.cuda.synchronize()
        assert out[0].data_ptr() == next_x.data_ptr() and out[1].data_ptr() == next_y.data_ptr()
        assert out[2].data_ptr() == next_rows.data_ptr()
        assert untouched(fbuf, -7.25, B * T, shift) and untouched(xbuf, 9.125, n * T, shift)
        assert untouched(ybuf, -5, n) and untouched(rbuf, -6, n)
        return final.cpu(), next_x.cpu(), next_y.cpu(), next_rows.cpu(), out[3].cpu()

    final, next_x, next_y, next_rows, counts = launch()
    # the restatement, from the same inputs and the same pre-filled outputs
    w_final = final0.clone()
    w_x, w_y, w_rows = torch.full((n, T), 9.125), torch.full((n,), -5, dtype=torch.int64), torch.full((n,), -6, dtype=torch.int32)
    *_, w_counts = C.multi_route(adv, x, z, labels, rows, w_final, next_x=w_x, next_y=w_y, next_rows=w_rows)
    k = int((~wrong).sum())
    assert counts.dtype == torch.int32 and counts.tolist() == w_counts.tolist() == [n - k, k]        # exact
    assert same_bits(final, w_final) and same_bits(next_x, w_x) and torch.equal(next_y, w_y) and torch.equal(next_rows, w_rows)
    # said directly: rows of final nobody names are bit-unchanged; rows past counts[1] of the next_* buffers are not written
    named = torch.zeros(B, dtype=torch.bool)
    named[rows[wrong].long()] = True
    assert same_bits(final[~named], final0[~named]) and same_bits(final[named], adv[wrong])
    assert (next_x[k:] == 9.125).all() and (next_y[k:] == -5).all() and (next_rows[k:] == -6).all()
    again = launch()                                                           # no atomics: reruns are bit-identical
    for a, b in zip((final, next_x, next_y, next_rows, counts), again):
        assert same_bits(a, b)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n,T", SHAPES)
def test_multi_route_kernel(cuda, n, T, pattern):
    launch_and_check(cuda, n, T, pattern, seed=100 + n + T + PATTERNS.index(pattern), shift=0)


@pytest.mark.parametrize("n,T", [(64, 1024), (5, 4099)])
def test_multi_route_kernel_unaligned_bases(cuda, n, T):
    """Every waveform base pointer one float past a 16-byte boundary: the scalar path, also where T % 4 == 0."""
    launch_and_check(cuda, n, T, "random", seed=7 + n, shift=1)


def test_multi_route_defaults_and_empty(cuda):
    """Without caller buffers the outputs are fresh n-row tensors; an empty sub-batch launches nothing and counts zero."""
    adv, x, z, labels, rows, wrong, B = route_inputs(5, 260, "alternating", 3)
    final = torch.zeros(B, 260, device=cuda)
    nx, ny, nr, counts = hip().multi_route(adv.to(cuda), x.to(cuda), z.to(cuda), labels.to(cuda), rows.to(cuda), final)
    k = int((~wrong).sum())
    assert nx.shape == (5, 260) and ny.shape == (5,) and nr.shape == (5,) and counts.tolist() == [5 - k, k]
    assert same_bits(nx[:k], x[~wrong]) and torch.equal(nr[:k].cpu(), rows[~wrong])
    e = torch.empty(0, 260, device=cuda)
    out = hip().multi_route(e, e.clone(), torch.empty(0, device=cuda), torch.empty(0, dtype=torch.int64, device=cuda),
                            torch.empty(0, dtype=torch.int32, device=cuda), final)
    assert out[0].shape == (0, 260) and out[3].tolist() == [0, 0]
    from audio_deepfake_adversarial_attacks_amd import _lib
    with pytest.raises(_lib.AdvstepError, match="advstep_multi_route_f32"):     # no compaction in place
        hip().multi_route(adv.to(cuda), (xd := x.to(cuda)), z.to(cuda), labels.to(cuda), rows.to(cuda), final, next_x=xd)


# ---- whole attacks ---------------------------------------------------------------------------------------------------------

def batch_with_two_flipped_labels(model, cuda, seed):
    from audio_deepfake_adversarial_attacks_amd.datasets.synthetic import synthetic_waveforms
    x, _ = synthetic_waveforms(6, seed=seed)
    x01, _, _ = hip().to_minmax(x.to(cuda))
    with torch.no_grad():
        y = (model.eval()(x01).reshape(-1) > 0).long()                          # every row classified correctly ...
    y[1], y[4] = 1 - y[1], 1 - y[4]                                             # ... but two
    return x01, y


def eager_loop(members, model, x, y):
    """multiattack.py:45-70 with eager indexing, judged on z > 0 by the model in eval mode."""
    fails = torch.arange(x.shape[0], device=x.device)
    final = x.clone()
    records = [x.shape[0]]
    for attack in members:
        adv = attack(x[fails], y[fails])
        model.eval()
        with torch.no_grad():
            pre = (model(adv).reshape(-1) > 0).long()
        wrong = pre != y[fails]
        final[fails[wrong]] = adv[wrong]
        fails = fails[~wrong]
        records.append(len(fails))
        if len(fails) == 0:
            break
    return final, records


def recorded(atk):
    seen, update = [], atk._update_multi_atk_records
    atk._update_multi_atk_records = lambda records: (seen.append(list(records)), update(records))[1]
    atk._start_multi_atk_records()
    return seen


@pytest.mark.parametrize("model_name", ["lcnn", "specrnet"])
def test_multiattack_on_detectors_equals_the_eager_loop(cuda, model_name, monkeypatch):
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    monkeypatch.setenv("ADVSTEP_ATTACK_GRAPH", "0")
    model = detector(model_name, cuda)
    x01, y = batch_with_two_flipped_labels(model, cuda, seed=51)
    eps, steps = 0.003, 4
    # FGSM at eps = 0 returns its input: stage 1 succeeds on exactly the two flipped rows, stage 2 sees exactly four survivors
    members = [torchattacks.FGSM(model, eps=0.0), torchattacks.PGD(model, eps=eps, alpha=eps / steps, steps=steps),
               torchattacks.MIFGSM(model, eps=eps, alpha=eps / steps, steps=steps, decay=1.0)]
    atk = torchattacks.MultiAttack(members)
    atk.set_training_mode(model_training=True, batchnorm_training=False)
    seen = recorded(atk)
    torch.manual_seed(7)
    got = atk(x01, y)
    torch.manual_seed(7)                                                        # the same Philox keys for PGD's random starts
    want, records = eager_loop(members, model, x01, y)
    assert seen == [records]
    assert same_bits(got, want)
    print(f"  {model_name}: records {records}")
    assert records[0] == 6 and records[1] == 4 and all(a >= b for a, b in zip(records, records[1:]))
    moved = (got != x01).any(dim=1).cpu()
    assert same_bits(got[~moved], x01[~moved])
    assert int((~moved).sum()) == 2 + records[-1]         # the two rows stage 1 "flipped" with eps = 0, and the survivors
    assert got.data_ptr() != x01.data_ptr() and not model.training


def test_graph_replay_only_captures_the_full_batch(cuda, monkeypatch):
    """The same batch three times.  The first member (PGD at eps = 0: a graph-replayed identity) runs at the full batch and is
    captured at its second call; the second member always sees the same four survivors — a shape that WOULD be captured at
    its second call — and must stay eager.  The result equals the eager run bit for bit."""
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    from audio_deepfake_adversarial_attacks_amd.torchattacks import graphed
    model = detector("lcnn", cuda)
    x01, y = batch_with_two_flipped_labels(model, cuda, seed=52)
    members = [torchattacks.PGD(model, eps=0.0, alpha=0.0, steps=4),
               torchattacks.MIFGSM(model, eps=0.003, alpha=0.00075, steps=4, decay=1.0)]
    atk = torchattacks.MultiAttack(members)
    atk.set_training_mode(model_training=True, batchnorm_training=False)
    seen = recorded(atk)
    graphed.clear()
    try:
        monkeypatch.setenv("ADVSTEP_ATTACK_GRAPH", "0")
        torch.manual_seed(9)
        want = atk(x01, y)
        monkeypatch.setenv("ADVSTEP_ATTACK_GRAPH", "1")
        got = []
        for _ in range(3):
            torch.manual_seed(9)
            got.append(atk(x01, y))
        shapes = [key[4] for key in graphed._GRAPHS]
        assert shapes == [tuple(x01.shape)]                                     # one capture, of the full batch
        assert all(same_bits(g, want) for g in got)
        assert all(r[:2] == [6, 4] for r in seen) and len(seen) == 4 and all(r == seen[0] for r in seen)
        assert all(a._graph_off is False for a in members)
        # the switch is per attack object: on its own, at a repeated shape, the second member captures as it always did
        sub, sub_y = x01[:4].contiguous(), y[:4].contiguous()
        members[1](sub, sub_y), members[1](sub, sub_y)
        assert sorted(key[4] for key in graphed._GRAPHS) == sorted([tuple(x01.shape), (4, x01.shape[1])])
    finally:
        graphed.clear()


def test_evaluation_loop_reports_the_remaining_rows(cuda):
    """generate_attacks() with AttackEnum.WORSTCASE on synthetic data; a single attack's report is as it was."""
    import yaml
    from audio_deepfake_adversarial_attacks_amd.aa.aa_types import AttackEnum
    from audio_deepfake_adversarial_attacks_amd.datasets.synthetic import SyntheticDetectionDataset
    from audio_deepfake_adversarial_attacks_amd.evaluation import generate_attacks
    from audio_deepfake_adversarial_attacks_amd.utils import set_seed
    from tests.conftest import ROOT
    cfg = yaml.safe_load((ROOT / "configs" / "aa_evaluation" / "lcnn.yaml").read_text())

    def run(member):
        set_seed(42)
        cls, params = AttackEnum[member].value
        return generate_attacks([None, None, None], cfg, str(cuda), attack_model_config=cfg, attack_method=cls,
                                attack_params=params, batch_size=8, dataset=SyntheticDetectionDataset(20), share_weights=True)

    rep = run("WORSTCASE")
    remaining = rep["multi_attack/remaining"]
    print(f"  remaining after each member: {remaining}, accuracy {rep['adv_eval/accuracy']:.2f}")
    assert rep["num_total"] == 16 and remaining[0] == rep["num_total"] and len(remaining) == 4
    assert all(isinstance(r, int) for r in remaining) and all(a >= b for a, b in zip(remaining, remaining[1:]))
    assert 0.0 <= rep["adv_eval/accuracy"] <= 100.0
    assert "multi_attack/remaining" not in run("PGD")
