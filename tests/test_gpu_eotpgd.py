"""GPU: torchattacks.EOTPGD over a simulated audio channel — the loop's plumbing on a linear detector, with every channel_apply and
channel_eot_step launch replayed on the CPU table (tests/channel_cpu_ops.py) byte for byte; the identity channel against PGD; EOTPGD
on LCNN; the `channel/*` figures of the evaluation loop."""

import numpy as np
import pytest
import torch

from tests import channel_cpu_ops as C
from tests.test_channel_host import identity_case
from tests.test_gpu_apgd import atk_call_context, detector

pytestmark = pytest.mark.gpu


def hip():
    from audio_deepfake_adversarial_attacks_amd import hip_ops
    return hip_ops


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


class Recording:
    """hip_ops, with the inputs and the output of every channel_apply and channel_eot_step call copied at the call."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        return getattr(hip(), name)

    def _record(self, name, args, kw):
        keep = lambda v: v.detach().clone() if isinstance(v, torch.Tensor) else v                # noqa: E731
        args, kw = [keep(a) for a in args], {k: keep(v) for k, v in kw.items() if k != "out"}
        out = getattr(hip(), name)(*args, **kw)
        self.calls.append((name, args, kw, out.detach().clone()))
        return out

    def channel_apply(self, *args, out=None, **kw):
        res = self._record("channel_apply", args, kw)
        return res if out is None else out.copy_(res)

    def channel_eot_step(self, *args, out=None, **kw):
        res = self._record("channel_eot_step", args, kw)
        return res if out is None else out.copy_(res)


def test_every_launch_of_the_loop_equals_the_cpu_table(cuda):
    """steps = 3, eot_iter = 2, a 5-tap channel with delays and noise, on a linear detector.  Each recorded launch is recomputed
    by the table from the launch's own inputs (so the detector's rounding does not enter), and the plumbing is checked on the
    recorded tensors: the draws of step i are slices [2 i, 2 i + 2) of the call's one `Channel.draw`, the Philox offset is 2 i under
    one seed, a step reads the buffer the previous one wrote, `orig` is the input, and gradient slot j is the model's gradient at
    channelled copy j (recomputed on the device by the same code: equal bits)."""
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    model, x, y, noise = identity_case(B=3, T=300, seed=5)
    model = C.LinearDetector(model.w.detach().float(), model.bias).to(cuda)
    ch = torchattacks.Channel(taps=5, decay=0.5, max_shift=4, gain_db=3.0, snr_db=(25, 35))
    drawn = []
    draw = ch.draw
    ch.draw = lambda *a, **kw: drawn.append(draw(*a, **kw)) or drawn[-1]
    steps, K, eps, alpha = 3, 2, 0.01, 0.004
    atk = torchattacks.EOTPGD(model, eps=eps, alpha=alpha, steps=steps, eot_iter=K, channel=ch)
    rec = Recording()
    atk.ops = rec
    atk.set_init_noise(noise)
    mn, mx = torch.tensor([-1.0, -0.5, -0.25]), torch.tensor([1.0, 1.5, 0.75])
    atk.set_minmax(mn, mx)
    x_d, y_d = x.to(cuda), y.to(cuda)
    adv = atk(x_d, y_d)
    assert torch.equal(x_d.cpu(), x) and adv.shape == x.shape

    assert [c[0] for c in rec.calls] == ["channel_apply", "channel_eot_step"] * steps and len(drawn) == 1
    taps, shift, gain, amp = drawn[0]
    assert taps.shape == (steps * K, 3, 5)
    start = torch.clamp(x + noise, 0, 1)
    seeds = set()
    prev_out = None
    for it in range(steps):
        (_, a_args, a_kw, through), (_, s_args, s_kw, out) = rec.calls[2 * it], rec.calls[2 * it + 1]
        cur, center, h, s, g, a, seed, offset = a_args
        seeds.add(seed)
        d = slice(it * K, (it + 1) * K)
        assert offset == it * K and not a_kw
        assert torch.equal(center.cpu(), torch.tensor([0.5, 0.25, 0.25]))
        assert all(torch.equal(p, q[d]) for p, q in zip((h, s, g, a), (taps, shift, gain, amp)))
        assert torch.equal(bits(cur), bits(start if it == 0 else prev_out))
        want = C.channel_apply(cur, center, h, s, g, a, seed, offset)
        assert torch.equal(bits(through), bits(want)), it
        adv_in, orig, grads, h2, s2, g2, alpha_, eps_ = s_args
        assert (alpha_, eps_) == (alpha, eps) and not s_kw
        assert torch.equal(bits(adv_in), bits(cur)) and torch.equal(bits(orig), bits(x))
        assert all(torch.equal(p, q[d]) for p, q in zip((h2, s2, g2), (taps, shift, gain)))
        for j in range(K):
            gj, _ = atk._input_gradient(through[j].clone(), y_d, None)
            assert torch.equal(bits(grads[j]), bits(gj)) and bool((gj != 0).any())
        assert not torch.equal(grads[0], grads[1])
        want = C.channel_eot_step(adv_in, orig, grads, h2, s2, g2, alpha_, eps_)
        assert torch.equal(bits(out), bits(want)), it
        prev_out = out
    assert len(seeds) == 1 and torch.equal(bits(adv), bits(prev_out))


@pytest.mark.parametrize("eot_iter", (1, 3))
def test_identity_channel_equals_pgd(cuda, eot_iter):
    """tests.test_channel_host.identity_case: the identity channel hands the detector PGD's own bytes, and the sum of eot_iter
    equal gradients has the sign of one."""
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    model, x, y, noise = identity_case()
    model = C.LinearDetector(model.w.detach().float(), model.bias).to(cuda)
    kw = dict(eps=0.01, alpha=0.003, steps=4)

    def run(atk):
        atk.set_init_noise(noise)
        return atk(x.to(cuda), y.to(cuda))

    want = run(torchattacks.PGD(model, **kw))
    got = run(torchattacks.EOTPGD(model, eot_iter=eot_iter, channel=torchattacks.Channel.identity(), **kw))
    assert torch.equal(bits(got), bits(want)) and bool((want.cpu() != x).any())
    assert torch.equal(bits(run(torchattacks.EOTPGD(model, eot_iter=eot_iter, **kw))), bits(want))


def test_attack_on_lcnn(cuda):
    """B = 2, steps = 2, eot_iter = 2, the `mild` channel.  |adv - x| <= eps (1 + 2u) + u (the allowance of the PGD tests: d is
    within the float32 eps and adv = fl(x + d) rounds once at magnitude <= 1); adv in [0, 1]; the inputs keep their bytes; the
    same seed gives the same bytes; no host read inside the call."""
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    from audio_deepfake_adversarial_attacks_amd.datasets.synthetic import synthetic_waveforms
    model = detector("lcnn", cuda)
    x, y = synthetic_waveforms(2, seed=47)
    x01, mn, mx = hip().to_minmax(x.to(cuda))
    y = y.to(cuda)
    keep_x, keep_y = x01.clone(), y.clone()
    eps = 0.001
    atk = torchattacks.EOTPGD(model, eps=eps, alpha=eps / 2, steps=2, eot_iter=2, channel="mild")
    atk.set_training_mode(model_training=True, batchnorm_training=False)

    def call():
        torch.manual_seed(3)
        atk.set_minmax(mn, mx)
        return atk(x01, y)

    first = call()
    u = 2.0 ** -24
    d = (first.double() - x01.double()).abs().max().item()
    print(f"  max |adv - x| = {d:.9g}, eps = {eps}")
    assert d <= float(np.float32(eps)) * (1 + 2 * u) + u and d > 0
    assert float(first.min()) >= 0.0 and float(first.max()) <= 1.0
    assert torch.equal(bits(x01), bits(keep_x)) and torch.equal(y, keep_y)
    assert torch.equal(bits(call()), bits(first))

    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            torch.ones(1, device=cuda).item()                                   # the mode works on this build
        torch.manual_seed(3)
        atk.set_minmax(mn, mx)
        with atk_call_context(atk):
            quiet = atk.forward(x01, y)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert torch.equal(bits(quiet), bits(first))


# ---- through the loop --------------------------------------------------------------------------------------------------------------------

CFG = {"data": {"seed": 42}, "checkpoint": {"path": ""},
       "model": {"name": "lcnn", "parameters": {"frontend_algorithm": ["lfcc"], "input_channels": 1}}}
KEYS = ["channel/accuracy", "channel/clean_accuracy", "channel/survival", "channel/flipped", "channel/draws"]


def loop(cuda, method, params, **kw):
    from audio_deepfake_adversarial_attacks_amd.datasets.synthetic import SyntheticDetectionDataset
    from audio_deepfake_adversarial_attacks_amd.evaluation import generate_attacks
    torch.manual_seed(5)
    rep = generate_attacks([None, None, None], CFG, str(cuda), attack_model_config=CFG if method else None, attack_method=method,
                           attack_params=params, batch_size=4, dataset=SyntheticDetectionDataset(8), share_weights=True,
                           shuffle=False, num_workers=0, return_scores=True, **kw)
    torch.cuda.synchronize()
    return rep


def test_loop_identity_channel(cuda):
    """8 synthetic utterances, batch 4, the registry's EOTPGD at 2 steps of 2 draws.  Through the identity channel every
    (utterance, draw) pair is the unchannelled utterance: channel/accuracy is adv_eval/accuracy and channel/clean_accuracy the
    accuracy of a NO_ATTACK run; and the run with `channel=` reports the adv_eval scores of the run without it, bit for bit (the
    scorer draws from generators of its own).  The NO_ATTACK run goes through the `mild` channel twice per utterance: the keys are
    there, accuracies within [0, 100] per cent like adv_eval/accuracy, the survival share within [0, 1]."""
    from audio_deepfake_adversarial_attacks_amd.aa.aa_types import AttackEnum
    method, params = AttackEnum["EOTPGD"].value
    params = {**params, "steps": 2, "eot_iter": 2}
    plain = loop(cuda, method, params)
    assert not [k for k in plain if k.startswith("channel/")]
    rep = loop(cuda, method, params, channel="identity", channel_draws=1)
    assert [k for k in rep if k.startswith("channel/")] == KEYS
    assert np.array_equal(rep["scores"]["y_pred"], plain["scores"]["y_pred"])
    assert {k: v for k, v in rep.items() if k.startswith("adv_eval/")} == {k: v for k, v in plain.items() if k.startswith("adv_eval/")}
    assert rep["channel/accuracy"] == rep["adv_eval/accuracy"] and rep["channel/draws"] == 1

    clean = loop(cuda, None, {}, channel="mild", channel_draws=2)
    assert rep["channel/clean_accuracy"] == clean["adv_eval/accuracy"]
    assert [k for k in clean if k.startswith("channel/")] == KEYS and clean["channel/draws"] == 2
    for k in ("channel/accuracy", "channel/clean_accuracy"):
        assert 0.0 <= clean[k] / 100 <= 1.0
    assert 0.0 <= clean["channel/survival"] <= 1.0 and clean["channel/flipped"] == 0       # nothing attacked, nothing flipped
    assert clean["channel/accuracy"] == clean["channel/clean_accuracy"]                   # the same draws for both


def test_loop_mild_channel_with_an_attack(cuda):
    from audio_deepfake_adversarial_attacks_amd.aa.aa_types import AttackEnum
    method, params = AttackEnum["PGD"].value
    rep = loop(cuda, method, {**params, "steps": 2}, channel="mild", channel_draws=2)
    assert [k for k in rep if k.startswith("channel/")] == KEYS and rep["num_total"] == 8
    for k in ("channel/accuracy", "channel/clean_accuracy"):
        assert 0.0 <= rep[k] / 100 <= 1.0
    assert 0.0 <= rep["channel/survival"] <= 1.0 and 0 <= rep["channel/flipped"] <= 8
