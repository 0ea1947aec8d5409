"""CPU: host logic of the simulated audio channel and EOTPGD — the adjoint identity of the CPU table tests/channel_cpu_ops.py, the
sampler torchattacks.Channel, the constructor surface and the registry, argument validation of the three entry points of
include/advstep_channel.h without a device, EOTPGD(channel=None) against the reference's fixture and EOTPGD(identity) against PGD."""
import ctypes

import numpy as np
import pytest
import torch

from tests import channel_cpu_ops as C
from tests.helpers import golden_for_this_cpu, surrogate_from

T_ = torch.from_numpy


@pytest.fixture(scope="module")
def lib():
    from audio_deepfake_adversarial_attacks_amd import build
    build.build()
    from audio_deepfake_adversarial_attacks_amd import _lib
    return _lib.load()


def stub(T=8):
    return C.LinearDetector(torch.ones(T), torch.zeros(1))


# ---- the table: <A x - A c, gy> = <x - c, A^T gy> -------------------------------------------------------------------------------------

IDENTITY_CASES = [(1, 1, 0), (5, 3, 2), (5, 7, -3), (37, 5, -40), (37, 9, 11), (64, 64, -63), (20, 3, 25), (300, 256, 17)]


@pytest.mark.parametrize("T,L,s", IDENTITY_CASES)
def test_adjoint_identity_of_the_table(T, L, s):
    """Both sides accumulated in float64 from the table's float32 results, in the waveform's domain (c = 0: x - c and c + g acc
    are then exact, and what is compared is the FIR, the gain and the draw sum).  A term h g x gy goes through its product, at
    most L tap sums, the product with the gain and, in the adjoint, at most K draw sums, one rounding of 2^-24 relative each:
    the bound is (L + K + 4) 2^-24 times the sum of the absolute values of the terms — computed here, in float64, not measured.
    A non-zero centre is covered by the silence check: a row of c comes out as c, byte for byte."""
    K, B = 3, 2
    rng = np.random.default_rng(1000 * T + L)
    x, c, c1 = rng.standard_normal((B, T)).astype(np.float32), np.zeros(B, np.float32), rng.standard_normal(B).astype(np.float32)
    h = rng.standard_normal((K, B, L)).astype(np.float32)
    shift = np.array([[s, -s], [s + 1, s - 1], [0, s]], np.int64)
    g = (rng.standard_normal((K, B)) + 2.0).astype(np.float32)
    gy = rng.standard_normal((K, B, T)).astype(np.float32)
    quiet = np.zeros((K, B), np.float32)
    silence = np.broadcast_to(c1[:, None], (B, T)).astype(np.float32)
    y, y0 = C.channel_apply_np(x, c, h, shift, g, quiet, seed=1), C.channel_apply_np(silence, c1, h, shift, g, quiet, seed=1)
    assert np.array_equal(y0, np.broadcast_to(c1[None, :, None], (K, B, T)))         # silence in, silence out
    G = C.channel_adjoint_np(gy, h, shift, g)
    xc = (x - c[:, None]).astype(np.float32).astype(np.float64)
    lhs = ((y.astype(np.float64) - c[None, :, None].astype(np.float64)) * gy).sum()
    rhs = (xc * G.astype(np.float64)).sum()
    terms = 0.0
    for j in range(K):
        for b in range(B):
            for i in range(L):
                t = np.arange(T)
                u = t - int(shift[j, b]) - i
                ok = (u >= 0) & (u < T)
                terms += np.abs(float(h[j, b, i]) * float(g[j, b]) * xc[b, u[ok]] * gy[j, b, t[ok]].astype(np.float64)).sum()
    bound = (L + K + 4) * 2.0 ** -24 * terms
    print(f"T={T} L={L} s={s}: |lhs - rhs| = {abs(lhs - rhs):.3e}, bound {bound:.3e}")
    assert abs(lhs - rhs) <= bound


def test_table_wholly_outside_and_draw_split():
    rng = np.random.default_rng(5)
    B, T, L, K = 2, 23, 4, 3
    x, c = rng.random((B, T), dtype=np.float32), np.array([0.25, 0.5], np.float32)
    h, g = rng.standard_normal((K, B, L)).astype(np.float32), np.ones((K, B), np.float32)
    a = np.full((K, B), 0.125, np.float32)
    shift = np.array([[T, -T - L], [2 ** 31 - 1, -2 ** 31], [1, -1]], np.int64)
    y = C.channel_apply_np(x, c, h, shift, g, a, seed=9, offset=4)
    for j in range(2):                                                                 # wholly outside: c + a n
        n = C.channel_noise(B, T, 9, 4 + j)
        assert np.array_equal(y[j], c[:, None] + a[j][:, None] * n)
        assert np.all(n >= -1.0) and np.all(n < 1.0)
    for j in range(K):                                                                 # K draws = K one-draw calls at offset + j
        one = C.channel_apply_np(x, c, h[j:j + 1], shift[j:j + 1], g[j:j + 1], a[j:j + 1], seed=9, offset=4 + j)
        assert np.array_equal(one[0], y[j])


# ---- the sampler -----------------------------------------------------------------------------------------------------------------------

def test_sampler_shapes_ranges_and_determinism():
    from audio_deepfake_adversarial_attacks_amd.torchattacks import CHANNELS, Channel
    ch = Channel(taps=24, decay=0.6, max_shift=7, gain_db=6.0, snr_db=(20, 40))
    x = torch.rand(5, 300, generator=torch.Generator().manual_seed(0))
    center = torch.full((5,), 0.5)
    torch.manual_seed(11)
    h, s, g, a = ch.draw(6, x, center)
    assert (h.shape, s.shape, g.shape, a.shape) == ((6, 5, 24), (6, 5), (6, 5), (6, 5))
    assert (h.dtype, s.dtype, g.dtype, a.dtype) == (torch.float32, torch.int32, torch.float32, torch.float32)
    assert all(t.is_contiguous() and t.device == x.device for t in (h, s, g, a))
    assert torch.allclose(h.double().square().sum(-1), torch.ones(6, 5, dtype=torch.float64), atol=1e-6)   # unit energy
    assert (h[..., 0] > 0).all()                                                       # the direct path
    assert s.min() >= -7 and s.max() <= 7
    lo, hi = 10 ** (-6 / 20), 10 ** (6 / 20)
    assert (g >= lo * (1 - 1e-6)).all() and (g <= hi * (1 + 1e-6)).all()
    rms = (x - 0.5).double().square().mean(1).sqrt()
    ratio = a.double() / (np.sqrt(3.0) * rms)                                          # 10^(-snr / 20), snr in [20, 40]
    assert (ratio >= 10 ** -2 * (1 - 1e-5)).all() and (ratio <= 10 ** -1 * (1 + 1e-5)).all()
    torch.manual_seed(11)
    again = ch.draw(6, x, center)
    assert all(torch.equal(p, q) for p, q in zip((h, s, g, a), again))
    other = ch.draw(6, x, center)
    assert not torch.equal(other[0], h)
    gen = lambda: torch.Generator().manual_seed(3)                                     # noqa: E731
    assert all(torch.equal(p, q) for p, q in zip(ch.draw(2, x, 0.5, generator=gen()), ch.draw(2, x, 0.5, generator=gen())))
    assert {"identity", "mild", "handset"} <= set(CHANNELS) and all(isinstance(v, Channel) for v in CHANNELS.values())


def test_identity_channel_and_refusals():
    from audio_deepfake_adversarial_attacks_amd.torchattacks import Channel
    from audio_deepfake_adversarial_attacks_amd.torchattacks.channel import resolve
    h, s, g, a = Channel.identity().draw(3, torch.rand(2, 10), torch.zeros(2))
    assert torch.equal(h, torch.ones(3, 2, 1)) and torch.equal(s, torch.zeros(3, 2, dtype=torch.int32))
    assert torch.equal(g, torch.ones(3, 2)) and torch.equal(a, torch.zeros(3, 2))
    for kw in ({"taps": 0}, {"taps": 257}, {"decay": 1.0}, {"decay": -0.1}, {"max_shift": -1}, {"gain_db": -1.0},
               {"gain_db": float("nan")}, {"snr_db": (40, 20)}, {"snr_db": float("nan")}):
        with pytest.raises(ValueError):
            Channel(**kw)
    assert resolve(None) is None and resolve("mild").taps == 32
    with pytest.raises(ValueError, match="unknown channel"):
        resolve("studio")
    with pytest.raises(TypeError):
        resolve(3)


# ---- surface ------------------------------------------------------------------------------------------------------------------------------

def test_class_is_exported_and_prints_as_the_reference(golden):
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    g = golden("eotpgd")
    assert {"EOTPGD", "Channel", "CHANNELS"} <= set(torchattacks.__all__)
    assert torchattacks.EOTPGD.__module__.endswith("attacks.eotpgd")
    assert str(torchattacks.EOTPGD(surrogate_from(g))) == str(g["str_EOTPGD"])
    atk = torchattacks.EOTPGD(stub(), channel="mild")
    assert str(atk) == str(torchattacks.EOTPGD(stub()))                               # the channel is not a printed hyper-parameter
    assert atk.channel is torchattacks.CHANNELS["mild"] and atk.wants_minmax and atk.replays_from_graph is False
    assert torchattacks.EOTPGD(stub()).channel is None and not torchattacks.EOTPGD(stub()).wants_minmax
    assert atk._supported_mode == ["default", "targeted"]
    for kw in ({"steps": 0}, {"eot_iter": 0}, {"eot_iter": 65, "channel": "mild"}, {"channel": "studio"}):
        with pytest.raises(ValueError):
            torchattacks.EOTPGD(stub(), **kw)
    with pytest.raises(TypeError):
        torchattacks.EOTPGD(stub(), channel=1.5)
    torchattacks.EOTPGD(stub(), eot_iter=65)                                          # without a channel there is no bound


def test_registry_members_construct():
    import evaluate_models_on_adversarial_attacks as cli
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    from audio_deepfake_adversarial_attacks_amd.aa.aa_types import AttackEnum
    want = {"EOTPGD": (0.0005, 10), "EOTPGD_eps00075": (0.00075, 10), "EOTPGD_eps001": (0.001, 10), "EOTPGD40_eps003": (0.003, 40)}
    for name, (eps, steps) in want.items():
        method, params = AttackEnum[name].value
        assert method is torchattacks.EOTPGD
        assert params == {"eps": eps, "alpha": 2.5 * eps / steps, "steps": steps, "eot_iter": 4, "channel": "mild"}
        atk = method(stub(), **params)
        assert atk.channel is torchattacks.CHANNELS["mild"]
    args = cli.parse_arguments(["--attack", "EOTPGD", "--channel", "handset", "--channel_draws", "3", "--synthetic", "8"])
    assert (args.attack, args.channel, args.channel_draws) == ("EOTPGD", "handset", 3)
    args = cli.parse_arguments(["--synthetic", "8"])
    assert args.channel is None and args.channel_draws == 1


# ---- the C ABI without a device -----------------------------------------------------------------------------------------------------------

def test_argument_validation_needs_no_device(lib):
    from audio_deepfake_adversarial_attacks_amd import _lib
    buf = (ctypes.c_float * 4096)()
    p = ctypes.addressof(buf)
    x, center, taps, shift, gain, noise, out, grads = (p + 1024 * k for k in (0, 1, 2, 3, 4, 5, 6, 8))

    def apply(B=2, T=8, K=2, L=3, **kw):
        a = dict(x=x, center=center, taps=taps, shift=shift, gain=gain, noise=noise, out=out)
        a.update(kw)
        return lib.advstep_channel_apply_f32(a["x"], a["center"], a["taps"], a["shift"], a["gain"], a["noise"], a["out"], B, T, K, L,
                                             1, 0, None)

    def adjoint(B=2, T=8, K=2, L=3, **kw):
        a = dict(grads=grads, taps=taps, shift=shift, gain=gain, out=out)
        a.update(kw)
        return lib.advstep_channel_adjoint_f32(a["grads"], a["taps"], a["shift"], a["gain"], a["out"], B, T, K, L, None)

    def step(B=2, T=8, K=2, L=3, **kw):
        a = dict(adv=x, orig=center, grads=grads, taps=taps, shift=shift, gain=gain, out=out)
        a.update(kw)
        return lib.advstep_channel_eot_step_f32(a["adv"], a["orig"], a["grads"], a["taps"], a["shift"], a["gain"], a["out"], B, T, K,
                                                L, 0.1, 0.1, 0.0, 1.0, None)

    for fn in (apply, adjoint, step):
        for kw in ({"B": -1}, {"T": -1}, {"K": -1}, {"B": 65536}, {"L": 0}, {"L": -1}, {"L": 257}, {"K": 65}, {"taps": None},
                   {"shift": None}, {"gain": None}, {"out": None}, {"out": taps}, {"out": shift}, {"out": gain}):
            assert fn(**kw) == _lib.EINVAL, (fn.__name__, kw)
        for kw in ({"B": 0}, {"T": 0}, {"K": 0}, {"B": 0, "out": None}, {"K": 0, "taps": None}):
            assert fn(**kw) == _lib.OK, (fn.__name__, kw)
    for kw in ({"x": None}, {"center": None}, {"noise": None}, {"out": x}, {"out": center}, {"out": noise}):
        assert apply(**kw) == _lib.EINVAL, kw
    for kw in ({"grads": None}, {"out": grads}, {"out": grads + 4}):
        assert adjoint(**kw) == _lib.EINVAL and step(**kw) == _lib.EINVAL, kw
    for kw in ({"adv": None}, {"orig": None}, {"out": center}, {"out": x + 4}):
        assert step(**kw) == _lib.EINVAL, kw
    assert apply(B=0, K=65) == _lib.EINVAL and apply(T=0, L=0) == _lib.EINVAL      # a bad size is refused before the empty return


def test_wrappers_refuse_cpu_tensors():
    from audio_deepfake_adversarial_attacks_amd import _lib, hip_ops
    x = torch.zeros(2, 8)
    h, s, g, a = torch.ones(1, 2, 1), torch.zeros(1, 2, dtype=torch.int32), torch.ones(1, 2), torch.zeros(1, 2)
    with pytest.raises(_lib.AdvstepError, match="no CPU fallback"):
        hip_ops.channel_apply(x, torch.zeros(2), h, s, g, a, seed=1)
    with pytest.raises(_lib.AdvstepError, match="no CPU fallback"):
        hip_ops.channel_adjoint(torch.zeros(1, 2, 8), h, s, g)
    with pytest.raises(_lib.AdvstepError, match="no CPU fallback"):
        hip_ops.channel_eot_step(x, x.clone(), torch.zeros(1, 2, 8), h, s, g, 0.1, 0.1)
    assert (hip_ops.CHANNEL_MAX_TAPS, hip_ops.CHANNEL_MAX_DRAWS) == (C.MAX_TAPS, C.MAX_DRAWS) == (256, 64)


# ---- the attack on the table ------------------------------------------------------------------------------------------------------------------

@pytest.fixture
def one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)  # the fixture was generated single-threaded
    yield
    torch.set_num_threads(n)


@pytest.mark.parametrize("mode", ("default", "targeted"))
@pytest.mark.parametrize("eot_iter", (1, 3))
def test_without_a_channel_bit_identical_to_the_reference(golden, one_thread, mode, eot_iter):
    """tests/golden/eotpgd.npz: the reference's unmodified EOTPGD with its own start draw recorded."""
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    g = golden_for_this_cpu(golden, "eotpgd")
    atk = torchattacks.EOTPGD(surrogate_from(g), eps=float(g["eps"]), alpha=float(g["alpha"]), steps=int(g["steps"]), eot_iter=eot_iter)
    atk.ops = C
    atk.set_init_noise(T_(g[f"{mode}_{eot_iter}_noise"]))
    if mode == "targeted":
        atk.set_mode_targeted_by_function(lambda images, labels: 1 - labels)
    x = T_(g["x"])
    adv = atk(x, T_(g["y"]))
    assert torch.equal(adv, T_(g[f"{mode}_{eot_iter}_adv"]))
    assert torch.equal(x, T_(g["x"])) and (adv != x).any()


def identity_case(B=4, T=50, seed=0):
    """x in [0.3, 0.7] and eps = 0.01: every sample the attack visits lies in [0.25, 1], where x - 0.5 is exact (Sterbenz) and
    (x - 0.5) + 0.5 gives x back, so the identity channel around the default centre 0.5 hands the detector PGD's own bytes."""
    gen = torch.Generator().manual_seed(seed)
    model = C.LinearDetector(torch.randn(T, generator=gen), torch.zeros(1))
    x = torch.rand(B, T, generator=gen) * 0.4 + 0.3
    y = torch.randint(0, 2, (B,), generator=gen)
    noise = (torch.rand(B, T, generator=gen) * 2 - 1) * 0.01
    return model, x, y, noise


@pytest.mark.parametrize("eot_iter", (1, 3))
def test_identity_channel_equals_pgd_on_the_table(eot_iter):
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    model, x, y, noise = identity_case()
    kw = dict(eps=0.01, alpha=0.003, steps=4)

    def run(atk):
        atk.ops = C
        atk.set_init_noise(noise)
        return atk(x, y)

    want = run(torchattacks.PGD(model, **kw))
    got = run(torchattacks.EOTPGD(model, eot_iter=eot_iter, channel=torchattacks.Channel.identity(), **kw))
    assert torch.equal(got, want) and (want != x).any()
    assert torch.equal(run(torchattacks.EOTPGD(model, eot_iter=eot_iter, **kw)), want)


def test_channel_attack_on_the_table_stays_in_the_ball_and_uses_the_handed_centre():
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    model, x, y, _ = identity_case(B=3, T=40, seed=2)
    ch = torchattacks.Channel(taps=5, decay=0.5, max_shift=3, gain_db=3.0, snr_db=30)
    atk = torchattacks.EOTPGD(model, eps=0.01, alpha=0.004, steps=3, eot_iter=2, channel=ch)
    calls = []

    class Spy:
        def __getattr__(self, name):
            return getattr(C, name)

        @staticmethod
        def channel_apply(x_, center, *a, **kw):
            calls.append(center.clone())
            return C.channel_apply(x_, center, *a, **kw)

    atk.ops = Spy()
    mn, mx = torch.tensor([[-1.0], [-0.5], [-0.25]]), torch.tensor([[1.0], [1.5], [0.75]])
    atk.set_minmax(mn, mx)
    torch.manual_seed(4)
    adv = atk(x, y)
    assert (adv - x).abs().max() <= 0.01 + 1e-7 and adv.min() >= 0 and adv.max() <= 1
    assert len(calls) == 3 and all(torch.equal(c, torch.tensor([0.5, 0.25, 0.25])) for c in calls)
    torch.manual_seed(4)
    atk.set_minmax(mn, mx)
    assert torch.equal(atk(x, y), adv)
    torch.manual_seed(4)
    atk.ops = Spy()
    calls.clear()
    atk(x, y)                                                                          # the min-max was consumed: centre 0.5
    assert all(torch.equal(c, torch.full((3,), 0.5)) for c in calls)
