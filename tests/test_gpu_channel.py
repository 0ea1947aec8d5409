"""GPU: the simulated audio channel — channel_apply, channel_adjoint and channel_eot_step against the BYTES of their numpy float32
restatement (tests/channel_cpu_ops.py: all three kernels are exact-order float32 computations, so there is no tolerance anywhere
in this file) on every shape at which a path changes: rows shorter than a quad, than a thread's run of 16, than the 4096-sample
tile, more than one tile (4100, 8200), T % 4 != 0; one tap, fewer taps than a chunk of 16, whole chunks (64, 256), more taps than
samples; delays that put the halo across a tile edge and windows wholly outside the row."""

import numpy as np
import pytest
import torch

from tests import channel_cpu_ops as C
from tests.test_gpu_apgd import same
from tests.test_gpu_momentum import padded, untouched

pytestmark = pytest.mark.gpu

LENGTHS = (1, 3, 4, 5, 255, 256, 257, 1021, 4100, 8200)
SHAPES = [(B, T) for T in LENGTHS for B in (1, 3)]
TAPS = (1, 2, 5, 64, 256)
DRAWS = (1, 3)
FILL = 3.5
SEED = (0x01234567 << 32) | 0x89ABCDEF            # non-zero high words; the offset's low word carries into the high one at draw 1
OFFSET = (5 << 32) | 0xFFFFFFFF
EPS, ALPHA = 0.01, 0.003


def hip():
    from audio_deepfake_adversarial_attacks_amd import hip_ops
    return hip_ops


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def on_side_stream(cuda, fn):
    side = torch.cuda.Stream(cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):
        res = fn()
    side.synchronize()
    return res


def delays(T, L):
    """None, one and three samples either way, the filter's length, a tile's length and its neighbours (a halo across a tile
    edge at T > 4096, wholly outside below it), the row's length either way and beyond (wholly outside), and the ends of int32."""
    return [0, 1, -1, 3, -3, L, -L, 4095, 4096, 4097, -4095, -4096, -4097, T, -T, T + L, -(T + L), T - 1, 1 - T, 2 ** 31 - 1, -2 ** 31]


def params(K, B, T, L, seed, shift=None):
    """taps (K, B, L), shift (K, B) int32, gain (K, B), noise (K, B), center (B) on the CPU."""
    g = torch.Generator().manual_seed(seed)
    taps = torch.randn(K, B, L, generator=g)
    if shift is None:
        d = delays(T, L)
        shift = torch.tensor([d[(seed + 5 * j + 3 * b) % 7] for j in range(K) for b in range(B)], dtype=torch.int32).reshape(K, B)
    gain = torch.rand(K, B, generator=g) * 1.5 + 0.5
    noise = torch.rand(K, B, generator=g) * 0.02
    center = torch.tensor([0.5, 0.3, 0.4375])[:B].contiguous()
    return taps, shift, gain, noise, center


def apply_np(x, p, seed=SEED, offset=OFFSET):
    taps, shift, gain, noise, center = p
    return torch.from_numpy(C.channel_apply_np(x.numpy(), center.numpy(), taps.numpy(), shift.numpy().astype(np.int64), gain.numpy(),
                                               noise.numpy(), seed, offset))


def adjoint_np(gy, p):
    taps, shift, gain, _, _ = p
    return torch.from_numpy(C.channel_adjoint_np(gy.numpy(), taps.numpy(), shift.numpy().astype(np.int64), gain.numpy()))


def dev(p, cuda):
    return tuple(t.to(cuda) for t in p)


def launch_apply(ops, x_d, pd, seed=SEED, offset=OFFSET, out=None):
    taps, shift, gain, noise, center = pd
    return ops.channel_apply(x_d, center, taps, shift, gain, noise, seed, offset, out=out)


# ---- a. the channel ---------------------------------------------------------------------------------------------------------------------

def check_apply(cuda, B, T, L, K, seed, shift=None):
    ops = hip()
    x = torch.rand(B, T, generator=torch.Generator().manual_seed(seed))
    p = params(K, B, T, L, seed, shift)
    want = apply_np(x, p)
    x_d, pd = x.to(cuda), dev(p, cuda)
    buf, out = padded((K, B, T), FILL, cuda)
    assert launch_apply(ops, x_d, pd, out=out) is out
    torch.cuda.synchronize()
    assert untouched(buf, FILL, K * B * T)
    assert torch.equal(bits(out), bits(want)), (B, T, L, K)
    fresh = launch_apply(ops, x_d, pd)
    assert fresh.shape == (K, B, T) and torch.equal(bits(fresh), bits(want))
    other = on_side_stream(cuda, lambda: launch_apply(ops, x_d, pd))
    assert torch.equal(bits(other), bits(want))
    assert same(x_d, x)
    return x, p, want


@pytest.mark.parametrize("B,T", SHAPES)
def test_apply_kernel_bytes(cuda, B, T):
    """Every draw equals the table's bytes; the guard round `out` is untouched; a rerun and a run on a side stream give the same
    bits; a K-draw call equals K one-draw calls with offset + j."""
    ops = hip()
    for L in TAPS:
        for K in DRAWS:
            x, p, want = check_apply(cuda, B, T, L, K, seed=100 * L + 10 * K + B + T)
            if K > 1 and L in (5, 64):
                x_d = x.to(cuda)
                for j in range(K):
                    one = launch_apply(ops, x_d, dev(tuple(t[j:j + 1] for t in p[:4]) + (p[4],), cuda), offset=OFFSET + j)
                    assert torch.equal(bits(one[0]), bits(want[j]))


@pytest.mark.parametrize("T,L", [(257, 5), (4100, 5), (4100, 64), (8200, 64), (8200, 256), (5, 7)])
def test_apply_every_delay(cuda, T, L):
    """One draw per delay of `delays` (K = 21), B = 2: row 1 takes the list backwards."""
    d = delays(T, L)
    shift = torch.tensor([d, d[::-1]], dtype=torch.int32).t().contiguous()
    x, p, want = check_apply(cuda, 2, T, L, len(d), seed=T + L, shift=shift)
    c, a = p[4], p[3]
    for j, s in enumerate(d):                                                      # wholly outside the row: c + a n
        if s >= T or s <= -(T + L - 1):
            n = torch.from_numpy(C.channel_noise(2, T, SEED, OFFSET + j))
            assert torch.equal(want[j, 0], c[0] + a[j, 0] * n[0]), s


def test_apply_production_row(cuda):
    check_apply(cuda, 1, 64_600, 64, 2, seed=7)


def test_apply_seed_offset_noise_and_unaligned_rows(cuda):
    """Another seed and another offset change only the noise: with noise = 0 the bytes do not depend on them, and with noise they
    differ from the base and equal the table's.  T % 4 == 0 from bases one float off a 16-byte boundary gives the same bytes."""
    ops = hip()
    B, T, L, K = 3, 4100, 5, 3
    x = torch.rand(B, T, generator=torch.Generator().manual_seed(1))
    p = params(K, B, T, L, 1)
    quiet = p[:3] + (torch.zeros(K, B),) + p[4:]
    x_d = x.to(cuda)
    base, base_quiet = launch_apply(ops, x_d, dev(p, cuda)), launch_apply(ops, x_d, dev(quiet, cuda))
    assert torch.equal(bits(base_quiet), bits(apply_np(x, quiet)))
    for seed, offset in ((SEED + 1, OFFSET), (SEED ^ (1 << 50), OFFSET), (SEED, OFFSET + 1), (SEED, OFFSET ^ (1 << 40))):
        other = launch_apply(ops, x_d, dev(p, cuda), seed, offset)
        assert not torch.equal(other, base) and torch.equal(bits(other), bits(apply_np(x, p, seed, offset)))
        assert torch.equal(bits(launch_apply(ops, x_d, dev(quiet, cuda), seed, offset)), bits(base_quiet))
    shifted = torch.empty(B * T + 1, device=cuda)[1:].view(B, T)
    assert shifted.data_ptr() % 16 == 4
    shifted.copy_(x)
    out = torch.empty(K * B * T + 1, device=cuda)[1:].view(K, B, T)
    launch_apply(ops, shifted, dev(p, cuda), out=out)
    assert torch.equal(bits(out), bits(base))
    assert torch.equal(bits(launch_apply(ops, shifted, dev(p, cuda))), bits(base))


def test_nan_and_inf_taps_stay_in_their_own_samples(cuda):
    """A NaN tap of draw 1, row 0 and an infinite tap of draw 2, row 1: every other (draw, row) has the bytes of the clean call, and
    the two hit rows equal the table's (NaN where the table has NaN)."""
    ops = hip()
    B, T, L, K = 2, 300, 5, 3
    x = torch.rand(B, T, generator=torch.Generator().manual_seed(2))
    p = params(K, B, T, L, 2, shift=torch.tensor([[0, 1], [2, -2], [-1, 3]], dtype=torch.int32))
    bad = p[0].clone()
    bad[1, 0, 2], bad[2, 1, 4] = float("nan"), float("inf")
    pb = (bad,) + p[1:]
    clean, got = launch_apply(ops, x.to(cuda), dev(p, cuda)), launch_apply(ops, x.to(cuda), dev(pb, cuda))
    want = apply_np(x, pb)
    assert same(got, want) and torch.isnan(want[1, 0]).all() and not torch.isfinite(want[2, 1]).all()
    for j in range(K):
        for b in range(B):
            if (j, b) not in ((1, 0), (2, 1)):
                assert torch.equal(bits(got[j, b]), bits(clean[j, b])) and bool(torch.isfinite(got[j, b]).all())
    gy = torch.randn(K, B, T, generator=torch.Generator().manual_seed(3))
    G, G_clean = ops.channel_adjoint(gy.to(cuda), *dev(pb[:3], cuda)), ops.channel_adjoint(gy.to(cuda), *dev(p[:3], cuda))
    assert same(G, adjoint_np(gy, pb)) and bool(torch.isfinite(G_clean).all())


# ---- b. the adjoint and the fused step ------------------------------------------------------------------------------------------------------

def step_inputs(B, T, seed):
    g = torch.Generator().manual_seed(seed)
    orig = torch.rand(B, T, generator=g)
    orig.view(-1)[::7] = 0.0
    orig.view(-1)[3::11] = 1.0
    adv = (orig + (torch.rand(B, T, generator=g) * 2 - 1) * EPS).clamp(0, 1)
    return adv, orig


def check_adjoint_and_step(cuda, B, T, L, K, seed, shift=None):
    ops = hip()
    p = params(K, B, T, L, seed, shift)
    gy = torch.randn(K, B, T, generator=torch.Generator().manual_seed(seed + 1))
    gy.view(-1)[::13] = 0.0
    adv, orig = step_inputs(B, T, seed + 2)
    want_G = adjoint_np(gy, p)
    want = torch.from_numpy(C.pgd_linf_step_np(adv.numpy(), want_G.numpy(), orig.numpy(), ALPHA, EPS))
    gy_d, adv_d, orig_d = gy.to(cuda), adv.to(cuda), orig.to(cuda)
    taps, shift_d, gain = dev(p[:3], cuda)

    buf, out = padded((B, T), FILL, cuda)
    assert ops.channel_adjoint(gy_d, taps, shift_d, gain, out=out) is out
    torch.cuda.synchronize()
    assert untouched(buf, FILL, B * T) and torch.equal(bits(out), bits(want_G)), (B, T, L, K)
    assert torch.equal(bits(on_side_stream(cuda, lambda: ops.channel_adjoint(gy_d, taps, shift_d, gain))), bits(want_G))

    sbuf, sout = padded((B, T), FILL, cuda)
    assert ops.channel_eot_step(adv_d, orig_d, gy_d, taps, shift_d, gain, ALPHA, EPS, out=sout) is sout
    torch.cuda.synchronize()
    assert untouched(sbuf, FILL, B * T) and torch.equal(bits(sout), bits(want)), (B, T, L, K)
    two = ops.pgd_linf_step(adv_d, out, orig_d, ALPHA, EPS)                         # the unfused pair on the device
    assert torch.equal(bits(two), bits(sout))
    abuf, alias = padded((B, T), FILL, cuda)
    alias.copy_(adv)
    assert ops.channel_eot_step(alias, orig_d, gy_d, taps, shift_d, gain, ALPHA, EPS, out=alias) is alias
    torch.cuda.synchronize()
    assert untouched(abuf, FILL, B * T) and torch.equal(bits(alias), bits(want))
    other = on_side_stream(cuda, lambda: ops.channel_eot_step(adv_d, orig_d, gy_d, taps, shift_d, gain, ALPHA, EPS))
    assert torch.equal(bits(other), bits(want))
    assert same(gy_d, gy) and same(adv_d, adv) and same(orig_d, orig)
    return want


@pytest.mark.parametrize("B,T", SHAPES)
def test_adjoint_and_step_kernel_bytes(cuda, B, T):
    """channel_adjoint equals the table; channel_eot_step equals the table AND hip_ops.pgd_linf_step on channel_adjoint's output,
    byte for byte, also with out = adv; guards untouched; a run on a side stream gives the same bits."""
    moved = False
    for L in TAPS:
        for K in DRAWS:
            want = check_adjoint_and_step(cuda, B, T, L, K, seed=100 * L + 10 * K + B + T)
            moved = moved or bool((want != step_inputs(B, T, 100 * L + 10 * K + B + T + 2)[0]).any())
    assert moved


@pytest.mark.parametrize("T,L", [(257, 5), (4100, 64), (8200, 256), (5, 7)])
def test_adjoint_every_delay(cuda, T, L):
    d = delays(T, L)
    shift = torch.tensor([d, d[::-1]], dtype=torch.int32).t().contiguous()
    check_adjoint_and_step(cuda, 2, T, L, len(d), seed=T + L, shift=shift)


def test_adjoint_production_row_and_unaligned_rows(cuda):
    ops = hip()
    check_adjoint_and_step(cuda, 1, 64_600, 64, 2, seed=9)
    B, T, L, K = 3, 4100, 5, 3
    p = params(K, B, T, L, 4)
    gy = torch.randn(K, B, T, generator=torch.Generator().manual_seed(5))
    adv, orig = step_inputs(B, T, 6)
    taps, shift, gain = dev(p[:3], cuda)
    base = ops.channel_eot_step(adv.to(cuda), orig.to(cuda), gy.to(cuda), taps, shift, gain, ALPHA, EPS, lo=0.25, hi=0.75)
    want = C.pgd_linf_step_np(adv.numpy(), adjoint_np(gy, p).numpy(), orig.numpy(), ALPHA, EPS, 0.25, 0.75)
    assert torch.equal(bits(base), bits(torch.from_numpy(want)))
    off = lambda t: torch.empty(t.numel() + 1, device=cuda)[1:].view(t.shape).copy_(t)          # noqa: E731
    a1, o1, g1 = off(adv), off(orig), off(gy)
    assert a1.data_ptr() % 16 == 4 and g1.data_ptr() % 16 == 4
    assert torch.equal(bits(ops.channel_eot_step(a1, o1, g1, taps, shift, gain, ALPHA, EPS, lo=0.25, hi=0.75)), bits(base))
    assert torch.equal(bits(ops.channel_adjoint(g1, taps, shift, gain)), bits(ops.channel_adjoint(gy.to(cuda), taps, shift, gain)))


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------

def test_wrappers_refuse_bad_arguments(cuda):
    ops = hip()
    B, T, K, L = 3, 8, 2, 4
    x = torch.zeros(B, T, device=cuda)
    taps, shift, gain, noise, center = dev(params(K, B, T, L, 0), cuda)
    gy = torch.zeros(K, B, T, device=cuda)
    with pytest.raises(TypeError, match="float32"):
        ops.channel_apply(x.double(), center, taps, shift, gain, noise, 1)
    with pytest.raises(TypeError, match="int32"):
        ops.channel_apply(x, center, taps, shift.long(), gain, noise, 1)
    with pytest.raises(ValueError, match="contiguous"):
        ops.channel_apply(x.t().contiguous().t(), center, taps, shift, gain, noise, 1)
    with pytest.raises(ValueError, match="taps must be"):
        ops.channel_apply(x, center, taps[:, :2].contiguous(), shift, gain, noise, 1)
    with pytest.raises(ValueError, match="between 1 and 256 taps"):
        ops.channel_apply(x, center, torch.zeros(K, B, 257, device=cuda), shift, gain, noise, 1)
    with pytest.raises(ValueError, match="at most 64 draws"):
        ops.channel_adjoint(torch.zeros(65, B, T, device=cuda), torch.zeros(65, B, L, device=cuda),
                            torch.zeros(65, B, dtype=torch.int32, device=cuda), torch.zeros(65, B, device=cuda))
    with pytest.raises(ValueError, match="gain must be"):
        ops.channel_apply(x, center, taps, shift, gain[:1], noise, 1)
    with pytest.raises(ValueError, match="noise must be"):
        ops.channel_apply(x, center, taps, shift, gain, noise[:, :2].contiguous(), 1)
    with pytest.raises(ValueError, match="one value per row"):
        ops.channel_apply(x, center[:2], taps, shift, gain, noise, 1)
    with pytest.raises(ValueError, match="out must hold"):
        ops.channel_apply(x, center, taps, shift, gain, noise, 1, out=torch.zeros(K, B, T + 1, device=cuda))
    with pytest.raises(ValueError, match="draws"):
        ops.channel_adjoint(gy[:1], taps, shift, gain)
    with pytest.raises(ValueError, match="grads must be"):
        ops.channel_eot_step(x, x.clone(), torch.zeros(K, B, T + 1, device=cuda), taps, shift, gain, 0.1, 0.1)
    with pytest.raises(ValueError, match="does not match"):
        ops.channel_eot_step(x, torch.zeros(B, T + 1, device=cuda), gy, taps, shift, gain, 0.1, 0.1)
    with pytest.raises(Exception, match="status 1"):                               # the ABI's own overlap rule
        ops.channel_eot_step(x, x.clone(), gy, taps, shift, gain, 0.1, 0.1, out=gy[0])
