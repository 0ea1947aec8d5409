"""Admits the references of tests/detector_ref.py (no GPU): each float64 reference equals float64 torch autograd through the
module's own expression (the lines of specrnet.py / rawnet3.py that include/advstep_detector.h quotes) to 1e-12 relative, and
each float32 restatement of a pooling operator gives the values and the winners of F.max_pool1d / F.max_pool2d(...,
return_indices=True) on the CPU, on inputs with ties, NaN, +-inf and -0.0."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import detector_ref as R

F32, F64 = torch.float32, torch.float64
REL = 1e-12


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rnd(shape, seed, dtype=F64):
    return torch.randn(shape, generator=gen(seed), dtype=dtype)


def close(got, want):
    scale = max(want.abs().max().item(), 1e-300)
    assert got.shape == want.shape
    assert (got - want).abs().max().item() <= REL * scale, ((got - want).abs().max().item(), scale)


def bits_equal(a, b):
    """Same bytes, NaN where the other has NaN."""
    na, nb = torch.isnan(a), torch.isnan(b)
    ia, ib = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return a.shape == b.shape and bool((na == nb).all() and (ia[~na] == ib[~nb]).all())


# ---- float64 references against autograd through the module expressions ----------------------------------------------------------------

@pytest.mark.parametrize("P", [1, 7, 133])
def test_selu_reference_is_autograd(P):
    x, s, t, gy = rnd((2, 3, P), 1) * 2, rnd(3, 2), rnd(3, 3), rnd((2, 3, P), 4)
    (y,), (gx, _, _) = R.autograd64(R.selu_expr, [x, s, t], [gy])
    close(R.affine_act_forward(x, s, t, None, 2, 0.0, F64), y)
    close(R.affine_act_backward(gy, x, s, t, None, 2, 0.0, F64), gx)


@pytest.mark.parametrize("mode", [0, 1])
def test_affine_and_link_references_are_autograd(mode):
    """The float64 evaluation of the restatements of modes 0 and 1 (and of the Res2Net link built on mode 1) is the module's chain:
    the grouping they restate is that chain's."""
    x, s, t, pre, gy = rnd((2, 3, 50), 5), rnd(3, 6), rnd(3, 7), rnd(3, 8), rnd((2, 3, 50), 9)
    if mode == 0:                                                    # specrnet.py:76-81: bn2 -> LeakyReLU(0.3)
        expr = lambda x, s, t: F.leaky_relu(x * R.ch(s, x) + R.ch(t, x), 0.3)
        (y,), (gx, _, _) = R.autograd64(expr, [x, s, t], [gy])
        pre = None
    else:                                                            # rawnet3.py:240-242: conv bias -> ReLU -> BatchNorm1d(eval)
        expr = lambda x, s, t, p: torch.relu(x + R.ch(p, x)) * R.ch(s, x) + R.ch(t, x)
        (y,), (gx, _, _, _) = R.autograd64(expr, [x, s, t, pre], [gy])
    close(R.affine_act_forward(x, s, t, pre, mode, 0.3, F64), y)
    close(R.affine_act_backward(gy, x, s, t, pre, mode, 0.3, F64), gx)
    if mode == 1:                                                    # rawnet3.py:244-258: sp = bn(relu(conv(sp))); next = sp + spx[i + 1]
        other, gz = rnd((2, 3, 50), 10), rnd((2, 3, 50), 11)
        link = lambda h, o: (expr(h, s, t, pre), expr(h, s, t, pre) + o)
        (y, z), (gh, _) = R.autograd64(link, [x, other], [gy, gz])
        y1, z1 = R.res2net_link_forward(x, s, t, pre, other, F64)
        close(y1, y), close(z1, z)
        close(R.res2net_link_backward(gy, gz, x, s, t, pre, F64), gh)


@pytest.mark.parametrize("L", [1, 5, 300])
def test_log_meannorm_reference_is_autograd(L):
    y, gx = rnd((3, L), 12), rnd((3, L), 13)
    y[0, 0] = 0.0
    eps = R.f32_scalar(1e-6)
    (x,), (gy,) = R.autograd64(lambda y: R.log_meannorm_expr(y, eps), [y], [gx])
    close(R.log_meannorm_forward(y, 1e-6, F64), x)
    close(R.log_meannorm_backward(gx, y, 1e-6, F64), gy)


@pytest.mark.parametrize("L", [1, 9, 257])
def test_afms_reference_is_autograd(L):
    """Modes 0 and 1 are the forward; modes 2 and 3 with the caller's sigmoid' and fc^T between them are its gradient."""
    N, C = 2, 3
    x, alpha, w, bias, g = rnd((N, C, L), 14), rnd(C, 15), rnd((C, C), 16), rnd(C, 17), rnd((N, C, L), 18)
    (out,), (gx, galpha, _, _) = R.autograd64(R.afms_expr, [x, alpha, w, bias], [g])
    rows = x.view(N * C, L)
    mean, _ = R.afms_row(0, rows, None, None, None, None, C, F64)
    y = torch.sigmoid(F.linear(mean.view(N, C), w, bias))
    close(R.afms_row(1, rows, None, alpha, y.view(-1), None, C, F64).view(N, C, L), out)
    gy, _ = R.afms_row(2, g.view(N * C, L), rows, alpha, None, None, C, F64)
    m = ((gy.view(N, C) * y * (1 - y)) @ w) / L
    close(R.afms_row(3, g.view(N * C, L), None, None, y.view(-1), m.view(-1), C, F64).view(N, C, L), gx)


@pytest.mark.parametrize("L", [1, 65, 429])
def test_weighted_stats_reference_is_autograd(L):
    x, w, gmu, gm2 = rnd((5, L), 19), rnd((5, L), 20), rnd(5, 21), rnd(5, 22)
    (mu, m2), (gx, gw) = R.autograd64(R.weighted_stats_expr, [x, w], [gmu, gm2])
    mu1, m21, _, _ = R.weighted_stats_forward(x, w, F64)
    close(mu1, mu), close(m21, m2)
    gx1, gw1 = R.weighted_stats_backward(x, w, gmu, gm2, F64)
    close(gx1, gx), close(gw1, gw)


@pytest.mark.parametrize("C", [1, 5, 64])
def test_gate_fc_reference_is_autograd(C):
    mean, w, bias, gg = rnd((3, C), 23), rnd((C, C), 24) / math.sqrt(C), rnd(C, 25), rnd((3, C), 26)
    (gate,), (gm, _, _) = R.autograd64(R.gate_fc_expr, [mean, w, bias], [gg])
    close(R.gate_fc_forward(mean, w, bias, F64)[0], gate)
    partial = torch.stack([gg * 0.25, gg * 0.75], dim=-1).view(3 * C, 2)      # two blocks that sum to gg
    close(R.gate_fc_backward(partial, gate, w, 1.0, F64)[0], gm)


@pytest.mark.parametrize("H,W", [(2, 2), (5, 12), (3, 6), (4, 1024), (7, 9)])
def test_attend_pool_references_are_autograd(H, W):
    """SpecRNet's attention end to end: gate_fc_forward, gate_maxpool2_forward, the gate's partial sums (and their pooled form),
    gate_fc_backward and the scatter with the mean's share reproduce autograd's d x."""
    N, C = 2, 3
    x, w, bias = rnd((N, C, H, W), 27), rnd((C, C), 28), rnd(C, 29)
    gy = rnd((N, C, H // 2, W // 2), 30)
    (out,), (gx, _, _) = R.autograd64(R.attend_pool_expr, [x, w, bias], [gy])
    gate = R.gate_fc_forward(x.mean(dim=(2, 3)), w, bias, F64)[0]
    y, sel, xw = R.gate_maxpool2_forward(x, gate, F64)
    close(y, out)
    part, _ = R.gate_partials(gy, sel, x)
    assert part.shape == (N * C, R.gate_blocks(H, W))
    close(R.gate_pooled(gy, xw, F64)[0], part.sum(dim=1))
    g_mean, _ = R.gate_fc_backward(part, gate, w, 1.0 / (H * W), F64)
    g_mean = g_mean * (1.0 / (H * W) / R.f32_scalar(1.0 / (H * W)))       # the reference takes inv_hw as the float32 the ABI carries
    close(R.unpool2(gy, sel, H, W, gate=gate, addc=g_mean, dtype=F64), gx)


# ---- the float32 restatements of the pooling operators against ATen's own on the CPU -------------------------------------------------------

def spiced(shape, seed):
    """float32 noise on a coarse grid (many ties) with NaN, +-inf, 0.0 and -0.0, and whole windows of equal values."""
    t = (torch.randn(shape, generator=gen(seed)) * 2).round() / 2
    f = t.view(-1)
    for k, v in enumerate((math.nan, math.inf, -math.inf, 0.0, -0.0, math.nan)):
        f[(7 * k + 3) % f.numel()::41] = v
    if f.numel() > 16:
        f[8:16] = -0.0
        f[9] = 0.0
    return t


def code2(idx, H, W):
    """F.max_pool2d's flat plane index -> the selection byte (bit 1 = dh, bit 0 = dw)."""
    Ho, Wo = idx.shape[2:]
    h, w = idx // W, idx % W
    i, j = torch.arange(Ho).view(1, 1, Ho, 1), torch.arange(Wo).view(1, 1, 1, Wo)
    return (2 * (h - 2 * i) + (w - 2 * j)).to(torch.uint8)


@pytest.mark.parametrize("H,W", [(2, 2), (3, 6), (5, 12), (7, 9), (2, 1028)])
def test_pool2_restatements_match_aten(H, W):
    a, b, bias = spiced((2, 3, H, W), 31), spiced((2, 3, H, W), 32), torch.tensor([0.5, -0.0, -1.0])
    for bb, bi in ((None, None), (b, None), (b, bias)):
        v = a if bb is None else a + bb
        v = v + (R.ch(bi, v) if bi is not None else 0.0)
        want, idx = F.max_pool2d(v, 2, return_indices=True)
        y, sel = R.add_maxpool2_forward(a, bb, bi)
        assert bits_equal(y, want) and torch.equal(sel, code2(idx, H, W))
    gate = torch.tensor([[0.25, 0.9, 0.0], [1.0, 0.5, 0.731]])
    want, idx = F.max_pool2d(a * gate.view(2, 3, 1, 1) + gate.view(2, 3, 1, 1), 2, return_indices=True)
    y, sel, xw = R.gate_maxpool2_forward(a, gate)
    assert bits_equal(y, want) and torch.equal(sel, code2(idx, H, W))
    assert bits_equal(xw, a.flatten(2).gather(2, idx.flatten(2)).view_as(idx))
    # the scatter: ATen's max_pool2d backward through the same winners (finite gradients; ATen accumulates into zeros)
    gy = torch.randn(want.shape, generator=gen(33))
    v = (a + b).nan_to_num(0.0, 50.0, -50.0).requires_grad_(True)
    F.max_pool2d(v, 2).backward(gy)
    _, sel = R.add_maxpool2_forward(v.detach(), None, None)
    assert torch.equal(R.unpool2(gy, sel, H, W), v.grad)


@pytest.mark.parametrize("k", [2, 3, 5, 8])
@pytest.mark.parametrize("L", [1, 8, 40, 83])
def test_pool1d_restatements_match_aten(k, L):
    a, b = spiced((2, 3, L), 34), spiced((2, 3, L), 35)
    s, t, pre = torch.tensor([0.5, -1.25, 2.0]), torch.tensor([0.25, -0.5, 0.0]), torch.tensor([0.5, 0.0, -1.0])
    if L < k:
        assert R.add_maxpool1d_forward(a, b, k)[0].shape == (2, 3, 0)
        return
    for bb in (None, b):
        want, idx = F.max_pool1d(a if bb is None else a + bb, k, return_indices=True)
        y, sel = R.add_maxpool1d_forward(a, bb, k)
        assert bits_equal(y, want) and torch.equal(sel.long(), idx - k * torch.arange(L // k))
    act = torch.relu(a + R.ch(pre, a)) * R.ch(s, a) + R.ch(t, a)
    want, idx = F.max_pool1d(act + b, k, return_indices=True)
    y, sel = R.tail_pool1d_forward(a, b, s, t, pre, k)
    assert bits_equal(y, want) and torch.equal(sel.long(), idx - k * torch.arange(L // k))
    # backward: max_pool1d's and the threshold's, through autograd on finite inputs
    h = a.nan_to_num(0.0, 50.0, -50.0).requires_grad_(True)
    r = b.nan_to_num(0.0, 50.0, -50.0).requires_grad_(True)
    gy = torch.randn(2, 3, L // k, generator=gen(36))
    F.max_pool1d(torch.relu(h + R.ch(pre, h)) * R.ch(s, h) + R.ch(t, h) + r, k).backward(gy)
    _, sel = R.tail_pool1d_forward(h.detach(), r.detach(), s, t, pre, k)
    g_h, g_res = R.tail_pool1d_backward(gy, sel, h.detach(), s, pre, k)
    assert torch.equal(g_res, r.grad) and torch.equal(g_h, h.grad)
    assert torch.equal(R.unpool1d(gy, sel, L, k), r.grad)
