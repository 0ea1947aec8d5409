"""`-m gpu`: the LCNN max-feature-map kernels (include/advstep_lcnn.h) against the ATen ops they replace, on the GPU,
bit for bit — values, input gradients, ties, NaN, odd sizes — and the fused LCNN against the plain one."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L(cuda):
    from audio_deepfake_adversarial_attacks_amd import lcnn_ops
    return lcnn_ops


def ref_mfm(x, bias=None):
    if bias is not None:
        x = x + bias.view(1, -1, 1, 1)
    n, c2, h, w = x.shape
    return x.view(n, 2, c2 // 2, h, w).max(1)[0]


def ref_mfm_pool(x, bias=None):
    return torch.nn.functional.max_pool2d(ref_mfm(x, bias), (2, 2), (2, 2))


def make(shape, cuda, seed, ties=False, nans=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    if ties:
        x = (x * 2).round() / 2          # many exact ties, between channel halves and inside pooling windows
    if nans:
        flat = x.view(-1)
        flat[torch.randint(0, flat.numel(), (max(flat.numel() // 50, 1),), generator=g)] = float("nan")
    return x.to(cuda)


def same(a, b):
    return torch.equal(torch.nan_to_num(a, nan=1234.5), torch.nan_to_num(b, nan=1234.5)) and \
        torch.equal(torch.isnan(a), torch.isnan(b))


# ---- float64 references of the convolution blocks, driven by a GIVEN selection --------------------------------------------------
# Selection bytes (include/advstep_lcnn.h): the pooled blocks (conv5, conv3x3 + pool) write one per pooled cell, bit 2 = channel
# half, bit 1 = dh, bit 0 = dw of the winner; the un-pooled 3x3 block one per 2x2 tile, bit 2 * row + col set where the second
# half won.  The input-gradient entry points take the bytes as input, so a reference built from the same bytes has no near-tie
# ambiguity: it must agree everywhere.  Bounds: 1e-5 (values) and 2e-5 (input gradients) of the output scale, for every
# reduction length the 3x3 kernels accept (up to Cin = 256 forward, K = 2C = 256 backward).  Measured on gfx950: at most
# 7.1e-7 of the scale for either, K = 256 included (parity_record wino_* / conv5_*), so fp32 Winograd needs no K-dependent bound.

POOL_SCAN = (0, 4, 1, 5, 2, 6, 3, 7)      # selection codes in the kernels' scan order a00 b00 a01 b01 a10 b10 a11 b11


def _abi():
    from audio_deepfake_adversarial_attacks_amd import _lib
    return _lib.load(), torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


def pool_candidates(conv):
    """(N, 2C, H, W) -> (N, C, H/2, W/2, 8): the 8 candidates of every pooled cell, indexed by selection code."""
    N, C2, H, W = conv.shape
    C, Ho, Wo = C2 // 2, H // 2, W // 2
    v = conv[:, :, :2 * Ho, :2 * Wo].reshape(N, 2, C, Ho, 2, Wo, 2)
    return v.permute(0, 2, 3, 5, 1, 4, 6).reshape(N, C, Ho, Wo, 8)


def tile_bits(sel, N, C, H, W):
    """(N, C, H, W) bool from one byte per 2x2 tile: True where the second half won (bits of positions outside the plane
    are ignored)."""
    TH, TW = (H + 1) // 2, (W + 1) // 2
    b = sel.reshape(N, C, TH, TW).long().repeat_interleave(2, 2).repeat_interleave(2, 3)[:, :, :H, :W]
    shift = 2 * (torch.arange(H, device=sel.device) % 2).view(-1, 1) + (torch.arange(W, device=sel.device) % 2).view(1, -1)
    return ((b >> shift) & 1).bool()


def dense_grad_pooled(gy, sel, H, W, gscale=None):
    """d(conv out) (N, 2C, H, W) in float64: gy (N, C, H/2, W/2) [* gscale] at the half / position each code names."""
    N, C, Ho, Wo = gy.shape
    g = gy.double() * (1.0 if gscale is None else gscale.double().view(1, -1, 1, 1))
    onehot = (sel.reshape(N, C, Ho, Wo, 1).long() == torch.arange(8, device=gy.device)).double()
    d = (g.unsqueeze(-1) * onehot).reshape(N, C, Ho, Wo, 2, 2, 2).permute(0, 4, 1, 2, 5, 3, 6)
    return torch.nn.functional.pad(d.reshape(N, 2 * C, 2 * Ho, 2 * Wo), (0, W - 2 * Wo, 0, H - 2 * Ho))


def dense_grad_unpooled(gy, sel, gscale=None):
    """d(conv out) (N, 2C, H, W) in float64: gy (N, C, H, W) [* gscale] to the half each tile bit names, 0 to the other."""
    N, C, H, W = gy.shape
    g = gy.double() * (1.0 if gscale is None else gscale.double().view(1, -1, 1, 1))
    tb = tile_bits(sel, N, C, H, W)
    return torch.cat([torch.where(tb, 0.0, g), torch.where(tb, g, 0.0)], 1)


def block_forward(kind, x, weight, bias=None, bn=None, y=None, sel=None):
    """One call of a block's forward C ABI (kind: conv5, pool2 = conv3x3 + pool, mfm = conv3x3 without pool) -> (y, sel).
    y / sel may be given (views carved out of sentinel buffers)."""
    from audio_deepfake_adversarial_attacks_amd import lcnn_ops
    lib, st = _abi()
    N, Cin, H, W = x.shape
    C = weight.shape[0] // 2
    shape = (N, C, H, W) if kind == "mfm" else (N, C, H // 2, W // 2)
    nsel = lib.advstep_conv3x3_mfm_sel_bytes(N, C, H, W) if kind == "mfm" else N * C * (H // 2) * (W // 2)
    y = torch.empty(shape, device=x.device) if y is None else y
    sel = torch.empty(max(nsel, 1), dtype=torch.uint8, device=x.device) if sel is None else sel
    if kind == "conv5":
        st = lib.advstep_conv5_mfm_pool2_forward_f32(_ptr(x), _ptr(weight), _ptr(bias), _ptr(y), _ptr(sel), N, C, H, W, st)
    else:
        fn = lib.advstep_conv3x3_mfm_forward_f32 if kind == "mfm" else lib.advstep_conv3x3_mfm_pool2_forward_f32
        st = fn(_ptr(x), _ptr(lcnn_ops._prepared_weights(weight, 0)), _ptr(bias), _ptr(None if bn is None else bn[0]),
                _ptr(None if bn is None else bn[1]), _ptr(y), _ptr(sel), N, Cin, C, H, W, st)
    assert st == 0
    return y, sel[:nsel]


def block_backward(kind, gy, sel, weight, gscale, Cin, H, W, gx=None, gout=None):
    """The input-gradient C ABI of a block from a given selection -> (gx, gout).  conv5 / pool2: one call from the compact
    (pooled gradient, bytes) form; mfm: the max-feature-map routing into gout (N, 2C, H, W), then the dense 3x3 input gradient."""
    from audio_deepfake_adversarial_attacks_amd import lcnn_ops
    lib, st = _abi()
    N, C = gy.shape[:2]
    gx = torch.empty(N, Cin, H, W, device=gy.device) if gx is None else gx
    if kind == "conv5":
        assert lib.advstep_conv5_mfm_pool2_backward_f32(_ptr(gy), _ptr(sel), _ptr(weight), _ptr(gx), N, C, H, W, st) == 0
    elif kind == "pool2":
        U = lcnn_ops._prepared_weights(weight, 2, gscale)
        assert lib.advstep_conv3x3_mfm_pool2_backward_f32(_ptr(gy), _ptr(sel), _ptr(U), _ptr(gx), N, Cin, C, H, W, st) == 0
    else:
        gout = torch.empty(N, 2 * C, H, W, device=gy.device) if gout is None else gout
        assert lib.advstep_conv3x3_mfm_backward_f32(_ptr(gy), _ptr(sel), _ptr(gscale), _ptr(gout), N, C, H, W, st) == 0
        U = lcnn_ops._prepared_weights(weight, 1)
        assert lib.advstep_conv3x3_backward_data_f32(_ptr(gout), _ptr(U), _ptr(gx), N, Cin, 2 * C, H, W, st) == 0
    return gx, gout


def ref_input_grad(kind, dense, weight, x_shape):
    return torch.nn.grad.conv2d_input(tuple(x_shape), weight.double(), dense, padding=2 if kind == "conv5" else 1)


def check_winners(kind, y, sel, conv, bn, tol):
    """The kernel's selection against the float64 pre-pool convolution (bias included): the candidate each byte names is
    within 2 tol of the maximum of its candidates; it IS the first maximum in the kernels' scan order wherever the top two are
    more than 2 tol apart; such clear decisions are >= 90 % of all; y is the named candidate [after the BatchNorm] within tol."""
    N, C2, H, W = conv.shape
    C = C2 // 2
    if y.numel() == 0:
        return {"clear_fraction": 1.0, "y_err_over_tol": 0.0}
    if kind == "mfm":
        a, b = conv[:, :C], conv[:, C:]
        took_b = tile_bits(sel, N, C, H, W)
        named, best = torch.where(took_b, b, a), torch.maximum(a, b)
        clear = (a - b).abs() > 2 * tol
        assert torch.equal(took_b[clear], (b > a)[clear])
    else:
        assert int(sel.max()) <= 7
        cand = pool_candidates(conv)
        code = sel.reshape(cand.shape[:-1]).long()
        named = cand.gather(-1, code.unsqueeze(-1)).squeeze(-1)
        scan = cand[..., list(POOL_SCAN)]
        top2 = scan.topk(2, dim=-1).values
        best = top2[..., 0]
        clear = top2[..., 0] - top2[..., 1] > 2 * tol
        first = torch.tensor(POOL_SCAN, device=conv.device)[scan.argmax(-1)]
        assert torch.equal(code[clear], first[clear])
    assert (best - named).max().item() <= 2 * tol
    frac = clear.double().mean().item()
    assert frac >= 0.9, frac
    ytol = tol
    if bn is not None:
        named = (named - bn[0].double().view(1, -1, 1, 1)) * bn[1].double().view(1, -1, 1, 1)
        ytol = tol * max(bn[1].max().item(), 1.0)
    yerr = (y.double() - named).abs().max().item()
    assert yerr <= ytol, (yerr, ytol)
    return {"clear_fraction": frac, "y_err_over_tol": yerr / ytol}


def check_through_own_selection(L, kind, x, weight, bias, bn, gy, gx=None):
    """Forward C ABI twice (equal bits), its selection checked against float64 (check_winners), then the autograd wrapper twice:
    the same y as the ABI, equal input gradients (`gx`, when given, is a third run), and that gradient against the float64
    reference built from the ABI's selection bytes - every entry within the gradient bound, no near-tie exceptions."""
    y, sel = block_forward(kind, x, weight, bias, bn)
    y2, sel2 = block_forward(kind, x, weight, bias, bn)
    assert torch.equal(y, y2) and torch.equal(sel, sel2)
    H, W = x.shape[2:]
    pad = 2 if kind == "conv5" else 1
    conv = torch.nn.functional.conv2d(x.double(), weight.double(), None if bias is None else bias.double(), padding=pad)
    fig = check_winners(kind, y, sel, conv, bn, 1e-5 * max(conv.abs().max().item(), 1.0))
    fn = {"conv5": L.conv5_mfm_pool2, "pool2": L.conv3x3_mfm_pool2, "mfm": L.conv3x3_mfm}[kind]
    grads = []
    for _ in range(2):
        xa = x.clone().requires_grad_(True)
        ya = fn(xa, weight, bias) if kind == "conv5" else fn(xa, weight, bias, bn)
        assert torch.equal(ya, y)
        grads.append(torch.autograd.grad(ya, xa, gy)[0])
    assert torch.equal(grads[0], grads[1]) and (gx is None or torch.equal(gx, grads[0]))
    gscale = None if bn is None else bn[1]
    dense = dense_grad_unpooled(gy, sel, gscale) if kind == "mfm" else dense_grad_pooled(gy, sel, H, W, gscale)
    ref = ref_input_grad(kind, dense, weight, x.shape)
    gerr = (grads[0].double() - ref).abs().max().item() / max(ref.abs().max().item(), 1.0)
    assert gerr <= 2e-5, gerr
    fig["grad_err_over_scale"] = gerr
    return fig


SHAPES = [(2, 4, 6, 8), (3, 2, 1, 4), (2, 6, 5, 7), (1, 2, 3, 3), (2, 8, 101, 20), (2, 64, 404, 80), (3, 10, 7, 12),
          (1, 2, 2, 2), (2, 4, 9, 16)]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("mode", ["plain", "ties", "nans"])
@pytest.mark.parametrize("with_bias", [False, True])
def test_mfm_matches_aten(L, cuda, shape, mode, with_bias):
    x = make(shape, cuda, 1, ties=mode == "ties", nans=mode == "nans").requires_grad_(True)
    bias = (torch.randn(shape[1], generator=torch.Generator().manual_seed(2)).to(cuda) if with_bias else None)
    if with_bias and mode == "ties":
        bias = (bias * 2).round() / 2
    y_ref = ref_mfm(x, bias)
    gy = make(tuple(y_ref.shape), cuda, 3)
    (gx_ref,) = torch.autograd.grad(y_ref, x, gy)
    y = L.mfm(x, bias)
    (gx,) = torch.autograd.grad(y, x, gy)
    assert same(y, y_ref)
    assert same(gx, gx_ref)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("mode", ["plain", "ties", "nans"])
@pytest.mark.parametrize("with_bias", [False, True])
def test_mfm_pool2_matches_aten(L, cuda, shape, mode, with_bias):
    if shape[2] < 2 or shape[3] < 2:
        pytest.skip("ATen rejects an empty pooled output")
    x = make(shape, cuda, 4, ties=mode == "ties", nans=mode == "nans").requires_grad_(True)
    bias = (torch.randn(shape[1], generator=torch.Generator().manual_seed(5)).to(cuda) if with_bias else None)
    if with_bias and mode == "ties":
        bias = (bias * 2).round() / 2
    y_ref = ref_mfm_pool(x, bias)
    gy = make(tuple(y_ref.shape), cuda, 6)
    (gx_ref,) = torch.autograd.grad(y_ref, x, gy)
    y = L.mfm_pool2(x, bias)
    (gx,) = torch.autograd.grad(y, x, gy)
    assert y.shape == y_ref.shape and same(y, y_ref)
    assert same(gx, gx_ref)


def test_bias_gradient_when_requested(L, cuda):
    x = make((2, 6, 8, 8), cuda, 7).requires_grad_(True)
    bias = torch.randn(6, device=cuda, requires_grad=True)
    for fn, ref in ((L.mfm, ref_mfm), (L.mfm_pool2, ref_mfm_pool)):
        gy = torch.randn_like(ref(x, bias))
        gx_ref, gb_ref = torch.autograd.grad(ref(x, bias), (x, bias), gy)
        gx, gb = torch.autograd.grad(fn(x, bias), (x, bias), gy)
        assert torch.equal(gx, gx_ref) and torch.allclose(gb, gb_ref, rtol=1e-5, atol=1e-6)


def test_input_validation(L, cuda):
    from audio_deepfake_adversarial_attacks_amd._lib import AdvstepError
    with pytest.raises(AdvstepError, match="no CPU fallback"):
        L.mfm(torch.rand(1, 2, 4, 4))
    with pytest.raises(ValueError):
        L.mfm(torch.rand(1, 3, 4, 4, device=cuda))
    with pytest.raises(ValueError):
        L.mfm(torch.rand(1, 4, 4, 4, device=cuda), torch.rand(3, device=cuda))
    assert L.mfm(torch.rand(0, 4, 4, 4, device=cuda)).shape == (0, 2, 4, 4)


def test_fused_lcnn_is_bit_identical_to_plain_lcnn(cuda, monkeypatch):
    """Same weights, same input: logits and input-gradient of the attack-mode model with and without the kernels.
    Compared at the spectrogram (the LFCC backward uses atomic index_add, so waveform gradients are not run-to-run
    reproducible even for the plain model; they are compared against that noise floor instead)."""
    from audio_deepfake_adversarial_attacks_amd.models.models import get_model
    torch.manual_seed(0)
    model = get_model("lcnn", {"frontend_algorithm": ["lfcc"], "input_channels": 1}, str(cuda)).to(cuda)
    model.train()
    for m in model.modules():
        if "BatchNorm" in m.__class__.__name__ or "Dropout" in m.__class__.__name__:
            m.eval()
    x = (torch.randn(4, 64_600, generator=torch.Generator().manual_seed(1)) * 0.05).to(cuda)
    spec = model._compute_frontend(x).detach()

    # the convolution-fusing kernels round differently from MIOpen; this test isolates the max-feature-map kernels
    monkeypatch.setenv("ADVSTEP_LCNN_CONV0", "0")
    monkeypatch.setenv("ADVSTEP_LCNN_CONV1X1", "0")
    monkeypatch.setenv("ADVSTEP_LCNN_CONV3X3", "0")
    monkeypatch.setenv("ADVSTEP_LCNN_LSTM", "0")
    monkeypatch.setenv("ADVSTEP_LCNN_BN", "0")
    monkeypatch.setenv("ADVSTEP_FUSED_LFCC", "0")

    def run(fused, frozen, waveform=False):
        monkeypatch.setenv("ADVSTEP_LCNN_FUSED", "1" if fused else "0")
        for p in model.parameters():
            p.requires_grad_(not frozen)
        a = (x if waveform else spec).clone().requires_grad_(True)
        z = model(a) if waveform else model._compute_embedding(a)
        (g,) = torch.autograd.grad(z.sum(), a)
        return z.detach(), g

    z0, g0 = run(False, False)
    for fused, frozen in ((True, False), (True, True)):     # without and with the bias add folded in
        z, g = run(fused, frozen)
        assert torch.equal(z, z0), (fused, frozen)
        assert torch.equal(g, g0), (fused, frozen)
    zw0, gw0 = run(False, False, waveform=True)
    zw1, gw1 = run(False, False, waveform=True)
    zw2, gw2 = run(True, True, waveform=True)
    assert torch.equal(zw0, zw2)
    noise = (gw0 - gw1).abs().max().item()
    assert (gw0 - gw2).abs().max().item() <= max(4 * noise, 1e-6 * gw0.abs().max().item())
    for p in model.parameters():
        p.requires_grad_(True)


# ---- fused first block: Conv2d(1, 2C, 5x5, pad 2) -> MFM -> MaxPool2d(2, 2) ------------------------------------------------

def ref_block0(x, weight, bias):
    return ref_mfm_pool(torch.nn.functional.conv2d(x, weight, bias, stride=1, padding=2))


@pytest.mark.parametrize("shape", [(2, 1, 12, 16), (3, 1, 9, 7), (1, 1, 2, 2), (2, 1, 101, 20), (4, 1, 404, 80), (2, 1, 5, 33),
                                   (3, 1, 14, 70), (2, 1, 9, 64), (5, 1, 11, 79), (1, 1, 2, 80), (37, 1, 6, 66)])
@pytest.mark.parametrize("C,with_bias", [(32, True), (3, False), (8, True), (32, False)])
def test_conv5_mfm_pool2_matches_float64_reference(L, cuda, parity_record, request, shape, C, with_bias):
    g = torch.Generator().manual_seed(shape[2] * 131 + shape[3] + C)
    x = torch.randn(shape, generator=g).to(cuda)
    weight = (torch.randn(2 * C, 1, 5, 5, generator=g) * 0.3).to(cuda)
    bias = torch.randn(2 * C, generator=g).to(cuda) if with_bias else None
    xr = x.double().requires_grad_(True)
    y_ref = ref_block0(xr, weight.double(), bias.double() if with_bias else None)
    gy = torch.randn(y_ref.shape, generator=g).to(cuda)
    (gx_ref,) = torch.autograd.grad(y_ref, xr, gy.double())
    xa = x.clone().requires_grad_(True)
    y = L.conv5_mfm_pool2(xa, weight, bias)
    (gx,) = torch.autograd.grad(y, xa, gy)
    assert y.shape == y_ref.shape
    # the same winners must be selected unless two candidates are within float rounding of each other (not at these seeds)
    assert (y.double() - y_ref).abs().max().item() <= 2e-5
    assert (gx.double() - gx_ref).abs().max().item() <= 2e-4 * max(gx_ref.abs().max().item(), 1.0)
    # and against the float32 ATen composition it replaces
    xf = x.clone().requires_grad_(True)
    yf = ref_block0(xf, weight, bias)
    (gxf,) = torch.autograd.grad(yf, xf, gy)
    assert (y - yf).abs().max().item() <= 2e-5
    close = (gx - gxf).abs() <= 2e-4 * max(gxf.abs().max().item(), 1.0)
    assert close.float().mean().item() >= 0.999       # MIOpen's own rounding may flip a near-tie winner
    # winners checked against float64 instead of assumed, and the gradient through the kernel's own selection: every entry
    fig = check_through_own_selection(L, "conv5", x, weight, bias, None, gy, gx)
    parity_record[f"conv5_block_{request.node.callspec.id}"] = fig


@pytest.mark.parametrize("shape,C", [((4, 1, 404, 80), 32), ((3, 1, 9, 16), 8), ((2, 1, 101, 20), 3), ((5, 1, 38, 128), 32),
                                     ((2, 1, 7, 2), 32), ((1, 1, 64, 66), 96)])
def test_conv5_backward_cell_centric_equals_the_gather(L, cuda, monkeypatch, shape, C):
    """Round 5: the first block's input gradient with a thread per pooled CELL (window table in LDS, one exchange per tile) against
    the patch-centric gather of rounds 1-4 on the same (gradient, selection bytes, weights): the same sums in another order - equal
    to float rounding, both finite, the tile seams (rows 17 / 34 / ... of the pooled plane at width 40), the trailing odd row and
    the narrow / wide / many-channel shapes included.  ADVSTEP_CONV0_BWD=gather selects the old kernel."""
    g = torch.Generator().manual_seed(shape[2] * 7 + shape[3] + C)
    x = torch.randn(shape, generator=g).to(cuda)
    weight = (torch.randn(2 * C, 1, 5, 5, generator=g) * 0.3).to(cuda)
    bias = torch.randn(2 * C, generator=g).to(cuda)
    outs = {}
    for mode in ("cells", "gather"):
        monkeypatch.setenv("ADVSTEP_CONV0_BWD", mode)
        xa = x.clone().requires_grad_(True)
        y = L.conv5_mfm_pool2(xa, weight, bias)
        gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(5)).to(cuda)
        (outs[mode],) = torch.autograd.grad(y, xa, gy)
    scale = outs["gather"].abs().max().item()
    assert torch.isfinite(outs["cells"]).all()
    assert (outs["cells"] - outs["gather"]).abs().max().item() <= 4e-6 * max(scale, 1.0)
    # a pooled gradient that is zero except ONE cell next to a tile seam: its 5x5 footprint must come out whole
    if shape[2] >= 40:
        gy1 = torch.zeros_like(gy)
        gy1[0, 0, 17, min(3, gy.shape[3] - 1)] = 1.0
        res = {}
        for mode in ("cells", "gather"):
            monkeypatch.setenv("ADVSTEP_CONV0_BWD", mode)
            xa = x.clone().requires_grad_(True)
            (res[mode],) = torch.autograd.grad(L.conv5_mfm_pool2(xa, weight, bias), xa, gy1)
        assert torch.equal(res["cells"], res["gather"]) and int((res["cells"] != 0).sum()) == 25


@pytest.mark.parametrize("kind", ["conv5", "conv3x3"])
def test_fused_conv_pool_selection_with_nans_ties_and_infinities(L, cuda, kind):
    """The pooling epilogues of the convolution kernels take a short path when no candidate in a wave is NaN and the
    exact ATen rule otherwise: NaNs must propagate exactly as max-feature-map + MaxPool2d do, ties (integer-valued data:
    the convolution is exact) and infinities must select like ATen, and the selection bytes must route the gradient the
    same way."""
    g = torch.Generator().manual_seed(11)
    if kind == "conv5":
        N, Cin, C, H, W, k = 3, 1, 32, 12, 70, 5
    else:
        N, Cin, C, H, W, k = 2, 32, 48, 10, 12, 3
    # small integers: every product and partial sum is exact in float32, so equal candidates are exactly equal
    x = torch.randint(-2, 3, (N, Cin, H, W), generator=g).float()
    weight = torch.randint(-1, 2, (2 * C, Cin, k, k), generator=g).float()
    bias = torch.randint(-1, 2, (2 * C,), generator=g).float()
    if kind == "conv5":       # (a Winograd convolution — MIOpen's and this library's 3x3 — smears non-finite inputs over
        x[0, 0, 3, 5] = float("nan")              # neighbouring tiles through inf - inf in its transforms: no common reference)
        x[1, 0, 7, 30] = float("inf")
        x[1, 0, 2, 3] = float("-inf")
    x, weight, bias = x.to(cuda), weight.to(cuda), bias.to(cuda)
    # reference convolution on the CPU in float64: a direct convolution, so a NaN / inf reaches exactly its receptive
    # field (MIOpen's Winograd / FFT algorithms smear them over neighbouring outputs)
    y_ref = ref_mfm_pool(torch.nn.functional.conv2d(x.cpu().double(), weight.cpu().double(), bias.cpu().double(),
                                                    padding=k // 2)).float().to(cuda)
    xa = x.clone().requires_grad_(True)
    y = L.conv5_mfm_pool2(xa, weight, bias) if kind == "conv5" else L.conv3x3_mfm_pool2(xa, weight, bias)
    assert torch.equal(torch.isnan(y), torch.isnan(y_ref)) and (kind != "conv5" or torch.isnan(y).any())
    finite = torch.isfinite(y_ref)
    assert torch.equal(torch.nan_to_num(y, nan=0.0, posinf=1e30, neginf=-1e30),
                       torch.nan_to_num(y_ref, nan=0.0, posinf=1e30, neginf=-1e30))
    # gradient routing on the samples without NaN / inf (a NaN anywhere poisons ATen's whole convolution backward)
    clean = torch.randint(-2, 3, (N, Cin, H, W), generator=g).float().to(cuda)
    ca, cr = clean.clone().requires_grad_(True), clean.clone().requires_grad_(True)
    yc = L.conv5_mfm_pool2(ca, weight, bias) if kind == "conv5" else L.conv3x3_mfm_pool2(ca, weight, bias)
    yr = ref_mfm_pool(torch.nn.functional.conv2d(cr, weight, bias, padding=k // 2))
    assert torch.equal(yc, yr)
    gy = torch.randint(-2, 3, yr.shape, generator=g).float().to(cuda)
    (ga,) = torch.autograd.grad(yc, ca, gy)
    (gr,) = torch.autograd.grad(yr, cr, gy)
    assert torch.equal(ga, gr) and finite.any()


def test_conv5_mfm_pool2_requires_frozen_weights(L, cuda):
    x = torch.randn(1, 1, 8, 8, device=cuda, requires_grad=True)
    w = torch.randn(4, 1, 5, 5, device=cuda, requires_grad=True)
    y = L.conv5_mfm_pool2(x, w, None)
    with pytest.raises(RuntimeError, match="input gradient only"):
        y.sum().backward()
    with pytest.raises(ValueError):
        L.conv5_mfm_pool2(torch.randn(1, 2, 8, 8, device=cuda), w.detach(), None)


def test_lcnn_with_fused_first_block_agrees_with_miopen_path(cuda, monkeypatch, parity_record):
    """Whole LCNN, attack mode, frozen parameters: fused first block + fused 1x1 blocks vs MIOpen convolutions.  The two
    convolutions round differently, so logits agree to float tolerance and input gradients to a small relative error.
    Measured (profiles/r02_parity.json): logits 3e-8, gradient relative L2 7e-7, no entry off by 1e-3 of the maximum."""
    from audio_deepfake_adversarial_attacks_amd.models.models import get_model
    torch.manual_seed(0)
    model = get_model("lcnn", {"frontend_algorithm": ["lfcc"], "input_channels": 1}, str(cuda)).to(cuda)
    model.train()
    for m in model.modules():
        if "BatchNorm" in m.__class__.__name__ or "Dropout" in m.__class__.__name__:
            m.eval()
    for p in model.parameters():
        p.requires_grad_(False)
    x = (torch.randn(4, 64_600, generator=torch.Generator().manual_seed(1)) * 0.05).to(cuda)
    spec = model._compute_frontend(x).detach()

    def run(conv0):
        monkeypatch.setenv("ADVSTEP_LCNN_CONV0", "1" if conv0 else "0")
        monkeypatch.setenv("ADVSTEP_LCNN_CONV1X1", "1" if conv0 else "0")
        monkeypatch.setenv("ADVSTEP_LCNN_CONV3X3", "1" if conv0 else "0")
        monkeypatch.setenv("ADVSTEP_LCNN_LSTM", "1" if conv0 else "0")
        a = spec.clone().requires_grad_(True)
        z = model._compute_embedding(a)
        (g,) = torch.autograd.grad(z.sum(), a)
        return z.detach(), g

    z0, g0 = run(False)
    z1, g1 = run(True)
    assert (z0 - z1).abs().max().item() <= 3.5e-7
    # different (equally valid) float rounding inside the convolution flips a handful of near-tie winners among the
    # 33 M max-feature-map / pool decisions; each flip re-routes one gradient entry.  Sparse, bounded differences:
    off = (g0 - g1).abs() > 1e-3 * g0.abs().max()
    fig = {"logit_max_abs": (z0 - z1).abs().max().item(), "grad_rel_l2": (g0 - g1).norm().item() / g0.norm().item(),
           "grad_entries": g0.numel(), "grad_entries_off_by_1e-3_of_max": int(off.sum()),
           "grad_max_abs_over_max": ((g0 - g1).abs().max() / g0.abs().max()).item()}
    parity_record["lcnn_fused_kernels_vs_miopen_path"] = fig
    # a near-tie max-feature-map / pool winner going the other way would re-route one gradient entry (~1e-3 of the relative
    # L2 each); none does on this input.  Bounds = 10x the measured figures (logits 3.4e-8, relative L2 6.9e-7, worst entry
    # 6.7e-7 of the largest): a kernel that loses three digits fails
    assert fig["grad_entries_off_by_1e-3_of_max"] == 0, fig
    assert fig["grad_rel_l2"] <= 7e-6 and fig["grad_max_abs_over_max"] <= 7e-6, fig
    for p in model.parameters():
        p.requires_grad_(True)


# ---- fused 1x1 blocks: Conv2d(Cin, 2C, 1x1) -> MFM -----------------------------------------------------------------------------

@pytest.mark.parametrize("N,Cin,C,H,W", [(2, 32, 32, 12, 10), (3, 48, 48, 7, 9), (2, 64, 64, 50, 10), (1, 32, 5, 1, 1),
                                         (2, 32, 32, 202, 40), (2, 48, 7, 3, 67)])
@pytest.mark.parametrize("with_bias", [True, False])
def test_conv1x1_mfm_matches_float64_reference(L, cuda, N, Cin, C, H, W, with_bias):
    g = torch.Generator().manual_seed(N * 1000 + Cin * 10 + C + H)
    x = torch.randn(N, Cin, H, W, generator=g).to(cuda)
    weight = (torch.randn(2 * C, Cin, 1, 1, generator=g) * 0.2).to(cuda)
    bias = torch.randn(2 * C, generator=g).to(cuda) if with_bias else None
    xr = x.double().requires_grad_(True)
    y_ref = ref_mfm(torch.nn.functional.conv2d(xr, weight.double(), bias.double() if with_bias else None))
    gy = torch.randn(y_ref.shape, generator=g).to(cuda)
    (gx_ref,) = torch.autograd.grad(y_ref, xr, gy.double())
    xa = x.clone().requires_grad_(True)
    y = L.conv1x1_mfm(xa, weight, bias)
    (gx,) = torch.autograd.grad(y, xa, gy)
    assert y.shape == y_ref.shape
    assert (y.double() - y_ref).abs().max().item() <= 2e-5
    assert (gx.double() - gx_ref).abs().max().item() <= 2e-5 * max(gx_ref.abs().max().item(), 1.0)


@pytest.mark.parametrize("Cin,C", [(48, 48), (32, 5), (48, 7), (64, 64), (64, 33)])
def test_conv1x1_mfm_writes_nothing_outside_its_tensors(cuda, Cin, C):
    """The kernels address channel rows through scalar offsets of a buffer descriptor, which the hardware does not
    range-check: accumulator rows beyond C (forward) / Cin (backward) — present whenever these are not multiples of 32 —
    must not be stored.  Outputs are carved out of sentinel-filled buffers and the sentinels checked afterwards."""
    from audio_deepfake_adversarial_attacks_amd import _lib
    lib = _lib.load()
    N, P = 3, 77
    g = torch.Generator().manual_seed(Cin + C)
    x = torch.randn(N, Cin, P, generator=g).to(cuda)
    w = (torch.randn(2 * C, Cin, generator=g) * 0.2).to(cuda)
    nsel = lib.advstep_conv1x1_mfm_sel_bytes(N, C, P) // 4       # opaque layout: its size comes from the library
    assert nsel == N * ((P + 31) // 32) * 64 * (2 if C <= 32 else 4) // 4
    pad = 64 * P
    ybuf = torch.full((pad + N * C * P + pad,), 7.5, device=cuda)
    sbuf = torch.full((pad + nsel + pad,), 0x5A5A5A5A, dtype=torch.int32, device=cuda)
    y, sel = ybuf[pad:pad + N * C * P], sbuf[pad:pad + nsel]
    stream = torch.cuda.current_stream(cuda).cuda_stream
    assert lib.advstep_conv1x1_mfm_forward_f32(x.data_ptr(), w.data_ptr(), None, None, None, y.data_ptr(), sel.data_ptr(),
                                               N, Cin, C, P, stream) == 0
    torch.cuda.synchronize()
    assert (ybuf[:pad] == 7.5).all() and (ybuf[pad + N * C * P:] == 7.5).all()
    assert (sbuf[:pad] == 0x5A5A5A5A).all() and (sbuf[pad + nsel:] == 0x5A5A5A5A).all()
    conv = torch.einsum("ok,nkp->nop", w.double(), x.double())
    want = torch.maximum(conv[:, :C], conv[:, C:])
    assert (y.view(N, C, P).double() - want).abs().max().item() <= 2e-5
    gy = torch.randn(N, C, P, generator=g).to(cuda)
    xpad = 64 * P
    gbuf = torch.full((xpad + N * Cin * P + xpad,), -3.25, device=cuda)
    gx = gbuf[xpad:xpad + N * Cin * P]
    assert lib.advstep_conv1x1_mfm_backward_f32(gy.data_ptr(), sel.data_ptr(), w.data_ptr(), None, gx.data_ptr(), N, Cin,
                                                C, P, stream) == 0
    torch.cuda.synchronize()
    assert (gbuf[:xpad] == -3.25).all() and (gbuf[xpad + N * Cin * P:] == -3.25).all()
    took_b = conv[:, C:] > conv[:, :C]
    gfull = torch.cat([torch.where(took_b, 0.0, gy.double()), torch.where(took_b, gy.double(), 0.0)], dim=1)
    want_gx = torch.einsum("ok,nop->nkp", w.double(), gfull)
    assert (gx.view(N, Cin, P).double() - want_gx).abs().max().item() <= 2e-5 * max(want_gx.abs().max().item(), 1.0)


def test_conv1x1_mfm_rejects_unsupported_and_unfrozen(L, cuda):
    w = torch.randn(8, 16, 1, 1, device=cuda)
    with pytest.raises(ValueError, match="Cin"):
        L.conv1x1_mfm(torch.randn(1, 16, 4, 4, device=cuda), w, None)
    x = torch.randn(1, 32, 4, 4, device=cuda, requires_grad=True)
    w = torch.randn(8, 32, 1, 1, device=cuda, requires_grad=True)
    with pytest.raises(RuntimeError, match="input gradient only"):
        L.conv1x1_mfm(x, w, None).sum().backward()


# ---- LSTM layer --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T,B,I", [(25, 6, 160), (1, 2, 160), (7, 128, 160), (3, 1, 32)])
def test_lstm_layer_matches_torch_lstm(L, cuda, T, B, I):
    torch.manual_seed(T * 100 + B)
    H = 80
    ref = torch.nn.LSTM(I, H, bidirectional=True).double()
    x = torch.randn(T, B, I, dtype=torch.float64, requires_grad=True)
    out_ref, _ = ref(x)
    dout = torch.randn_like(out_ref)
    (dx_ref,) = torch.autograd.grad(out_ref, x, dout)

    w_ih = torch.cat([ref.weight_ih_l0, ref.weight_ih_l0_reverse]).float().to(cuda).contiguous()
    w_hh = torch.stack([ref.weight_hh_l0, ref.weight_hh_l0_reverse]).float().to(cuda).contiguous()
    bias = torch.cat([ref.bias_ih_l0 + ref.bias_hh_l0, ref.bias_ih_l0_reverse + ref.bias_hh_l0_reverse]).float().to(cuda)
    xg = x.detach().float().to(cuda).requires_grad_(True)
    out = L.lstm_layer(xg, w_ih.detach(), w_hh.detach(), bias.detach())
    (dx,) = torch.autograd.grad(out, xg, dout.float().to(cuda))
    assert out.shape == (T, B, 2 * H)
    assert (out.double().cpu() - out_ref).abs().max().item() <= 2e-6
    assert (dx.double().cpu() - dx_ref).abs().max().item() <= 2e-5 * max(dx_ref.abs().max().item(), 1.0)


def test_blstm_layer_uses_kernel_when_frozen_and_matches_miopen(cuda, monkeypatch):
    from audio_deepfake_adversarial_attacks_amd.models.lcnn import BLSTMLayer
    torch.manual_seed(3)
    layer = BLSTMLayer(160, 160).to(cuda).train()
    x = torch.randn(16, 25, 160, device=cuda)

    def run(kernel, frozen):
        monkeypatch.setenv("ADVSTEP_LCNN_LSTM", "1" if kernel else "0")
        for p in layer.parameters():
            p.requires_grad_(not frozen)
        a = x.clone().requires_grad_(True)
        y = layer(a)
        (g,) = torch.autograd.grad(y, a, torch.ones_like(y))
        return y.detach(), g

    y0, g0 = run(False, False)          # MIOpen
    y1, g1 = run(True, True)            # HIP kernel
    y2, g2 = run(True, False)           # parameters need grad -> falls back to MIOpen, identical to y0
    assert torch.equal(y2, y0)
    assert (y1 - y0).abs().max().item() <= 2e-6 and (g1 - g0).abs().max().item() <= 2e-5 * max(g0.abs().max().item(), 1.0)
    for p in layer.parameters():
        p.requires_grad_(True)


# ---- eval-mode BatchNorm folded into the block kernels ---------------------------------------------------------------------------

def _bn_ref(y, mean, var, eps=1e-5):
    return torch.nn.functional.batch_norm(y, mean, var, None, None, False, 0.1, eps)


@pytest.mark.parametrize("kind", ["mfm", "mfm_pool2", "conv1x1"])
def test_folded_batchnorm_matches_aten(L, cuda, kind):
    g = torch.Generator().manual_seed(11)
    C = 32
    mean = torch.randn(C, generator=g).to(cuda)
    var = (torch.rand(C, generator=g) + 0.5).to(cuda)
    bn = (mean, (1.0 / torch.sqrt(var + 1e-5)).contiguous())
    if kind == "conv1x1":
        x = torch.randn(3, 32, 9, 10, generator=g).to(cuda).requires_grad_(True)
        w = (torch.randn(2 * C, 32, 1, 1, generator=g) * 0.2).to(cuda)
        b = torch.randn(2 * C, generator=g).to(cuda)
        ref = _bn_ref(ref_mfm(torch.nn.functional.conv2d(x, w, b)), mean, var)
        got = L.conv1x1_mfm(x, w, b, bn)
        tol = 2e-5
    else:
        x = make((3, 2 * C, 10, 12), cuda, 12).requires_grad_(True)
        b = torch.randn(2 * C, generator=g).to(cuda)
        ref = _bn_ref((ref_mfm_pool if kind == "mfm_pool2" else ref_mfm)(x, b), mean, var)
        got = (L.mfm_pool2 if kind == "mfm_pool2" else L.mfm)(x, b, bn)
        tol = 1e-6   # same operations; ATen may use rsqrt for invstd
    gy = torch.randn(ref.shape, generator=g).to(cuda)
    (g_ref,) = torch.autograd.grad(ref, x, gy)
    (g_got,) = torch.autograd.grad(got, x, gy)
    assert (got - ref).abs().max().item() <= tol * max(ref.abs().max().item(), 1.0)
    assert (g_got - g_ref).abs().max().item() <= max(tol, 2e-6) * max(g_ref.abs().max().item(), 1.0)


# ---- fused 3x3 blocks on the matrix cores: Conv2d(Cin, 2C, 3x3, pad 1) -> MFM -> MaxPool2d(2, 2) [-> BN] ---------------------

@pytest.mark.parametrize("N,Cin,C,H,W", [(2, 32, 48, 12, 10), (1, 48, 64, 11, 9), (2, 64, 32, 50, 10), (3, 32, 32, 6, 8),
                                         (2, 32, 48, 202, 40), (1, 48, 64, 101, 20), (5, 32, 16, 2, 2)])
@pytest.mark.parametrize("with_bias,with_bn", [(True, True), (False, False)])
def test_conv3x3_mfm_pool2_matches_float64_reference(L, cuda, N, Cin, C, H, W, with_bias, with_bn):
    """Winograd F(2x2, 3x3) in fp32 against a float64 direct convolution: values within 1e-5 of the output scale (the
    same error class as MIOpen's own fp32 Winograd kernel).  The input gradient is compared twice: against float64 autograd,
    whose max-pool picks its OWN winners - a last-bit difference may pick another winner at a near tie, an equally valid
    subgradient, so a few entries may differ (the fraction and count clauses) - and, with no exception, against the float64
    reference evaluated with the winners the kernel recorded (check_through_own_selection)."""
    g = torch.Generator().manual_seed(N * 1000 + Cin * 10 + C + H)
    x = torch.randn(N, Cin, H, W, generator=g).to(cuda)
    weight = (torch.randn(2 * C, Cin, 3, 3, generator=g) * 0.1).to(cuda)
    bias = torch.randn(2 * C, generator=g).to(cuda) if with_bias else None
    bn = None
    if with_bn:
        mean = torch.randn(C, generator=g).to(cuda)
        var = (torch.rand(C, generator=g) + 0.5).to(cuda)
        bn = (mean, (1.0 / torch.sqrt(var + 1e-5)).contiguous())
    xr = x.double().requires_grad_(True)
    conv = torch.nn.functional.conv2d(xr, weight.double(), bias.double() if with_bias else None, padding=1)
    y_ref = ref_mfm_pool(conv)
    if with_bn:
        y_ref = (y_ref - bn[0].double().view(1, -1, 1, 1)) * bn[1].double().view(1, -1, 1, 1)
    xa = x.clone().requires_grad_(True)
    y = L.conv3x3_mfm_pool2(xa, weight, bias, bn)
    assert y.shape == y_ref.shape == (N, C, H // 2, W // 2)
    scale = max(y_ref.abs().max().item(), 1.0)
    assert (y.double() - y_ref).abs().max().item() <= 1e-5 * scale
    if y.numel() == 0:
        return
    gy = torch.randn(y_ref.shape, generator=g).to(cuda)
    (gx,) = torch.autograd.grad(y, xa, gy)
    (gx_ref,) = torch.autograd.grad(y_ref, xr, gy.double())
    err = (gx.double() - gx_ref).abs()
    tol = 2e-5 * max(gx_ref.abs().max().item(), 1.0)
    # at most a handful of pooling windows may resolve a near tie differently
    assert (err > tol).float().mean().item() <= 1e-3, ((err > tol).sum().item(), err.max().item())
    assert (err.max().item() <= tol) or (err > tol).sum().item() <= 9 * 8 * Cin
    check_through_own_selection(L, "pool2", x, weight, bias, bn, gy, gx)


@pytest.mark.parametrize("N,C,H,W", [(4, 32, 50, 10), (3, 32, 11, 9), (2, 64, 50, 10), (3, 64, 7, 13), (1, 64, 2, 2)])
def test_conv3x3_pool2_backward_half_slice_launch_equals_the_single_launch(L, cuda, monkeypatch, N, C, H, W):
    """a one-slice input gradient (Cin = 32 output rows) on a plane that does not fill the chip is launched as
    its two 16-row halves (round 5, `ga.halves`; every NT = 1 kernel then reads its A operand as one component of the
    stored pair).  A/B through the switch the launcher reads at call time: the same bits, for the resident weights
    (K = 2 C = 64) and the streamed ones (K = 128), on even and odd planes."""
    g = torch.Generator().manual_seed(C * 100 + H * 10 + W)
    Cin = 32
    x = torch.randn(N, Cin, H, W, generator=g).to(cuda)
    weight = (torch.randn(2 * C, Cin, 3, 3, generator=g) * 0.1).to(cuda)
    bias = torch.randn(2 * C, generator=g).to(cuda)
    mean, var = torch.randn(C, generator=g).to(cuda), (torch.rand(C, generator=g) + 0.5).to(cuda)
    bn = (mean, (1.0 / torch.sqrt(var + 1e-5)).contiguous())
    gy = torch.randn(N, C, H // 2, W // 2, generator=g).to(cuda)
    got = {}
    for halves in ("1", "0"):
        monkeypatch.setenv("ADVSTEP_WINO_HALVES", halves)
        xa = x.clone().requires_grad_(True)
        y = L.conv3x3_mfm_pool2(xa, weight, bias, bn)
        (got[halves],) = torch.autograd.grad(y, xa, gy)
    assert torch.equal(got["1"], got["0"])
    # and the gradient is the right one (float64 direct convolution through the kernel's own winners, as in the test above)
    xr = x.double().requires_grad_(True)
    conv = torch.nn.functional.conv2d(xr, weight.double(), bias.double(), padding=1)
    y_ref = (ref_mfm_pool(conv) - mean.double().view(1, -1, 1, 1)) * bn[1].double().view(1, -1, 1, 1)
    (gx_ref,) = torch.autograd.grad(y_ref, xr, gy.double())
    err = (got["1"].double() - gx_ref).abs()
    tol = 2e-5 * max(gx_ref.abs().max().item(), 1.0)
    assert (err.max().item() <= tol) or (err > tol).sum().item() <= 9 * 8 * Cin
    # through the kernel's own winners: every entry
    check_through_own_selection(L, "pool2", x, weight, bias, bn, gy, got["1"])


def test_conv3x3_backward_data_matches_aten(L, cuda):
    """The input-gradient convolution on its own (K = 96 and K = 128: the double-buffered weight stream)."""
    from audio_deepfake_adversarial_attacks_amd import _lib
    from audio_deepfake_adversarial_attacks_amd.lcnn_ops import _prepared_weights
    lib = _lib.load()
    g = torch.Generator().manual_seed(5)
    for N, Cin, Cout, H, W in ((2, 32, 96, 20, 12), (1, 48, 128, 13, 7), (3, 32, 64, 10, 10)):
        weight = (torch.randn(Cout, Cin, 3, 3, generator=g) * 0.1).to(cuda)
        gout = torch.randn(N, Cout, H, W, generator=g).to(cuda)
        want = torch.nn.grad.conv2d_input((N, Cin, H, W), weight.double(), gout.double(), padding=1)
        gx = torch.empty(N, Cin, H, W, device=cuda)
        st = lib.advstep_conv3x3_backward_data_f32(gout.data_ptr(), _prepared_weights(weight, 1).data_ptr(), gx.data_ptr(), N, Cin,
                                                   Cout, H, W, torch.cuda.current_stream().cuda_stream)
        assert st == 0
        assert (gx.double() - want).abs().max().item() <= 1e-5 * max(want.abs().max().item(), 1.0), (N, Cin, Cout)


def test_conv3x3_rejects_unsupported(L, cuda):
    assert L.conv3x3_supported(32, 96) and L.conv3x3_supported(48, 128) and L.conv3x3_supported(64, 64)
    assert not L.conv3x3_supported(1, 64) and not L.conv3x3_supported(32, 48) and not L.conv3x3_supported(40, 64)
    x = torch.randn(1, 32, 4, 4, device=cuda, requires_grad=True)
    w = torch.randn(64, 32, 3, 3, device=cuda, requires_grad=True)
    y = L.conv3x3_mfm_pool2(x, w, None)
    (gx,) = torch.autograd.grad(y.sum(), x)          # input gradient only: the weight gets none
    assert gx.shape == x.shape


@pytest.mark.parametrize("N,Cin,C,H,W", [(2, 64, 32, 50, 10), (3, 32, 16, 7, 9), (1, 48, 64, 4, 6)])
@pytest.mark.parametrize("with_bn", [True, False])
def test_conv3x3_mfm_without_pool_matches_float64_reference(L, cuda, N, Cin, C, H, W, with_bn):
    """The un-pooled block (lcnn.py:142-144): same Winograd kernel, max-feature-map + BatchNorm epilogue, one selection
    byte per 2x2 tile; 1e-5 of the output scale, gradient within 2e-5 of float64 autograd except at near-tie flips, and
    everywhere against the float64 reference through the kernel's own selection."""
    g = torch.Generator().manual_seed(N * 100 + Cin + C + H)
    x = torch.randn(N, Cin, H, W, generator=g).to(cuda)
    weight = (torch.randn(2 * C, Cin, 3, 3, generator=g) * 0.1).to(cuda)
    bias = torch.randn(2 * C, generator=g).to(cuda)
    bn = None
    if with_bn:
        mean = torch.randn(C, generator=g).to(cuda)
        var = (torch.rand(C, generator=g) + 0.5).to(cuda)
        bn = (mean, (1.0 / torch.sqrt(var + 1e-5)).contiguous())
    xr = x.double().requires_grad_(True)
    y_ref = ref_mfm(torch.nn.functional.conv2d(xr, weight.double(), bias.double(), padding=1))
    if with_bn:
        y_ref = (y_ref - bn[0].double().view(1, -1, 1, 1)) * bn[1].double().view(1, -1, 1, 1)
    xa = x.clone().requires_grad_(True)
    y = L.conv3x3_mfm(xa, weight, bias, bn)
    assert y.shape == y_ref.shape
    assert (y.double() - y_ref).abs().max().item() <= 1e-5 * max(y_ref.abs().max().item(), 1.0)
    gy = torch.randn(y_ref.shape, generator=g).to(cuda)
    (gx,) = torch.autograd.grad(y, xa, gy)
    (gx_ref,) = torch.autograd.grad(y_ref, xr, gy.double())
    err = (gx.double() - gx_ref).abs()
    tol = 2e-5 * max(gx_ref.abs().max().item(), 1.0)
    assert (err > tol).float().mean().item() <= 1e-3
    # through the kernel's own winners: every entry
    check_through_own_selection(L, "mfm", x, weight, bias, bn, gy, gx)


def test_conv3x3_batch_is_split_for_the_32bit_buffer_descriptor(L, cuda, monkeypatch):
    """The Winograd kernels address a tensor through a 32-bit buffer descriptor (< 2 GiB per call); larger batches are
    split by the wrapper.  Forcing the split on a small problem must not change a single bit."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(5, 32, 12, 10, generator=g).to(cuda)
    w = (torch.randn(96, 32, 3, 3, generator=g) * 0.1).to(cuda)
    b = torch.randn(96, generator=g).to(cuda)
    gy = torch.randn(5, 48, 6, 5, generator=g).to(cuda)

    def run():
        xa = x.clone().requires_grad_(True)
        y = L.conv3x3_mfm_pool2(xa, w, b)
        (gx,) = torch.autograd.grad(y, xa, gy)
        return y.detach(), gx

    y0, g0 = run()
    assert L._batch_chunks(5, 1) == [(0, 5)] and L._batch_chunks(5, (1 << 29) // 2) == [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5)]
    monkeypatch.setattr(L, "_batch_chunks", lambda N, per: [(0, 2), (2, 5)])
    y1, g1 = run()
    assert torch.equal(y0, y1) and torch.equal(g0, g1)


# ---- every launch branch of lcnn_wino.hip::launch_wino, by shape ------------------------------------------------------------------
# Forward: Cin <= 64 keeps its weight chunks resident in LDS, Cin > 64 streams them; C sets the slice count (16 max-feature-map
# pairs per slice); bias and BatchNorm enter through the per-slice constants.  Input gradient (reduction K = 2C): K <= 64
# resident, K > 64 streamed; Cin sets the slices (32 rows each), Cin % 32 == 16 launches the half-empty last slice on its own
# (NT = 1), and the compact backward of a one-slice layer (Cin = 32) on a small plane runs as two 16-row halves
# (ADVSTEP_WINO_HALVES=0 turns that off; the dense path has no such launch).  Planes: odd widths take the WODD kernels,
# odd heights / widths leave edge tiles partial, H or W = 1 pools to nothing (the compact backward then zeroes gx), 15 tiles
# per sample at N = 3 make groups of 16 tiles straddle samples and leave the last one partial.

def _plane(N, H, W):
    return f"{N}x{H}x{W}" + ("-WODD" if W % 2 else "")


def _fwd_case(N, Cin, C, H, W, bias, bn, tag):
    return pytest.param(N, Cin, C, H, W, bias, bn, id=f"{'streamed' if Cin > 64 else 'resident'}-Cin{Cin}-C{C}-"
                        f"{'bias' if bias else 'nobias'}-{'bn' if bn else 'nobn'}-{tag}-{_plane(N, H, W)}")


FWD_CASES = [
    _fwd_case(2, 32, 16, 7, 10, True, True, "Hodd"),
    _fwd_case(1, 48, 32, 6, 9, True, False, "Wodd"),
    _fwd_case(2, 64, 48, 9, 11, False, True, "HWodd"),
    _fwd_case(1, 80, 64, 3, 3, False, False, "3x3"),
    _fwd_case(1, 128, 128, 2, 2, True, True, "2x2-one-tile"),
    _fwd_case(3, 48, 16, 1, 9, False, True, "H1"),
    _fwd_case(2, 80, 32, 10, 1, True, False, "W1"),
    _fwd_case(3, 32, 64, 5, 10, True, True, "15tiles-N3"),
    _fwd_case(3, 256, 48, 6, 9, True, False, "15tiles-N3"),
    _fwd_case(2, 128, 16, 11, 13, False, True, "HWodd"),
    _fwd_case(1, 256, 128, 8, 6, False, False, "K256"),
    _fwd_case(1, 32, 48, 202, 40, True, True, "model"),
    _fwd_case(1, 48, 64, 101, 20, True, True, "model"),
    _fwd_case(2, 64, 32, 50, 10, True, True, "model"),
]


def _random_block(g, cuda, N, Cin, C, H, W, with_bias=True, with_bn=True):
    x = torch.randn(N, Cin, H, W, generator=g).to(cuda)
    weight = (torch.randn(2 * C, Cin, 3, 3, generator=g) * 0.1).to(cuda)
    bias = torch.randn(2 * C, generator=g).to(cuda) if with_bias else None
    bn = None
    if with_bn:
        mean, var = torch.randn(C, generator=g).to(cuda), (torch.rand(C, generator=g) + 0.5).to(cuda)
        bn = (mean, (1.0 / torch.sqrt(var + 1e-5)).contiguous())
    return x, weight, bias, bn


@pytest.mark.parametrize("kind", ["pool2", "mfm"])
@pytest.mark.parametrize("N,Cin,C,H,W,with_bias,with_bn", FWD_CASES)
def test_conv3x3_forward_launch_branches_against_float64(L, cuda, parity_record, request, kind, N, Cin, C, H, W, with_bias,
                                                         with_bn):
    """Pooled (kind pool2) and un-pooled (mfm) forward on every launch branch: selection and values against the float64
    convolution, and the input gradient through the kernel's own selection (check_through_own_selection)."""
    g = torch.Generator().manual_seed(N * 7919 + Cin * 131 + C * 17 + H * 5 + W)
    x, weight, bias, bn = _random_block(g, cuda, N, Cin, C, H, W, with_bias, with_bn)
    gy = torch.randn((N, C, H, W) if kind == "mfm" else (N, C, H // 2, W // 2), generator=g).to(cuda)
    fig = check_through_own_selection(L, kind, x, weight, bias, bn, gy)
    parity_record[f"wino_fwd_{request.node.callspec.id}"] = fig


def _bwd_case(N, Cin, C, H, W, bn, tag, halves=True):
    K = 2 * C
    branch = [f"Cin{Cin}", f"K{K}", "streamed" if K > 64 else "resident"]
    if Cin % 32 == 16:
        branch.append("NT1-last-slice")
    if Cin == 32:
        branch.append("halves" if halves else "halves-off")
    return pytest.param(N, Cin, C, H, W, bn, halves, id="-".join(branch + ["bn" if bn else "nobn", tag, _plane(N, H, W)]))


BWD_CASES = [
    _bwd_case(2, 32, 32, 7, 10, True, "Hodd"),
    _bwd_case(2, 32, 32, 7, 10, False, "Hodd", halves=False),
    _bwd_case(1, 32, 48, 6, 9, True, "Wodd"),
    _bwd_case(2, 48, 16, 9, 11, True, "HWodd"),
    _bwd_case(1, 80, 64, 3, 3, False, "3x3"),
    _bwd_case(1, 64, 128, 2, 2, True, "2x2-one-tile"),
    _bwd_case(3, 96, 48, 1, 9, False, "H1"),
    _bwd_case(2, 256, 16, 10, 1, True, "W1"),
    _bwd_case(3, 48, 32, 6, 10, True, "15tiles-N3"),
    _bwd_case(3, 256, 128, 5, 9, False, "15tiles-N3"),
    _bwd_case(1, 32, 48, 202, 40, True, "model"),
    _bwd_case(1, 48, 64, 101, 20, True, "model"),
    _bwd_case(2, 64, 32, 50, 10, True, "model"),
]


@pytest.mark.parametrize("kind", ["pool2", "mfm"])
@pytest.mark.parametrize("N,Cin,C,H,W,with_bn,halves", BWD_CASES)
def test_conv3x3_input_gradient_of_a_synthetic_selection_matches_float64(L, cuda, monkeypatch, parity_record, request, kind,
                                                                         N, Cin, C, H, W, with_bn, halves):
    """The input-gradient entry points fed random selections instead of a forward's (no ties, so no escape clause): pool2 = the
    compact backward (a code 0-7 per pooled cell), mfm = the max-feature-map routing (a byte 0-15 per 2x2 tile, bits of
    positions outside an odd plane included: they must be ignored) + the dense input-gradient convolution.  Reference:
    gy scattered to the decoded positions [* the BatchNorm's invstd], then a float64 transposed convolution; every entry within
    2e-5 of the gradient scale."""
    monkeypatch.setenv("ADVSTEP_WINO_HALVES", "1" if halves else "0")
    g = torch.Generator().manual_seed(N * 7919 + Cin * 131 + C * 17 + H * 5 + W + (kind == "mfm"))
    weight = (torch.randn(2 * C, Cin, 3, 3, generator=g) * 0.1).to(cuda)
    gscale = (torch.rand(C, generator=g) + 0.5).to(cuda) if with_bn else None
    if kind == "pool2":
        gy = torch.randn(N, C, H // 2, W // 2, generator=g).to(cuda)
        sel = torch.randint(0, 8, gy.shape, generator=g, dtype=torch.uint8).to(cuda)
        dense = dense_grad_pooled(gy, sel, H, W, gscale)
    else:
        gy = torch.randn(N, C, H, W, generator=g).to(cuda)
        sel = torch.randint(0, 16, (N, C, (H + 1) // 2, (W + 1) // 2), generator=g, dtype=torch.uint8).to(cuda)
        dense = dense_grad_unpooled(gy, sel, gscale)
    gx, gout = block_backward(kind, gy, sel, weight, gscale, Cin, H, W)
    if kind == "mfm":
        assert torch.equal(gout, dense.float())       # one fp32 product per entry: exact
    ref = ref_input_grad(kind, dense, weight, (N, Cin, H, W))
    err = (gx.double() - ref).abs().max().item() / max(ref.abs().max().item(), 1.0)
    parity_record[f"wino_bwd_{request.node.callspec.id}"] = {"grad_err_over_scale": err}
    assert err <= 2e-5, err
    gx2, _ = block_backward(kind, gy, sel, weight, gscale, Cin, H, W)
    assert torch.equal(gx, gx2)


@pytest.mark.parametrize("mode", ["cells", "gather"])
@pytest.mark.parametrize("N,C,H,W", [pytest.param(2, 32, 12, 16, id="even-W16"), pytest.param(3, 8, 9, 7, id="Wodd-gather-only"),
                                     pytest.param(1, 32, 6, 130, id="W130-gather-only"), pytest.param(1, 96, 10, 18, id="C96"),
                                     pytest.param(2, 3, 11, 2, id="Hodd-W2"), pytest.param(1, 32, 404, 80, id="model404x80")])
def test_conv5_input_gradient_of_a_synthetic_selection_matches_float64(L, cuda, monkeypatch, parity_record, request, mode,
                                                                       N, C, H, W):
    """The first block's input gradient from random selection codes, both kernels (ADVSTEP_CONV0_BWD; odd widths and pooled
    widths over 64 take the gather whatever the switch says), against the float64 transposed 5x5 convolution of the scattered
    gradient: every entry within 2e-5 of the scale."""
    monkeypatch.setenv("ADVSTEP_CONV0_BWD", mode)
    g = torch.Generator().manual_seed(N * 1009 + C * 31 + H * 7 + W)
    weight = (torch.randn(2 * C, 1, 5, 5, generator=g) * 0.3).to(cuda)
    gy = torch.randn(N, C, H // 2, W // 2, generator=g).to(cuda)
    sel = torch.randint(0, 8, gy.shape, generator=g, dtype=torch.uint8).to(cuda)
    gx, _ = block_backward("conv5", gy, sel, weight, None, 1, H, W)
    ref = ref_input_grad("conv5", dense_grad_pooled(gy, sel, H, W), weight, (N, 1, H, W))
    err = (gx.double() - ref).abs().max().item() / max(ref.abs().max().item(), 1.0)
    parity_record[f"conv5_bwd_{request.node.callspec.id}"] = {"grad_err_over_scale": err}
    assert err <= 2e-5, err
    gx2, _ = block_backward("conv5", gy, sel, weight, None, 1, H, W)
    assert torch.equal(gx, gx2)


def test_conv3x3_xcd_slice_placement_changes_no_bit(L, cuda, monkeypatch):
    """ADVSTEP_WINO_XCD=0 (round-robin slices) against the default placement, which puts the slices of one tile range on one
    XCD.  N = 2 at 202 x 40 is 253 tile groups: the forward at C = 48 (3 slices) and both input gradients at Cin = 64 (2 slices)
    get 32 tile ranges, a multiple of 8 that adds no pass, so the default takes the XCD placement.  It only reassigns work:
    every output bit must be the same."""
    g = torch.Generator().manual_seed(40)
    x, weight, bias, bn = _random_block(g, cuda, 2, 32, 48, 202, 40)
    wb = (torch.randn(96, 64, 3, 3, generator=g) * 0.1).to(cuda)
    gscale = (torch.rand(48, generator=g) + 0.5).to(cuda)
    gyp = torch.randn(2, 48, 101, 20, generator=g).to(cuda)
    selp = torch.randint(0, 8, gyp.shape, generator=g, dtype=torch.uint8).to(cuda)
    gym = torch.randn(2, 48, 202, 40, generator=g).to(cuda)
    selm = torch.randint(0, 16, (2, 48, 101, 20), generator=g, dtype=torch.uint8).to(cuda)
    outs = {}
    for xcd in ("default", "0"):
        if xcd == "default":
            monkeypatch.delenv("ADVSTEP_WINO_XCD", raising=False)
        else:
            monkeypatch.setenv("ADVSTEP_WINO_XCD", xcd)
        outs[xcd] = (*block_forward("pool2", x, weight, bias, bn), *block_forward("mfm", x, weight, bias, bn),
                     block_backward("pool2", gyp, selp, wb, gscale, 64, 202, 40)[0],
                     *block_backward("mfm", gym, selm, wb, gscale, 64, 202, 40))
    assert all(torch.equal(a, b) for a, b in zip(outs["default"], outs["0"]))


def _carved(n, dtype, cuda):
    """(buffer, view of n elements): 64 floats (256 bytes) of sentinel on both sides - the view keeps the allocator's 256-byte
    alignment - and an interior of NaN (floats) or 0xFF (selection bytes), which every output element must overwrite."""
    floats = dtype == torch.float32
    pad = 64 if floats else 256
    buf = torch.full((pad + n + pad,), -7.25 if floats else 0x5A, dtype=dtype, device=cuda)
    buf[pad:pad + n] = float("nan") if floats else 0xFF
    return buf, buf[pad:pad + n]


@pytest.mark.parametrize("Cin,C", [pytest.param(48, 16, id="Cin48-C16"), pytest.param(80, 48, id="Cin80-C48")])
@pytest.mark.parametrize("N,H,W", [pytest.param(2, 6, 9, id="Wodd"), pytest.param(2, 7, 10, id="Hodd"),
                                   pytest.param(1, 9, 11, id="HWodd"), pytest.param(1, 3, 3, id="3x3"),
                                   pytest.param(1, 2, 2, id="2x2"), pytest.param(3, 1, 9, id="H1-pooled-empty"),
                                   pytest.param(2, 10, 1, id="W1-pooled-empty"), pytest.param(3, 5, 10, id="15tiles-N3")])
def test_conv3x3_and_conv5_write_nothing_outside_their_tensors(L, cuda, monkeypatch, Cin, C, N, H, W):
    """Every store of the 3x3 (pooled / un-pooled forward, compact backward, max-feature-map routing, dense input gradient) and
    first-block (forward, both backward kernels) entry points, on odd and edge planes: outputs carved out of sentinel buffers
    (_carved); afterwards the sentinels are intact, no NaN / 0xFF is left inside, and no selection byte exceeds 7 (pooled) or
    15 (one per 2x2 tile).  With H / 2 == 0 or W / 2 == 0 the pooled gradients are zero-filled (their memset path)."""
    g = torch.Generator().manual_seed(N * 100 + H * 10 + W + Cin)
    x, weight, bias, bn = _random_block(g, cuda, N, Cin, C, H, W)
    Ho, Wo, TH, TW = H // 2, W // 2, (H + 1) // 2, (W + 1) // 2
    outs = []

    def out(shape, dtype=torch.float32, top=None):
        n = int(np.prod(shape))
        buf, view = _carved(n, dtype, cuda)
        outs.append((buf, view, top))
        return view.view(shape)

    yp, sp = out((N, C, Ho, Wo)), out((N * C * Ho * Wo,), torch.uint8, 7)
    block_forward("pool2", x, weight, bias, bn, yp, sp)
    ym, sm = out((N, C, H, W)), out((N * C * TH * TW,), torch.uint8, 15)
    block_forward("mfm", x, weight, bias, bn, ym, sm)
    gyp = torch.randn(N, C, Ho, Wo, generator=g).to(cuda)
    gxp = out((N, Cin, H, W))
    block_backward("pool2", gyp, sp, weight, bn[1], Cin, H, W, gx=gxp)
    gym = torch.randn(N, C, H, W, generator=g).to(cuda)
    block_backward("mfm", gym, sm, weight, bn[1], Cin, H, W, gx=out((N, Cin, H, W)), gout=out((N, 2 * C, H, W)))
    x5 = torch.randn(N, 1, H, W, generator=g).to(cuda)
    w5 = (torch.randn(2 * C, 1, 5, 5, generator=g) * 0.3).to(cuda)
    y5, s5 = out((N, C, Ho, Wo)), out((N * C * Ho * Wo,), torch.uint8, 7)
    block_forward("conv5", x5, w5, bias, None, y5, s5)
    gx5 = {}
    for mode in ("cells", "gather"):
        monkeypatch.setenv("ADVSTEP_CONV0_BWD", mode)
        gx5[mode] = out((N, 1, H, W))
        block_backward("conv5", gyp, s5, w5, None, 1, H, W, gx=gx5[mode])
    torch.cuda.synchronize()
    for buf, view, top in outs:
        pad = buf.numel() - view.numel()
        sentinel = -7.25 if top is None else 0x5A
        assert (buf[:pad // 2] == sentinel).all() and (buf[pad // 2 + view.numel():] == sentinel).all()
        if top is None:
            assert not torch.isnan(view).any()
        elif view.numel():
            assert int(view.max()) <= top
    if Ho == 0 or Wo == 0:
        assert not gxp.any() and not gx5["cells"].any() and not gx5["gather"].any()


# ---- GRU layer (SpecRNet) --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T,B,I,layers", [(50, 6, 64, 2), (1, 2, 64, 1), (7, 128, 64, 2), (3, 1, 128, 1)])
def test_gru_layer_matches_torch_gru(L, cuda, T, B, I, layers):
    torch.manual_seed(T * 100 + B)
    H = 64
    ref = torch.nn.GRU(I, H, num_layers=layers, bidirectional=True).double()
    x = torch.randn(T, B, I, dtype=torch.float64, requires_grad=True)
    out_ref, _ = ref(x)
    dout = torch.randn_like(out_ref)
    (dx_ref,) = torch.autograd.grad(out_ref, x, dout)

    xg = x.detach().float().to(cuda).requires_grad_(True)
    seq = xg
    for layer in range(layers):
        sfx = [f"_l{layer}", f"_l{layer}_reverse"]
        w_ih = torch.cat([getattr(ref, "weight_ih" + s) for s in sfx]).float().to(cuda).contiguous()
        w_hh = torch.stack([getattr(ref, "weight_hh" + s) for s in sfx]).float().to(cuda).contiguous()
        b_ih = torch.cat([getattr(ref, "bias_ih" + s) for s in sfx]).float().to(cuda).contiguous()
        b_hh = torch.stack([getattr(ref, "bias_hh" + s) for s in sfx]).float().to(cuda).contiguous()
        seq = L.gru_layer(seq, w_ih.detach(), w_hh.detach(), b_ih.detach(), b_hh.detach())
    (dx,) = torch.autograd.grad(seq, xg, dout.float().to(cuda))
    assert seq.shape == (T, B, 2 * H)
    assert (seq.double().cpu() - out_ref).abs().max().item() <= 3e-6
    assert (dx.double().cpu() - dx_ref).abs().max().item() <= 3e-5 * max(dx_ref.abs().max().item(), 1.0)


def test_specrnet_uses_gru_kernel_when_frozen_and_matches_miopen(cuda, monkeypatch):
    from audio_deepfake_adversarial_attacks_amd.models.models import get_model
    monkeypatch.setenv("ADVSTEP_SPECRNET_ELEM", "0")     # this test isolates the GRU kernels (the elementwise fusions have their own)
    torch.manual_seed(5)
    model = get_model("specrnet", {"frontend_algorithm": ["mel_spec"], "input_channels": 2}, str(cuda)).to(cuda)
    model.train()                      # attack mode (attack.py:311-319): train, BatchNorm / Dropout in eval
    for m in model.modules():
        if "BatchNorm" in m.__class__.__name__ or "Dropout" in m.__class__.__name__:
            m.eval()
    spec = torch.randn(6, 2, 80, 404, device=cuda)

    def run(kernel, frozen):
        monkeypatch.setenv("ADVSTEP_SPECRNET_GRU", "1" if kernel else "0")
        for p in model.parameters():
            p.requires_grad_(not frozen)
        a = spec.clone().requires_grad_(True)
        z = model._compute_embedding(a)
        (g,) = torch.autograd.grad(z.sum(), a)
        return z.detach(), g

    z0, g0 = run(False, True)           # MIOpen
    z1, g1 = run(True, True)            # HIP kernels
    z2, g2 = run(True, False)           # parameters need grad -> torch.nn.GRU, identical to z0
    assert torch.equal(z2, z0)
    assert (z1 - z0).abs().max().item() <= 2e-5 * max(z0.abs().max().item(), 1.0)
    assert (g1 - g0).abs().max().item() <= 1e-4 * max(g0.abs().max().item(), 1e-6)
    for p in model.parameters():
        p.requires_grad_(True)


def test_lcnn_tail_as_one_node_matches_the_separate_ops(cuda, monkeypatch, parity_record):
    """lcnn_ops.lcnn_tail (pack -> two recurrent layers -> skip + mean + Linear as ONE autograd node, the mean's gradient read
    with a zero frame stride, the two gradients of `hidden` summed while they return to the convolution's layout) against the
    same fused LSTM kernels driven by the separate torch ops (src/models/lcnn.py:196-205): logits and the gradient w.r.t. the
    convolution trunk's output.  Same kernels for the recurrences; only the summation order of the mean / Linear differs."""
    from audio_deepfake_adversarial_attacks_amd.models import lcnn
    torch.manual_seed(7)
    body = lcnn.BaseLCNN(input_channels=1, num_coefficients=80).to(cuda)
    body.train()
    for m in body.modules():
        if "BatchNorm" in m.__class__.__name__ or "Dropout" in m.__class__.__name__:
            m.eval()
    for p in body.parameters():
        p.requires_grad_(False)
    spec = torch.randn(6, 1, 80, 404, generator=torch.Generator().manual_seed(8)).to(cuda)

    def run(tail):
        monkeypatch.setenv("ADVSTEP_LCNN_TAIL", "1" if tail else "0")
        a = spec.clone().requires_grad_(True)
        z = body(a)
        (g,) = torch.autograd.grad((z * torch.arange(1, 7, device=cuda).view(6, 1)).sum(), a)
        return z.detach(), g

    z0, g0 = run(False)
    z1, g1 = run(True)
    fig = {"logit_max_abs": (z0 - z1).abs().max().item(), "grad_rel_l2": ((g0 - g1).norm() / g0.norm()).item(),
           "grad_max_abs_over_max": ((g0 - g1).abs().max() / g0.abs().max()).item()}
    parity_record["lcnn_tail_one_node_vs_separate_ops"] = fig
    assert z1.shape == (6, 1) and fig["logit_max_abs"] <= 3e-7, fig
    assert fig["grad_rel_l2"] <= 5e-6 and fig["grad_max_abs_over_max"] <= 5e-6, fig
    with torch.no_grad():                                  # the scoring pass (no autograd) takes the same node
        monkeypatch.setenv("ADVSTEP_LCNN_TAIL", "1")
        assert (body.eval()(spec) - body(spec)).abs().max().item() == 0.0
