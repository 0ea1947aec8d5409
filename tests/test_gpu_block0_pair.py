"""`-m gpu`: the first LCNN block and the 1x1 block behind it as one kernel each way (advstep_conv5_conv1x1_mfm_forward_f32,
advstep_conv5_conv1x1_mfm_backward_f32) against the two launches each replaces, through the C ABI.  The fused kernels run the
same fma chains in the same order - the first block's packed FMAs, v_mfma_f32_32x32x2_f32 over the 1x1 block's k-steps - so
every comparison is `torch.equal` on the raw bits (floats viewed as int32: NaN payloads included), whole buffers, no
tolerance.

Shapes (N = 2, C = 32): 12 x 10 (30 pooled positions: less than one 32-pixel tile), 36 x 20 (180 positions: three waves of one
workgroup, ragged last tiles for the 32- and the 64-position grouping), 8 x 128 (the widest plane the cell-centric first-block
backward takes), and 40 x 32 in the bounds test (320 positions: a second workgroup)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

C = 32
SHAPES = [pytest.param(12, 10, id="12x10"), pytest.param(36, 20, id="36x20"), pytest.param(8, 128, id="8x128")]


@pytest.fixture(scope="module")
def L(cuda):
    from audio_deepfake_adversarial_attacks_amd import lcnn_ops
    return lcnn_ops


def _abi():
    from audio_deepfake_adversarial_attacks_amd import _lib
    return _lib.load(), torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def block(cuda, N, H, W, seed, with_bias=True, with_bn=True, ties=False):
    """x, (weight, bias) of the first block, (weight1, bias1) of the 1x1 block, (mean, invstd) or None."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, 1, H, W, generator=g)
    w5 = torch.randn(2 * C, 1, 5, 5, generator=g) * 0.3
    w1 = torch.randn(2 * C, C, 1, 1, generator=g) * 0.2
    b5 = torch.randn(2 * C, generator=g) * 0.1 if with_bias else None
    b1 = torch.randn(2 * C, generator=g) * 0.1 if with_bias else None
    if ties:
        # values on a coarse binary grid (every sum exact), the two halves of the even channels equal: exact ties between the
        # max-feature-map halves of both blocks; a constant 6 x 6 corner of the input: exact ties between pool candidates
        x = (x * 2).round() / 2
        x[:, :, :6, :6] = 1.0
        w5 = (w5 * 8).round() / 8
        w1 = (w1 * 8).round() / 8
        w5[C::2] = w5[:C:2]
        w1[C::2] = w1[:C:2]
        if with_bias:
            b5 = (b5 * 8).round() / 8
            b1 = (b1 * 8).round() / 8
            b5[C::2] = b5[:C:2]
            b1[C::2] = b1[:C:2]
    bn = None
    if with_bn:
        bn = (torch.randn(C, generator=g).to(cuda), (torch.rand(C, generator=g) + 0.5).to(cuda))
    dev = lambda t: None if t is None else t.to(cuda)
    return dev(x), dev(w5), dev(b5), dev(w1), dev(b1), bn


def outputs(lib, cuda, N, P):
    y = torch.full((N, C, P), float("nan"), device=cuda)
    idx = torch.full((N * C * P,), 0xFF, dtype=torch.uint8, device=cuda)
    sel = torch.full((lib.advstep_conv1x1_mfm_sel_bytes(N, C, P),), 0xFF, dtype=torch.uint8, device=cuda)
    return y, idx, sel


def two_launches(x, w5, b5, w1, b1, bn):
    """The reference: advstep_conv5_mfm_pool2_forward_f32, then advstep_conv1x1_mfm_forward_f32 -> (y, idx, sel)."""
    lib, st = _abi()
    N, _, H, W = x.shape
    P = (H // 2) * (W // 2)
    y, idx, sel = outputs(lib, x.device, N, P)
    mid = torch.empty(N, C, P, device=x.device)
    assert lib.advstep_conv5_mfm_pool2_forward_f32(_ptr(x), _ptr(w5), _ptr(b5), _ptr(mid), _ptr(idx), N, C, H, W, st) == 0
    assert lib.advstep_conv1x1_mfm_forward_f32(_ptr(mid), _ptr(w1), _ptr(b1), _ptr(bn and bn[0]), _ptr(bn and bn[1]), _ptr(y),
                                               _ptr(sel), N, C, C, P, st) == 0
    return y, idx, sel


def one_launch(x, w5, b5, w1, b1, bn, out=None):
    lib, st = _abi()
    N, _, H, W = x.shape
    y, idx, sel = out or outputs(lib, x.device, N, (H // 2) * (W // 2))
    assert lib.advstep_conv5_conv1x1_mfm_supported(C, C, H, W) == 1
    assert lib.advstep_conv5_conv1x1_mfm_forward_f32(_ptr(x), _ptr(w5), _ptr(b5), _ptr(w1), _ptr(b1), _ptr(bn and bn[0]),
                                                     _ptr(bn and bn[1]), _ptr(y), _ptr(idx), _ptr(sel), N, C, C, H, W, st) == 0
    return y, idx, sel


def assert_same_bits(got, want):
    for name, g, w in zip(("y", "selection bytes", "masks"), got, want):
        assert torch.equal(bits(g), bits(w)), name


@pytest.mark.parametrize("with_bn", [False, True], ids=["nobn", "bn"])
@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("H,W", SHAPES)
def test_forward_equals_the_two_launches(cuda, H, W, with_bias, with_bn):
    args = block(cuda, 2, H, W, H * W + 2 * with_bias + with_bn, with_bias, with_bn)
    want = two_launches(*args)
    assert_same_bits(one_launch(*args), want)
    assert not torch.isnan(want[0]).any() and int(want[1].max()) <= 7


@pytest.mark.parametrize("H,W", SHAPES)
def test_forward_with_exact_ties(cuda, H, W):
    args = block(cuda, 2, H, W, 7, ties=True)
    want = two_launches(*args)
    # the planted ties are there: equal halves (code < 4 with both candidates equal cannot be seen from outside, so count the
    # first block's sums instead) and pool candidates that agree
    conv = torch.nn.functional.conv2d(args[0].double(), args[1].double(), args[2].double(), padding=2)
    assert torch.equal(conv[:, :C:2], conv[:, C::2]) and (conv[:, :, 2:4, 2:4] == conv[:, :, 2:3, 2:3]).all()
    assert_same_bits(one_launch(*args), want)


def test_forward_with_a_nan_and_an_infinity(cuda):
    x, *rest = block(cuda, 2, 36, 20, 8)
    x[0, 0, 7, 9] = float("nan")
    x[1, 0, 20, 3] = float("inf")
    want = two_launches(x, *rest)
    assert torch.isnan(want[0]).any() and not torch.isnan(want[0]).all()
    assert_same_bits(one_launch(x, *rest), want)


@pytest.mark.parametrize("H,W", SHAPES + [pytest.param(40, 32, id="40x32-two-workgroups")])
def test_forward_writes_nothing_outside_its_tensors(cuda, H, W):
    """y, the selection bytes and the masks carved out of sentinel buffers; the sentinels survive, every element of y and every
    selection byte is overwritten, and the masks equal the two-launch ones where that kernel writes them (mask slots of pixels
    beyond the plane stay as allocated in both)."""
    lib, _ = _abi()
    N, P = 2, (H // 2) * (W // 2)
    args = block(cuda, N, H, W, 9)
    carved = []
    for n, dtype in ((N * C * P, torch.float32), (N * C * P, torch.uint8), (lib.advstep_conv1x1_mfm_sel_bytes(N, C, P), torch.uint8)):
        pad = 64 if dtype == torch.float32 else 256
        buf = torch.full((pad + n + pad,), -7.25 if dtype == torch.float32 else 0x5A, dtype=dtype, device=cuda)
        buf[pad:pad + n] = float("nan") if dtype == torch.float32 else 0xFF
        carved.append((buf, buf[pad:pad + n], pad))
    got = one_launch(*args, out=(carved[0][1].view(N, C, P), carved[1][1], carved[2][1]))
    torch.cuda.synchronize()
    for buf, view, pad in carved:
        sentinel = -7.25 if buf.dtype == torch.float32 else 0x5A
        assert (buf[:pad] == sentinel).all() and (buf[pad + view.numel():] == sentinel).all()
    assert not torch.isnan(got[0]).any() and int(got[1].max()) <= 7
    assert_same_bits(got, two_launches(*args))


def two_backward_launches(gy, sel, w1, gscale, idx, w5, H, W):
    """The reference: advstep_conv1x1_mfm_backward_f32 into a temporary, then advstep_conv5_mfm_pool2_backward_f32."""
    lib, st = _abi()
    N, P = gy.shape[0], (H // 2) * (W // 2)
    mid = torch.empty(N, C, P, device=gy.device)
    gx = torch.full((N, 1, H, W), float("nan"), device=gy.device)
    assert lib.advstep_conv1x1_mfm_backward_f32(_ptr(gy), _ptr(sel), _ptr(w1), _ptr(gscale), _ptr(mid), N, C, C, P, st) == 0
    assert lib.advstep_conv5_mfm_pool2_backward_f32(_ptr(mid), _ptr(idx), _ptr(w5), _ptr(gx), N, C, H, W, st) == 0
    return gx


def one_backward_launch(gy, sel, w1, gscale, idx, w5, H, W, gx=None):
    lib, st = _abi()
    N = gy.shape[0]
    gx = torch.full((N, 1, H, W), float("nan"), device=gy.device) if gx is None else gx
    assert lib.advstep_conv5_conv1x1_mfm_backward_supported(C, C, H, W) == 1
    assert lib.advstep_conv5_conv1x1_mfm_backward_f32(_ptr(gy), _ptr(sel), _ptr(w1), _ptr(gscale), _ptr(idx), _ptr(w5), _ptr(gx),
                                                      N, C, C, H, W, st) == 0
    return gx


def output_gradient(cuda, N, H, W, zeros):
    g = torch.Generator().manual_seed(3)
    gy = torch.randn(N, C, H // 2, W // 2, generator=g)
    if zeros:
        kind = torch.randint(0, 3, gy.shape, generator=g)
        gy = torch.where(kind == 0, torch.zeros(()), torch.where(kind == 1, -torch.zeros(()), gy))
        assert (gy == 0).any() and torch.signbit(gy[gy == 0]).any()
    return gy.to(cuda)


BWD_SHAPES = SHAPES + [pytest.param(44, 80, id="44x80-two-tiles")]        # 22 pooled rows of 40: two row tiles, halo rows


@pytest.mark.parametrize("with_gscale", [False, True], ids=["noscale", "gscale"])
@pytest.mark.parametrize("zeros", [False, True], ids=["random", "zeros"])
@pytest.mark.parametrize("H,W", BWD_SHAPES)
def test_backward_equals_the_two_launches(cuda, H, W, zeros, with_gscale):
    """From the forward's own selection bytes and masks, for a random dY and for one with zeros and negative zeros; gscale = the
    folded BatchNorm's invstd.  gx sits between sentinels: nothing is written outside it, every element of it is."""
    x, w5, b5, w1, b1, bn = block(cuda, 2, H, W, 11 + H, with_bn=with_gscale)
    _, idx, sel = two_launches(x, w5, b5, w1, b1, bn)
    gy = output_gradient(cuda, 2, H, W, zeros)
    gscale = bn[1] if with_gscale else None
    want = two_backward_launches(gy, sel, w1, gscale, idx, w5, H, W)
    buf = torch.full((64 + 2 * H * W + 64,), -7.25, device=cuda)
    buf[64:-64] = float("nan")
    got = one_backward_launch(gy, sel, w1, gscale, idx, w5, H, W, gx=buf[64:-64].view(2, 1, H, W))
    torch.cuda.synchronize()
    assert (buf[:64] == -7.25).all() and (buf[-64:] == -7.25).all() and not torch.isnan(got).any()
    assert torch.equal(bits(got), bits(want)) and got.abs().sum() > 0


def gradient(L, paired, x, w5, b5, w1, b1, bn, gy):
    xr = x.clone().requires_grad_(True)
    y = L.conv5_conv1x1_mfm(xr, w5, b5, w1, b1, bn) if paired else L.conv1x1_mfm(L.conv5_mfm_pool2(xr, w5, b5), w1, b1, bn)
    (gx,) = torch.autograd.grad(y, xr, gy)
    return y, gx


@pytest.mark.parametrize("fused_bwd", ["1", "0"], ids=["bwd-fused", "bwd-two-launches"])
@pytest.mark.parametrize("H,W", SHAPES)
def test_input_gradient_of_the_node_equals_the_two_nodes(L, cuda, monkeypatch, H, W, fused_bwd):
    """The pair's autograd node (it saves the selection bytes and the masks only) against the two blocks' own nodes, with its
    backward fused and as two launches through a temporary."""
    monkeypatch.setenv("ADVSTEP_LCNN_BLOCK0_PAIR_BWD", fused_bwd)
    args = block(cuda, 2, H, W, 13 + H)
    gy = output_gradient(cuda, 2, H, W, False)
    y1, gx1 = gradient(L, True, *args, gy)
    y2, gx2 = gradient(L, False, *args, gy)
    assert torch.equal(bits(y1), bits(y2)) and torch.equal(bits(gx1), bits(gx2)) and gx1.abs().sum() > 0


# ---- routing ---------------------------------------------------------------------------------------------------------------

def trunk(cuda, C0=C, C1=C, with_bn=True):
    """A BaseLCNN whose transform is the first block, a 1x1 block [and its BatchNorm] only."""
    from audio_deepfake_adversarial_attacks_amd.models import lcnn
    torch.manual_seed(0)
    model = lcnn.BaseLCNN(input_channels=1)
    layers = [torch.nn.Conv2d(1, 2 * C0, (5, 5), 1, padding=(2, 2)), lcnn.MaxFeatureMap2D(), torch.nn.MaxPool2d((2, 2), (2, 2)),
              torch.nn.Conv2d(C0, 2 * C1, (1, 1)), lcnn.MaxFeatureMap2D()]
    if with_bn:
        layers.append(torch.nn.BatchNorm2d(C1, affine=False))
    model.m_transform = torch.nn.Sequential(*layers)
    model = model.to(cuda).eval()
    for p in model.parameters():
        p.requires_grad_(False)
    return model


def launches(model, x):
    """{entry point: launches} of one forward + backward of the trunk, and (y, gx)."""
    from audio_deepfake_adversarial_attacks_amd import hip_ops
    xr = x.clone().requires_grad_(True)
    hip_ops.start_profile("*")
    y = model._transform(xr)
    (gx,) = torch.autograd.grad(y.sum(), xr)
    ms = hip_ops.stop_profile()
    return {k: len(v) for k, v in ms.items()}, y, gx


PAIR = {"conv5_mfm_pool2_forward": 1, "conv5_mfm_pool2_backward": 1}                    # one launch each way
PAIR_FWD = dict(PAIR, conv1x1_mfm_backward=1)                                            # ... in the forward only
TWO = dict(PAIR_FWD, conv1x1_mfm_forward=1)


@pytest.mark.parametrize("C0,C1,H,W,want", [
    pytest.param(32, 32, 12, 10, PAIR, id="lcnn-shape"), pytest.param(32, 32, 13, 10, TWO, id="odd-H"),
    pytest.param(32, 32, 12, 11, TWO, id="odd-W"), pytest.param(48, 48, 12, 10, TWO, id="C48"),
    pytest.param(32, 48, 12, 10, TWO, id="1x1-block-of-48"),
    pytest.param(32, 32, 4, 132, PAIR_FWD, id="wider-than-the-cell-kernel")])
def test_routing(cuda, monkeypatch, C0, C1, H, W, want):
    monkeypatch.delenv("ADVSTEP_LCNN_BLOCK0_PAIR", raising=False)
    monkeypatch.delenv("ADVSTEP_LCNN_BLOCK0_PAIR_BWD", raising=False)
    model = trunk(cuda, C0, C1)
    x = torch.randn(2, 1, H, W, generator=torch.Generator().manual_seed(1)).to(cuda)
    counts, y, gx = launches(model, x)
    assert counts == want
    if want == PAIR:
        monkeypatch.setenv("ADVSTEP_LCNN_BLOCK0_PAIR_BWD", "0")           # only the forward is fused
        counts1, y1, gx1 = launches(model, x)
        assert counts1 == PAIR_FWD and torch.equal(bits(y), bits(y1)) and torch.equal(bits(gx), bits(gx1))
    monkeypatch.setenv("ADVSTEP_LCNN_BLOCK0_PAIR", "0")
    counts0, y0, gx0 = launches(model, x)
    assert counts0 == TWO
    assert torch.equal(bits(y), bits(y0)) and torch.equal(bits(gx), bits(gx0))


def test_routing_leaves_an_unfrozen_or_unfoldable_tail_alone(cuda, monkeypatch):
    """A 1x1 block whose weights want gradients keeps its own path; a BatchNorm in training mode is not folded but the pair
    still forms in front of it."""
    monkeypatch.delenv("ADVSTEP_LCNN_BLOCK0_PAIR", raising=False)
    monkeypatch.delenv("ADVSTEP_LCNN_BLOCK0_PAIR_BWD", raising=False)
    x = torch.randn(2, 1, 12, 10, generator=torch.Generator().manual_seed(2)).to(cuda)
    model = trunk(cuda)
    model.m_transform[3].weight.requires_grad_(True)
    assert "conv1x1_mfm_forward" not in launches(model, x)[0] and launches(model, x)[0]["conv5_mfm_pool2_forward"] == 1
    model = trunk(cuda)
    model.m_transform[5].train()
    counts, y, _ = launches(model, x)
    assert counts == PAIR
    assert y.mean(dim=(0, 2, 3)).abs().max() < 1e-5          # the BatchNorm module itself normalised with batch statistics


# ---- the whole model ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lcnn_model(cuda):
    from audio_deepfake_adversarial_attacks_amd.models.models import get_model
    torch.manual_seed(0)
    model = get_model("lcnn", {"frontend_algorithm": ["lfcc"], "input_channels": 1}, str(cuda)).to(cuda).eval()
    for p in model.parameters():          # as inside an attack: the fused blocks want frozen parameters
        p.requires_grad_(False)
    return model


@pytest.fixture()
def fresh_graphs():
    from audio_deepfake_adversarial_attacks_amd.torchattacks import graphed
    graphed.clear()
    yield graphed
    graphed.clear()


def waves(cuda, n, seed, T):
    from audio_deepfake_adversarial_attacks_amd.datasets.synthetic import synthetic_waveforms
    from audio_deepfake_adversarial_attacks_amd.aa import utils as aa_utils
    x, y = synthetic_waveforms(n, T, seed)
    x01, _, _ = aa_utils.to_minmax(x.to(cuda))
    return x01, y.to(cuda)


def first_block_forward_launches(model, x):
    from audio_deepfake_adversarial_attacks_amd import hip_ops
    hip_ops.start_profile("conv5_mfm_pool2_forward", "conv1x1_mfm_forward")
    with torch.no_grad():
        model(x)
    ms = hip_ops.stop_profile()
    return len(ms["conv5_mfm_pool2_forward"]), len(ms["conv1x1_mfm_forward"])


# T = 6 400 gives 41 frames, an odd plane: the model keeps two launches there whatever the switch says.  T = 6 560 gives 42
# frames: the pair runs (checked with the launch profile).
@pytest.mark.parametrize("T,paired", [pytest.param(6400, False, id="T6400"), pytest.param(6560, True, id="T6560")])
def test_logits_and_waveform_gradient_do_not_depend_on_the_switch(cuda, monkeypatch, lcnn_model, T, paired):
    x01, _ = waves(cuda, 2, 3, T)
    got = {}
    for switch in ("1", "0"):
        monkeypatch.setenv("ADVSTEP_LCNN_BLOCK0_PAIR", switch)
        assert first_block_forward_launches(lcnn_model, x01) == ((1, 3) if paired and switch == "1" else (1, 4))
        xr = x01.clone().requires_grad_(True)
        logits = lcnn_model(xr)
        (gx,) = torch.autograd.grad(logits.sum(), xr)
        got[switch] = (logits.detach(), gx)
    assert torch.equal(bits(got["1"][0]), bits(got["0"][0])) and torch.equal(bits(got["1"][1]), bits(got["0"][1]))
    assert got["1"][1].abs().sum() > 0


@pytest.mark.parametrize("T", [6400, 6560])
def test_graph_replay_does_not_depend_on_the_switch(cuda, monkeypatch, fresh_graphs, lcnn_model, T):
    """PGD, 4 steps: eager launches with the switch off against eager, captured and replayed iterations with it on."""
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    atk = torchattacks.PGD(lcnn_model, eps=0.003, alpha=0.001, steps=4, random_start=False)
    atk.set_training_mode(model_training=False, batchnorm_training=False)
    x01, y = waves(cuda, 2, 4, T)
    monkeypatch.setenv("ADVSTEP_LCNN_BLOCK0_PAIR", "0")
    monkeypatch.setenv("ADVSTEP_ATTACK_GRAPH", "0")
    want = atk(x01, y)
    assert not torch.equal(want, x01)
    monkeypatch.setenv("ADVSTEP_LCNN_BLOCK0_PAIR", "1")
    assert torch.equal(atk(x01, y), want)
    monkeypatch.setenv("ADVSTEP_ATTACK_GRAPH", "1")
    for held in (0, 1, 1):                                   # first sight, second sight (capture), replay
        assert torch.equal(atk(x01, y), want) and len(fresh_graphs._GRAPHS) == held


@pytest.mark.parametrize("T", [6400, 6560])
def test_two_batches_in_flight_do_not_depend_on_the_switch(cuda, monkeypatch, fresh_graphs, T):
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    from audio_deepfake_adversarial_attacks_amd.datasets.synthetic import SyntheticDetectionDataset
    from audio_deepfake_adversarial_attacks_amd.evaluation import generate_attacks
    cfg = {"data": {"seed": 42}, "checkpoint": {"path": ""},
           "model": {"name": "lcnn", "parameters": {"frontend_algorithm": ["lfcc"], "input_channels": 1}}}

    def scores(switch, in_flight):
        monkeypatch.setenv("ADVSTEP_LCNN_BLOCK0_PAIR", switch)
        torch.manual_seed(5)
        fresh_graphs.clear()
        rep = generate_attacks([None, None, None], cfg, str(cuda), attack_model_config=cfg, attack_method=torchattacks.PGD,
                               attack_params={"eps": 0.003, "steps": 4}, batch_size=2, dataset=SyntheticDetectionDataset(12, T), share_weights=True,
                               shuffle=False, num_workers=0, return_scores=True, in_flight=in_flight)
        return torch.as_tensor(rep["scores"]["y_pred"])

    want = scores("0", 1)
    assert torch.equal(scores("1", 1), want) and torch.equal(scores("1", 2), want)


def test_a_listener_on_the_per_block_entry_points_keeps_the_two_calls(L, cuda, monkeypatch):
    """Whoever wraps lcnn_ops.conv5_mfm_pool2 / conv1x1_mfm (the parity attribution does, to read each block's input and
    winners) must keep being called: the model does not form the pair then, and gives the same bits."""
    monkeypatch.delenv("ADVSTEP_LCNN_BLOCK0_PAIR", raising=False)
    model = trunk(cuda)
    x = torch.randn(2, 1, 12, 10, generator=torch.Generator().manual_seed(4)).to(cuda)
    counts, y, gx = launches(model, x)
    assert counts == PAIR
    seen, original = [], L.conv1x1_mfm

    def listener(inp, *args, **kwargs):
        seen.append(tuple(inp.shape))
        return original(inp, *args, **kwargs)

    monkeypatch.setattr(L, "conv1x1_mfm", listener)
    counts1, y1, gx1 = launches(model, x)
    assert counts1 == TWO and seen == [(2, C, 6, 5)]
    assert torch.equal(bits(y), bits(y1)) and torch.equal(bits(gx), bits(gx1))
