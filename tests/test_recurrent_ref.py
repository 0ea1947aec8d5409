"""The references of tests/recurrent_ref.py pinned without a GPU: against torch.nn.LSTM / torch.nn.GRU in float64 (values and
autograd gradients, D = 2, D = 1 and the reverse direction on its own), the closed-form backward against autograd, the tail's
one-liners against the module chain, and the admission condition of every case the GPU suite uses."""
import pytest
import torch

from tests import recurrent_ref as R

ULP64 = 2.0 ** -52
# The loops and the modules do the same float64 operations; only the order inside the h W_hh^T products (and, for the GRU, of
# the three-term gate sums) may differ: a few ulp on values that are O(1).  A gradient sums T steps of 4H (3H) such terms.
TAU_VALUE = 8 * ULP64
TAU_GRAD = 64 * ULP64


def _rel(a, ref):
    return ((a - ref).abs().max() / ref.abs().max().clamp(min=1.0)).item()


def _module_case(kind, I, T, B, D, seed):
    torch.manual_seed(seed)
    H = R.LSTM_H if kind == "lstm" else R.GRU_H
    mod = (torch.nn.LSTM if kind == "lstm" else torch.nn.GRU)(I, H, bidirectional=D == 2).double()
    x = torch.randn(T, B, I, dtype=torch.float64)
    dout = torch.randn(T, B, D * H, dtype=torch.float64)
    return mod, x, dout


def _project(mod, kind, x, sfx):
    """gx (T, B, D, G*H), w_hh (D, G*H, H) [, b_hh (D, 3H)] from a module's parameters, as lcnn_ops' layers form them."""
    w_ih = [getattr(mod, "weight_ih_l0" + s) for s in sfx]
    b_ih = [getattr(mod, "bias_ih_l0" + s) for s in sfx]
    b_hh = [getattr(mod, "bias_hh_l0" + s) for s in sfx]
    w_hh = torch.stack([getattr(mod, "weight_hh_l0" + s) for s in sfx]).detach()
    if kind == "lstm":
        gx = torch.stack([x @ w.t() + bi + bh for w, bi, bh in zip(w_ih, b_ih, b_hh)], 2)
        return gx, w_hh, None
    gx = torch.stack([x @ w.t() + bi for w, bi in zip(w_ih, b_ih)], 2)
    return gx, w_hh, torch.stack(b_hh).detach()


def _forward(kind, gx, w_hh, b_hh):
    return R.lstm_forward(gx, w_hh, torch.float64) if kind == "lstm" else R.gru_forward(gx, w_hh, b_hh, torch.float64)


@pytest.mark.parametrize("kind,I", [("lstm", 160), ("gru", 64)])
@pytest.mark.parametrize("T,B", [(25, 3), (1, 2), (2, 1), (7, 4)])
@pytest.mark.parametrize("D", [1, 2])
def test_forward_and_autograd_match_the_torch_modules(kind, I, T, B, D):
    mod, x, dout = _module_case(kind, I, T, B, D, 100 * T + 10 * B + D)
    a = x.clone().requires_grad_(True)
    b = x.clone().requires_grad_(True)
    y_mod, state = mod(a)
    gx, w_hh, b_hh = _project(mod, kind, b, ["", "_reverse"][:D])
    fwd = _forward(kind, gx, w_hh, b_hh)
    assert fwd[0].shape == y_mod.shape
    assert _rel(fwd[0], y_mod) <= TAU_VALUE
    if kind == "lstm":                                     # the module's final cell state: step T - 1 of each direction
        c_last = torch.stack([fwd[2][R._time_of(T - 1, d, T), :, d] for d in range(D)])
        assert _rel(c_last, state[1]) <= TAU_VALUE
    (g_mod,) = torch.autograd.grad(y_mod, a, dout)
    (g_ref,) = torch.autograd.grad(fwd[0], b, dout)
    assert _rel(g_ref, g_mod) <= TAU_GRAD


@pytest.mark.parametrize("kind,I", [("lstm", 160), ("gru", 64)])
def test_reverse_direction_alone_is_a_forward_module_on_flipped_time(kind, I):
    """d = 1 of a D = 2 run against a UNIdirectional module that holds the reverse direction's weights and sees the input
    flipped in time: the reverse direction without the bidirectional module's own bookkeeping."""
    T, B = 9, 3
    bi, x, dout = _module_case(kind, I, T, B, 2, 17)
    H = bi.hidden_size
    uni = type(bi)(I, H).double()
    with torch.no_grad():
        for n in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"):
            getattr(uni, n).copy_(getattr(bi, n + "_reverse"))
    a = x.clone().requires_grad_(True)
    b = x.clone().requires_grad_(True)
    y_uni = uni(a.flip(0))[0].flip(0)
    gx, w_hh, b_hh = _project(bi, kind, b, ["", "_reverse"])
    out = _forward(kind, gx, w_hh, b_hh)[0][:, :, H:]
    assert _rel(out, y_uni) <= TAU_VALUE
    (g_uni,) = torch.autograd.grad(y_uni, a, dout[:, :, H:])
    (g_ref,) = torch.autograd.grad(out, b, dout[:, :, H:])
    assert _rel(g_ref, g_uni) <= TAU_GRAD


@pytest.mark.parametrize("kind", ["lstm", "gru"])
@pytest.mark.parametrize("row", [("default", 25, 3, 2), ("default", 1, 2, 1), ("default", 2, 2, 2), ("default", 3, 1, 1),
                                 ("x4", 25, 3, 2), ("sat", 25, 3, 2), ("sat", 60, 2, 1)])
def test_closed_form_backward_is_autograd_backward(kind, row):
    """The stage reference (closed form from saved state) against float64 autograd through the forward, on the forward's own
    float64 state; also with dout zero but for one element."""
    case = R.make_case(kind, row)
    T, B, D = row[1:]
    for one_hot in (False, True):
        if one_hot:
            d1 = torch.zeros_like(case["dout"])
            d1[T // 2, B - 1, (D - 1) * (case["dout"].shape[2] // D) + 5] = 1.5
            case = dict(case, dout=d1)
        fwd, g_auto = R.autograd_dgx(kind, case, torch.float64)
        if kind == "lstm":
            g_closed = R.lstm_backward(case["dout"], case["w_hh"], fwd[1], fwd[2])
        else:
            g_closed = R.gru_backward(case["dout"], case["w_hh"], fwd[1], fwd[0])
        assert R.per_row_err(g_closed, g_auto) <= 1e-12


def test_bcast_and_outer_are_backward_of_the_expanded_gradient():
    case = R.make_case("lstm", ("default", 7, 3, 2))
    out, gates, cell = R.lstm_forward(case["gx"], case["w_hh"], torch.float64)
    g = torch.Generator().manual_seed(3)
    dz, row = torch.randn(3, generator=g), torch.randn(2 * R.LSTM_H, generator=g)
    full = (dz.double().view(1, 3, 1) * row.double().view(1, 1, -1)).expand(7, -1, -1)
    want = R.lstm_backward(full, case["w_hh"], gates, cell)
    assert torch.equal(R.lstm_backward_outer(dz, row, case["w_hh"], gates, cell), want)
    assert torch.equal(R.lstm_backward_bcast(full[0], case["w_hh"], gates, cell), want)


def test_tail_one_liners_are_the_module_chain():
    """pack / tail_forward / unpack_add(_outer) against permute + view, (lstm + hidden).mean(1) -> Linear and its autograd."""
    B, C, T, W = 3, 5, 7, 9
    g = torch.Generator().manual_seed(5)
    x4 = torch.randn(B, C, T, W, generator=g, dtype=torch.float64, requires_grad=True)
    hidden = x4.permute(0, 2, 1, 3).contiguous().view(B, T, C * W)
    xt = R.pack(x4)
    assert torch.equal(xt, hidden.permute(1, 0, 2))
    lin = torch.nn.Linear(C * W, 1).double()
    a = torch.randn(T, B, C * W, generator=g, dtype=torch.float64)
    z_mod = lin((a.permute(1, 0, 2) + hidden).mean(1)).view(B)
    assert _rel(R.tail_forward(a, xt, lin.weight, lin.bias), z_mod) <= TAU_VALUE
    assert _rel(R.tail_forward(a, xt, lin.weight, None), z_mod - lin.bias) <= TAU_VALUE
    dz = torch.randn(B, generator=g, dtype=torch.float64)
    dxt = torch.randn(T, B, C * W, generator=g, dtype=torch.float64)
    (g_mod,) = torch.autograd.grad([z_mod, xt], x4, [dz, dxt])            # the mean's row + the gradient through `xt`
    row = lin.weight.detach().view(-1) / T
    assert _rel(R.unpack_add_outer(dxt, dz, row, B, C, T, W), g_mod) <= TAU_VALUE
    assert torch.equal(R.unpack_add(dxt, dz.view(B, 1) * row.view(1, -1), B, C, T, W), R.unpack_add_outer(dxt, dz, row, B, C, T, W))


# ---- the case table -----------------------------------------------------------------------------------------------------------------

ADMIT = 1e-5     # the plain float32 chain's dgx error over max |dgx64| per (utterance, direction): beyond it a case is chaotic

CASES = [(k, row) for k in ("lstm", "gru") for row in R.case_table(k)]


@pytest.mark.parametrize("kind,row", CASES, ids=[R.case_id(k, r) for k, r in CASES])
def test_case_is_admitted(kind, row):
    """Every recurrent case of the GPU suite: the plain float32 chain follows float64 to ADMIT (so that a bound on the kernels
    means something), and the saturating cases do reach the regions they are there for."""
    case = R.make_case(kind, row)
    scaling, T, B, D = row
    fwd64, g64 = R.autograd_dgx(kind, case, torch.float64)
    _, g32 = R.autograd_dgx(kind, case, torch.float32)
    assert torch.isfinite(g64).all() and torch.isfinite(g32).all()
    assert R.per_row_err(g32, g64) <= ADMIT
    assert case["w_hh"].abs().max().item() <= 4.0 / (R.LSTM_H if kind == "lstm" else R.GRU_H) ** 0.5
    if scaling == "sat":
        H = R.LSTM_H if kind == "lstm" else R.GRU_H
        gx = case["gx"]
        # |h| <= 1: the recurrent term moves a pre-activation by at most sum_k |w_hh[j][k]| + |b_hh| < H / sqrt(H) + 1 = 9.9
        assert (gx.abs() >= 30).float().mean().item() >= 0.04 and (gx <= -100).any() and (gx >= 100).any()
        acts = fwd64[1][..., :3 * H]
        assert (acts.float() == 1.0).any() and (acts.float().abs() < 1e-30).any()     # saturated after rounding to float32
        if kind == "lstm" and T >= 404:
            assert fwd64[2].abs().max().item() >= 10.0         # many steps of f = 1: 1 - tanh(c)^2 rounds to 0 in float32
