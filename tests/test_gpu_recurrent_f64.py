"""The recurrent kernels (csrc/lcnn_lstm.hip: LSTM forward, three backward entry points, four tail kernels; csrc/specrnet_gru.hip:
GRU forward and backward) against the float64 references of tests/recurrent_ref.py, element by element and stage by stage: the
C ABI is called with a given gx, no projection GEMM sits between a kernel and its check.

  * forward: out, gates, cell (LSTM) / out and the four quarters of saved (GRU) against the float64 recurrence;
  * backward, stage: dgx against the closed form evaluated in float64 on the forward KERNEL's own float32 state;
  * backward, end to end: dgx against float64 autograd through the float64 forward;
  * the same figures for the plain float32 chain (the references run in float32 on the CPU): the kernel's error must stay within
    a stated ratio of the chain's error on the same case, plus FLOOR;
  * every output is a view inside a NaN-filled allocation (nothing outside it is written, no NaN survives inside), every stage
    runs twice (no atomics: the same bits), the argument checks return before any launch.
Gradients are normalised per (utterance, direction) by max |reference|; values by max(1, max |reference|) (gates and outputs are
bounded by 1, cell states and a_n are not; the LSTM's by its cell scale, see forward_err).  The cases (tests/recurrent_ref.py: default scale, 4x, saturating gx; T 1 .. 404,
B 1 .. 257, D 1 and 2) are admitted by tests/test_recurrent_ref.py: on each the float32 chain follows float64 to 1e-5.

unpack_add_outer: csrc is built with -ffp-contract=off, so dz[b] * row[k] is rounded before the add (no fma) and the result is
compared bit for bit with the float32 torch expression."""
import math

import pytest
import torch

from tests import recurrent_ref as R

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64

# ---- bounds, calibrated on gfx950: each is at most 4x the worst figure measured over the case table (in brackets; every figure
# is written to parity_record under rnn_f64_*), and all are tighter than the 2e-6 / 3e-6 (outputs) and 2e-5 / 3e-5 (gradients)
# of tests/test_gpu_lcnn_ops.py::test_lstm_layer_matches_torch_lstm / test_gru_layer_matches_torch_gru -------------------------------
FLOOR = 2.0 ** -23            # one ulp of float32 at the normalising scale: two correctly rounded float32 results differ by it
TAU_FWD = {                   # forward values (see forward_err for the scale), worst of out / gates / cell or out / saved
    ("lstm", "default"): 1.5e-6,   # [3.9e-7; plain float32 chain 2.3e-7]
    ("lstm", "x4"): 1.5e-6,        # [3.8e-7; chain 3.5e-7]
    ("lstm", "sat"): 1.9e-6,       # [8.6e-7; chain 6.7e-7]
    ("gru", "default"): 1.1e-6,    # [3.0e-7; chain 4.2e-7]
    ("gru", "x4"): 2.9e-6,         # [1.13e-6; chain 1.88e-6]
    ("gru", "sat"): 1.0e-6}        # [2.6e-7; chain 4.1e-7]
TAU_STAGE = {                 # dgx against the closed form on the kernel's own state, per (utterance, direction)
    ("lstm", "default"): 1.1e-6,   # [2.8e-7; the closed form in float32 2.4e-7]
    ("lstm", "x4"): 1.2e-6,        # [3.2e-7; 5.3e-7]
    ("lstm", "sat"): 2.4e-6,       # [6.2e-7; 5.2e-7]
    ("gru", "default"): 8.5e-7,    # [2.2e-7; 2.1e-7]
    ("gru", "x4"): 1.1e-6,         # [2.9e-7; 5.5e-7]
    ("gru", "sat"): 7.5e-7}        # [2.0e-7; 1.9e-7]
TAU_E2E = {                   # dgx against float64 autograd end to end, per (utterance, direction)
    ("lstm", "default"): 2.0e-6,   # [5.0e-7; plain float32 chain 3.2e-7]
    ("lstm", "x4"): 4.0e-6,        # [1.05e-6; chain 8.4e-7]
    ("lstm", "sat"): 6.5e-6,       # [1.66e-6; chain 1.36e-6]
    ("gru", "default"): 2.4e-6,    # [6.1e-7; chain 2.8e-7]
    ("gru", "x4"): 4.4e-6,         # [1.11e-6; chain 1.06e-6]
    ("gru", "sat"): 2.8e-6}        # [7.2e-7; chain 2.2e-7]
# (error - FLOOR) / the plain float32 chain's error on the same case.  Over a group of cases the kernels and the chain are level
# (the figures above); case by case the quotient scatters, and its largest values are where the chain's own error is below
# 2 ulp.  The one systematic term: the kernels form tanh(v) as 2 / (1 + expf(-2v)) - 1, which is good to an ABSOLUTE ulp(1) = 1.2e-7
# (libm's tanhf: relative), so a saturated n or g carries up to twice the chain's error into 1 - n*n.  That is the end-to-end
# 4.7 of gru-x4-T1-B2-D2 (a single step, |pre-activation| up to 17: 1.0e-6 against the chain's 1.9e-7) and 4.0 of
# gru-sat-T2-B2-D2; on the kernel's own saved n (the stage figures) the backward kernels are at the closed form's level.
RATIO_FWD = 6.0               # forward values, per tensor  [2.2: lstm-default-T404-B1-D1, 2.3e-7 against 1.2e-7]
RATIO_STAGE = 4.0             # dgx from the same saved state  [1.5: lstm-sat]
RATIO_E2E = 10.0              # dgx end to end  [4.7, see above; LSTM 2.8]
TAU_TAIL_FWD = 7e-7           # z over sum_k |w_k| mean_t |a + xt| + |bias|  [1.84e-7]
RATIO_TAIL_FWD = 3.0          # [0.83]
TAU_TAIL_LOGIT = 5e-7         # lcnn_tail end to end: logits over max(1, max |z64|)  [1.3e-7; float32 modules 1.4e-7]
TAU_TAIL_GRAD = 1.9e-6        # ... dx4 per utterance over max |dx4_64[b]|  [4.8e-7; float32 modules 2.7e-7]
RATIO_TAIL = 5.0              # [logits 0.08, gradient 1.5]


def _abi():
    from audio_deepfake_adversarial_attacks_amd import _lib
    return _lib, _lib.load(), torch.cuda.current_stream().cuda_stream


PAD = 1_000       # floats on either side of a carved view: 4000 bytes, the view stays 16-byte aligned


def carve(shape, cuda):
    """A contiguous view of `shape` inside a larger NaN-filled buffer."""
    n = math.prod(shape)
    buf = torch.full((n + 2 * PAD,), float("nan"), device=cuda)
    return buf, buf[PAD:PAD + n].view(shape)


def intact(buf, view):
    """Nothing outside the view was written and no NaN survives inside it."""
    n = view.numel()
    return bool(torch.isnan(buf[:PAD]).all() and torch.isnan(buf[PAD + n:]).all() and not torch.isnan(view).any())


def untouched(buf):
    return bool(torch.isnan(buf).all())


def ratio(err, plain):
    over = max(err - FLOOR, 0.0)
    return over / plain if plain > 0 else (0.0 if over == 0 else math.inf)


# ---- running the stages (each twice: the same bits) ---------------------------------------------------------------------------------

def lstm_fwd(cuda, gx, w_hh):
    _lib, lib, st = _abi()
    T, B, D, H4 = gx.shape
    H = H4 // 4
    runs = []
    for _ in range(2):
        bufs = [carve(s, cuda) for s in ((T, B, D * H), (T, B, D, H4), (T, B, D, H))]
        _lib.check(lib.advstep_lstm_forward_f32(gx.data_ptr(), w_hh.data_ptr(), *(v.data_ptr() for _, v in bufs), T, B, D, H, st),
                   "lstm_forward")
        torch.cuda.synchronize()
        assert all(intact(b, v) for b, v in bufs)
        runs.append([v for _, v in bufs])
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    return runs[0]


def lstm_bwd(cuda, entry, grads, w_hh, gates, cell):
    """entry: "full" (dout), "bcast" (dout_row) or "outer" (dz, row)."""
    _lib, lib, st = _abi()
    T, B, D, H4 = gates.shape
    fn = {"full": lib.advstep_lstm_backward_f32, "bcast": lib.advstep_lstm_backward_bcast_f32,
          "outer": lib.advstep_lstm_backward_outer_f32}[entry]
    runs = []
    for _ in range(2):
        buf, dgx = carve((T, B, D, H4), cuda)
        _lib.check(fn(*(g.data_ptr() for g in grads), w_hh.data_ptr(), gates.data_ptr(), cell.data_ptr(), dgx.data_ptr(), T, B, D,
                      H4 // 4, st), "lstm_backward_" + entry)
        torch.cuda.synchronize()
        assert intact(buf, dgx)
        runs.append(dgx)
    assert torch.equal(*runs)
    return runs[0]


def gru_fwd(cuda, gx, w_hh, b_hh):
    _lib, lib, st = _abi()
    T, B, D, H3 = gx.shape
    H = H3 // 3
    runs = []
    for _ in range(2):
        bufs = [carve(s, cuda) for s in ((T, B, D * H), (T, B, D, 4 * H))]
        _lib.check(lib.advstep_gru_forward_f32(gx.data_ptr(), w_hh.data_ptr(), b_hh.data_ptr(), *(v.data_ptr() for _, v in bufs),
                                               T, B, D, H, st), "gru_forward")
        torch.cuda.synchronize()
        assert all(intact(b, v) for b, v in bufs)
        runs.append([v for _, v in bufs])
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    return runs[0]


def gru_bwd(cuda, dout, w_hh, saved, out):
    _lib, lib, st = _abi()
    T, B, D, H4 = saved.shape
    H = H4 // 4
    runs = []
    for _ in range(2):
        buf, dgx = carve((T, B, D, 3 * H), cuda)
        _lib.check(lib.advstep_gru_backward_f32(dout.data_ptr(), w_hh.data_ptr(), saved.data_ptr(), out.data_ptr(), dgx.data_ptr(),
                                                T, B, D, H, st), "gru_backward")
        torch.cuda.synchronize()
        assert intact(buf, dgx)
        runs.append(dgx)
    assert torch.equal(*runs)
    return runs[0]


def run_kernels(kind, cuda, case):
    """-> (forward tensors on the CPU as the references order them, dgx on the CPU)."""
    dev = {k: v.to(cuda) for k, v in case.items()}
    if kind == "lstm":
        out, gates, cell = lstm_fwd(cuda, dev["gx"], dev["w_hh"])
        dgx = lstm_bwd(cuda, "full", (dev["dout"],), dev["w_hh"], gates, cell)
        return (out.cpu(), gates.cpu(), cell.cpu()), dgx.cpu()
    out, saved = gru_fwd(cuda, dev["gx"], dev["w_hh"], dev["b_hh"])
    dgx = gru_bwd(cuda, dev["dout"], dev["w_hh"], saved, out)
    return (out.cpu(), saved.cpu()), dgx.cpu()


def closed_form(kind, case, fwd, dtype):
    """The stage reference on a given saved state."""
    if kind == "lstm":
        return R.lstm_backward(case["dout"], case["w_hh"], fwd[1], fwd[2], dtype)
    return R.gru_backward(case["dout"], case["w_hh"], fwd[1], fwd[0], dtype)


def forward_err(kind, fwd, fwd64, D):
    """{tensor name: worst error per (utterance, direction)} of the forward tensors, each (T, B, D, .).  GRU: over
    max(1, max |ref|) of the tensor (r, z, n, h are bounded by 1, a_n is not).  LSTM: all three over max(1, max |cell64|) of the
    (utterance, direction): the cell is a float32 accumulator, so its ABSOLUTE error is a few ulp of the largest value it has
    held, and h = o tanh(c) hands that on unattenuated wherever the same unit's c later passes near 0 (slope 1).  With
    max |c| <= 2.5 (default, x4) this is the absolute error to within that factor; on the saturating T = 404 cases
    (max |c| = 16 .. 18, ulp 1.9e-6) the plain float32 chain itself is off by 0.7e-6 .. 1.6e-6 absolute in `out`."""
    names = ("out", "gates", "cell") if kind == "lstm" else ("out", "saved")
    scale = R.row_scale(fwd64[2], 1.0) if kind == "lstm" else None
    errs = {}
    for name, x, ref in zip(names, fwd, fwd64):
        if x.dim() == 3:
            x, ref = R.by_direction(x, D), R.by_direction(ref, D)
        errs[name] = R.per_row_err(x, ref, floor_scale=1.0, scale=scale)
    return errs


# ---- the case table -------------------------------------------------------------------------------------------------------------------

CASES = [(k, row) for k in ("lstm", "gru") for row in R.case_table(k)]


@pytest.mark.parametrize("kind,row", CASES, ids=[R.case_id(k, r) for k, r in CASES])
def test_recurrent_stages_match_float64(cuda, parity_record, kind, row):
    scaling, T, B, D = row
    case = R.make_case(kind, row)
    fwd64, g64 = R.autograd_dgx(kind, case, F64)
    fwd32, g32 = R.autograd_dgx(kind, case, F32)
    fwd, dgx = run_kernels(kind, cuda, case)
    assert all(a.shape == b.shape for a, b in zip(fwd, fwd64)) and dgx.shape == g64.shape
    stage64 = closed_form(kind, case, fwd, F64)
    stage32 = closed_form(kind, case, fwd, F32)
    e_fwd, p_fwd = forward_err(kind, fwd, fwd64, D), forward_err(kind, fwd32, fwd64, D)
    rec = {"fwd": max(e_fwd.values()), "plain_fwd": max(p_fwd.values()), "fwd_each": e_fwd, "plain_fwd_each": p_fwd,
           "stage": R.per_row_err(dgx, stage64), "plain_stage": R.per_row_err(stage32, stage64),
           "e2e": R.per_row_err(dgx, g64), "plain_e2e": R.per_row_err(g32, g64)}
    for q in ("fwd", "stage", "e2e"):
        rec["ratio_" + q] = ratio(rec[q], rec["plain_" + q])
    rec["ratio_fwd"] = max(ratio(e_fwd[n], p_fwd[n]) for n in e_fwd)
    parity_record[f"rnn_f64_{R.case_id(kind, row)}"] = rec
    print(R.case_id(kind, row), rec)
    key = (kind, scaling)
    assert rec["fwd"] <= TAU_FWD[key] and all(e_fwd[n] <= FLOOR + RATIO_FWD * p_fwd[n] for n in e_fwd), rec
    assert rec["stage"] <= TAU_STAGE[key] and rec["stage"] <= FLOOR + RATIO_STAGE * rec["plain_stage"], rec
    assert rec["e2e"] <= TAU_E2E[key] and rec["e2e"] <= FLOOR + RATIO_E2E * rec["plain_e2e"], rec


@pytest.mark.parametrize("kind", ["lstm", "gru"])
@pytest.mark.parametrize("T,B,D,t0,b0,d0,u0", [(25, 3, 2, 11, 1, 1, 7), (25, 3, 2, 24, 2, 0, 79), (3, 2, 2, 1, 0, 1, 0),
                                                (2, 2, 1, 0, 1, 0, 33), (404, 2, 2, 200, 1, 1, 63), (1, 1, 1, 0, 0, 0, 5)])
def test_single_element_gradient_lands_where_it_belongs(cuda, parity_record, kind, T, B, D, t0, b0, d0, u0):
    """dout zero but for one (t, b, unit): a mis-indexed step or direction is a misplaced nonzero, not a small error.  Every
    (t, b, d) row the closed form leaves exactly zero (another utterance, the other direction, the steps after t0 in that
    direction's order) must be exactly zero; the rest matches it element by element."""
    H = R.LSTM_H if kind == "lstm" else R.GRU_H
    u0 = u0 % H
    case = R.make_case(kind, ("default", T, B, D))
    case["dout"] = torch.zeros_like(case["dout"])
    case["dout"][t0, b0, d0 * H + u0] = 1.5
    fwd, dgx = run_kernels(kind, cuda, case)
    ref = closed_form(kind, case, fwd, F64)
    zero_rows = ref.abs().amax(-1) == 0
    live = [t for t in range(T) if (t <= t0 if d0 == 0 else t >= t0)]
    assert int((~zero_rows).sum()) == len(live) and not zero_rows[live, b0, d0].any()      # the reference's own support
    assert (dgx[zero_rows] == 0).all()
    err = R.per_row_err(dgx, ref)
    parity_record[f"rnn_f64_{kind}_onehot_T{T}_B{B}_D{D}_t{t0}"] = err
    assert err <= TAU_STAGE[(kind, "default")], err


@pytest.mark.parametrize("T,B,D", [(25, 6, 2), (1, 2, 1), (2, 3, 2), (3, 1, 1), (404, 2, 1), (25, 257, 2)])
def test_lstm_backward_bcast_and_outer(cuda, parity_record, T, B, D):
    """advstep_lstm_backward_bcast_f32 (zero frame stride) and advstep_lstm_backward_outer_f32 (both strides zero, one factor per
    utterance): the same kernel as advstep_lstm_backward_f32 with other strides, so bit-identical to it on the expanded float32
    gradient, and against the float64 closed form of the expanded gradient on the kernel's own state."""
    case = R.make_case("lstm", ("default", T, B, D))
    g = torch.Generator().manual_seed(T * 1_000 + B)
    dz, row = torch.randn(B, generator=g), torch.randn(D * R.LSTM_H, generator=g) / T
    dev = {k: v.to(cuda) for k, v in case.items()}
    out, gates, cell = lstm_fwd(cuda, dev["gx"], dev["w_hh"])
    dzc, rowc = dz.to(cuda), row.to(cuda)
    dout_row = (dzc.view(B, 1) * rowc.view(1, -1)).contiguous()              # the float32 product, formed as the kernel forms it
    full = dout_row.unsqueeze(0).expand(T, -1, -1).contiguous()
    want = lstm_bwd(cuda, "full", (full,), dev["w_hh"], gates, cell)
    got_b = lstm_bwd(cuda, "bcast", (dout_row,), dev["w_hh"], gates, cell)
    got_o = lstm_bwd(cuda, "outer", (dzc, rowc), dev["w_hh"], gates, cell)
    assert torch.equal(got_b, want) and torch.equal(got_o, want)
    gates_c, cell_c = gates.cpu(), cell.cpu()
    ref_b = R.lstm_backward_bcast(dout_row.cpu(), case["w_hh"], gates_c, cell_c)
    ref_o = R.lstm_backward_outer(dz, row, case["w_hh"], gates_c, cell_c)
    e_b, e_o = R.per_row_err(got_b.cpu(), ref_b), R.per_row_err(got_o.cpu(), ref_o)
    parity_record[f"rnn_f64_lstm_bcast_T{T}_B{B}_D{D}"] = e_b
    parity_record[f"rnn_f64_lstm_outer_T{T}_B{B}_D{D}"] = e_o
    # the outer form's reference multiplies in float64: one more float32 rounding of dout (FLOOR x 2) on the kernel's side
    assert e_b <= TAU_STAGE[("lstm", "default")] and e_o <= TAU_STAGE[("lstm", "default")], (e_b, e_o)


# ---- the tail kernels -------------------------------------------------------------------------------------------------------------------

# (B, C, T, W): LCNN's own; one above 4096 x 256 = 1 048 576 elements (the grid-stride loop's second trip); odd sizes; a size-1
# axis in each position
PACK_SHAPES = [(128, 32, 25, 5), (300, 32, 25, 5), (3, 5, 7, 9), (1, 5, 7, 9), (3, 1, 7, 9), (3, 5, 1, 9), (3, 5, 7, 1),
               (1, 1, 1, 1), (257, 3, 11, 13)]


@pytest.mark.parametrize("B,C,T,W", PACK_SHAPES)
def test_tail_pack_and_unpack_add_are_bit_exact(cuda, B, C, T, W):
    """pack, unpack_add and unpack_add_outer are copies and one add (the outer form's product is rounded first: no fma, see the
    module docstring): bit for bit the float32 torch expression."""
    _lib, lib, st = _abi()
    g = torch.Generator().manual_seed(B * 7 + C * 5 + T * 3 + W)
    x4 = torch.randn(B, C, T, W, generator=g)
    dxt = torch.randn(T, B, C * W, generator=g)
    g0 = torch.randn(B, C * W, generator=g)
    dz, row = torch.randn(B, generator=g), torch.randn(C * W, generator=g)
    x4c, dxtc, g0c, dzc, rowc = (t.to(cuda) for t in (x4, dxt, g0, dz, row))
    results = []
    for _ in range(2):
        pb, xt = carve((T, B, C * W), cuda)
        ub, dx4 = carve((B, C, T, W), cuda)
        ob, dx4o = carve((B, C, T, W), cuda)
        _lib.check(lib.advstep_lcnn_tail_pack_f32(x4c.data_ptr(), xt.data_ptr(), B, C, T, W, st), "pack")
        _lib.check(lib.advstep_lcnn_tail_unpack_add_f32(dxtc.data_ptr(), g0c.data_ptr(), dx4.data_ptr(), B, C, T, W, st), "unpack_add")
        _lib.check(lib.advstep_lcnn_tail_unpack_add_outer_f32(dxtc.data_ptr(), dzc.data_ptr(), rowc.data_ptr(), dx4o.data_ptr(), B, C,
                                                              T, W, st), "unpack_add_outer")
        torch.cuda.synchronize()
        assert intact(pb, xt) and intact(ub, dx4) and intact(ob, dx4o)
        results.append((xt.cpu(), dx4.cpu(), dx4o.cpu()))
    assert all(torch.equal(a, b) for a, b in zip(*results))
    xt, dx4, dx4o = results[0]
    assert torch.equal(xt, R.pack(x4, F32))
    assert torch.equal(dx4, R.unpack_add(dxt, g0, B, C, T, W, F32))
    assert torch.equal(dx4o, R.unpack_add_outer(dxt, dz, row, B, C, T, W, F32))
    # and the float64 statement of the same (exact but for the one add)
    assert (dx4.double() - R.unpack_add(dxt, g0, B, C, T, W)).abs().max().item() <= 2.0 ** -24 * 16


@pytest.mark.parametrize("B", [1, 257])
@pytest.mark.parametrize("with_bias", [True, False])
def test_tail_forward_matches_float64(cuda, parity_record, B, with_bias):
    """skip + mean over frames + one-row Linear for every F the header promises (<= 256: around the wave boundaries 64 and 256)
    and T around the 8-frame batches of the loop, bias and no bias."""
    _lib, lib, st = _abi()
    worst, worst_ratio = 0.0, 0.0
    for F in (1, 63, 64, 65, 160, 255, 256):
        for T in (1, 7, 8, 9, 25, 404):
            g = torch.Generator().manual_seed(F * 1_000 + T + B)
            a = torch.randn(T, B, F, generator=g)
            xt = torch.randn(T, B, F, generator=g)
            w = (2 * torch.rand(F, generator=g) - 1) / math.sqrt(F)
            bias = torch.randn(1, generator=g) if with_bias else None
            ac, xc, wc = a.to(cuda), xt.to(cuda), w.to(cuda)
            bc = bias.to(cuda) if with_bias else None
            runs = []
            for _ in range(2):
                zb, z = carve((B,), cuda)
                _lib.check(lib.advstep_lcnn_tail_forward_f32(ac.data_ptr(), xc.data_ptr(), wc.data_ptr(),
                                                             bc.data_ptr() if with_bias else None, z.data_ptr(), T, B, F, st),
                           "tail_forward")
                torch.cuda.synchronize()
                assert intact(zb, z)
                runs.append(z.cpu())
            assert torch.equal(*runs)
            z64 = R.tail_forward(a, xt, w, bias)
            scale = (a.double() + xt.double()).abs().mean(0) @ w.double().abs() + (abs(bias.item()) if with_bias else 0.0)
            err = ((runs[0].double() - z64).abs() / scale).max().item()
            plain = ((R.tail_forward(a, xt, w, bias, F32).double() - z64).abs() / scale).max().item()
            worst, worst_ratio = max(worst, err), max(worst_ratio, ratio(err, plain))
            assert err <= TAU_TAIL_FWD and err <= FLOOR + RATIO_TAIL_FWD * plain, (F, T, err, plain)
    parity_record[f"rnn_f64_tail_forward_B{B}_bias{int(with_bias)}"] = {"err": worst, "ratio": worst_ratio}
    print("tail_forward", B, with_bias, worst, worst_ratio)


# ---- lcnn_tail end to end ----------------------------------------------------------------------------------------------------------------

def _tail_modules(seed):
    """Two BLSTM layers and the Linear of LCNN's tail in float32 (default init; bias_hh zeroed so that the b_ih + b_hh the
    kernels are handed is exact in float32)."""
    torch.manual_seed(seed)
    F, H = 2 * R.LSTM_H, R.LSTM_H
    mods = [torch.nn.LSTM(F, H, bidirectional=True), torch.nn.LSTM(F, H, bidirectional=True), torch.nn.Linear(F, 1)]
    with torch.no_grad():
        for m in mods[:2]:
            m.bias_hh_l0.zero_(), m.bias_hh_l0_reverse.zero_()
    return mods


def _packed(m, cuda):
    w_ih = torch.cat([m.weight_ih_l0, m.weight_ih_l0_reverse]).detach().to(cuda).contiguous()
    w_hh = torch.stack([m.weight_hh_l0, m.weight_hh_l0_reverse]).detach().to(cuda).contiguous()
    bias = torch.cat([m.bias_ih_l0 + m.bias_hh_l0, m.bias_ih_l0_reverse + m.bias_hh_l0_reverse]).detach().to(cuda).contiguous()
    return w_ih, w_hh, bias


def _tail_reference(mods, w_out, b_out, x4, coef, dtype):
    """torch.nn.LSTM x 2 + skip + mean + Linear (src/models/lcnn.py:196-205) in `dtype` on the CPU: logits (B), dx4."""
    import copy
    l1, l2 = (copy.deepcopy(m).to(dtype) for m in mods[:2])
    a = x4.to(dtype).clone().requires_grad_(True)
    B, C, T, W = a.shape
    hidden = a.permute(0, 2, 1, 3).contiguous().view(B, T, C * W)
    seq = hidden.permute(1, 0, 2)
    y = l2(l1(seq)[0])[0]
    z = (y + seq).mean(0) @ w_out.to(dtype).view(-1)
    if b_out is not None:
        z = z + b_out.to(dtype).view(())
    (g,) = torch.autograd.grad((z * coef.to(dtype)).sum(), a)
    return z.detach(), g


def _tail_check(L, mods, packed, w_out, b_out, x4, coef, cuda):
    a = x4.to(cuda).requires_grad_(True)
    z = L.lcnn_tail(a, packed[0], packed[1], w_out, b_out)
    (g,) = torch.autograd.grad((z.view(-1) * coef.to(cuda)).sum(), a)
    w_cpu, b_cpu = w_out.detach().cpu(), None if b_out is None else b_out.detach().cpu()
    z64, g64 = _tail_reference(mods, w_cpu, b_cpu, x4, coef, F64)
    z32, g32 = _tail_reference(mods, w_cpu, b_cpu, x4, coef, F32)
    zscale = z64.abs().max().clamp(min=1.0)

    def gerr(x):
        return ((x.double().cpu() - g64).abs().flatten(1).amax(1) / g64.abs().flatten(1).amax(1)).max().item()
    return {"logit": ((z.detach().view(-1).double().cpu() - z64).abs().max() / zscale).item(),
            "plain_logit": ((z32.double() - z64).abs().max() / zscale).item(), "grad": gerr(g), "plain_grad": gerr(g32)}


@pytest.mark.parametrize("B,bias", [(1, True), (6, True), (6, False), (257, True)])
def test_lcnn_tail_matches_float64_modules(cuda, parity_record, B, bias):
    """lcnn_ops.lcnn_tail (pack, two projection GEMMs + recurrent kernels, tail forward; backward_outer, backward, unpack_add_outer)
    against float64 torch.nn.LSTM x 2 + skip + mean + Linear with the weights copied, non-uniform dz; then the Linear's weight
    changed IN PLACE (a version bump) and T changed between calls: the cached w / T of _LcnnTail must follow both."""
    from audio_deepfake_adversarial_attacks_amd import lcnn_ops as L
    mods = _tail_modules(B)
    packed = [_packed(m, cuda) for m in mods[:2]]
    w_out = mods[2].weight.detach().clone().to(cuda)                   # ONE tensor object for every call: what the cache is keyed on
    b_out = mods[2].bias.detach().clone().to(cuda) if bias else None
    g = torch.Generator().manual_seed(100 + B)
    coef = torch.randn(B, generator=g) + torch.arange(1, B + 1) / B
    steps = [("first", 25, None), ("weight-changed", 25, -1.7), ("T-changed", 9, None), ("T-back", 25, None)]
    for tag, T, factor in steps:
        if factor is not None:
            w_out.mul_(factor)
        x4 = torch.randn(B, 32, T, 5, generator=g)
        rec = _tail_check(L, mods, packed, w_out, b_out, x4, coef, cuda)
        rec["ratio_logit"], rec["ratio_grad"] = ratio(rec["logit"], rec["plain_logit"]), ratio(rec["grad"], rec["plain_grad"])
        parity_record[f"rnn_f64_lcnn_tail_B{B}_bias{int(bias)}_{tag}"] = rec
        print("lcnn_tail", B, bias, tag, rec)
        assert rec["logit"] <= TAU_TAIL_LOGIT and rec["logit"] <= FLOOR + RATIO_TAIL * rec["plain_logit"], (tag, rec)
        assert rec["grad"] <= TAU_TAIL_GRAD and rec["grad"] <= FLOOR + RATIO_TAIL * rec["plain_grad"], (tag, rec)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------

def test_argument_checks_return_before_any_launch(cuda):
    """Unsupported H, D = 3, a null pointer, tail_forward with F = 257 or T = 0, the GRU's B = 65 536, negative sizes: the
    invalid-argument status, nothing launched, the NaN-filled outputs untouched.  Empty T or B: OK, nothing written."""
    _lib, lib, st = _abi()
    assert lib.advstep_lstm_supported(80) == 1 and lib.advstep_lstm_supported(81) == 0 and lib.advstep_lstm_supported(64) == 0
    assert lib.advstep_gru_supported(64) == 1 and lib.advstep_gru_supported(65) == 0 and lib.advstep_gru_supported(80) == 0
    T, B, D = 2, 2, 2
    src = torch.randn(T * B * 3 * 4 * 81, device=cuda)            # readable input of ample size for every call below
    outs = [torch.full((T * B * 3 * 4 * 81,), float("nan"), device=cuda) for _ in range(3)]
    s, (o0, o1, o2) = src.data_ptr(), (o.data_ptr() for o in outs)
    EINVAL, OK = _lib.EINVAL, _lib.OK
    refused = [
        lib.advstep_lstm_forward_f32(s, s, o0, o1, o2, T, B, D, 81, st),
        lib.advstep_lstm_forward_f32(s, s, o0, o1, o2, T, B, 3, 80, st),
        lib.advstep_lstm_forward_f32(s, s, o0, o1, o2, T, B, 0, 80, st),
        lib.advstep_lstm_forward_f32(None, s, o0, o1, o2, T, B, D, 80, st),
        lib.advstep_lstm_forward_f32(s, s, o0, None, o2, T, B, D, 80, st),
        lib.advstep_lstm_forward_f32(s, s, o0, o1, o2, -1, B, D, 80, st),
        lib.advstep_lstm_backward_f32(s, s, s, s, o0, T, B, D, 81, st),
        lib.advstep_lstm_backward_f32(s, s, s, s, o0, T, B, 3, 80, st),
        lib.advstep_lstm_backward_f32(None, s, s, s, o0, T, B, D, 80, st),
        lib.advstep_lstm_backward_f32(s, s, s, s, None, T, B, D, 80, st),
        lib.advstep_lstm_backward_bcast_f32(s, s, s, s, o0, T, B, D, 81, st),
        lib.advstep_lstm_backward_bcast_f32(s, s, s, s, o0, T, B, 3, 80, st),
        lib.advstep_lstm_backward_bcast_f32(s, None, s, s, o0, T, B, D, 80, st),
        lib.advstep_lstm_backward_outer_f32(s, s, s, s, s, o0, T, B, D, 81, st),
        lib.advstep_lstm_backward_outer_f32(s, s, s, s, s, o0, T, B, 3, 80, st),
        lib.advstep_lstm_backward_outer_f32(None, s, s, s, s, o0, T, B, D, 80, st),
        lib.advstep_lstm_backward_outer_f32(s, None, s, s, s, o0, T, B, D, 80, st),
        lib.advstep_gru_forward_f32(s, s, s, o0, o1, T, B, D, 65, st),
        lib.advstep_gru_forward_f32(s, s, s, o0, o1, T, B, 3, 64, st),
        lib.advstep_gru_forward_f32(s, s, None, o0, o1, T, B, D, 64, st),
        lib.advstep_gru_forward_f32(s, s, s, o0, o1, T, 65_536, D, 64, st),
        lib.advstep_gru_backward_f32(s, s, s, s, o0, T, B, D, 65, st),
        lib.advstep_gru_backward_f32(s, s, s, s, o0, T, B, 3, 64, st),
        lib.advstep_gru_backward_f32(s, s, s, None, o0, T, B, D, 64, st),
        lib.advstep_gru_backward_f32(s, s, s, s, o0, T, 65_536, D, 64, st),
        lib.advstep_lcnn_tail_forward_f32(s, s, s, s, o0, T, B, 257, st),
        lib.advstep_lcnn_tail_forward_f32(s, s, s, s, o0, 0, B, 160, st),
        lib.advstep_lcnn_tail_forward_f32(s, s, s, s, o0, T, B, 0, st),
        lib.advstep_lcnn_tail_forward_f32(s, None, s, s, o0, T, B, 160, st),
        lib.advstep_lcnn_tail_pack_f32(None, o0, 2, 3, 4, 5, st),
        lib.advstep_lcnn_tail_pack_f32(s, o0, 2, -3, 4, 5, st),
        lib.advstep_lcnn_tail_unpack_add_f32(s, None, o0, 2, 3, 4, 5, st),
        lib.advstep_lcnn_tail_unpack_add_f32(s, s, o0, 2, 3, 4, -5, st),
        lib.advstep_lcnn_tail_unpack_add_outer_f32(s, s, None, o0, 2, 3, 4, 5, st),
        lib.advstep_lcnn_tail_unpack_add_outer_f32(s, s, s, None, 2, 3, 4, 5, st),
    ]
    assert refused == [EINVAL] * len(refused), refused
    empty = [
        lib.advstep_lstm_forward_f32(s, s, o0, o1, o2, 0, B, D, 80, st),
        lib.advstep_lstm_forward_f32(s, s, o0, o1, o2, T, 0, D, 80, st),
        lib.advstep_lstm_backward_f32(s, s, s, s, o0, 0, B, D, 80, st),
        lib.advstep_lstm_backward_bcast_f32(s, s, s, s, o0, T, 0, D, 80, st),
        lib.advstep_lstm_backward_outer_f32(s, s, s, s, s, o0, 0, B, D, 80, st),
        lib.advstep_gru_forward_f32(s, s, s, o0, o1, 0, B, D, 64, st),
        lib.advstep_gru_backward_f32(s, s, s, s, o0, T, 0, D, 64, st),
        lib.advstep_lcnn_tail_forward_f32(s, s, s, s, o0, T, 0, 160, st),
        lib.advstep_lcnn_tail_pack_f32(s, o0, 2, 0, 4, 5, st),
        lib.advstep_lcnn_tail_unpack_add_f32(s, s, o0, 0, 3, 4, 5, st),
        lib.advstep_lcnn_tail_unpack_add_outer_f32(s, s, s, o0, 2, 3, 0, 5, st),
    ]
    assert empty == [OK] * len(empty), empty
    torch.cuda.synchronize()
    assert all(untouched(o) for o in outs)
