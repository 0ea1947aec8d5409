"""Plain references for the recurrent kernels (csrc/lcnn_lstm.hip, csrc/specrnet_gru.hip): what include/advstep_lcnn.h documents,
restated with explicit loops over the steps, in the dtype the caller names.  Importable without a GPU.

With dtype=torch.float64 these are the references of tests/test_gpu_recurrent_f64.py; with dtype=torch.float32 they are the
"plain float32 chain" whose own error against float64 the kernels' error is compared with.  Two kinds of backward:
  * `autograd_dgx`: float autograd through the forward (the end-to-end reference);
  * `lstm_backward` / `gru_backward`: the closed form evaluated from SAVED state handed to it (the stage reference): given the
    forward kernel's own float32 gates / cell / saved / out it judges a backward kernel isolated from forward error.
Layouts (sequence-first, D directions, direction 1 runs over time in reverse, zero initial state):
  LSTM  gx (T, B, D, 4H)  w_hh (D, 4H, H)  gate order i, f, g, o   out (T, B, D*H)  gates (T, B, D, 4H) activated  cell (T, B, D, H)
  GRU   gx (T, B, D, 3H)  w_hh (D, 3H, H)  b_hh (D, 3H)  gate order r, z, n   out (T, B, D*H)  saved (T, B, D, 4H) = r, z, n, a_n
tests/test_recurrent_ref.py pins all of it against torch.nn.LSTM / torch.nn.GRU in float64."""
import math

import torch

LSTM_H = 80      # LCNN's hidden size: the one advstep_lstm_supported() accepts
GRU_H = 64       # SpecRNet's: the one advstep_gru_supported() accepts


def _time_of(step, d, T):
    return step if d == 0 else T - 1 - step


# ---- LSTM -------------------------------------------------------------------------------------------------------------------------

def lstm_forward(gx, w_hh, dtype):
    """-> (out (T, B, D*H), gates (T, B, D, 4H), cell (T, B, D, H))."""
    gx, w_hh = gx.to(dtype), w_hh.to(dtype)
    T, B, D, H4 = gx.shape
    H = H4 // 4
    outs, gates, cells = [], [], []
    for d in range(D):
        h = torch.zeros(B, H, dtype=dtype)
        c = torch.zeros(B, H, dtype=dtype)
        o_d, g_d, c_d = [None] * T, [None] * T, [None] * T
        for step in range(T):
            t = _time_of(step, d, T)
            pre = gx[t, :, d] + h @ w_hh[d].t()
            i, f = torch.sigmoid(pre[:, :H]), torch.sigmoid(pre[:, H:2 * H])
            g, o = torch.tanh(pre[:, 2 * H:3 * H]), torch.sigmoid(pre[:, 3 * H:])
            c = f * c + i * g
            h = o * torch.tanh(c)
            o_d[t], g_d[t], c_d[t] = h, torch.cat([i, f, g, o], 1), c
        outs.append(torch.stack(o_d)), gates.append(torch.stack(g_d)), cells.append(torch.stack(c_d))
    if T == 0:
        return gx.new_zeros(0, B, D * H), gx.new_zeros(0, B, D, H4), gx.new_zeros(0, B, D, H)
    return torch.cat(outs, 2), torch.stack(gates, 2), torch.stack(cells, 2)


def lstm_backward(dout, w_hh, gates, cell, dtype=torch.float64):
    """dgx (T, B, D, 4H) from dout (T, B, D*H) and the saved activated gates and cell states, in closed form."""
    dout, w_hh, gates, cell = dout.to(dtype), w_hh.to(dtype), gates.to(dtype), cell.to(dtype)
    T, B, D, H4 = gates.shape
    H = H4 // 4
    dgx = torch.zeros(T, B, D, H4, dtype=dtype)
    for d in range(D):
        dh_rec = torch.zeros(B, H, dtype=dtype)
        dc_next = torch.zeros(B, H, dtype=dtype)
        for step in range(T - 1, -1, -1):
            t = _time_of(step, d, T)
            i, f, g, o = gates[t, :, d].split(H, 1)
            c = cell[t, :, d]
            c_prev = cell[_time_of(step - 1, d, T), :, d] if step > 0 else torch.zeros_like(c)
            tc = torch.tanh(c)
            dh = dout[t, :, d * H:(d + 1) * H] + dh_rec
            d_o = dh * tc * o * (1 - o)
            dc = dh * o * (1 - tc * tc) + dc_next
            d_i, d_f, d_g = dc * g * i * (1 - i), dc * c_prev * f * (1 - f), dc * i * (1 - g * g)
            dc_next = dc * f
            dg = torch.cat([d_i, d_f, d_g, d_o], 1)
            dgx[t, :, d] = dg
            dh_rec = dg @ w_hh[d]
    return dgx


def lstm_backward_bcast(dout_row, w_hh, gates, cell, dtype=torch.float64):
    """dout[t] = dout_row (B, D*H) for every frame."""
    return lstm_backward(dout_row.to(dtype).unsqueeze(0).expand(gates.shape[0], -1, -1), w_hh, gates, cell, dtype)


def lstm_backward_outer(dz, row, w_hh, gates, cell, dtype=torch.float64):
    """dout[t][b][f] = dz[b] * row[f]."""
    return lstm_backward_bcast(dz.to(dtype).reshape(-1, 1) * row.to(dtype).reshape(1, -1), w_hh, gates, cell, dtype)


# ---- GRU --------------------------------------------------------------------------------------------------------------------------

def gru_forward(gx, w_hh, b_hh, dtype):
    """-> (out (T, B, D*H), saved (T, B, D, 4H) = r, z, n, a_n = W_hn h + b_hn)."""
    gx, w_hh, b_hh = gx.to(dtype), w_hh.to(dtype), b_hh.to(dtype)
    T, B, D, H3 = gx.shape
    H = H3 // 3
    outs, saved = [], []
    for d in range(D):
        h = torch.zeros(B, H, dtype=dtype)
        o_d, s_d = [None] * T, [None] * T
        for step in range(T):
            t = _time_of(step, d, T)
            a = h @ w_hh[d].t() + b_hh[d]
            g = gx[t, :, d]
            r = torch.sigmoid(g[:, :H] + a[:, :H])
            z = torch.sigmoid(g[:, H:2 * H] + a[:, H:2 * H])
            a_n = a[:, 2 * H:]
            n = torch.tanh(g[:, 2 * H:] + r * a_n)
            h = (1 - z) * n + z * h
            o_d[t], s_d[t] = h, torch.cat([r, z, n, a_n], 1)
        outs.append(torch.stack(o_d)), saved.append(torch.stack(s_d))
    if T == 0:
        return gx.new_zeros(0, B, D * H), gx.new_zeros(0, B, D, 4 * H)
    return torch.cat(outs, 2), torch.stack(saved, 2)


def gru_backward(dout, w_hh, saved, out, dtype=torch.float64):
    """dgx (T, B, D, 3H) from dout (T, B, D*H), the saved r, z, n, a_n and the forward's own output (h_{t-1}), in closed form."""
    dout, w_hh, saved, out = dout.to(dtype), w_hh.to(dtype), saved.to(dtype), out.to(dtype)
    T, B, D, H4 = saved.shape
    H = H4 // 4
    dgx = torch.zeros(T, B, D, 3 * H, dtype=dtype)
    for d in range(D):
        dh_rec = torch.zeros(B, H, dtype=dtype)       # through W_hh and through z * h_{t-1}
        for step in range(T - 1, -1, -1):
            t = _time_of(step, d, T)
            r, z, n, a_n = saved[t, :, d].split(H, 1)
            h_prev = out[_time_of(step - 1, d, T), :, d * H:(d + 1) * H] if step > 0 else torch.zeros_like(r)
            dh = dout[t, :, d * H:(d + 1) * H] + dh_rec
            dn_pre = dh * (1 - z) * (1 - n * n)
            dz_pre = dh * (h_prev - n) * z * (1 - z)
            dr_pre = dn_pre * a_n * r * (1 - r)
            dgx[t, :, d] = torch.cat([dr_pre, dz_pre, dn_pre], 1)
            dh_rec = dh * z + torch.cat([dr_pre, dz_pre, dn_pre * r], 1) @ w_hh[d]
    return dgx


def autograd_dgx(kind, case, dtype):
    """(forward outputs detached, dgx) by autograd through the forward in `dtype`: the end-to-end reference (float64) or the
    plain float32 chain."""
    gx = case["gx"].to(dtype).clone().requires_grad_(True)
    if kind == "lstm":
        fwd = lstm_forward(gx, case["w_hh"], dtype)
    else:
        fwd = gru_forward(gx, case["w_hh"], case["b_hh"], dtype)
    if gx.numel() == 0:
        return tuple(f.detach() for f in fwd), torch.zeros_like(gx)
    (g,) = torch.autograd.grad(fwd[0], gx, case["dout"].to(dtype))
    return tuple(f.detach() for f in fwd), g


# ---- around the two BLSTM layers ----------------------------------------------------------------------------------------------------

def pack(x4, dtype=torch.float64):
    """x4 (B, C, T, W) -> xt (T, B, C*W)."""
    B, C, T, W = x4.shape
    return x4.to(dtype).permute(2, 0, 1, 3).reshape(T, B, C * W)


def tail_forward(a, xt, w, bias, dtype=torch.float64):
    """z (B) = bias + sum_k w[k] * mean_t(a[t][b][k] + xt[t][b][k])."""
    z = (a.to(dtype) + xt.to(dtype)).mean(0) @ w.to(dtype).reshape(-1)
    return z if bias is None else z + bias.to(dtype).reshape(())


def unpack_add(dxt, g0, B, C, T, W, dtype=torch.float64):
    """dx4 (B, C, T, W) = dxt (T, B, C*W) + g0 (B, C*W)."""
    return (dxt.to(dtype) + g0.to(dtype).unsqueeze(0)).reshape(T, B, C, W).permute(1, 2, 0, 3).contiguous()


def unpack_add_outer(dxt, dz, row, B, C, T, W, dtype=torch.float64):
    """unpack_add with g0[b][k] = dz[b] * row[k] (the product rounded to `dtype` before the add)."""
    return unpack_add(dxt, dz.to(dtype).reshape(B, 1) * row.to(dtype).reshape(1, C * W), B, C, T, W, dtype)


# ---- the case table ---------------------------------------------------------------------------------------------------------------
# Saturation comes from gx, never from w_hh: with w_hh at 16x the default-init scale the recurrences turn chaotic (float32
# against float64 gives 1e-5 .. 6e-5 of max |dgx| for the LSTM, 1e-3 and overflow for the GRU) and no bound means anything.
#   default  w_hh ~ U(-1/sqrt(H), 1/sqrt(H)) (torch's default init), gx ~ N(0, 1): pre-activations within a few units
#   x4       w_hh and gx four times that
#   sat      w_hh at default scale, gx ~ N(0, 1) with 6 % of its elements moved to +-(30 .. 40) (sigmoid and tanh saturated:
#            g (1 - g) and 1 - n*n round to 0) and 1 % to +-(100 .. 120) (expf overflows to inf on the negative side); for the
#            LSTM the forget gate of every 16th unit held at +35 for all steps (f = 1: the cell state keeps accumulating; with every
#            fourth unit held the float32 chain itself is off by 1.1e-5 of max |dgx| at T = 404: not admitted)

SCALINGS = ("default", "x4", "sat")

# (T, B, D): every T of {1, 2, 3, 25, 404}, B of {1, 2, 128, 257} and D of {1, 2}; T = 2, 3 are the LSTM backward's pipeline
# start-up; 404 is the longest frame axis of LCNN and SpecRNet; 50 what SpecRNet's GRU sees (404 frames pooled three times);
# B = 257 is more workgroups than compute units x directions hold at once
SHAPES_ALL = [(1, 1, 1), (1, 2, 2), (2, 1, 1), (2, 2, 2), (3, 2, 2), (3, 257, 1), (25, 1, 1), (25, 2, 1), (25, 128, 2),
              (25, 257, 2), (404, 1, 1), (404, 2, 2), (404, 6, 2)]
SHAPES_SCALED = [(1, 2, 2), (2, 2, 2), (3, 2, 2), (25, 2, 1), (25, 128, 2), (404, 1, 1), (404, 2, 2)]
GRU_EXTRA = [(50, 128, 2), (50, 2, 1)]


def case_table(kind):
    """[(scaling, T, B, D)] of the recurrent cases of the GPU suite."""
    rows = [("default",) + s for s in SHAPES_ALL + (GRU_EXTRA if kind == "gru" else [])]
    for scaling in ("x4", "sat"):
        rows += [(scaling,) + s for s in SHAPES_SCALED + ([(50, 128, 2)] if kind == "gru" else [])]
    return rows


def case_id(kind, row):
    scaling, T, B, D = row
    return f"{kind}-{scaling}-T{T}-B{B}-D{D}"


def case_seed(kind, row):
    scaling, T, B, D = row
    return (1 + SCALINGS.index(scaling)) * 1_000_003 + T * 7_919 + B * 31 + D + (0 if kind == "lstm" else 500_009)


def make_case(kind, row):
    """float32 CPU tensors gx, w_hh, dout (and b_hh for the GRU) of a case, from its seed."""
    scaling, T, B, D = row
    H, G = (LSTM_H, 4) if kind == "lstm" else (GRU_H, 3)
    g = torch.Generator().manual_seed(case_seed(kind, row))
    k = 1.0 / math.sqrt(H)
    uniform = lambda *s: (2 * torch.rand(*s, generator=g) - 1) * k                  # noqa: E731
    w_hh = uniform(D, G * H, H)
    b_hh = uniform(D, G * H)
    gx = torch.randn(T, B, D, G * H, generator=g)
    dout = torch.randn(T, B, D * H, generator=g)
    if scaling == "x4":
        w_hh, gx = 4 * w_hh, 4 * gx
    elif scaling == "sat":
        u = torch.rand(gx.shape, generator=g)
        sign = torch.where(torch.rand(gx.shape, generator=g) < 0.5, -1.0, 1.0)
        mag = torch.rand(gx.shape, generator=g)
        gx = torch.where(u < 0.06, sign * (30 + 10 * mag), gx)
        gx = torch.where(u < 0.01, sign * (100 + 20 * mag), gx)
        if kind == "lstm":
            gx[:, :, :, H:2 * H:16] = 35.0
    case = {"gx": gx.contiguous(), "w_hh": w_hh.contiguous(), "dout": dout.contiguous()}
    if kind == "gru":
        case["b_hh"] = b_hh.contiguous()
    return case


def per_row_err(x, ref, floor_scale=0.0, scale=None):
    """max over (utterance, direction) of max |x - ref| / scale for tensors (T, B, D, ...); scale (B, D) defaults to
    max(max |ref|, floor_scale) of that (utterance, direction).  Where the scale is exactly zero x must be exactly zero."""
    T, B, D = ref.shape[:3]
    if ref.numel() == 0:
        return 0.0
    diff = (x.double() - ref.double()).abs().permute(1, 2, 0, 3).reshape(B * D, -1).amax(1)
    if scale is None:
        scale = row_scale(ref, floor_scale)
    scale = scale.reshape(B * D).double()
    err = torch.where(scale > 0, diff / scale.clamp(min=1e-300), torch.where(diff > 0, math.inf, 0.0).double())
    return err.max().item()


def row_scale(ref, floor_scale=0.0):
    """(B, D): max(max |ref|, floor_scale) per (utterance, direction) of a tensor (T, B, D, ...)."""
    T, B, D = ref.shape[:3]
    return ref.double().abs().permute(1, 2, 0, 3).reshape(B, D, -1).amax(2).clamp(min=floor_scale)


def by_direction(out, D):
    """out (T, B, D*H) -> (T, B, D, H)."""
    T, B, DH = out.shape
    return out.reshape(T, B, D, DH // D)
