"""CPU references for every entry point of csrc/detector_elem.hip (include/advstep_detector.h), in plain torch on the CPU.  Nothing of
the package's wrappers is used; tests/test_detector_ref.py admits them, tests/test_gpu_detector_edges.py holds the kernels to them.

Two kinds:
  * float32 RESTATEMENTS of the kernels that are built only from +, *, comparisons and selection (affine_act modes 0 and 1,
    res2net_link, every pooling forward and backward, tail_pool1d, weighted_stats_backward, afms_row modes 1 and 3), with the
    kernel's own grouping of operations.  The library is built with -ffp-contract=off and torch's CPU float32 ops round once per
    op, so these are the kernel's bits.  The max-pool scan is written out: row-major over the window, take v when
    v > best or isnan(v), best = -inf at the start; `sel` is a byte.
  * float64 REFERENCES of every sum and of everything that holds expf / logf (closed forms, `dtype=F64`), and next to each the
    plain float32 CHAIN the kernel replaced (`*_chain32`, torch ops with autograd on the CPU): what float32 costs on that case.
Most functions take `dtype`: F32 gives the restatement (or, where the kernel's order of summation is not restated, just a
float32 evaluation), F64 the reference.  Tensors are (N, C, P) / (N, C, H, W) / (rows, L) as in the header."""
import math

import torch
import torch.nn.functional as F

F32, F64 = torch.float32, torch.float64
U = 2.0 ** -24                                      # unit roundoff of float32
SELU_ALPHA, SELU_SCALE = 1.6732632423543772848170429916717, 1.0507009873554804934193349852946
K_BLOCK, K_TAIL_OUT, ROW_CAP = 256, 448, 8192      # detector_elem.hip: kBlock, kTailOut, kRowCap


def gamma(m):
    """Higham's gamma_m = m u / (1 - m u): the relative error bound of m float32 roundings in a row."""
    return m * U / (1.0 - m * U)


def ch(v, like):
    """A per-channel vector (C) against an (N, C, ...) tensor."""
    return v.view(1, -1, *([1] * (like.dim() - 2)))


def relu_nan(r):
    """at::relu = clamp_min(0): NaN stays NaN, -0.0 becomes +0.0 (the kernel's r > 0 ? r : (r != r ? r : 0))."""
    return torch.where(r > 0, r, torch.where(torch.isnan(r), r, torch.zeros_like(r)))


def _selu_as(dtype):
    """alpha * scale as the kernel has it: the product of the two float32 constants, rounded to float32."""
    if dtype == F64:
        return SELU_ALPHA * SELU_SCALE
    return (torch.tensor(SELU_ALPHA, dtype=F32) * torch.tensor(SELU_SCALE, dtype=F32)).item()


# ---- affine_act, res2net_link -----------------------------------------------------------------------------------------------------

def affine_act_forward(x, scale, shift, pre, mode, slope, dtype=F32):
    x, s, t = x.to(dtype), ch(scale.to(dtype), x), ch(shift.to(dtype), x)
    if mode == 1:
        r = x + (ch(pre.to(dtype), x) if pre is not None else 0.0)
        return relu_nan(r) * s + t
    v = x * s + t
    if mode == 0:
        return torch.where(v > 0, v, v * slope)
    return torch.where(v <= 0, (torch.exp(v) - 1.0) * _selu_as(dtype), v * SELU_SCALE)


def affine_act_backward(gy, x, scale, shift, pre, mode, slope, dtype=F32):
    gy, x, s, t = gy.to(dtype), x.to(dtype), ch(scale.to(dtype), x), ch(shift.to(dtype), x)
    if mode == 1:
        r = x + (ch(pre.to(dtype), x) if pre is not None else 0.0)
        return torch.where(r <= 0, torch.zeros_like(gy), gy * s)
    v = x * s + t
    if mode == 0:
        one = torch.ones_like(v)
        return gy * torch.where(v > 0, one, one * slope) * s
    return gy * torch.where(v <= 0, _selu_as(dtype) * torch.exp(v), torch.full_like(v, SELU_SCALE)) * s


def selu_expr(x, scale, shift):
    """specrnet.py:159, 173: BatchNorm2d(eval), folded to one multiply-add, then SELU."""
    return F.selu(x * ch(scale, x) + ch(shift, x))


def res2net_link_forward(h, scale, shift, pre, other, dtype=F32):
    """-> (y, z or None)."""
    y = affine_act_forward(h, scale, shift, pre, 1, 0.0, dtype)
    return y, (None if other is None else y + other.to(dtype))


def res2net_link_backward(g1, g2, h, scale, shift, pre, dtype=F32):
    g = g1.to(dtype) + (g2.to(dtype) if g2 is not None else 0.0)        # the kernel adds 0.0f for an absent g2
    return affine_act_backward(g, h, scale, shift, pre, 1, 0.0, dtype)


# ---- the max-pool scan ---------------------------------------------------------------------------------------------------------------

def scan(win):
    """win (..., k) -> (best (...), code (...) uint8): ATen's max_pool scan, written out."""
    best = torch.full(win.shape[:-1], -math.inf, dtype=win.dtype)
    code = torch.zeros(win.shape[:-1], dtype=torch.uint8)
    for e in range(win.shape[-1]):
        v = win[..., e]
        take = (v > best) | torch.isnan(v)
        best = torch.where(take, v, best)
        code = torch.where(take, torch.full_like(code, e), code)
    return best, code


def windows2(v):
    """(N, C, H, W) -> (N, C, H/2, W/2, 4): the 2x2 windows, row-major inside a window; a trailing odd row / column is dropped."""
    N, C, H, W = v.shape
    Ho, Wo = H // 2, W // 2
    return v[:, :, :2 * Ho, :2 * Wo].reshape(N, C, Ho, 2, Wo, 2).permute(0, 1, 2, 4, 3, 5).reshape(N, C, Ho, Wo, 4)


def windows1(v, k):
    N, C, L = v.shape
    return v[:, :, :(L // k) * k].reshape(N, C, L // k, k)


def add_maxpool2_forward(a, b, bias, dtype=F32):
    """-> (y, sel): MaxPool2d(2)((a [+ b]) + bias[c]); the kernel adds 0.0f for an absent bias."""
    v = a.to(dtype) if b is None else a.to(dtype) + b.to(dtype)
    v = v + (ch(bias.to(dtype), v) if bias is not None else 0.0)
    return scan(windows2(v))


def gate_maxpool2_forward(x, gate, dtype=F32):
    """-> (y, sel, xw): MaxPool2d(2)(x * gate[n, c] + gate[n, c]) and the winner's un-gated input."""
    x = x.to(dtype)
    g = gate.to(dtype).view(x.shape[0], x.shape[1], 1, 1)
    y, sel = scan(windows2(x * g + g))
    return y, sel, windows2(x).gather(-1, sel.long().unsqueeze(-1)).squeeze(-1)


def unpool2(gy, sel, H, W, gate=None, addc=None, dtype=F32):
    """g (N, C, H, W) = gy * gate[n, c] + addc[n, c] at the winner of every window, addc elsewhere (odd tails included); the
    kernel multiplies by 1.0f for an absent gate and adds 0.0f for an absent addc (so a -0.0 of gy becomes +0.0)."""
    N, C, Ho, Wo = gy.shape
    c0 = addc.to(dtype).view(N, C, 1, 1) if addc is not None else torch.zeros(1, 1, 1, 1, dtype=dtype)
    gt = gate.to(dtype).view(N, C, 1, 1) if gate is not None else 1.0
    val = gy.to(dtype) * gt + c0
    win = c0.unsqueeze(-1).expand(N, C, Ho, Wo, 4).clone()
    win.scatter_(-1, sel.long().unsqueeze(-1), val.unsqueeze(-1))
    g = c0.expand(N, C, H, W).clone()
    g[:, :, :2 * Ho, :2 * Wo] = win.view(N, C, Ho, Wo, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(N, C, 2 * Ho, 2 * Wo)
    return g


def gate_blocks(H, W):
    """advstep_gate_maxpool2_blocks: workgroups of 256 threads over the H * ceil(W / 4) four-float row segments of a plane."""
    return 0 if H <= 0 or W <= 0 else -(-(H * ((W + 3) // 4)) // K_BLOCK)


def gate_partials(gy, sel, x):
    """-> (partial, mass) float64 (N * C, blocks): the sum of gy * (x_winner + 1) over the winners that a workgroup of
    pool2_backward_kernel owns (its thread idx = h * ceil(W / 4) + w / 4 handles input row h, columns 4 q .. 4 q + 3), and the
    sum of the terms' magnitudes."""
    N, C, H, W = x.shape
    Ho, Wo = gy.shape[2:]
    blocks, Wq = gate_blocks(H, W), (W + 3) // 4
    xw = windows2(x.to(F64)).gather(-1, sel.long().unsqueeze(-1)).squeeze(-1)
    t = gy.to(F64) * (xw + 1.0)
    i = torch.arange(Ho).view(1, 1, Ho, 1)
    j = torch.arange(Wo).view(1, 1, 1, Wo)
    blk = ((2 * i + (sel.long() >> 1)) * Wq + j // 2) // K_BLOCK
    flat = (torch.arange(N * C).view(N, C, 1, 1) * blocks + blk).reshape(-1)
    part, mass = torch.zeros(N * C * blocks, dtype=F64), torch.zeros(N * C * blocks, dtype=F64)
    part.index_add_(0, flat, t.reshape(-1))
    mass.index_add_(0, flat, t.abs().reshape(-1))
    return part.view(N * C, blocks), mass.view(N * C, blocks)


def gate_pooled(gy, xw, dtype=F64):
    """ggate (N * C) = sum over the pooled plane of gy * (xw + 1); with float64 also the sum of magnitudes."""
    t = gy.to(dtype) * (xw.to(dtype) + 1.0)
    rows, size = gy.shape[0] * gy.shape[1], gy[0, 0].numel()
    return t.reshape(rows, size).sum(dim=1), t.abs().reshape(rows, size).sum(dim=1)


def add_maxpool1d_forward(a, b, k, dtype=F32):
    v = a.to(dtype) if b is None else a.to(dtype) + b.to(dtype)
    return scan(windows1(v, k))


def unpool1d(gy, sel, L, k):
    """g (N, C, L): gy's own bits at the winners, +0.0 elsewhere and in the dropped tail."""
    N, C, Lo = gy.shape
    win = torch.zeros(N, C, Lo, k, dtype=gy.dtype)
    win.scatter_(-1, sel.long().unsqueeze(-1), gy.unsqueeze(-1))
    g = torch.zeros(N, C, L, dtype=gy.dtype)
    g[:, :, :Lo * k] = win.view(N, C, Lo * k)
    return g


def tail_pool1d_forward(h, res, scale, shift, pre, k, dtype=F32):
    v = affine_act_forward(h, scale, shift, pre, 1, 0.0, dtype) + res.to(dtype)
    return scan(windows1(v, k))


def tail_pool1d_backward(gy, sel, h, scale, pre, k, dtype=F32):
    """-> (g_h, g_res).  Without a single window (L < k) the entry point clears both outputs with a memset: +0.0 everywhere, where
    the kernel's 0 * scale[c] gives -0.0 in the dropped tail of a channel with a negative scale."""
    g = unpool1d(gy.to(dtype), sel, h.shape[2], k)
    if gy.shape[2] == 0:
        return torch.zeros_like(g), g
    return affine_act_backward(g, h, scale, torch.zeros_like(scale), pre, 1, 0.0, dtype), g


# ---- log_meannorm (rawnet3.py:80-85) ------------------------------------------------------------------------------------------------

def f32_scalar(v):
    """The float32 a C `float` argument carries."""
    return torch.tensor(v, dtype=F32).item()


def log_meannorm_expr(y, eps):
    x = torch.log(torch.abs(y) + eps)
    return x - torch.mean(x, dim=-1, keepdim=True)


def log_meannorm_forward(y, eps, dtype=F64):
    x = torch.log(y.to(dtype).abs() + f32_scalar(eps))
    return x - x.sum(dim=-1, keepdim=True) / y.shape[-1]


def log_meannorm_backward(gx, y, eps, dtype=F64):
    gx, y = gx.to(dtype), y.to(dtype)
    return (gx - gx.sum(dim=-1, keepdim=True) / y.shape[-1]) / (y.abs() + f32_scalar(eps)) * torch.sign(y)


# ---- AFMS row kernels (rawnet3.py:161-182) ----------------------------------------------------------------------------------------------

def afms_row(mode, a, b, alpha, r0, r1, C, dtype=F64):
    """(rows, L) tensors, c = row % C.  Modes 1 and 3 with F32 are the kernel's bits; modes 0 and 2 return (value, sum |term|)
    (mode 0: of the mean's terms a / L)."""
    a = a.to(dtype)
    rows, L = a.shape
    al = alpha.to(dtype)[torch.arange(rows) % C].view(rows, 1) if alpha is not None else None
    if mode == 0:
        return a.sum(dim=1) / L, a.abs().sum(dim=1) / L
    if mode == 1:
        return (a + al) * r0.to(dtype).view(rows, 1)
    if mode == 2:
        t = a * (b.to(dtype) + al)
        return t.sum(dim=1), t.abs().sum(dim=1)
    return a * r0.to(dtype).view(rows, 1) + r1.to(dtype).view(rows, 1)


def afms_expr(x, alpha, w, bias):
    """rawnet3.py:176-181: y = sigmoid(fc(mean_t x)); out = (x + alpha) * y."""
    y = torch.sigmoid(F.linear(x.mean(dim=2), w, bias))
    return (x + alpha.view(1, -1, 1)) * y.unsqueeze(-1)


# ---- attentive statistics (rawnet3.py:131-132) ----------------------------------------------------------------------------------------------

def weighted_stats_forward(x, w, dtype=F64):
    """-> (mu, m2, sum |x w|, sum |x x w|)."""
    x, w = x.to(dtype), w.to(dtype)
    a, b = x * w, (x * x) * w
    return a.sum(dim=1), b.sum(dim=1), a.abs().sum(dim=1), b.abs().sum(dim=1)


def weighted_stats_backward(x, w, gmu, gm2, dtype=F32):
    """-> (gx, gw), the kernel's grouping: gmu w + (2 gm2) (x w);  gmu x + gm2 (x x)."""
    x, w, ga, gb = x.to(dtype), w.to(dtype), gmu.to(dtype).view(-1, 1), gm2.to(dtype).view(-1, 1)
    return ga * w + (2.0 * gb) * (x * w), ga * x + gb * (x * x)


def weighted_stats_expr(x, w):
    return torch.sum(x * w, dim=-1), torch.sum((x ** 2) * w, dim=-1)


# ---- SpecRNet's attention gate (specrnet.py:145-149) ----------------------------------------------------------------------------------------

def gate_fc_expr(mean, w, bias):
    return torch.sigmoid(F.linear(mean, w, bias))


def gate_fc_forward(mean, w, bias, dtype=F64):
    """-> (gate, pre-activation, sum of the magnitudes of the pre-activation's terms)."""
    mean, w = mean.to(dtype), w.to(dtype)
    z, mass = mean @ w.t(), mean.abs() @ w.abs().t()
    if bias is not None:
        z, mass = z + bias.to(dtype), mass + bias.to(dtype).abs()
    return 1.0 / (1.0 + torch.exp(-z)), z, mass


def gate_fc_backward(partial, gate, w, inv_hw, dtype=F64):
    """g_mean (N, C) = inv_hw * ((sum_blocks partial) * gate * (1 - gate)) . w from partial (N * C, blocks); -> (g_mean, the same
    with every factor and term replaced by its magnitude)."""
    N, C = gate.shape
    gate, w, inv = gate.to(dtype), w.to(dtype), f32_scalar(inv_hw)
    p = partial.to(dtype).view(N, C, -1)
    t, tm = p.sum(dim=2) * gate * (1.0 - gate), p.abs().sum(dim=2) * gate.abs() * (1.0 - gate).abs()
    return (t @ w) * inv, (tm @ w.abs()) * abs(inv)


def attend_pool_expr(x, w, bias):
    """specrnet.py:145-149 and the pooling after it (:163-172): gate = sigmoid(fc(mean_hw x)); MaxPool2d(2)(x * gate + gate)."""
    gate = torch.sigmoid(F.linear(x.mean(dim=(2, 3)), w, bias)).view(x.shape[0], x.shape[1], 1, 1)
    return F.max_pool2d(x * gate + gate, 2)


# ---- the plain float32 chains the kernels replaced (torch ops with autograd, on the CPU) -------------------------------------------------

def chain32(expr, inputs, gy=None):
    """expr(*float32 leaves) -> (outputs, gradients of sum(out * gy) to every leaf, or None)."""
    leaves = [t.to(F32).clone().requires_grad_(gy is not None) for t in inputs]
    out = expr(*leaves)
    if gy is None:
        return out.detach(), None
    out.backward(gy.to(F32))
    return out.detach(), [t.grad for t in leaves]


def autograd64(expr, inputs, gys):
    """The same in float64: (outputs as a tuple, gradients of sum_k sum(out_k * gy_k) to every leaf)."""
    leaves = [t.to(F64).clone().requires_grad_(True) for t in inputs]
    out = expr(*leaves)
    out = out if isinstance(out, tuple) else (out,)
    torch.autograd.backward(out, [g.to(F64) for g in gys])
    return tuple(o.detach() for o in out), [t.grad for t in leaves]
