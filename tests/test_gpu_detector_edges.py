"""`-m gpu`: every entry point of csrc/detector_elem.hip through the C ABI (no autograd between a kernel and its check), at the
seams of its launch geometry and on both load / store routes, against the CPU references of tests/detector_ref.py (admitted by
tests/test_detector_ref.py).

Placement.  Slot, Placer, routes and on_routes are those of tests/test_gpu_row_edges.py; ByteSlot adds the `sel` bytes.  Every
device tensor of a launch, inputs and per-channel vectors included, lies between canaries, and no canary may change.  Every case
runs with all bases 16-byte aligned and with every float tensor one float past a 16-byte boundary; at the SEAM shapes of a kernel
each float tensor is also shifted alone (a launcher that forgets one pointer in its `vec` test takes the float4 route from a
misaligned base there).  Every launch runs twice and gives the same bytes.

Routes.  All outputs are byte-identical across the routes, the sums included: affine_act_kernel and res2net_link_kernel are
elementwise (the route only regroups elements over threads); pool2_forward_kernel's routes differ in the loads alone;
pool2_backward_kernel's in the store alone, its partial sums are formed from `sel`, gy and x before the store and reduced in a
fixed order (two terms per thread, the wave butterfly, four wave sums in index order); pool1d_*, tail_pool1d_*, log_meannorm,
afms_row, wstats_*, gate_grad_pooled and gate_fc_* have one route only (no 16-byte access), so a shifted base changes nothing
in them.

What is asserted.
  * Elementwise and selection kernels (affine_act modes 0 and 1, res2net_link, all pooling forwards and backwards, tail_pool1d,
    weighted_stats_backward, afms_row modes 1 and 3): the bytes of the float32 restatement, values and `sel`, NaN where it has
    NaN.  No case is left out: the arithmetic in front of every comparison is exact IEEE on both sides (-ffp-contract=off).
    For the Res2Net link the channels of the wide tensor outside the slice are canary too (and an odd batch stride leaves one
    canary element between the batches).
  * Mode 2 (SELU), log_meannorm and gate_fc_forward (expf / logf): against float64, err <= TAU and (err - FLOOR) <= RATIO x the
    error of the plain float32 chain on the CPU on the same case (tests/test_gpu_recurrent_f64.py's ratio() / FLOOR), err over
    the scale named at each constant.  TAU and RATIO are at most 4x the worst figure measured on gfx950 over this module's case
    table (in brackets; every figure goes to parity_record under detector_f64_*), and no TAU is looser than the tolerance
    tests/test_gpu_detector_ops.py applies to the same quantity (2e-6 forward values, 1e-5 gradients).
  * Pure-arithmetic sums: |got - float64| <= gamma_(d + r) * sum |t_i| (gamma_m = m u / (1 - m u), u = 2^-24, the sum of the
    magnitudes in float64), d = the longest chain of additions the code forms, r = the roundings inside a term; nothing measured:
      weighted_stats_forward   d = ceil(L / 64) + 6     (a lane's strided terms, 6 shuffle steps);  r = 1 (mu), 2 (m2)
      afms_row mode 0 / 2      d = ceil(L / 256) + 6 + 4 (thread terms, shuffle steps, block_sum's 4 wave sums added to 0);
                               r = 1 (mode 0: the division by L), 2 (mode 2: b + alpha, the product)
      gate partials            d = 2 + 6 + 3            (a thread's two windows, shuffle steps, 3 adds of the wave sums);  r = 2
      pooled gate gradient     d = ceil(L / 256) + 6 + 3;  r = 2 (xw + 1, the product)
      gate_fc_backward         m = blocks + C + 3: blocks - 1 adds of the partials, s * g, 1 - g, the product, C fused
                               multiply-adds (one rounding each), the factor inv_hw
      gate_fc_forward          C fused multiply-adds in front of the sigmoid: its error reaches the gate through sigmoid' <= 1/4,
                               so |gate - float64| <= gamma_C * sum |t_i| / 4 + TAU_SIGMOID (the sigmoid's own error, measured
                               at C <= 2 where the dot product has one or two roundings)
    and for each sum a one-hot case (one non-zero term at the first element, the last, and the last of a thread stride): the sum
    is then that float32 term exactly, which a dropped element cannot survive.
  * The refused calls (k = 1, k = 9, mode = 3, C = 0 / 257, L over the row cap, a NULL required pointer) return ADVSTEP_EINVAL
    before any launch: the outputs stay canary.

Inputs keep their ingredients at every size: zeros, -0.0, a subnormal (1e-40), ties inside a window, values exactly at an
activation's threshold, and, where no sum would be poisoned, NaN and +-inf.  The device keeps float32 subnormals (no flush), as
the CPU does: the restatements hold bit for bit with the subnormal in place.

Shapes: 6 planes (N = 2, C = 3, so nc % C differs from nc) except for the Res2Net link, whose alignment phase depends on the
channel alone and whose float4 route needs C * P % 4 == 0: N = 2, C = 4 (heads 0 .. 3 at odd P in one launch).

Found by this module and fixed in detector_elem.hip: pool2_forward_kernel's scalar route formed a + 0.0f for an absent b, which
turned a -0.0 input into +0.0 where the float4 route kept it (visible in xw, and in y with a -0.0 bias): test_gate_maxpool2_forward
has a -0.0 winner in the last pooled column of a plane.

646 cases, 6 s on gfx950."""
import math

import pytest
import torch

from tests import detector_ref as R
from tests.test_gpu_recurrent_f64 import FLOOR, ratio
from tests.test_gpu_row_edges import CANARY, PAD, on_routes

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
NAN, INF, SUB = math.nan, math.inf, 1e-40
N, C = 2, 3
EINVAL = 1

# ---- calibrated on gfx950: each constant is at most 4x the worst figure over this module's cases [in brackets; the plain float32
# chain's worst beside it]; every figure is written to parity_record under detector_f64_* ------------------------------------------
TAU = {
    "selu_fwd": 4.2e-7,          # over max(1, max |ref|)  [1.05e-7; chain 1.05e-7]
    "selu_bwd": 2.7e-7,          # over max |ref|          [6.95e-8; chain 7.73e-8]
    "logmn_fwd": 6.0e-7,         # over max(1, max |ref|)  [1.52e-7; chain 9.72e-8]
    "logmn_bwd": 2.7e-7,         # over max |ref|          [6.80e-8; chain 6.80e-8]
    "gatefc_fwd": 1.2e-6,        # absolute (a gate is at most 1)  [3.22e-7 at C = 256; chain 1.62e-7]
}
# (err - FLOOR) / the chain's error on the same case.  SELU both ways and log_meannorm's backward never left FLOOR (one float32
# ulp at the scale) on any case, so their measured ratio is 0 and 4 x 0 asks just that: err <= FLOOR.
RATIO = {"selu_fwd": 0.0,        # [0: err <= FLOOR on every case]
         "selu_bwd": 0.0,        # [0]
         "logmn_fwd": 4.8,       # [1.21]
         "logmn_bwd": 0.0,       # [0]
         "gatefc_fwd": 5.0}      # [1.30]
TAU_SIGMOID = 1.7e-7             # gate_fc_forward at C <= 2 against float64, absolute  [4.40e-8]


# ---- plumbing -----------------------------------------------------------------------------------------------------------------------------

def abi():
    from audio_deepfake_adversarial_attacks_amd import _lib
    return _lib.load(), torch.cuda.current_stream().cuda_stream


def addr(t, offset=0):
    """The address of a device tensor (plus `offset` floats); None stays NULL."""
    return None if t is None else t.data_ptr() + 4 * offset


def call(name, *args):
    lib, stream = abi()
    return getattr(lib, name)(*(addr(a) if isinstance(a, torch.Tensor) else a for a in args), stream)


def ok(name, *args):
    status = call(name, *args)
    assert status == 0, (name, status)


class ByteSlot:
    """A uint8 device tensor between canary bytes."""

    def __init__(self, src, cuda, fill=0xA5):
        shape = tuple(src.shape) if isinstance(src, torch.Tensor) else tuple(src)
        self.n, self.fill = math.prod(shape), fill
        self.buf = torch.full((PAD + self.n + PAD,), fill, dtype=torch.uint8, device=cuda)
        self.t = self.buf[PAD:PAD + self.n].view(shape)
        if isinstance(src, torch.Tensor):
            self.t.copy_(src)

    def intact(self):
        return bool((self.buf[:PAD] == self.fill).all() and (self.buf[PAD + self.n:] == self.fill).all())


def put(place, name, src):
    """place(name, src) for a float tensor or shape; None and empty tensors become NULL (an empty view has no address)."""
    if src is None or math.prod(src.shape if isinstance(src, torch.Tensor) else src) == 0:
        return None
    return place(name, src)


def put_bytes(place, src):
    if math.prod(src.shape if isinstance(src, torch.Tensor) else src) == 0:
        return None
    slot = ByteSlot(src, place.cuda)
    place.slots.append(slot)
    return slot.t


def raw(t):
    return t if t.dtype == torch.uint8 else t.contiguous().view(torch.int32)


def run(cuda, names, launch, seam=False):
    """launch(place) -> a tuple of device tensors (or None), on every route (each name alone too at a seam shape), twice: the
    same bytes both times and on every route, no canary changed.  -> the CPU copies."""
    key = 4 if seam else 8                   # test_gpu_row_edges.routes: aligned + shifted, at its SINGLE lengths each name alone
    first, again = on_routes(cuda, key, names, launch), on_routes(cuda, key, names, launch)
    assert len(first) == (2 + len(names) if seam else 2)
    base = first["aligned"]
    for label in first:
        for k, (a, b, c) in enumerate(zip(first[label], again[label], base)):
            if a is None:
                assert b is None and c is None
                continue
            assert torch.equal(raw(a), raw(b)), ("two runs differ", label, k)
            assert torch.equal(raw(a), raw(c)), ("routes differ", label, k)
    return base


def same(a, b):
    """The same bytes, NaN where the restatement has NaN."""
    if a.dtype == torch.uint8:
        return a.shape == b.shape and torch.equal(a, b)
    na, nb = torch.isnan(a), torch.isnan(b)
    return a.shape == b.shape and bool((na == nb).all()) and torch.equal(raw(a)[~na], raw(b)[~nb])


def gen(seed):
    return torch.Generator().manual_seed(seed)


def noise(shape, seed, special=True, scale=1.0, off=0):
    """N(0, scale^2) with a 0.0, a -0.0, a subnormal, a tie between neighbours every 11 elements and, with `special`, one NaN,
    one +inf and one -inf (each only where half of the tensor stays noise); `off` moves them."""
    t = torch.randn(shape, generator=gen(seed)) * scale
    f = t.view(-1)
    n = f.numel()
    if n >= 12:
        f[5::11] = f[4::11][:f[5::11].numel()]
    vals = [0.0, -0.0, SUB] + ([NAN, INF, -INF] if special else [])
    step = max(n // (len(vals) + 1), 1)
    for k, v in enumerate(vals):
        if n >= 2 * (k + 1):
            f[(1 + off + k * step) % n] = v
    return t


FIG = {}


def calibrated(key, got, ref, plain, parity_record, floor_scale, label):
    """err = max |got - ref| over max(floor_scale, max |ref|) on the finite entries of the float64 reference (elsewhere got is NaN
    where it is NaN and equal where it is infinite); the same for the plain float32 chain; the figures are printed and recorded."""
    fin = torch.isfinite(ref)
    assert torch.equal(torch.isnan(got), torch.isnan(ref)), label
    inf = torch.isinf(ref)
    assert torch.equal(got[inf].double(), ref[inf]), label
    if not fin.any():
        return
    scale = max(ref[fin].abs().max().item(), floor_scale)
    err = (got.double() - ref)[fin].abs().max().item() / scale
    pl = (plain.double() - ref)[fin]
    pl = pl[torch.isfinite(pl)].abs().max().item() / scale if torch.isfinite(pl).any() else 0.0
    q = ratio(err, pl)
    for k, v in ((key + "_err", err), (key + "_plain", pl), (key + "_ratio", q)):
        FIG[k] = max(FIG.get(k, 0.0), v)
        parity_record["detector_f64_" + k] = FIG[k]
    print(f"{key} {label}: err {err:.3e}, plain float32 chain {pl:.3e}, ratio {q:.2f}")
    assert err <= TAU[key], (label, err)
    assert q <= RATIO[key], (label, err, pl, q)


def within(got, ref, m, mass, label, amp=1.0):
    """|got - ref| <= gamma_m * sum |t_i| + m * amp * 2^-149, NaN nowhere.  The second term is the standard model's underflow
    allowance (a rounding into the subnormal range is off by up to 2^-150 absolutely; the inputs hold a subnormal), amp = the
    largest factor a later operation applies to it."""
    assert torch.isfinite(got).all(), label
    excess = (got.double() - ref).abs() - R.gamma(m) * mass - m * amp * 2.0 ** -149
    assert (excess <= 0).all(), (label, m, excess.max().item())


SCALE, SHIFT, PRE = torch.tensor([0.5, -1.25, 2.0]), torch.tensor([0.25, -0.625, 0.0]), torch.tensor([0.5, -0.75, 0.0])


# ---- affine_act ---------------------------------------------------------------------------------------------------------------------------

PLANES = (1, 2, 3, 4, 5, 7, 4095, 4096, 4097, 4099, 4100, 4103, 8195)
SEAM_P = (7, 4096, 4103)


def at_threshold(x, mode, pre):
    """One element per plane exactly where the activation switches: x + pre == 0 (mode 1), x * scale + shift == 0 (modes 0, 2:
    -0.5, -0.5 and 0 with SCALE and SHIFT, exact in float32 and in float64, so that SELU's derivative, which jumps there, takes
    the same branch in the kernel and in the float64 reference)."""
    P = x.shape[2]
    if P >= 4:
        thr = -(pre if pre is not None else torch.zeros(x.shape[1])) if mode == 1 else (-SHIFT.double() / SCALE.double()).float()
        x[:, :, P // 2] = thr.view(1, -1)
    return x


@pytest.mark.parametrize("bwd", [False, True])
@pytest.mark.parametrize("mode", [0, 1, "1 without pre", 2])
@pytest.mark.parametrize("P", PLANES)
def test_affine_act(cuda, parity_record, P, mode, bwd):
    """6 planes, so at odd P heads 0 .. 3 occur in one launch (P = 1, 2: head > P), bodies of 1023 .. 1025 quads (P = 4095 ..
    4103; a tile is 1024), two tiles and a third of one quad (8195), tails 0 .. 3."""
    pre = PRE if mode == 1 else None
    m = 1 if mode == "1 without pre" else mode
    x = at_threshold(noise((N, C, P), 1, scale=2.0), m, pre)
    gy = noise((N, C, P), 2, off=1) if bwd else None
    names = ("x", "scale", "shift") + (("pre",) if pre is not None else ()) + ("out",) + (("gy",) if bwd else ())

    def launch(p):
        dx, ds, dt, dp, out = p("x", x), p("scale", SCALE), p("shift", SHIFT), put(p, "pre", pre), p("out", x.shape)
        if bwd:
            ok("advstep_affine_act_backward_f32", p("gy", gy), dx, ds, dt, dp, out, N, C, P, m, 0.3)
        else:
            ok("advstep_affine_act_forward_f32", dx, ds, dt, dp, out, N, C, P, m, 0.3)
        return (out,)

    got, = run(cuda, names, launch, seam=P in SEAM_P)
    if m != 2:
        want = R.affine_act_backward(gy, x, SCALE, SHIFT, pre, m, 0.3) if bwd else R.affine_act_forward(x, SCALE, SHIFT, pre, m, 0.3)
        assert same(got, want)
        return
    if bwd:
        ref = R.affine_act_backward(gy, x, SCALE, SHIFT, None, 2, 0.0, F64)
        plain = R.chain32(R.selu_expr, [x, SCALE, SHIFT], gy)[1][0]
        calibrated("selu_bwd", got, ref, plain, parity_record, 1e-30, f"P={P}")
    else:
        ref = R.affine_act_forward(x, SCALE, SHIFT, None, 2, 0.0, F64)
        calibrated("selu_fwd", got, ref, R.chain32(R.selu_expr, [x, SCALE, SHIFT])[0], parity_record, 1.0, f"P={P}")


# ---- res2net_link -------------------------------------------------------------------------------------------------------------------------

LC, LCW = 4, 12                                   # the link's channels; channels of the wide (concatenated) tensor
S4, T4, P4 = torch.tensor([0.5, -1.25, 2.0, 1.0]), torch.tensor([0.25, -0.5, 0.0, -0.0]), torch.tensor([0.5, -0.75, 0.0, SUB])


def slices(flat, off, bs, P):
    """The (N, LC, P) channel slice at element `off` of every batch of a flat wide tensor with batch stride bs."""
    return torch.stack([flat[n * bs + off:n * bs + off + LC * P].view(LC, P) for n in range(N)])


def embed(flat, off, bs, val):
    for n in range(N):
        flat[n * bs + off:n * bs + off + val[n].numel()] = val[n].reshape(-1)
    return flat


@pytest.mark.parametrize("bwd", [False, True])
@pytest.mark.parametrize("layout", ["strides % 4 == 0", "odd strides", "absent"])
@pytest.mark.parametrize("P", PLANES)
def test_res2net_link(cuda, P, layout, bwd):
    """Channel slices (channels 4 .. 7 and 8 .. 11 of 12) of wide tensors whose batch stride is 12 P (float4 route when the bases
    are aligned) or 12 P + 1 (element route; one canary element between the batches of an output); `absent`: no other / z
    (forward), no g2 (backward).  The whole wide output is compared: canary outside the slice."""
    bs = LCW * P + (1 if layout == "odd strides" else 0)
    off1, off2 = 4 * P, 8 * P
    h = at_threshold(noise((N, LC, P), 3, scale=2.0), 1, P4)
    w1, w2 = noise((N * bs,), 4, off=1), (None if layout == "absent" else noise((N * bs,), 5, off=2))
    pre = None if layout == "absent" else P4

    def vectors(p):
        return p("scale", S4), p("shift", T4), put(p, "pre", pre)

    if bwd:
        names = ("g1", "h", "scale", "shift", "gx") + (() if w2 is None else ("g2", "pre"))

        def launch(p):
            d1, d2, dh, gx = p("g1", w1), put(p, "g2", w2), p("h", h), p("gx", h.shape)
            ok("advstep_res2net_link_backward_f32", addr(d1, off1), bs, addr(d2, off2), bs, dh, *vectors(p), gx, N, LC, P)
            return (gx,)

        got, = run(cuda, names, launch, seam=P in SEAM_P)
        g2 = None if w2 is None else slices(w2, off2, bs, P)
        assert same(got, R.res2net_link_backward(slices(w1, off1, bs, P), g2, h, S4, T4, pre))
        return
    names = ("h", "scale", "shift", "y") + (() if w2 is None else ("other", "z", "pre"))

    def launch(p):
        dh, y, do = p("h", h), p("y", (N * bs,)), put(p, "other", w2)
        z = None if w2 is None else p("z", h.shape)
        ok("advstep_res2net_link_forward_f32", dh, *vectors(p), addr(y, off1), bs, addr(do, off2), bs, z, N, LC, P)
        return y, z

    y, z = run(cuda, names, launch, seam=P in SEAM_P)
    y_ref, z_ref = R.res2net_link_forward(h, S4, T4, pre, None if w2 is None else slices(w2, off2, bs, P))
    assert same(y, embed(torch.full((N * bs,), CANARY), off1, bs, y_ref))
    assert (z is None and z_ref is None) or same(z, z_ref)


# ---- the 2x2 pooling family -----------------------------------------------------------------------------------------------------------------

HW = [(2, 2), (2, 3), (3, 2), (2, 4), (3, 6), (2, 8), (5, 12), (4, 1024), (2, 1028), (3, 1026), (1, 8), (8, 1)]
SEAM_HW = ((2, 4), (5, 12), (2, 1028))
GATE = torch.tensor([[0.25, 0.9, 0.5], [1.0, 0.731, 0.0]])
BIAS = torch.tensor([0.5, -0.0, -1.0])


def plane_input(H, W, seed, special=True):
    """noise() with, in plane (0, 0), a window in the last pooled column of the first pooled row whose winner is a -0.0 (the
    element route's thread when W / 2 is odd), and in plane (0, 1) a window of four equal values."""
    x = noise((N, C, H, W), seed, special)
    if H >= 2 and W >= 2:
        j = 2 * (W // 2 - 1)
        x[0, 0, 0:2, j:j + 2] = torch.tensor([[-5.0, -0.0], [-5.0, -5.0]])
        x[0, 1, 0:2, 0:2] = 1.5
    return x


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("with_b", [False, True])
@pytest.mark.parametrize("H,W", HW)
def test_add_maxpool2_forward(cuda, H, W, with_b, with_bias):
    a, b = plane_input(H, W, 6), (noise((N, C, H, W), 7, off=3) if with_b else None)
    bias = BIAS if with_bias else None
    names = ("a", "y") + (("b",) if with_b else ()) + (("bias",) if with_bias else ())

    def launch(p):
        y, sel = put(p, "y", (N, C, H // 2, W // 2)), put_bytes(p, (N, C, H // 2, W // 2))
        ok("advstep_add_maxpool2_forward_f32", p("a", a), put(p, "b", b), put(p, "bias", bias), y, sel, N, C, H, W)
        return y, sel

    y, sel = run(cuda, names, launch, seam=(H, W) in SEAM_HW)
    want_y, want_sel = R.add_maxpool2_forward(a, b, bias)
    assert (y is None and want_y.numel() == 0) or (same(y, want_y) and same(sel, want_sel))


@pytest.mark.parametrize("with_xw", [False, True])
@pytest.mark.parametrize("H,W", HW)
def test_gate_maxpool2_forward(cuda, H, W, with_xw):
    x = plane_input(H, W, 8)
    names = ("x", "gate", "y") + (("xw",) if with_xw else ())

    def launch(p):
        shape = (N, C, H // 2, W // 2)
        y, sel, xw = put(p, "y", shape), put_bytes(p, shape), (put(p, "xw", shape) if with_xw else None)
        if with_xw:
            ok("advstep_gate_maxpool2_forward_xw_f32", p("x", x), p("gate", GATE), y, sel, xw, N, C, H, W)
        else:
            ok("advstep_gate_maxpool2_forward_f32", p("x", x), p("gate", GATE), y, sel, N, C, H, W)
        return y, sel, xw

    y, sel, xw = run(cuda, names, launch, seam=(H, W) in SEAM_HW)
    want = R.gate_maxpool2_forward(x, GATE)
    if want[0].numel() == 0:
        assert y is None
        return
    assert same(y, want[0]) and same(sel, want[1]) and (xw is None or same(xw, want[2]))
    if with_xw:
        assert want[1][0, 0, 0, -1] == 1 and raw(xw)[0, 0, 0, -1].item() == -2 ** 31      # the -0.0 winner, with its sign


GATE_D, GATE_R = 2 + 6 + 3, 2


@pytest.mark.parametrize("entry", ["plain", "input", "input + addc", "gate + input", "gate"])
@pytest.mark.parametrize("H,W", HW)
def test_pool2_backward(cuda, H, W, entry):
    """The four entry points over pool2_backward_kernel: the float4 store (W % 4 == 0 and g aligned) and the element store give
    the same bytes; odd trailing rows and columns hold addc (or +0.0); the gate's partial sums per workgroup within
    gamma_(11 + 2) of float64."""
    sums = entry in ("gate + input", "gate")
    x = plane_input(H, W, 9, special=not sums)
    shape = (N, C, H // 2, W // 2)
    if entry == "plain":
        _, sel = R.add_maxpool2_forward(x, None, None)
    else:
        _, sel, _ = R.gate_maxpool2_forward(x, GATE)
    gy = noise(shape, 10, special=not sums, off=2)
    addc = noise((N, C), 11, special=False) if entry == "input + addc" else None
    blocks = abi()[0].advstep_gate_maxpool2_blocks(H, W)
    assert blocks == R.gate_blocks(H, W)
    names = {"plain": ("gy", "g"), "input": ("gy", "gate", "g"), "input + addc": ("gy", "gate", "addc", "g"),
             "gate + input": ("gy", "x", "gate", "g", "partial"), "gate": ("gy", "x", "partial")}[entry]
    names = tuple(n for n in names if n != "gy" or gy.numel())

    def launch(p):
        dgy, dsel = put(p, "gy", gy), put_bytes(p, sel)
        g = None if entry == "gate" else p("g", x.shape)
        partial = p("partial", (N * C, blocks)) if sums else None
        if entry == "plain":
            ok("advstep_maxpool2_backward_f32", dgy, dsel, g, N, C, H, W)
        elif entry == "gate":
            ok("advstep_gate_maxpool2_backward_gate_f32", dgy, dsel, p("x", x), partial, N, C, H, W)
        elif entry == "gate + input":
            ok("advstep_gate_maxpool2_backward_f32", dgy, dsel, p("x", x), p("gate", GATE), g, partial, N, C, H, W)
        else:
            ok("advstep_gate_maxpool2_backward_input_f32", dgy, dsel, p("gate", GATE), put(p, "addc", addc), g, N, C, H, W)
        return g, partial

    g, partial = run(cuda, names, launch, seam=(H, W) in SEAM_HW)
    if g is not None:
        assert same(g, R.unpool2(gy, sel, H, W, gate=None if entry == "plain" else GATE, addc=addc))
    if sums:
        ref, mass = R.gate_partials(gy, sel, x)
        within(partial, ref, GATE_D + GATE_R, mass, (H, W))
        if gy.numel():                                             # one-hot: the first and the last pooled output of every plane
            for pos in {0, gy[0, 0].numel() - 1}:
                hot = torch.zeros_like(gy)
                hot.view(N, C, -1)[:, :, pos] = gy.view(N, C, -1)[:, :, pos] + 3.0

                def launch_hot(p):
                    part = p("partial", (N * C, blocks))
                    ok("advstep_gate_maxpool2_backward_gate_f32", p("gy", hot), put_bytes(p, sel), p("x", x), part, N, C, H, W)
                    return (part,)

                got, = run(cuda, ("gy", "x", "partial"), launch_hot)
                xw = R.windows2(x).gather(-1, sel.long().unsqueeze(-1)).squeeze(-1)
                term = (hot * (xw + 1.0)).view(N * C, -1)[:, pos]
                assert torch.equal(got.sum(dim=1), term) and ((got != 0).sum(dim=1) <= 1).all(), pos


@pytest.mark.parametrize("size", [0, 1, 255, 256, 257])
def test_gate_pooled_gradient(cuda, size):
    """ggate = sum gy (xw + 1) over a pooled plane of `size` elements (H = 2, W = 2 size, or (2, 1) for none: the kernel then
    writes 0 from NULL inputs); d = ceil(size / 256) + 6 + 3, r = 2."""
    H, W = 2, max(2 * size, 1)
    gy, xw = noise((N, C, 1, size), 12, special=False), noise((N, C, 1, size), 13, special=False, off=1)

    def launcher(dy):
        def launch(p):
            out = p("ggate", (N * C,))
            ok("advstep_gate_maxpool2_backward_gate_pooled_f32", put(p, "gy", dy), put(p, "xw", xw), out, N, C, H, W)
            return (out,)
        return launch

    names = ("ggate",) + (("gy", "xw") if size else ())
    got, = run(cuda, names, launcher(gy), seam=size == 257)
    ref, mass = R.gate_pooled(gy, xw)
    within(got, ref, -(-size // 256) + 6 + 3 + 2, mass, size)
    if size == 0:
        assert torch.equal(raw(got), torch.zeros(N * C, dtype=torch.int32))
    for pos in sorted({0, size - 1, 255} & set(range(size))):
        hot = torch.zeros_like(gy)
        hot[..., pos] = gy[..., pos] + 3.0
        got, = run(cuda, names, launcher(hot))
        assert torch.equal(got, (hot * (xw + 1.0)).view(N * C, -1)[:, pos]), pos


# ---- MaxPool1d(k) and the Bottle2neck tail --------------------------------------------------------------------------------------------------

KS = (2, 3, 5, 8)


def pool1d_lengths(k):
    return [k - 1, k, k * 256, k * 256 + k - 1, k * 257]


def tied(x, k):
    """A window of equal values and one whose winner is its last element."""
    if x.shape[2] >= 3 * k:
        x[:, :, k:2 * k] = 0.75
        x[0, 0, 2 * k:3 * k] = -3.0
        x[0, 0, 3 * k - 1] = 2.0
    return x


@pytest.mark.parametrize("with_b", [False, True])
@pytest.mark.parametrize("k,L", [(k, L) for k in KS for L in pool1d_lengths(k)])
def test_add_maxpool1d_forward(cuda, k, L, with_b):
    a, b = tied(noise((N, C, L), 14), k), (noise((N, C, L), 15, off=1) if with_b else None)

    def launch(p):
        y, sel = put(p, "y", (N, C, L // k)), put_bytes(p, (N, C, L // k))
        ok("advstep_add_maxpool1d_forward_f32", p("a", a), put(p, "b", b), y, sel, N, C, L, k)
        return y, sel

    names = ("a",) + (("b",) if with_b else ()) + (("y",) if L >= k else ())
    y, sel = run(cuda, names, launch, seam=L == k * 256 and k in (2, 5))
    want_y, want_sel = R.add_maxpool1d_forward(a, b, k)
    assert (y is None and L < k) or (same(y, want_y) and same(sel, want_sel))


@pytest.mark.parametrize("k,L", [(k, L) for k in KS for L in pool1d_lengths(k)])
def test_maxpool1d_backward(cuda, k, L):
    """L = k - 1: no window, the memset route (gy and sel NULL); else the last window's thread also clears the dropped tail."""
    _, sel = R.add_maxpool1d_forward(tied(noise((N, C, L), 16), k), None, k)
    gy = noise((N, C, L // k), 17, off=1)

    def launch(p):
        g = p("g", (N, C, L))
        ok("advstep_maxpool1d_backward_f32", put(p, "gy", gy), put_bytes(p, sel), g, N, C, L, k)
        return (g,)

    got, = run(cuda, ("g",) + (("gy",) if L >= k else ()), launch, seam=L == k * 256 and k in (2, 5))
    assert same(got, R.unpool1d(gy, sel, L, k))


TAIL_LO = (0, 1, 447, 448, 449, 896, 897)
TAIL_CASES = [(k, Lo, t) for k in KS for Lo in TAIL_LO for t in (0, k - 1)]
TAIL_SEAM = ((8, 448, 0), (3, 449, 2), (5, 896, 4))


@pytest.mark.parametrize("k,Lo,drop", TAIL_CASES)
def test_tail_pool1d_forward(cuda, k, Lo, drop):
    """A workgroup owns 448 outputs (Lo = 448, 896: full tiles; 449, 897: a tile of one output); k = 8 at 448 fills the LDS
    window.  `pre` is NULL in the cases without a dropped tail."""
    L = Lo * k + drop
    pre = PRE if drop else None
    h, res = tied(at_threshold(noise((N, C, L), 18, scale=2.0), 1, pre), k), noise((N, C, L), 19, off=1)

    def launch(p):
        y, sel = put(p, "y", (N, C, Lo)), put_bytes(p, (N, C, Lo))
        ok("advstep_tail_pool1d_forward_f32", put(p, "h", h), put(p, "res", res), p("scale", SCALE), p("shift", SHIFT),
           put(p, "pre", pre), y, sel, N, C, L, k)
        return y, sel

    names = ("scale", "shift") + (("h", "res") if L else ()) + (("y",) if Lo else ()) + (("pre",) if drop else ())
    y, sel = run(cuda, names, launch, seam=(k, Lo, drop) in TAIL_SEAM)
    want_y, want_sel = R.tail_pool1d_forward(h, res, SCALE, SHIFT, pre, k)
    assert (y is None and Lo == 0) or (same(y, want_y) and same(sel, want_sel))


@pytest.mark.parametrize("k,Lo,drop", TAIL_CASES)
def test_tail_pool1d_backward(cuda, k, Lo, drop):
    """The last tile also owns the dropped tail (gradient +0.0); Lo = 0 with a tail: the memset route for both outputs."""
    L = Lo * k + drop
    pre = PRE if drop else None
    h = tied(at_threshold(noise((N, C, L), 20, scale=2.0), 1, pre), k)
    _, sel = R.tail_pool1d_forward(h, noise((N, C, L), 21, off=1), SCALE, SHIFT, pre, k)
    gy = noise((N, C, Lo), 22, off=2)

    def launch(p):
        g_h, g_res = put(p, "g_h", (N, C, L)), put(p, "g_res", (N, C, L))
        ok("advstep_tail_pool1d_backward_f32", put(p, "gy", gy), put_bytes(p, sel), put(p, "h", h), p("scale", SCALE),
           put(p, "pre", pre), g_h, g_res, N, C, L, k)
        return g_h, g_res

    names = ("scale",) + (("h", "g_h", "g_res") if L else ()) + (("gy",) if Lo else ()) + (("pre",) if drop else ())
    g_h, g_res = run(cuda, names, launch, seam=(k, Lo, drop) in TAIL_SEAM)
    want = R.tail_pool1d_backward(gy, sel, h, SCALE, pre, k)
    assert (g_h is None and L == 0) or (same(g_h, want[0]) and same(g_res, want[1]))


# ---- log_meannorm ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bwd", [False, True])
@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("L", [1, 255, 256, 257, 8191, 8192])
def test_log_meannorm(cuda, parity_record, L, rows, bwd):
    """Rows of 1 .. 8192 frames (32 per thread at the cap), zeros, -0.0 and a subnormal in every launch; with three rows the last
    one holds a NaN: its whole forward row is NaN (the mean), in the backward only that element."""
    y = noise((rows, L), 23, special=False, scale=0.1)
    if rows == 3:
        y[2, L // 2] = NAN
    gx = noise((rows, L), 24, special=False, off=1)

    def launch(p):
        out = p("out", (rows, L))
        if bwd:
            ok("advstep_log_meannorm_backward_f32", p("gx", gx), p("y", y), 1e-6, out, rows, L)
        else:
            ok("advstep_log_meannorm_forward_f32", p("y", y), 1e-6, out, rows, L)
        return (out,)

    got, = run(cuda, ("y", "out") + (("gx",) if bwd else ()), launch, seam=L in (256, 8192))
    eps = R.f32_scalar(1e-6)
    if bwd:
        ref = R.log_meannorm_backward(gx, y, 1e-6)
        plain = R.chain32(lambda t: R.log_meannorm_expr(t, eps), [y], gx)[1][0]
        calibrated("logmn_bwd", got, ref, plain, parity_record, 1e-30, f"L={L} rows={rows}")
    else:
        ref = R.log_meannorm_forward(y, 1e-6)
        plain = R.chain32(lambda t: R.log_meannorm_expr(t, eps), [y])[0]
        calibrated("logmn_fwd", got, ref, plain, parity_record, 1.0, f"L={L} rows={rows}")
        assert rows == 1 or torch.isnan(got[2]).all()


# ---- AFMS row kernels -------------------------------------------------------------------------------------------------------------------------

def hot_rows(t, pos):
    """t with everything but column `pos` zeroed (the kept entries moved away from 0)."""
    hot = torch.zeros_like(t)
    hot[:, pos] = t[:, pos] + 3.0
    return hot


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("L", [1, 255, 256, 257, 1025])
def test_afms_row(cuda, L, mode):
    """rows = N * C = 6, alpha by row % 3.  Modes 1 and 3: the restatement's bytes.  Modes 0 and 2: d = ceil(L / 256) + 6 + 4."""
    rows = N * C
    sums = mode in (0, 2)
    a, b = noise((rows, L), 25, special=not sums), noise((rows, L), 26, special=False, off=1)
    alpha, r0, r1 = PRE, noise((rows,), 27, special=False), noise((rows,), 28, special=False, off=1)
    use = {0: ("a",), 1: ("a", "alpha", "r0"), 2: ("a", "b", "alpha"), 3: ("a", "r0", "r1")}[mode]

    def launcher(da):
        def launch(p):
            src = {"a": da, "b": b, "alpha": alpha, "r0": r0, "r1": r1}
            dev = {n: (p(n, src[n]) if n in use else None) for n in src}
            out = p("out", (rows,) if sums else (rows, L))
            ok("advstep_afms_row_f32", mode, dev["a"], dev["b"], dev["alpha"], dev["r0"], dev["r1"], out, rows, C, L)
            return (out,)
        return launch

    got, = run(cuda, use + ("out",), launcher(a), seam=L in (256, 257))
    if not sums:
        assert same(got, R.afms_row(mode, a, b, alpha, r0, r1, C, F32))
        return
    ref, mass = R.afms_row(mode, a, b, alpha, r0, r1, C)
    within(got, ref, -(-L // 256) + 6 + 4 + (1 if mode == 0 else 2), mass, L)
    al = alpha[torch.arange(rows) % C]
    for pos in sorted({0, L - 1, 255} & set(range(L))):
        hot = hot_rows(a, pos)
        got, = run(cuda, use + ("out",), launcher(hot))
        want = hot[:, pos] / torch.tensor(float(L)) if mode == 0 else hot[:, pos] * (b[:, pos] + al)
        assert torch.equal(got, want), pos


# ---- attentive statistics -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows", [1, 3, 4, 5])
@pytest.mark.parametrize("L", [1, 63, 64, 65, 429])
def test_weighted_stats_forward(cuda, rows, L):
    """One wave per row, four rows per workgroup (rows = 4: full; 5: a workgroup with one row); d = ceil(L / 64) + 6."""
    x, w = noise((rows, L), 29, special=False), noise((rows, L), 30, special=False, off=1)

    def launcher(dw):
        def launch(p):
            mu, m2 = p("mu", (rows,)), p("m2", (rows,))
            ok("advstep_weighted_stats_forward_f32", p("x", x), p("w", dw), mu, m2, rows, L)
            return mu, m2
        return launch

    names = ("x", "w", "mu", "m2")
    mu, m2 = run(cuda, names, launcher(w), seam=(rows, L) in ((4, 64), (5, 65)))
    ref_mu, ref_m2, mass_mu, mass_m2 = R.weighted_stats_forward(x, w)
    d = -(-L // 64) + 6
    within(mu, ref_mu, d + 1, mass_mu, ("mu", rows, L))
    within(m2, ref_m2, d + 2, mass_m2, ("m2", rows, L))
    for pos in sorted({0, L - 1, 63} & set(range(L))):
        hot = hot_rows(w, pos)
        mu, m2 = run(cuda, names, launcher(hot))
        assert torch.equal(mu, x[:, pos] * hot[:, pos]) and torch.equal(m2, (x[:, pos] * x[:, pos]) * hot[:, pos]), pos


@pytest.mark.parametrize("rows", [1, 3, 4, 5])
@pytest.mark.parametrize("L", [1, 63, 64, 65, 429])
def test_weighted_stats_backward(cuda, rows, L):
    x, w = noise((rows, L), 31), noise((rows, L), 32, off=1)
    gmu, gm2 = noise((rows,), 33, special=False), noise((rows,), 34, special=False, off=1)

    def launch(p):
        gx, gw = p("gx", (rows, L)), p("gw", (rows, L))
        ok("advstep_weighted_stats_backward_f32", p("x", x), p("w", w), p("gmu", gmu), p("gm2", gm2), gx, gw, rows, L)
        return gx, gw

    gx, gw = run(cuda, ("x", "w", "gmu", "gm2", "gx", "gw"), launch, seam=(rows, L) in ((4, 64), (5, 65)))
    want = R.weighted_stats_backward(x, w, gmu, gm2)
    assert same(gx, want[0]) and same(gw, want[1])


# ---- the attention gate on (N, C) -------------------------------------------------------------------------------------------------------------

FC_C = (1, 2, 63, 64, 65, 255, 256)


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("Cg", FC_C)
def test_gate_fc_forward(cuda, parity_record, Cg, n, with_bias):
    """One workgroup per sample, thread = output channel, up to the 256 the kernel is built for."""
    mean, w = noise((n, Cg), 35, special=False), noise((Cg, Cg), 36, special=False, off=1) / math.sqrt(Cg)
    bias = noise((Cg,), 37, special=False, off=2) if with_bias else None

    def launcher(dm, db):
        def launch(p):
            gate = p("gate", (n, Cg))
            ok("advstep_gate_fc_forward_f32", p("mean", dm), p("w", w), put(p, "bias", db), gate, n, Cg)
            return (gate,)
        return launch

    names = ("mean", "w", "gate") + (("bias",) if with_bias else ())
    got, = run(cuda, names, launcher(mean, bias), seam=Cg in (64, 256))
    ref, _, mass = R.gate_fc_forward(mean, w, bias)
    plain = R.gate_fc_expr(mean, w, bias)                                    # float32 addmm + sigmoid on the CPU
    assert torch.isfinite(got).all()
    excess = ((got.double() - ref).abs() - 0.25 * R.gamma(Cg) * mass).max().item()
    if Cg <= 2:
        FIG["gatefc_sigmoid"] = max(FIG.get("gatefc_sigmoid", 0.0), (got.double() - ref).abs().max().item())
        parity_record["detector_f64_gatefc_sigmoid"] = FIG["gatefc_sigmoid"]
    print(f"gate_fc_forward C={Cg} N={n}: |gate - f64| beyond gamma_C sum|t| / 4: {excess:.3e}")
    assert excess <= TAU_SIGMOID
    calibrated("gatefc_fwd", got, ref, plain, parity_record, 1.0, f"C={Cg} N={n} bias={with_bias}")
    for pos in sorted({0, Cg - 1}):                       # one-hot: a single term in front of the sigmoid, one rounding
        hot = hot_rows(mean, pos)
        got, = run(cuda, ("mean", "w", "gate"), launcher(hot, None))
        z = (w[:, pos].view(1, Cg) * hot[:, pos].view(n, 1)).double()
        assert ((got.double() - 1.0 / (1.0 + torch.exp(-z))).abs() <= TAU_SIGMOID).all(), pos


@pytest.mark.parametrize("blocks", [1, 2, 5])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("Cg", FC_C)
def test_gate_fc_backward(cuda, Cg, n, blocks):
    """m = blocks + C + 3 roundings on every term (see the module's docstring)."""
    partial = noise((n * Cg, blocks), 38, special=False)
    gate = torch.sigmoid(noise((n, Cg), 39, special=False, off=1))
    w = noise((Cg, Cg), 40, special=False, off=2) / math.sqrt(Cg)
    inv = 1.0 / 60.0

    def launcher(dp):
        def launch(p):
            out = p("g_mean", (n, Cg))
            ok("advstep_gate_fc_backward_f32", p("partial", dp), blocks, p("gate", gate), p("w", w), inv, out, n, Cg)
            return (out,)
        return launch

    names = ("partial", "gate", "w", "g_mean")
    got, = run(cuda, names, launcher(partial), seam=Cg in (64, 256) and blocks == 2)
    ref, mass = R.gate_fc_backward(partial, gate, w, inv)
    within(got, ref, blocks + Cg + 3, mass, (Cg, n, blocks), amp=max(1.0, w.abs().max().item()))
    inv32 = torch.tensor(inv, dtype=F32)
    for k in sorted({0, Cg - 1}):                         # one-hot: one channel's last block
        hot = torch.zeros_like(partial)
        hot.view(n, Cg, blocks)[:, k, blocks - 1] = partial.view(n, Cg, blocks)[:, k, blocks - 1] + 3.0
        got, = run(cuda, names, launcher(hot))
        t = (hot.view(n, Cg, blocks)[:, k, blocks - 1] * gate[:, k]) * (1.0 - gate[:, k])
        assert torch.equal(got, (t.view(n, 1) * w[k].view(1, Cg)) * inv32), k


# ---- refused calls ----------------------------------------------------------------------------------------------------------------------------

def test_refused_calls_return_before_any_launch(cuda):
    """Each call is refused with ADVSTEP_EINVAL and leaves its (fully sized) outputs canary."""
    L = 16
    dev = lambda t: t.to(cuda)
    x, v = dev(noise((N, C, L), 41)), dev(SCALE)
    rowsx = dev(noise((N * C, L), 42))
    big = dev(torch.zeros(1, R.ROW_CAP + 1))
    m, wfc = dev(noise((1, 257), 43, special=False)), dev(torch.zeros(257, 257))
    outs = []

    def out(shape, dtype=F32):
        fill = CANARY if dtype == F32 else 0xA5
        outs.append((torch.full(shape, fill, dtype=dtype, device=cuda), fill))
        return outs[-1][0]

    u8 = torch.uint8
    sel = torch.zeros((N, C, L), dtype=u8, device=cuda)
    assert abi()[0].advstep_log_meannorm_max_length() == R.ROW_CAP
    refused = [
        call("advstep_affine_act_forward_f32", x, v, v, v, out(x.shape), N, C, L, 3, 0.3),
        call("advstep_affine_act_backward_f32", x, x, v, v, v, out(x.shape), N, C, L, 3, 0.3),
        call("advstep_affine_act_forward_f32", None, v, v, v, out(x.shape), N, C, L, 0, 0.3),
        call("advstep_afms_row_f32", 4, rowsx, rowsx, v, v, v, out(rowsx.shape), N * C, C, L),
        call("advstep_afms_row_f32", 1, rowsx, None, None, rowsx, None, out(rowsx.shape), N * C, C, L),
        call("advstep_add_maxpool2_forward_f32", x.view(N, C, 4, 4), None, None, out((N, C, 2, 2)), None, N, C, 4, 4),
        call("advstep_weighted_stats_forward_f32", rowsx, rowsx, None, out((N * C,)), N * C, L),
        call("advstep_log_meannorm_forward_f32", big, 1e-6, out(big.shape), 1, R.ROW_CAP + 1),
        call("advstep_log_meannorm_backward_f32", big, big, 1e-6, out(big.shape), 1, R.ROW_CAP + 1),
        call("advstep_gate_fc_forward_f32", m, wfc, None, out((1, 257)), 1, 257),
        call("advstep_gate_fc_forward_f32", m, wfc, None, out((1, 257)), 1, 0),
        call("advstep_gate_fc_forward_f32", m, None, None, out((1, 256)), 1, 256),
        call("advstep_gate_fc_backward_f32", m, 1, m, wfc, 1.0, out((1, 257)), 1, 257),
        call("advstep_gate_fc_backward_f32", m, 1, m, wfc, 1.0, out((1, 257)), 1, 0),
    ]
    for k in (1, 9):
        refused += [
            call("advstep_add_maxpool1d_forward_f32", x, None, out(x.shape), out(x.shape, u8), N, C, L, k),
            call("advstep_maxpool1d_backward_f32", x, sel, out(x.shape), N, C, L, k),
            call("advstep_tail_pool1d_forward_f32", x, x, v, v, v, out(x.shape), out(x.shape, u8), N, C, L, k),
            call("advstep_tail_pool1d_backward_f32", x, sel, x, v, v, out(x.shape), out(x.shape), N, C, L, k),
        ]
    refused.append(call("advstep_tail_pool1d_forward_f32", x, None, v, v, v, out((N, C, L // 2)), out((N, C, L // 2), u8), N, C, L, 2))
    torch.cuda.synchronize()
    assert refused == [EINVAL] * len(refused), refused
    assert all(bool((t == fill).all()) for t, fill in outs)
