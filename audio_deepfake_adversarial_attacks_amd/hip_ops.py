"""Torch-facing wrappers of the C ABI (include/advstep.h): device tensors in, raw pointers + HIP stream out.

PyTorch is used for plumbing only — device memory, the current HIP stream, autograd around the model.  Every
function requires contiguous float32 tensors that live on a HIP device and launches on torch's *current*
stream of that device, so the kernels are ordered with the model's forward/backward work without any
synchronisation.  There is NO CPU path here: a CPU tensor, a missing libadvstep.so or a non-zero status
raises.

Reference op chains replaced (see the header for line-by-line citations):
  to_minmax / revert_minmax          src/aa/utils.py:4-14
  fgsm_step                          adversarial_attacks/torchattacks/attacks/fgsm.py:59-60
  pgd_linf_init / pgd_linf_step      .../attacks/pgd.py:54-57, 74-76
  pgd_l2_init / pgd_l2_step          .../attacks/pgdl2.py:55-62, 78-88
  cw_*                               .../attacks/cw.py:57, 72-77, 87-103
  ce2_loss_grad                      .../attacks/pgd.py:62,50,68 (and the same lines of fgsm.py / pgdl2.py)
  mi_step / vt_*                     .../attacks/mifgsm.py:70-76, nifgsm.py:56,67-71, vmifgsm.py:77-101
  multi_route                        .../attacks/multiattack.py:55-66
  perturbation_stats                 src/aa/qualitative/attacks_postanalysis.py (the distortion figures beside the WAV pairs)
  row_pgd_*_step / radius_*          no counterpart: the per-row radius steps and the bisection of torchattacks.MinRadiusPGD
  l1_box_project / apgdl1_*          no counterpart: l1-APGD (Croce & Hein, ICML 2021), torchattacks.APGDL1
  l0_box_project / pgdl0_step        no counterpart: PGD0 (Croce & Hein, ICCV 2019), torchattacks.PGDL0
  seg_pgd_step / snr_row_radius      no counterpart: PGD under an SNR or segmental-SNR budget, torchattacks.PGDSNR
  universal_colsum / universal_apply no counterpart: one perturbation for every utterance, torchattacks.UniversalPGD
  spsa_probe / spsa_step             no counterpart: the score-based black-box attack, torchattacks.SPSA
  hsj_search_* / hsj_probe / hsj_candidates / hsj_take  no counterpart: the label-only black-box attack, torchattacks.HopSkipJump
  channel_apply / _adjoint / _eot_step  no counterpart: the simulated audio channel of torchattacks.Channel / EOTPGD
  stft_power / masking_hinge_grad / psy_step  no counterpart: the psychoacoustic masking hinge of torchattacks.PsyPGD
  smooth_noise / smooth_tally        no counterpart: the noisy copies and the votes of torchattacks.Smoothing
  smoothadv_fill / _loss_grad / _step  no counterpart: PGD on the smoothed detector's soft vote, torchattacks.SmoothAdvPGD
  fmn_begin / fmn_norms / fmn_step   no counterpart: Fast Minimum-Norm (Pintor et al., NeurIPS 2021), torchattacks.FMN
  fmn_sparse_step                    no counterpart: its L1 and L0 forms in one fused row launch, torchattacks.FMNSparse
  filter_apply / _tap_grad / _tap_update  no counterpart: one adversarial FIR filter for every utterance, torchattacks.UniversalFilter
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch

from . import _lib
from .metrics import PERTURBATION_PLANES  # noqa: F401  (re-exported: the planes of perturbation_stats)

NAME = "hip"

# ---------------------------------------------------------------------------------------------------------
# plumbing
# ---------------------------------------------------------------------------------------------------------

_workspaces: Dict[tuple, torch.Tensor] = {}     # (device, stream handle, B, T) -> row-reduction scratch; (..., "perturb") -> perturbation_stats' partials
_profile: Optional[Dict[str, List[Tuple[torch.cuda.Event, torch.cuda.Event]]]] = None
_profile_work: Dict[str, List[float]] = {}      # per bracketed launch: the arithmetic the caller says it did (flop), or 0
_profile_bytes: Dict[str, List[float]] = {}     # per bracketed launch: the bytes of the operands the caller named, or 0
_profile_all = False                            # start_profile("*"): every entry point
_profile_graph_ok = False                       # start_profile(..., graph_ok=True): only launches OUTSIDE captured graphs matter
_launch_depth = 0                               # > 0 while a bracketed launch is being issued (bench.py's library-op brackets skip what is inside)


def _require(t: torch.Tensor, name: str, dtype=torch.float32) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise _lib.AdvstepError(
            f"{name}: tensor lives on '{t.device}'. The attack kernels run only on a HIP device "
            "(there is no CPU fallback in this package; the CPU restatement is the test-only oracle/ tree).")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: tensor must be contiguous")
    return t


def _same_shape(*named) -> None:
    first_name, first = named[0]
    for name, t in named[1:]:
        if t.shape != first.shape or t.device != first.device:
            raise ValueError(f"{name} {tuple(t.shape)}@{t.device} does not match {first_name} "
                             f"{tuple(first.shape)}@{first.device}")


def _rows(t: torch.Tensor, name: str) -> Tuple[int, int]:
    if t.dim() < 2:
        raise ValueError(f"{name}: expected (B, ...) with at least 2 dims, got {tuple(t.shape)}")
    B = t.shape[0]
    return B, (t.numel() // B if B else 0)


def _stream(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


_WORKSPACE_SLOTS = 32      # bound of the scratch table: distinct (device, stream, B, T) kept alive at once


def _workspace(device: torch.device, B: int, T: int) -> Tuple[int, int]:
    # one scratch per (device, stream, batch shape): the layout of the single-pass PGD-L2 exchange area depends on (B, T), and a
    # buffer that only ever sees one shape and one stream never shows a call words another layout or another stream's call left
    # behind (include/advstep.h).  The table is a small LRU: variable-length clips or short last batches
    # would otherwise add a zero-filled buffer per distinct shape for the life of the process.  Evicting is safe: the tensor
    # was allocated and only ever used on the stream of its key, so the caching allocator re-issues its memory in stream order;
    # a captured graph OWNS the buffers it baked in (`release_stream_workspaces`), they are not in this table any more.
    key = (device.index if device.index is not None else torch.cuda.current_device(), _stream(device), int(B), int(T))
    # zero-filled ONCE: epoch 0, no row flagged (include/advstep.h)
    return _scratch(key, lambda: torch.zeros(max(_lib.load().advstep_row_workspace_bytes(B, T), 256), dtype=torch.uint8,
                                             device=device))


def _scratch(key: tuple, alloc) -> Tuple[int, int]:
    """The table's buffer of `key` = (device, stream handle, ...) as (pointer, bytes), allocated by `alloc` on a miss."""
    ws = _workspaces.pop(key, None)
    if ws is None:
        ws = alloc()
        while len(_workspaces) >= _WORKSPACE_SLOTS:
            _workspaces.pop(next(iter(_workspaces)))                 # least recently used first (dicts keep insertion order)
    _workspaces[key] = ws                                            # (re-)inserted last = most recently used
    return ws.data_ptr(), ws.numel()


def release_stream_workspaces(stream_handle: int) -> list:
    """Hand over — and forget — every scratch buffer keyed by `stream_handle`.  A captured graph calls this right after its
    capture: the graph replays kernels that write to these ADDRESSES, so it must own the buffers, and an eager call on a stream
    that torch later gives the same handle (its pool is round-robin) must NOT get the same buffer — two streams sharing one
    workspace is outside the C ABI's contract (the exchange's call counter is advanced by a plain read-modify-write)."""
    keys = [k for k in _workspaces if k[1] == stream_handle]
    return [_workspaces.pop(k) for k in keys]


def _out_like(ref: torch.Tensor, out: Optional[torch.Tensor], name: str = "out") -> torch.Tensor:
    if out is None:
        return torch.empty_like(ref, memory_format=torch.contiguous_format)
    _require(out, name)
    _same_shape(("input", ref), (name, out))
    return out


class _Launch:
    """Device guard + optional HIP-event bracket around one C-ABI call (events sit on the launch stream).  `work` = the
    floating-point operations the launch must do — for the Winograd F(2x2, 3x3) kernels what goes through the matrix cores: 2 x 16
    products per 2x2 output tile, output row and reduction channel = a direct 3x3 convolution's count / 2.25, unpadded;
    `tensors` = the operands the launch reads or writes once (its algorithmic HBM bytes = the sum of their sizes).  Both are
    kept next to the bracket's duration for bench.py's rooflines (`roofline_model`, `roofline_step`)."""

    def __init__(self, name: str, device: torch.device, work: float = 0.0, tensors=()):
        self.name, self.device, self.work = name, device, work
        self.nbytes = float(sum(t.numel() * t.element_size() for t in tensors if t is not None)) if tensors else 0.0
        self.guard = torch.cuda.device(device)

    def __enter__(self):
        global _launch_depth
        _launch_depth += 1
        self.guard.__enter__()
        self.pair = None
        if (_profile is not None and (_profile_all or self.name in _profile)
                and not torch.cuda.is_current_stream_capturing()):       # an event cannot be recorded into a graph
            self.pair = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            self.pair[0].record(torch.cuda.current_stream(self.device))
        return self

    def __exit__(self, *exc):
        global _launch_depth
        _launch_depth -= 1
        if self.pair is not None:
            self.pair[1].record(torch.cuda.current_stream(self.device))
            _profile.setdefault(self.name, []).append(self.pair)
            _profile_work.setdefault(self.name, []).append(self.work)
            _profile_bytes.setdefault(self.name, []).append(self.nbytes)
        return self.guard.__exit__(*exc)


def _call(symbol: str, device: torch.device, *args, bracket: Optional[str] = None, work: float = 0.0, tensors=()) -> None:
    """The one way into a status-returning entry point of the C ABI: `symbol` (its full name, given once) is called with
    `args` — a tensor as its address, None as a null pointer, anything else as it is — and torch's current stream of `device`
    as the last argument; a non-zero status raises under that name.  `bracket`: the call runs inside `_Launch(bracket, device,
    work, tensors)`; None: no guard and no events (the caller holds a bracket of its own, or the call never had one)."""
    if bracket is not None:
        with _Launch(bracket, device, work, tensors):
            return _call(symbol, device, *args)
    status = getattr(_lib.load(), symbol)(*[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args], _stream(device))
    _lib.check(status, symbol)


def _on_device(t: torch.Tensor, name: str, device: torch.device) -> None:
    if t.device != device:
        raise ValueError(f"{name} must live on {device}, got {t.device}")


def _stacked_out(out: Optional[torch.Tensor], n: int, like: torch.Tensor) -> torch.Tensor:
    """`out`, or a fresh (n, *like.shape) tensor: n stacked copies' worth of float32 values on like's device."""
    if out is None:
        out = torch.empty((n,) + tuple(like.shape), dtype=torch.float32, device=like.device)
    _require(out, "out")
    if out.numel() != n * like.numel() or out.device != like.device:
        B, T = _rows(like, "input")
        raise ValueError(f"out must hold ({n}, {B}, {T}) values on {like.device}, got {tuple(out.shape)}@{out.device}")
    return out


def _shaped(t: Optional[torch.Tensor], name: str, shape: tuple, device: torch.device) -> torch.Tensor:
    """`t`, or a fresh float32 tensor when it is None: exactly `shape`, on `device`."""
    if t is None:
        return torch.empty(shape, dtype=torch.float32, device=device)
    _require(t, name)
    if tuple(t.shape) != tuple(shape) or t.device != device:
        raise ValueError(f"{name} must be {tuple(shape)} on {device}, got {tuple(t.shape)}@{t.device}")
    return t


def start_profile(*entry_points: str, graph_ok: bool = False) -> None:
    """Bracket every later launch of the named entry points ("*": of every entry point) with HIP events on their launch
    stream.  graph_ok: the caller prices launches that stay OUTSIDE the attacks' captured graphs (the update steps,
    min-max, random starts) and the iteration may keep replaying its model part from a hipGraph (torchattacks/graphed.py);
    without it profiling keeps the whole loop eager so that launches of the model part can be bracketed too."""
    global _profile, _profile_all, _profile_graph_ok
    _profile_graph_ok = bool(graph_ok)
    _profile_all = "*" in entry_points
    _profile = {n: [] for n in entry_points if n != "*"}
    _profile_work.clear()
    _profile_bytes.clear()


def stop_profile(with_work=False):
    """Synchronise and return {entry point: [milliseconds per launch]}; with_work: also {entry point: [flop per launch]};
    with_work="bytes": also {entry point: [algorithmic bytes per launch]} as a third result."""
    global _profile, _profile_all, _profile_graph_ok
    prof, _profile, _profile_all, _profile_graph_ok = _profile or {}, None, False, False
    torch.cuda.synchronize()
    ms = {n: [a.elapsed_time(b) for a, b in pairs] for n, pairs in prof.items()}
    if with_work == "bytes":
        return (ms, {n: list(_profile_work.get(n, [])) for n in prof}, {n: list(_profile_bytes.get(n, [])) for n in prof})
    if with_work:
        return ms, {n: list(_profile_work.get(n, [])) for n in prof}
    return ms


# ---------------------------------------------------------------------------------------------------------
# a1 / a2
# ---------------------------------------------------------------------------------------------------------

def to_minmax(batch_x: torch.Tensor):
    """src/aa/utils.py:4-9 — returns (x01 (B,T), mn (B,1), mx (B,1))."""
    x = _require(batch_x, "batch_x")
    B, T = _rows(x, "batch_x")
    x01 = torch.empty_like(x)
    mn = torch.empty((B, 1), dtype=torch.float32, device=x.device)
    mx = torch.empty((B, 1), dtype=torch.float32, device=x.device)
    with _Launch("minmax_normalize", x.device, tensors=(x, x, x01)):
        ws, ws_bytes = _workspace(x.device, B, T)
        _call("advstep_minmax_normalize_f32", x.device, x, x01, mn, mx, B, T, ws, ws_bytes)
    return x01, mn, mx


def revert_minmax(batch_x: torch.Tensor, mn: torch.Tensor, mx: torch.Tensor, out: Optional[torch.Tensor] = None):
    """src/aa/utils.py:12-14."""
    x = _require(batch_x, "batch_x")
    B, T = _rows(x, "batch_x")
    _require(mn, "mn"), _require(mx, "mx")
    if mn.numel() != B or mx.numel() != B:
        raise ValueError(f"mn/mx must hold one value per row ({B}), got {mn.numel()} / {mx.numel()}")
    out = _out_like(x, out)
    _call("advstep_minmax_revert_f32", x.device, x, mn, mx, out, B, T, bracket="minmax_revert", tensors=(x, out))
    return out


# ---------------------------------------------------------------------------------------------------------
# a4 / a5
# ---------------------------------------------------------------------------------------------------------

def fgsm_step(x, grad, eps: float, lo: float = 0.0, hi: float = 1.0, out=None):
    _require(x, "x"), _require(grad, "grad")
    _same_shape(("x", x), ("grad", grad))
    out = _out_like(x, out)
    _call("advstep_fgsm_step_f32", x.device, x, grad, out, x.numel(), eps, lo, hi, bracket="fgsm_step", tensors=(x, grad, out))
    return out


def pgd_linf_init(x, eps: float, noise=None, seed: Optional[int] = None, offset: int = 0, lo: float = 0.0,
                  hi: float = 1.0, out=None):
    """Random start of pgd.py:54-57.  `noise` (the caller's U(-eps, eps) draw) or a Philox `seed`."""
    _require(x, "x")
    out = _out_like(x, out)
    if noise is not None:
        _require(noise, "noise")
        _same_shape(("x", x), ("noise", noise))
        _call("advstep_pgd_linf_init_noise_f32", x.device, x, noise, out, x.numel(), lo, hi,
              bracket="pgd_linf_init", tensors=(x, noise, out))
    else:
        if seed is None:
            raise ValueError("pgd_linf_init needs either `noise` or a Philox `seed`")
        _call("advstep_pgd_linf_init_philox_f32", x.device, x, out, x.numel(), eps, lo, hi, seed, offset,
              bracket="pgd_linf_init", tensors=(x, out))
    return out


def pgd_linf_step(adv, grad, orig, alpha: float, eps: float, lo: float = 0.0, hi: float = 1.0, out=None):
    _require(adv, "adv"), _require(grad, "grad"), _require(orig, "orig")
    _same_shape(("adv", adv), ("grad", grad), ("orig", orig))
    out = _out_like(adv, out)
    _call("advstep_pgd_linf_step_f32", adv.device, adv, grad, orig, out, adv.numel(), alpha, eps, lo, hi,
          bracket="pgd_linf_step", tensors=(adv, grad, orig, out))
    return out


# ---------------------------------------------------------------------------------------------------------
# a6
# ---------------------------------------------------------------------------------------------------------

def pgd_l2_init(x, eps: float, draws=None, seed: Optional[int] = None, offset: int = 0, lo: float = 0.0,
                hi: float = 1.0, out=None):
    """Random start of pgdl2.py:55-62.  `draws` = (normal (B,T), r (B)) or a Philox `seed`."""
    _require(x, "x")
    B, T = _rows(x, "x")
    out = _out_like(x, out)
    with _Launch("pgd_l2_init", x.device, tensors=(x, out)):
        ws, ws_bytes = _workspace(x.device, B, T)
        if draws is not None:
            normal, r = draws
            _require(normal, "normal"), _require(r, "r")
            _same_shape(("x", x), ("normal", normal))
            if r.numel() != B:
                raise ValueError(f"r must hold one value per row ({B}), got {r.numel()}")
            _call("advstep_pgd_l2_init_noise_f32", x.device, x, normal, r, out, B, T, eps, lo, hi, ws, ws_bytes)
        else:
            if seed is None:
                raise ValueError("pgd_l2_init needs either `draws` or a Philox `seed`")
            _call("advstep_pgd_l2_init_philox_f32", x.device, x, out, B, T, eps, lo, hi, seed, offset, ws, ws_bytes)
    return out


def pgd_l2_step(adv, grad, orig, alpha: float, eps: float, eps_div: float = 1e-10, lo: float = 0.0, hi: float = 1.0,
                out=None, return_norms: bool = False):
    _require(adv, "adv"), _require(grad, "grad"), _require(orig, "orig")
    _same_shape(("adv", adv), ("grad", grad), ("orig", orig))
    B, T = _rows(adv, "adv")
    out = _out_like(adv, out)
    gn = dn = None
    if return_norms:
        gn = torch.empty(B, dtype=torch.float32, device=adv.device)
        dn = torch.empty(B, dtype=torch.float32, device=adv.device)
    with _Launch("pgd_l2_step", adv.device, tensors=(adv, grad, orig, out)):
        ws, ws_bytes = _workspace(adv.device, B, T)
        _call("advstep_pgd_l2_step_f32", adv.device, adv, grad, orig, out, B, T, alpha, eps, eps_div, lo, hi, gn, dn, ws, ws_bytes)
    return (out, gn, dn) if return_norms else out


def pgd_l2_repaired_rows(like: torch.Tensor) -> int:
    """Diagnostics (synchronises): how many rows of the LAST single-pass pgd_l2_step / pgd_l2_init call on this device and
    stream were recomputed by the repair kernel because their in-launch norm exchange was abandoned (include/advstep.h)."""
    _require(like, "like")
    B, T = _rows(like, "like")
    count = torch.zeros(1, dtype=torch.int32, device=like.device)
    with torch.cuda.device(like.device):
        ws, ws_bytes = _workspace(like.device, B, T)
        _call("advstep_pgd_l2_repaired_rows", like.device, ws, ws_bytes, B, T, count)
    return int(count.item())


# ---------------------------------------------------------------------------------------------------------
# a7
# ---------------------------------------------------------------------------------------------------------

def cw_init_w(x, out=None):
    _require(x, "x")
    out = _out_like(x, out)
    _call("advstep_cw_init_w_f32", x.device, x, out, x.numel(), bracket="cw_init_w", tensors=(x, out))
    return out


def cw_tanh_sqdist(w, x, adv_out=None):
    """Returns (adv = 1/2 (tanh w + 1), l2 (B) = row sums of (adv - x)^2)."""
    _require(w, "w"), _require(x, "x")
    _same_shape(("w", w), ("x", x))
    B, T = _rows(w, "w")
    adv = _out_like(w, adv_out, "adv_out")
    l2 = torch.empty(B, dtype=torch.float32, device=w.device)
    with _Launch("cw_tanh_sqdist", w.device, tensors=(w, x, adv)):
        ws, ws_bytes = _workspace(w.device, B, T)
        _call("advstep_cw_tanh_sqdist_f32", w.device, w, x, adv, l2, B, T, ws, ws_bytes)
    return adv, l2


def cw_adam_step(w, m, v, x, grad_adv, step: int, lr: float = 0.01, beta1: float = 0.9, beta2: float = 0.999,
                 adam_eps: float = 1e-8) -> None:
    """In-place Adam step on (w, m, v); `step` is 1-based."""
    for name, t in (("w", w), ("m", m), ("v", v), ("x", x), ("grad_adv", grad_adv)):
        _require(t, name)
    _same_shape(("w", w), ("m", m), ("v", v), ("x", x), ("grad_adv", grad_adv))
    _call("advstep_cw_adam_step_f32", w.device, w, m, v, x, grad_adv, w.numel(), step, lr, beta1, beta2, adam_eps,
          bracket="cw_adam_step", tensors=(w, w, m, m, v, v, x, grad_adv))


def cw_best_update(adv, mask, best) -> None:
    """In place: best = mask * adv + (1 - mask) * best, mask (B) float32 in {0, 1}."""
    _require(adv, "adv"), _require(mask, "mask"), _require(best, "best")
    _same_shape(("adv", adv), ("best", best))
    B, T = _rows(adv, "adv")
    if mask.numel() != B:
        raise ValueError(f"mask must hold one value per row ({B}), got {mask.numel()}")
    _call("advstep_cw_best_update_f32", adv.device, adv, mask, best, B, T, bracket="cw_best_update", tensors=(adv, best, best))


# ---------------------------------------------------------------------------------------------------------
# a8
# ---------------------------------------------------------------------------------------------------------

def ce2_loss_grad(z, labels, scale: float = 1.0):
    """CE(cat([-z, z], 1), labels) (mean) in closed form: returns (d cost / d z shaped like z, cost (1,))."""
    _require(z, "z")
    _require(labels, "labels", torch.int64)
    B = z.numel()
    if labels.numel() != B:
        raise ValueError(f"labels must hold one value per logit ({B}), got {labels.numel()}")
    dz = torch.empty_like(z)
    loss = torch.empty(1, dtype=torch.float32, device=z.device)
    _call("advstep_ce2_loss_grad_f32", z.device, z, labels, dz, loss, B, scale, bracket="ce2_loss_grad")
    return dz, loss


# ---------------------------------------------------------------------------------------------------------
# f3: FAB (include/advstep_fab.h; reference adversarial_attacks/torchattacks/attacks/fab.py:208-292, 562-717)
# ---------------------------------------------------------------------------------------------------------

FAB_NORMS = {"Linf": 0, "L2": 1, "L1": 2}


def _fab_kind(norm: str) -> int:
    try:
        return FAB_NORMS[norm]
    except KeyError:
        raise ValueError("norm not supported") from None    # fab.py:224


def fab_hyperplane(gz, x, z=None, labels=None, norm: str = "Linf"):
    """Row statistics of the logit gradient + the closest-boundary selection for cat([-z, z]) (fab.py:90-112, 210-229).
    Returns (wscale, b, gnorm, gdot), each (B); wscale / b are None when z / labels are not given."""
    _require(gz, "gz"), _require(x, "x")
    _same_shape(("gz", gz), ("x", x))
    B, T = _rows(gz, "gz")
    dev = gz.device
    gnorm, gdot = torch.empty(B, device=dev), torch.empty(B, device=dev)
    wscale = b = None
    if z is not None:
        _require(z, "z"), _require(labels, "labels", torch.int64)
        if z.numel() != B or labels.numel() != B:
            raise ValueError(f"z / labels must hold one value per row ({B})")
        wscale, b = torch.empty(B, device=dev), torch.empty(B, device=dev)
    else:
        labels = None                            # the selection's four operands go in together or not at all
    _call("advstep_fab_hyperplane_f32", dev, gz, x, z, labels, wscale, b, gnorm, gdot, B, T, _fab_kind(norm),
          bracket="fab_hyperplane")
    return wscale, b, gnorm, gdot


def fab_projection(points, w, b, norm: str = "Linf", wscale=None, out=None):
    """projection_{linf,l2,l1}(points, w, b) (fab.py:562-717) for R rows: returns (d (R, T), its attack norm (R)).
    w may hold fewer rows than points (R % w_rows == 0): row r uses w[r % w_rows] * wscale[r % w_rows]."""
    _require(points, "points"), _require(w, "w"), _require(b, "b")
    R, _ = _rows(points, "points")
    w_rows, _ = _rows(w, "w")
    T, Tw = points[0].numel() if R else w.shape[1:].numel(), w.shape[1:].numel()
    if Tw != T or w_rows == 0 or R % w_rows or b.numel() != R or w.device != points.device:
        raise ValueError(f"points {tuple(points.shape)}, w {tuple(w.shape)}, b {tuple(b.shape)} do not line up")
    if wscale is not None:
        _require(wscale, "wscale")
        if wscale.numel() != w_rows:
            raise ValueError(f"wscale must hold one value per row of w ({w_rows})")
    d = _out_like(points, out, "out")
    dnorm = torch.empty(R, device=points.device)
    _call("advstep_fab_projection_f32", points.device, points, w, wscale, b, d, dnorm, R, w_rows, T, _fab_kind(norm),
          bracket="fab_projection")
    return d, dnorm


def fab_combine(x1, x0, d1, d2, n1, n2, eta: float, alpha_max: float, out=None):
    """clamp((x1 + eta d1)(1 - alpha) + (x0 + eta d2) alpha, 0, 1), alpha from the two move norms (fab.py:257-267)."""
    for name, t in (("x1", x1), ("x0", x0), ("d1", d1), ("d2", d2), ("n1", n1), ("n2", n2)):
        _require(t, name)
    _same_shape(("x1", x1), ("x0", x0), ("d1", d1), ("d2", d2))
    B, T = _rows(x1, "x1")
    if n1.numel() != B or n2.numel() != B:
        raise ValueError(f"n1 / n2 must hold one value per row ({B})")
    res = _out_like(x1, out, "out")
    _call("advstep_fab_combine_f32", x1.device, x1, x0, d1, d2, n1, n2, res, B, T, eta, alpha_max, bracket="fab_combine")
    return res


def fab_backward_step(x1, x0, adv, res2, is_adv, beta: float, norm: str = "Linf") -> None:
    """In place, rows with is_adv != 0: keep the closest adversarial point so far, then step back towards the clean
    point by beta (fab.py:271-290).  is_adv (B) uint8 or bool."""
    _require(x1, "x1"), _require(x0, "x0"), _require(adv, "adv"), _require(res2, "res2")
    _same_shape(("x1", x1), ("x0", x0), ("adv", adv))
    B, T = _rows(x1, "x1")
    if is_adv.dtype == torch.bool:
        is_adv = is_adv.view(torch.uint8)
    _require(is_adv, "is_adv", torch.uint8)
    if res2.numel() != B or is_adv.numel() != B:
        raise ValueError(f"res2 / is_adv must hold one value per row ({B})")
    _call("advstep_fab_backward_step_f32", x1.device, x1, x0, adv, res2, is_adv, B, T, beta, _fab_kind(norm),
          bracket="fab_backward_step")


# ---------------------------------------------------------------------------------------------------------
# APGD (include/advstep_apgd.h; reference adversarial_attacks/torchattacks/attacks/apgd.py:81-213)
# ---------------------------------------------------------------------------------------------------------

APGD_NORMS = {"Linf": 0, "L2": 1}
_APGD_MODES = {"grad": 0, "start": 1, "step": 2}


def _apgd_norm(norm: str) -> int:
    try:
        return APGD_NORMS[norm]
    except KeyError:
        raise ValueError(f"APGD norm must be 'Linf' or 'L2', got {norm!r}") from None


def _per_row(t: torch.Tensor, name: str, B: int, dtype=torch.float32, device=None) -> torch.Tensor:
    _require(t, name, dtype)
    if t.numel() != B:
        raise ValueError(f"{name} must hold one value per row ({B}), got {t.numel()}")
    if device is not None:
        _on_device(t, name, device)
    return t


def _optional_rows(t: Optional[torch.Tensor], name: str, B: int, device) -> Optional[torch.Tensor]:
    """One float32 value per row, (B,) or (B, 1), on `device` — or None, which the library takes as a null pointer."""
    return None if t is None else _per_row(t, name, B, device=device)


def apgd_init(x, eps: float, norm: str = "Linf", draw=None, seed: Optional[int] = None, offset: int = 0,
              lo: float = 0.0, hi: float = 1.0, out=None):
    """Random start of apgd.py:89-95.  `draw` = the caller's (B, T) draw (U[0, 1) for L-inf, N(0, 1) for L2) or a Philox
    `seed`."""
    _require(x, "x")
    B, T = _rows(x, "x")
    kind = _apgd_norm(norm)
    out = _out_like(x, out)
    with _Launch("apgd_init", x.device, tensors=(x, draw, out)):
        ws, ws_bytes = _workspace(x.device, B, T)
        if draw is not None:
            _require(draw, "draw")
            _same_shape(("x", x), ("draw", draw))
            _call("advstep_apgd_init_noise_f32", x.device, x, draw, out, B, T, kind, eps, lo, hi, ws, ws_bytes)
        else:
            if seed is None:
                raise ValueError("apgd_init needs either `draw` or a Philox `seed`")
            _call("advstep_apgd_init_philox_f32", x.device, x, out, B, T, kind, eps, lo, hi, seed, offset, ws, ws_bytes)
    return out


def apgd_eval(z, labels, state=None, mode: str = "grad", i: int = 0):
    """Per-row loss of cat([-z, z], 1), d(sum of losses)/dz and, for mode 'start' / 'step', the update of the per-row state
    (`state`: acc, flags, loss_best, loss_best_last_check, reduced_last_check, loss_steps; see include/advstep_apgd.h).
    Returns (dz shaped like z, loss (B))."""
    _require(z, "z")
    B = z.numel()
    _per_row(labels, "labels", B, torch.int64)
    m = _APGD_MODES[mode]
    dz = torch.empty_like(z)
    loss = torch.empty(B, dtype=torch.float32, device=z.device)
    rows = [None] * 6                            # mode 'grad': no state, six null pointers
    if m:
        rows = [_per_row(getattr(state, name), name, B, dt)
                for name, dt in (("acc", torch.uint8), ("flags", torch.uint8), ("loss_best", torch.float32),
                                 ("loss_best_last_check", torch.float32), ("reduced_last_check", torch.uint8))]
        _require(state.loss_steps, "loss_steps")
        if state.loss_steps.dim() != 2 or state.loss_steps.shape[1] != B or not 0 <= i < state.loss_steps.shape[0]:
            raise ValueError(f"loss_steps {tuple(state.loss_steps.shape)} has no row {i} of {B} losses")
        rows.append(state.loss_steps)
    acc, flags, best, last_check, reduced, steps = rows
    _call("advstep_apgd_eval_f32", z.device, z, labels, dz, loss, m, i, acc, flags, best, last_check, reduced, steps, B,
          bracket="apgd_eval")
    return dz, loss


def apgd_checkpoint(state, i: int, k: int, rho: float) -> None:
    """In place on `state`: the step-size checkpoint of apgd.py:194-211 after iteration i with window k."""
    B = state.loss_best.numel()
    _require(state.loss_steps, "loss_steps")
    steps = state.loss_steps.shape[0]
    for name, dt in (("loss_best", torch.float32), ("loss_best_last_check", torch.float32),
                     ("reduced_last_check", torch.uint8), ("step_size", torch.float32), ("flags", torch.uint8)):
        _per_row(getattr(state, name), name, B, dt)
    if state.loss_steps.shape != (steps, B) or not (0 <= i < steps and k >= 1 and i - k >= -1):
        raise ValueError(f"checkpoint at i={i}, k={k} does not fit loss_steps {tuple(state.loss_steps.shape)}")
    _call("advstep_apgd_checkpoint_f32", state.loss_best.device, state.loss_steps, steps, i, k, rho, state.loss_best,
          state.loss_best_last_check, state.reduced_last_check, state.step_size, state.flags, B, bracket="apgd_checkpoint")


def apgd_track(x_adv, grad, x_best, grad_best, x_best_adv, flags) -> None:
    """In place, flagged rows only: fooled -> x_best_adv = x_adv; improved -> x_best = x_adv, grad_best = grad;
    reset -> x_adv = x_best, grad = grad_best (apgd.py:178, 186-189, 207-208)."""
    named = (("x_adv", x_adv), ("grad", grad), ("x_best", x_best), ("grad_best", grad_best), ("x_best_adv", x_best_adv))
    for name, t in named:
        _require(t, name)
    _same_shape(*named)
    B, T = _rows(x_adv, "x_adv")
    _per_row(flags, "flags", B, torch.uint8)
    _call("advstep_apgd_track_f32", x_adv.device, x_adv, grad, x_best, grad_best, x_best_adv, flags, B, T, bracket="apgd_track")


def _apgd_step_args(cur, prev, grad, x, step_size):
    named = (("cur", cur), ("prev", prev), ("grad", grad), ("x", x))
    for name, t in named:
        _require(t, name)
    _same_shape(*named)
    B, T = _rows(cur, "cur")
    _per_row(step_size, "step_size", B)
    return B, T


def apgd_linf_step(cur, prev, grad, x, step_size, eps: float, a: float, out=None):
    """The L-inf momentum step of apgd.py:141-149; `out` may be `prev` (ping-pong)."""
    B, T = _apgd_step_args(cur, prev, grad, x, step_size)
    out = _out_like(cur, out)
    _call("advstep_apgd_linf_step_f32", cur.device, cur, prev, grad, x, step_size, out, B, T, eps, a,
          bracket="apgd_linf_step", tensors=(cur, prev, grad, x, out))
    return out


def apgd_l2_step(cur, prev, grad, x, step_size, eps: float, a: float, out=None, return_norms: bool = False):
    """The L2 momentum step of apgd.py:151-157; `out` may be `prev` (ping-pong).  return_norms: also (B, 3) =
    ||g||, ||x1 - x||, ||x2 - x|| per row."""
    B, T = _apgd_step_args(cur, prev, grad, x, step_size)
    out = _out_like(cur, out)
    norms = torch.empty((B, 3), dtype=torch.float32, device=cur.device)
    # compulsory traffic: grad x4, cur x3, x x3, prev x2, out x1 (four row passes that recompute rather than store)
    with _Launch("apgd_l2_step", cur.device, tensors=(grad,) * 4 + (cur,) * 3 + (x,) * 3 + (prev,) * 2 + (out,)):
        ws, ws_bytes = _workspace(cur.device, B, T)
        _call("advstep_apgd_l2_step_f32", cur.device, cur, prev, grad, x, step_size, out, norms, B, T, eps, a, ws, ws_bytes)
    return (out, norms) if return_norms else out


# ---------------------------------------------------------------------------------------------------------
# l1-APGD (include/advstep_apgdl1.h; Croce & Hein, "Mind the box", ICML 2021 — no counterpart in the reference tree).
# apgd_eval and apgd_track above serve it unchanged.
# ---------------------------------------------------------------------------------------------------------

def _positive_eps(eps: float) -> float:
    if not eps > 0:
        raise ValueError(f"the L1 radius must be positive, got {eps!r}")
    return eps


def l1_box_project(x, u, eps: float, out=None):
    """Euclidean projection of each row of u onto {z : ||z - x||_1 <= eps, 0 <= z <= 1} (x in [0, 1]); `out` may be `u`."""
    _require(x, "x"), _require(u, "u")
    _same_shape(("x", x), ("u", u))
    B, T = _rows(x, "x")
    out = _out_like(u, out)
    _call("advstep_l1_box_project_f32", x.device, x, u, out, _positive_eps(eps), B, T,
          bracket="l1_box_project", tensors=(x, u, out))
    return out


def apgdl1_init(x, eps: float, draw=None, seed: Optional[int] = None, offset: int = 0, out=None):
    """The random start of l1-APGD: the projection of x + t, t ~ N(0, 1) from the caller's (B, T) `draw` or a Philox `seed`
    (the normal stream of pgd_l2_init)."""
    _require(x, "x")
    B, T = _rows(x, "x")
    out = _out_like(x, out)
    with _Launch("apgdl1_init", x.device, tensors=(x, draw, out)):
        if draw is not None:
            _require(draw, "draw")
            _same_shape(("x", x), ("draw", draw))
            _call("advstep_apgdl1_init_f32", x.device, x, draw, out, B, T, _positive_eps(eps))
        else:
            if seed is None:
                raise ValueError("apgdl1_init needs either `draw` or a Philox `seed`")
            _call("advstep_apgdl1_init_philox_f32", x.device, x, out, B, T, _positive_eps(eps), seed, offset)
    return out


def apgdl1_step(cur, grad, x, step_size, topk, eps: float, out=None, return_stats: bool = False):
    """One l1-APGD iteration: the sign step on the coordinates whose |grad| reaches the row's top-k threshold, spread over
    their count, then the projection about x; `out` may be `cur`.  return_stats: also (B, 2) = threshold, count per row."""
    named = (("cur", cur), ("grad", grad), ("x", x))
    for name, t in named:
        _require(t, name)
    _same_shape(*named)
    B, T = _rows(cur, "cur")
    _per_row(step_size, "step_size", B), _per_row(topk, "topk", B)
    out = _out_like(cur, out)
    stats = torch.empty((B, 2), dtype=torch.float32, device=cur.device) if return_stats else None
    _call("advstep_apgdl1_step_f32", cur.device, cur, grad, x, step_size, topk, out, stats, B, T, _positive_eps(eps),
          bracket="apgdl1_step", tensors=(cur, grad, x, out))
    return (out, stats) if return_stats else out


def apgdl1_checkpoint(cur, x_best, x, state, eps: float) -> None:
    """In place on `state` (flags, sp_old, topk, step_size): the sparsity checkpoint of l1-APGD, from the best point including
    this iteration's improvement (`cur` where flags bit 1 is set, else `x_best`).  Call it before apgd_track."""
    named = (("cur", cur), ("x_best", x_best), ("x", x))
    for name, t in named:
        _require(t, name)
    _same_shape(*named)
    B, T = _rows(cur, "cur")
    for name, dt in (("flags", torch.uint8), ("sp_old", torch.float32), ("topk", torch.float32),
                     ("step_size", torch.float32)):
        _per_row(getattr(state, name), name, B, dt)
    _call("advstep_apgdl1_checkpoint_f32", cur.device, cur, x_best, x, state.flags, state.sp_old, state.topk,
          state.step_size, B, T, _positive_eps(eps), bracket="apgdl1_checkpoint", tensors=(cur, x))


# ---------------------------------------------------------------------------------------------------------
# the L0 threat model (include/advstep_l0.h): the exact-k projection and the PGD0 step of torchattacks.PGDL0
# ---------------------------------------------------------------------------------------------------------

def _l0_budget(k, eps_inf) -> Tuple[int, float]:
    if isinstance(k, bool) or int(k) != k or k < 1:
        raise ValueError(f"k must be an integer >= 1 (the samples an utterance may change), got {k!r}")
    if not eps_inf > 0:
        raise ValueError(f"the per-sample cap eps_inf must be positive (inf: none), got {eps_inf!r}")
    return int(k), float(eps_inf)


def l0_box_project(x, u, k: int, eps_inf: float = float("inf"), out=None):
    """Projection of each row of u onto {z : at most k samples differ from x, max(0, x - eps_inf) <= z <= min(1, x + eps_inf)}
    (x in [0, 1]): the k samples whose keeping saves most squared distance, ties to the lower index; `out` may be `u`."""
    _require(x, "x"), _require(u, "u")
    _same_shape(("x", x), ("u", u))
    B, T = _rows(x, "x")
    k, eps_inf = _l0_budget(k, eps_inf)
    out = _out_like(u, out)
    _call("advstep_l0_box_project_f32", x.device, x, u, out, k, eps_inf, B, T, bracket="l0_box_project", tensors=(x, u, out))
    return out


def pgdl0_step(cur, grad, x, step: float, k: int, eps_inf: float = float("inf"), out=None, return_stats: bool = False):
    """One PGD0 iteration: cur + step * grad / (||grad||_1 + 1e-10) per row, then `l0_box_project` about x; `out` may be `cur`.
    return_stats: also (B, 4) = the row's ||grad||_1, score threshold, scores above it, index of the last kept tie."""
    named = (("cur", cur), ("grad", grad), ("x", x))
    for name, t in named:
        _require(t, name)
    _same_shape(*named)
    B, T = _rows(cur, "cur")
    k, eps_inf = _l0_budget(k, eps_inf)
    if not step >= 0:
        raise ValueError(f"step must be non-negative, got {step!r}")
    out = _out_like(cur, out)
    stats = torch.empty((B, 4), dtype=torch.float32, device=cur.device) if return_stats else None
    _call("advstep_pgdl0_step_f32", cur.device, cur, grad, x, out, stats, step, k, eps_inf, B, T,
          bracket="pgdl0_step", tensors=(cur, grad, x, out))
    return (out, stats) if return_stats else out


# ---------------------------------------------------------------------------------------------------------
# momentum attacks (include/advstep_momentum.h; reference .../attacks/mifgsm.py:70-76, nifgsm.py:56,67-71,
# vmifgsm.py:77-101, vnifgsm.py:65,78-102)
# ---------------------------------------------------------------------------------------------------------

def mi_step(adv, grad, orig, momentum, alpha: float, eps: float, decay: float, v=None, nes_out=None,
            nes_scale: float = 0.0, lo: float = 0.0, hi: float = 1.0, out=None, return_mean: bool = False):
    """One whole momentum update: a = grad (+ v); m' = a / mean_T |a| + momentum * decay (momentum IN PLACE);
    out = clamp(orig + clamp(adv + alpha * sign(m') - orig, -eps, eps), lo, hi); nes_out = out + nes_scale * m' when given.
    `out` may be `adv`.  return_mean: also the (B) row means of |a|."""
    named = [("adv", adv), ("grad", grad), ("orig", orig), ("momentum", momentum)]
    if v is not None:
        named.append(("v", v))
    if nes_out is not None:
        named.append(("nes_out", nes_out))
    for name, t in named:
        _require(t, name)
    _same_shape(*named)
    B, T = _rows(adv, "adv")
    out = _out_like(adv, out)
    gmean = torch.empty(B, dtype=torch.float32, device=adv.device) if return_mean else None
    # compulsory traffic: grad twice, momentum in and back, adv, orig, out (+ v twice, + nes_out)
    with _Launch("mi_step", adv.device, tensors=(grad, grad, momentum, momentum, adv, orig, out, v, v, nes_out)):
        ws, ws_bytes = _workspace(adv.device, B, T)
        _call("advstep_mi_step_f32", adv.device, adv, grad, v, orig, momentum, out, nes_out, B, T, alpha, eps, decay, nes_scale,
              lo, hi, gmean, ws, ws_bytes)
    return (out, gmean) if return_mean else out


def vt_neighbor(adv, bound: float, draw=None, seed: Optional[int] = None, offset: int = 0, out=None):
    """A variance-tuning neighbour of vmifgsm.py:84-85: adv + U(-bound, bound), not clamped.  `draw` (the caller's draw) or a
    Philox `seed`; neighbour j of iteration i of an attack call takes offset = i * N + j."""
    _require(adv, "adv")
    out = _out_like(adv, out)
    if draw is not None:
        _require(draw, "draw")
        _same_shape(("adv", adv), ("draw", draw))
        _call("advstep_vt_neighbor_noise_f32", adv.device, adv, draw, out, adv.numel(),
              bracket="vt_neighbor", tensors=(adv, draw, out))
    else:
        if seed is None:
            raise ValueError("vt_neighbor needs either `draw` or a Philox `seed`")
        _call("advstep_vt_neighbor_philox_f32", adv.device, adv, out, adv.numel(), bound, seed, offset,
              bracket="vt_neighbor", tensors=(adv, out))
    return out


def vt_accumulate(gv, g, first: bool) -> None:
    """In place: gv = g when `first` (the zero-filled accumulator of vmifgsm.py:82 plus g), else gv += g."""
    _require(gv, "gv"), _require(g, "g")
    _same_shape(("gv", gv), ("g", g))
    _call("advstep_vt_accumulate_f32", gv.device, gv, g, gv.numel(), 1 if first else 0,
          bracket="vt_accumulate", tensors=(g, gv) if first else (gv, g, gv))


def vt_variance(gv, adv_grad, N: int, out=None):
    """vmifgsm.py:97: gv / N - adv_grad."""
    _require(gv, "gv"), _require(adv_grad, "adv_grad")
    _same_shape(("gv", gv), ("adv_grad", adv_grad))
    if int(N) < 1:
        raise ValueError(f"N must be at least 1, got {N}")
    out = _out_like(gv, out)
    _call("advstep_vt_variance_f32", gv.device, gv, adv_grad, out, gv.numel(), int(N),
          bracket="vt_variance", tensors=(gv, adv_grad, out))
    return out


# ---------------------------------------------------------------------------------------------------------
# MultiAttack's row router (include/advstep_multi.h; reference .../attacks/multiattack.py:55-66)
# ---------------------------------------------------------------------------------------------------------

def multi_route(adv, x, z, labels, rows, final, next_x=None, next_y=None, next_rows=None):
    """One stage of MultiAttack's bookkeeping over the n rows of a sub-batch: row i is wrong when (z[i] > 0) != labels[i];
    a wrong row goes to final[rows[i]] = adv[i], a kept row to the next free row k of next_x / next_y / next_rows (= x[i],
    labels[i], rows[i]), in ascending i.  Returns (next_x, next_y, next_rows, counts): the buffers are n rows long and only
    their first counts[1] rows are written; counts = int32 (number wrong, number kept) on the device — the caller narrows
    after reading it.  next_x must not be x, adv or final (no compaction in place); final is none of the others."""
    _require(adv, "adv"), _require(x, "x"), _require(z, "z"), _require(final, "final")
    _require(labels, "labels", torch.int64), _require(rows, "rows", torch.int32)
    _same_shape(("adv", adv), ("x", x))
    n, T = _rows(adv, "adv")
    B, Tf = _rows(final, "final")
    if (n and Tf != T) or final.device != adv.device:
        raise ValueError(f"final {tuple(final.shape)}@{final.device} does not hold rows of adv {tuple(adv.shape)}@{adv.device}")
    for name, t in (("z", z), ("labels", labels), ("rows", rows)):
        if t.numel() != n or t.device != adv.device:
            raise ValueError(f"{name} must hold one value per row of adv ({n}) on {adv.device}, got {tuple(t.shape)}@{t.device}")
    next_x = _out_like(x, next_x, "next_x")
    if next_y is None:
        next_y = torch.empty(n, dtype=torch.int64, device=adv.device)
    if next_rows is None:
        next_rows = torch.empty(n, dtype=torch.int32, device=adv.device)
    _require(next_y, "next_y", torch.int64), _require(next_rows, "next_rows", torch.int32)
    if next_y.numel() != n or next_rows.numel() != n:
        raise ValueError(f"next_y and next_rows must hold {n} values, got {next_y.numel()} and {next_rows.numel()}")
    if n and T == 0:
        raise ValueError("multi_route: rows of zero samples cannot be routed")
    # n == 0: the library launches nothing and writes nothing, not even counts
    counts = (torch.zeros if n == 0 else torch.empty)(2, dtype=torch.int32, device=adv.device)
    scratch = torch.empty(max(n, 1), dtype=torch.int32, device=adv.device)
    # compulsory traffic: every row is read once (from adv or from x) and written once (to final or to next_x)
    _call("advstep_multi_route_f32", adv.device, adv, x, z, labels, rows, final, next_x, next_y, next_rows, counts, scratch,
          n, B, T, bracket="multi_route", tensors=(adv, adv))
    return next_x, next_y, next_rows, counts


# ---------------------------------------------------------------------------------------------------------
# per-utterance perturbation report (include/advstep_perturb.h)
# ---------------------------------------------------------------------------------------------------------

# PERTURBATION_PLANES (imported above from the numpy-only metrics module): the rows of perturbation_stats' result, in order


def perturbation_stats(x, adv, out=None):
    """(6, B) float32, one row per name of PERTURBATION_PLANES, of d = adv - x per utterance: max |d|, mean |d|, ||d||_2,
    sum x^2, 10 log10(sum x^2 / sum d^2) and the segmental SNR over full 256-sample segments, each clamped to [-10, 35] dB
    (definitions and corner cases: include/advstep_perturb.h).  One read of x and adv, two launches on the current stream,
    no synchronisation; reruns are bit-identical."""
    _require(x, "x"), _require(adv, "adv")
    _same_shape(("x", x), ("adv", adv))
    B, T = _rows(x, "x")
    out = _shaped(out, "out", (len(PERTURBATION_PLANES), B), x.device)
    lib = _lib.load()
    with _Launch("perturbation_stats", x.device, tensors=(x, adv)):
        # partials only, rewritten by every call: keyed by stream like the row workspace (two lanes never share one), and
        # handed to a captured graph by release_stream_workspaces with the rest of its stream's buffers
        key = (x.device.index if x.device.index is not None else torch.cuda.current_device(), _stream(x.device), int(B), int(T),
               "perturb")
        ws, ws_bytes = _scratch(key, lambda: torch.empty(max(lib.advstep_perturb_stats_workspace_bytes(B, T), 256),
                                                         dtype=torch.uint8, device=x.device))
        _call("advstep_perturb_stats_f32", x.device, x, adv, out, ws, ws_bytes, B, T)
    return out


# ---------------------------------------------------------------------------------------------------------
# minimal-radius search (include/advstep_radius.h): PGD steps with a radius per row, and the bisection's bookkeeping
# ---------------------------------------------------------------------------------------------------------

RADIUS_PLANES = ("lo", "hi", "eps", "best")     # the rows of a search state, in the order of include/advstep_radius.h


def row_pgd_linf_step(adv, grad, orig, eps_rows, alpha_abs: float, alpha_rel: float, lo: float = 0.0, hi: float = 1.0,
                      out=None):
    """pgd_linf_step with a radius per row: e = eps_rows[b], a = alpha_abs + alpha_rel * e,
    out = clamp(orig + clamp((adv + a * sign(grad)) - orig, -e, e), lo, hi).  `out` may be `adv`."""
    _require(adv, "adv"), _require(grad, "grad"), _require(orig, "orig")
    _same_shape(("adv", adv), ("grad", grad), ("orig", orig))
    B, T = _rows(adv, "adv")
    _per_row(eps_rows, "eps_rows", B)
    out = _out_like(adv, out)
    _call("advstep_row_pgd_linf_step_f32", adv.device, adv, grad, orig, eps_rows, alpha_abs, alpha_rel, lo, hi, out, B, T,
          bracket="row_pgd_linf_step", tensors=(adv, grad, orig, out))
    return out


def row_pgd_l2_step(adv, grad, orig, eps_rows, alpha_abs: float, alpha_rel: float, eps_div: float = 1e-10, lo: float = 0.0,
                    hi: float = 1.0, out=None, return_norms: bool = False):
    """pgd_l2_step (three launches) with a radius per row: e = eps_rows[b], a = alpha_abs + alpha_rel * e; a row whose
    step leaves it where `orig` is (||d|| = 0) comes back as clamp(orig), also at e = 0.  `out` may be `adv`."""
    _require(adv, "adv"), _require(grad, "grad"), _require(orig, "orig")
    _same_shape(("adv", adv), ("grad", grad), ("orig", orig))
    B, T = _rows(adv, "adv")
    _per_row(eps_rows, "eps_rows", B)
    out = _out_like(adv, out)
    gn = dn = None
    if return_norms:
        gn = torch.empty(B, dtype=torch.float32, device=adv.device)
        dn = torch.empty(B, dtype=torch.float32, device=adv.device)
    # compulsory traffic: grad three times, adv and orig twice, out once
    with _Launch("row_pgd_l2_step", adv.device, tensors=(grad,) * 3 + (adv,) * 2 + (orig,) * 2 + (out,)):
        ws, ws_bytes = _workspace(adv.device, B, T)
        _call("advstep_row_pgd_l2_step_f32", adv.device, adv, grad, orig, eps_rows, alpha_abs, alpha_rel, eps_div, lo, hi, out,
              gn, dn, B, T, ws, ws_bytes)
    return (out, gn, dn) if return_norms else out


def radius_begin(z0, labels, eps_max: float, state=None):
    """The search state (4, B) = lo, hi, eps, best (RADIUS_PLANES) from the clean logits: a row the model already gets wrong
    ((z0 > 0) != label) starts and stays at radius 0 with best = 0; every other row starts at eps_max with best = +inf."""
    _require(z0, "z0")
    B = z0.numel()
    _per_row(labels, "labels", B, torch.int64)
    if not float(eps_max) >= 0.0:
        raise ValueError(f"eps_max must be a radius >= 0, got {eps_max}")
    state = _shaped(state, "state", (len(RADIUS_PLANES), B), z0.device)
    _call("advstep_radius_begin_f32", z0.device, z0, labels, eps_max, state, B, bracket="radius_begin")
    return state


def radius_round(adv, z, labels, first: bool, state, best_adv, out=None):
    """One round of the bisection after the attempt `adv` at the radii state[2] was judged (z = the logit of model(adv)):
    flipped and eps < best -> best = hi = eps and the row is copied into best_adv; not flipped -> lo = eps and the row is
    copied iff `first`; then eps = (lo + hi) / 2.  Returns the NEW state, written to `out` (another (4, B) buffer than `state`:
    the launch only reads `state`); best_adv is updated in place.  One launch, no host read.  Empty work (B == 0 or rows of no
    samples) launches nothing and writes nothing, `out` included, as the library defines it."""
    _require(adv, "adv"), _require(z, "z"), _require(best_adv, "best_adv")
    _same_shape(("adv", adv), ("best_adv", best_adv))
    B, T = _rows(adv, "adv")
    if z.numel() != B or z.device != adv.device:
        raise ValueError(f"z must hold one logit per row of adv ({B}) on {adv.device}, got {tuple(z.shape)}@{z.device}")
    _per_row(labels, "labels", B, torch.int64)
    _shaped(_require(state, "state"), "state", (len(RADIUS_PLANES), B), adv.device)
    out = _shaped(out, "out", (len(RADIUS_PLANES), B), adv.device)
    # compulsory traffic: at most one read and one write of every row (only the rows that improve move)
    _call("advstep_radius_round_f32", adv.device, adv, z, labels, 1 if first else 0, state, out, best_adv, B, T,
          bracket="radius_round", tensors=(adv, best_adv))
    return out


# ---------------------------------------------------------------------------------------------------------
# minimal-norm attack (include/advstep_fmn.h): the iterate's row norms and the step of torchattacks.FMN
# ---------------------------------------------------------------------------------------------------------

FMN_PLANES = ("eps", "best", "found", "dnorm")  # the rows of an attack state, in the order of include/advstep_fmn.h
FMN_NORMS = ("dsq", "dmax", "gsq", "gabs")      # the partial planes fmn_norms writes; the workspace's fifth is the L2 move's
FMN_TILE = 4096                                 # samples per partial


def fmn_workspace(B: int, T: int, device) -> torch.Tensor:
    """A fresh workspace of the FMN entry points for a (B, T) batch: flat float32, five planes of one partial per (row, tile).
    No zero-fill is needed (include/advstep_fmn.h); one stream at a time."""
    return torch.empty(max(_lib.load().advstep_fmn_workspace_bytes(B, T), 16) // 4, dtype=torch.float32, device=device)


def fmn_partials(ws: torch.Tensor, B: int, T: int) -> torch.Tensor:
    """The (4, B, C) view of the partials `fmn_norms` left in `ws` (FMN_NORMS; C = ceil(T / 4096) tiles)."""
    C = -(-T // FMN_TILE)
    plane = ws.numel() // 5
    return ws[:4 * plane].view(4, plane)[:, :B * C].view(4, B, C)


def _fmn_ws(ws: Optional[torch.Tensor], B: int, T: int, device) -> torch.Tensor:
    if ws is None:
        return fmn_workspace(B, T, device)
    _require(ws, "ws")
    if ws.device != device or ws.numel() * 4 < _lib.load().advstep_fmn_workspace_bytes(B, T):
        raise ValueError(f"ws must be fmn_workspace({B}, {T}) on {device}, got {ws.numel()} floats on {ws.device}")
    return ws


def fmn_begin(state=None, B: Optional[int] = None, device=None):
    """The attack state (4, B) = eps, best, found, dnorm (FMN_PLANES) before the first step: eps = best = +inf, found = 0."""
    if state is None:
        state = torch.empty((len(FMN_PLANES), int(B)), dtype=torch.float32, device=device)
    _require(state, "state")
    if state.dim() != 2 or state.shape[0] != len(FMN_PLANES):
        raise ValueError(f"state must be ({len(FMN_PLANES)}, B), got {tuple(state.shape)}")
    _call("advstep_fmn_begin_f32", state.device, state, state.shape[1], bracket="fmn_begin")
    return state


def fmn_norms(adv, grad, orig, ws=None):
    """Per-(row, tile) partials of sum d^2, max |d|, sum g^2 and sum |g| (d = adv - orig, g = grad; grad None: the g planes get
    0), left in the workspace `ws` (a fresh `fmn_workspace` when None), which is returned for `fmn_step`; `fmn_partials` views
    them.  One launch, 12 B per sample, no host read."""
    _require(adv, "adv"), _require(orig, "orig")
    _same_shape(("adv", adv), ("orig", orig))
    if grad is not None:
        _require(grad, "grad")
        _same_shape(("adv", adv), ("grad", grad))
    B, T = _rows(adv, "adv")
    ws = _fmn_ws(ws, B, T, adv.device)
    _call("advstep_fmn_norms_f32", adv.device, adv, grad, orig, B, T, ws, ws.numel() * 4, bracket="fmn_norms",
          tensors=(adv, grad, orig))
    return ws


def fmn_step(adv, grad, orig, z, labels, state, best_adv, ws, alpha: float, gamma: float, norm: str = "Linf", move: bool = True,
             eps_div: float = 1e-10, lo: float = 0.0, hi: float = 1.0, state_out=None, out=None, row_norms=None):
    """One step of the FMN recurrence after `fmn_norms` of the same adv, grad, orig left its partials in `ws` (z = the logit of
    model(adv), grad = dz / d adv turned towards the other class): the row's decision from `state` into `state_out` (another
    (4, B) buffer: the launch only reads `state`), the row's iterate into `best_adv` iff it is adversarial and smaller than
    every earlier one, then the move and the projection into the row's new radius (include/advstep_fmn.h has the expressions).
    move=False is the last call: decision and copy only, grad may be None.  Returns (state_out, out) — out is None when
    move=False.  row_norms: an optional (5, B) tensor that receives the row norms the decision used.  No host read."""
    _require(adv, "adv"), _require(orig, "orig"), _require(best_adv, "best_adv"), _require(z, "z")
    _same_shape(("adv", adv), ("orig", orig), ("best_adv", best_adv))
    if grad is not None:
        _require(grad, "grad")
        _same_shape(("adv", adv), ("grad", grad))
    elif move:
        raise ValueError("fmn_step needs the gradient to move (grad=None only with move=False)")
    B, T = _rows(adv, "adv")
    if z.numel() != B or z.device != adv.device:
        raise ValueError(f"z must hold one logit per row of adv ({B}) on {adv.device}, got {tuple(z.shape)}@{z.device}")
    _per_row(labels, "labels", B, torch.int64)
    kind = _apgd_norm(norm)
    if not 0.0 < float(gamma) < 1.0:
        raise ValueError(f"gamma must lie in (0, 1), got {gamma}")
    _shaped(_require(state, "state"), "state", (len(FMN_PLANES), B), adv.device)
    state_out = _shaped(state_out, "state_out", (len(FMN_PLANES), B), adv.device)
    if row_norms is not None:
        _shaped(_require(row_norms, "row_norms"), "row_norms", (5, B), adv.device)
    ws = _fmn_ws(_require(ws, "ws"), B, T, adv.device)
    out = _out_like(adv, out) if move else None
    # compulsory traffic: adv, grad, orig and out once (the L2 form reads the three inputs twice); improved rows move once more
    traffic = (adv, grad, orig, out) + ((adv, grad, orig) if kind == 1 else ()) if move else ()
    _call("advstep_fmn_step_f32", adv.device, adv, grad, orig, z, labels, state, state_out, best_adv, out, row_norms, float(alpha),
          float(gamma), kind, 1 if move else 0, float(eps_div), lo, hi, B, T, ws, ws.numel() * 4, bracket="fmn_step",
          tensors=traffic)
    return state_out, out


FMN_SPARSE_NORMS = ("dabs", "dcnt", "gsq", "gmax")   # the row norms fmn_sparse_step's decision uses (include/advstep_fmn_sparse.h)
_FMN_SPARSE_KINDS = {"L1": 2, "L0": 3}               # include/advstep_fmn.h's numbering, continued


def fmn_sparse_step(adv, grad, orig, z, labels, state, best_adv, alpha: float, gamma: float, norm: str, move: bool = True,
                    eps_div: float = 1e-10, state_out=None, out=None, row_norms=None):
    """One step of the FMN recurrence for the L1 or the L0 threat model, ONE launch without a workspace (z = the logit of
    model(adv), grad = dz / d adv turned towards the other class): the row's norms, its decision from `state` into `state_out`
    (another (4, B) buffer: the launch only reads `state`), the row's iterate into `best_adv` iff it is adversarial and smaller
    than every earlier one, then the move and the exact projection (L1 ball or k-sparse set, intersected with the box [0, 1])
    into the row's NEW radius (include/advstep_fmn_sparse.h has the expressions).  move=False is the last call: decision and
    copy only, grad may be None.  Returns (state_out, out) — out is None when move=False.  row_norms: an optional (4, B) tensor
    that receives FMN_SPARSE_NORMS as the decision used them.  No host read."""
    _require(adv, "adv"), _require(orig, "orig"), _require(best_adv, "best_adv"), _require(z, "z")
    _same_shape(("adv", adv), ("orig", orig), ("best_adv", best_adv))
    if grad is not None:
        _require(grad, "grad")
        _same_shape(("adv", adv), ("grad", grad))
    elif move:
        raise ValueError("fmn_sparse_step needs the gradient to move (grad=None only with move=False)")
    B, T = _rows(adv, "adv")
    if z.numel() != B or z.device != adv.device:
        raise ValueError(f"z must hold one logit per row of adv ({B}) on {adv.device}, got {tuple(z.shape)}@{z.device}")
    _per_row(labels, "labels", B, torch.int64)
    if norm not in _FMN_SPARSE_KINDS:
        raise ValueError(f"fmn_sparse_step norm must be 'L1' or 'L0', got {norm!r}")
    if not 0.0 < float(gamma) < 1.0:
        raise ValueError(f"gamma must lie in (0, 1), got {gamma}")
    _shaped(_require(state, "state"), "state", (len(FMN_PLANES), B), adv.device)
    state_out = _shaped(state_out, "state_out", (len(FMN_PLANES), B), adv.device)
    if row_norms is not None:
        _shaped(_require(row_norms, "row_norms"), "row_norms", (len(FMN_SPARSE_NORMS), B), adv.device)
    out = _out_like(adv, out) if move else None
    # compulsory traffic: adv, grad, orig and out once (every later pass re-reads the row from cache); improved rows move once more
    _call("advstep_fmn_sparse_step_f32", adv.device, adv, grad, orig, z, labels, state, state_out, best_adv, out, row_norms,
          float(alpha), float(gamma), _FMN_SPARSE_KINDS[norm], 1 if move else 0, float(eps_div), B, T, bracket="fmn_sparse_step",
          tensors=(adv, grad, orig, out) if move else (adv, orig))
    return state_out, out


# ---------------------------------------------------------------------------------------------------------
# SNR-budget PGD (include/advstep_snr.h): the segmental step and the radii of the global budget
# ---------------------------------------------------------------------------------------------------------

def _snr_rho(rho: float) -> float:
    if not float(rho) >= 0.0:
        raise ValueError(f"rho = 10^(-snr_db / 20) must be >= 0, got {rho}")
    return float(rho)


def seg_pgd_step(adv, grad, orig, offset_rows, rho: float, alpha_rel: float, eps_div: float, lo: float = 0.0, hi: float = 1.0,
                 out=None):
    """The PGD step under a segmental-SNR budget: every 256-sample segment of a row is an L2 ball of radius
    r = rho * sqrt(sum (orig + c)^2) over the segment, c = offset_rows[b] (None: 0); the segment's gradient is normalised by its
    own norm, the step is alpha_rel * r, and the segment is projected onto its own ball (include/advstep_snr.h).  One launch,
    16 B per sample.  `out` may be `adv`."""
    _require(adv, "adv"), _require(grad, "grad"), _require(orig, "orig")
    _same_shape(("adv", adv), ("grad", grad), ("orig", orig))
    B, T = _rows(adv, "adv")
    c = _optional_rows(offset_rows, "offset_rows", B, adv.device)     # the rows' c = mn / (mx - mn), or None (c = 0)
    rho = _snr_rho(rho)
    out = _out_like(adv, out)
    _call("advstep_seg_pgd_step_f32", adv.device, adv, grad, orig, c, rho, alpha_rel, eps_div, lo, hi, out, B, T,
          bracket="seg_pgd_step", tensors=(adv, grad, orig, out))
    return out


def snr_row_radius(x, offset_rows, rho: float, out=None):
    """(B,) float32: rho * sqrt(sum_t (x + c)^2) per row, c = offset_rows[b] (None: 0) — the radii at which `row_pgd_l2_step`
    is the PGD step under a global SNR budget.  Two launches, no host read."""
    _require(x, "x")
    B, T = _rows(x, "x")
    c = _optional_rows(offset_rows, "offset_rows", B, x.device)
    rho = _snr_rho(rho)
    if out is None:
        out = torch.empty(B, dtype=torch.float32, device=x.device)
    _per_row(out, "out", B)
    with _Launch("snr_row_radius", x.device, tensors=(x,)):
        ws, ws_bytes = _workspace(x.device, B, T)
        _call("advstep_snr_row_radius_f32", x.device, x, c, rho, out, B, T, ws, ws_bytes)
    return out


# ---------------------------------------------------------------------------------------------------------
# universal perturbation (include/advstep_universal.h): the column sum over a batch and the broadcast of one delta
# ---------------------------------------------------------------------------------------------------------

UNIVERSAL_GROUP_ROWS = 16                       # ADVSTEP_UNIVERSAL_GROUP_ROWS: rows per group of universal_colsum's first launch


def universal_colsum(grad, row_weight=None, out=None):
    """(1, T) float32: out[t] = sum_b w_b * grad[b, t], w_b = row_weight[b] (None: 1) — the gradient of the batch's loss with
    respect to one perturbation shared by its rows.  Every product rounds once and the order of the additions depends on (B, T)
    alone (include/advstep_universal.h): reruns, on any stream, are bit-identical.  One launch for B <= 16, two above; no host
    read."""
    _require(grad, "grad")
    B, T = _rows(grad, "grad")
    w = _optional_rows(row_weight, "row_weight", B, grad.device)      # the rows' w_b, or None (w_b = 1)
    if out is None:
        out = torch.empty((1, T), dtype=torch.float32, device=grad.device)
    _require(out, "out")
    if out.numel() != T or out.device != grad.device:
        raise ValueError(f"out must hold one value per column ({T}) on {grad.device}, got {tuple(out.shape)}@{out.device}")
    lib = _lib.load()
    with _Launch("universal_colsum", grad.device, tensors=(grad, out)):
        # partial planes only, rewritten by every call: keyed by stream like the row workspace
        key = (grad.device.index if grad.device.index is not None else torch.cuda.current_device(), _stream(grad.device), int(B),
               int(T), "universal")
        ws, ws_bytes = _scratch(key, lambda: torch.empty(max(lib.advstep_universal_workspace_bytes(B, T), 256), dtype=torch.uint8,
                                                         device=grad.device))
        _call("advstep_universal_colsum_f32", grad.device, grad, w, out, B, T, ws, ws_bytes)
    return out


def universal_apply(x, delta, row_weight=None, lo: float = 0.0, hi: float = 1.0, out=None):
    """out[b, t] = clamp(x[b, t] + w_b * delta[t], lo, hi), w_b = row_weight[b] (None: 1): one perturbation of T samples added
    to every row.  One launch, 8 B per sample, no host read.  `out` may be `x`."""
    _require(x, "x"), _require(delta, "delta")
    B, T = _rows(x, "x")
    if delta.numel() != T or delta.device != x.device:
        raise ValueError(f"delta must hold one value per sample of a row ({T}) on {x.device}, got {tuple(delta.shape)}@{delta.device}")
    w = _optional_rows(row_weight, "row_weight", B, x.device)
    out = _out_like(x, out)
    _call("advstep_universal_apply_f32", x.device, x, delta, w, out, B, T, lo, hi, bracket="universal_apply", tensors=(x, out))
    return out


# ---------------------------------------------------------------------------------------------------------
# score-based black-box attack (include/advstep_spsa.h): the probe slots of an iteration and the sign step along the estimate
# ---------------------------------------------------------------------------------------------------------

SPSA_MAX_DIRECTIONS = 1024                      # ADVSTEP_SPSA_MAX_DIRECTIONS: direction pairs of one iteration


def spsa_probe(adv, delta: float, seed: int, offset: int = 0, s0: int = 0, ns: int = 1, lo: float = 0.0, hi: float = 1.0,
               out=None):
    """(ns, *adv.shape) float32: slots s0 .. s0 + ns - 1 of an SPSA iteration on `adv` (B, T) — slot 0 is adv itself, slot 1 + 2j is
    clamp(adv + delta v_j, lo, hi), slot 2 + 2j is clamp(adv - delta v_j, lo, hi), v_j the Rademacher direction j that the
    kernel regenerates from Philox (seed, offset; include/advstep_spsa.h has the bit mapping).  A fill in chunks gives the bytes
    of a whole one.  One launch, 4 B read and 4 * ns B written per sample, no host read."""
    _require(adv, "adv")
    B, T = _rows(adv, "adv")
    s0, ns = int(s0), int(ns)
    if s0 < 0 or ns < 0 or s0 + ns > 1 + 2 * SPSA_MAX_DIRECTIONS:
        raise ValueError(f"slots {s0} .. {s0 + ns - 1} are outside 0 .. {2 * SPSA_MAX_DIRECTIONS}")
    out = _stacked_out(out, ns, adv)
    _call("advstep_spsa_probe_f32", adv.device, adv, out, B, T, s0, ns, delta, lo, hi, seed, offset,
          bracket="spsa_probe", tensors=(adv, out))
    return out


def spsa_step(adv, orig, z, labels, queries, alpha: float, eps: float, seed: int, offset: int = 0, lo: float = 0.0,
              hi: float = 1.0, out=None):
    """One SPSA sign step from the logits `z` (S, B) of the S = 1 + 2n slots `spsa_probe` filled with the same (seed, offset).
    A row that slot 0 already shows fooled — (z[0, b] > 0) != (labels[b] == 1) — is copied and its `queries` (B, int32) entry
    stays; every other row moves along sign(sum_j v_j d_j), d_j = -+(z[1 + 2j, b] - z[2 + 2j, b]), is projected exactly as by
    `pgd_linf_step`, and counts S queries.  The estimate is never stored: one launch, 12 B per sample, no host read.  `out` may
    be `adv`."""
    _require(adv, "adv"), _require(orig, "orig"), _require(z, "z")
    _same_shape(("adv", adv), ("orig", orig))
    B, T = _rows(adv, "adv")
    if z.dim() != 2 or z.shape[1] != B or z.shape[0] < 1 or z.shape[0] % 2 != 1 or z.device != adv.device:
        raise ValueError(f"z must be (1 + 2n, {B}) on {adv.device}, got {tuple(z.shape)}@{z.device}")
    n = (z.shape[0] - 1) // 2
    if n > SPSA_MAX_DIRECTIONS:
        raise ValueError(f"at most {SPSA_MAX_DIRECTIONS} direction pairs per iteration, got {n}")
    _per_row(labels, "labels", B, torch.int64, adv.device), _per_row(queries, "queries", B, torch.int32, adv.device)
    out = _out_like(adv, out)
    _call("advstep_spsa_step_f32", adv.device, adv, orig, z, labels, queries, out, B, T, n, alpha, eps, lo, hi, seed, offset,
          bracket="spsa_step", tensors=(adv, orig, out, z))
    return out


# ---------------------------------------------------------------------------------------------------------
# randomized smoothing (include/advstep_smooth.h): the Gaussian-noised copies of a batch and the vote count over their logits
# ---------------------------------------------------------------------------------------------------------

def smooth_noise(x, sigma: float, seed: int, offset: int = 0, s0: int = 0, ns: int = 1, out=None):
    """(ns, *x.shape) float32: copies s0 .. s0 + ns - 1 of `x` (B, T) under Gaussian noise, x + sigma * z with z the standard
    normals the kernel regenerates from Philox at counter offset + s (seed; include/advstep_smooth.h has the mapping).  No clamp;
    a NaN in x propagates.  A fill in chunks gives the bytes of a whole one.  One launch, 4 B read and 4 * ns B written per
    sample, no host read."""
    _require(x, "x")
    B, T = _rows(x, "x")
    s0, ns, sigma = int(s0), int(ns), float(sigma)
    if s0 < 0 or ns < 0:
        raise ValueError(f"s0 and ns must not be negative, got {s0} and {ns}")
    if not 0.0 <= sigma < float("inf"):                             # (a NaN sigma fails the comparison)
        raise ValueError(f"sigma must be a finite noise level >= 0, got {sigma}")
    out = _stacked_out(out, ns, x)
    _call("advstep_smooth_noise_f32", x.device, x, out, B, T, s0, ns, sigma, seed, offset,
          bracket="smooth_noise", tensors=(x, out))
    return out


def smooth_tally(z, counts):
    """counts[b] += #{s : z[s, b] > 0} for the logits `z` (ns, B) of ns noisy copies; `counts` (B,) int32, read and written.
    A NaN logit is class 0.  One launch, no host read."""
    _require(z, "z")
    if z.dim() != 2:
        raise ValueError(f"z must be (ns, B), got {tuple(z.shape)}")
    ns, B = z.shape
    _per_row(counts, "counts", B, torch.int32, z.device)
    _call("advstep_smooth_tally_i32", z.device, z, counts, B, ns, bracket="smooth_tally", tensors=(z, counts))
    return counts


# ---------------------------------------------------------------------------------------------------------
# the attack on the smoothed detector (include/advstep_smoothadv.h): the noised copies of the iterate in the detector's domain,
# the soft vote over their logits with its gradient, and the sum over the slot gradients fused with PGD's step
# ---------------------------------------------------------------------------------------------------------

SMOOTHADV_NORMS = {"Linf": 0, "L2": 1}          # ADVSTEP_SMOOTHADV_LINF / _L2


def smoothadv_fill(adv, sigma: float, seed: int, offset: int = 0, s0: int = 0, ns: int = 1, scale=None, shift=None, out=None):
    """(ns, *adv.shape) float32: copies s0 .. s0 + ns - 1 of (shift_b + scale_b * adv) + sigma * z, `scale` / `shift` one float32 per
    row or both None (then the bytes are `smooth_noise`'s), z as in `smooth_noise` at counter offset + s.  With scale = mx - mn
    and shift = mn the copies are those of the reverted iterate, which is never stored.  One launch, 4 B read and 4 * ns B written
    per sample, no host read."""
    _require(adv, "adv")
    B, T = _rows(adv, "adv")
    s0, ns, sigma = int(s0), int(ns), float(sigma)
    if s0 < 0 or ns < 0:
        raise ValueError(f"s0 and ns must not be negative, got {s0} and {ns}")
    if not 0.0 <= sigma < float("inf"):                             # (a NaN sigma fails the comparison)
        raise ValueError(f"sigma must be a finite noise level >= 0, got {sigma}")
    if (scale is None) != (shift is None):
        raise ValueError("scale and shift are given together or not at all")
    scale, shift = _optional_rows(scale, "scale", B, adv.device), _optional_rows(shift, "shift", B, adv.device)
    out = _stacked_out(out, ns, adv)
    _call("advstep_smoothadv_fill_f32", adv.device, adv, scale, shift, out, B, T, s0, ns, sigma, seed, offset,
          bracket="smoothadv_fill", tensors=(adv, out))
    return out


def smoothadv_loss_grad(z, labels, scale: float = 1.0):
    """The soft vote of m noised copies: for logits `z` (m, B) and labels (B) int64 returns (dz (m, B), cost (B)) with cost_b =
    -log(mean_i sigmoid(s z_ib)), s = 2 y_b - 1, and dz = scale * d cost_b / d z_ib (scale = -1: targeted).  The cost is per row,
    not a batch mean.  One launch, no host read."""
    _require(z, "z")
    if z.dim() != 2:
        raise ValueError(f"z must be (m, B), got {tuple(z.shape)}")
    m, B = z.shape
    _per_row(labels, "labels", B, torch.int64, z.device)
    dz = torch.empty_like(z)
    cost = torch.empty(B, dtype=torch.float32, device=z.device)
    _call("advstep_smoothadv_loss_grad_f32", z.device, z, labels, dz, cost, B, m, float(scale), bracket="smoothadv_loss_grad",
          tensors=(z, dz, cost))
    return dz, cost


def smoothadv_step(adv, orig, grads, alpha: float, eps: float, norm: str = "L2", eps_div: float = 1e-10, lo: float = 0.0,
                   hi: float = 1.0, out=None, gsum=None):
    """PGD's step along the slot-order float32 sum of `grads` (m, *adv.shape): `out` has the bits of `pgd_l2_step` / `pgd_linf_step`
    on (adv, sum, orig).  The sum is written to `gsum` and returned as (out, gsum) when `gsum` is given.  L-inf: one launch,
    (m + 2) * 4 B read per sample; L2: three, the first of which also leaves the sum's row norms.  `out` may be `adv`."""
    _require(adv, "adv"), _require(orig, "orig"), _require(grads, "grads")
    _same_shape(("adv", adv), ("orig", orig))
    B, T = _rows(adv, "adv")
    if norm not in SMOOTHADV_NORMS:
        raise ValueError(f"norm must be one of {sorted(SMOOTHADV_NORMS)}, got {norm!r}")
    if grads.dim() < 1 or grads.shape[0] < 1 or grads.numel() != grads.shape[0] * adv.numel() or grads.device != adv.device:
        raise ValueError(f"grads must hold (m, {B}, {T}) values with m >= 1 on {adv.device}, got {tuple(grads.shape)}@{grads.device}")
    m = grads.shape[0]
    out = _out_like(adv, out)
    sums = _out_like(adv, gsum, "gsum")
    with _Launch("smoothadv_step", adv.device, tensors=(adv, orig, grads, sums, out)):
        ws, ws_bytes = _workspace(adv.device, B, T) if norm == "L2" else (None, 0)
        _call("advstep_smoothadv_step_f32", adv.device, adv, orig, grads, sums, out, B, T, m, SMOOTHADV_NORMS[norm], alpha, eps, eps_div,
              lo, hi, ws, ws_bytes)
    return out if gsum is None else (out, gsum)


# ---------------------------------------------------------------------------------------------------------
# label-only black-box attack (include/advstep_hsj.h): the bisection towards the boundary, the probes of a normal estimate, the
# candidate steps along its sign and the choice among them
# ---------------------------------------------------------------------------------------------------------

HSJ_PLANES = ("lo", "hi", "mid", "dist0")       # the rows of a boundary-search state, in the order of include/advstep_hsj.h
HSJ_MAX_DIRECTIONS = 1024                       # ADVSTEP_HSJ_MAX_DIRECTIONS: probes of one normal estimate
HSJ_MAX_TRIALS = 8                              # ADVSTEP_HSJ_MAX_TRIALS: candidate slots of one step


def _hsj_state(t: torch.Tensor, name: str, B: int, device) -> torch.Tensor:
    return _shaped(_require(t, name), name, (len(HSJ_PLANES), B), device)


def _hsj_rows(cur, orig, B, **per_row):
    """The per-row operands of the HopSkipJump entry points: name=(tensor, dtype), each (B,) on cur's device."""
    if orig is not None:
        _require(orig, "orig")
        _same_shape(("cur", cur), ("orig", orig))
    for name, (t, dtype) in per_row.items():
        _per_row(t, name, B, dtype, cur.device)


def _hsj_logits(z, name: str, B: int, cap: int, device) -> int:
    _require(z, name)
    if z.dim() != 2 or z.shape[1] != B or z.device != device:
        raise ValueError(f"{name} must be (n, {B}) on {device}, got {tuple(z.shape)}@{z.device}")
    if z.shape[0] > cap:
        raise ValueError(f"{name}: at most {cap} rows of logits, got {z.shape[0]}")
    return int(z.shape[0])


def hsj_search_open(cur, orig, dist, active, out, state=None, lo: float = 0.0, hi: float = 1.0):
    """Open a boundary search: per active row lo = 0, hi = dist0 = dist, mid = (lo + hi) / 2, and `out` = point(mid) =
    clamp(orig + clamp(cur - orig, -mid, mid), lo, hi), the first probe to be judged.  An inactive row (active[b] == 0) is copied
    and every plane of its state is dist.  Returns the (4, B) state (HSJ_PLANES).  One launch, no host read."""
    _require(cur, "cur"), _require(out, "out")
    _same_shape(("cur", cur), ("out", out))
    B, T = _rows(cur, "cur")
    _hsj_rows(cur, orig, B, dist=(dist, torch.float32), active=(active, torch.int32))
    state = _shaped(state, "state", (len(HSJ_PLANES), B), cur.device)
    _call("advstep_hsj_search_open_f32", cur.device, cur, orig, dist, active, state, out, B, T, lo, hi,
          bracket="hsj_search_open", tensors=(cur, orig, out))
    return state


def hsj_search_next(cur, orig, z, labels, active, state, out, state_out=None, lo: float = 0.0, hi: float = 1.0):
    """One round of the bisection after the probe at state[2] was judged (z = its logits): adversarial -> hi = mid, else lo = mid;
    then mid = (lo + hi) / 2 and `out` = point(mid).  Returns the NEW state, written to `state_out` (another buffer than `state`:
    the launch only reads `state`).  One launch, no host read."""
    _require(cur, "cur"), _require(out, "out")
    _same_shape(("cur", cur), ("out", out))
    B, T = _rows(cur, "cur")
    _hsj_rows(cur, orig, B, z=(z, torch.float32), labels=(labels, torch.int64), active=(active, torch.int32))
    _hsj_state(state, "state", B, cur.device)
    state_out = _shaped(state_out, "state_out", (len(HSJ_PLANES), B), cur.device)
    _call("advstep_hsj_search_next_f32", cur.device, cur, orig, z, labels, active, state, state_out, out, B, T, lo, hi,
          bracket="hsj_search_next", tensors=(cur, orig, out))
    return state_out


def hsj_search_close(cur, orig, z, labels, active, state, queries, rounds: int, out=None, lo: float = 0.0, hi: float = 1.0):
    """Close a boundary search after its last probe was judged: the same decision as a round, then a row with hi < dist0 becomes
    point(hi) — the bytes of the probe that was judged adversarial — and any other row keeps cur's bytes.  `queries` (B, int32)
    gains `rounds` for every active row.  `out` may be `cur`.  One launch, no host read."""
    _require(cur, "cur")
    B, T = _rows(cur, "cur")
    _hsj_rows(cur, orig, B, z=(z, torch.float32), labels=(labels, torch.int64), active=(active, torch.int32),
              queries=(queries, torch.int32))
    _hsj_state(state, "state", B, cur.device)
    if int(rounds) < 0:
        raise ValueError(f"rounds must be >= 0, got {rounds}")
    out = _out_like(cur, out)
    _call("advstep_hsj_search_close_f32", cur.device, cur, orig, z, labels, active, state, queries, int(rounds), out, B, T, lo, hi,
          bracket="hsj_search_close", tensors=(cur, orig, out))
    return out


def hsj_probe(cur, mag, active, seed: int, offset: int = 0, s0: int = 0, ns: int = 1, lo: float = 0.0, hi: float = 1.0, out=None):
    """(ns, *cur.shape) float32: probes s0 .. s0 + ns - 1 of a normal estimate at `cur` (B, T) — slot j is
    clamp(cur + mag[b] v_j, lo, hi), v_j the Rademacher direction j of `spsa_probe` (the same Philox mapping); there is no copy of
    cur among the slots.  An inactive row is cur's bytes in every slot.  One launch, 4 B read and 4 * ns B written per sample."""
    _require(cur, "cur")
    B, T = _rows(cur, "cur")
    _hsj_rows(cur, None, B, mag=(mag, torch.float32), active=(active, torch.int32))
    s0, ns = int(s0), int(ns)
    if s0 < 0 or ns < 0 or s0 + ns > HSJ_MAX_DIRECTIONS:
        raise ValueError(f"slots {s0} .. {s0 + ns - 1} are outside 0 .. {HSJ_MAX_DIRECTIONS - 1}")
    out = _stacked_out(out, ns, cur)
    _call("advstep_hsj_probe_f32", cur.device, cur, mag, active, out, B, T, s0, ns, lo, hi, seed, offset,
          bracket="hsj_probe", tensors=(cur, out))
    return out


def hsj_candidates(cur, z, labels, dist, active, xi_rel: float, trials: int, seed: int, offset: int = 0, lo: float = 0.0,
                   hi: float = 1.0, out=None):
    """(trials, *cur.shape) float32: the candidate steps from the logits `z` (n, B) of the n probes `hsj_probe` filled with the
    same (seed, offset).  s = the sign of the integer form of HopSkipJump's estimate (include/advstep_hsj.h), xi = dist * xi_rel,
    slot k = clamp(cur + (xi * 2^-k) s, lo, hi).  The estimate is never stored: one launch, no host read."""
    _require(cur, "cur")
    B, T = _rows(cur, "cur")
    _hsj_rows(cur, None, B, labels=(labels, torch.int64), dist=(dist, torch.float32), active=(active, torch.int32))
    n = _hsj_logits(z, "z", B, HSJ_MAX_DIRECTIONS, cur.device)
    trials = int(trials)
    if not 0 <= trials <= HSJ_MAX_TRIALS:
        raise ValueError(f"trials must be in 0 .. {HSJ_MAX_TRIALS}, got {trials}")
    out = _stacked_out(out, trials, cur)
    _call("advstep_hsj_candidates_f32", cur.device, cur, z, labels, dist, active, out, B, T, n, trials, xi_rel, lo, hi, seed, offset,
          bracket="hsj_candidates", tensors=(cur, out, z))
    return out


def hsj_take(cur, cand, zc, labels, active, queries, n: int, out=None):
    """The step: per active row the first slot of `cand` (trials, B, T) whose logit in `zc` (trials, B) is adversarial becomes the
    row, and `queries` gains n + k + 1 (what an attacker who tries the slots in turn spends); if none is, the row stays and
    `queries` gains n + trials.  `out` may be `cur`: only the rows that move are then written.  One launch, no host read."""
    _require(cur, "cur"), _require(cand, "cand")
    B, T = _rows(cur, "cur")
    _hsj_rows(cur, None, B, labels=(labels, torch.int64), active=(active, torch.int32), queries=(queries, torch.int32))
    trials = _hsj_logits(zc, "zc", B, HSJ_MAX_TRIALS, cur.device)
    if cand.numel() != trials * B * T or cand.device != cur.device:
        raise ValueError(f"cand must hold ({trials}, {B}, {T}) values on {cur.device}, got {tuple(cand.shape)}@{cand.device}")
    if not 0 <= int(n) <= HSJ_MAX_DIRECTIONS:
        raise ValueError(f"n must be in 0 .. {HSJ_MAX_DIRECTIONS}, got {n}")
    out = _out_like(cur, out)
    _call("advstep_hsj_take_f32", cur.device, cur, cand, zc, labels, active, queries, out, B, T, int(n), trials,
          bracket="hsj_take", tensors=(cur, out))
    return out


# ---------------------------------------------------------------------------------------------------------
# simulated audio channel (include/advstep_channel.h): K draws of a FIR + delay + gain + noise, and the adjoint summed over the draws
# ---------------------------------------------------------------------------------------------------------

CHANNEL_MAX_TAPS = 256                          # ADVSTEP_CHANNEL_MAX_TAPS
CHANNEL_MAX_DRAWS = 64                          # ADVSTEP_CHANNEL_MAX_DRAWS


def _channel_params(taps, shift, gain, B: int, device, noise=None) -> Tuple[int, int]:
    """(K, L) of a draw's parameter tensors: taps (K, B, L) float32, shift (K, B) int32, gain (K, B) and noise (K, B) float32."""
    _require(taps, "taps"), _require(shift, "shift", torch.int32), _require(gain, "gain")
    if taps.dim() != 3 or taps.shape[1] != B:
        raise ValueError(f"taps must be (K, {B}, L), got {tuple(taps.shape)}")
    K, L = int(taps.shape[0]), int(taps.shape[2])
    if not 1 <= L <= CHANNEL_MAX_TAPS:
        raise ValueError(f"a channel has between 1 and {CHANNEL_MAX_TAPS} taps, got {L}")
    if K > CHANNEL_MAX_DRAWS:
        raise ValueError(f"at most {CHANNEL_MAX_DRAWS} draws per call, got {K}")
    named = [("shift", shift), ("gain", gain)] + ([("noise", _require(noise, "noise"))] if noise is not None else [])
    for name, t in named:
        if tuple(t.shape) != (K, B):
            raise ValueError(f"{name} must be ({K}, {B}), got {tuple(t.shape)}")
    for name, t in [("taps", taps)] + named:
        _on_device(t, name, device)
    return K, L


def channel_apply(x, center, taps, shift, gain, noise, seed: int, offset: int = 0, out=None):
    """(K, *x.shape) float32: K draws of the channel on x (B, T) — out[j] = (c + gain[j] * FIR(taps[j], x - c delayed by shift[j]))
    + noise[j] * n, with silence (c = `center`, one value per row) outside the utterance and n in [-1, 1) regenerated from Philox
    (seed, offset + j); include/advstep_channel.h fixes the arithmetic.  Not clamped.  One launch, 4 B read and 4 K B written per
    sample, no host read."""
    _require(x, "x")
    B, T = _rows(x, "x")
    _per_row(center, "center", B, device=x.device)
    K, L = _channel_params(taps, shift, gain, B, x.device, noise)
    out = _stacked_out(out, K, x)
    _call("advstep_channel_apply_f32", x.device, x, center, taps, shift, gain, noise, out, B, T, K, L, seed, offset,
          bracket="channel_apply", work=2.0 * K * L * B * T, tensors=(x, out))
    return out


def _channel_grads(grads, like, name: str = "grads") -> int:
    _require(grads, name)
    if grads.dim() < 2 or tuple(grads.shape[1:]) != tuple(like.shape) or grads.device != like.device:
        raise ValueError(f"{name} must be (K, {', '.join(map(str, like.shape))}) on {like.device}, got "
                         f"{tuple(grads.shape)}@{grads.device}")
    return int(grads.shape[0])


def channel_adjoint(grads, taps, shift, gain, out=None):
    """(B, T) float32: the channel's adjoint applied to the K gradients `grads` (K, B, T) and summed over the draws in draw
    order — the gradient at the channel's input of sum_j loss_j(channel_j(x)).  One launch, 4 K B read and 4 B written per sample."""
    _require(grads, "grads")
    if grads.dim() < 3:
        raise ValueError(f"grads: expected (K, B, ...), got {tuple(grads.shape)}")
    like = grads[0]
    B, T = _rows(like, "grads[0]")
    K, L = _channel_params(taps, shift, gain, B, grads.device)
    if K != grads.shape[0]:
        raise ValueError(f"grads holds {grads.shape[0]} draws, the parameters {K}")
    out = _out_like(like, out)
    _call("advstep_channel_adjoint_f32", grads.device, grads, taps, shift, gain, out, B, T, K, L,
          bracket="channel_adjoint", work=2.0 * K * L * B * T, tensors=(grads, out))
    return out


def channel_eot_step(adv, orig, grads, taps, shift, gain, alpha: float, eps: float, lo: float = 0.0, hi: float = 1.0, out=None):
    """`pgd_linf_step(adv, channel_adjoint(grads, taps, shift, gain), orig, alpha, eps)` byte for byte, in one launch: the summed
    gradient stays in registers.  4 K + 12 B per sample.  `out` may be `adv`."""
    _require(adv, "adv"), _require(orig, "orig")
    _same_shape(("adv", adv), ("orig", orig))
    B, T = _rows(adv, "adv")
    Kg = _channel_grads(grads, adv)
    K, L = _channel_params(taps, shift, gain, B, adv.device)
    if K != Kg:
        raise ValueError(f"grads holds {Kg} draws, the parameters {K}")
    out = _out_like(adv, out)
    _call("advstep_channel_eot_step_f32", adv.device, adv, orig, grads, taps, shift, gain, out, B, T, K, L, alpha, eps, lo, hi,
          bracket="channel_eot_step", work=2.0 * K * L * B * T, tensors=(adv, orig, grads, out))
    return out


# ---------------------------------------------------------------------------------------------------------
# universal adversarial filter (include/advstep_filter.h): one FIR for the batch, the gradient of its taps and their Adam step
# ---------------------------------------------------------------------------------------------------------

FILTER_MAX_TAPS = 1025                          # ADVSTEP_FILTER_MAX_TAPS
FILTER_GROUP_ROWS = 16                          # ADVSTEP_FILTER_GROUP_ROWS: rows per group of the fold over rows
_FILTER_TILE = 4096                             # samples of a row that one workgroup filters


def _filter_taps(taps, device, name: str = "taps") -> int:
    """L of a filter: `taps` holds an odd number of float32 values, 1 .. FILTER_MAX_TAPS, on `device`."""
    _require(taps, name)
    L = int(taps.numel())
    if not 1 <= L <= FILTER_MAX_TAPS or L % 2 == 0:
        raise ValueError(f"a filter has an odd number of taps between 1 and {FILTER_MAX_TAPS}, got {L}")
    _on_device(taps, name, device)
    return L


def _filter_workspace(device: torch.device, B: int, T: int, L: int) -> Tuple[int, int]:
    # the (tile, row) partials of the tap gradient, rewritten by every filter_tap_grad: keyed by stream like the row workspace
    key = (device.index if device.index is not None else torch.cuda.current_device(), _stream(device), int(B), int(T), "filter", int(L))
    nbytes = _lib.load().advstep_filter_workspace_bytes(B, T, L)
    return _scratch(key, lambda: torch.empty(max(nbytes, 256), dtype=torch.uint8, device=device))


def filter_apply(x, center, taps, row_mask=None, lo: float = 0.0, hi: float = 1.0, out=None):
    """out[b] = clamp(c_b + FIR(taps, x_b - c_b), lo, hi) for the rows with row_mask[b] != 0 (None: every row), x_b's bits for the
    others: ONE centred filter of L taps (odd, <= 1025) for the batch, with silence (c = `center`, one value per row) outside the
    utterance; include/advstep_filter.h fixes the arithmetic.  One launch, 8 B per sample, no host read.  `out` may be `x`: where
    rows are longer than a 4096-sample tile (and L > 1) the launch cannot run in place, and the rows are filtered into a scratch
    tensor that is then copied over `x`."""
    _require(x, "x")
    B, T = _rows(x, "x")
    _per_row(center, "center", B, device=x.device)
    L = _filter_taps(taps, x.device)
    m = _optional_rows(row_mask, "row_mask", B, x.device)
    out = _out_like(x, out)
    in_place = out.data_ptr() == x.data_ptr() and T > _FILTER_TILE and L > 1
    dst = torch.empty_like(x) if in_place else out
    _call("advstep_filter_apply_f32", x.device, x, center, m, taps, dst, B, T, L, lo, hi,
          bracket="filter_apply", work=2.0 * L * B * T, tensors=(x, dst))
    if in_place:
        out.copy_(dst)
    return out


def filter_tap_grad(x, center, grad, out_adv, taps: int, row_mask=None, lo: float = 0.0, hi: float = 1.0) -> None:
    """The per-(tile, row) partials of d loss / d taps for a filter of `taps` taps, from grad = d loss / d out_adv and out_adv =
    filter_apply(x, ...): dh[i] = sum_b sum_t gm[b, t] (x - c)[b, t + P - i], gm = grad where the row is unmasked and lo < out_adv
    < hi, else 0.  They stay in this stream's workspace for `filter_tap_update` with the same (B, T, taps), which folds them: the
    gradient never needs a host read.  One launch, 12 B per sample."""
    _require(x, "x"), _require(grad, "grad"), _require(out_adv, "out_adv")
    B, T = _rows(x, "x")
    for name, t in (("grad", grad), ("out_adv", out_adv)):
        if t.numel() != x.numel() or t.device != x.device:
            raise ValueError(f"{name} must hold ({B}, {T}) values on {x.device}, got {tuple(t.shape)}@{t.device}")
    _per_row(center, "center", B, device=x.device)
    L = int(taps)
    if not 1 <= L <= FILTER_MAX_TAPS or L % 2 == 0:
        raise ValueError(f"a filter has an odd number of taps between 1 and {FILTER_MAX_TAPS}, got {L}")
    m = _optional_rows(row_mask, "row_mask", B, x.device)
    with _Launch("filter_tap_grad", x.device, work=2.0 * L * B * T, tensors=(x, grad, out_adv)):
        ws, ws_bytes = _filter_workspace(x.device, B, T, L)
        _call("advstep_filter_tap_grad_f32", x.device, x, center, m, grad, out_adv, ws, ws_bytes, B, T, L, lo, hi)


def filter_tap_update(taps, adam_m, adam_v, B: int, T: int, step: int, lr: float, beta1: float = 0.9, beta2: float = 0.999,
                      adam_eps: float = 1e-8, ascend: bool = True, dh_out=None):
    """Fold the partials `filter_tap_grad` left on this stream for a (B, T) batch into dh (L,) in the order the header fixes, and
    take one Adam step on `taps` along it, in place with its moments `adam_m`, `adam_v` (`step` is 1-based; ascend: the taps climb
    the loss).  dh_out (L,): also receives dh.  One small launch, no host read.  Returns dh_out."""
    L = _filter_taps(taps, taps.device)
    for name, t in (("adam_m", adam_m), ("adam_v", adam_v)) + ((("dh_out", dh_out),) if dh_out is not None else ()):
        _require(t, name)
        if t.numel() != L or t.device != taps.device:
            raise ValueError(f"{name} must hold one value per tap ({L}) on {taps.device}, got {tuple(t.shape)}@{t.device}")
    B, T, step = int(B), int(T), int(step)
    if B < 0 or T < 0 or step < 1:
        raise ValueError(f"B and T must not be negative and step is 1-based, got B {B}, T {T}, step {step}")
    with _Launch("filter_tap_update", taps.device, tensors=(taps, taps, adam_m, adam_m, adam_v, adam_v)):
        ws, _ = _filter_workspace(taps.device, B, T, L)
        _call("advstep_filter_tap_update_f32", taps.device, ws, taps, adam_m, adam_v, dh_out, B, T, L, step, lr, beta1, beta2,
              adam_eps, int(bool(ascend)))
    return dh_out


# ---------------------------------------------------------------------------------------------------------
# psychoacoustic masking (include/advstep_masking.h): the short-time power spectrum, the fused hinge with its gradient and the
# mixed step of torchattacks.PsyPGD; the threshold itself is torchattacks/masking.py's
# ---------------------------------------------------------------------------------------------------------

MASKING_NFFT, MASKING_BINS = 512, 257


def _masking_frames(t: torch.Tensor, window: torch.Tensor, hop: int) -> Tuple[int, int, int]:
    B, T = _rows(t, "a")
    _require(window, "window")
    if window.numel() != MASKING_NFFT or window.device != t.device:
        raise ValueError(f"window must hold {MASKING_NFFT} floats on {t.device}, got {tuple(window.shape)}@{window.device}")
    hop = int(hop)
    if not _lib.load().advstep_stft_bands_supported(MASKING_NFFT, hop, T):
        raise ValueError(f"unsupported framing: n_fft {MASKING_NFFT}, hop {hop}, T {T} (128 <= hop <= 512 and T > 257)")
    return B, T, 1 + T // hop


def stft_power(a, b, window, hop: int, out=None):
    """(B, NF, 257) float32: |STFT|^2 of `a - b` (of `a` when `b` is None) in the frontend's framing — n_fft 512, `window` (512),
    centre framing with reflect padding, NF = 1 + T // hop.  One launch; the difference is formed in registers."""
    _require(a, "a")
    if b is not None:
        _require(b, "b")
        _same_shape(("a", a), ("b", b))
    B, T, NF = _masking_frames(a, window, hop)
    out = _shaped(out, "out", (B, NF, MASKING_BINS), a.device)
    _call("advstep_stft_power_f32", a.device, a, b, window, out, B, T, NF, int(hop), MASKING_NFFT,
          bracket="stft_power", tensors=(a, out) if b is None else (a, b, out))
    return out


def masking_hinge_grad(adv, x, window, theta, row_scale, hop: int, out=None, stats=None):
    """The masking hinge of `adv - x` against `theta` (B, NF, 257) with the row scales `row_scale` (B): returns (grad, stats) —
    grad (B, T) = d loss_b / d adv, stats (B, 3) = (loss_b = s_b sum max(P - theta, 0), #{P > theta}, max P / theta).  A zero fill
    and ONE launch: forward and backward share the spectrum in registers.  `out` / `stats`: buffers to write into."""
    _require(adv, "adv"), _require(x, "x"), _require(theta, "theta")
    _same_shape(("adv", adv), ("x", x))
    B, T, NF = _masking_frames(adv, window, hop)
    if tuple(theta.shape) != (B, NF, MASKING_BINS) or theta.device != adv.device:
        raise ValueError(f"theta must be {(B, NF, MASKING_BINS)} on {adv.device}, got {tuple(theta.shape)}@{theta.device}")
    _per_row(row_scale, "row_scale", B, device=adv.device)
    out = _out_like(adv, out)
    stats = _shaped(stats, "stats", (B, 3), adv.device)
    _call("advstep_masking_hinge_grad_f32", adv.device, adv, x, window, theta, row_scale, out, stats, B, T, NF, int(hop),
          MASKING_NFFT, bracket="masking_hinge_grad", tensors=(adv, x, theta, out, out))
    return out, stats


def psy_step(cur, g_ce, g_mask, x, lam: float, step: float, eps: float, out=None):
    """out = clamp(x + clamp(cur + step * sign(u) - x, -eps, eps), 0, 1) with u = g_ce / mean|g_ce| - lam * g_mask / mean|g_mask|
    per row (a term whose mean is 0 is dropped).  lam == 0: `pgd_linf_step(cur, g_ce, x, step, eps)` bit for bit, and `g_mask`
    may be None.  One launch; `out` may be `cur`."""
    named = [("cur", cur), ("g_ce", g_ce), ("x", x)]
    if g_mask is not None:
        named.append(("g_mask", g_mask))
    elif lam != 0:
        raise ValueError("g_mask may only be None when lam == 0")
    for name, t in named:
        _require(t, name)
    _same_shape(*named)
    if not (lam >= 0 and step >= 0 and eps >= 0):
        raise ValueError(f"lam, step and eps must be non-negative, got {lam!r}, {step!r}, {eps!r}")
    B, T = _rows(cur, "cur")
    out = _out_like(cur, out)
    _call("advstep_psy_step_f32", cur.device, cur, g_ce, g_mask, x, float(lam), float(step), float(eps), out, B, T,
          bracket="psy_step", tensors=tuple(t for _, t in named) + (out,))
    return out
