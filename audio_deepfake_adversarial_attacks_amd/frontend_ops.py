"""The LFCC frontend after the STFT as one differentiable op backed by the HIP kernels of include/advstep_frontend.h
(SURVEY.md section 8-f2): power -> sparse linear filterbank -> dB with the batch-wide floor -> DCT, forward and
backward, written frame-major so LCNN's first block reads it without a transpose copy.

`lfcc_tail(spec, tables, dct, top_db)` takes torch.stft's complex output (B, F, NF) and returns (B, K, NF) — a view of
a contiguous (B, NF, K) buffer; `lfcc_from_waveform` starts from the waveform; `fused_cepstrum` chooses between them for
frontends.LFCC and frontends.MFCC.  Numerically it follows frontends.LFCC (this repository's restatement of torchaudio's
LFCC) to float rounding, including torchaudio's gradient path through `amax` (floored gradients flow to the batch
maximum); tests/test_gpu_frontend_ops.py.  HIP tensors only."""
from __future__ import annotations

import os
from typing import NamedTuple, Optional

import torch

from . import _lib, fft_plans
from .hip_ops import _Launch, _call
from .lcnn_ops import _IdKeyed


def enabled(switch: str) -> bool:
    """The frontend's A/B switches, each on unless set to "0" and read at call time (tests flip them; torchattacks/graphed.py
    keys its captures on the environment):
      ADVSTEP_FUSED_LFCC=0           LFCC / MFCC run the plain torch op chain;
      ADVSTEP_FUSED_STFT=0           torch.stft (pad + strided frames + clone) in front of the fused LFCC tail;
      ADVSTEP_INLDS_FFT=0            framing kernel + hipFFT + filterbank kernel instead of the in-LDS FFT kernels;
      ADVSTEP_DIRECT_FFT=0           that path's FFTs through torch.fft instead of the direct hipFFT plans;
      ADVSTEP_FUSED_MEL=0            the mel-spec frontend runs the plain torch op chain;
      ADVSTEP_MEL_BWD_FROM_OUTPUT=0  the mel-spec backward recomputes the spectrum from the waveform."""
    return os.environ.get(switch, "1") != "0"


class FilterbankTables(NamedTuple):
    """Sparse form of a (F, M) triangular filterbank: per band the first bin + `span` weights, and the transpose."""
    fb_start: torch.Tensor   # (M,) int32
    fb_w: torch.Tensor       # (M, span) float32
    span: int
    fbt_start: torch.Tensor  # (F,) int32
    fbt_w: torch.Tensor      # (F, span_t) float32
    span_t: int


def filterbank_tables(filter_mat: torch.Tensor) -> FilterbankTables:
    fb = filter_mat.detach().float().cpu()
    F, M = fb.shape

    def pack(mat):  # rows of `mat` are the outputs; gather each row's non-zero run
        n_out = mat.shape[0]
        starts, spans = [], []
        for r in range(n_out):
            nz = torch.nonzero(mat[r]).flatten()
            starts.append(int(nz.min()) if nz.numel() else 0)
            spans.append(int(nz.max()) - int(nz.min()) + 1 if nz.numel() else 1)
        span = max(spans)
        w = torch.zeros(n_out, span)
        for r in range(n_out):
            hi = min(starts[r] + span, mat.shape[1])
            w[r, : hi - starts[r]] = mat[r, starts[r]:hi]
        return torch.tensor(starts, dtype=torch.int32), w, span

    fb_start, fb_w, span = pack(fb.t().contiguous())      # per band over bins
    fbt_start, fbt_w, span_t = pack(fb)                    # per bin over bands
    dev = filter_mat.device
    return FilterbankTables(fb_start.to(dev), fb_w.to(dev).contiguous(), span, fbt_start.to(dev),
                            fbt_w.to(dev).contiguous(), span_t)


_FRAGMENTS = _IdKeyed()      # weak, keyed by tensor identity


def dct_fragments(dct: torch.Tensor) -> Optional[torch.Tensor]:
    """The DCT matrix in the operand order of the matrix-core projection kernels (advstep_lfcc_project_prepare_f32), cached
    per tensor object and version (the entry dies with the tensor: a recycled address cannot hit it); None for sizes without
    such a path."""
    lib = _lib.load()
    M, K = dct.shape
    n = lib.advstep_lfcc_project_fragment_floats(M, K)
    if n == 0 or not dct.is_contiguous():
        return None
    key = (dct.data_ptr(), dct._version, str(dct.device))
    hit = _FRAGMENTS.get(dct)
    if hit is not None and hit[0] == key:
        return hit[1]
    if torch.cuda.is_current_stream_capturing():
        # a table built inside a capture would be filled only when the graph replays, and this cache would hand it to eager
        # callers before that: take the two-launch path for this call (graphed.py warms up eagerly, so this does not happen
        # on the shipped path)
        return None
    frag = torch.empty(n, dtype=torch.float32, device=dct.device)
    _call("advstep_lfcc_project_prepare_f32", dct.device, dct, M, K, frag)
    # once per weight version: the table is shared by every stream that calls later, so it must be complete before it is
    # published (a second stream's first call is not ordered behind this launch)
    torch.cuda.current_stream(dct.device).synchronize()
    _FRAGMENTS[dct] = (key, frag)
    return frag


def _rearm(ctx, stats: torch.Tensor) -> None:
    """A further backward pass through the same forward (retain_graph): the floored-gradient sum the previous one accumulated
    in `stats[2]` starts again from 0 - and so does the tie counter `stats[1]` where the backward pass is the one that fills it
    (the matrix-core path: stats[3] == 1; the two-launch forward counts the ties itself).  `stats` is this node's own scratch,
    kept as a plain attribute of ctx - NOT among the saved tensors, whose version check would refuse the third pass after
    this in-place reset - and so is the fragment table the forward pass chose: who counts the ties was decided
    there, the backward pass must not look the table up again (a cache miss would hand it the other kernel)."""
    if ctx.backward_calls:
        if ctx.ties_in_backward:
            stats[1:3].zero_()
        else:
            stats[2:3].zero_()
    ctx.backward_calls += 1


class _Lfcc(torch.autograd.Function):
    """The LFCC frontend from one of three spectrum sources, then the same two launches each way: [filterbank + dB] ->
    [batch max + floor + DCT]; backward: [DCT^T + floor mask + dB' + tie count] -> [floor fix-up + filterbank^T].
      "tail":   `x` is torch.stft's complex output (B, F, NF); the gradient returned is complex.
      "frames": `x` is the waveform (B, T): framing kernel -> hipFFT r2c in front, hipFFT c2r -> overlap-add kernel behind
                (torch.fft with ADVSTEP_DIRECT_FFT=0).  No padded copy, no strided-frame clone, no index_add.
      "fused":  `x` is the waveform, the STFT inside the kernels: framing + FFT + power join the filterbank launch, and the
                backward's second launch is [floor fix-up + filterbank^T + spectrum recomputed + inverse FFT + window +
                overlap-add], with dx zero-filled by the first."""

    @staticmethod
    def forward(ctx, source: str, x, window, hop, tables: FilterbankTables, dct, top_db: float):
        fused = source == "fused"
        M, K = dct.shape
        dev = x.device
        lib = _lib.load()
        if source == "tail":
            B, F, NF = x.shape
            T = nfft = None
            sn = x.transpose(1, 2)
            if not sn.is_contiguous():       # torch.stft's native layout is already (B, NF, F)
                sn = sn.contiguous()
            spec = torch.view_as_real(sn)    # (B, NF, F, 2) float32
        else:
            B, T = x.shape
            nfft = window.numel()
            NF, F = 1 + T // hop, nfft // 2 + 1
            spec = x if fused else _frames_rfft(x, window, hop, NF)
        band_db = torch.empty((B, NF, M), dtype=torch.float32, device=dev)
        nblk = lib.advstep_stft_bands_block_count(B, NF) if fused else lib.advstep_lfcc_block_count(B, M, NF)
        block_max = torch.empty(max(nblk, 1), dtype=torch.float32, device=dev)
        stats = torch.empty(4, dtype=torch.float32, device=dev)
        out = torch.empty((B, NF, K), dtype=torch.float32, device=dev)
        frag = dct_fragments(dct)
        # bytes on the fused path: waveform in, band rows out + back in, cepstra out
        with _Launch("lfcc_forward", dev, tensors=(x, band_db, band_db, out) if fused else ()):
            if fused:
                _call("advstep_stft_bands_f32", dev, x, window, tables.fb_start, tables.fb_w, tables.span, band_db, block_max,
                      B, T, NF, hop, nfft, M)
            else:
                _call("advstep_lfcc_bands_f32", dev, spec, tables.fb_start, tables.fb_w, tables.span, band_db, block_max,
                      B, F, M, NF)
            # batch maximum + floor + DCT: one launch (every workgroup reduces the block maxima itself)
            _call("advstep_lfcc_max_project_f32", dev, band_db, dct, frag, block_max, nblk, stats, top_db, out, B, M, NF, K)
        ctx.save_for_backward(spec, band_db, dct, tables.fbt_start, tables.fbt_w, window)
        ctx.stats, ctx.frag = stats, frag      # not saved tensors: see _rearm
        ctx.meta = (source, B, T, F, NF, M, K, tables.span_t, float(top_db), hop, nfft)
        ctx.backward_calls = 0
        ctx.ties_in_backward = frag is not None and M == 128 and K == 80
        return out.transpose(1, 2)

    @staticmethod
    def backward(ctx, gout):
        spec, band_db, dct, fbt_start, fbt_w, window = ctx.saved_tensors
        stats, frag = ctx.stats, ctx.frag
        source, B, T, F, NF, M, K, span_t, top_db, hop, nfft = ctx.meta
        fused = source == "fused"
        dev = gout.device
        go = gout.transpose(1, 2).contiguous()     # (B, NF, K); a no-op when the consumer is frame-major
        dband = torch.empty((B, NF, M), dtype=torch.float32, device=dev)
        if fused:
            dx = torch.empty((B, T), dtype=torch.float32, device=dev)
        else:
            dspec = torch.empty((B, NF, F, 2), dtype=torch.float32, device=dev)
        _rearm(ctx, stats)
        with _Launch("lfcc_backward", dev, tensors=(go, band_db, dband, dband, spec, dx, dx) if fused else ()):
            # on the fused path this also zero-fills dx, which the overlap-add of the second launch accumulates into
            _call("advstep_lfcc_project_backward_zero_f32", dev, go, dct, frag, band_db, stats, top_db, dband, B, M, NF, K,
                  dx if fused else None, dx.numel() if fused else 0)
            if fused:
                _call("advstep_stft_bands_backward_fixup_f32", dev, spec, window, dband, band_db, stats, fbt_start, fbt_w, span_t,
                      dx, 1, B, T, NF, hop, nfft, M)
            else:
                _call("advstep_lfcc_floor_fixup_f32", dev, band_db, stats, dband, band_db.numel())
                # hermitian_half on the frames path: its c2r inverse takes the pre-scaled half spectrum
                _call("advstep_lfcc_bands_backward_f32", dev, dband, spec, fbt_start, fbt_w, span_t, dspec, B, F, M, NF,
                      int(source == "frames"))
        if source == "tail":
            return None, torch.view_as_complex(dspec).transpose(1, 2), None, None, None, None, None
        if source == "frames":
            dx = _irfft_overlap_add(dspec, window, hop, T)
        return None, dx, None, None, None, None, None


def _frames_rfft(x: torch.Tensor, window: torch.Tensor, hop: int, NF: int) -> torch.Tensor:
    """Framing kernel -> one-sided r2c FFT: (B, T) -> the interleaved complex spectrum (B, NF, F, 2)."""
    B, T = x.shape
    nfft = window.numel()
    F = nfft // 2 + 1
    dev = x.device
    frames = torch.empty((B, NF, nfft), dtype=torch.float32, device=dev)
    _call("advstep_stft_frames_f32", dev, x, window, frames, B, T, NF, hop, nfft, bracket="stft_frames")
    sr = torch.empty((B, NF, F, 2), dtype=torch.float32, device=dev)
    if not (enabled("ADVSTEP_DIRECT_FFT") and fft_plans.rfft_into(frames.view(B * NF, nfft), sr.view(B * NF, F, 2))):
        sr = torch.view_as_real(torch.fft.rfft(frames, dim=-1))           # same library, plus a defensive input clone
    return sr


def _irfft_overlap_add(dspec: torch.Tensor, window: torch.Tensor, hop: int, T: int) -> torch.Tensor:
    """The adjoint of _frames_rfft: spectrum gradient (B, NF, F, 2) -> waveform gradient (B, T)."""
    B, NF, F, _ = dspec.shape
    nfft = window.numel()
    dev = dspec.device
    # gradient of the one-sided real FFT = unnormalised c2r inverse of the pre-scaled half spectrum
    dframes = torch.empty((B, NF, nfft), dtype=torch.float32, device=dev)
    if not (enabled("ADVSTEP_DIRECT_FFT") and fft_plans.irfft_into(dspec.view(B * NF, F, 2), dframes.view(B * NF, nfft))):
        dframes = torch.fft.irfft(torch.view_as_complex(dspec), n=nfft, dim=-1, norm="forward").contiguous()
    dx = torch.empty((B, T), dtype=torch.float32, device=dev)
    _call("advstep_stft_overlap_add_f32", dev, dframes, window, dx, B, T, NF, hop, nfft, bracket="stft_overlap_add")
    return dx


def lfcc_from_waveform(x: torch.Tensor, window_nfft: torch.Tensor, hop: int, tables: FilterbankTables, dct: torch.Tensor,
                       top_db: float = 80.0) -> torch.Tensor:
    """Waveform (B, T) -> LFCC (B, K, 1 + T // hop); `window_nfft` is the analysis window zero-padded (centred) to n_fft."""
    if not x.is_cuda or x.dtype != torch.float32 or x.dim() != 2:
        raise _lib.AdvstepError("lfcc_from_waveform needs a float32 (B, T) waveform on a HIP device (no CPU fallback)")
    inlds = enabled("ADVSTEP_INLDS_FFT") and _lib.load().advstep_stft_bands_supported(window_nfft.numel(), hop, x.shape[1])
    return _Lfcc.apply("fused" if inlds else "frames", x.contiguous(), window_nfft, hop, tables, dct, top_db)


def lfcc_tail(spec: torch.Tensor, tables: FilterbankTables, dct: torch.Tensor, top_db: float = 80.0) -> torch.Tensor:
    """Complex STFT (B, F, NF) -> LFCC (B, K, NF) (view of a frame-major buffer)."""
    if not spec.is_cuda or spec.dtype != torch.complex64 or spec.dim() != 3:
        raise _lib.AdvstepError("lfcc_tail needs a complex64 (B, F, NF) STFT on a HIP device (no CPU fallback)")
    return _Lfcc.apply("tail", spec, None, None, tables, dct, top_db)


def fused_cepstrum(x: torch.Tensor, window_nfft, hop: int, tables, dct: torch.Tensor, top_db: float) -> Optional[torch.Tensor]:
    """Waveform (B, T) -> filterbank -> dB -> DCT of its power STFT through the fused kernels (LFCC, or MFCC with a mel bank),
    or None where none applies and the caller runs the torch op chain.  `window_nfft` and `tables` are the caller's cached
    derivations of its buffers, passed as zero-argument callables so that they are built only once a kernel applies."""
    M, K = dct.shape
    if not (x.is_cuda and x.dim() == 2 and x.dtype == torch.float32 and enabled("ADVSTEP_FUSED_LFCC")
            and M <= 128 and K in (20, 40, 80)):
        return None
    tables, window = tables(), window_nfft()
    nfft = window.numel()
    if x.shape[1] > nfft // 2 and nfft % 4 == 0 and enabled("ADVSTEP_FUSED_STFT"):
        # framing, FFT, filterbank, dB in one kernel; floor + DCT in another (and two more on the way back)
        return lfcc_from_waveform(x, window, hop, tables, dct, top_db)
    # (torch.stft pads a window shorter than n_fft the same way)
    spec = torch.stft(x, n_fft=nfft, hop_length=hop, window=window, center=True, pad_mode="reflect", normalized=False,
                      onesided=True, return_complex=True)
    return lfcc_tail(spec, tables, dct, top_db)


class _MelSpecFromWaveform(torch.autograd.Function):
    """The mel-spec frontend (src/frontends.py:53-79) with the STFT inside the kernels: (B, T) -> (B, 2, M, NF)."""

    @staticmethod
    def forward(ctx, x, window, hop, tables: FilterbankTables):
        B, T = x.shape
        nfft = window.numel()
        NF = 1 + T // hop
        M = tables.fb_start.numel()
        dev = x.device
        out = torch.empty((B, 2, M, NF), dtype=torch.float32, device=dev)
        _call("advstep_stft_mel_f32", dev, x, window, tables.fb_start, tables.fb_w, tables.span, out, B, T, NF, hop, nfft, M,
              bracket="stft_mel", tensors=(x, out))
        ctx.from_output = enabled("ADVSTEP_MEL_BWD_FROM_OUTPUT")
        ctx.save_for_backward(out if ctx.from_output else x, window, tables.fb_start, tables.fb_w, tables.fbt_start, tables.fbt_w)
        ctx.meta = (B, T, NF, M, tables.span, tables.span_t, hop, nfft)
        return out

    @staticmethod
    def backward(ctx, gout):
        x, window, fb_start, fb_w, fbt_start, fbt_w = ctx.saved_tensors
        B, T, NF, M, span, span_t, hop, nfft = ctx.meta
        dev = gout.device
        go = gout.contiguous()
        dx = torch.empty((B, T), dtype=torch.float32, device=dev)
        if ctx.from_output:
            # d x from d out and out alone (Y = |Y| e^{i phase} is all the gradient needs): no spectrum is recomputed
            _call("advstep_stft_mel_backward_from_output_f32", dev, window, go, x, fbt_start, fbt_w, span_t, dx, B, T, NF, hop, nfft,
                  M, bracket="stft_mel_backward", tensors=(go, x, dx, dx))
            return dx, None, None, None
        _call("advstep_stft_mel_backward_f32", dev, x, window, go, fb_start, fb_w, span, fbt_start, fbt_w, span_t, dx, B, T, NF, hop,
              nfft, M, bracket="stft_mel_backward", tensors=(go, x, dx, dx))
        return dx, None, None, None


def mel_spec_supported(nfft: int, hop: int, T: int, n_mels: int, span: int = 1, span_t: int = 1) -> bool:
    return bool(_lib.load().advstep_stft_bands_supported(nfft, hop, T)) and n_mels <= 80 and span <= 48 and span_t <= 8


def mel_spec_from_waveform(x: torch.Tensor, window_nfft: torch.Tensor, hop: int, tables: FilterbankTables) -> torch.Tensor:
    """Waveform (B, T) -> (B, 2, n_mels, 1 + T // hop): magnitude and phase of the mel-projected complex STFT."""
    if not x.is_cuda or x.dtype != torch.float32 or x.dim() != 2:
        raise _lib.AdvstepError("mel_spec_from_waveform needs a float32 (B, T) waveform on a HIP device (no CPU fallback)")
    return _MelSpecFromWaveform.apply(x.contiguous(), window_nfft, hop, tables)

