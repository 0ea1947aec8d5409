"""The STFT frontend kernels (csrc/lfcc_stft.hip, csrc/lfcc.hip) against float64 references, element by element, on every
launch path: the LFCC / MFCC cepstra and the mel-spec frontend end to end (values and waveform gradients), and the C-ABI stages
one at a time (band dB, floor + DCT, the band and mel adjoints), with the stores checked against sentinel-filled allocations and
every path run twice for bit-reproducibility.

The reference is this repository's own arithmetic (frontends.py, a restatement of torchaudio's) evaluated in float64 on the CPU
with explicit framing: reflect pad by n_fft / 2, frames at f * hop, the module's float32 window promoted and centred in n_fft,
rfft, |X|^2, the module's filterbank, 10 log10 clamp(., 1e-10), the batch-wide floor at max - 80 dB with torch's `amax` /
`maximum` gradient routing, the module's DCT; for the mel-spec frontend the rectangular-window STFT, the mel bank on the real
and imaginary parts, magnitude and phase.  Gradients are float64 autograd.  The reference itself is held (without a GPU)
against the modules' plain chain in float64 and against tests/golden/frontends_xcheck.npz.

Bounds are per element: cepstra and mel magnitude to tau * max|ref|, waveform gradients to tau_g * max|ref| per utterance.  On
the ill-conditioned inputs (DC-heavy, tones, floored batches) float32 power has a large relative error in weak bands that the
log amplifies; there the kernel's error is bounded by a stated multiple of the plain float32 chain's error on the same case.
Bands within DELTA_DB of the floor in float64 may legally take either side: they are counted (a handful at most) and the
reference is evaluated with each of them on either side."""
import itertools
import math
import zlib

import pytest
import torch
import torch.nn.functional as Fn

from audio_deepfake_adversarial_attacks_amd import frontends

NFFT = 512
TOP_DB = 80.0

# ---- bounds, calibrated on gfx950: each is at most 4x the worst error measured for it (in brackets; all figures are written
# to parity_record under stft_f64_*) and tighter than the torch-chain tolerances of tests/test_gpu_frontend_ops.py -------------
TAU_CEPS = 2.5e-6        # cepstra, well-conditioned input: max |y - y64| / max |y64|  [7.3e-7; plain float32 chain 7.3e-7]
TAU_CEPS_GRAD = 4e-5     # their waveform gradient, per utterance over max |dx64[b]|  [1.4e-5 (MFCC); plain chain 1.4e-5]
TAU_MEL = 1.5e-6         # mel magnitude, every input (no log) over max |m64|  [4.8e-7; plain chain 5.2e-7]
TAU_MEL_PHASE = 4e-4     # mel phase in radians where |Y| > 1e-3 max |Y|  [1.5e-4; plain chain 2.8e-4]
TAU_MEL_GRAD = 4e-5      # waveform gradient of the mel-spec frontend, per utterance  [1.7e-5; plain chain 2.2e-5]
RATIO_ILL = 3.0          # ill-conditioned input: error <= fixed bound + RATIO_ILL x the plain chain's  [1.2 values, 1.95 gradients]
TAU_STAGE_POWER = 2e-7   # band power of advstep_stft_bands_f32 over the frame's one-sided energy  [5.1e-8]
TAU_STAGE_PROJECT = 2e-6  # floor + DCT on the kernel's own band_db, over max |out64|  [8.9e-7]
TAU_STAGE_ADJ = 6e-7     # band adjoint from a given band gradient, per utterance  [1.8e-7]
TAU_STAGE_MEL_GRAD = 1e-5  # mel adjoints from a given cotangent, per utterance  [2.8e-6]
DELTA_DB = 1e-2          # a band this close to the floor (float64) may be floored or not  [at most 1 per case]
MAX_AMBIGUOUS = 4


# ---- float64 references (CPU) -------------------------------------------------------------------------------------------------

def centred_window(window, n_fft=NFFT):
    """The analysis window promoted to float64 and zero-padded (centred) to n_fft, as frontends._cached_window_nfft does."""
    w = window.detach().cpu().double()
    out = torch.zeros(n_fft, dtype=torch.float64)
    left = (n_fft - w.numel()) // 2
    out[left:left + w.numel()] = w
    return out


def ref_spectrum(x, wpad, hop):
    """torch.stft(center=True, reflect, window) by hand: (B, T) -> complex (B, 1 + T // hop, n_fft // 2 + 1)."""
    n = wpad.numel()
    xp = Fn.pad(x.unsqueeze(1), (n // 2, n // 2), mode="reflect").squeeze(1)
    return torch.fft.rfft(xp.unfold(-1, n, hop) * wpad, dim=-1)


def ref_band_power(x, wpad, hop, fb):
    X = ref_spectrum(x, wpad, hop)
    return (X.real ** 2 + X.imag ** 2) @ fb                               # (B, NF, M)


def ref_band_db(x, wpad, hop, fb):
    """Band dB before the floor, (B, NF, M)."""
    return 10.0 * torch.log10(torch.clamp(ref_band_power(x, wpad, hop, fb), min=1e-10))


def ref_floor_dct(db, dct, top_db=TOP_DB, flip=None):
    """The batch-wide floor (torch.max against amax - top_db: ties at the maximum share its gradient, a band equal to the floor
    sends half its gradient each way) and the DCT: (B, NF, M) -> (B, NF, K).  `flip`: a bool mask of bands that take the other
    side of the floor decision (decision-ambiguous bands)."""
    floor = db.amax() - top_db
    if flip is None or not flip.any():
        return torch.maximum(db, floor) @ dct
    keep = (db > floor) ^ flip
    return torch.where(keep, db, floor) @ dct


def ref_cepstrum(x, p, flip=None):
    """LFCC / MFCC (B, T) -> (B, NF, K) in float64; p = params_of(module)."""
    return ref_floor_dct(ref_band_db(x, p["window"], p["hop"], p["fb"]), p["dct"], flip=flip)


def ref_mel(x, p):
    """MelSpecFrontend (B, T) -> (B, 2, M, NF) in float64."""
    X = ref_spectrum(x, p["window"], p["hop"])
    Y = torch.complex(X.real @ p["fb"], X.imag @ p["fb"])
    return torch.stack([Y.abs(), Y.angle()], 1).transpose(-1, -2)


def params_of(fe):
    """Window / hop / filterbank / DCT of a frontend module, in float64 on the CPU."""
    if isinstance(fe, frontends.MelSpecFrontend):
        rect = torch.ones(fe.win_length, dtype=torch.float64)
        return {"window": centred_window(rect), "hop": fe.hop_length, "fb": fe.mel_scale.fb.detach().cpu().double()}
    if isinstance(fe, frontends.LFCC):
        sg, fb = fe.Spectrogram, fe.filter_mat
    else:
        sg, fb = fe.MelSpectrogram.spectrogram, fe.MelSpectrogram.mel_scale.fb
    return {"window": centred_window(sg.window), "hop": sg.hop_length, "fb": fb.detach().cpu().double(),
            "dct": fe.dct_mat.detach().cpu().double()}


def ref_adjoint_bands(x, p, dband):
    """dx from d loss / d(band power) (B, NF, M): the adjoint of the band stage at fixed x."""
    a = x.detach().cpu().double().requires_grad_(True)
    (g,) = torch.autograd.grad(ref_band_power(a, p["window"], p["hop"], p["fb"]), a, dband.cpu().double())
    return g


def wide_bank(n_bins, M, step, widths, seed):
    """A non-triangular bank of overlapping wide bands (band m covers bins [step m, step m + widths[m % len]) with positive
    weights): up to max(widths) / step bands per bin, so the kernels' span_t > 2 instantiations run."""
    g = torch.Generator().manual_seed(seed)
    fb = torch.zeros(n_bins, M)
    for m in range(M):
        s = min(step * m, n_bins - 1)
        e = min(s + widths[m % len(widths)], n_bins)
        fb[s:e, m] = 0.2 + 0.8 * torch.rand(e - s, generator=g)
    return fb


# ---- the CPU self-check of the reference ----------------------------------------------------------------------------------------

def make_frontend(kind, hop=160, win=400, n_filter=128, n_ceps=80):
    if kind == "lfcc":
        return frontends.LFCC(n_filter=n_filter, n_lfcc=n_ceps, win_length=win, hop_length=hop)
    if kind == "mfcc":
        return frontends.MFCC(n_mfcc=n_ceps, win_length=win, hop_length=hop)
    return frontends.MelSpecFrontend(win_length=win, hop_length=hop)


@pytest.mark.parametrize("kind,hop,win,T", [("lfcc", 160, 400, 4_000), ("lfcc", 128, 512, 300), ("mfcc", 160, 400, 4_000),
                                            ("mfcc", 200, 320, 1_111), ("mel", 160, 400, 4_000), ("mel", 256, 512, 700)])
def test_reference_is_the_modules_float64_chain(kind, hop, win, T):
    """The explicit-framing reference against the modules' own plain chain (torch.stft) run as .double() on the CPU: values
    and gradients to 1e-12 of their scale, a floored batch included."""
    fe = make_frontend(kind, hop, win).double()
    g = torch.Generator().manual_seed(T + hop)
    x = (2 * torch.rand(3, T, generator=g, dtype=torch.float64) - 1)
    x[1] *= 1e-5                                  # -100 dB: floored
    x[2, T // 3: 2 * T // 3] = 0.0
    p = params_of(fe)
    a = x.clone().requires_grad_(True)
    b = x.clone().requires_grad_(True)
    y_mod = fe(a)
    if kind == "mel":
        y_ref = ref_mel(b, p)
        gy = torch.randn(y_ref.shape, generator=g, dtype=torch.float64)
        gy[:, 1] *= (y_ref[:, 0].detach() ** 2).clamp(max=1.0)
        z_mod, z_ref = torch.polar(y_mod[:, 0], y_mod[:, 1]), torch.polar(y_ref[:, 0], y_ref[:, 1])
        assert ((z_mod - z_ref).abs().max() / y_ref[:, 0].abs().max()).item() <= 1e-12
    else:
        y_ref = ref_cepstrum(b, p).transpose(1, 2)
        gy = torch.randn(y_ref.shape, generator=g, dtype=torch.float64)
        assert ((y_mod - y_ref).abs().max() / y_ref.abs().max()).item() <= 1e-12
    (g_mod,) = torch.autograd.grad(y_mod, a, gy)
    (g_ref,) = torch.autograd.grad(y_ref, b, gy)
    assert ((g_mod - g_ref).abs().max() / g_ref.abs().max()).item() <= 1e-12


@pytest.mark.parametrize("tag", ["full", "short", "loud"])
def test_reference_matches_independent_implementation(golden, tag):
    """The same fixture and tolerances as tests/test_frontends.py holds the plain chain to."""
    from tests.test_frontends import lfcc_error, mel_error
    pl, pm = params_of(frontends.LFCC()), params_of(frontends.MelSpecFrontend())
    lfcc = lambda x: ref_cepstrum(x.double(), pl).transpose(1, 2)            # noqa: E731
    mel = lambda x: ref_mel(x.double(), pm)                                   # noqa: E731
    assert lfcc_error(lfcc, golden("frontends_xcheck"), tag) <= 1e-5
    assert mel_error(mel, golden("frontends_xcheck"), tag) <= 2e-5


# ---- inputs -------------------------------------------------------------------------------------------------------------------

WELL = ("noise",)


def make_input(family, B, T, seed):
    """(B, T) float32 on the CPU.  noise: broadband in [-1, 1] (well-conditioned); rand: torch.rand (DC-heavy); tone: a tone plus
    weak noise; floor: a silent and a partly silent utterance in the batch (the floor is active); tie: one partly silent utterance
    twice (an exact tie at the batch maximum); edge-first / edge-last: the batch maximum in the first / last frame (reflection
    region), floor active."""
    g = torch.Generator().manual_seed(seed)
    noise = lambda *s: 2 * torch.rand(*s, generator=g) - 1                  # noqa: E731
    if family == "noise":
        return noise(B, T)
    if family == "rand":
        return torch.rand(B, T, generator=g)
    if family == "tone":
        t = torch.arange(T, dtype=torch.float64) / 16_000
        f = 440.0 + 1_000.0 * torch.rand(B, 1, generator=g, dtype=torch.float64)
        return (0.5 * torch.sin(2 * math.pi * f * t)).float() + 1e-2 * noise(B, T)
    x = noise(max(B, 2), T)
    lo, hi = T // 4, T // 2
    if family == "floor":
        x[1] *= 1e-7
        x[-1, lo:hi] = 0.0
        return x[:B] if B >= 3 else x
    if family == "tie":
        x[0, lo:hi] = 0.0
        return x[:1].repeat(2, 1)
    if family in ("edge-first", "edge-last"):
        x *= 0.05
        x[:, lo:hi] = 0.0
        n = min(150, T // 4)
        sl = slice(0, n) if family == "edge-first" else slice(T - n, T)
        x[0, sl] = 8 * noise(n)
        return x
    raise ValueError(family)


# ---- running a module on a launch path ----------------------------------------------------------------------------------------

ENV_DEFAULTS = {"ADVSTEP_FUSED_LFCC": "1", "ADVSTEP_FUSED_MEL": "1", "ADVSTEP_FUSED_STFT": "1", "ADVSTEP_STFT_REG": "1",
                "ADVSTEP_INLDS_FFT": "1", "ADVSTEP_DIRECT_FFT": "1", "ADVSTEP_MEL_BWD_FROM_OUTPUT": "1"}
PATH_ENV = {
    "reg": {},                                                   # register-FFT kernels
    "radix4": {"ADVSTEP_STFT_REG": "0"},                         # the radix-4 in-LDS kernels
    "hipfft": {"ADVSTEP_INLDS_FFT": "0"},                        # framing kernel + hipFFT plans + band / project / overlap-add
    "torchfft": {"ADVSTEP_INLDS_FFT": "0", "ADVSTEP_DIRECT_FFT": "0"},
    "tail": {"ADVSTEP_FUSED_STFT": "0"},                         # torch.stft + lfcc_tail
    "from-wave": {"ADVSTEP_MEL_BWD_FROM_OUTPUT": "0"},           # mel backward recomputing the spectrum
    "plain-f32": {"ADVSTEP_FUSED_LFCC": "0", "ADVSTEP_FUSED_MEL": "0"},
}


def set_path(monkeypatch, path):
    for k, v in {**ENV_DEFAULTS, **PATH_ENV[path]}.items():
        monkeypatch.setenv(k, v)


def run(fe, x, gy, monkeypatch, path):
    set_path(monkeypatch, path)
    a = x.clone().requires_grad_(True)
    y = fe(a)
    (g,) = torch.autograd.grad(y, a, gy)
    return y.detach(), g


def build_module(variant, hop, win, cuda):
    """variant -> (module on the GPU, kind).  Custom banks go in through the modules' buffers (copy_ bumps _version)."""
    if variant == "lfcc":
        fe, kind = frontends.LFCC(win_length=win, hop_length=hop), "ceps"
    elif variant in ("lfcc-wide-fwd60", "lfcc-wide-fwd40"):
        fe, kind = frontends.LFCC(n_filter=int(variant[-2:]), win_length=win, hop_length=hop), "ceps"
    elif variant in ("lfcc-K20", "lfcc-K40"):
        fe, kind = frontends.LFCC(n_lfcc=int(variant[-2:]), win_length=win, hop_length=hop), "ceps"
    elif variant == "mfcc":
        fe, kind = frontends.MFCC(win_length=win, hop_length=hop), "ceps"
    elif variant == "lfcc-spant":
        fe, kind = frontends.LFCC(win_length=win, hop_length=hop), "ceps"
        fe.filter_mat.copy_(wide_bank(257, 128, 2, (4, 7, 10, 13, 16), 1))
    elif variant == "mfcc-spant":
        fe, kind = frontends.MFCC(win_length=win, hop_length=hop), "ceps"
        fe.MelSpectrogram.mel_scale.fb.copy_(wide_bank(257, 128, 2, (16, 5, 11, 8), 2))
    elif variant == "mel":
        fe, kind = frontends.MelSpecFrontend(win_length=win, hop_length=hop), "mel"
    elif variant == "mel-wide":
        fe, kind = frontends.MelSpecFrontend(win_length=win, hop_length=hop), "mel"
        fe.mel_scale = frontends.MelScale(32, frontends.SAMPLING_RATE, NFFT // 2 + 1, persistent=False)
    elif variant == "mel-spant":
        fe, kind = frontends.MelSpecFrontend(win_length=win, hop_length=hop), "mel"
        fe.mel_scale.fb.copy_(wide_bank(257, 80, 3, (24, 9, 15, 6, 21), 3))
    else:
        raise ValueError(variant)
    fe = fe.to(cuda)
    if variant.endswith("spant"):
        if kind == "mel":
            tables = fe._fused_state(cuda)[0]
        else:
            tables = frontends._cached_tables(fe, fe.filter_mat if variant.startswith("lfcc") else fe.MelSpectrogram.mel_scale.fb)
        assert 2 < tables.span_t <= 8, tables.span_t      # not silently a triangular bank (nor beyond the kernels' cap)
    return fe, kind


# ---- the error measures -------------------------------------------------------------------------------------------------------

def rel_max(a, ref):
    scale = ref.abs().max().item()
    return (a.double().cpu() - ref).abs().max().item() / scale if scale > 0 else float(a.abs().max().item() > 0) * math.inf


def grad_err(g, g64):
    """max over utterances of max |dx - dx64| / max |dx64| for that utterance; an utterance whose reference gradient is exactly
    zero (floored throughout) must come out exactly zero."""
    worst = 0.0
    for b in range(g64.shape[0]):
        scale = g64[b].abs().max().item()
        d = (g[b].double().cpu() - g64[b]).abs().max().item()
        worst = max(worst, d / scale if scale > 0 else (math.inf if d > 0 else 0.0))
    return worst


def phase_err(y, y64):
    big = y64[:, 0] > 1e-3 * y64[:, 0].abs().max()
    d = torch.remainder(y[:, 1].double().cpu() - y64[:, 1] + math.pi, 2 * math.pi) - math.pi
    return d[big].abs().max().item()


def ceps_reference(x, gy, p):
    """float64 cepstra + waveform gradient as a list of (value, gradient) pairs, one per combination of the floor decisions of
    the decision-ambiguous bands; their number; whether the floor is active anywhere."""
    xd = x.double()
    with torch.no_grad():
        db = ref_band_db(xd, p["window"], p["hop"], p["fb"])
        floor = db.amax() - TOP_DB
        amb = ((db - floor).abs() <= DELTA_DB) | (((db + 100.0).abs() <= DELTA_DB) & (db > floor + DELTA_DB))
    n_amb = int(amb.sum())
    assert n_amb <= MAX_AMBIGUOUS, n_amb
    floored = bool((db < floor).any())
    idx = amb.nonzero()
    variants = []
    for bits in itertools.product((False, True), repeat=n_amb):
        flip = torch.zeros_like(amb)
        for (b, f, m), on in zip(idx.tolist(), bits):
            flip[b, f, m] = on
        a = xd.clone().requires_grad_(True)
        y = ref_cepstrum(a, p, flip=flip).transpose(1, 2)
        (g,) = torch.autograd.grad(y, a, gy.cpu().double())
        variants.append((y.detach(), g))
    return variants, n_amb, floored


def ceps_errors(y, g, variants):
    """The smallest (value error, gradient error) over the legal reference variants (one unless bands are ambiguous)."""
    return min(((rel_max(y, yv), grad_err(g, gv)) for yv, gv in variants), key=lambda e: max(e[0] / TAU_CEPS, e[1] / TAU_CEPS_GRAD))


# ---- the launch-path matrix ---------------------------------------------------------------------------------------------------
# (path, module variant, family, B, T, hop, win)

def _matrix():
    rows = []
    shapes_all = [(3, 64_600, 160, 400), (1, 258, 160, 400), (2, 259, 128, 512), (8, 1_000, 200, 320), (1, 257, 160, 400),
                  (2, 3_000, 127, 400)]
    for path in ("reg", "radix4", "hipfft", "torchfft", "tail"):
        rows += [(path, "lfcc", "noise") + s for s in shapes_all]
    # NF = 32 / 33, 64 / 65, 128 / 129 at hop 160 (the forward and backward workgroup boundaries) and T around 512
    edges = [k * 160 + d for k in (32, 64, 128) for d in (-1, 0, 1)] + [400, 511, 512, 513, 64_000]
    hops = [(128, 300, 512), (128, 16_000, 400), (200, 513, 400), (200, 64_000, 320), (256, 600, 512), (256, 16_160, 400),
            (400, 777, 400), (400, 32_000, 320), (512, 1_025, 512), (512, 64_600, 400)]
    for path in ("reg", "radix4"):
        rows += [(path, "lfcc", "noise", 1 + 2 * (i % 2), T, 160, 400) for i, T in enumerate(edges)]
        rows += [(path, "lfcc", "noise", 2, T, hop, win) for hop, T, win in hops]
    for path in ("reg", "radix4", "hipfft"):
        for fam in ("rand", "tone", "floor", "tie", "edge-first", "edge-last"):
            rows.append((path, "lfcc", fam, 3, 16_160, 160, 400))
            rows.append((path, "lfcc", fam, 3, 1_111, 128, 512))
    for path in ("reg", "radix4"):
        for variant in ("lfcc-wide-fwd60", "lfcc-wide-fwd40", "lfcc-K20", "lfcc-K40", "mfcc", "lfcc-spant", "mfcc-spant"):
            rows.append((path, variant, "noise", 3, 16_160, 160, 400))
            rows.append((path, variant, "noise", 2, 300, 128, 512))
        for variant in ("mfcc", "lfcc-spant", "mfcc-spant"):
            rows.append((path, variant, "floor", 3, 8_000, 160, 400))
    rows.append(("hipfft", "mfcc", "noise", 3, 16_160, 160, 400))
    rows.append(("hipfft", "lfcc-spant", "noise", 2, 300, 128, 512))
    mel_shapes = [(3, 64_600, 160, 400), (1, 258, 160, 400), (2, 259, 128, 512), (3, 5_121, 160, 400), (2, 1_000, 256, 512),
                  (2, 16_000, 400, 400), (1, 600, 512, 512), (8, 10_239, 160, 320)]
    for path in ("reg", "radix4", "from-wave"):
        rows += [(path, "mel", "noise") + s for s in mel_shapes]
        rows += [(path, "mel-wide", "noise") + s for s in mel_shapes[:4]]
        rows += [(path, "mel-spant", "noise") + s for s in mel_shapes[:4]]
        rows += [(path, "mel", fam, 3, 16_160, 160, 400) for fam in ("floor", "tone")]
    return rows


MATRIX = _matrix()


def _id(row):
    path, variant, fam, B, T, hop, win = row
    return f"{variant}-{path}-{fam}-B{B}-T{T}-hop{hop}-win{win}"


@pytest.mark.gpu
@pytest.mark.parametrize("row", MATRIX, ids=[_id(r) for r in MATRIX])
def test_frontend_path_matches_float64(cuda, monkeypatch, parity_record, row):
    path, variant, fam, B, T, hop, win = row
    fe, kind = build_module(variant, hop, win, cuda)
    p = params_of(fe)
    seed = zlib.crc32(_id(row).encode()) % 100_003
    x = make_input(fam, B, T, seed)
    B = x.shape[0]
    g = torch.Generator().manual_seed(seed + 1)
    NF = 1 + T // hop
    rec, floored = {}, False
    if kind == "ceps":
        K = p["dct"].shape[1]
        gy = torch.randn(B, K, NF, generator=g)
        variants, n_amb, floored = ceps_reference(x, gy, p)
        xc, gyc = x.to(cuda), gy.to(cuda)
        y, dx = run(fe, xc, gyc, monkeypatch, path)
        assert y.shape == (B, K, NF)
        e_y, e_g = ceps_errors(y, dx, variants)
        yp, dxp = run(fe, xc, gyc, monkeypatch, "plain-f32")
        p_y, p_g = ceps_errors(yp, dxp, variants)
        rec = {"ceps": e_y, "grad": e_g, "plain_ceps": p_y, "plain_grad": p_g, "ambiguous": n_amb}
        if fam in WELL:
            assert e_y <= TAU_CEPS and e_g <= TAU_CEPS_GRAD, rec
        else:
            assert e_y <= TAU_CEPS + RATIO_ILL * p_y and e_g <= TAU_CEPS_GRAD + RATIO_ILL * p_g, rec
    else:
        xd = x.double()
        y64 = ref_mel(xd, p).detach()
        gy = torch.randn(y64.shape, generator=g, dtype=torch.float64)
        gy[:, 1] *= (y64[:, 0] ** 2).clamp(max=1.0)          # the phase's cotangent weighted by |Y|^2 (away from Y = 0)
        a = xd.clone().requires_grad_(True)
        (g64,) = torch.autograd.grad(ref_mel(a, p), a, gy)
        xc, gyc = x.to(cuda), gy.float().to(cuda)
        y, dx = run(fe, xc, gyc, monkeypatch, path)
        assert y.shape == y64.shape
        yp, dxp = run(fe, xc, gyc, monkeypatch, "plain-f32")
        rec = {"mag": rel_max(y[:, 0], y64[:, 0]), "phase": phase_err(y, y64), "grad": grad_err(dx, g64),
               "plain_mag": rel_max(yp[:, 0], y64[:, 0]), "plain_phase": phase_err(yp, y64), "plain_grad": grad_err(dxp, g64)}
        assert rec["mag"] <= TAU_MEL and rec["phase"] <= TAU_MEL_PHASE, rec
        if fam in WELL:
            assert rec["grad"] <= TAU_MEL_GRAD, rec
        else:
            assert rec["grad"] <= TAU_MEL_GRAD + RATIO_ILL * rec["plain_grad"], rec
    # fixed summation order (the overlap-add's border atomics have two operands): the same bits again.  Two documented
    # exceptions for the gradient: with the floor active, the floored share is ONE scalar summed with float atomics over
    # workgroups (its last bit may differ); the tail path's framing backward is torch.stft's own (ATen).
    y2, dx2 = run(fe, xc, gyc, monkeypatch, path)
    assert torch.equal(y, y2)
    if floored or path == "tail":
        assert (dx - dx2).abs().max().item() <= 1e-6 * dx.abs().max().item()
    else:
        assert torch.equal(dx, dx2)
    parity_record[f"stft_f64_{_id(row)}"] = rec


# ---- C-ABI stages ---------------------------------------------------------------------------------------------------------------

def _abi():
    from audio_deepfake_adversarial_attacks_amd import _lib
    return _lib, _lib.load(), torch.cuda.current_stream().cuda_stream


def carve(n, cuda, fill=float("nan"), pad=1_000):
    """A view of n floats inside a larger buffer filled with `fill` (pad floats on either side)."""
    buf = torch.full((n + 2 * pad,), fill, device=cuda)
    return buf, buf[pad:pad + n]


def outside_intact(buf, n, fill=float("nan"), pad=1_000):
    rest = torch.cat([buf[:pad], buf[pad + n:]])
    return bool(torch.isnan(rest).all()) if math.isnan(fill) else bool((rest == fill).all())


STAGE_SHAPES = [(3, 16_160, 160, 400), (2, 258, 160, 400), (2, 5_121, 160, 512), (3, 300, 128, 400), (1, 1_025, 512, 320),
                (2, 20_479, 200, 400)]


def _stage_setup(cuda, B, T, hop, win, variant="lfcc", seed=0):
    fe, _ = build_module(variant, hop, win, cuda)
    p = params_of(fe)
    tables = frontends._cached_tables(fe, fe.filter_mat)
    x = make_input("noise", B, T, seed + T)
    return fe, p, tables, x


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["reg", "radix4"])
@pytest.mark.parametrize("B,T,hop,win", STAGE_SHAPES)
def test_stage_bands_forward(cuda, monkeypatch, parity_record, path, B, T, hop, win):
    """advstep_stft_bands_f32 against the band power of the float64 reference, in the power domain over the frame's one-sided
    energy (Parseval: what float32 FFT error scales with); block_max (NaN before the call) holds the maximum of the kernel's own
    band_db over each workgroup's frames, the unused tail no NaN; nothing outside band_db / block_max is written."""
    _lib, lib, st = _abi()
    set_path(monkeypatch, path)
    fe, p, tables, x = _stage_setup(cuda, B, T, hop, win)
    NF, M = 1 + T // hop, tables.fb_start.numel()
    n_blk = lib.advstep_stft_bands_block_count(B, NF)
    buf, band = carve(B * NF * M, cuda)
    bbuf, bmax = carve(n_blk, cuda)
    xc, w = x.to(cuda), fe._window_nfft()
    _lib.check(lib.advstep_stft_bands_f32(xc.data_ptr(), w.data_ptr(), tables.fb_start.data_ptr(), tables.fb_w.data_ptr(),
                                          tables.span, band.data_ptr(), bmax.data_ptr(), B, T, NF, hop, NFFT, M, st), "bands")
    torch.cuda.synchronize()
    assert outside_intact(buf, band.numel()) and outside_intact(bbuf, n_blk)
    band = band.view(B, NF, M)
    X = ref_spectrum(x.double(), p["window"], hop)
    P64 = (X.real ** 2 + X.imag ** 2) @ p["fb"]
    energy = (X.real ** 2 + X.imag ** 2).sum(-1, keepdim=True)
    P = torch.pow(10.0, band.double().cpu() / 10.0)
    err = ((P - P64).abs() / energy).max().item()
    # frames per workgroup: 32 (register kernel, span <= 4) or 16 (radix-4); the rest of block_max is filled (-inf)
    fpb = 32 if path == "reg" and tables.span <= 4 else 16
    blocks = -(-NF // fpb)
    want = torch.nn.functional.pad(band, (0, 0, 0, blocks * fpb - NF), value=-math.inf).view(B, blocks, fpb * M).amax(-1)
    assert torch.equal(bmax[:B * blocks].view(B, blocks), want)
    assert not torch.isnan(bmax).any()
    parity_record[f"stft_f64_stage_bands_{path}_B{B}_T{T}_hop{hop}_win{win}"] = err
    assert err <= TAU_STAGE_POWER, err


@pytest.mark.gpu
@pytest.mark.parametrize("K", [80, 40, 20])
def test_stage_floor_and_project(cuda, parity_record, K):
    """advstep_lfcc_max_project_f32 (matrix cores at K = 80, the two vector launches otherwise) on the kernel's own band_db
    against float64 of the same input, floored batch: the floor decisions are shared (the floor is max - 80 rounded to float32,
    as the kernel and torch form it); the output written inside a sentinel-filled allocation."""
    from audio_deepfake_adversarial_attacks_amd import frontend_ops
    _lib, lib, st = _abi()
    fe, _ = build_module(f"lfcc-K{K}" if K != 80 else "lfcc", 160, 400, cuda)
    tables = fe._tables()
    x = make_input("floor", 3, 8_000, 5).to(cuda)
    B, T = x.shape
    NF, M = 1 + T // 160, 128
    band = torch.empty(B, NF, M, device=cuda)
    n_blk = lib.advstep_stft_bands_block_count(B, NF)
    bmax = torch.empty(n_blk, device=cuda)
    _lib.check(lib.advstep_stft_bands_f32(x.data_ptr(), fe._window_nfft().data_ptr(), tables.fb_start.data_ptr(),
                                          tables.fb_w.data_ptr(), tables.span, band.data_ptr(), bmax.data_ptr(), B, T, NF, 160,
                                          NFFT, M, st), "bands")
    dct = fe.dct_mat
    frag = frontend_ops.dct_fragments(dct)
    assert (frag is not None) == (K == 80)
    stats = torch.full((4,), 7.0, device=cuda)
    buf, out = carve(B * NF * K, cuda)           # 16-byte aligned: 1000 floats into the allocation
    _lib.check(lib.advstep_lfcc_max_project_f32(band.data_ptr(), dct.data_ptr(), 0 if frag is None else frag.data_ptr(),
                                                bmax.data_ptr(), n_blk, stats.data_ptr(), TOP_DB, out.data_ptr(), B, M, NF, K, st),
               "max_project")
    torch.cuda.synchronize()
    assert outside_intact(buf, B * NF * K)
    db = band.double().cpu()
    floor = torch.tensor(band.max().item() - TOP_DB, dtype=torch.float32).double()
    assert stats[0].item() == band.max().item()
    out64 = torch.maximum(db, floor) @ dct.double().cpu()
    err = rel_max(out.view(B, NF, K), out64)
    assert (db < floor).any()                       # the floor is active
    parity_record[f"stft_f64_stage_project_K{K}"] = err
    assert err <= TAU_STAGE_PROJECT, err


def _fixup_reference(band, dband, stats):
    """dband + the floored gradient sum shared out over the batch maxima (advstep_lfcc_floor_fixup_f32), in float64."""
    db = band.double().cpu()
    at_max = db == stats[0].item()
    share = stats[2].item() / stats[1].item()
    dlog = 10.0 / (math.log(10.0) * torch.pow(10.0, db / 10.0))
    return dband.double().cpu() + at_max * share * dlog


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["plain", "fixup"])
@pytest.mark.parametrize("path", ["reg", "radix4"])
@pytest.mark.parametrize("B,T,hop,win", STAGE_SHAPES)
def test_stage_bands_backward(cuda, monkeypatch, parity_record, entry, path, B, T, hop, win):
    """advstep_stft_bands_backward{,_fixup}_f32 from a given band gradient against the float64 adjoint of the band stage; the
    fix-up entry with a floored-gradient sum shared by two tied maxima (stats = {max, 2, s, 1}).  dx is a view inside a NaN-filled
    allocation: the kernels' own zero fill, the overlap-add stores and atomics must stay inside it."""
    _lib, lib, st = _abi()
    set_path(monkeypatch, path)
    variant = "lfcc-spant" if (T % 2) else "lfcc"
    fe, p, tables, x = _stage_setup(cuda, B, T, hop, win, variant=variant)
    NF, M = 1 + T // hop, tables.fb_start.numel()
    g = torch.Generator().manual_seed(T + B)
    dband = torch.randn(B, NF, M, generator=g) * 1e-2
    xc, w = x.to(cuda), fe._window_nfft()
    dbc = dband.to(cuda)
    buf, dx = carve(B * T, cuda)
    if entry == "plain":
        _lib.check(lib.advstep_stft_bands_backward_f32(xc.data_ptr(), w.data_ptr(), dbc.data_ptr(), tables.fbt_start.data_ptr(),
                                                       tables.fbt_w.data_ptr(), tables.span_t, dx.data_ptr(), B, T, NF, hop,
                                                       NFFT, M, st), "bands_backward")
        want = dband
    else:
        band = torch.empty(B, NF, M, device=cuda)
        bmax = torch.empty(lib.advstep_stft_bands_block_count(B, NF), device=cuda)
        _lib.check(lib.advstep_stft_bands_f32(xc.data_ptr(), w.data_ptr(), tables.fb_start.data_ptr(), tables.fb_w.data_ptr(),
                                              tables.span, band.data_ptr(), bmax.data_ptr(), B, T, NF, hop, NFFT, M, st), "bands")
        stats = torch.tensor([band.max().item(), 2.0, 0.37, 1.0], device=cuda)
        want = _fixup_reference(band, dband, stats)
        _lib.check(lib.advstep_stft_bands_backward_fixup_f32(xc.data_ptr(), w.data_ptr(), dbc.data_ptr(), band.data_ptr(),
                                                             stats.data_ptr(), tables.fbt_start.data_ptr(), tables.fbt_w.data_ptr(),
                                                             tables.span_t, dx.data_ptr(), 0, B, T, NF, hop, NFFT, M, st),
                   "bands_backward_fixup")
    torch.cuda.synchronize()
    assert outside_intact(buf, B * T)
    g64 = ref_adjoint_bands(x.double(), p, want)
    err = grad_err(dx.view(B, T), g64)
    parity_record[f"stft_f64_stage_bands_backward_{entry}_{path}_{variant}_B{B}_T{T}_hop{hop}_win{win}"] = err
    assert err <= TAU_STAGE_ADJ, err


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["from-output-reg", "from-output-radix4", "from-wave"])
@pytest.mark.parametrize("variant", ["mel", "mel-wide", "mel-spant"])
@pytest.mark.parametrize("B,T,hop,win", [(2, 258, 160, 400), (3, 5_121, 160, 400), (2, 301, 128, 512), (1, 2_049, 512, 512)])
def test_stage_mel(cuda, monkeypatch, parity_record, entry, variant, B, T, hop, win):
    """advstep_stft_mel_f32 and its two backward entry points from a given cotangent against float64 (magnitude and adjoint);
    outputs and dx inside NaN-filled allocations."""
    _lib, lib, st = _abi()
    set_path(monkeypatch, "radix4" if entry == "from-output-radix4" else "reg")
    fe, _ = build_module(variant, hop, win, cuda)
    p = params_of(fe)
    tables, window = fe._fused_state(cuda)
    x = make_input("noise", B, T, T) * 0.5
    NF, M = 1 + T // hop, tables.fb_start.numel()
    xc = x.to(cuda)
    obuf, out = carve(B * 2 * M * NF, cuda)
    _lib.check(lib.advstep_stft_mel_f32(xc.data_ptr(), window.data_ptr(), tables.fb_start.data_ptr(), tables.fb_w.data_ptr(),
                                        tables.span, out.data_ptr(), B, T, NF, hop, NFFT, M, st), "mel")
    xd = x.double().requires_grad_(True)
    y64 = ref_mel(xd, p)
    g = torch.Generator().manual_seed(T)
    gy = torch.randn(y64.shape, generator=g, dtype=torch.float64)
    gy[:, 1] *= (y64[:, 0].detach() ** 2).clamp(max=1.0)
    (g64,) = torch.autograd.grad(y64, xd, gy)
    go = gy.float().to(cuda)
    buf, dx = carve(B * T, cuda)
    if entry == "from-wave":
        _lib.check(lib.advstep_stft_mel_backward_f32(xc.data_ptr(), window.data_ptr(), go.data_ptr(), tables.fb_start.data_ptr(),
                                                     tables.fb_w.data_ptr(), tables.span, tables.fbt_start.data_ptr(),
                                                     tables.fbt_w.data_ptr(), tables.span_t, dx.data_ptr(), B, T, NF, hop, NFFT, M,
                                                     st), "mel_backward")
    else:
        _lib.check(lib.advstep_stft_mel_backward_from_output_f32(window.data_ptr(), go.data_ptr(), out.data_ptr(),
                                                                 tables.fbt_start.data_ptr(), tables.fbt_w.data_ptr(), tables.span_t,
                                                                 dx.data_ptr(), B, T, NF, hop, NFFT, M, st), "mel_backward_out")
    torch.cuda.synchronize()
    assert outside_intact(obuf, out.numel()) and outside_intact(buf, B * T)
    y = out.view(B, 2, M, NF)
    e_m, e_g = rel_max(y[:, 0], y64[:, 0].detach()), grad_err(dx.view(B, T), g64)
    parity_record[f"stft_f64_stage_mel_{entry}_{variant}_B{B}_T{T}_hop{hop}"] = {"mag": e_m, "grad": e_g}
    assert e_m <= TAU_MEL and e_g <= TAU_STAGE_MEL_GRAD, (e_m, e_g)


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["reg", "radix4"])
def test_hop128_short_signals_are_bit_reproducible(cuda, monkeypatch, path):
    """hop 128, T 258 .. 600 (1 + T // 128 = 3 .. 5 frames): where the "at most two workgroups reach a sample" argument behind
    the overlap-add's float atomics has the least room; LFCC and mel-spec gradients come out bit-identical run to run."""
    lfcc, _ = build_module("lfcc", 128, 512, cuda)
    mel, _ = build_module("mel", 128, 512, cuda)
    for T in (258, 259, 383, 384, 385, 511, 512, 513, 600):
        x = make_input("noise", 3, T, T).to(cuda)
        for fe in (lfcc, mel):
            with torch.no_grad():
                shape = fe(x).shape
            gy = torch.randn(shape, generator=torch.Generator().manual_seed(T)).to(cuda)
            y1, g1 = run(fe, x, gy, monkeypatch, path)
            y2, g2 = run(fe, x, gy, monkeypatch, path)
            assert torch.equal(y1, y2) and torch.equal(g1, g2), T
            assert torch.isfinite(g1).all()
