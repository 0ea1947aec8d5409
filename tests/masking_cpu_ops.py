"""Float64 restatement (numpy, CPU) of the masking ops of include/advstep_masking.h and of torchattacks/masking.py's threshold:
the test-side twin the kernels are held against.  Frames are cut from an explicitly reflect-padded signal and transformed with
numpy's rfft; the gradient is the analytic adjoint (checked against float64 autograd in tests/test_masking_host.py).

psy_step is restated in the dtype of its inputs with the kernel's operation order, so that in float32, given the device's two
row means, it agrees with the kernel byte for byte; `device_mean_abs` re-plays the kernel's fixed summation order."""
import numpy as np

N_FFT, BINS, PAD = 512, 257, 256


def hann(dtype=np.float64):
    """The periodic Hann(512) window."""
    n = np.arange(N_FFT, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * n / N_FFT)).astype(dtype)


def reflect_index(T):
    """Sample index behind every padded position p = q + 256, q = -256 .. T + 255."""
    q = np.arange(-PAD, T + PAD)
    q = np.where(q < 0, -q, q)
    return np.where(q >= T, 2 * (T - 1) - q, q)


def frame_index(T, hop):
    """(NF, 512) sample indices of the frames of a T-sample row: centre framing, reflect padding, NF = 1 + T // hop."""
    NF = 1 + T // hop
    pos = np.arange(NF)[:, None] * hop + np.arange(N_FFT)[None, :]
    return reflect_index(T)[pos]


def stft(d, window, hop):
    """(B, T) float64 -> complex (B, NF, 257)."""
    d = np.asarray(d, dtype=np.float64)
    return np.fft.rfft(d[:, frame_index(d.shape[1], hop)] * np.asarray(window, dtype=np.float64), axis=-1)


def stft_power(a, b, window, hop):
    d = np.asarray(a, dtype=np.float64) - (0.0 if b is None else np.asarray(b, dtype=np.float64))
    X = stft(d, window, hop)
    return X.real ** 2 + X.imag ** 2


def stft_adjoint(G, window, hop, T):
    """The adjoint of d -> X = stft(d) applied to the cotangent G = dL/dRe X + i dL/dIm X (B, NF, 257): dL/dd (B, T).
    dL/dy[n] = Re sum_k G[k] e^(+2 pi i k n / 512) over the 257 one-sided bins, each once; then the window and the overlap-add
    through the reflect index."""
    G = np.asarray(G, dtype=np.complex128)
    k = np.arange(BINS)[:, None] * np.arange(N_FFT)[None, :]
    C = np.exp(2j * np.pi * (k % N_FFT) / N_FFT)                              # (257, 512)
    dy = (G @ C).real * np.asarray(window, dtype=np.float64)                  # (B, NF, 512)
    out = np.zeros((G.shape[0], T), dtype=np.float64)
    idx = frame_index(T, hop)
    for b in range(G.shape[0]):
        np.add.at(out[b], idx.ravel(), dy[b].ravel())
    return out


def hinge(adv, x, window, theta, s, hop, decide=None):
    """The masking hinge: returns dict(loss (B), count (B), worst (B), grad (B, T), P, e).  `decide`: a bool (B, NF, 257) that
    replaces e > 0 (the device's decision on the cells too close to call)."""
    adv, x = np.asarray(adv, dtype=np.float64), np.asarray(x, dtype=np.float64)
    theta, s = np.asarray(theta, dtype=np.float64), np.asarray(s, dtype=np.float64)
    X = stft(adv - x, window, hop)
    P = X.real ** 2 + X.imag ** 2
    e = P - theta
    act = (e > 0) if decide is None else decide
    with np.errstate(divide="ignore", invalid="ignore"):
        worst = np.maximum(0.0, (P / theta).max(axis=(1, 2)))
    grad = stft_adjoint(2.0 * s[:, None, None] * np.where(act, X, 0.0), window, hop, adv.shape[1])
    return {"loss": s * np.where(act, e, 0.0).sum(axis=(1, 2)), "count": act.sum(axis=(1, 2)).astype(np.float64),
            "worst": worst, "grad": grad, "P": P, "e": e}


def sign(u):
    return (0 < u).astype(u.dtype) - (u < 0).astype(u.dtype)


def psy_step(cur, g_ce, g_mask, x, lam, step, eps, means=None):
    """The mixed step in the inputs' dtype, the kernel's operation order.  means = (m1 (B), m2 (B)): the row means of |g_ce| and
    |g_mask| to use (the device's); None: this function's own."""
    dt = cur.dtype
    lam, step, eps = dt.type(lam), dt.type(step), dt.type(eps)
    if lam == 0:
        u = g_ce
    else:
        if means is None:
            means = (np.abs(g_ce).sum(axis=1) / dt.type(cur.shape[1]), np.abs(g_mask).sum(axis=1) / dt.type(cur.shape[1]))
        m1, m2 = (np.asarray(m, dtype=dt)[:, None] for m in means)
        with np.errstate(divide="ignore", invalid="ignore"):
            u = np.where(m1 != 0, g_ce / m1, dt.type(0))
            u = np.where(m2 != 0, u - lam * (g_mask / m2), u)
    a = cur + step * sign(u)
    d = np.minimum(np.maximum(a - x, -eps), eps)
    return np.minimum(np.maximum(x + d, dt.type(0)), dt.type(1))


def device_mean_abs(g, vec):
    """mean |g| per row in float32 in the order of csrc/row_workgroup.h: thread t of 1024 takes samples t, t + 1024, ... (vec:
    quads, lanes x, y, z, w in order), a wave's 64 partials meet in an xor butterfly (offsets 32 .. 1), the 16 waves add in order."""
    g = np.abs(np.asarray(g, dtype=np.float32))
    B, T = g.shape
    if B > 512:                                                              # in blocks of rows: the padded copy is 16 KB per row
        return np.concatenate([device_mean_abs(g[i:i + 512], vec) for i in range(0, B, 512)])
    width = 4096 if vec else 1024
    padded = np.zeros((B, -(-T // width) * width), dtype=np.float32)
    padded[:, :T] = g
    acc = np.zeros((B, 1024), dtype=np.float32)
    if vec:
        for chunk in padded.reshape(B, -1, 1024, 4).transpose(1, 0, 2, 3):
            for j in range(4):
                acc = acc + chunk[:, :, j]
    else:
        for chunk in padded.reshape(B, -1, 1024).transpose(1, 0, 2):
            acc = acc + chunk
    v = acc.reshape(B, 16, 64)
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[:, :, lane ^ off]
    total = v[:, 0, 0]
    for w in range(1, 16):
        total = total + v[:, w, 0]
    return total / np.float32(T)


# ---- the threshold (torchattacks/masking.py) ------------------------------------------------------------------------------

def bark(f):
    return 13.0 * np.arctan(0.00076 * f) + 3.5 * np.arctan((f / 7500.0) ** 2)


def ath_db(f):
    k = np.maximum(f, 20.0) / 1000.0
    return 3.64 * k ** -0.8 - 6.5 * np.exp(-0.6 * (k - 3.3) ** 2) + 1e-3 * k ** 4


def tables(sr=16000):
    f = np.arange(BINS, dtype=np.float64) * sr / N_FFT
    z = bark(f)
    ath_rel = 10.0 ** ((ath_db(f) - 96.0) / 10.0)
    n = (np.abs(z[None, :] - z[:, None]) < 0.5).sum(axis=1).astype(np.float64)
    d = z[:, None] - z[None, :] + 0.474
    sf = 15.81 + 7.5 * d - 17.5 * np.sqrt(1.0 + d * d)
    M = 10.0 ** ((sf - 14.5 - z[None, :]) / 10.0) / n[:, None]
    return z, ath_rel, M, n


def threshold(x, hop=128, sr=16000):
    """(theta (B, NF, 257), s (B)) in float64."""
    _, ath_rel, M, _ = tables(sr)
    P = stft_power(x, None, hann(), hop)
    P[:, :, :2] = 0.0
    ref = np.maximum(P.max(axis=(1, 2)), 1e-30)
    theta = ref[:, None, None] * np.maximum(ath_rel, (P / ref[:, None, None]) @ M.T)
    return theta, 1.0 / (ref * P.shape[1] * BINS)
