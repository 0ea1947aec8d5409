"""Channel: the sampler of the simulated audio channel (no counterpart in the reference).

A draw of the channel is what `hip_ops.channel_apply` needs per (draw, utterance): an impulse response, an integer delay, a gain
and a noise amplitude (include/advstep_channel.h has the arithmetic that consumes them).  The sampler only produces these small
tensors, with torch ops on the images' device — no host read, no copy — and from torch's generators, so `torch.manual_seed`
reproduces them; the per-sample work (the FIR, the noise itself) is the kernels'."""
import math

import torch


class Channel:
    r"""Loudspeaker -> air -> microphone (or a codec, or a phone line) in four numbers per draw and utterance.

    * impulse response h (L = `taps` samples): a unit direct path plus exponentially decaying random taps,
      h[0] = 1, h[i] = decay^i * N(0, 1) for i >= 1, then h / ||h||_2: unit energy, so the gain below is the channel's gain.
    * delay s: an integer uniform in [-max_shift, max_shift] samples (the attacker does not control the alignment of what the
      detector sees; the utterance is silent outside its T samples).
    * gain g = 10^(G / 20), G uniform in [-gain_db, gain_db] dB.
    * noise amplitude a = sqrt(3) * rms(x - c) * 10^(-S / 20), S uniform in [snr_db[0], snr_db[1]] dB (a single number: that SNR;
      None: no noise): uniform noise a * U(-1, 1) has the power a^2 / 3, so the noise sits S dB below the utterance.  rms is taken
      over the utterance as it is given, centred on c.

    Arguments:
        taps (int): length of the impulse response, 1 .. 256. (Default: 64)
        decay (float): ratio of the standard deviations of neighbouring taps, in [0, 1). (Default: 0.5)
        max_shift (int): largest delay either way, in samples. (Default: 160)
        gain_db (float): largest gain either way, in dB. (Default: 6.0)
        snr_db (float, pair or None): the noise floor's SNR in dB, or its range. (Default: (20, 40))

    `draw(n, images, center)` returns (taps (n, B, L) float32, shift (n, B) int32, gain (n, B) float32, noise (n, B) float32).
    The named presets are in `CHANNELS`.

    Examples::
        >>> channel = torchattacks.Channel(taps=32, max_shift=16)
        >>> h, s, g, a = channel.draw(8, images, center)
        >>> y = hip_ops.channel_apply(images, center, h, s, g, a, seed=1)     # (8, B, T)
    """

    def __init__(self, taps=64, decay=0.5, max_shift=160, gain_db=6.0, snr_db=(20, 40)):
        if not 1 <= int(taps) <= 256:
            raise ValueError(f"taps must be between 1 and 256, got {taps}")
        if not 0.0 <= float(decay) < 1.0:
            raise ValueError(f"decay must lie in [0, 1), got {decay}")
        if int(max_shift) < 0 or int(max_shift) >= 2 ** 31:
            raise ValueError(f"max_shift must be a non-negative int32, got {max_shift}")
        if not float(gain_db) >= 0.0:
            raise ValueError(f"gain_db must be >= 0, got {gain_db}")
        if snr_db is not None:
            lo, hi = (snr_db, snr_db) if isinstance(snr_db, (int, float)) else snr_db
            if not float(lo) <= float(hi):                           # (a NaN fails the comparison)
                raise ValueError(f"snr_db must be a number or an ordered pair of dB, got {snr_db}")
            snr_db = (float(lo), float(hi))
        self.taps, self.decay, self.max_shift, self.gain_db, self.snr_db = int(taps), float(decay), int(max_shift), float(gain_db), snr_db

    @classmethod
    def identity(cls):
        """One tap of 1, delay 0, gain 1, no noise: the channel that changes nothing."""
        return cls(taps=1, decay=0.0, max_shift=0, gain_db=0.0, snr_db=None)

    def __repr__(self):
        return (f"Channel(taps={self.taps}, decay={self.decay}, max_shift={self.max_shift}, gain_db={self.gain_db}, "
                f"snr_db={self.snr_db})")

    @torch.no_grad()
    def draw(self, n, images, center, generator=None):
        """`n` draws for each of the B utterances `images` (B, ...) centred on `center` (B values, or a float).  `generator`: a
        torch.Generator of the images' device (None: that device's default generator, which `torch.manual_seed` seeds)."""
        n, B, dev = int(n), images.shape[0], images.device
        kw = dict(device=dev, dtype=torch.float32, generator=generator)
        L = self.taps
        h = torch.randn((n, B, L), **kw) * (self.decay ** torch.arange(L, device=dev, dtype=torch.float32))
        h[..., 0] = 1.0
        h = h / h.square().sum(dim=-1, keepdim=True).sqrt()
        if self.max_shift:
            shift = torch.randint(-self.max_shift, self.max_shift + 1, (n, B), device=dev, generator=generator).to(torch.int32)
        else:
            shift = torch.zeros((n, B), device=dev, dtype=torch.int32)
        gain = torch.pow(10.0, (torch.rand((n, B), **kw) * 2.0 - 1.0) * (self.gain_db / 20.0))
        if self.snr_db is None:
            noise = torch.zeros((n, B), device=dev, dtype=torch.float32)
        else:
            lo, hi = self.snr_db
            snr = lo + (hi - lo) * torch.rand((n, B), **kw)
            c = center.to(device=dev, dtype=torch.float32).reshape(B, 1) if isinstance(center, torch.Tensor) else float(center)
            rms = (images.detach().reshape(B, -1).to(torch.float32) - c).square().mean(dim=1).sqrt()
            noise = math.sqrt(3.0) * rms.reshape(1, B) * torch.pow(10.0, -snr / 20.0)
        return h.contiguous(), shift.contiguous(), gain.contiguous(), noise.contiguous()


# Named presets: choices of scale for "a good room and microphone" and "a telephone handset".  Nobody has measured them against a
# real device; they fix what a reported channel/* figure or an EOTPGD member means, nothing more.
CHANNELS = {
    "identity": Channel.identity(),
    "mild": Channel(taps=32, decay=0.5, max_shift=16, gain_db=3.0, snr_db=(30, 40)),
    "handset": Channel(taps=128, decay=0.8, max_shift=160, gain_db=6.0, snr_db=(15, 30)),
}


def resolve(channel):
    """A `Channel`, the name of a preset in `CHANNELS`, or None."""
    if channel is None or isinstance(channel, Channel):
        return channel
    if isinstance(channel, str):
        if channel not in CHANNELS:
            raise ValueError(f"unknown channel '{channel}': the presets are {sorted(CHANNELS)}")
        return CHANNELS[channel]
    raise TypeError(f"channel must be a Channel, the name of a preset or None, got {type(channel).__name__}")
