"""Log-mel spectrogram on the GPU (tools/get_melspec.py): host-side tables + one fused HIP kernel.

Replaces ``MelSpecExtractor`` (torchaudio ``Spectrogram(power=1, center=False, window_fn=hann_window)`` on the wave
zero-padded by n_fft // 2 and (n_fft + 1) // 2, ``MelScale(mel_scale="htk", norm=None)``, ``log(clamp(., clamp))``).
torchaudio is absent from this environment, so its semantics are restated here: ``mel_filterbank`` follows
``torchaudio.functional.melscale_fbanks`` operation for operation in float32 on torch CPU, ``stft_basis`` is the
windowed DFT that ``torch.stft(center=False)`` computes (the window centred in the n_fft frame), and ``n_frames`` its
frame count.  The device work is ``ops.logmel_split`` (csrc/melspec.hip).
"""
from __future__ import annotations

import math

import torch

from . import ops

CONFIG_KEYS = ("n_mels", "sample_rate", "win_length", "hop_length", "n_fft", "fmin", "fmax", "clamp")


def _hz_to_mel(f: float) -> float:
    return 2595.0 * math.log10(1.0 + f / 700.0)


def mel_filterbank(cfg) -> torch.Tensor:
    """[n_fft // 2 + 1, n_mels] float32 triangular filters, as ``melscale_fbanks(n_freqs, fmin, fmax, n_mels,
    sample_rate, norm=None, mel_scale="htk")`` builds them (float32 torch CPU ops; ``fmax`` None: sample_rate // 2)."""
    n_freqs = cfg["n_fft"] // 2 + 1
    fmax = cfg.get("fmax")
    fmax = float(cfg["sample_rate"] // 2) if fmax is None else float(fmax)
    all_freqs = torch.linspace(0, cfg["sample_rate"] // 2, n_freqs)
    m_pts = torch.linspace(_hz_to_mel(float(cfg["fmin"])), _hz_to_mel(fmax), cfg["n_mels"] + 2)
    f_pts = 700.0 * (10 ** (m_pts / 2595.0) - 1.0)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts.unsqueeze(0) - all_freqs.unsqueeze(1)
    down = (-1.0 * slopes[:, :-2]) / f_diff[:-1]
    up = slopes[:, 2:] / f_diff[1:]
    return torch.max(torch.zeros(1), torch.min(down, up))


def stft_basis(cfg) -> torch.Tensor:
    """[2, n_fft // 2 + 1, win_length] float64: w[n] cos(t) and -w[n] sin(t), t = 2 pi (n + off) k / n_fft with off =
    (n_fft - win_length) // 2 and w the float32 periodic Hann window: frame f's spectrum (torch.stft, center=False,
    on the padded wave) is sum_n x[f hop - win_length / 2 + n] (basis[0, k, n] + i basis[1, k, n]), samples outside
    the wave being zeros (the window is zero over the rest of the n_fft frame)."""
    n_fft, win = cfg["n_fft"], cfg["win_length"]
    off = (n_fft - win) // 2
    w = torch.hann_window(win, dtype=torch.float32).double()
    k = torch.arange(n_fft // 2 + 1, dtype=torch.int64)[:, None]
    n = torch.arange(win, dtype=torch.int64)[None, :] + off
    t = ((k * n) % n_fft).double() * (2.0 * math.pi / n_fft)     # the angle reduced exactly before the f64 product
    return torch.stack((w * torch.cos(t), -w * torch.sin(t)))


def n_frames(n: int, cfg) -> int:
    """Frames of an n-sample wave: torch.stft(center=False) over n + n_fft // 2 + (n_fft + 1) // 2 samples."""
    n_fft = cfg["n_fft"]
    return (int(n) + n_fft // 2 + (n_fft + 1) // 2 - n_fft) // cfg["hop_length"] + 1


def needed_bins(fb: torch.Tensor) -> tuple[int, int]:
    """[lo, hi): the span of bins whose filterbank row is not all zero (default config: 2..743 of 1025); the others
    contribute nothing to any mel, so the kernel never computes them."""
    nz = torch.nonzero(fb.abs().sum(1) > 0).flatten()
    if nz.numel() == 0:
        return 0, 1
    return int(nz[0]), int(nz[-1]) + 1


def _fragments(t: torch.Tensor) -> torch.Tensor:
    """f32 [rows, K] (rows % 16 == 0, K % 32 == 0) -> split-f16 planes in MFMA fragment order [2, rows / 16, K / 32,
    64, 8]: element (lane, j) of a block is [row lane & 15][k 8 (lane >> 4) + j]."""
    rows, K = t.shape
    hi = t.to(torch.float16)
    lo = ((t - hi.float()) * 2048.0).to(torch.float16)
    p = torch.stack((hi, lo)).view(2, rows // 16, 16, K // 32, 4, 8)
    return p.permute(0, 1, 3, 4, 2, 5).reshape(2, rows // 16, K // 32, 64, 8).contiguous()


def build_tables(cfg):
    """(basis, fb) host tables of hfa_logmel_split for ``cfg`` (include/hfa.h gives the layout)."""
    fbank = mel_filterbank(cfg)
    lo, hi = needed_bins(fbank)
    nb_pad = (hi - lo + 63) // 64 * 64
    win = cfg["win_length"]
    kpad = (win + 127) // 128 * 128
    b = stft_basis(cfg)[:, lo:hi].to(torch.float32)                       # [2, nb, win]
    cols = torch.zeros(nb_pad // 16, 2, 16, kpad, dtype=torch.float32)
    full = torch.zeros(2, nb_pad, win, dtype=torch.float32)
    full[:, : hi - lo] = b
    cols[:, :, :, :win] = full.view(2, nb_pad // 16, 16, win).permute(1, 0, 2, 3)
    ft = torch.zeros(128, nb_pad, dtype=torch.float32)
    ft[: cfg["n_mels"], : hi - lo] = fbank[lo:hi].t()
    return _fragments(cols.view(-1, kpad)), _fragments(ft)


class MelSpecExtractor:
    """tools/get_melspec.py:57-87 with the reference's constructor signature; ``__call__(waveform [N])`` returns
    [1, n_mels, frames] (:86-87), ``batch`` the same for B rows at once.  ``flag`` (int32 device tensor) is raised
    when a magnitude left f16 range (>= 65504: a wave thousands of times full scale); ``overflowed()`` reads and
    clears it."""

    def __init__(self, n_mels, sample_rate, win_length, hop_length, n_fft, fmin, fmax, clamp, device=None):
        self.cfg = dict(n_mels=n_mels, sample_rate=sample_rate, win_length=win_length, hop_length=hop_length,
                        n_fft=n_fft, fmin=fmin, fmax=fmax, clamp=clamp)
        self.device = torch.device(device or "cuda")
        if n_fft % 2 or n_fft < win_length or win_length % 32 or win_length > 2048 or hop_length % 8 or n_mels > 128:
            raise ValueError("MelSpecExtractor: outside the kernel's envelope (win_length a multiple of 32 and <= "
                             "2048, n_fft even and >= win_length, hop_length a multiple of 8, n_mels <= 128)")
        basis, fb = build_tables(self.cfg)
        self.basis, self.fb = basis.to(self.device), fb.to(self.device)
        self.flag = torch.zeros(1, dtype=torch.int32, device=self.device)

    def batch(self, waves: torch.Tensor, lengths=None) -> torch.Tensor:
        """waves [B, N] (rows zero-padded or not: ``lengths``, host ints or an int32 device tensor, gives each row's
        own samples) -> [B, n_mels, N // hop + 1]; row b's frames past lengths[b] // hop + 1 are zeros."""
        x = waves.to(self.device, torch.float32)
        B, N = x.shape
        if x.stride(-1) != 1 or x.data_ptr() % 16 or (B > 1 and x.stride(0) % 4):
            buf = torch.empty((B, (N + 3) // 4 * 4), dtype=torch.float32, device=self.device)
            buf[:, :N] = x
            x = buf[:, :N]
        lens = None
        if lengths is not None:
            lens = lengths if isinstance(lengths, torch.Tensor) else torch.tensor(
                [int(n) for n in lengths], dtype=torch.int32).to(self.device)
        c = self.cfg
        return ops.logmel_split(x, self.basis, self.fb, win_length=c["win_length"], hop_length=c["hop_length"],
                                n_fft=c["n_fft"], n_mels=c["n_mels"], clamp=c["clamp"], lens=lens, flag=self.flag)

    def __call__(self, waveform: torch.Tensor, key_shift=0) -> torch.Tensor:
        return self.batch(waveform.reshape(1, -1))

    def overflowed(self) -> bool:
        bad = bool(int(self.flag.item()))
        if bad:
            self.flag.zero_()
        return bad
