"""TEST INFRASTRUCTURE: the log-mel oracle of tests/test_melspec.py and tests/test_melspec_gpu.py.

torchaudio (tools/get_melspec.py's back end) is not installed, so the reference is restated on torch CPU, written
independently of hubertfa_amd/melspec.py: the float32 periodic Hann window and the float32 htk filterbank (both part of
the reference's behaviour), ``torch.stft(center=False)`` on the wave zero-padded by n_fft // 2 and (n_fft + 1) // 2,
magnitude, ``mag @ fb``.  ``dtype`` float64 is the oracle; float32 is the arithmetic torchaudio itself runs, whose
distance from the oracle scales the tests' bar.
"""
import math

import torch

DEFAULT = dict(n_mels=128, sample_rate=44100, win_length=1024, hop_length=512, n_fft=2048, fmin=40, fmax=16000,
               clamp=0.00001)
SECOND = dict(n_mels=80, sample_rate=16000, win_length=512, hop_length=128, n_fft=512, fmin=0, fmax=None,
              clamp=0.00001)


def fbanks_f32(cfg):
    """torchaudio.functional.melscale_fbanks(norm=None, mel_scale="htk") in float32."""
    sr, n_freqs, n_mels = cfg["sample_rate"], cfg["n_fft"] // 2 + 1, cfg["n_mels"]
    f_max = float(sr // 2) if cfg["fmax"] is None else float(cfg["fmax"])
    m_min = 2595.0 * math.log10(1.0 + float(cfg["fmin"]) / 700.0)
    m_max = 2595.0 * math.log10(1.0 + f_max / 700.0)
    freqs = torch.linspace(0, sr // 2, n_freqs)
    f_pts = 700.0 * (10 ** (torch.linspace(m_min, m_max, n_mels + 2) / 2595.0) - 1.0)
    diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts[None, :] - freqs[:, None]
    return torch.clamp(torch.minimum(-slopes[:, :-2] / diff[:-1], slopes[:, 2:] / diff[1:]), min=0.0)


def fbanks_f64(cfg):
    """The same triangles from closed forms in float64 (an independent formula: per-filter edges, no slopes table)."""
    sr, n_fft, n_mels = cfg["sample_rate"], cfg["n_fft"], cfg["n_mels"]
    f_max = float(sr // 2) if cfg["fmax"] is None else float(cfg["fmax"])
    mel = lambda f: 2595.0 * math.log10(1.0 + f / 700.0)  # noqa: E731
    m_lo, m_hi = mel(float(cfg["fmin"])), mel(f_max)
    edges = [700.0 * (10.0 ** ((m_lo + (m_hi - m_lo) * i / (n_mels + 1)) / 2595.0) - 1.0) for i in range(n_mels + 2)]
    fb = torch.zeros(n_fft // 2 + 1, n_mels, dtype=torch.float64)
    for k in range(n_fft // 2 + 1):
        f = (sr // 2) * k / (n_fft // 2)
        for m in range(n_mels):
            lo, c, hi = edges[m], edges[m + 1], edges[m + 2]
            if lo < f < hi:
                fb[k, m] = (f - lo) / (c - lo) if f <= c else (hi - f) / (hi - c)
    return fb


def spectrum(x, cfg, dtype=torch.float64, complex_out=False):
    """[bins, frames] STFT of the padded wave (magnitude unless ``complex_out``)."""
    n_fft, win, hop = cfg["n_fft"], cfg["win_length"], cfg["hop_length"]
    xp = torch.nn.functional.pad(x.to(dtype), (n_fft // 2, (n_fft + 1) // 2))
    w = torch.hann_window(win, dtype=torch.float32).to(dtype)
    s = torch.stft(xp, n_fft, hop_length=hop, win_length=win, window=w, center=False, normalized=False,
                   onesided=True, return_complex=True)
    return s if complex_out else s.abs()


def mel_linear(x, cfg, dtype=torch.float64):
    """[n_mels, frames] clamp(mag @ fb, clamp) before the log, in ``dtype`` (x: CPU float32 [N])."""
    mag = spectrum(x, cfg, dtype)
    mel = torch.matmul(mag.transpose(-1, -2), fbanks_f32(cfg).to(dtype)).transpose(-1, -2)
    return torch.clamp(mel, min=cfg["clamp"])


def error(mel, mel64, cfg):
    """max |mel - mel64| / (mel64 + 1e-3 P_f) over the spectrogram, P_f the frame's largest oracle value (floored at
    clamp): relative where the energy is, and against a thousandth of the frame's peak in the leakage floor, where a
    log-domain comparison is meaningless (a pure tone leaks to ~1e-7 of its peak)."""
    mel, mel64 = mel.double(), mel64.double()
    peak = torch.clamp(mel64.max(dim=0, keepdim=True).values, min=cfg["clamp"])
    return float(((mel - mel64).abs() / (mel64 + 1e-3 * peak)).max())


def bar(x, cfg):
    """-> (mel64, e_torch_f32, the bound max(4 e_torch_f32, 2e-5)) for one wave."""
    mel64 = mel_linear(x, cfg, torch.float64)
    e32 = error(mel_linear(x, cfg, torch.float32), mel64, cfg)
    return mel64, e32, max(4.0 * e32, 2e-5)
