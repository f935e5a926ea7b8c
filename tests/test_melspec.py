"""Host side of the log-mel spectrogram (hubertfa_amd/melspec.py) and hfa_logmel_split's argument envelope."""
import ctypes
import os

import pytest

torch = pytest.importorskip("torch")

import melspec_ref as ref  # noqa: E402


def test_mel_filterbank_default_config():
    from hubertfa_amd.melspec import mel_filterbank, needed_bins
    fb = mel_filterbank(ref.DEFAULT)
    assert fb.dtype == torch.float32 and tuple(fb.shape) == (1025, 128)
    err = float((fb.double() - ref.fbanks_f64(ref.DEFAULT)).abs().max())
    print(f"filterbank vs the f64 closed form: {err:.2e}")
    assert err <= 2e-5
    nz = torch.nonzero(fb.abs().sum(1) > 0).flatten().tolist()
    assert nz == list(range(2, 744))
    assert needed_bins(fb) == (2, 744)
    assert torch.equal(fb, ref.fbanks_f32(ref.DEFAULT))      # the float32 table is part of the reference's behaviour


@pytest.mark.parametrize("n", [1, 511, 512, 513, 1023, 1024, 1536, 4097])
def test_n_frames_matches_stft(n):
    from hubertfa_amd.melspec import n_frames
    for cfg in (ref.DEFAULT, ref.SECOND):
        assert n_frames(n, cfg) == ref.spectrum(torch.zeros(n), cfg).shape[-1] == n // cfg["hop_length"] + 1


@pytest.mark.parametrize("cfg", [ref.DEFAULT, ref.SECOND], ids=["default", "second"])
def test_stft_basis_reconstructs_spectrum(cfg):
    """Pins the window offset in the n_fft frame, the frame origin (f hop - win_length / 2) and the sign of the
    imaginary part: frames x basis equals torch.stft's complex spectrum in float64."""
    from hubertfa_amd.melspec import n_frames, stft_basis
    g = torch.Generator().manual_seed(5)
    x = torch.randn(1536, generator=g, dtype=torch.float64)
    win, hop = cfg["win_length"], cfg["hop_length"]
    basis = stft_basis(cfg)
    assert basis.dtype == torch.float64 and tuple(basis.shape) == (2, cfg["n_fft"] // 2 + 1, win)
    F = n_frames(x.numel(), cfg)
    xz = torch.cat((torch.zeros(win // 2, dtype=torch.float64), x, torch.zeros(F * hop + win, dtype=torch.float64)))
    frames = torch.stack([xz[f * hop: f * hop + win] for f in range(F)])             # x[f hop - win/2 + n]
    got = torch.complex(frames @ basis[0].T, frames @ basis[1].T).T                   # [bins, frames]
    want = ref.spectrum(x, cfg, torch.float64, complex_out=True)
    err = float((got - want).abs().max())
    print(f"basis reconstruction error: {err:.2e}")
    assert got.shape == want.shape and err <= 1e-10


def test_table_layout():
    """build_tables: fragment-order split planes whose hi + lo / 2^11 give the basis and the filterbank back."""
    from hubertfa_amd.melspec import build_tables, mel_filterbank, needed_bins, stft_basis
    cfg = ref.SECOND
    basis, fb = build_tables(cfg)
    fbank = mel_filterbank(cfg)
    lo, hi = needed_bins(fbank)
    assert lo == 1 and hi == cfg["n_fft"] // 2      # fmax = Nyquist: every bin but DC and the Nyquist bin itself,
    #                                                 whose float32 filterbank row is exactly zero
    nb_pad, kpad = fb.shape[2] * 32, basis.shape[2] * 32
    assert nb_pad % 64 == 0 and nb_pad >= hi - lo and kpad % 128 == 0 and kpad >= cfg["win_length"]
    assert tuple(basis.shape) == (2, nb_pad // 8, kpad // 32, 64, 8) and tuple(fb.shape) == (2, 8, nb_pad // 32, 64, 8)

    def unfrag(t):      # [2, rb, ks, 64, 8] -> hi + lo / 2^11 as [rb * 16, ks * 32]
        v = t[0].double() + t[1].double() / 2048.0
        rb, ks = v.shape[:2]
        return v.view(rb, ks, 4, 16, 8).permute(0, 3, 1, 2, 4).reshape(rb * 16, ks * 32)
    b = unfrag(basis).view(nb_pad // 16, 2, 16, kpad)
    want = torch.zeros(2, nb_pad, kpad, dtype=torch.float64)
    want[:, : hi - lo, : cfg["win_length"]] = stft_basis(cfg)[:, lo:hi]
    assert float((b.permute(1, 0, 2, 3).reshape(2, nb_pad, kpad) - want).abs().max()) < 2.0 ** -21
    f = unfrag(fb)
    wantf = torch.zeros(128, nb_pad, dtype=torch.float64)
    wantf[: cfg["n_mels"], : hi - lo] = fbank[lo:hi].T.double()
    assert float((f - wantf).abs().max()) < 2.0 ** -21


def _lib():
    from hubertfa_amd import _lib, ops  # noqa: F401  (ops registers the signature)
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libhfa.so not built (run __graft_entry__.build())")
    return _lib


@pytest.mark.parametrize("case", ["win_length=1000", "hop=100", "n_mels=129", "n_fft<win_length", "misaligned"])
def test_logmel_rejects_outside_envelope(case):
    """Validation precedes any HIP call, so on a host without a GPU the entry answers HFA_EINVAL (never a HIP
    error) for each argument outside the envelope; the pointers are never dereferenced."""
    L = _lib()
    a = dict(B=1, N=4096, x=0x10000, x_bs=4096, lens=0, win=1024, hop=512, n_fft=2048, n_mels=128, nb_pad=768,
             basis=0x20000, fb=0x30000, clamp=1e-5, frames=9, y=0x40000, y_bs=128 * 9, y_ld=9, oflow=0, stream=0)
    a.update({"win_length=1000": dict(win=1000), "hop=100": dict(hop=100), "n_mels=129": dict(n_mels=129),
              "n_fft<win_length": dict(n_fft=512), "misaligned": dict(x=0x10008)}[case])
    P = ctypes.c_void_p
    rc = L.lib().hfa_logmel_split(a["B"], a["N"], P(a["x"]), a["x_bs"], P(a["lens"]), a["win"], a["hop"], a["n_fft"],
                                  a["n_mels"], a["nb_pad"], P(a["basis"]), P(a["fb"]), a["clamp"], a["frames"],
                                  P(a["y"]), a["y_bs"], a["y_ld"], P(a["oflow"]), P(a["stream"]))
    assert rc == L.HFA_EINVAL, L.lib().hfa_last_error()
    assert b"hfa_logmel_split" in L.lib().hfa_last_error()
