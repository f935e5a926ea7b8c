"""The fused log-mel kernel (csrc/melspec.hip) against the float64 oracle of tests/melspec_ref.py, and the layers above
it: MelSpecExtractor, ForcedAlignmentTask.make_input_feature, extract_features.py.

Bar per case: e_hip <= max(4 e_torch_f32, 2e-5) in melspec_ref.error's metric, e_torch_f32 being the same pipeline in
torch float32 on the CPU (what torchaudio runs), computed here.  The factor 4: the GEMM-form DFT accumulates K = 1024
products in f32 where the FFT has ~11 butterfly stages (sqrt K against log K, about 3x); the floor 2e-5 is for inputs
on which torch f32 is essentially exact.  Measured on MI355X (e_hip / e_torch_f32 per case): profiles/melspec/melspec_bench.txt.
"""
import functools
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import melspec_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAME_TILE = 64          # melspec.hip's frame tile at both configs here


def _wave(kind, n, seed=0):
    g = torch.Generator().manual_seed(1000 + seed + n)
    if kind == "gauss":
        return 0.1 * torch.randn(n, generator=g)
    if kind == "zeros":
        return torch.zeros(n)
    if kind == "sign":
        return torch.randint(0, 2, (n,), generator=g).float() * 2.0 - 1.0
    if kind == "sine":
        return 0.5 * torch.sin(2.0 * math.pi * 440.0 * torch.arange(n, dtype=torch.float64) / 44100.0).float()
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def _extractor(name):
    from hubertfa_amd.melspec import MelSpecExtractor
    return MelSpecExtractor(**(ref.DEFAULT if name == "default" else ref.SECOND), device="cuda")


@functools.lru_cache(maxsize=None)
def _reference(kind, n, name):
    """(wave, mel64, e_torch_f32, bound): computed once per case, shared and never modified."""
    x = _wave(kind, n)
    return (x,) + ref.bar(x, ref.DEFAULT if name == "default" else ref.SECOND)


def _check(y, kind, n, name):
    cfg = ref.DEFAULT if name == "default" else ref.SECOND
    x, mel64, e32, bound = _reference(kind, n, name)
    assert y.dtype == torch.float32 and tuple(y.shape) == (1, cfg["n_mels"], n // cfg["hop_length"] + 1)
    assert bool(torch.isfinite(y).all())
    e = ref.error(torch.exp(y[0].double().cpu()), mel64, cfg)
    print(f"[{name} {kind} N={n}] e_hip {e:.2e}  e_torch_f32 {e32:.2e}  bound {bound:.2e}")
    assert e <= bound
    return e, e32


CASES = [("gauss", n) for n in (1, 511, 512, 513, 1023, 1536, 4097)] + [("zeros", 4096), ("sign", 8192)]


@pytest.mark.parametrize("kind,n", CASES)
def test_default_config_single_row(kind, n):
    ex = _extractor("default")
    y = ex(_wave(kind, n).cuda())
    _check(y, kind, n, "default")
    assert not ex.overflowed()
    if kind == "zeros":
        assert bool((y == torch.log(torch.tensor(ref.DEFAULT["clamp"], dtype=torch.float32))).all())


@pytest.mark.parametrize("kind,n", [("gauss", FRAME_TILE * 512), ("sine", 44100)])
def test_tile_edges(kind, n):
    """One frame more than the frame tile (a second workgroup with a single valid frame), and 87 frames of a pure
    tone, whose leakage floor is 1e-7 of its peak."""
    _check(_extractor("default")(_wave(kind, n).cuda()), kind, n, "default")


def test_second_config():
    """sr 16000, n_fft = win_length = 512, hop 128, 80 mels, fmin 0, fmax None: nothing of the default is hard-coded."""
    _check(_extractor("second")(_wave("gauss", 3000).cuda()), "gauss", 3000, "second")


def test_variable_length_batch_masks_and_matches_alone():
    ex = _extractor("default")
    lens = [1, 700, 4097, 44100]
    rows = [_wave("gauss", n, seed=7) for n in lens]
    batch = torch.full((4, max(lens)), 1e3)                 # garbage past each row's end: the kernel must mask it
    for b, r in enumerate(rows):
        batch[b, : lens[b]] = r
    y = ex.batch(batch.cuda(), lens)
    assert tuple(y.shape) == (4, 128, max(lens) // 512 + 1)
    for b, r in enumerate(rows):
        alone = ex(r.cuda())
        f = lens[b] // 512 + 1
        assert tuple(alone.shape) == (1, 128, f)
        assert torch.equal(y[b, :, :f], alone[0]), f"row {b}: differs from the row alone"
        assert bool((y[b, :, f:] == 0).all()), f"row {b}: frames past its own count are not zeros"
    assert not ex.overflowed()


def test_overflow_flag():
    """A tone of amplitude A on bin 64 has the magnitude A sum(w) / 2 = 256 A there: A = 400 (102 400 >= 65 504, the
    f16 limit of the magnitude planes) raises the flag, A = 1 and A = 200 (51 200) do not.  Every load and store is
    in range: this checks the guard's arithmetic."""
    ex = _extractor("default")
    tone = torch.cos(2.0 * math.pi * 64.0 * torch.arange(4096, dtype=torch.float64) / 2048.0).float()
    for amp, want in ((1.0, False), (200.0, False), (400.0, True)):
        ex((amp * tone).cuda())
        assert ex.overflowed() == want, amp
    assert not ex.overflowed()                              # reading the flag cleared it


@pytest.fixture(scope="module")
def task(tmp_path_factory):
    """The synthetic Hubert-base checkpoint of tests/ckpt_files.py (a HF folder + a Lightning .ckpt naming it)."""
    pytest.importorskip("transformers")
    import ckpt_files
    from hubertfa_amd.task import ForcedAlignmentTask
    tmp = str(tmp_path_factory.mktemp("melspec_ckpt"))
    meta = json.load(open(os.path.join(REPO, "tests", "golden", "loaders.json")))
    folder = os.path.join(tmp, "cnhubert")
    ckpt_files.write_hf_folder(folder, "hf")
    path = os.path.join(tmp, "model.ckpt")
    ckpt_files.write_lightning_ckpt(path, meta, hubert_model_path=folder)
    t = ForcedAlignmentTask.load_from_checkpoint(path, device=torch.device("cuda"))
    t.ckpt_path = path
    return t


def test_get_melspec_is_lazy(task):
    task.on_predict_start()
    assert task._melspec is None                # the aligner's start-up creates nothing for the mel
    ex = task.get_melspec
    assert ex is task.get_melspec and ex.cfg["n_mels"] == task.melspec_config["n_mels"]


def test_make_input_feature(task):
    from hubertfa_amd import synth
    sr, hop = 44100, 512
    lens = [int(0.3 * sr), int(1.0 * sr), int(1.7 * sr)]
    batch = np.zeros((3, max(lens)), np.float32)
    for b, n in enumerate(lens):
        batch[b, :n] = synth.synth_audio(n, sr, seed=60 + b)
    waves = torch.from_numpy(batch).cuda()
    rows = task.make_input_feature(waves, lengths=lens)
    feats, n_frames, wl = task.encode_batch(waves, lengths=lens)
    assert len(rows) == 3
    for b, (units, mel, wav_length) in enumerate(rows):
        t = n_frames[b]
        assert t == lens[b] // hop + 1 and tuple(units.shape) == (1, 768, t) and tuple(mel.shape) == (1, 128, t)
        assert torch.equal(units[0], feats[b, :t].t())
        assert torch.equal(mel, task.get_melspec(waves[b, : lens[b]]))
        assert wav_length == lens[b] / sr == wl[b]
    # a 16 kHz row: the mel of the Resampler's own 44.1 kHz wave
    n16 = 16000
    w16 = torch.from_numpy(synth.synth_audio(n16, 16000, seed=70)[None]).cuda()
    (units, mel, wav_length), = task.make_input_feature(w16, wav_sr=16000)
    up = task.upsampler(16000)(w16, split=task.unitsEncoder.split_resample)[0].cpu()
    assert up.numel() == 44100 and wav_length == 1.0 and tuple(units.shape) == (1, 768, 87)
    mel64, e32, bound = ref.bar(up, ref.DEFAULT)
    e = ref.error(torch.exp(mel[0].double().cpu()), mel64, ref.DEFAULT)
    print(f"[make_input_feature 16 kHz] e_hip {e:.2e}  e_torch_f32 {e32:.2e}  bound {bound:.2e}")
    assert tuple(mel.shape) == (1, 128, 87) and e <= bound


def test_extract_features_cli(task, tmp_path):
    from hubertfa_amd import synth
    from hubertfa_amd.wav_io import read_wav, write_wav
    seg = tmp_path / "segments"
    seg.mkdir()
    secs = (0.4, 0.9, 0.65)
    for i, s in enumerate(secs):
        write_wav(seg / f"u{i}.wav", synth.synth_audio(int(s * 44100), 44100, seed=80 + i), 44100)
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, os.path.join(REPO, "extract_features.py"), "-c", task.ckpt_path, "-f",
                        str(seg), "--batch_size", "4"], env=env, cwd=REPO, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    for i, s in enumerate(secs):
        z = np.load(seg / "features" / f"u{i}.npz")
        x, sr = read_wav(str(seg / f"u{i}.wav"))
        (units, mel, wav_length), = task.make_input_feature(torch.from_numpy(np.ascontiguousarray(x[:1])).cuda())
        t = x.shape[1] // 512 + 1
        assert z["input_feature"].shape == (1, 768, t) and z["melspec"].shape == (1, 128, t)
        assert np.array_equal(z["input_feature"], units.cpu().numpy())
        assert np.array_equal(z["melspec"], mel.cpu().numpy())
        assert float(z["wav_length"]) == wav_length == x.shape[1] / sr
