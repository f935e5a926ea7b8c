"""The infer.py drop-in CLI on a folder of synthetic wav/.lab pairs -> TextGrids + confidence.csv."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_infer_cli_end_to_end(tmp_path):
    from click.testing import CliRunner
    import infer
    from hubertfa_amd import synth
    from hubertfa_amd.export_tool import read_textgrid
    from hubertfa_amd.task import synth_checkpoint
    from hubertfa_amd.wav_io import write_wav
    d = synth.synth_dictionary(n_words=40)
    dpath = tmp_path / "dict.txt"
    dpath.write_text("".join(f"{w}\t{' '.join(p)}\n" for w, p in d.items()))
    seg = tmp_path / "segments"
    seg.mkdir()
    SECS = (2.0, 2.0, 3.5, 2.7, 1.3)
    for i, secs in enumerate(SECS):
        write_wav(seg / f"u{i}.wav", synth.synth_audio(int(secs * 16000), seed=i), 16000)
        (seg / f"u{i}.lab").write_text(synth.synth_lab(5, d, seed=i))
    ck = tmp_path / "m.ckpt"
    synth_checkpoint(str(ck))
    mpath = tmp_path / "metrics.jsonl"
    r = CliRunner().invoke(infer.main, ["-c", str(ck), "-f", str(seg), "-d", str(dpath), "-sc",
                                        "--hubert_path", "synth:0", "--metrics", str(mpath)])
    assert r.exit_code == 0, r.output + repr(r.exception)
    import json
    m = json.loads(mpath.read_text().strip().splitlines()[-1])
    assert m["files"] == m["aligned"] == len(SECS) and m["errors"] == 0 and m["world"] == 1
    assert abs(m["audio_s"] - sum(SECS)) < 1e-3 and m["rtf_inv_align"] > 0 and m["dp_frames"] > 0
    for i, secs in enumerate(SECS):
        tg = read_textgrid(seg / "TextGrid" / f"u{i}.TextGrid")
        words = [t for t in tg["words"] if t[2] != "SP"]
        assert [w[2] for w in words] == synth.synth_lab(5, d, seed=i).split(" ")
        assert abs(tg["phones"][-1][1] - secs) < 1e-3
    assert (seg / "confidence" / "confidence.csv").exists()
    # variable-length batches (default) write exactly what one-utterance batches (the reference's B=1) write
    batched = {i: (seg / "TextGrid" / f"u{i}.TextGrid").read_text() for i in range(len(SECS))}
    out1 = tmp_path / "one"
    r = CliRunner().invoke(infer.main, ["-c", str(ck), "-f", str(seg), "-d", str(dpath), "--hubert_path", "synth:0",
                                        "--batch_size", "1", "--out_path", str(out1)])
    assert r.exit_code == 0, r.output + repr(r.exception)
    for i in range(len(SECS)):
        one = next(out1.rglob(f"u{i}.TextGrid")).read_text()
        assert one == batched[i], f"u{i}: batched TextGrid differs from the B=1 run"


def test_pipelined_predict_repeatable(tmp_path):
    """The CLI's two-stream pipeline (encoder of batch i+1 beside head + DP of batch i), one-utterance batches,
    repeated: every run's intervals and confidences are identical (an intermittent intra-kernel LDS race in the
    pipelined split attention showed up only here, under the concurrent side stream)."""
    import infer
    import hubertfa_amd.g2p as g2p_mod
    import torch
    from hubertfa_amd import synth
    from hubertfa_amd.task import ForcedAlignmentTask, synth_checkpoint
    from hubertfa_amd.wav_io import write_wav
    d = synth.synth_dictionary(n_words=40)
    dpath = tmp_path / "dict.txt"
    dpath.write_text("".join(f"{w}\t{' '.join(p)}\n" for w, p in d.items()))
    seg = tmp_path / "segments"
    seg.mkdir()
    for i, secs in enumerate((2.0, 2.0, 3.5, 2.7, 1.3)):
        write_wav(seg / f"u{i}.wav", synth.synth_audio(int(secs * 16000), seed=i), 16000)
        (seg / f"u{i}.lab").write_text(synth.synth_lab(5, d, seed=i))
    ck = tmp_path / "m.ckpt"
    synth_checkpoint(str(ck))
    g = g2p_mod.DictionaryG2P(dictionary=str(dpath))
    g.set_in_format("lab")
    rows = list(g.get_dataset(sorted(seg.rglob("*.wav"))))
    torch.set_grad_enabled(False)
    task = ForcedAlignmentTask.load_from_checkpoint(str(ck), device=torch.device("cuda"), hubert_model_path="synth:0")

    def key(records):
        return {k: (np.asarray(r["ph_time_int"]).tobytes(), np.asarray(r["frame_confidence"]).tobytes(),
                    np.asarray(r["edge_diff"]).tobytes()) for k, r in records.items()}
    keys = list(range(len(rows)))
    ref = key(infer._predict(task, rows, keys, 32, []))
    assert len(ref) == len(rows)
    for rep in range(8):
        got = key(infer._predict(task, rows, keys, 1, []))
        assert got == ref, f"rep {rep}: {[n for n in got if got[n] != ref[n]]} differ"


def test_predict_long_files_held_dp(tmp_path):
    """The CLI's loop with long files whose DP task.submit holds for the next encoder (threshold lowered so 50-100 s
    files qualify), short ones between them (not held: the loop's depth switches 1 <-> 2), one file per batch: the
    records equal those of the same run with nothing held."""
    import infer
    import hubertfa_amd.g2p as g2p_mod
    import torch
    from hubertfa_amd import synth
    from hubertfa_amd.task import ForcedAlignmentTask, synth_checkpoint
    from hubertfa_amd.wav_io import write_wav
    d = synth.synth_dictionary(n_words=40)
    dpath = tmp_path / "dict.txt"
    dpath.write_text("".join(f"{w}\t{' '.join(p)}\n" for w, p in d.items()))
    seg = tmp_path / "segments"
    seg.mkdir()
    for i, secs in enumerate((100.0, 2.0, 60.0, 50.0, 3.0)):
        write_wav(seg / f"u{i}.wav", synth.synth_audio(int(secs * 16000), seed=i), 16000)
        (seg / f"u{i}.lab").write_text(synth.synth_lab(max(5, int(secs)), d, seed=i))
    ck = tmp_path / "m.ckpt"
    synth_checkpoint(str(ck))
    g = g2p_mod.DictionaryG2P(dictionary=str(dpath))
    g.set_in_format("lab")
    rows = list(g.get_dataset(sorted(seg.rglob("*.wav"))))
    torch.set_grad_enabled(False)
    task = ForcedAlignmentTask.load_from_checkpoint(str(ck), device=torch.device("cuda"), hubert_model_path="synth:0")

    def key(records):
        return {k: (np.asarray(r["ph_time_int"]).tobytes(), np.asarray(r["frame_confidence"]).tobytes(),
                    np.asarray(r["edge_diff"]).tobytes()) for k, r in records.items()}
    keys = list(range(len(rows)))
    task.defer_dp_frames = None
    ref = key(infer._predict(task, rows, keys, 1, []))
    task.defer_dp_frames = 4096
    got = key(infer._predict(task, rows, keys, 1, []))
    assert len(ref) == len(rows) and got == ref, [n for n in got if got[n] != ref.get(n)]


def _mixed_folder(tmp_path):
    """Mixed lengths and two sample rates (16 kHz / 22.05 kHz) -> (segments dir, dictionary, checkpoint)."""
    from hubertfa_amd import synth
    from hubertfa_amd.task import synth_checkpoint
    from hubertfa_amd.wav_io import write_wav
    d = synth.synth_dictionary(n_words=40)
    dpath = tmp_path / "dict.txt"
    dpath.write_text("".join(f"{w}\t{' '.join(p)}\n" for w, p in d.items()))
    seg = tmp_path / "segments"
    seg.mkdir()
    files = ((2.0, 16000), (3.1, 16000), (1.2, 22050), (4.0, 16000), (2.6, 22050), (0.9, 16000), (5.3, 16000))
    for i, (secs, sr) in enumerate(files):
        write_wav(seg / f"m{i}.wav", synth.synth_audio(int(secs * sr), sr, seed=40 + i), sr)
        (seg / f"m{i}.lab").write_text(synth.synth_lab(4 + i % 3, d, seed=40 + i))
    ck = tmp_path / "m.ckpt"
    synth_checkpoint(str(ck))
    return seg, dpath, ck, len(files)


def _torchrun(args, env_extra=None, nproc=2, timeout=420, script="infer.py"):
    import socket
    import subprocess
    import sys
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, **(env_extra or {}))
    cmd = [sys.executable, "-u", "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}",
           "--master-addr", "127.0.0.1", f"--master-port={port}", os.path.join(repo, script), *args]
    return subprocess.run(cmd, env=env, cwd=repo, capture_output=True, text=True, timeout=timeout)


def test_infer_two_ranks_match_one_rank(tmp_path):
    """torchrun with 2 ranks (both on GPU 0, gloo data backend): LPT shards of mixed-length, mixed-rate files, the
    boundary-array gather to rank 0, and rank 0's TextGrids byte-identical to the one-rank run; then the same
    with rank 1's shard failing (fault injection): rank 0 re-runs it and the output is still identical."""
    from click.testing import CliRunner
    import infer
    seg, dpath, ck, n = _mixed_folder(tmp_path)
    base = ["-c", str(ck), "-f", str(seg), "-d", str(dpath), "--hubert_path", "synth:0", "--batch_size", "3", "-sc"]
    out1 = tmp_path / "one"
    r = CliRunner().invoke(infer.main, base + ["--out_path", str(out1)])   # one GPU: the streaming export
    assert r.exit_code == 0, r.output + repr(r.exception)
    one = {p.name: p.read_bytes() for p in out1.rglob("*.TextGrid")}
    assert len(one) == n
    conf = sorted(seg.rglob("confidence.csv"))
    conf1 = [c.read_bytes() for c in conf]
    assert conf1
    for tag, extra in (("two", None), ("requeue", {"HFA_FAULT_INJECT_RANK": "1"})):
        out = tmp_path / tag
        p = _torchrun(base + ["--out_path", str(out), "--dist_backend", "gloo", "--device", "0"], extra)
        assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
        got = {q.name: q.read_bytes() for q in out.rglob("*.TextGrid")}
        assert got == one, f"{tag}: {[k for k in one if got.get(k) != one[k]]} differ from the one-rank run"
        assert [c.read_bytes() for c in conf] == conf1, f"{tag}: confidence.csv differs from the one-rank run"
        if extra:
            assert "re-running" in p.stdout and "shard failed" in p.stdout


def test_bench_contract_two_ranks():
    """The N > 1 bench launch, rehearsed with 2 ranks on GPU 0 over gloo and started the way a plain
    `python bench.py --gpus 2` is (no outer torchrun: bench.py starts torch.distributed.run itself as a child,
    verdict r04 item 1): one process per rank, barrier + synchronize around the timed steps, max over ranks; rank 0
    alone prints one JSON line whose value is the whole-job rate (global batch = world x per-rank batch), whose
    metric is BASELINE.json's, and whose `ranks` block shows the process group's two distinct ranks."""
    import json
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, "-u", os.path.join(repo, "bench.py"), "--gpus", "2", "--steps", "2",
                        "--warmup", "1", "--batch", "4", "--seconds", "2", "--no-cpu-baseline", "--dist-backend", "gloo",
                        "--device", "0"], env=env, cwd=repo, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    base = json.load(open(os.path.join(repo, "BASELINE.json")))
    assert d["metric"] == base["metric"]
    assert d["n_gpus"] == 2 and d["steps"] == 2 and d["warmup"] == 1 and d["scaling"] == "weak"
    assert d["config"]["global_batch"] == 8 and d["higher_is_better"] is True
    assert d["value"] > 0 and abs(d["value"] - 2 * 4 * 2.0 * 2 / (2 * d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    assert d["roofline"]["bound"] == "mfma" and 0 < d["roofline"]["frac"] < 1
    rk = d["ranks"]
    assert rk["world_size"] == 2 and rk["backend"] == "gloo"
    assert sorted(r["rank"] for r in rk["ranks"]) == [0, 1] and all(r["device"] == 0 for r in rk["ranks"])


@pytest.mark.timeout(600)
def test_bench_two_ranks_config3_block():
    """An N > 1 bench line carries BASELINE config 3 (512 x 10 s over the node) after its weak-scaling region: the
    2-rank rehearsal (gloo, both ranks on GPU 0) times 256 utterances per rank and reports them as `config3`."""
    import json
    p = _torchrun(["--full", "--gpus", "2", "--steps", "1", "--warmup", "1", "--batch", "4", "--seconds", "10",
                   "--no-cpu-baseline", "--dist-backend", "gloo", "--device", "0"], script="bench.py", timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["config"]["global_batch"] == 8 and d["ranks"]["world_size"] == 2
    c3 = d["config3"]
    assert c3["per_gpu_batch"] == 256 and c3["global_batch"] == 512 and c3["steps"] == 1
    assert c3["value"] > 0 and abs(c3["value"] - 512 * 10.0 / (c3["ms_per_step"] * 1e-3)) < 1e-6 * c3["value"]


@pytest.mark.timeout(600)
def test_bench_eight_ranks_rehearsal():
    """Verdict r05 item 4: the 8-rank launch the driver's N = 8 run makes, rehearsed on one GPU (gloo, every rank on
    GPU 0, a plain `python bench.py --gpus 8` that starts torch.distributed.run itself): the census has 8 distinct
    ranks in one process group of world size 8, the weak-scaling line is the 8-rank aggregate, and the config-3 block
    runs BASELINE config 3's 64 utterances per GPU (512 over the node) with 8 processes sharing the host."""
    import json
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, "-u", os.path.join(repo, "bench.py"), "--full", "--gpus", "8", "--steps", "2",
                        "--warmup", "1", "--batch", "2", "--seconds", "10", "--no-cpu-baseline", "--dist-backend",
                        "gloo", "--device", "0"], env=env, cwd=repo, capture_output=True, text=True, timeout=580)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 8 and d["config"]["global_batch"] == 16 and d["config"]["parallelism"] == "utterance-dp8"
    rk = d["ranks"]
    assert rk["world_size"] == 8 and rk["backend"] == "gloo" and len(rk["ranks"]) == 8
    assert sorted(r["rank"] for r in rk["ranks"]) == list(range(8))
    c3 = d["config3"]
    assert c3["per_gpu_batch"] == 64 and c3["global_batch"] == 512 and c3["steps"] == 2
    assert c3["value"] > 0 and abs(c3["value"] - 512 * 10.0 / (c3["ms_per_step"] * 1e-3)) < 1e-6 * c3["value"]


def test_predict_isolates_failing_file(tmp_path):
    """A batch that raises a recoverable error is re-run file by file; the file that fails alone is logged and
    skipped, every other file gets exactly its normal result."""
    import infer
    import hubertfa_amd.g2p as g2p_mod
    import torch
    from hubertfa_amd._lib import HFA_EINVAL, HFAArgumentError
    from hubertfa_amd.task import ForcedAlignmentTask
    seg, dpath, ck, n = _mixed_folder(tmp_path)
    g = g2p_mod.DictionaryG2P(dictionary=str(dpath))
    g.set_in_format("lab")
    rows = list(g.get_dataset(sorted(seg.rglob("*.wav"))))
    torch.set_grad_enabled(False)
    task = ForcedAlignmentTask.load_from_checkpoint(str(ck), device=torch.device("cuda"), hubert_model_path="synth:0")
    keys = list(range(len(rows)))
    ref = infer._predict(task, rows, keys, 4, [])
    assert sorted(ref) == keys
    poison = int(round(3.1 * 16000))                  # m1.wav's sample count
    submit = task.submit

    def bad_submit(waves, *a, lengths=None, **kw):
        lens = lengths if lengths is not None else [waves.shape[-1]] * waves.shape[0]
        if poison in lens:
            raise HFAArgumentError("injected: lattice beyond the kernel's limits", HFA_EINVAL)
        return submit(waves, *a, lengths=lengths, **kw)
    task.submit = bad_submit
    errors = []
    got = infer._predict(task, rows, keys, 4, errors)
    task.submit = submit
    assert len(errors) == 1 and str(errors[0][0]).endswith("m1.wav")
    assert sorted(got) == [k for k in keys if not str(rows[k][0]).endswith("m1.wav")]
    for k in got:
        for f in ("ph_time_int", "ph_idx_seq", "frame_confidence", "edge_diff"):
            assert np.array_equal(got[k][f], ref[k][f]), (k, f)


def test_infer_cli_skips_unreadable_and_multichannel(tmp_path):
    """A file that is not a WAV is logged and skipped (the rest of the folder is aligned); a stereo 24-bit file
    is aligned on its channel 0 (the reference's waveform[0]) exactly like the mono 16-bit file holding the same
    samples."""
    import struct
    from click.testing import CliRunner
    import infer
    from hubertfa_amd.wav_io import read_wav
    seg, dpath, ck, n = _mixed_folder(tmp_path)
    (seg / "zz_bad.wav").write_bytes(b"not a wav file at all")
    (seg / "zz_bad.lab").write_text((seg / "m0.lab").read_text())
    x, sr = read_wav(seg / "m3.wav")                                # 16-bit samples: exact in 24 bits
    v = np.round(x[0].astype(np.float64) * (1 << 23)).astype(np.int64)
    frames = np.stack([v, -v], axis=1).reshape(-1)                 # channel 1 differs
    pcm = b"".join(int(s & 0xFFFFFF).to_bytes(3, "little") for s in frames)
    fmt = struct.pack("<HHIIHH", 1, 2, sr, sr * 6, 6, 24)
    body = b"fmt " + struct.pack("<I", 16) + fmt + b"data" + struct.pack("<I", len(pcm)) + pcm
    (seg / "zz_st.wav").write_bytes(b"RIFF" + struct.pack("<I", 4 + len(body)) + b"WAVE" + body)
    (seg / "zz_st.lab").write_text((seg / "m3.lab").read_text())
    out = tmp_path / "out"
    r = CliRunner().invoke(infer.main, ["-c", str(ck), "-f", str(seg), "-d", str(dpath), "--hubert_path", "synth:0",
                                        "--batch_size", "4", "--out_path", str(out)])
    assert r.exit_code == 0, r.output + repr(r.exception)
    assert "zz_bad.wav" in r.output and "not a RIFF/WAVE file" in r.output
    got = {p.name for p in out.rglob("*.TextGrid")}
    assert "zz_bad.TextGrid" not in got and len(got) == n + 1
    assert (out / "TextGrid" / "zz_st.TextGrid").read_text() == (out / "TextGrid" / "m3.TextGrid").read_text()


def test_hip_error_fails_the_shard(tmp_path):
    """A HIP-level libhfa error (rc = -(hipError_t)) in the middle of a shard is not a per-file error: the rank
    reports its shard as failed (so it is re-queued on a healthy rank) instead of re-running and logging every
    file, and the errors the shard had logged before are dropped (its files are re-run elsewhere); an export error
    of one file in the streaming export is logged for that file and the rest are written."""
    import infer
    import hubertfa_amd.g2p as g2p_mod
    import torch
    from hubertfa_amd._lib import HFALibraryError
    from hubertfa_amd.task import ForcedAlignmentTask
    seg, dpath, ck, n = _mixed_folder(tmp_path)
    (seg / "zz_bad.wav").write_bytes(b"not a wav file at all")      # logged by the shard before the failure
    (seg / "zz_bad.lab").write_text((seg / "m0.lab").read_text())
    g = g2p_mod.DictionaryG2P(dictionary=str(dpath))
    g.set_in_format("lab")
    rows = list(g.get_dataset(sorted(seg.rglob("*.wav"))))
    torch.set_grad_enabled(False)
    task = ForcedAlignmentTask.load_from_checkpoint(str(ck), device=torch.device("cuda"), hubert_model_path="synth:0")
    keys = list(range(len(rows)))
    submit, calls = task.submit, []

    def hip_fail_submit(*a, **kw):
        calls.append(1)
        if len(calls) == 2:
            raise HFALibraryError("injected: hfa_conv_gemm_split failed (rc=-719): unspecified launch failure", -719)
        return submit(*a, **kw)
    task.submit = hip_fail_submit
    errors = [["earlier.wav", ValueError("logged before this shard")]]
    got, ok = infer._run(task, rows, keys, 2, errors)
    task.submit = submit
    assert not ok and got == {} and len(calls) == 2, (ok, len(calls))
    assert [e[0] for e in errors] == ["earlier.wav"]
    # streaming export: one file's TextGrid write fails -> that file is in the log, every other file is written
    stream = infer._StreamingExport(rows, task.melspec_config["sample_rate"], task.decoder.frame_length,
                                    str(tmp_path / "out"))
    write = stream.writer.write_textgrid

    def bad_write(pred, made=None):
        if str(pred[0]).endswith("m2.wav"):
            raise ValueError("overlapping intervals (injected)")
        return write(pred, made)
    stream.writer.write_textgrid = bad_write
    errors = []
    got, ok = infer._run(task, rows, keys, 2, errors, stream)
    preds, log = stream.results()
    assert ok and len(got) == n
    assert [str(e[0]).endswith("zz_bad.wav") for e in errors] == [True]
    assert len(log) == 1 and str(log[0][0]).endswith("m2.wav")
    assert sorted(p.name for p in (tmp_path / "out").rglob("*.TextGrid")) == \
        sorted(f"m{i}.TextGrid" for i in range(n) if i != 2)


def test_predict_decode_error_on_the_loader_thread(tmp_path, monkeypatch):
    """A file whose decode fails after the header scan (it changed on disk in between) fails on the loader thread,
    which decodes each batch one batch ahead of its launch: the error surfaces at that batch's launch, the batch is
    re-run file by file, the file is logged and skipped, and every other file gets exactly its normal result."""
    import infer
    import hubertfa_amd.g2p as g2p_mod
    import torch
    from hubertfa_amd import wav_io
    from hubertfa_amd.task import ForcedAlignmentTask
    seg, dpath, ck, n = _mixed_folder(tmp_path)
    g = g2p_mod.DictionaryG2P(dictionary=str(dpath))
    g.set_in_format("lab")
    rows = list(g.get_dataset(sorted(seg.rglob("*.wav"))))
    torch.set_grad_enabled(False)
    task = ForcedAlignmentTask.load_from_checkpoint(str(ck), device=torch.device("cuda"), hubert_model_path="synth:0")
    keys = list(range(len(rows)))
    ref = infer._predict(task, rows, keys, 2, [])
    real = wav_io.read_wav_into

    def flaky(path, row, channel=0):
        if str(path).endswith("m3.wav"):
            raise ValueError(f"{path}: changed on disk since the header scan")
        return real(path, row, channel=channel)
    monkeypatch.setattr(wav_io, "read_wav_into", flaky)
    errors = []
    got = infer._predict(task, rows, keys, 2, errors)
    assert len(errors) == 1 and str(errors[0][0]).endswith("m3.wav")
    assert sorted(got) == [k for k in keys if not str(rows[k][0]).endswith("m3.wav")]
    for k in got:
        for f in ("ph_time_int", "ph_idx_seq", "frame_confidence", "edge_diff"):
            assert np.array_equal(got[k][f], ref[k][f]), (k, f)
