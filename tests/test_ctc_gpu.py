"""The CTC kernels (csrc/ctc.hip) against torch's CPU ctc_loss in float64 and numpy, and the layers above them:
ops.ctc_score, AlignmentDecoder.ctc_batch, ForcedAlignmentTask.ctc_score_batch / align_batch(ctc=True),
score_transcripts.py.

Bar for nll, per row: |nll - nll_f64| / nll_f64 <= max(4 e32, 1e-6), e32 being the worst relative error of torch's own
float32 ctc_loss on the same batch (the log-mel test's precedent max(4 e_torch_f32, floor); the floor is about 8x the
1.2e-7 worst case of a numpy emulation of the kernel's scheme -- f32 alpha rebased every 16 steps against an f64 offset
-- which leaves room for the device's exp and log).  An oracle of +inf must be met by exactly +inf.  Measured on
MI355X: DESIGN.md §3.5.

Logits are seeded randn * scale in the head's layout: V + 2 columns, the CTC blank in column 1, label c in column
c + 2; columns 0 and 2 hold 1e30, which would wreck every result if a kernel read them.
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
F = torch.nn.functional

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REBASE = 16              # ctc.hip kRebase
PREFETCH = 8             # ctc.hip's prefetch group of the one-wave forms (4 and 2 at 8 and 16 waves)
FLOOR = 1e-6


def _head_layout(x):
    """CTC logits [B, T, V] -> the head's [B, T, V + 2] with garbage in the two columns that are not CTC's."""
    B, T, V = x.shape
    full = torch.full((B, T, V + 2), 1e30)
    full[:, :, 1] = x[:, :, 0]
    full[:, :, 3:] = x[:, :, 1:]
    return full


def _oracle(x, Ts, tgs, dtype):
    """torch's CPU ctc_loss per row on the row's own [:T] slice, in ``dtype``; T = 0 (torch refuses an empty input):
    the empty product, 0 for an empty transcript and +inf otherwise."""
    out = []
    for b, (T, tg) in enumerate(zip(Ts, tgs)):
        if T == 0:
            out.append(0.0 if len(tg) == 0 else float("inf"))
            continue
        lp = F.log_softmax(x[b, :T].to(dtype), dim=-1).unsqueeze(1)
        tgt = torch.as_tensor(np.asarray(tg, np.int64)).view(1, -1)
        out.append(float(F.ctc_loss(lp, tgt, [T], [len(tg)], blank=0, reduction="none", zero_infinity=False)[0]))
    return np.array(out, np.float64)


def _score(x, Ts, tgs):
    from hubertfa_amd import ops
    nll, best, ids, n = ops.ctc_score(_head_layout(x).cuda(), Ts, tgs, [len(t) for t in tgs])
    return nll.cpu().numpy(), best.cpu().numpy(), ids.cpu().numpy(), n.cpu().numpy()


def _check(tag, x, Ts, tgs):
    """Run the batch and hold every row's nll to the bar; returns the worst relative error."""
    want = _oracle(x, Ts, tgs, torch.float64)
    w32 = _oracle(x, Ts, tgs, torch.float32)
    fin = np.isfinite(want) & (want != 0)
    e32 = float(np.max(np.abs(w32[fin] - want[fin]) / want[fin])) if fin.any() else 0.0
    bound = max(4.0 * e32, FLOOR)
    got = _score(x, Ts, tgs)[0]
    assert got.dtype == np.float64 and not np.isnan(got).any()
    assert np.array_equal(got[~fin], want[~fin]), (tag, got[~fin], want[~fin])      # +inf (and 0 at T = L = 0) exactly
    e = float(np.max(np.abs(got[fin] - want[fin]) / want[fin])) if fin.any() else 0.0
    print(f"[{tag}] e_hip {e:.2e}  e_torch_f32 {e32:.2e}  bound {bound:.2e}")
    assert e <= bound, (tag, got, want)
    return e


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _targets(L, V, seed, repeats=None):
    """L ids in 1..V-1; ``repeats``: exactly that many adjacent equal pairs (None: whatever the draw gives)."""
    r = np.random.default_rng(seed)
    if repeats is None:
        return r.integers(1, V, L)
    t = np.empty(L, np.int64)
    rep = set(r.choice(np.arange(1, L), repeats, replace=False).tolist()) if repeats else set()
    for j in range(L):
        if j in rep:
            t[j] = t[j - 1]
        else:
            t[j] = r.integers(1, V)
            while j > 0 and t[j] == t[j - 1]:
                t[j] = r.integers(1, V)
    return t


# ---- 1. accuracy ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,V,L,scale", [(4, 861, 63, 45, 1), (4, 861, 63, 45, 6), (2, 70, 5, 33, 2),
                                           (1, 3000, 63, 300, 4), (3, 400, 63, 40, 30)])
def test_accuracy(B, T, V, L, scale):
    """Row 0 at full T and L with targets[0, 1] = targets[0, 0]; the other rows shorter.  scale = 30: a near one-hot
    softmax, most paths thousands of nats below the best one."""
    x = _randn((B, T, V), 100 + T + L) * scale
    Ts = [T - (T // 7) * b for b in range(B)]
    tgs = [_targets(L // (b + 1), V, 200 + b) for b in range(B)]
    tgs[0][1] = tgs[0][0]
    _check(f"accuracy B={B} T={T} V={V} L={L} scale={scale}", x, Ts, tgs)


# ---- 2. state tiling -----------------------------------------------------------------------------------------------
# L + 1 (blank, label) pairs over lanes: one wave with 1 / 2 / 4 pairs per lane up to 64 / 128 / 256 pairs, 4 pairs per
# lane over 2 / 4 / 8 / 16 waves up to 512 / 1024 / 2048 / 4096 pairs, then 8 pairs per lane over 16 waves.  So the
# form changes between L = 63|64, 127|128, 255|256, 511|512, 1023|1024, 2047|2048, 4095|4096; lanes change at every
# multiple of the pairs per lane and waves at every 64 lanes (L = 300: two waves of 4 pairs per lane).
ISSUE_L = [0, 1, 2, 31, 32, 63, 64, 127, 128, 255, 256, 300]
FORM_L = [511, 512, 1023, 1024, 2047, 2048]


@pytest.mark.parametrize("L", ISSUE_L + FORM_L)
def test_state_tiling_edges(L):
    T, V = 2 * L + 5, 63
    _check(f"tiling L={L} T={T}", _randn((1, T, V), 300 + L), [T], [_targets(L, V, 400 + L)])


@pytest.mark.parametrize("L", [4095, 4096])
def test_state_tiling_widest_forms(L):
    """The last 4-pairs form and the first 8-pairs one (16 waves); T = L + L / 8 + 8 keeps the CPU oracle quick."""
    T, V = L + L // 8 + 8, 63
    _check(f"tiling L={L} T={T}", _randn((1, T, V), 300 + L), [T], [_targets(L, V, 400 + L)])


# ---- 3. time edges -------------------------------------------------------------------------------------------------
TIME_EDGES = sorted({1, 2, 3, PREFETCH - 1, PREFETCH, PREFETCH + 1, 2 * PREFETCH + 1, REBASE - 1, REBASE, REBASE + 1,
                     2 * REBASE + 1})


def test_time_edges():
    """T around the prefetch group, the two groups in flight and the rebase period, with L = 0, L = 1 and L = T
    without repeats (one feasible path); every (T, L) also alone, where the form follows its own L."""
    V = 63
    cases = [(T, L) for T in TIME_EDGES for L in (0, 1, T)]
    x = _randn((len(cases), max(TIME_EDGES), V), 500) * 2
    Ts = [T for T, _ in cases]
    tgs = [_targets(L, V, 600 + i, repeats=0) for i, (_, L) in enumerate(cases)]
    _check("time edges (one batch)", x, Ts, tgs)
    for T in TIME_EDGES:
        i = cases.index((T, T))
        _check(f"time edges T=L={T} alone", x[i:i + 1, :T], [T], [tgs[i]])


def test_empty_utterance():
    """T = 0 (torch's ctc_loss refuses it): the empty product, nll = 0 for L = 0 and +inf for L > 0; n = 0."""
    x = _randn((2, 4, 9), 7)
    nll, _, _, n = _score(x, [0, 0], [np.zeros(0, np.int64), np.array([3, 4])])
    assert nll[0] == 0.0 and nll[1] == np.inf and n.tolist() == [0, 0]


# ---- 4. infeasible and degenerate ----------------------------------------------------------------------------------
def test_infeasible_and_degenerate():
    V, L = 20, 12
    rows = [(L - 1, _targets(L, V, 1, repeats=0), True),              # T < L
            (L, _targets(L, V, 2, repeats=1), True),                  # T = L with one adjacent repeat
            (L + 3 - 1, _targets(L, V, 3, repeats=3), True),          # T = L + r - 1 with r = 3 repeats
            (L + 3, _targets(L, V, 3, repeats=3), False),             # ... and one frame more: feasible
            (2 * L - 1, np.full(L, 5), False)]                        # all-equal targets at T = 2 L - 1: one path
    x = _randn((len(rows), 2 * L, V), 700) * 3
    Ts, tgs = [r[0] for r in rows], [r[1] for r in rows]
    _check("infeasible / degenerate", x, Ts, tgs)
    nll, best, ids, n = _score(x, Ts, tgs)
    assert not np.isnan(nll).any()
    assert [bool(np.isposinf(v)) for v in nll] == [r[2] for r in rows]


# ---- 5. batch independence -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [0, 8])
def test_batch_rows_equal_rows_alone(cap):
    """NaN in every logit row t >= T[b] and -1 in targets[b, L[b]:]: nothing past a row's own lengths reaches a result,
    and every row has the bits it has alone at B = 1 (where the forward takes the form of its own L); again with the
    prologue's grid capped at 8 workgroups."""
    import contextlib
    from hubertfa_amd import ops
    V = 63
    Ts, Ls = [861, 300, 17, 1, 640], [45, 140, 0, 1, 70]
    x = _head_layout(_randn((5, max(Ts), V), 800) * 3)
    tg = np.full((5, max(Ls)), -1, np.int32)
    for b in range(5):
        x[b, Ts[b]:] = float("nan")
        tg[b, :Ls[b]] = _targets(Ls[b], V, 810 + b)
    i32 = lambda a: torch.as_tensor(np.asarray(a, np.int32)).cuda()      # noqa: E731

    def run(logits, T, L, targets):
        with (ops.grid_cap(cap) if cap else contextlib.nullcontext()):
            emis, best = ops.ctc_prologue(logits.cuda(), i32(T), i32(L), i32(targets))
            nll = ops.ctc_forward(emis, i32(T), i32(L), i32(targets))
            ids, n = ops.ctc_greedy(best, i32(T))
        return nll.cpu().numpy(), best.cpu().numpy(), ids.cpu().numpy(), n.cpu().numpy()
    nll, best, ids, n = run(x, Ts, Ls, tg)
    assert np.isfinite(nll).all()
    for b in range(5):
        a_nll, a_best, a_ids, a_n = run(x[b:b + 1, :Ts[b]], Ts[b:b + 1], Ls[b:b + 1], tg[b:b + 1, :Ls[b]])
        assert nll[b].tobytes() == a_nll[0].tobytes(), (b, nll[b], a_nll[0])
        assert n[b] == a_n[0] and np.array_equal(best[b, :Ts[b]], a_best[0]) and \
            np.array_equal(ids[b, :n[b]], a_ids[0, :a_n[0]]), b


# ---- 6. greedy decode ----------------------------------------------------------------------------------------------
def _greedy_numpy(ctc_logits):
    """tools/alignment_decoder.py:145-150."""
    ctc = np.argmax(ctc_logits, axis=-1)
    ctc_index = np.concatenate([[0], ctc])
    ctc_index = (ctc_index[1:] != ctc_index[:-1]) * ctc != 0
    return ctc[ctc_index]


def _onehot(classes, V):
    x = np.zeros((len(classes), V), np.float32)
    x[np.arange(len(classes)), classes] = 5.0
    return x


def test_greedy_decode():
    from hubertfa_amd.alignment_decoder import AlignmentDecoder
    V = 63
    ties = np.zeros((6, V), np.float32)                 # exact ties: the lowest class wins (np.argmax)
    ties[0, [7, 3, 40]] = 2.0                           # -> 3
    ties[1, [3, 62]] = 1.0                              # -> 3 again (a repeat: dropped)
    ties[2, :] = 0.0                                    # all equal -> 0, the blank
    ties[3, [62, 61]] = 9.0                             # -> 61
    ties[4, [0, 5]] = 4.0                               # -> 0
    ties[5, [5, 64 % V + 10]] = 4.0                     # -> 5
    rows = {"random": _randn((200, V), 900).numpy(),
            "ties": ties,
            "repeats": _onehot([4, 4, 0, 4, 4, 9, 9, 0, 0, 9, 4], V),      # 4 4 _ 4 4 9 9 _ _ 9 4 -> 4 4 9 9 4
            "all blank": _onehot([0] * 70, V),
            "T=1": _onehot([17], V),
            "T=1 blank": _onehot([0], V),
            "every frame changes": _onehot([1 + (7 * t) % 61 for t in range(300)], V)}
    names = list(rows)
    Ts = [rows[k].shape[0] for k in names]
    x = torch.zeros((len(names), max(Ts), V))
    for b, k in enumerate(names):
        x[b, :Ts[b]] = torch.from_numpy(rows[k])
    _, best, ids, n = _score(x, Ts, [np.zeros(0, np.int64)] * len(names))
    dec = AlignmentDecoder({"vocab": {}}, {"hop_length": 512, "sample_rate": 44100})
    for b, k in enumerate(names):
        want = _greedy_numpy(rows[k])
        assert np.array_equal(best[b, :Ts[b]], np.argmax(rows[k], axis=-1)), k
        assert np.array_equal(ids[b, :n[b]], want), (k, ids[b, :n[b]], want)
        dec.ctc_logits = rows[k]
        assert np.array_equal(ids[b, :n[b]], dec.ctc()), k
    assert ids[names.index("ties"), :n[names.index("ties")]].tolist() == [3, 61, 5]
    assert ids[names.index("repeats"), :n[names.index("repeats")]].tolist() == [4, 4, 9, 9, 4]
    assert n[names.index("all blank")] == 0 and n[names.index("T=1")] == 1 and n[names.index("T=1 blank")] == 0
    assert n[names.index("every frame changes")] == 300


# ---- 7. task level -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def task(tmp_path_factory):
    """The synthetic Hubert-base checkpoint of tests/ckpt_files.py (a HF folder + a Lightning .ckpt naming it)."""
    pytest.importorskip("transformers")
    import ckpt_files
    from hubertfa_amd.task import ForcedAlignmentTask
    tmp = str(tmp_path_factory.mktemp("ctc_ckpt"))
    meta = json.load(open(os.path.join(REPO, "tests", "golden", "loaders.json")))
    folder = os.path.join(tmp, "cnhubert")
    ckpt_files.write_hf_folder(folder, "hf")
    path = os.path.join(tmp, "model.ckpt")
    ckpt_files.write_lightning_ckpt(path, meta, hubert_model_path=folder)
    t = ForcedAlignmentTask.load_from_checkpoint(path, device=torch.device("cuda"))
    t.ckpt_path = path
    return t


@functools.lru_cache(maxsize=None)
def _waves():
    from hubertfa_amd import synth
    sr = 44100
    lens = [int(0.6 * sr), int(1.3 * sr), int(2.0 * sr)]
    batch = np.zeros((3, max(lens)), np.float32)
    for b, n in enumerate(lens):
        batch[b, :n] = synth.synth_audio(n, sr, seed=90 + b)
    return batch, lens


def _transcripts(task):
    """SP-framed transcripts over the synthetic vocabulary (an ignored phoneme inside one of them)."""
    names = [p for p, i in task.vocab["vocab"].items() if i != 0]
    r = np.random.default_rng(5)
    seqs = []
    for b, k in enumerate((4, 7, 9)):
        ph = ["SP"] + [names[int(i)] for i in r.integers(0, len(names), k)] + ["SP"]
        if b == 1:
            ph.insert(3, "AP")
        seqs.append(ph)
    return seqs


def test_task_ctc_score_batch(task):
    batch, lens = _waves()
    waves = torch.from_numpy(batch).cuda()
    seqs = _transcripts(task)
    res = task.ctc_score_batch(waves, seqs, lengths=lens)
    assert len(res) == 3
    feats, n_frames, wl = task.encode_batch(waves, lengths=lens)
    for b, r in enumerate(res):
        alone = task.ctc_score_batch(waves[b:b + 1, :lens[b]], seqs[b:b + 1])[0]
        # T: the frames decode keeps (alignment_decoder.py:45-50), at most the n_frames encode_batch returns
        assert r["T"] == alone["T"] == task.decoder.num_frames(wl[b], n_frames[b]) <= n_frames[b]
        assert np.float64(r["ctc_nll"]).tobytes() == np.float64(alone["ctc_nll"]).tobytes(), b
        assert r["ctc_confidence"] == alone["ctc_confidence"] and r["ctc_phones"] == alone["ctc_phones"]
        assert np.array_equal(r["ctc_phone_ids"], alone["ctc_phone_ids"])
        assert r["ctc_confidence"] == float(np.clip(np.exp(-r["ctc_nll"] / r["T"]), 1e-6, 1 - 1e-6))
        # against torch's f64 CTC on task.forward's ctc_logits for the same features
        T = r["T"]
        frame, edge, ctc = task.forward(feats[b:b + 1, :n_frames[b]])     # (decode trims the logits to T itself)
        x = ctc[0, :T].cpu()
        tg = task.decoder.ctc_targets(seqs[b])
        want = _oracle(x[None], [T], [tg], torch.float64)[0]
        e32 = abs(_oracle(x[None], [T], [tg], torch.float32)[0] - want) / want
        e = abs(r["ctc_nll"] - want) / want
        print(f"[task row {b}] T={T} L={len(tg)} nll {r['ctc_nll']:.6f}  e_hip {e:.2e}  e_torch_f32 {e32:.2e}")
        assert e <= max(4 * e32, FLOOR)
        # the greedy phones against the host helper after a plain decode of that utterance
        task.decoder.decode(frame, edge, ctc, wl[b], seqs[b])
        assert np.array_equal(r["ctc_phone_ids"], task.decoder.ctc())
        inv = task.decoder.id_to_phone()
        assert r["ctc_phones"] == [inv[int(i)] for i in r["ctc_phone_ids"]]


def test_task_align_batch_ctc(task):
    batch, lens = _waves()
    waves = torch.from_numpy(batch).cuda()
    seqs = _transcripts(task)
    plain = task.align_batch(waves, seqs, lengths=lens)
    both = task.align_batch(waves, seqs, lengths=lens, ctc=True)
    score = task.ctc_score_batch(waves, seqs, lengths=lens)
    for p, q, s in zip(plain, both, score):
        assert not [k for k in p if k.startswith("ctc_")]
        assert set(q) - set(p) == {"ctc_nll", "ctc_confidence", "ctc_phones", "ctc_phone_ids"}
        for k in p:
            assert np.array_equal(np.asarray(p[k]), np.asarray(q[k])), k
        assert np.float64(q["ctc_nll"]).tobytes() == np.float64(s["ctc_nll"]).tobytes()
        assert q["ctc_confidence"] == s["ctc_confidence"] and q["ctc_phones"] == s["ctc_phones"]


def test_task_wrong_transcript_scores_worse(task):
    """Right: the row's own greedy phones as its transcript; wrong: those reversed, or another row's phones."""
    batch, lens = _waves()
    waves = torch.from_numpy(batch).cuda()
    greedy = [r["ctc_phones"] for r in task.ctc_score_batch(waves, [["SP"]] * 3, lengths=lens)]
    assert all(len(g) >= 2 and g != g[::-1] for g in greedy), greedy
    right = task.ctc_score_batch(waves, greedy, lengths=lens)
    rev = task.ctc_score_batch(waves, [g[::-1] for g in greedy], lengths=lens)
    other = task.ctc_score_batch(waves, [greedy[(b + 1) % 3] for b in range(3)], lengths=lens)
    for b in range(3):
        T = right[b]["T"]
        print(f"[row {b}] nll/T right {right[b]['ctc_nll'] / T:.4f}  reversed {rev[b]['ctc_nll'] / T:.4f}  "
              f"another row's {other[b]['ctc_nll'] / T:.4f}")
        assert right[b]["ctc_nll"] / T < rev[b]["ctc_nll"] / T
        assert right[b]["ctc_nll"] / T < other[b]["ctc_nll"] / T


# ---- 8. CLI --------------------------------------------------------------------------------------------------------
def test_score_transcripts_cli(task, tmp_path):
    import csv
    from hubertfa_amd import synth
    import hubertfa_amd.g2p as g2p_mod
    from hubertfa_amd.wav_io import read_wav, write_wav
    d = synth.synth_dictionary(n_words=40)
    dpath = tmp_path / "dict.txt"
    dpath.write_text("".join(f"{w}\t{' '.join(p)}\n" for w, p in d.items()))
    seg = tmp_path / "segments"
    seg.mkdir()
    secs = (0.9, 1.6, 1.2)
    for i, s in enumerate(secs):
        write_wav(seg / f"u{i}.wav", synth.synth_audio(int(s * 44100), 44100, seed=80 + i), 44100)
        (seg / f"u{i}.lab").write_text(synth.synth_lab(3 + i, d, seed=i))
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, os.path.join(REPO, "score_transcripts.py"), "-c", task.ckpt_path, "-f",
                        str(seg), "-g", "Dictionary", "-d", str(dpath), "--batch_size", "4"], env=env, cwd=REPO,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    rows = list(csv.DictReader(open(seg / "ctc_scores.csv", newline="", encoding="utf-8")))
    assert len(rows) == 3 and sorted(r["name"] for r in rows) == ["u0", "u1", "u2"]
    conf = [float(r["ctc_confidence"]) for r in rows]
    assert conf == sorted(conf)
    g = g2p_mod.DictionaryG2P(dictionary=str(dpath))
    g.set_in_format("lab")
    data = {os.path.basename(str(w))[:-4]: ph for w, ph, _, _ in g.get_dataset(sorted(seg.rglob("*.wav")))}
    from score_transcripts import edit_distance
    for r in rows:
        x, sr = read_wav(str(seg / (r["name"] + ".wav")))
        ph = data[r["name"]]
        want = task.ctc_score_batch(torch.from_numpy(np.ascontiguousarray(x[:1])).cuda(), [ph])[0]
        nonsp = [q for q in ph if task.vocab["vocab"][q] != 0]
        assert float(r["ctc_nll"]) == want["ctc_nll"] and float(r["ctc_confidence"]) == want["ctc_confidence"]
        assert int(r["n_frames"]) == want["T"] and int(r["n_phones"]) == len(nonsp)
        assert r["ctc_phones"].split() == want["ctc_phones"]
        assert int(r["phone_edit_distance"]) == edit_distance(want["ctc_phones"], nonsp)
