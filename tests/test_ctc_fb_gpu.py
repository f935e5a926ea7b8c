"""The CTC forward-backward kernels (csrc/ctc.hip: hfa_ctc_forward_alpha, hfa_ctc_backward, hfa_ctc_grad) and the layers
above them (ops.ctc_posteriors / ctc_nll, AlignmentDecoder.ctc_batch(posteriors=True), ForcedAlignmentTask.
ctc_score_batch(posteriors=True), score_transcripts.py --phones) against the float64 oracle of tests/ctc_fb_ref.py.

The bar, per array and per row: |device - oracle| <= max(4 e_emu, floor), e_emu being the worst error on that array of
the float32 emulation of the kernels' documented scheme (ctc_fb_ref.emulate) and floor = 2e-5 for occ and grad (three
f32 roundings at magnitude <= 64 in the exponent of a value <= 1), times the row's T for frames, centre and logp, which
are sums over t.  torch's float32 ctc_loss is no yardstick here: its alpha is not rebased and its gradient is off by
2e-3 .. 5e-2 at T >= 400.  Measured on MI355X: DESIGN.md §3.6.

Logits are seeded randn * scale in the head's layout (V + 2 columns, 1e30 in columns 0 and 2).
"""
import contextlib
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import ctc_fb_ref as ref

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _randn(shape, seed):
    return (np.random.default_rng(seed).standard_normal(shape)).astype(np.float32)


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


def _run(x, Ts, tgs, cap=0, nan_fill=False, weight=None, pad_targets=0):
    """The kernels on a batch: x [B, Tmax, V] CTC logits (numpy; put into the head's layout here), row lengths Ts and
    target lists tgs.  ``nan_fill``: NaN in every logit row t >= T[b] and in every output beforehand; ``pad_targets``:
    the value of targets[b, L[b]:].  Returns numpy arrays; ctc_forward_alpha's nll is held to ctc_forward's bits."""
    from hubertfa_amd import ops
    B, Tmax, V = x.shape
    Ls = [len(t) for t in tgs]
    Lmax = max(Ls) if Ls else 0
    full = ref.head_layout(x)
    if nan_fill:
        for b in range(B):
            full[b, Ts[b]:] = np.nan
    _, _, tg_h, cp, ci = ops.ctc_class_index(Ts, tgs, Ls, V)
    tg_h = tg_h.copy()
    for b in range(B):
        tg_h[b, Ls[b]:] = pad_targets
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()      # noqa: E731
    logits, T_t, L_t, tg_t = dev(full), dev(np.asarray(Ts, np.int32)), dev(np.asarray(Ls, np.int32)), dev(tg_h)
    fill = (lambda *s: torch.full(s, float("nan"), device="cuda")) if nan_fill else \
        (lambda *s: torch.empty(s, device="cuda"))
    with (ops.grid_cap(cap) if cap else contextlib.nullcontext()):
        emis, _ = ops.ctc_prologue(logits, T_t, L_t, tg_t)
        plain = ops.ctc_forward(emis, T_t, L_t, tg_t)
        nll, alpha, aoff = ops.ctc_forward_alpha(emis, T_t, L_t, tg_t)
        out = (fill(B, Tmax, Lmax + 1), fill(B, Lmax), fill(B, Lmax), fill(B, Lmax))
        occ, frames, centre, logp = ops.ctc_backward(emis, T_t, L_t, tg_t, nll, alpha, aoff, out=out)
        g = fill(B, Tmax, V + 2) if nan_fill else None
        grad = ops.ctc_grad(logits, T_t, L_t, occ, nll, dev(cp), dev(ci),
                            None if weight is None else dev(np.asarray(weight, np.float32)), out=g)
    torch.cuda.synchronize()
    assert nll.cpu().numpy().tobytes() == plain.cpu().numpy().tobytes(), "forward_alpha's nll differs from forward's"
    grad = grad.cpu().numpy()
    if nan_fill:
        assert np.isnan(grad[:, :, [0, 2]]).all(), "hfa_ctc_grad touched a column that is no CTC class"
    else:
        assert not grad[:, :, [0, 2]].any()
    return dict(nll=nll.cpu().numpy(), occ=occ.cpu().numpy(), frames=frames.cpu().numpy(),
                centre=centre.cpu().numpy(), logp=logp.cpu().numpy(),
                grad=np.concatenate([grad[:, :, 1:2], grad[:, :, 3:]], axis=2))


def _row(d, b, T, L):
    """Row b of a device result within its own T and L, after checking that everything past them is zero."""
    for k in ("occ", "grad"):
        assert not np.isnan(d[k][b]).any(), (k, b)
        assert not d[k][b, T:].any(), (k, b)
    assert not d["occ"][b, :, L + 1:].any(), b
    for k in ("frames", "centre", "logp"):
        assert not np.isnan(d[k][b]).any() and not d[k][b, L:].any(), (k, b)
    return dict(nll=d["nll"][b], occ=d["occ"][b, :T, :L + 1], grad=d["grad"][b, :T], frames=d["frames"][b, :L],
                centre=d["centre"][b, :L], logp=d["logp"][b, :L])


def _hold(tag, got, x, tg, w=1.0):
    """Hold one row to the bar; prints every figure before it asserts.  Returns the worst error per array."""
    T = x.shape[0]
    want, emu = ref.oracle(x, tg), ref.emulate(x, tg)
    bar = ref.bars(want, emu, T)
    if not np.isfinite(want["nll"]):
        assert got["nll"] == np.inf and not got["occ"].any() and not got["grad"].any(), tag
        assert not got["frames"].any() and not got["centre"].any() and np.all(np.isneginf(got["logp"])), tag
        return {}
    assert abs(got["nll"] - want["nll"]) <= 1e-6 * max(abs(want["nll"]), 1e-30) or want["nll"] == got["nll"], tag
    errs = {}
    for k in ("occ", "frames", "centre", "logp", "grad"):
        ref_k = want[k] * w if k == "grad" else want[k]
        errs[k] = float(np.max(np.abs(got[k] - ref_k))) if ref_k.size else 0.0
    errs["rowsum"] = float(np.max(np.abs(got["occ"].sum(axis=1, dtype=np.float64) - 1))) if T else 0.0
    print(f"[{tag}] " + "  ".join(f"{k} {errs[k]:.1e} (bar {bar[k]:.1e})" for k in errs))
    for k in errs:
        lim = max(bar[k] * abs(w), ref.FLOOR) if k == "grad" else bar[k]
        assert errs[k] <= lim, (tag, k, errs[k], lim)
    return errs


def _check(tag, x, Ts, tgs, **kw):
    d = _run(x, Ts, tgs, **kw)
    assert not np.isnan(d["nll"]).any()
    for b, (T, tg) in enumerate(zip(Ts, tgs)):
        _hold(f"{tag} row {b}", _row(d, b, T, len(tg)), x[b, :T], tg)
    return d


# ---- 1. accuracy ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,V,L,scale", [(4, 861, 63, 45, 1), (4, 861, 63, 45, 6), (2, 70, 5, 33, 2),
                                           (3, 400, 63, 40, 30)])
def test_accuracy(B, T, V, L, scale):
    """Row 0 at full T and L with targets[0, 1] = targets[0, 0]; the other rows shorter."""
    x = _randn((B, T, V), 100 + T + L) * scale
    Ts = [T - (T // 7) * b for b in range(B)]
    tgs = [_targets(L // (b + 1), V, 200 + b) for b in range(B)]
    tgs[0][1] = tgs[0][0]
    _check(f"accuracy B={B} T={T} V={V} L={L} scale={scale}", x, Ts, tgs)


# ---- 2. state tiling -----------------------------------------------------------------------------------------------
# The forms change between L = 63|64, 127|128, 255|256, 511|512, 1023|1024, 2047|2048, 4095|4096 (as the forward's).
@pytest.mark.parametrize("L", [0, 1, 2, 63, 64, 127, 128, 255, 256, 300, 511, 512, 1023, 1024, 2047, 2048])
def test_state_tiling_edges(L):
    T, V = 2 * L + 5, 63
    _check(f"tiling L={L} T={T}", _randn((1, T, V), 300 + L), [T], [_targets(L, V, 400 + L)])


@pytest.mark.parametrize("L", [4095, 4096])
def test_state_tiling_widest_forms(L):
    T, V = L + L // 8 + 8, 63
    _check(f"tiling L={L} T={T}", _randn((1, T, V), 300 + L), [T], [_targets(L, V, 400 + L)])


# ---- 3. time edges -------------------------------------------------------------------------------------------------
TIME_EDGES = [1, 2, 3, 7, 8, 9, 15, 16, 17, 33]


def test_time_edges():
    """T around the prefetch groups and the rebase period, each with L = 0, 1 and T (no repeats: one feasible path),
    in one batch and alone; alone every row has the batch's bits."""
    V = 63
    cases = [(T, L) for T in TIME_EDGES for L in (0, 1, T)]
    x = _randn((len(cases), max(TIME_EDGES), V), 500) * 2
    Ts = [T for T, _ in cases]
    tgs = [_targets(L, V, 600 + i, repeats=0) for i, (_, L) in enumerate(cases)]
    d = _check("time edges (one batch)", x, Ts, tgs)
    for i, (T, L) in enumerate(cases):
        a = _row(_run(x[i:i + 1, :T], [T], [tgs[i]]), 0, T, L)
        r = _row(d, i, T, L)
        for k in r:
            assert np.asarray(r[k]).tobytes() == np.asarray(a[k]).tobytes(), (T, L, k)
        if L == T:                                       # one path: gamma is 0 or 1 (its accuracy: the bar above)
            assert np.allclose(a["occ"][:, 1:], np.eye(T), atol=1e-3) and np.allclose(a["occ"][:, 0], 0, atol=1e-3)


# ---- 4. repeated labels --------------------------------------------------------------------------------------------
def test_repeated_labels():
    """The rows where the skip rule and the class index matter: pairs of equal labels, and all-equal targets at
    T = 2 L - 1 (one path: gamma is 0 or 1, blanks between the labels)."""
    x = _randn((1, 23, 9), 700) * 2
    _check("repeats pairs", x, [23], [np.array([1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6])])
    L = 12
    x = _randn((1, 2 * L - 1, 9), 701) * 2
    d = _check("repeats all equal", x, [2 * L - 1], [np.full(L, 5)])
    occ = d["occ"][0]
    assert np.allclose(occ[0::2, 1:], np.eye(L), atol=1e-3) and np.allclose(occ[1::2, 0], 1, atol=1e-3)
    assert np.allclose(d["frames"][0], 1, atol=1e-3) and np.allclose(d["centre"][0], 2 * np.arange(L), atol=1e-2)


# ---- 5. infeasible and empty ---------------------------------------------------------------------------------------
def test_infeasible_and_empty():
    V, L = 20, 12
    rows = [(L - 1, _targets(L, V, 1, repeats=0), True),              # T < L
            (L, _targets(L, V, 2, repeats=1), True),                  # T = L with one adjacent repeat
            (L + 3 - 1, _targets(L, V, 3, repeats=3), True),          # T = L + r - 1 with r = 3 repeats
            (L + 3, _targets(L, V, 3, repeats=3), False),             # ... and one frame more: feasible
            (2 * L - 1, np.full(L, 5), False),                        # all-equal targets at T = 2 L - 1: one path
            (0, np.zeros(0, np.int64), False),                        # T = L = 0: nothing but zeros
            (0, np.array([3, 4]), True)]                              # T = 0 with L = 2
    x = _randn((len(rows), 2 * L, V), 700) * 3
    d = _check("infeasible / empty", x, [r[0] for r in rows], [r[1] for r in rows], nan_fill=True)
    assert [bool(np.isposinf(v)) for v in d["nll"]] == [r[2] for r in rows] and d["nll"][5] == 0.0
    for b, (T, tg, bad) in enumerate(rows):
        if bad:
            assert not d["occ"][b].any() and not d["grad"][b].any() and not d["frames"][b].any()
            assert np.all(np.isneginf(d["logp"][b, :len(tg)])) and not d["logp"][b, len(tg):].any()


# ---- 6. batch independence -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [0, 8])
def test_batch_rows_equal_rows_alone(cap):
    """NaN in every logit row t >= T[b], -1 in targets[b, L[b]:] and NaN in every output beforehand: every row's occ,
    summaries and grad, within its own T and L, have the bits it gets alone at B = 1 (where the kernels take the form
    of its own L), and everything past them is zero; again with the row kernels' grid capped at 8 workgroups."""
    V = 63
    Ts, Ls = [861, 300, 17, 1, 640], [45, 140, 0, 1, 70]
    x = _randn((5, max(Ts), V), 800) * 3
    tgs = [_targets(Ls[b], V, 810 + b) for b in range(5)]
    w = [0.5, 1.0, -0.75, 0.25, 1.0]
    d = _run(x, Ts, tgs, cap=cap, nan_fill=True, weight=w, pad_targets=-1)
    assert np.isfinite(d["nll"]).all()
    for b in range(5):
        r = _row(d, b, Ts[b], Ls[b])
        a = _row(_run(x[b:b + 1, :Ts[b]], Ts[b:b + 1], tgs[b:b + 1], cap=cap, nan_fill=True, weight=w[b:b + 1]), 0,
                 Ts[b], Ls[b])
        for k in r:
            assert np.asarray(r[k]).tobytes() == np.asarray(a[k]).tobytes(), (b, k)


# ---- 7. autograd ---------------------------------------------------------------------------------------------------
def test_autograd():
    """(ctc_nll(x) * w).sum().backward() against the same expression on torch float64 (log_softmax inside the graph),
    B = 3 with distinct w and one infeasible row, whose nll stays +inf and whose gradient is zero."""
    from hubertfa_amd import ops
    F = torch.nn.functional
    V, Ts = 20, [50, 9, 37]
    tgs = [_targets(12, V, 1), _targets(10, V, 2), _targets(9, V, 3, repeats=2)]        # row 1: T < L
    w = np.array([0.5, 1.0, -0.75])
    x = _randn((3, 50, V), 900) * 3
    xg = torch.from_numpy(ref.head_layout(x)).cuda().requires_grad_(True)
    with torch.enable_grad():                            # (the CLIs switch autograd off process-wide)
        nll = ops.ctc_nll(xg, Ts, tgs, [len(t) for t in tgs])
        assert nll.dtype == torch.float64 and nll.requires_grad
        (nll * torch.from_numpy(w).cuda()).sum().backward()
    got = xg.grad.cpu().numpy()
    assert not got[:, :, [0, 2]].any() and not np.isnan(got).any()
    assert torch.isposinf(nll[1]) and not got[1].any()
    got = np.concatenate([got[:, :, 1:2], got[:, :, 3:]], axis=2)
    for b in (0, 2):
        xt = torch.from_numpy(x[b, :Ts[b]]).double().requires_grad_(True)
        with torch.enable_grad():
            loss = F.ctc_loss(F.log_softmax(xt, dim=-1).unsqueeze(1), torch.from_numpy(tgs[b]).view(1, -1), [Ts[b]],
                              [len(tgs[b])], blank=0, reduction="sum") * w[b]
            loss.backward()
        want = xt.grad.numpy()
        o, e = ref.oracle(x[b, :Ts[b]], tgs[b]), ref.emulate(x[b, :Ts[b]], tgs[b])
        bar = max(ref.bars(o, e, Ts[b])["grad"] * abs(w[b]), ref.FLOOR)
        err = float(np.max(np.abs(got[b, :Ts[b]] - want)))
        print(f"[autograd row {b}] grad err {err:.1e} (bar {bar:.1e})  nll {float(nll[b].detach()):.6f} vs {o['nll']:.6f}")
        assert err <= bar and not got[b, Ts[b]:].any()
        assert abs(float(nll[b].detach()) - o["nll"]) <= 1e-6 * o["nll"]


# ---- 8. localisation -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 5, 11])
def test_localisation(k):
    from hubertfa_amd import ops
    x, tg = ref.localisation_fixture(k)
    nll, occ, frames, centre, logp, best, ids, n = ops.ctc_posteriors(
        torch.from_numpy(ref.head_layout(x[None])).cuda(), [96], [tg], [12])
    got = dict(nll=float(nll[0]), occ=occ[0].cpu().numpy(), frames=frames[0].cpu().numpy(),
               centre=centre[0].cpu().numpy(), logp=logp[0].cpu().numpy())
    want, emu = ref.oracle(x, tg), ref.emulate(x, tg)
    bar = ref.bars(want, emu, 96)
    for key in ("occ", "frames", "centre", "logp"):
        err = float(np.max(np.abs(got[key] - want[key])))
        print(f"[localisation k={k}] {key} {err:.1e} (bar {bar[key]:.1e})")
        assert err <= bar[key], key
    assert int(np.argmin(np.exp(got["logp"]))) == k
    true = [3, 7, 11, 5, 9, 2, 14, 6, 17, 8, 12, 4]
    assert ids[0, :int(n[0])].cpu().tolist() == true          # the greedy decode rides along, as ctc_score gives it


# ---- 9. task and CLI -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def task(tmp_path_factory):
    """The synthetic Hubert-base checkpoint of tests/ckpt_files.py (a HF folder + a Lightning .ckpt naming it)."""
    pytest.importorskip("transformers")
    import ckpt_files
    from hubertfa_amd.task import ForcedAlignmentTask
    tmp = str(tmp_path_factory.mktemp("ctc_fb_ckpt"))
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
    names = [p for p, i in task.vocab["vocab"].items() if i != 0]
    r = np.random.default_rng(5)
    seqs = []
    for b, k in enumerate((4, 7, 9)):
        ph = ["SP"] + [names[int(i)] for i in r.integers(0, len(names), k)] + ["SP"]
        if b == 1:
            ph.insert(3, "AP")
        seqs.append(ph)
    return seqs


PHONE_KEYS = ("ctc_phone_confidence", "ctc_phone_centre_s", "ctc_phone_frames")


def test_task_ctc_score_batch_posteriors(task):
    batch, lens = _waves()
    waves = torch.from_numpy(batch).cuda()
    seqs = _transcripts(task)
    plain = task.ctc_score_batch(waves, seqs, lengths=lens)
    res = task.ctc_score_batch(waves, seqs, lengths=lens, posteriors=True)
    for b, (p, r) in enumerate(zip(plain, res)):
        assert set(p) == {"ctc_nll", "ctc_confidence", "ctc_phones", "ctc_phone_ids", "T"}     # today's keys
        assert set(r) - set(p) == set(PHONE_KEYS)
        for k in p:
            assert np.array_equal(np.asarray(p[k]), np.asarray(r[k])), k
        assert np.float64(p["ctc_nll"]).tobytes() == np.float64(r["ctc_nll"]).tobytes()
        alone = task.ctc_score_batch(waves[b:b + 1, :lens[b]], seqs[b:b + 1], posteriors=True)[0]
        L = len(task.decoder.ctc_targets(seqs[b]))
        for k in PHONE_KEYS:
            assert r[k].dtype == np.float64 and r[k].shape == (L,) and r[k].tobytes() == alone[k].tobytes(), (b, k)
        assert np.all(r["ctc_phone_confidence"] > 0) and np.all(r["ctc_phone_confidence"] <= 1)
        assert np.all(r["ctc_phone_frames"] >= 1 - 1e-3) and np.all(r["ctc_phone_centre_s"] >= 0)
        assert np.all(r["ctc_phone_centre_s"] < r["T"] * task.decoder.frame_length)
    feats, n_frames, wl = task.encode_batch(waves, lengths=lens)
    logits, _ = task.head_logits(feats, n_frames)
    Ts = [task.decoder.num_frames(v, logits.shape[1]) for v in wl]
    dev = task.decoder.ctc_batch(logits, Ts, seqs, host=False, posteriors=True)
    assert all(isinstance(dev[k], torch.Tensor) and dev[k].is_cuda for k in ("occ", "frames", "centre", "logp"))
    assert "occ" not in task.decoder.ctc_batch(logits, Ts, seqs, host=False)


def test_score_transcripts_cli_phones(task, tmp_path):
    import csv
    from hubertfa_amd import synth
    import hubertfa_amd.g2p as g2p_mod
    from hubertfa_amd.wav_io import read_wav, write_wav
    d = synth.synth_dictionary(n_words=40)
    dpath = tmp_path / "dict.txt"
    dpath.write_text("".join(f"{w}\t{' '.join(p)}\n" for w, p in d.items()))
    seg = tmp_path / "segments"
    seg.mkdir()
    for i, s in enumerate((0.9, 1.6, 1.2)):
        write_wav(seg / f"u{i}.wav", synth.synth_audio(int(s * 44100), 44100, seed=80 + i), 44100)
        (seg / f"u{i}.lab").write_text(synth.synth_lab(3 + i, d, seed=i))
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, os.path.join(REPO, "score_transcripts.py"), "-c", task.ckpt_path, "-f", str(seg), "-g",
           "Dictionary", "-d", str(dpath), "--batch_size", "4"]
    p = subprocess.run(cmd, env=env, cwd=REPO, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert not (seg / "ctc_phone_scores.csv").exists()
    without = (seg / "ctc_scores.csv").read_bytes()
    p = subprocess.run(cmd + ["--phones"], env=env, cwd=REPO, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert (seg / "ctc_scores.csv").read_bytes() == without
    order = [r["name"] for r in csv.DictReader(open(seg / "ctc_scores.csv", newline="", encoding="utf-8"))]
    rows = list(csv.DictReader(open(seg / "ctc_phone_scores.csv", newline="", encoding="utf-8")))
    assert list(rows[0]) == ["name", "index", "phone", "centre_s", "frames", "confidence"]
    g = g2p_mod.DictionaryG2P(dictionary=str(dpath))
    g.set_in_format("lab")
    data = {os.path.basename(str(w))[:-4]: ph for w, ph, _, _ in g.get_dataset(sorted(seg.rglob("*.wav")))}
    at = 0
    for name in order:                                   # files in ctc_scores.csv's order, phones in transcript order
        x, sr = read_wav(str(seg / (name + ".wav")))
        ph = data[name]
        want = task.ctc_score_batch(torch.from_numpy(np.ascontiguousarray(x[:1])).cuda(), [ph], posteriors=True)[0]
        nonsp = [q for q in ph if task.vocab["vocab"][q] != 0]
        for j, q in enumerate(nonsp):
            r = rows[at]
            at += 1
            assert (r["name"], int(r["index"]), r["phone"]) == (name, j, q)
            assert float(r["confidence"]) == want["ctc_phone_confidence"][j]
            assert float(r["centre_s"]) == want["ctc_phone_centre_s"][j]
            assert float(r["frames"]) == want["ctc_phone_frames"][j]
    assert at == len(rows)
