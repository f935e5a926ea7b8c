"""The full-label alignment-loss kernels (csrc/loss.hip: hfa_fa_frame_loss, hfa_fa_emd, hfa_fa_loss_reduce) and the layers
above them (ops.fa_loss, losses.FALoss, ForcedAlignmentTask.loss_batch, score_labels.py) against the float64 restatement
of tests/fa_loss_ref.py, which test_fa_loss.py holds to the reference's own modules.

Bars: losses and row_terms, relative error <= max(4 e_f32, 1e-6); gradient, absolute error <= max(4 e_f32, 1e-6 max|g|);
updated tables max(4 e_f32, 1e-6).  e_f32 is the reference's own float32 error where the fixture has it (the losses and
the gradient of the fixture cases) and the restatement run in float32 otherwise.  Every input comes from a seed that keeps
1e-5 from every bin edge and sign change (fa_loss_ref.draw_case; asserted before any device call), so bin indices and
counts must match exactly and no element is left out of any comparison.  Measured on MI355X: DESIGN.md §3.7.
"""
import contextlib
import csv
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import fa_loss_ref as ref
from test_fa_loss import load_case, restate, tables_after

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(autouse=True)
def _autograd_on():
    with torch.enable_grad():                            # (other tests' CLIs switch autograd off process-wide)
        yield


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def drawn(B, Tmax, V, Ts, lts, seed, ls=0.0, mask_live=None):
    """(inputs, float64 run, float32 run), computed once per shape and shared."""
    inp, o64 = ref.draw_case(B, Tmax, V, Ts, lts, seed, 10, ls, mask_live)
    assert ref.margins_ok(o64), o64["margin"]
    o32 = ref.run(inp["logits"], inp["T"], inp["label_type"], inp["ph_frame"], inp["ph_edge"], inp["ph_mask"],
                  inp["tables"], 10, ls, np.float32)
    return inp, o64, o32


def raw_run(inp, cap=0, coef=None, logits=None, grad=None, rows=None):
    """The three kernels through their ops on (a row subset of) a case; numpy results."""
    from hubertfa_amd import ops
    sel = slice(None) if rows is None else rows
    x = dev(inp["logits"][sel]) if logits is None else logits
    T, lt = dev(inp["T"][sel]), dev(inp["label_type"][sel])
    pf, pe, pm = dev(inp["ph_frame"][sel]), dev(inp["ph_edge"][sel]), dev(inp["ph_mask"][sel])
    tab = dev(ref.pack_tables(inp["tables"]))
    V = x.shape[2] - 2
    with (ops.grid_cap(cap) if cap else contextlib.nullcontext()):
        sums, fac = ops.fa_emd(x, T, lt, pe)
        if coef is None:
            terms, bins = ops.fa_frame_loss(x, T, lt, pf, pe, pm, tab, inp["num_bins"], inp["label_smoothing"])
            g = None
        else:
            terms, bins, g = ops.fa_frame_loss(x, T, lt, pf, pe, pm, tab, inp["num_bins"], inp["label_smoothing"],
                                               coef=dev(np.asarray(coef, np.float32)), emd_fac=fac, grad=grad)
        row_terms, losses, norm, hist = ops.fa_loss_reduce(T, lt, terms, bins, pf, sums, V, inp["num_bins"])
    torch.cuda.synchronize()
    out = dict(terms=terms, bins=bins, sums=sums, fac=fac, row_terms=row_terms, losses=losses, norm=norm, hist=hist)
    if g is not None:
        out["grad"] = g
    return {k: v.cpu().numpy() for k, v in out.items()}


def rel(got, want):
    return np.abs(got - want) / np.maximum(np.abs(want), 1e-300)


def check_case(tag, inp, o64, o32, e_loss=None, up=(1.0, 0.7, 1.3, 0.4)):
    """ops.fa_loss forward and backward (upstream ``up``) against the float64 run; prints every figure first."""
    from hubertfa_amd import ops
    x = dev(inp["logits"]).requires_grad_(True)
    losses, row_terms, norm, hist, _ = ops.fa_loss(x, inp["T"], inp["label_type"], inp["ph_frame"], inp["ph_edge"],
                                                   inp["ph_mask"], dev(ref.pack_tables(inp["tables"])),
                                                   inp["num_bins"], inp["label_smoothing"], stats=True)
    upv = np.asarray(up, np.float64)
    (losses * dev(upv)).sum().backward()
    torch.cuda.synchronize()
    g = x.grad.cpu().numpy().astype(np.float64)
    losses, row_terms, norm, hist = (t.detach().cpu().numpy() for t in (losses, row_terms, norm, hist))
    want_g = np.tensordot(upv, o64["grads"], axes=1)
    e32_g = np.abs(np.tensordot(upv, o32["grads"].astype(np.float64), axes=1) - want_g).max()
    live = o64["norm"] > 0
    e32_l = rel(o32["losses"].astype(np.float64), o64["losses"]) * live if e_loss is None else e_loss
    e32_r = rel(o32["row_terms"].astype(np.float64), o64["row_terms"]) * (o64["row_terms"] != 0)
    err_l = rel(losses, o64["losses"]) * live
    err_r = rel(row_terms, o64["row_terms"]) * (o64["row_terms"] != 0)
    err_g = np.abs(g - want_g).max()
    bar_g = max(4 * e32_g, 1e-6 * np.abs(want_g).max())
    print(f"FA_LOSS {tag}: loss rel err {err_l} (e_f32 {e32_l}); row_terms rel err max {err_r.max():.3g} (e_f32 max "
          f"{e32_r.max():.3g}); grad abs err {err_g:.3g} (e_f32 {e32_g:.3g}, max|g| {np.abs(want_g).max():.3g}, bar "
          f"{bar_g:.3g})")
    assert np.array_equal(norm, o64["norm"])
    assert np.array_equal(hist, np.concatenate([o64["hist"][n] for n in ref.TABLES]))
    assert np.all(err_l <= np.maximum(4 * e32_l, 1e-6))
    assert np.all(losses[~live] == 0)
    assert np.all(err_r <= np.maximum(4 * e32_r, 1e-6))
    assert np.all(row_terms[o64["row_terms"] == 0] == 0)
    assert err_g <= bar_g
    assert np.all(g[:, :, 1] == 0)
    assert np.all(g[want_g == 0] == 0)                    # rows / frames / dead classes that take no part
    return dict(loss=err_l, rows=err_r.max(), grad=err_g)


# ---- accuracy --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("ls0", "ls01", "mixed"))
def test_fixture_cases(name):
    fx = np.load(os.path.join(HERE, "golden", "fa_loss.npz"))
    inp = load_case(fx, name)
    o64 = restate(inp)
    assert ref.margins_ok(o64), o64["margin"]
    o32 = ref.run(inp["logits"], inp["T"], inp["label_type"], inp["ph_frame"], inp["ph_edge"], inp["ph_mask"],
                  inp["tables"], inp["num_bins"], inp["label_smoothing"], np.float32)
    p = name + "_"
    e_loss = rel(fx[p + "f32_losses"][:4], fx[p + "f64_losses"][:4])      # the reference's own float32 error
    check_case(name, inp, o64, o32, e_loss=e_loss)
    raw = raw_run(inp)
    assert np.array_equal(raw["bins"], o64["bins"])
    # the reference's float32 gradient error (autograd) sets the same bar for the four-term gradient
    from hubertfa_amd import ops
    x = dev(inp["logits"]).requires_grad_(True)
    w = inp["weights"]
    losses = ops.fa_loss(x, inp["T"], inp["label_type"], inp["ph_frame"], inp["ph_edge"], inp["ph_mask"],
                         dev(ref.pack_tables(inp["tables"])), inp["num_bins"], inp["label_smoothing"])
    (losses * dev(w[:4])).sum().backward()
    e_ref = np.abs(fx[p + "f32_grad4"] - fx[p + "f64_grad4"]).max()
    err = np.abs(x.grad.cpu().numpy() - fx[p + "f64_grad4"]).max()
    print(f"FA_LOSS {name}: grad4 abs err {err:.3g}, the reference's float32 {e_ref:.3g}")
    assert err <= max(4 * e_ref, 1e-6 * np.abs(fx[p + "f64_grad4"]).max())


def test_config2_geometry():
    check_case("B4_T861_V63", *drawn(4, 861, 63, (861, 700, 861, 433), (2, 2, 3, 2), 21, 0.08))


@pytest.mark.parametrize("V", (2, 63, 64, 65, 129, 1024))
def test_class_counts(V):
    inp, o64, o32 = drawn(2, 9, V, (9, 5), (2, 2), 30 + V, 0.1)
    check_case(f"V{V}", inp, o64, o32)
    assert np.array_equal(raw_run(inp)["bins"], o64["bins"])


def test_short_rows():
    inp, o64, o32 = drawn(3, 3, 5, (1, 2, 3), (2, 2, 2), 41)
    check_case("T123", inp, o64, o32)
    one = raw_run(inp, rows=slice(0, 1), coef=(1, 1, 1, 1))      # T = 1: no difference pair, the term is exactly 0
    assert one["losses"][3] == 0 and one["norm"][3] == 0 and np.all(one["terms"][:, :, 2] == 0)
    assert np.all(one["bins"][0, 0, 3:] == -1)


def test_scan_tiles():
    Ts = (255, 256, 257, 1023, 1025, 3000)
    inp, o64, o32 = drawn(6, 3000, 4, Ts, (2,) * 6, 51)
    check_case("scan", inp, o64, o32)
    raw = raw_run(inp)
    for b, T in enumerate(Ts):                                   # the sign counts are integers: exact
        x0 = inp["logits"][b, :T, 0].astype(np.float64)
        d = 1 / (1 + np.exp(-x0)) - inp["ph_edge"][b, :T]
        F, R = np.cumsum(d), np.cumsum(d[::-1])[::-1]
        fac = np.cumsum(np.sign(F)[::-1])[::-1] + (3000 - T) * np.sign(F[-1]) + np.cumsum(np.sign(R))
        assert np.array_equal(raw["fac"][b, :T], fac.astype(np.int32)), T
        assert np.all(raw["fac"][b, T:] == 0)
        want = np.abs(F).sum(), np.abs(R).sum(), abs(F[-1])
        assert np.all(rel(raw["sums"][b], np.asarray(want)) <= 1e-6), (T, raw["sums"][b], want)


def test_no_full_label_row():
    inp, o64, _ = drawn(3, 40, 7, (40, 33, 12), (0, 1, 1), 61)
    from hubertfa_amd import ops
    x = dev(inp["logits"]).requires_grad_(True)
    losses = ops.fa_loss(x, inp["T"], inp["label_type"], inp["ph_frame"], inp["ph_edge"], inp["ph_mask"],
                         dev(ref.pack_tables(inp["tables"])))
    losses.sum().backward()
    assert losses.dtype == torch.float64 and np.all(losses.detach().cpu().numpy() == 0)
    assert np.all(x.grad.cpu().numpy() == 0)
    assert np.all(raw_run(inp)["hist"] == 0)


def test_single_live_class():
    inp, o64, o32 = drawn(2, 50, 9, (50, 31), (2, 2), 71, 0.08, 1)
    assert np.all(inp["ph_mask"].sum(axis=1) == 1)
    check_case("one_live_class", inp, o64, o32)


# ---- layout ----------------------------------------------------------------------------------------------------------
def test_strided_views_and_nan_hygiene():
    inp, o64, _ = drawn(4, 37, 12, (37, 20, 30, 9), (2, 1, 3, 0), 81, 0.1, 5)
    B, Tmax, C = inp["logits"].shape
    coef = (0.3, 1.1, 0.7, 0.9)
    plain = raw_run(inp, coef=coef)
    big = torch.full((B, Tmax + 6, C + 9), float("nan"), device="cuda")
    view = big[:, :Tmax, 3:3 + C]
    x = inp["logits"].copy()
    for b in range(B):
        x[b, inp["T"][b]:] = np.nan                                   # past each row's T
        if inp["label_type"][b] < 2:
            x[b] = np.nan                                             # rows that take no part
        x[b, :, 2:][:, inp["ph_mask"][b] == 0] = np.nan               # dead classes
    x[:, :, 1] = np.nan                                               # the CTC blank is never read
    view.copy_(dev(x))
    assert not view.is_contiguous()
    sentinel = -12345.0
    gbig = torch.full((B, Tmax + 2, C + 5), sentinel, device="cuda")
    gview = gbig[:, :Tmax, 2:2 + C]
    got = raw_run(inp, coef=coef, logits=view, grad=gview)
    for k in ("terms", "bins", "sums", "fac", "row_terms", "losses", "norm", "hist"):
        assert np.array_equal(got[k], plain[k]), k
    g = gbig.cpu().numpy()
    assert np.array_equal(g[:, :Tmax, 2], plain["grad"][:, :, 0])
    assert np.array_equal(g[:, :Tmax, 4:2 + C], plain["grad"][:, :, 2:])
    keep = np.ones(g.shape, bool)
    keep[:, :Tmax, 2] = False
    keep[:, :Tmax, 4:2 + C] = False
    assert np.all(g[keep] == sentinel)                                # column 1 and everything outside the view
    assert np.all(np.isfinite(plain["grad"]))


# ---- determinism -----------------------------------------------------------------------------------------------------
def test_same_bits_alone_in_a_batch_and_under_grid_caps():
    inp, _, _ = drawn(3, 300, 17, (300, 257, 64), (2, 2, 3), 91, 0.1)
    coef = (0.5, 0.25, 2.0, 1.0)
    base = raw_run(inp, coef=coef)
    for cap in (1, 7, 256):
        got = raw_run(inp, cap=cap, coef=coef)
        for k in base:
            assert np.array_equal(got[k], base[k]), (cap, k)
    for b in range(3):
        one = raw_run(inp, coef=coef, rows=slice(b, b + 1))
        for k in ("terms", "bins", "sums", "fac", "row_terms", "grad"):
            assert np.array_equal(one[k][0], base[k][b]), (b, k)


# ---- autograd --------------------------------------------------------------------------------------------------------
def test_backward_with_a_random_upstream():
    inp, o64, o32 = drawn(3, 120, 20, (120, 77, 101), (2, 0, 2), 101, 0.1)
    up = np.random.default_rng(5).uniform(-2, 2, 4)
    check_case("upstream", inp, o64, o32, up=tuple(up))


@pytest.mark.parametrize("valid", (False, True))
def test_faloss_five_terms(valid):
    """FALoss on the fixture's mixed batch: the five losses, total(...).backward() through all of them (the CTC's
    column 1 included) and the tables after the call against the restatement."""
    from hubertfa_amd.losses import FALoss
    fx = np.load(os.path.join(HERE, "golden", "fa_loss.npz"))
    inp = load_case(fx, "mixed")
    o64 = restate(inp)
    assert ref.margins_ok(o64), o64["margin"]
    loss = FALoss(20, inp["num_bins"], inp["alpha"], inp["label_smoothing"], weights=inp["weights"])
    for n in loss.tables:
        loss.tables[n] = dev(inp["tables"][n])
    x = dev(inp["logits"]).requires_grad_(True)
    seqs = [inp["ph_id_seq"][b, :inp["L"][b]] for b in range(len(inp["L"]))]
    losses = loss(x, inp["T"], inp["ph_frame"], inp["ph_edge"], seqs, inp["L"], inp["ph_mask"], inp["label_type"],
                  valid=valid)
    loss.total(losses).backward()
    torch.cuda.synchronize()
    got = np.asarray([float(v.detach()) for v in losses])
    want = fx["mixed_f64_losses"]
    e32 = rel(fx["mixed_f32_losses"], want)
    print("FA_LOSS FALoss: rel err", rel(got, want), "the reference's float32", e32)
    assert np.all(rel(got, want) <= np.maximum(4 * e32, 1e-6))
    g = x.grad.cpu().numpy()
    e32_g = np.abs(fx["mixed_f32_grad"] - fx["mixed_f64_grad"]).max()
    err = np.abs(g - fx["mixed_f64_grad"]).max()
    print(f"FA_LOSS FALoss: grad abs err {err:.3g}, the reference's float32 {e32_g:.3g}")
    assert err <= max(4 * e32_g, 1e-6 * np.abs(fx["mixed_f64_grad"]).max())
    assert np.abs(g[:, :, 1]).max() > 0                               # the CTC term reached its blank column
    after = {n: inp["tables"][n].astype(np.float64) for n in loss.tables} if valid else tables_after(inp, o64)
    for n, t in loss.tables.items():
        e_ref = 0.0 if valid else np.abs(fx["mixed_f32_after." + n] - fx["mixed_f64_after." + n]).max()
        err = np.abs(t.cpu().numpy().astype(np.float64) - after[n]).max()
        print(f"FA_LOSS FALoss: table {n} err {err:.3g} (the reference's float32 {e_ref:.3g})")
        assert err <= max(4 * e_ref, 1e-6), n


# ---- task and CLI ----------------------------------------------------------------------------------------------------
LOSS_CONFIG = {"losses": {"weights": [8.0, 0.1, 0.01, 0.1, 2.0]},          # the reference's train_config weights
               "function": {"num_bins": 10, "alpha": 0.999, "label_smoothing": 0.0}}


def _write_csv(path, items):
    with open(path, "w", newline="") as fh:
        wr = csv.writer(fh)
        wr.writerow(["name", "ph_seq", "ph_dur"])
        for it in items:
            wr.writerow([it["name"], " ".join(it["ph_seq"]), " ".join(f"{v:.6f}" for v in it["ph_dur"])])


def _pad(waves):
    n = max(len(w) for w in waves)
    out = np.zeros((len(waves), n), np.float32)
    for i, w in enumerate(waves):
        out[i, :len(w)] = w
    return out, [len(w) for w in waves]


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """synth_checkpoint (with the reference's loss weights), three synthetic waves of different lengths, and two label
    sets: ``items`` (equal durations) and ``own`` (the model's own alignment of each file, which is what
    transcriptions.csv holds: the labels this model agrees with most)."""
    from hubertfa_amd.task import ForcedAlignmentTask, synth_checkpoint
    from hubertfa_amd.wav_io import write_wav
    d = tmp_path_factory.mktemp("labelled")
    ckpt = str(d / "model.ckpt")
    ck = synth_checkpoint(None)
    ck["hyper_parameters"]["loss_config"] = LOSS_CONFIG
    torch.save(ck, ckpt)
    task = ForcedAlignmentTask.load_from_checkpoint(ckpt)
    sr = task.melspec_config["sample_rate"]
    names = [p for p in task.vocab["vocab"] if p not in ("SP", "AP")]
    r = np.random.default_rng(3)
    items, waves = [], []
    for i, secs in enumerate((1.3, 0.9, 1.1)):
        n = int(secs * sr)
        w = (np.round(r.standard_normal(n) * 0.1 * 32768) / 32768).astype(np.float32)   # what the 16-bit file holds
        k = 5 + i
        phones = ["SP"] + [names[(3 * i + j) % len(names)] for j in range(k - 2)] + ["SP"]
        write_wav(str(d / f"u{i}.wav"), w, sr)
        waves.append(w)
        items.append(dict(name=f"u{i}", ph_seq=phones, ph_dur=[secs / k] * k))
    padded, lengths = _pad(waves)
    own = []
    for it, a, w in zip(items, task.align_batch(task.upload(padded), [it["ph_seq"] for it in items], lengths=lengths),
                        waves):
        ph, du, cur = [], [], 0.0
        for p, (s, e) in zip(a["ph_seq"], a["ph_intervals"]):
            if s > cur + 1e-9:
                ph.append("SP")
                du.append(float(s - cur))
            ph.append(str(p))
            du.append(float(e - s))
            cur = float(e)
        if cur < len(w) / sr - 1e-9:
            ph.append("SP")
            du.append(len(w) / sr - cur)
        own.append(dict(name=it["name"], ph_seq=ph, ph_dur=[float(f"{v:.6f}") for v in du]))   # as the CSV holds them
    _write_csv(d / "transcriptions.csv", own)
    return dict(dir=str(d), ckpt=ckpt, task=task, items=items, own=own, waves=waves, sr=sr)


def test_loss_batch_matches_faloss_and_rows_alone(corpus):
    from hubertfa_amd.labels import make_ph_data
    from hubertfa_amd.losses import FALoss
    task, items = corpus["task"], corpus["items"]
    waves, lengths = _pad(corpus["waves"])
    res = task.loss_batch(task.upload(waves), items, lengths=lengths)
    assert len(res["rows"]) == 3 and res["losses"].shape == (5,)
    # the same losses from head_logits computed separately and FALoss called by hand
    feats, n_frames, wl = task.encode_batch(task.upload(waves), None, lengths)
    logits, _ = task.head_logits(feats, n_frames)
    Ts = [task.decoder.num_frames(w, logits.shape[1]) for w in wl]
    V = task.vocab["vocab_size"]
    fl = task.melspec_config["hop_length"] / task.melspec_config["sample_rate"]
    Tmax = max(Ts)
    pf, pe, pm, seqs = np.zeros((3, Tmax), np.int32), np.zeros((3, Tmax), np.float32), np.zeros((3, V), np.int32), []
    for b, it in enumerate(items):
        ids = [task.vocab["vocab"][p] for p in it["ph_seq"]]
        s, e, f, m, _ = make_ph_data(task.vocab, Ts[b], 2, ids, it["ph_dur"], fl)
        pf[b, :Ts[b]], pe[b, :Ts[b]], pm[b] = f, e, m
        seqs.append(s)
    loss = FALoss.from_checkpoint({}, LOSS_CONFIG, vocab_size=V)
    by_hand = loss(logits[:, :Tmax], Ts, pf, pe, seqs, [len(s) for s in seqs], pm, [2, 2, 2], valid=True)
    assert np.array_equal(res["losses"], np.asarray([float(v.detach()) for v in by_hand]))
    assert all(np.isfinite(res["losses"])) and res["losses"][0] > 0
    for b in range(3):                                            # a row alone gives the same row_terms
        one = task.loss_batch(task.upload(corpus["waves"][b][None]), [items[b]])["rows"][0]
        for k in ref.NAMES[:4] + ("ctc_nll", "frames"):
            assert one[k] == res["rows"][b][k], (b, k)


def _score(ckpt, folder):
    run = subprocess.run([sys.executable, os.path.join(REPO, "score_labels.py"), "-c", ckpt, "-f", str(folder)],
                         capture_output=True, text=True, cwd=REPO)
    assert run.returncode == 0, run.stderr[-2000:]
    out = list(csv.DictReader(open(os.path.join(folder, "label_losses.csv"))))
    assert out[-1]["name"] == "MEAN"
    return out[:-1], out[-1]


def test_score_labels_cli_ranks_the_shifted_file_first(corpus, tmp_path):
    """One line per file, worst first, each the row loss_batch gives; the file whose labels the model agrees with most
    goes to the top once its labels slide 300 ms late (0.3 s of SP in front, 0.3 s cut off the end)."""
    import shutil
    task = corpus["task"]
    waves, lengths = _pad(corpus["waves"])
    rows = task.loss_batch(task.upload(waves), corpus["own"], lengths=lengths)["rows"]
    w = LOSS_CONFIG["losses"]["weights"]
    before = {it["name"]: sum(wk * r[k] for wk, k in zip(w, ref.NAMES[:4])) for it, r in zip(corpus["own"], rows)}
    best = min(before, key=before.get)
    d = tmp_path / "c"
    shutil.copytree(corpus["dir"], d)
    shifted = []
    for it in corpus["own"]:
        it = dict(it, ph_seq=list(it["ph_seq"]), ph_dur=list(it["ph_dur"]))
        if it["name"] == best:
            it["ph_seq"].insert(0, "SP")
            it["ph_dur"].insert(0, 0.3)
            rem = 0.3
            while rem > 1e-9:
                cut = min(rem, it["ph_dur"][-1])
                it["ph_dur"][-1] -= cut
                rem -= cut
                if it["ph_dur"][-1] <= 1e-9:
                    it["ph_dur"].pop()
                    it["ph_seq"].pop()
        shifted.append(it)
    _write_csv(d / "transcriptions.csv", shifted)
    files, mean = _score(corpus["ckpt"], d)
    print("FA_LOSS score_labels: before", before, "after", [(r["name"], r["total"]) for r in files])
    assert sorted(r["name"] for r in files) == ["u0", "u1", "u2"]
    assert set(ref.NAMES[:4]) | {"total", "ctc_nll", "frames"} <= set(files[0])
    totals = [float(r["total"]) for r in files]
    assert totals == sorted(totals, reverse=True)
    assert abs(float(mean["total"]) - sum(totals) / 3) <= 1e-9 * abs(float(mean["total"]))
    assert files[0]["name"] == best and totals[0] > before[best]
    for r in files[1:]:                                            # the untouched files: loss_batch's rows
        own = rows[[it["name"] for it in corpus["own"]].index(r["name"])]
        assert float(r["total"]) == before[r["name"]] and int(r["frames"]) == own["frames"]
        assert all(float(r[k]) == own[k] for k in ref.NAMES[:4] + ("ctc_nll",))
