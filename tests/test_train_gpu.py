"""Head fine-tuning on the device (csrc/train.hip: hfa_wgrad_f32, hfa_adamw_f32; ops.wgrad / adamw_step / head_linear;
hubertfa_amd.train.HeadTrainer; finetune_head.py) against float64.

Bars, as DESIGN.md §3.5-§3.7: absolute error <= max(4 e_f32, 1e-6 max|.|) for arrays, relative max(4 e_f32, 1e-6) for
scalars, where e_f32 is the error of the float32 CPU form of the same computation against float64 (numpy's einsum,
torch.optim.AdamW on float32 tensors, tests/train_ref.py run in float32), never anything from the code under test.  Every
figure is printed before it is asserted.  Measured on MI355X: DESIGN.md §3.8.
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import fa_loss_ref as ref
import train_ref
from test_fa_loss import load_case

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
SENTINEL = -12345.0


@pytest.fixture(autouse=True)
def _autograd_on():
    with torch.enable_grad():                            # (other tests' CLIs switch autograd off process-wide)
        yield


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def chunk_rows():
    from hubertfa_amd import _lib, ops  # noqa: F401
    return int(_lib.lib().hfa_wgrad_chunk_rows())


# ---- hfa_wgrad_f32 -----------------------------------------------------------------------------------------------------
def _lens_of(token, chunk):
    return {"1": 1, "2": 2, "chunk-1": chunk - 1, "chunk": chunk, "chunk+1": chunk + 1, "3000": 3000}[token]


def _wgrad_reference(G, X, lens):
    """float64 and float32 einsum of the same float32 inputs over the rows t < lens[b]."""
    live = np.arange(G.shape[1])[None, :] < np.asarray(lens)[:, None]
    Gm, Xm = np.where(live[:, :, None], G, 0).astype(np.float32), np.where(live[:, :, None], X, 0).astype(np.float32)
    dW = np.einsum("btn,btc->nc", Gm.astype(np.float64), Xm.astype(np.float64))
    db = Gm.astype(np.float64).sum(axis=(0, 1))
    dW32, db32 = np.einsum("btn,btc->nc", Gm, Xm), Gm.sum(axis=(0, 1), dtype=np.float32)
    ss = (dW ** 2).sum() + (db ** 2).sum()
    ss32 = float((dW32 ** 2).sum(dtype=np.float32) + (db32 ** 2).sum(dtype=np.float32))
    return dW, db, ss, dW32.astype(np.float64), db32.astype(np.float64), ss32


def _wgrad_run(G, X, lens, cap=0):
    """hfa_wgrad_f32 through ops.wgrad on views into padded buffers: NaN in every padding row and column of G and X,
    sentinels around dW, db, sumsq and the workspace.  Returns the results and whether every band is intact."""
    import contextlib
    from hubertfa_amd import _lib, ops
    B, Tmax, N = G.shape
    C = X.shape[2]
    Gn, Xn = G.copy(), X.copy()
    for b in range(B):
        Gn[b, lens[b]:], Xn[b, lens[b]:] = np.nan, np.nan
    Gb = torch.full((B, Tmax + 2, N + 5), float("nan"), device="cuda")
    Xb = torch.full((B, Tmax + 1, C + 9), float("nan"), device="cuda")
    Gv, Xv = Gb[:, :Tmax, 2:2 + N], Xb[:, :Tmax, 3:3 + C]
    Gv.copy_(dev(Gn))
    Xv.copy_(dev(Xn))
    Wb = torch.full((N + 2, C + 7), SENTINEL, device="cuda")
    bb = torch.full((N + 6,), SENTINEL, device="cuda")
    sb = torch.full((3,), SENTINEL, dtype=torch.float64, device="cuda")
    nbytes = int(_lib.lib().hfa_wgrad_workspace_bytes(B, Tmax, N, C))
    wb = torch.full((nbytes + 128,), 0xA5, dtype=torch.uint8, device="cuda")
    dW, db, ss = Wb[1:1 + N, 4:4 + C], bb[3:3 + N], sb[1]
    with (ops.grid_cap(cap) if cap else contextlib.nullcontext()):
        ops.wgrad(Gv, Xv, dev(np.asarray(lens, np.int32)), dW, db, ss, wb[64:64 + nbytes])
    torch.cuda.synchronize()
    out = (dW.cpu().numpy().copy(), db.cpu().numpy().copy(), float(ss))
    Wh, bh, sh, wh = Wb.cpu().numpy(), bb.cpu().numpy(), sb.cpu().numpy(), wb.cpu().numpy()
    keep = np.ones(Wh.shape, bool)
    keep[1:1 + N, 4:4 + C] = False
    intact = bool(np.all(Wh[keep] == SENTINEL) and np.all(bh[:3] == SENTINEL) and np.all(bh[3 + N:] == SENTINEL) and
                  sh[0] == SENTINEL and sh[2] == SENTINEL and np.all(wh[:64] == 0xA5) and
                  np.all(wh[64 + nbytes:] == 0xA5))
    return out, intact


def _wgrad_check(tag, B, Tmax, N, C, lens, seed):
    r = np.random.default_rng(seed)
    X = r.standard_normal((B, Tmax, C)).astype(np.float32)
    G0 = r.standard_normal((B, Tmax, N)).astype(np.float32)
    for scale in (1e-6, 1.0):                             # the losses' 1 / sum T normalisers put G around 1e-6
        G = (G0 * np.float32(scale)).astype(np.float32)
        dW, db, ss, dW32, db32, ss32 = _wgrad_reference(G, X, lens)
        (gW, gb, gs), intact = _wgrad_run(G, X, lens)
        eW, eb = np.abs(dW32 - dW).max(), np.abs(db32 - db).max()
        errW, errb = np.abs(gW - dW).max(), np.abs(gb - db).max()
        barW, barb = max(4 * eW, 1e-6 * np.abs(dW).max()), max(4 * eb, 1e-6 * np.abs(db).max())
        es = abs(ss32 - ss) / ss if ss else 0.0
        errs = abs(gs - ss) / ss if ss else abs(gs)
        print(f"WGRAD {tag} x{scale:g}: dW err {errW:.3g} (e_f32 {eW:.3g}, bar {barW:.3g}, max {np.abs(dW).max():.3g}); "
              f"db err {errb:.3g} (e_f32 {eb:.3g}, bar {barb:.3g}); sumsq rel err {errs:.3g} (e_f32 {es:.3g})")
        assert np.all(np.isfinite(gW)) and np.all(np.isfinite(gb)) and np.isfinite(gs)     # no padding NaN came through
        assert intact
        assert errW <= barW and errb <= barb
        assert errs <= max(4 * es, 1e-6)
        again, _ = _wgrad_run(G, X, lens)
        same = [again]
        for cap in (8, 3):                                # (3: fewer workgroups than the 8 chunks of the ragged batch)
            capped, ok = _wgrad_run(G, X, lens, cap=cap)
            assert ok
            same.append(capped)
        for a in same:
            assert np.array_equal(a[0], gW) and np.array_equal(a[1], gb) and a[2] == gs


@pytest.mark.parametrize("C", (8, 32, 192, 200))
@pytest.mark.parametrize("N", (1, 3, 16, 17, 65, 67))
def test_wgrad_widths_on_a_ragged_batch(N, C):
    chunk = chunk_rows()
    _wgrad_check(f"N{N}_C{C}", 4, chunk + 3, N, C, (chunk + 1, 0, 37, 2), 100 * N + C)


@pytest.mark.parametrize("token", ("1", "2", "chunk-1", "chunk", "chunk+1", "3000"))
def test_wgrad_row_counts(token):
    T = _lens_of(token, chunk_rows())
    _wgrad_check(f"T{token}", 1, T + 1, 65, 192, (T,), 7 + T)


def test_wgrad_no_live_row_gives_zeros():
    (gW, gb, gs), intact = _wgrad_run(np.ones((2, 5, 3), np.float32), np.ones((2, 5, 8), np.float32), (0, 0))
    assert intact and np.all(gW == 0) and np.all(gb == 0) and gs == 0


# ---- hfa_adamw_f32 -----------------------------------------------------------------------------------------------------
STEPS, MAX_LR, WD = 25, 3e-2, 0.1


@functools.lru_cache(maxsize=None)
def _adamw_case(n):
    """25 steps of clip_grad_norm_ + torch.optim.AdamW under one_cycle's lr / beta1 on the CPU, float64 and float32, from
    float32 gradients with exact zeros and 1e-9 entries and a norm that crosses max_norm."""
    from hubertfa_amd.schedulers import one_cycle
    r = np.random.default_rng(n)
    p0 = r.standard_normal(n).astype(np.float32)
    grads = []
    for k in range(STEPS):
        g = (r.standard_normal(n) * (0.3 if k % 3 else 3.0)).astype(np.float32)
        i = np.arange(n)
        g[i % 7 == 3] = 0.0
        g[i % 7 == 5] = 1e-9
        grads.append(g)
    norms = [float(np.sqrt((g.astype(np.float64) ** 2).sum())) for g in grads]
    max_norm = float(np.sqrt(min(norms) * max(norms)))
    runs = {}
    for dt in (torch.float64, torch.float32):
        p = torch.nn.Parameter(torch.from_numpy(p0).to(dt).clone())      # (a float32 tensor would share p0's memory)
        opt = torch.optim.AdamW([p], lr=1e-3, weight_decay=WD)
        for k in range(STEPS):
            lr, b1 = one_cycle(k, STEPS, MAX_LR)
            opt.param_groups[0]["lr"], opt.param_groups[0]["betas"] = lr, (b1, 0.999)
            p.grad = torch.from_numpy(grads[k]).to(dt).clone()        # (clip_grad_norm_ scales it in place)
            torch.nn.utils.clip_grad_norm_([p], max_norm)
            opt.step()
        st = opt.state[p]
        runs[dt] = tuple(t.detach().double().numpy() for t in (p, st["exp_avg"], st["exp_avg_sq"]))
    clipped = [nm + 1e-6 > max_norm for nm in norms]
    return p0, grads, norms, max_norm, clipped, runs[torch.float64], runs[torch.float32]


@pytest.mark.parametrize("n", (1, 3, 255, 256, 257, 12545))
def test_adamw_25_steps(n):
    from hubertfa_amd import ops
    from hubertfa_amd.schedulers import one_cycle
    p0, grads, norms, max_norm, clipped, want, f32 = _adamw_case(n)
    assert any(clipped) and not all(clipped), (norms, max_norm)        # the clip is active on some steps, idle on others
    p = dev(p0)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    skipped = torch.zeros(1, dtype=torch.int32, device="cuda")
    for k in range(STEPS):
        lr, b1 = one_cycle(k, STEPS, MAX_LR)
        ss = dev(np.asarray((grads[k].astype(np.float64) ** 2).sum()))
        ops.adamw_step(p, m, v, dev(grads[k]), ss, skipped, lr=lr, beta1=b1, weight_decay=WD, step=k + 1,
                       max_norm=max_norm)
    torch.cuda.synchronize()
    for name, got, w, e in zip("pmv", (p, m, v), want, f32):
        got = got.cpu().numpy().astype(np.float64)
        e32, err = np.abs(e - w).max(), np.abs(got - w).max()
        bar = max(4 * e32, 1e-6 * np.abs(w).max())
        print(f"ADAMW n={n} {name}: err {err:.3g} (e_f32 {e32:.3g}, bar {bar:.3g}, max {np.abs(w).max():.3g})")
        assert err <= bar
    assert int(skipped) == 0
    # a non-finite norm: the step is skipped, bit for bit, and counted
    before = [t.clone() for t in (p, m, v)]
    for bad in (float("inf"), float("nan")):
        ops.adamw_step(p, m, v, dev(grads[0]), dev(np.asarray(bad)), skipped, lr=1e-2, beta1=0.9, weight_decay=WD,
                       step=STEPS + 1, max_norm=max_norm)
    assert all(torch.equal(a, b) for a, b in zip(before, (p, m, v)))
    assert int(skipped) == 2
    ops.adamw_step(p, m, v, dev(grads[0]), dev(np.asarray(np.inf)), skipped[:1].zero_(), lr=1e-2, step=1)
    assert int(skipped) == 1


# ---- ops.head_linear ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _head_case():
    """The fixture's mixed batch under a random head: y [B, Tmax, 32] and W [22, 32] from the first seed whose logits
    keep the margins; the restatement's d total / d W, d total / d b in float64 and float32."""
    fx = np.load(os.path.join(HERE, "golden", "fa_loss.npz"))
    inp = load_case(fx, "mixed")
    B, Tmax, NC = inp["logits"].shape
    C = 32
    seqs = [inp["ph_id_seq"][b, :inp["L"][b]] for b in range(B)]
    w = np.asarray(inp["weights"], np.float64)
    for seed in range(200):
        r = np.random.default_rng(500 + seed)
        y = r.standard_normal((B, Tmax, C)).astype(np.float32)
        W = (r.standard_normal((NC, C)) * 0.35).astype(np.float32)
        b = (r.standard_normal(NC) * 0.5).astype(np.float32)
        res = {}
        for dt in (np.float64, np.float32):
            logits = (y.astype(dt) @ W.astype(dt).T + b.astype(dt)).astype(dt)
            out = ref.run(logits, inp["T"], inp["label_type"], inp["ph_frame"], inp["ph_edge"], inp["ph_mask"],
                          inp["tables"], inp["num_bins"], inp["label_smoothing"], dt)
            if dt is np.float64 and (not ref.margins_ok(out) or
                                     train_ref.ctc_margin(logits, inp["T"], inp["label_type"], seqs) < 1e-5):
                break
            term = ref.ctc_term if dt is np.float64 else train_ref.ctc_term32     # (float32: the CTC recursions too)
            ctc = term(logits, inp["T"], inp["label_type"], seqs, inp["tables"][ref.CTC_TABLE])
            G = np.tensordot(w[:4].astype(dt), out["grads"], axes=1) + dt(w[4]) * ctc[1].astype(dt)
            res[dt] = (np.einsum("btn,btc->nc", G, y.astype(dt)).astype(np.float64),
                       G.sum(axis=(0, 1), dtype=dt).astype(np.float64))
        if len(res) == 2:
            return inp, seqs, y, W, b, res[np.float64], res[np.float32]
    raise RuntimeError("no seed keeps the margin")


@pytest.mark.parametrize("path", ("split", "f32"))
def test_head_linear_gradient(path):
    from hubertfa_amd import ops
    from hubertfa_amd.losses import FALoss
    inp, seqs, y, W, b, (dW, db), (dW32, db32) = _head_case()         # (CPU, before any device call)
    N, C = W.shape
    n4 = -(-N // 4) * 4
    loss = FALoss(N - 2, inp["num_bins"], inp["alpha"], inp["label_smoothing"], weights=inp["weights"])
    for n in loss.tables:
        loss.tables[n] = dev(inp["tables"][n])
    Wp, bp = torch.zeros((n4, C), device="cuda"), torch.zeros(n4, device="cuda")
    Wp[:N], bp[:N] = dev(W), dev(b)
    Wp.requires_grad_()
    bp.requires_grad_()
    yn = y.copy()
    for r, T in enumerate(inp["T"]):
        yn[r, T:] = np.nan                                            # padding frames never reach the gradient
    Ws = ops.split(Wp.detach(), flag=torch.zeros(1, dtype=torch.int32, device="cuda")) if path == "split" else None
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    logits = ops.head_linear(dev(yn), None, Wp, Ws, bp, dev(inp["T"].astype(np.int32)), flag=flag)
    assert logits.shape == (y.shape[0], y.shape[1], n4)
    losses = loss(logits[:, :, :N], inp["T"], inp["ph_frame"], inp["ph_edge"], seqs, inp["L"], inp["ph_mask"],
                  inp["label_type"], valid=True)
    loss.total(losses).backward()
    torch.cuda.synchronize()
    gW, gb = Wp.grad.cpu().numpy().astype(np.float64), bp.grad.cpu().numpy().astype(np.float64)
    eW, eb = np.abs(dW32 - dW).max(), np.abs(db32 - db).max()
    errW, errb = np.abs(gW[:N] - dW).max(), np.abs(gb[:N] - db).max()
    barW, barb = max(4 * eW, 1e-6 * np.abs(dW).max()), max(4 * eb, 1e-6 * np.abs(db).max())
    print(f"HEAD_LINEAR {path}: dW err {errW:.3g} (e_f32 {eW:.3g}, bar {barW:.3g}, max {np.abs(dW).max():.3g}); db err "
          f"{errb:.3g} (e_f32 {eb:.3g}, bar {barb:.3g})")
    assert errW <= barW and errb <= barb
    assert np.all(gW[N:] == 0) and np.all(gb[N:] == 0)               # the padded head's padding rows


# ---- HeadTrainer -------------------------------------------------------------------------------------------------------
# (one ramp only, on a light term: a heavy term's weight growing with the step would hide the descent in the total)
LOSS_CONFIG = {"losses": {"weights": [8.0, 0.1, 0.01, 0.1, 2.0],
                          "enable_RampUpScheduler": [False, False, False, True, False]},
               "function": {"num_bins": 10, "alpha": 0.999, "label_smoothing": 0.08}}
OPT_CONFIG = {"lr": {"backbone": 0.0, "head": 2e-2}, "weight_decay": 0.1, "total_steps": 8,
              "freeze": {"backbone": True, "head": False}}
CLIP, HEAD_SEED, NEW_V, HIDDEN = 0.5, 3, 20, 192
ROW_T, ROW_TYPES = (40, 57, 200, 73, 64, 90), (2, 1, 2, 2, 1, 2)
BATCHES = ((0, 1, 2, 3), (4, 5, 0), (1, 3, 5), (2, 4), (0, 1, 2, 3, 4, 5), (5,), (3, 0, 4), (4, 1))
ALL = tuple(range(6))
FIRST_SEED = 2


def _ref_trainer(rows, dtype):
    from hubertfa_amd.schedulers import one_cycle
    from hubertfa_amd.train import init_head
    W0, b0 = init_head(NEW_V + 2, HIDDEN, HEAD_SEED)
    tables = {n: np.ones(k, np.float32) for n, k in zip(ref.TABLES + (ref.CTC_TABLE,), (NEW_V, 10, 10, 3, 10, 3, 10))}
    fn = LOSS_CONFIG["function"]
    return train_ref.RefTrainer(rows, W0.numpy(), b0.numpy(), tables, LOSS_CONFIG["losses"]["weights"],
                                LOSS_CONFIG["losses"]["enable_RampUpScheduler"], OPT_CONFIG["total_steps"],
                                lambda k: one_cycle(k, OPT_CONFIG["total_steps"], OPT_CONFIG["lr"]["head"]),
                                OPT_CONFIG["weight_decay"], CLIP, fn["num_bins"], fn["alpha"], fn["label_smoothing"],
                                dtype)


@functools.lru_cache(maxsize=None)
def _trajectory():
    """The float64 run of the 8 steps on the first seed whose every step keeps 1e-4 from every discontinuity, so no
    element is excluded from any comparison, with its state before every step (``snaps``; snaps[8]: after the last).
    Two float32 runs give e_f32: ``sync32``, in which every step starts from the float64 run's state rounded to float32
    (the per-step losses), and ``ref32``, left to run on its own (the
    final head and tables of a free run)."""
    for seed in range(FIRST_SEED, FIRST_SEED + 400):
        rows = train_ref.draw_rows(9000 + seed, ROW_T, ROW_TYPES, HIDDEN, NEW_V)
        tr = _ref_trainer(rows, np.float64)
        first = tr.evaluate(ALL)
        steps, snaps = [], []
        for idx in BATCHES:
            snaps.append(tr.snapshot())
            steps.append(tr.step(idx))
            if tr.margins[-1] < 1e-4:
                break
        else:
            snaps.append(tr.snapshot())
            last = tr.evaluate(ALL)
            free = _ref_trainer(rows, np.float32)
            for idx in BATCHES:
                free.step(idx)
            t32 = _ref_trainer(rows, np.float32)
            steps32 = []
            for k, idx in enumerate(BATCHES):
                t32.restore(snaps[k])
                steps32.append(t32.step(idx))
            t32.restore(snaps[0])
            first32 = t32.evaluate(ALL)
            t32.restore(snaps[8])
            return dict(seed=seed, rows=rows, ref=tr, first=first, last=last, steps=steps, snaps=snaps, ref32=free,
                        steps32=steps32, first32=first32, last32=t32.evaluate(ALL))
    raise RuntimeError("no seed keeps the margin")


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """The CPU preconditions; then on the device the 8 steps left to run on their own (``free``: the final head and
    tables, the descent, the checkpoint), and the same 8 steps each started from the float64 run's state (load_state:
    ``got``), which is what the per-step comparisons use: a free run's losses past the first step carry the
    weights' accumulated float32 error, which AdamW's m / sqrt(v) amplifies, and no single float32 run bounds another's
    at a given step (measured on MI355X that way: step 7's CTC loss 1.18e-6 off, the float32 run's own 2.74e-7)."""
    tj = _trajectory()
    tr = tj["ref"]
    print(f"TRAINER seed {tj['seed']}: least margin {min(tr.margins):.3g}; clipped {tr.clipped}; evaluate total "
          f"{tj['first'][1]:.6g} -> {tj['last'][1]:.6g}")
    assert min(tr.margins) >= 1e-4
    assert tj["last"][1] < tj["first"][1]
    from hubertfa_amd import synth
    from hubertfa_amd.task import ForcedAlignmentTask, synth_checkpoint
    from hubertfa_amd.train import HeadTrainer
    d = tmp_path_factory.mktemp("trainer")
    ckpt = str(d / "model.ckpt")
    synth_checkpoint(ckpt)
    task = ForcedAlignmentTask.load_from_checkpoint(ckpt)
    assert task.head.head_w.shape[1] == HIDDEN
    trainer = HeadTrainer(task, OPT_CONFIG, LOSS_CONFIG, gradient_clip_val=CLIP, vocab=synth.synth_vocab(NEW_V - 1),
                          seed=HEAD_SEED)
    for r in tj["rows"]:
        trainer.add_features(r["y"], r)
    free_first = [float(v) for v in trainer.evaluate(ALL)]
    free = [[float(v) for v in trainer.step(idx)] for idx in BATCHES]
    free_last = [float(v) for v in trainer.evaluate(ALL)]
    free_state = trainer.state()
    got = []
    for k, idx in enumerate(BATCHES):
        trainer.load_state(tj["snaps"][k])
        got.append([float(v) for v in trainer.step(idx)])
    trainer.load_state(tj["snaps"][0])
    first = [float(v) for v in trainer.evaluate(ALL)]
    trainer.load_state(tj["snaps"][8])
    last = [float(v) for v in trainer.evaluate(ALL)]
    trainer.load_state(free_state)                       # (the checkpoint tests below save the free run's head)
    torch.cuda.synchronize()
    return dict(tj, trainer=trainer, task=task, got=got, got_first=first, got_last=last, free=free,
                free_first=free_first, free_last=free_last, free_state=free_state, dir=d, ckpt=ckpt)


def _rel(got, want):
    return abs(got - want) / abs(want) if want else abs(got)


def test_trainer_losses_follow_the_restatement(trained):
    """Every step's five losses and total within relative max(4 e_f32, 1e-6), e_f32 the float32 restatement's error at
    that step; the device and the float32 restatement both start the step from the float64 run's state (see ``trained``)."""
    seq = [("first", trained["got_first"], trained["first"], trained["first32"])] + \
        [(f"step {k}", g, w, w32) for k, (g, w, w32) in enumerate(zip(trained["got"], trained["steps"],
                                                                      trained["steps32"]))] + \
        [("last", trained["got_last"], trained["last"], trained["last32"])]
    for tag, got, (losses, total), f32 in seq:
        want = list(losses) + [total]
        e32 = [_rel(a, b) for a, b in zip(list(f32[0]) + [f32[1]], want)]
        err = [_rel(a, b) for a, b in zip(got, want)]
        print(f"TRAINER {tag}: losses {np.asarray(got)}; rel err {np.asarray(err)}; e_f32 {np.asarray(e32)}")
        assert all(e <= max(4 * f, 1e-6) for e, f in zip(err, e32)), tag
    for k, (g, (losses, total)) in enumerate(zip(trained["free"], trained["steps"])):     # recorded, not gated
        print(f"TRAINER free run step {k}: rel err {np.asarray([_rel(a, b) for a, b in zip(g, list(losses) + [total])])}")
    assert trained["free_last"][5] < trained["free_first"][5]
    assert int(trained["trainer"].skipped) == 0 and trained["free_state"]["step"] == 8


def _check_state(tag, st, want, f32):
    """Head and tables of a device state against a float64 snapshot, e_f32 from a float32 one."""
    for name, got, w, e in (("W", st["weight"].numpy(), want["weight"], f32["weight"]),
                            ("b", st["bias"].numpy(), want["bias"], f32["bias"])) + \
            tuple((n, st["tables"][n].numpy(), want["tables"][n], f32["tables"][n]) for n in want["tables"]):
        e32 = np.abs(np.asarray(e, np.float64) - w).max()
        err = np.abs(got.astype(np.float64) - w).max()
        bar = max(4 * e32, 1e-6 * np.abs(w).max())
        print(f"TRAINER {tag} {name}: err {err:.3g} (e_f32 {e32:.3g}, bar {bar:.3g}, max {np.abs(w).max():.3g})")
        assert err <= bar, (tag, name)


def test_trainer_final_head_and_tables(trained):
    """The free run's final head and tables against the float64 run's; e_f32 from the free float32 run."""
    st = trained["free_state"]
    _check_state("final", st, trained["ref"].snapshot(), trained["ref32"].snapshot())
    n4 = trained["trainer"].n4
    for t in (st["padded_weight"], st["padded_bias"], *st["exp_avg"], *st["exp_avg_sq"], *st["grad"]):
        assert t.shape[0] == n4 and torch.all(t[NEW_V + 2:] == 0)     # the padding rows never move


def test_trainer_checkpoint_round_trip(trained):
    from hubertfa_amd import ops
    from hubertfa_amd.losses import FALoss
    from hubertfa_amd.task import ForcedAlignmentTask
    trainer = trained["trainer"]
    out = str(trained["dir"] / "tuned.ckpt")
    trainer.save(out)
    loaded = ForcedAlignmentTask.load_from_checkpoint(out)
    assert loaded.vocab["vocab_size"] == NEW_V and loaded.head.vocab_size == NEW_V
    batch = trainer._batch((2,))
    mine = trainer.logits(batch)
    h = loaded.head
    theirs = ops.head_linear(batch["y"], None, h.head_wp, h.head_ws, h.head_bp, batch["lens"], flag=h.flag)
    assert h.head_ws is not None and torch.equal(mine, theirs[:, :, :NEW_V + 2])
    ck = torch.load(out, map_location="cpu", weights_only=True)
    src = torch.load(trained["ckpt"], map_location="cpu", weights_only=True)["state_dict"]
    assert all(torch.equal(ck["state_dict"][k], v) for k, v in src.items() if k.startswith("backbone."))
    assert ck["state_dict"]["head.weight"].shape == (NEW_V + 2, HIDDEN)
    hp = ck["hyper_parameters"]
    assert hp["loss_config"] == LOSS_CONFIG and hp["optimizer_config"] == OPT_CONFIG
    again = FALoss.from_checkpoint(ck["state_dict"], hp["loss_config"])
    assert again.vocab_size == NEW_V
    for n, t in trainer.loss.tables.items():
        assert torch.equal(again.tables[n], t), n


def test_same_vocabulary_keeps_the_head(trained):
    from hubertfa_amd import synth
    from hubertfa_amd.task import ForcedAlignmentTask
    from hubertfa_amd.train import HeadTrainer
    src = torch.load(trained["ckpt"], map_location="cpu", weights_only=True)["state_dict"]
    for vocab in (None, synth.synth_vocab(62)):
        task = ForcedAlignmentTask.load_from_checkpoint(trained["ckpt"])
        st = HeadTrainer(task, OPT_CONFIG, LOSS_CONFIG, vocab=vocab, seed=1).state()
        assert torch.equal(st["weight"], src["head.weight"].float()) and torch.equal(st["bias"], src["head.bias"].float())


def test_head_outside_the_split_range_is_caught(trained):
    """The trainer skips LatticeHead's one-time |w| < 16 test; a weight the split planes cannot hold raises the head's
    flag, which check_range (save, the CLI's read-backs) turns into an error and a fall-back to the f32 GEMM."""
    from hubertfa_amd.task import ForcedAlignmentTask
    from hubertfa_amd.train import HeadTrainer
    task = ForcedAlignmentTask.load_from_checkpoint(trained["ckpt"])
    trainer = HeadTrainer(task, OPT_CONFIG, LOSS_CONFIG)
    assert trainer.split
    trainer.check_range()                                             # in range: nothing happens
    st = trainer.state()
    st["weight"] = st["weight"].clone()
    st["weight"][3, 5] = 1e5
    trainer.load_state(st)
    with pytest.raises(RuntimeError):
        trainer.save(str(trained["dir"] / "bad.ckpt"))
    assert not os.path.exists(trained["dir"] / "bad.ckpt")
    assert not trainer.split and task.head.head_ws is None
    trainer.check_range()                                             # on the f32 GEMM from here on


# ---- finetune_head.py --------------------------------------------------------------------------------------------------
def _write_folder(d, vocab, sr=44100, secs=2.0):
    """Three synthetic files with labels from ``vocab`` (u1 weak) in score_labels.py's layout."""
    import csv
    from hubertfa_amd.wav_io import write_wav
    names = [p for p in vocab["vocab"] if p not in ("SP", "AP")]
    r = np.random.default_rng(11)
    with open(d / "transcriptions.csv", "w", newline="") as fh:
        wr = csv.writer(fh)
        wr.writerow(["name", "ph_seq", "ph_dur"])
        for i in range(3):
            write_wav(str(d / f"u{i}.wav"), (r.standard_normal(int(secs * sr)) * 0.1).astype(np.float32), sr)
            k = 5 + i
            phones = ["SP"] + [names[(3 * i + j) % len(names)] for j in range(k - 2)] + ["SP"]
            durs = "" if i == 1 else " ".join(f"{secs / k:.6f}" for _ in range(k))       # u1: a weak label
            wr.writerow([f"u{i}", " ".join(phones), durs])


def test_finetune_head_cli_same_vocabulary_keeps_the_head(tmp_path):
    """Without --vocab, on a checkpoint that carries no loss_config: the checkpoint's vocabulary and head continue (a
    0-step run writes the head's bytes back) under the reference's default loss_config."""
    from finetune_head import DEFAULT_LOSS_CONFIG
    from hubertfa_amd import synth
    from hubertfa_amd.task import synth_checkpoint
    ckpt, out = str(tmp_path / "model.ckpt"), str(tmp_path / "out.ckpt")
    src = synth_checkpoint(ckpt)
    _write_folder(tmp_path, synth.synth_vocab(62))
    run = subprocess.run([sys.executable, os.path.join(REPO, "finetune_head.py"), "-c", ckpt, "-f", str(tmp_path),
                          "--steps", "0", "-o", out], capture_output=True, text=True, cwd=REPO)
    assert run.returncode == 0, run.stderr[-2000:]
    ck = torch.load(out, map_location="cpu", weights_only=True)
    for k in ("head.weight", "head.bias"):
        assert torch.equal(ck["state_dict"][k], src["state_dict"][k].float()), k
    hp = ck["hyper_parameters"]
    assert hp["vocab_text"] == src["hyper_parameters"]["vocab_text"] and hp["loss_config"] == DEFAULT_LOSS_CONFIG
    assert ck["global_step"] == 0 and "CTC_GHM_loss_fn.ema" in ck["state_dict"]


def test_finetune_head_cli(tmp_path):
    import csv
    import yaml
    from finetune_head import batch_plan
    from hubertfa_amd import synth
    from hubertfa_amd.labels import read_transcriptions
    from hubertfa_amd.task import ForcedAlignmentTask, synth_checkpoint
    from hubertfa_amd.train import LOSS_NAMES, HeadTrainer
    from hubertfa_amd.wav_io import read_wav
    d = tmp_path
    ckpt = str(d / "model.ckpt")
    ck = synth_checkpoint(None)
    ck["hyper_parameters"]["loss_config"] = LOSS_CONFIG
    torch.save(ck, ckpt)
    vocab = synth.synth_vocab(NEW_V - 1)
    with open(d / "vocab.yaml", "w") as fh:
        yaml.safe_dump(vocab, fh)
    sr = 44100
    _write_folder(d, vocab, sr)
    out, log = str(d / "out.ckpt"), str(d / "run.jsonl")
    args = ["--steps", "4", "--batch_seconds", "5", "--lr", "0.01", "--clip", "0.5", "--seed", "4", "--log_every", "3"]
    run = subprocess.run([sys.executable, os.path.join(REPO, "finetune_head.py"), "-c", ckpt, "-f", str(d), "--vocab",
                          str(d / "vocab.yaml"), "--hubert_path", "synth:0", "-o", out, "--log", log] + args,
                         capture_output=True, text=True, cwd=REPO)
    assert run.returncode == 0, run.stderr[-2000:]
    lines = [json.loads(s) for s in open(log)]
    assert [ln["step"] for ln in lines] == [0, 1, 2, 3]
    keys = LOSS_NAMES + ("total_loss",)
    assert all(np.isfinite(ln[k]) for ln in lines for k in keys + ("lr", "beta1"))
    # the same first step by hand
    task = ForcedAlignmentTask.load_from_checkpoint(ckpt, hubert_model_path="synth:0")
    opt = {"lr": {"backbone": 0.0, "head": 0.01}, "weight_decay": 0.1, "total_steps": 4,
           "freeze": {"backbone": True, "head": False}}
    trainer = HeadTrainer(task, opt, LOSS_CONFIG, gradient_clip_val=0.5, vocab=vocab, seed=4)
    items = read_transcriptions(str(d))
    waves = np.stack([read_wav(str(d / f"{it['name']}.wav"))[0][0] for it in items])
    trainer.cache(task.upload(waves), items, wav_sr=sr, lengths=[waves.shape[1]] * 3)
    plan = batch_plan([row["T"] * trainer.frame_length for row in trainer.rows], 4, 5.0, 4)
    assert all(1 <= len(p) <= 2 for p in plan)                        # 2 s files, 5 s batches
    lr, b1 = trainer.schedule()
    by_hand = [float(v) for v in trainer.step(plan[0])]
    print("FINETUNE step 0:", lines[0], "by hand", by_hand)
    assert lines[0]["lr"] == lr and lines[0]["beta1"] == b1
    assert [lines[0][k] for k in keys] == by_hand
    # the new checkpoint scores its folder's labels
    score = subprocess.run([sys.executable, os.path.join(REPO, "score_labels.py"), "-c", out, "-f", str(d),
                            "--hubert_path", "synth:0"], capture_output=True, text=True, cwd=REPO)
    assert score.returncode == 0, score.stderr[-2000:]
    rows = list(csv.DictReader(open(d / "label_losses.csv")))
    assert sorted(x["name"] for x in rows) == ["MEAN", "u0", "u1", "u2"]
