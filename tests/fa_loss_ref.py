"""Restatement of the reference's five alignment losses (test_fa_loss.py, test_fa_loss_gpu.py); numpy only.

``run``: the four full-label terms of _get_loss (networks/task/forced_alignment.py:188-254: GHMLoss, MultiLabelGHMLoss(1)
on the edge and on the edge-difference pairs, BinaryEMDLoss) from their definitions, their gradients with
respect to the head logits written out by hand, the bincounts and the margins of every discontinuity.  ``ctc_term``: the
fifth (CTCGHMLoss) on tests/ctc_fb_ref.py's forward-backward.  ``update_ema``: GHMLoss.py:5-9.  Everything runs in
``dtype``: float64 is the yardstick; float32 gives the error the formulas have in the device's precision (e_f32).

Head layout: column 0 the edge, column 1 the CTC blank, columns 2.. the V frame classes.
"""
import numpy as np

import ctc_fb_ref

NAMES = ("ph_frame_GHM_loss", "ph_edge_GHM_loss", "ph_edge_EMD_loss", "ph_edge_diff_loss", "ctc_GHM_loss")
TABLES = ("ph_frame_GHM_loss_fn.class_ema", "ph_frame_GHM_loss_fn.GD_ema", "ph_edge_GHM_loss_fn.GD_stat_ema",
          "ph_edge_GHM_loss_fn.label_stat_ema_each_class", "ph_edge_diff_GHM_loss_fn.GD_stat_ema",
          "ph_edge_diff_GHM_loss_fn.label_stat_ema_each_class")
CTC_TABLE = "CTC_GHM_loss_fn.ema"
MARGIN = 1e-5


def make_tables(V, num_bins, seed):
    """Non-uniform positive tables (each normalised to mean 1, as update_ema leaves them) under the reference's names."""
    r = np.random.default_rng(seed)
    out = {}
    for n, k in zip(TABLES + (CTC_TABLE,), (V, num_bins, num_bins, 3, num_bins, 3, 10)):
        v = r.uniform(0.3, 1.7, k)
        out[n] = (v / v.sum() * k).astype(np.float32)
    return out


def pack_tables(tables):
    return np.concatenate([np.asarray(tables[n], np.float32) for n in TABLES])


def update_ema(ema, alpha, num_bins, hist, dtype=np.float64, hist_dtype=None):
    """``hist_dtype``: the dtype the counts arrive in and are normalised in (the edge term's arrive as float32 whatever
    the model's dtype: its mask is forced_alignment.py:208-209's time_mask.float())."""
    hd = hist_dtype or dtype
    ema, hist = np.asarray(ema, dtype), np.asarray(hist, hd)
    hist = hist / (hist.sum(dtype=hd) + hd(1e-10)) * hd(num_bins)
    ema = ema * dtype(alpha) + (hd(1 - float(alpha)) * hist).astype(dtype)
    return ema / (ema.sum(dtype=dtype) + dtype(1e-10)) * dtype(num_bins)


def _sig(x):
    return 1 / (1 + np.exp(-x))


def _bce(x, g):
    return np.maximum(x, 0) - x * g + np.log1p(np.exp(-np.abs(x)))


def _frac_margin(v):
    v = np.asarray(v, np.float64)
    return float(np.min(np.abs(v - np.rint(v)))) if v.size else np.inf


def _ghm_edge(x, g, gd_ema, lab_ema, nb, dtype):
    """MultiLabelGHMLoss(1) per sample: weighted loss, d / d x, the two bins and the two margins."""
    p = _sig(x)
    gd = np.abs(p - g) * dtype(nb)
    b = np.clip(np.floor(gd).astype(np.int64), 0, nb - 1)
    lb = np.clip(np.floor(g * dtype(3)).astype(np.int64), 0, 2)
    w = np.sqrt((1 / gd_ema[b] + dtype(1e-3)) * (1 / lab_ema[lb] + dtype(1e-3)))
    return _bce(x, g) * w, w * (p - g), b, lb, _frac_margin(gd), _frac_margin(g * dtype(3))


def run(logits, T, label_type, ph_frame, ph_edge, ph_mask, tables, num_bins=10, label_smoothing=0.0,
        dtype=np.float64):
    """Returns a dict: losses [4], row_terms [B, 4] (unnormalised sums; EMD (sum|F| + sum|R|) / 2), norm [4], grads
    [4, B, Tmax, V + 2] (d losses[k] / d logits), terms [B, Tmax, 3], bins [B, Tmax, 5] (-1 where not counted), hist
    {table name: counts}, margin = (GD bins, label bins, cumulative sums): the least distance to a discontinuity."""
    x_all = np.asarray(logits, dtype)
    B, Tmax, C = x_all.shape
    V, nb = C - 2, int(num_bins)
    # the reference clamps a .float() one-hot by Python floats (GHMLoss.py:256-260): float32 targets in every dtype
    ls, hs = dtype(np.float32(label_smoothing)), dtype(np.float32(1 - float(label_smoothing)))
    tab = {n: np.asarray(tables[n], dtype) for n in TABLES}
    full = np.asarray(label_type) >= 2
    row_terms = np.zeros((B, 4), dtype)
    ug = np.zeros((4, B, Tmax, C), dtype)                    # gradients of the unnormalised sums
    terms = np.zeros((B, Tmax, 3), dtype)
    bins = np.full((B, Tmax, 5), -1, np.int64)
    hist = {n: np.zeros(len(tab[n]), np.int64) for n in TABLES}
    norm = np.zeros(4, dtype)
    m_gd, m_lab, m_cum = [np.inf], [np.inf], [np.inf]
    for b in np.nonzero(full)[0]:
        Tb = int(min(max(int(T[b]), 0), Tmax))
        norm[2] += Tmax
        if Tb == 0:
            continue
        x = x_all[b, :Tb]
        lab = np.asarray(ph_frame[b, :Tb], np.int64)
        g = np.asarray(ph_edge[b, :Tb], dtype)
        live = np.asarray(ph_mask[b]) != 0
        ar = np.arange(Tb)
        # frame term
        if live.any():
            xl = x[:, 2:][:, live]
            d = xl - xl.max(axis=1, keepdims=True)
            lsm = d - np.log(np.exp(d).sum(axis=1, keepdims=True, dtype=dtype))
            p = np.zeros((Tb, V), dtype)
            p[:, live] = np.exp(lsm)
            tg = np.full((Tb, V), ls, dtype)
            tg[ar, lab] = hs
            tg = tg * live[None, :]
            raw = -(tg[:, live] * lsm).sum(axis=1, dtype=dtype)
            gd = np.abs(p[ar, lab] - tg[ar, lab]) * dtype(nb)
            bf = np.clip(np.floor(gd).astype(np.int64), 0, nb - 1)
            w = np.sqrt(tab[TABLES[0]][lab] * tab[TABLES[1]][bf])
            terms[b, :Tb, 0] = raw / w
            ug[0, b, :Tb, 2:] = (tg.sum(axis=1, keepdims=True, dtype=dtype) * p - tg) / w[:, None]
            bins[b, :Tb, 0] = bf
            hist[TABLES[0]] += np.bincount(lab, minlength=V)[:V]
            hist[TABLES[1]] += np.bincount(bf, minlength=nb)
            norm[0] += Tb
            m_gd.append(_frac_margin(gd))
        # edge term
        x0 = x[:, 0]
        te, de, be, le, mg, ml = _ghm_edge(x0, g, tab[TABLES[2]], tab[TABLES[3]], nb, dtype)
        terms[b, :Tb, 1] = te
        ug[1, b, :Tb, 0] = de
        bins[b, :Tb, 1], bins[b, :Tb, 2] = be, le
        hist[TABLES[2]] += np.bincount(be, minlength=nb)
        hist[TABLES[3]] += np.bincount(le, minlength=3)
        norm[1] += Tb
        m_gd.append(mg)
        m_lab.append(ml)
        # edge-difference term: pair t = frames (t, t + 1)
        p0 = _sig(x0)
        dp = p0 * (1 - p0)
        if Tb > 1:
            z = ((p0[1:] - p0[:-1]) + 1) / 2
            gz = ((g[1:] - g[:-1]) + 1) / 2
            td, dd, bd, ld, mg, ml = _ghm_edge(z, gz, tab[TABLES[4]], tab[TABLES[5]], nb, dtype)
            terms[b, :Tb - 1, 2] = td
            ug[3, b, 1:Tb, 0] += dd * dp[1:] / 2
            ug[3, b, :Tb - 1, 0] -= dd * dp[:-1] / 2
            bins[b, :Tb - 1, 3], bins[b, :Tb - 1, 4] = bd, ld
            hist[TABLES[4]] += np.bincount(bd, minlength=nb)
            hist[TABLES[5]] += np.bincount(ld, minlength=3)
            norm[3] += Tb - 1
            m_gd.append(mg)
            m_lab.append(ml)
        # EMD term
        d = p0 - g
        F = np.cumsum(d, dtype=dtype)
        R = np.cumsum(d[::-1], dtype=dtype)[::-1]
        pad = Tmax - Tb
        row_terms[b, 2] = ((np.abs(F).sum(dtype=dtype) + pad * np.abs(F[-1])) + np.abs(R).sum(dtype=dtype)) / 2
        sF, sR = np.sign(F), np.sign(R)
        ug[2, b, :Tb, 0] = dp * (np.cumsum(sF[::-1])[::-1] + pad * sF[-1] + np.cumsum(sR)) / 2
        m_cum.append(float(min(np.abs(F).min(), np.abs(R).min())))
        row_terms[b, 0] = terms[b, :, 0].sum(dtype=dtype)
        row_terms[b, 1] = terms[b, :, 1].sum(dtype=dtype)
        row_terms[b, 3] = terms[b, :, 2].sum(dtype=dtype)
    safe = np.where(norm > 0, norm, 1)
    losses = np.where(norm > 0, row_terms.sum(axis=0, dtype=dtype) / safe, 0).astype(dtype)
    grads = ug / safe[:, None, None, None] * (norm > 0)[:, None, None, None]
    return dict(losses=losses, row_terms=row_terms, norm=norm, grads=grads, terms=terms, bins=bins, hist=hist,
                margin=(min(m_gd), min(m_lab), min(m_cum)))


def margins_ok(out):
    """The condition on test inputs: no floor or sign argument within MARGIN of its discontinuity (float64 run)."""
    return all(m >= MARGIN for m in out["margin"])


def ctc_term(logits, T, label_type, ph_id_seq, ema, num_bins=10):
    """CTCGHMLoss.forward (GHMLoss.py:21-56) over the rows with label_type >= 1, float64: returns (loss, grad
    [B, Tmax, V + 2] = d loss / d logits, non-zero in column 1 and columns 3.., hist [num_bins] of the clipped
    per-frame confidences, as torch.histc(bins=num_bins, min=0, max=1))."""
    x_all = np.asarray(logits, np.float64)
    B, Tmax, C = x_all.shape
    ema = np.asarray(ema, np.float64)
    weak = np.nonzero(np.asarray(label_type) >= 1)[0]
    grad = np.zeros((B, Tmax, C))
    hist = np.zeros(num_bins, np.int64)
    if len(weak) == 0:
        return 0.0, grad, hist
    loss = 0.0
    for b in weak:
        Tb = int(T[b])
        x = np.concatenate([x_all[b, :Tb, 1:2], x_all[b, :Tb, 3:]], axis=1)
        o = ctc_fb_ref.oracle(x, np.asarray(ph_id_seq[b], np.int64))
        conf = min(max(np.exp(-o["nll"] / Tb), 1e-6), 1 - 1e-6)
        k = min(max(int(np.floor(conf * num_bins)), 0), num_bins - 1)
        w = 1 / (ema[k] + 1e-10)
        loss += o["nll"] * w / len(weak)
        grad[b, :Tb, 1] = o["grad"][:, 0] * w / len(weak)
        grad[b, :Tb, 3:] = o["grad"][:, 1:] * w / len(weak)
        hist[k] += 1
    return loss, grad, hist


def draw_case(B, Tmax, V, Ts, label_types, seed, num_bins=10, label_smoothing=0.0, mask_live=None, scale=2.0,
              max_tries=200):
    """Seeded inputs that keep MARGIN from every discontinuity (the float64 restatement decides; the seed is advanced
    until they do): logits [B, Tmax, V + 2] f32, ph_frame, ph_edge in (0, 1), ph_mask (every drawn label live;
    ``mask_live``: that many live classes at the most), tables.  Returns (inputs dict, the float64 run)."""
    for k in range(max_tries):
        r = np.random.default_rng(seed + 1000 * k)
        logits = (r.standard_normal((B, Tmax, V + 2)) * scale).astype(np.float32)
        n_live = V if mask_live is None else max(1, min(mask_live, V))
        ph_mask = np.zeros((B, V), np.int32)
        ph_frame = np.zeros((B, Tmax), np.int32)
        for b in range(B):
            livec = np.sort(r.choice(V, n_live, replace=False))
            ph_mask[b, livec] = 1
            ph_frame[b] = livec[r.integers(0, n_live, Tmax)]
        ph_edge = r.uniform(0.02, 0.98, (B, Tmax)).astype(np.float32)
        tables = make_tables(V, num_bins, seed + 7)
        inp = dict(logits=logits, T=np.asarray(Ts, np.int32), label_type=np.asarray(label_types, np.int32),
                   ph_frame=ph_frame, ph_edge=ph_edge, ph_mask=ph_mask, tables=tables, num_bins=num_bins,
                   label_smoothing=label_smoothing, seed=seed + 1000 * k)
        out = run(logits, inp["T"], inp["label_type"], ph_frame, ph_edge, ph_mask, tables, num_bins, label_smoothing)
        if margins_ok(out):
            return inp, out
    raise RuntimeError("no seed keeps the margin")
