"""References for the CTC forward-backward tests (test_ctc_fb.py, test_ctc_fb_gpu.py); numpy only.

``oracle``: float64 forward-backward written from the definitions.  Extended states s = 0..2L, blank_j
= 2j, label_j = 2j + 1; y[t, s] the log-softmax emission of s's class; alpha and beta in torch's convention (both
include y[t, s]); gamma(t, s) = exp(alpha + beta - y + nll).

``emulate``: the kernels' documented scheme in float32 -- f32 log-softmax, f32 alpha and beta with the row maximum moved
into an f64 offset after every 16th step, gamma = exp(f32(alpha_rel + beta_rel - y) + f32(aoff + boff + nll)), f32
sums over t in the kernel's order (descending t).  Its own error against the oracle sets the bar for the device:
|device - oracle| <= max(4 e_emu, floor) per array and case.

Both return a dict: nll (float), occ [T, L + 1], frames / centre / logp [L], Gam [T, V] (the class posterior), grad
[T, V] = softmax - Gam; an infeasible pair gives nll = inf, zeros, and logp = -inf.
"""
import numpy as np

REBASE = 16
FLOOR = 2e-5             # three f32 roundings at magnitude <= 64 (ulp 7.6e-6) in the exponent of a value <= 1


def _lse3(a, b, c):
    """log(exp(a) + exp(b) + exp(c)) elementwise in the arrays' dtype, as ctc.hip's lse3; -inf when all are."""
    hi = np.maximum(np.maximum(a, b), c)
    lo = np.minimum(np.minimum(a, b), c)
    mid = np.maximum(np.minimum(a, b), np.minimum(np.maximum(a, b), c))
    mm = np.where(np.isneginf(hi), 0, hi).astype(a.dtype)
    with np.errstate(invalid="ignore"):
        return hi + np.log(1 + np.exp(mid - mm) + np.exp(lo - mm))


def _scan(ye_row, cls, skip, T, dtype, rebase):
    """The alpha rows [T, S] (relative to off [T] when ``rebase``) and the final row; ye_row(t) -> y[t, cls]."""
    S = cls.shape[0]
    ninf = dtype(-np.inf)
    prev = np.full(S, ninf, dtype)
    prev[0] = 0                                   # the virtual row before frame 0
    rows, off, offset = np.empty((T, S), dtype), np.zeros(T), 0.0
    pad = np.full(2, ninf, dtype)
    for t in range(T):
        p = np.concatenate([pad, prev])
        prev = ye_row(t) + _lse3(prev, p[1:-1], np.where(skip, p[:-2], ninf))
        if rebase and t % REBASE == REBASE - 1:
            m = prev.max()
            prev = prev - m
            offset += float(m)
        rows[t], off[t] = prev, offset
    return rows, off


def _run(x, tg, dtype, rebase):
    x = np.asarray(x, dtype)
    tg = np.asarray(tg, np.int64).reshape(-1)
    T, V = x.shape
    L = tg.shape[0]
    S = 2 * L + 1
    ninf = dtype(-np.inf)
    d = x - x.max(axis=1, keepdims=True) if T else x
    y = d - np.log(np.exp(d).sum(axis=1, keepdims=True, dtype=dtype)) if T else x      # log_softmax in ``dtype``
    cls = np.zeros(S, np.int64)
    cls[1::2] = tg
    skip = np.zeros(S, bool)                      # state s may be entered from s - 2
    skip[3::2] = tg[1:] != tg[:-1]
    skip_up = np.concatenate([skip, [False, False]])[2:]
    out = dict(occ=np.zeros((T, L + 1), dtype), frames=np.zeros(L, dtype), centre=np.zeros(L, dtype),
               logp=np.full(L, ninf, dtype), Gam=np.zeros((T, V), dtype), grad=np.zeros((T, V), dtype))
    if T == 0:
        out["nll"] = 0.0 if L == 0 else np.inf
        return out
    alpha, aoff = _scan(lambda t: y[t, cls], cls, skip, T, dtype, rebase)
    fin = np.array([alpha[-1, -1], alpha[-1, -2] if L else -np.inf], np.float64)
    if np.isneginf(fin.max()):
        out["nll"] = np.inf
        return out
    nll = -(aoff[-1] + fin.max() + np.log1p(np.exp(fin.min() - fin.max())))
    out["nll"] = float(nll)
    beta = np.full(S, ninf, dtype)
    beta[-1] = 0                                  # the virtual row after frame T - 1
    boff = 0.0
    pad = np.full(2, ninf, dtype)
    fr, ce, lp = np.zeros(L, dtype), np.zeros(L, dtype), np.zeros(L, dtype)
    for k in range(T):
        t = T - 1 - k
        ye = y[t, cls]
        n = np.concatenate([beta, pad])
        beta = ye + _lse3(beta, n[1:-1], np.where(skip_up, n[2:], ninf))
        if rebase and k % REBASE == REBASE - 1:
            m = beta.max()
            beta = beta - m
            boff += float(m)
        c = dtype(aoff[t] + (boff + nll))
        dead = np.isneginf(alpha[t]) | np.isneginf(beta)
        with np.errstate(invalid="ignore"):
            g = np.where(dead, 0, np.exp(((alpha[t] + beta) - ye) + c)).astype(dtype)
        out["occ"][t, 0] = g[0::2].sum(dtype=dtype)
        gl = g[1::2]
        out["occ"][t, 1:] = gl
        fr += gl
        ce += dtype(t) * gl
        with np.errstate(invalid="ignore"):
            lp += np.where(gl > 0, gl * ye[1::2], 0).astype(dtype)
        np.add.at(out["Gam"][t], cls, g)
    out["frames"], out["centre"], out["logp"] = fr, ce / fr, lp / fr
    out["grad"] = np.exp(y) - out["Gam"]
    return out


def oracle(x, tg):
    """float64, no rebasing."""
    return _run(x, tg, np.float64, False)


def emulate(x, tg):
    """The kernels' scheme in float32 (x is rounded to f32 first, as the device reads it)."""
    return _run(np.asarray(x, np.float32), tg, np.float32, True)


KEYS = ("occ", "frames", "centre", "logp", "Gam", "grad")


def bars(want, emu, T):
    """The absolute bar of every array for one row: max(4 e_emu, floor); the floor of the sums over t is FLOOR * T.
    ``rowsum`` is the bar for |sum_j occ[t, j] - 1|."""
    out = {}
    for k in KEYS:
        fin = np.isfinite(want[k])
        e = float(np.max(np.abs(emu[k][fin] - want[k][fin]))) if fin.any() else 0.0
        out[k] = max(4 * e, FLOOR * (max(T, 1) if k in ("frames", "centre", "logp") else 1))
    e = float(np.max(np.abs(emu["occ"].sum(axis=1, dtype=np.float64) - 1))) if want["occ"].shape[0] and \
        np.isfinite(want["nll"]) else 0.0
    out["rowsum"] = max(4 * e, FLOOR)
    return out


def head_layout(x):
    """CTC logits [.., V] -> the head's [.., V + 2]: the blank in column 1, label c in column c + 2, and 1e30 in
    columns 0 and 2, which would wreck every result if a kernel read them."""
    x = np.asarray(x, np.float32)
    full = np.full(x.shape[:-1] + (x.shape[-1] + 2,), 1e30, np.float32)
    full[..., 1] = x[..., 0]
    full[..., 3:] = x[..., 1:]
    return full


def localisation_fixture(k=None):
    """V = 20, twelve labels of 6 frames at logit 5.0 followed by 2 blank frames (T = 96), every other logit 0;
    the transcript has position ``k`` replaced by class 19 (None: the true one).  Returns (x [96, 20], transcript)."""
    labels = [3, 7, 11, 5, 9, 2, 14, 6, 17, 8, 12, 4]
    x = np.zeros((96, 20), np.float32)
    for j, c in enumerate(labels):
        x[8 * j:8 * j + 6, c] = 5.0
        x[8 * j + 6:8 * j + 8, 0] = 5.0
    tg = np.array(labels, np.int64)
    if k is not None:
        tg[k] = 19
    return x, tg
