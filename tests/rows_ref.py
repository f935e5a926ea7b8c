"""Plain float64 CPU restatements of the row kernels (norm.hip LayerNorm, attention.hip with per-row lengths, the
small kernels of misc.hip, viterbi.hip's lattice prologue), for tests/test_rows_gpu.py.  No kernel is called here."""
import numpy as np
import torch

F = torch.nn.functional


def randn(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def close(got, ref, rtol, atol):
    """tests/test_kernels_gpu.py's _close: |got - ref| <= atol + rtol |ref| element-wise (NaN fails)."""
    got = got.detach().cpu().double()
    ref = ref.detach().cpu().double()
    err = (got - ref).abs()
    bound = atol + rtol * ref.abs()
    assert bool((err <= bound).all()), \
        f"max err {float(err.nan_to_num(nan=float('inf')).max()):.3e}, " \
        f"worst err/bound {float((err / bound).nan_to_num(nan=float('inf')).max()):.3f}"


# ---- LayerNorm -------------------------------------------------------------------------------------------------
def activation(t, act):
    return [lambda v: v, F.gelu, F.hardswish][act](t)


def layernorm(x, gamma, beta, eps=1e-5, act=0, residual=None):
    """act(layer_norm((x + residual) in f32, then everything in f64)) over the last dim."""
    h = x if residual is None else x + residual
    C = x.shape[-1]
    return activation(F.layer_norm(h.double(), (C,), gamma.double(), beta.double(), eps), act)


def split_planes(y):
    """The split-f16 planes of an f32 tensor: hi = f16(y), lo = f16((y - hi) * 2^11) (round to nearest even)."""
    hi = y.half()
    lo = ((y - hi.float()) * 2048.0).half()
    return torch.stack([hi, lo])


def layernorm_stat_bound(x, gamma, ref, eps=1e-5):
    """Per-element error bound for rows with |mean| >> std: the project's tolerance plus the rounding of a float32
    mean of values of size max|x| (4 * 2^-24 * max_c |x|), carried through the normalisation (* rstd * |gamma_c|)."""
    xd = x.double()
    rstd = 1.0 / torch.sqrt(xd.var(-1, unbiased=False, keepdim=True) + eps)
    xmax = xd.abs().amax(-1, keepdim=True)
    return 2e-5 + 1e-5 * ref.abs() + 4 * 2.0 ** -24 * xmax * rstd * gamma.double().abs()


# ---- attention ---------------------------------------------------------------------------------------------------
def attention(q, k, v, H, D, lens=None):
    """f64 softmax(Q K^T / sqrt(D)) V per (batch, head) on q, k, v [B, L, H * D]; with lens, keys >= lens[b] are
    masked (query rows past the length: don't care)."""
    B, L = q.shape[:2]
    q, k, v = (t.double().reshape(B, L, H, D).transpose(1, 2) for t in (q, k, v))
    s = (q @ k.transpose(-1, -2)) * D ** -0.5
    if lens is not None:
        mask = torch.arange(L)[None, :] >= torch.tensor(lens)[:, None]          # [B, L] keys
        s = s.masked_fill(mask[:, None, None, :], float("-inf"))
    return (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B, L, H * D)


# ---- misc.hip ----------------------------------------------------------------------------------------------------
def mask_rows(x, lens):
    """x [B, T, ...] numpy: rows t >= lens[b] -> 0."""
    t = np.arange(x.shape[1])[None, :] < np.asarray(lens)[:, None]
    return np.where(t.reshape(t.shape + (1,) * (x.ndim - 2)), x, np.float32(0))


def pad_rows(x, left, n_out):
    """y[b, i] = x[b, i - left] inside [0, N), else 0, for i < n_out."""
    B, N = x.shape
    y = np.zeros((B, n_out), np.float32)
    lo, hi = left, min(left + N, n_out)
    if hi > lo:
        y[:, lo:hi] = x[:, : hi - lo]
    return y


def gather_index(n, ratio, U):
    """UnitsEncoder's nearest-frame index: f32 product, round half to even, clamped to the row's last unit."""
    k = np.arange(n, dtype=np.float32)
    return np.minimum(np.rint(np.float32(ratio) * k), U - 1).astype(np.int64)


def units_gather(units, n_frames_b, U_b, T_pad, ratio):
    """units [B, U, C] numpy -> [B, T_pad, C]: row k < n_frames_b[b] is units[b, index[k]], the rest zeros."""
    B, _, C = units.shape
    out = np.zeros((B, T_pad, C), np.float32)
    for b in range(B):
        n = int(n_frames_b[b])
        out[b, :n] = units[b, gather_index(n, ratio, int(U_b[b]))]
    return out


def wav_normalize(x, lens=None, eps=1e-7):
    """zero_mean_unit_var_norm per row over its own len samples (biased variance), zeros past it; f64."""
    x = x.double()
    B, N = x.shape
    out = torch.zeros(B, N, dtype=torch.float64)
    for b in range(B):
        n = N if lens is None else int(lens[b])
        if n > 0:
            r = x[b, :n]
            out[b, :n] = (r - r.mean()) / torch.sqrt(r.var(unbiased=False) + eps)
    return out


# ---- lattice prologue ----------------------------------------------------------------------------------------------
def lattice_prologue(logits, ids, T, S):
    """One utterance of AlignmentDecoder.decode's device part.  logits [Tl, V + 2] f32 (the head's layout: edge,
    ctc blank, V frame classes), ids [>= S] ints.  The mask x - 1e9 * (v not allowed) is formed in float32 as the
    original does; everything after it in f64.  Returns a dict of numpy f64 arrays over the T valid frames."""
    V = logits.shape[1] - 2
    ids = np.asarray(ids[:S], dtype=np.int64)
    allowed = np.zeros(V, bool)
    allowed[0] = True
    allowed[ids] = True
    x = logits[:T, 2:].float() - (torch.from_numpy(~allowed)[None] * 1e9).float()
    xd = x.double()
    lp = torch.log_softmax(xd, -1).numpy()
    sm = torch.softmax(xd, -1).numpy()
    e = ((torch.sigmoid(logits[:T, 0].double()) - 0.1) / 0.8).clamp(0, 1).numpy()
    ep = np.clip(e + np.concatenate(([0.0], e[:-1])), 0, 1) if T else e
    diff = np.concatenate((e[1:] - e[:-1], [0.0])) if T else e
    with np.errstate(divide="ignore"):
        out = dict(allowed=allowed, ph_prob_log=lp, ph_frame_pred=sm, prob_log=lp[:, ids], e=e, edge_prob=ep,
                   edge_diff=diff, edge_log=np.log(ep + 1e-6), not_edge_log=np.log(1 - ep + 1e-6))
    return out


def dp_row0(prob_log, ids, T, S, Smax):
    """_decode's initialisation from the lattice's own row 0: dp[0, 0] = L[0, 0]; with an id-0 first phone and S > 1
    also dp[0, 1] = L[0, 1]; every other state (the padding pitch included) -inf; all -inf for T = 0."""
    row = np.full(Smax, -np.inf)
    if T > 0:
        row[0] = prob_log[0, 0]
        if S > 1 and ids[0] == 0:
            row[1] = prob_log[0, 1]
    return row


def edge_band(ep):
    """Frames whose edge_prob p has p or 1 - p inside (0, 1e-3): log(. + 1e-6) amplifies float32 rounding there."""
    return ((ep > 0) & (ep < 1e-3)) | ((1 - ep > 0) & (1 - ep < 1e-3))
