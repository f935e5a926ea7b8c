"""Thin torch wrappers over the libhfa C-ABI: tensors -> raw device pointers + the current HIP stream.

PyTorch is plumbing here (device memory, streams); every op below launches a hand-written gfx950 kernel from
libhfa.so.  Inputs must already be on the GPU — there is no CPU path and no silent fallback.
"""
from __future__ import annotations

import contextlib
import ctypes

import torch

from . import _lib

_P = ctypes.c_void_p


def _ptr(t: torch.Tensor | None):
    return _P(0) if t is None else _P(t.data_ptr())


def _stream(device=None):
    return _P(torch.cuda.current_stream(device).cuda_stream)


def _need(t: torch.Tensor, dtype, name: str, contiguous: bool = True):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor")
    if t.device.type != "cuda":
        raise _lib.HFALibraryError(f"{name}: must be a GPU tensor (no CPU fallback), got {t.device}")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if contiguous and not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")
    return t


# ------------------------------------------------------------------------------------------------------------
# Alignment decoder (viterbi.hip)
# ------------------------------------------------------------------------------------------------------------
def viterbi_forward(prob_log, not_edge_log, edge_log, curr, dp, bt, ph_seq_id, T, S, pad=None, steps=None):
    """In-place batched forward_pass (alignment_decoder.py:170-230).

    prob_log/dp [B,Tmax,Smax] f32 (dp row 0 pre-initialised), bt [B,Tmax,Smax] int8, curr [B,Smax] f64,
    not_edge_log/edge_log [B,Tmax] f32, ph_seq_id [B,Smax] i32, T/S/pad [B] i32.  ``steps`` (t_begin, t_end):
    only those time steps, continuing from dp row t_begin - 1 and curr (consecutive ranges = one whole call).
    """
    B, Tmax, Smax = prob_log.shape
    for t, dt, n in ((prob_log, torch.float32, "prob_log"), (not_edge_log, torch.float32, "not_edge_log"),
                     (edge_log, torch.float32, "edge_log"), (curr, torch.float64, "curr"),
                     (dp, torch.float32, "dp"), (bt, torch.int8, "bt"), (ph_seq_id, torch.int32, "ph_seq_id"),
                     (T, torch.int32, "T"), (S, torch.int32, "S")):
        _need(t, dt, n)
    if pad is not None:
        _need(pad, torch.int32, "pad")
    assert dp.shape == prob_log.shape and bt.shape == prob_log.shape
    assert curr.shape == (B, Smax) and ph_seq_id.shape == (B, Smax)
    assert not_edge_log.shape == (B, Tmax) and edge_log.shape == (B, Tmax)

    t0, t1 = (1, max(Tmax, 1)) if steps is None else (int(steps[0]), int(steps[1]))

    def launch():
        _lib.call("hfa_viterbi_forward_steps", B, Tmax, Smax, _ptr(T), _ptr(S), _ptr(pad), _ptr(prob_log),
                  _ptr(not_edge_log), _ptr(edge_log), _ptr(curr), _ptr(dp), _ptr(bt), _ptr(ph_seq_id), t0, t1,
                  _stream(prob_log.device))
    if PROBE is None:
        return launch()
    # SURVEY §8(d) algorithmic bytes: prob_log in + dp out (4 B each) + bt out (1 B) per cell, 8 B edge terms
    # per frame; counted on the padded planes (exact when every utterance of the batch fills them).  A step range
    # (a held DP, task.submit) counts its own time steps: ``units`` carries them, so the per-step figures hold.
    n = max(t1 - t0, 0) if steps is not None else Tmax
    PROBE("viterbi_forward_kernel", B * (9.0 * n * Smax + 8.0 * n), launch, kind="bytes", units=n)


def viterbi_backtrack(dp, bt, ph_seq_id, T, S):
    """Batched end-state + backtrack + frame confidence (alignment_decoder.py:263-288).

    Returns (ph_idx_seq [B,Tmax] i32, ph_time_int [B,Tmax] i32, n [B] i32, frame_conf [B,Tmax] f32);
    row b is valid up to n[b] (ascending t) / T[b].
    """
    B, Tmax, Smax = dp.shape
    _need(dp, torch.float32, "dp")
    _need(bt, torch.int8, "bt")
    _need(ph_seq_id, torch.int32, "ph_seq_id")
    _need(T, torch.int32, "T")
    _need(S, torch.int32, "S")
    dev = dp.device
    idx = torch.empty((B, Tmax), dtype=torch.int32, device=dev)
    tint = torch.empty((B, Tmax), dtype=torch.int32, device=dev)
    n = torch.empty((B,), dtype=torch.int32, device=dev)
    fc = torch.empty((B, Tmax), dtype=torch.float32, device=dev)
    _lib.call("hfa_viterbi_backtrack", B, Tmax, Smax, _ptr(T), _ptr(S), _ptr(dp), _ptr(bt), _ptr(ph_seq_id),
              _ptr(idx), _ptr(tint), _ptr(n), _ptr(fc), _stream(dev))
    return idx, tint, n, fc


def lattice_prologue(frame_logits, edge_logits, ph_seq_id, T, S, want_frame_probs: bool = False,
                     init_dp: bool = False):
    """Mask + log_softmax/softmax + edge sigmoid/diff/prob + gather to the [T,S] lattice (alignment_decoder.py
    :35-84, 239-242).  frame_logits [B,Tl,V] and edge_logits [B,Tl] may be strided views (last dim unit stride).
    ``init_dp``: also allocate the DP's dp / bt / curr and write _decode's initialisation (:244-254) in the same
    launch (out["dp"], out["bt"], out["curr"], ready for viterbi_forward)."""
    B, Tl, V = frame_logits.shape
    Smax = ph_seq_id.shape[1]
    _need(frame_logits, torch.float32, "frame_logits", contiguous=False)
    _need(edge_logits, torch.float32, "edge_logits", contiguous=False)
    if frame_logits.stride(2) != 1:
        raise ValueError("frame_logits: last dim must have unit stride")
    _need(ph_seq_id, torch.int32, "ph_seq_id")
    _need(T, torch.int32, "T")
    _need(S, torch.int32, "S")
    Tmax = Tl
    dev = frame_logits.device
    out = {
        "prob_log": torch.empty((B, Tmax, Smax), dtype=torch.float32, device=dev),
        "edge_log": torch.empty((B, Tmax), dtype=torch.float32, device=dev),
        "not_edge_log": torch.empty((B, Tmax), dtype=torch.float32, device=dev),
        "edge_diff": torch.empty((B, Tmax), dtype=torch.float32, device=dev),
        "edge_prob": torch.empty((B, Tmax), dtype=torch.float64, device=dev),
        "ph_prob_log": torch.empty((B, Tmax, V), dtype=torch.float32, device=dev) if want_frame_probs else None,
        "ph_frame_pred": torch.empty((B, Tmax, V), dtype=torch.float32, device=dev) if want_frame_probs else None,
        "dp": torch.empty((B, Tmax, Smax), dtype=torch.float32, device=dev) if init_dp else None,
        "bt": torch.empty((B, Tmax, Smax), dtype=torch.int8, device=dev) if init_dp else None,
        "curr": torch.empty((B, Smax), dtype=torch.float64, device=dev) if init_dp else None,
    }
    _lib.call("hfa_lattice_prologue", B, Tmax, V, Smax, _ptr(T), _ptr(S), _ptr(frame_logits),
              frame_logits.stride(1), frame_logits.stride(0), _ptr(edge_logits), edge_logits.stride(1),
              edge_logits.stride(0), _ptr(ph_seq_id), _ptr(out["ph_prob_log"]), _ptr(out["ph_frame_pred"]),
              _ptr(out["prob_log"]), _ptr(out["edge_log"]), _ptr(out["not_edge_log"]), _ptr(out["edge_diff"]),
              _ptr(out["edge_prob"]), _ptr(out["dp"]), _ptr(out["curr"]), _stream(dev))
    return out


def viterbi_init(prob_log, ph_seq_id, T, S):
    """_decode's dp / bt / curr initialisation (alignment_decoder.py:244-254) for a lattice that did not come
    through lattice_prologue: returns (dp, bt, curr) ready for viterbi_forward."""
    B, Tmax, Smax = prob_log.shape
    _need(prob_log, torch.float32, "prob_log")
    _need(ph_seq_id, torch.int32, "ph_seq_id")
    _need(T, torch.int32, "T")
    _need(S, torch.int32, "S")
    dev = prob_log.device
    dp = torch.empty((B, Tmax, Smax), dtype=torch.float32, device=dev)
    bt = torch.empty((B, Tmax, Smax), dtype=torch.int8, device=dev)
    curr = torch.empty((B, Smax), dtype=torch.float64, device=dev)
    _lib.call("hfa_viterbi_init", B, Tmax, Smax, _ptr(T), _ptr(S), _ptr(prob_log), _ptr(ph_seq_id), _ptr(dp),
              _ptr(curr), _stream(dev))
    return dp, bt, curr


# ------------------------------------------------------------------------------------------------------------
# Encoder kernels (gemm.hip, attention.hip, norm.hip, conv.hip, misc.hip)
# ------------------------------------------------------------------------------------------------------------
EPI_NONE, EPI_GELU = 0, 1
GEMM_F16 = 0x100          # hfa.h HFA_GEMM_F16: opt-in one-product f16 arithmetic on the split GEMM
ACT_NONE, ACT_GELU, ACT_HARDSWISH = 0, 1, 2

_P_, _I_, _LL_, _F_ = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_float
_lib.register("hfa_conv_gemm_f32", [_I_, _I_, _I_, _I_, _I_, _P_, _LL_, _LL_, _I_, _I_, _I_, _I_, _I_, _P_, _LL_, _I_,
                                    _P_, _LL_, _P_, _LL_, _LL_, _I_, _P_, _LL_, _LL_, _I_, _I_, _P_])
_lib.register("hfa_gemm_tuning", [_I_, _I_])
_lib.register("hfa_gemm_kernel_name", [_I_, _I_, _I_, _I_, _I_, _P_, _LL_, _LL_, _I_, _I_, _I_, _I_, _I_, _P_, _LL_,
                                       _I_, _P_, _LL_, _P_, _LL_, _LL_, _I_, _P_, _LL_, _LL_, _I_, _I_], ctypes.c_char_p)
_lib.register("hfa_conv_gemm_split", [_I_, _I_, _I_, _I_, _I_, _P_, _LL_, _LL_, _LL_, _I_, _I_, _I_, _I_, _I_, _P_,
                                       _LL_, _LL_, _I_, _P_, _LL_, _P_, _LL_, _LL_, _I_, _P_, _LL_, _P_, _P_, _LL_,
                                       _LL_, _LL_, _I_, _I_, _P_, _P_])
_lib.register("hfa_gemm_split_kernel_name", [_I_, _I_, _I_, _I_, _I_, _I_, _I_], ctypes.c_char_p)
_lib.register("hfa_gemm_split_tuning", [_I_])
_lib.register("hfa_split_f16", [_I_, _I_, _P_, _LL_, _P_, _LL_, _LL_, _P_, _P_])
_lib.register("hfa_gemm_f32", [_I_, _I_, _I_, _P_, _I_, _P_, _I_, _P_, _P_, _I_, _P_, _I_, _I_, _P_])
_lib.register("hfa_attention_f32", [_I_, _I_, _I_, _I_, _F_, _P_, _LL_, _I_, _P_, _LL_, _I_, _P_, _LL_, _I_, _P_,
                                    _LL_, _I_, _P_, _P_])
_lib.register("hfa_attention_split", [_I_, _I_, _I_, _I_, _F_, _P_, _LL_, _LL_, _I_, _P_, _LL_, _LL_, _I_, _P_, _LL_,
                                      _LL_, _I_, _P_, _LL_, _LL_, _I_, _P_, _P_])
_lib.register("hfa_attention_split_tuning", [_I_])
_lib.register("hfa_attention_split_form", [_I_])
_lib.register("hfa_attention_split_kernel_name", [_I_, _I_, _I_], ctypes.c_char_p)
_lib.register("hfa_layernorm_split", [_I_, _I_, _P_, _LL_, _P_, _LL_, _P_, _P_, _F_, _I_, _P_, _LL_, _I_, _P_, _P_, _LL_,
                                      _LL_, _P_, _P_])
_lib.register("hfa_layernorm_f32",[_I_, _I_, _P_, _LL_, _P_, _LL_, _P_, _P_, _F_, _I_, _P_, _LL_, _I_, _P_, _P_])
_lib.register("hfa_groupnorm_f32", [_I_, _I_, _I_, _I_, _P_, _LL_, _I_, _P_, _P_, _F_, _I_, _P_, _LL_, _I_, _P_,
                                    _P_, _P_])
_lib.register("hfa_groupnorm_workspace_bytes", [_I_, _I_, _I_, _I_], ctypes.c_longlong)
_lib.register("hfa_groupnorm_split", [_I_, _I_, _I_, _I_, _P_, _LL_, _I_, _P_, _P_, _F_, _I_, _P_, _LL_, _I_, _P_, _P_,
                                      _LL_, _I_, _LL_, _P_, _P_, _P_])
_lib.register("hfa_conv0_workspace_bytes", [_I_, _I_], ctypes.c_longlong)
_lib.register("hfa_conv0_f32", [_I_, _I_, _P_, _LL_, _P_, _P_, _I_, _P_, _P_, _F_, _P_, _P_, _LL_, _P_, _P_])
_lib.register("hfa_conv0_split", [_I_, _I_, _P_, _LL_, _P_, _P_, _I_, _P_, _P_, _F_, _P_, _P_, _LL_, _LL_, _P_, _P_,
                                   _P_])
_lib.register("hfa_units_gather_f32", [_I_, _I_, _I_, _P_, _LL_, _I_, _I_, _I_, _F_, _P_, _LL_, _I_, _P_, _P_, _P_])
_lib.register("hfa_mask_rows_f32", [_I_, _I_, _I_, _P_, _LL_, _I_, _P_, _P_])
_lib.register("hfa_wav_normalize_f32", [_I_, _I_, _P_, _LL_, _F_, _P_, _LL_, _P_, _P_, _P_])
_lib.register("hfa_wav_normalize_workspace_bytes", [_I_], ctypes.c_longlong)
_lib.register("hfa_pad_rows_f32", [_I_, _I_, _P_, _LL_, _I_, _I_, _P_, _LL_, _P_])
_lib.register("hfa_add_f32", [_LL_, _P_, _P_, _P_, _P_])
_lib.register("hfa_selftest_erf", [_LL_, _P_, _P_, _P_, _P_])
_lib.register("hfa_selftest_gelu", [_LL_, _P_, _P_, _P_])
_lib.register("hfa_resample_workspace_bytes", [_I_, _I_, _I_, _I_], ctypes.c_longlong)
_lib.register("hfa_resample_f32", [_I_, _I_, _P_, _LL_, _I_, _I_, _P_, _I_, _I_, _P_, _P_, _LL_, _P_])


class KernelProbe:
    """Times every launch of the watched kernels with HIP events on the launching stream (bench.py).

    ``name`` is the rocprof kernel symbol stem of the dominant kernel, e.g. ``gemm_f32_kernel<1, true, ...>``;
    ``extra`` names further kernels to time (the DP, conv0, attention).  Per launch the algorithmic work (FLOPs
    for MFMA kernels, bytes for HBM/latency-bound ones) is recorded next to the event pair, so
    achieved = sum(work) / sum(durations).  Census mode (name None) times nothing and tallies FLOPs per
    MFMA instantiation so bench.py can pick the dominant one."""

    def __init__(self, name: str | None, extra=()):
        self.name = name
        self.watch = set(extra) | ({name} if name else set())
        self.records = {}
        self.census = {}
        self.active = True           # False: launches pass through untimed (bench.py samples the timed steps)

    def dominant(self) -> str:
        return max(self.census, key=self.census.get)

    def __call__(self, name: str, work: float, launch, kind: str = "flops", shape=None, units=None, label=None):
        if self.name is None:
            if kind == "flops":
                self.census[name] = self.census.get(name, 0.0) + work
            return launch()
        if name not in self.watch or not self.active:
            return launch()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        launch()
        e.record()
        self.records.setdefault(name, []).append((s, e, work, units))

    def summary(self, name: str | None = None):
        """launches, total / average ms, work; ``units`` = the launches' own units (the DP's time steps) when
        every launch reported them, else None."""
        torch.cuda.synchronize()
        recs = self.records.get(name or self.name, [])
        n = len(recs)
        ms = sum(s.elapsed_time(e) for s, e, _, _ in recs)
        w = sum(f for _, _, f, _ in recs)
        u = sum(x for *_, x in recs) if recs and all(x is not None for *_, x in recs) else None
        return {"launches": n, "total_ms": ms, "avg_ms": ms / max(n, 1), "work": w, "avg_work": w / max(n, 1),
                "flops": w, "avg_flops": w / max(n, 1), "units": u}


PROBE = None


def _gemm_name(*args) -> str:
    """rocprof symbol stem of the instantiation hfa_conv_gemm_f32 dispatches to for these arguments (the
    library answers from the same plan it launches)."""
    return _lib.lib().hfa_gemm_kernel_name(*args).decode()


def conv_gemm(A, W, C, *, M, N, K, Zb=1, G=1, sAb=0, sAg=0, ldx, stride=1, pad=0, Cg=None, Tin=None, sWg=0,
              ldw=None, bias=None, sBg=0, R=None, sRb=0, sRg=0, ldr=0, sCb=0, sCg=0, ldc, epilogue=EPI_NONE):
    """Implicit-GEMM conv / Linear on MFMA (see gemm.hip for the exact A/W/C addressing)."""
    for t, n in ((A, "A"), (W, "W"), (C, "C")):
        _need(t, torch.float32, n, contiguous=False)

    args = (M, N, K, Zb, G, _ptr(A), sAb, sAg, ldx, stride, pad, Cg or K, Tin if Tin is not None else M, _ptr(W),
            sWg, ldw if ldw is not None else K, _ptr(bias), sBg, _ptr(R), sRb, sRg, ldr, _ptr(C), sCb, sCg, ldc,
            epilogue)

    def launch():
        _lib.call("hfa_conv_gemm_f32", *args, _stream(C.device))
    if PROBE is None:
        return launch()
    PROBE(_gemm_name(*args), 2.0 * M * N * K * Zb * G, launch)


def linear(x, W, bias=None, residual=None, out=None, epilogue=EPI_NONE):
    """y = epi(x @ W^T + bias) (+ residual); x [..., K] rows contiguous, W [N, K] contiguous."""
    K = x.shape[-1]
    N = W.shape[0]
    x2 = x.reshape(-1, K)
    M = x2.shape[0]
    if out is None:
        out = torch.empty((*x.shape[:-1], N), dtype=torch.float32, device=x.device)
    o2 = out.view(-1, N)
    r2 = residual.reshape(-1, N) if residual is not None else None
    _need(W, torch.float32, "W")

    args = (M, N, K, _ptr(x2), x2.stride(0), _ptr(W), W.stride(0), _ptr(bias), _ptr(r2),
            r2.stride(0) if r2 is not None else 0, _ptr(o2), o2.stride(0), epilogue)

    def launch():
        _lib.call("hfa_gemm_f32", *args, _stream(x.device))
    if PROBE is None:
        launch()
    else:                       # hfa_gemm_f32 is hfa_conv_gemm_f32 with Zb = G = 1, stride 1, Cg = K, Tin = M
        PROBE(_gemm_name(M, N, K, 1, 1, _ptr(x2), 0, 0, x2.stride(0), 1, 0, K, M, _ptr(W), 0, W.stride(0), _ptr(bias),
                         0, _ptr(r2), 0, 0, r2.stride(0) if r2 is not None else 0, _ptr(o2), 0, 0, o2.stride(0),
                         epilogue), 2.0 * M * N * K, launch)
    return out


# ---- split-f16 operands (gemm.hip gemm_split_kernel) ----------------------------------------------------------
# A split tensor is a float16 tensor [2, *shape]: plane 0 = f16(x), plane 1 = f16((x - plane0) * 2^11).
_OFLOW = {}


def split_flag(device) -> torch.Tensor:
    """Device int32 flag the split producers raise when a value leaves f16 range (|x| >= 65504 / non-finite);
    the caller re-runs that batch on the f32 path (see task.ForcedAlignmentTask)."""
    key = torch.device(device)
    if key.type == "cuda" and key.index is None:
        key = torch.device("cuda", torch.cuda.current_device())
    if key not in _OFLOW:
        _OFLOW[key] = torch.zeros(1, dtype=torch.int32, device=key)
    return _OFLOW[key]


def split(x, out=None, flag=None):
    """f32 [..., C] (row-strided) -> split planes [2, ..., C]; out-of-range values raise ``flag`` (default: the
    device's split_flag)."""
    _need(x, torch.float32, "x", contiguous=False)
    C = x.shape[-1]
    x2 = x.reshape(-1, C) if x.dim() != 2 else x
    if x2.stride(-1) != 1:
        raise ValueError("split: last dim must be contiguous")
    rows = x2.shape[0]
    if out is None:
        out = torch.empty((2, *x.shape), dtype=torch.float16, device=x.device)
    o2 = out.view(2, rows, C)
    _lib.call("hfa_split_f16", rows, C, _ptr(x2), x2.stride(0), _ptr(o2), o2.stride(1), o2.stride(0),
              _ptr(split_flag(x.device) if flag is None else flag), _stream(x.device))
    return out


def _split_name(M, N, K, Z, out_split, epilogue, Cg) -> str:
    return _lib.lib().hfa_gemm_split_kernel_name(M, N, K, Z, int(out_split), epilogue, Cg).decode()


def conv_gemm_split(As, Ws, C=None, Cs=None, *, M, N, K, Zb=1, G=1, sAb=0, sAg=0, ldx, stride=1, pad=0, Cg=None,
                    Tin=None, sWg=0, ldw=None, bias=None, sBg=0, R=None, sRb=0, sRg=0, ldr=0, sCb=0, sCg=0, ldc,
                    epilogue=EPI_NONE, flag=None, f16=False):
    """conv_gemm on split operands (As, Ws: [2, ...] f16 planes; strides in elements of one plane).  Output to f32
    C (+R), to split planes Cs [2, ...] (bias/GELU epilogue only), or both (dual: the planes of the final C).
    R may be f32 or split planes [2, ...] f16 (f32 C alone; its strides in halves of one plane).
    ``f16``: the opt-in fast mode (high planes only, one f16 product per MAC: f16-class accuracy)."""
    Rs = None
    if R is not None and R.dtype == torch.float16:
        R, Rs = None, R
    if f16:
        epilogue |= GEMM_F16
    _need(As, torch.float16, "As", contiguous=False)
    _need(Ws, torch.float16, "Ws", contiguous=False)
    if C is None and Cs is None:
        raise ValueError("conv_gemm_split: C and / or Cs")
    dev = (C if C is not None else Cs).device
    args = (M, N, K, Zb, G, _ptr(As), As.stride(0), sAb, sAg, ldx, stride, pad, Cg or K, Tin if Tin is not None else M,
            _ptr(Ws), Ws.stride(0), sWg, ldw if ldw is not None else K, _ptr(bias), sBg, _ptr(R), sRb, sRg, ldr,
            _ptr(Rs), Rs.stride(0) if Rs is not None else 0,
            _ptr(C), _ptr(Cs), Cs.stride(0) if Cs is not None else 0, sCb, sCg, ldc, epilogue,
            _ptr(split_flag(dev) if flag is None else flag))

    def launch():
        _lib.call("hfa_conv_gemm_split", *args, _stream(dev))
    if PROBE is None:
        return launch()
    PROBE(_split_name(M, N, K, Zb * G, Cs is not None and C is None, epilogue, Cg or K), 2.0 * M * N * K * Zb * G, launch,
          shape=(M, N, K, Zb * G))


def linear_split(xs, Ws, bias=None, residual=None, out=None, epilogue=EPI_NONE, out_split=False, flag=None,
                 f16=False):
    """y = epi(x @ W^T + bias) (+ residual) with x, W given as split planes [2, ..., K] / [2, N, K]; y f32, or split
    planes [2, ..., N] when out_split (no residual), or both as (y, planes) when out_split == "dual"."""
    K = xs.shape[-1]
    N = Ws.shape[1]
    lead = xs.shape[1:-1]
    M = 1
    for d in lead:
        M *= d
    dual = out_split == "dual"
    planes = out_split and not dual
    if out is None:
        out = torch.empty(((2,) if planes else ()) + (*lead, N), dtype=torch.float16 if planes else torch.float32,
                          device=xs.device)
    hs = torch.empty((2, *lead, N), dtype=torch.float16, device=xs.device) if dual else None
    if residual is None:
        r2 = None
    elif residual.dtype == torch.float16:                  # split planes [2, ..., N] (a LayerNorm's plane output)
        r2 = residual.reshape(2, -1, N)
    else:
        r2 = residual.reshape(-1, N)
    conv_gemm_split(xs, Ws, C=None if planes else out, Cs=out if planes else hs, M=M, N=N, K=K,
                    ldx=xs.stride(-2) if xs.dim() > 2 else K, bias=bias, R=r2, ldr=r2.stride(-2) if r2 is not None else 0,
                    ldc=N, epilogue=epilogue, flag=flag, f16=f16)
    return (out, hs) if dual else out


def _lens(lens):
    """Optional per-row lengths of a variable-length batch: None or an int32 device tensor [B]."""
    if lens is None:
        return None
    _need(lens, torch.int32, "lengths")
    return lens


def attention(q, k, v, out, *, B, H, L, head_dim, scale, q_bs, q_ld, k_bs, k_ld, v_bs, v_ld, o_bs, o_ld,
              key_len=None):
    """Flash attention; ``key_len`` [B] int32 (optional): per-row lengths (keys and queries beyond are padding)."""
    kl = _lens(key_len)

    def launch():
        _lib.call("hfa_attention_f32", B, H, L, head_dim, float(scale), _ptr(q), q_bs, q_ld, _ptr(k), k_bs, k_ld,
                  _ptr(v), v_bs, v_ld, _ptr(out), o_bs, o_ld, _ptr(kl), _stream(out.device))
    if PROBE is None:
        launch()
    else:                       # QK^T and PV: 2 * 2 * L * L * head_dim per (batch, head)
        PROBE("attn_fwd_f32_kernel", 4.0 * B * H * L * L * head_dim, launch, kind="flops_aux")
    return out


def attention_split(qkv_s, out_s, *, B, H, L, head_dim, scale, key_len=None):
    """Flash attention on split planes (attention.hip attn_fwd_split16_kernel / attn_fwd_split_kernel): ``qkv_s``
    [2, B, L, 3*H*head_dim] f16 planes of the fused QKV projection (Q | K | V column blocks), ``out_s``
    [2, B, L, H*head_dim] planes."""
    _need(qkv_s, torch.float16, "qkv_s")
    _need(out_s, torch.float16, "out_s")
    D = H * head_dim
    if qkv_s.shape != (2, B, L, 3 * D) or out_s.shape != (2, B, L, D):
        raise ValueError(f"attention_split: qkv_s {tuple(qkv_s.shape)} / out_s {tuple(out_s.shape)} do not match "
                         f"B={B} L={L} H={H} head_dim={head_dim}")
    kl = _lens(key_len)
    sp, bs, ld = qkv_s.stride(0), qkv_s.stride(1), qkv_s.stride(2)
    base = qkv_s.data_ptr()

    def launch():
        _lib.call("hfa_attention_split", B, H, L, head_dim, float(scale), _P(base), sp, bs, ld, _P(base + 2 * D),
                  sp, bs, ld, _P(base + 4 * D), sp, bs, ld, _ptr(out_s), out_s.stride(0), out_s.stride(1),
                  out_s.stride(2), _ptr(kl), _stream(out_s.device))
    if PROBE is None:
        launch()
    else:
        PROBE(attention_split_probe_name(), 4.0 * B * H * L * L * head_dim, launch, kind="flops_aux",
              shape=(B, H, L, head_dim))
    return out_s


def attention_split_probe_name() -> str:
    """rocprof symbol stem of the split attention the library launches under the current MFMA form
    (hfa_attention_split_form): "attn_fwd_split16_kernel" (16x16x32, the default) or "attn_fwd_split_kernel"."""
    return _lib.lib().hfa_attention_split_kernel_name(1, 1, 1).decode().split("<")[0]


def layernorm(x, gamma, beta, eps=1e-5, act=ACT_NONE, out=None, residual=None, t_len=None, out_split=None,
              flag=None):
    """Row LayerNorm (+act) over the last dim; with ``t_len`` [B] (x is [B, T, C]) rows t >= t_len[b] -> 0.
    ``out_split`` ([2, ..., C] f16, or True to allocate): the output also as split planes (returned second)."""
    C = x.shape[-1]
    x2 = x.reshape(-1, C)
    if out is False:                                      # split planes only (out_split required)
        if out_split is None or out_split is False:
            raise ValueError("layernorm: out=False needs out_split")
        o2 = None
    else:
        if out is None:
            out = torch.empty_like(x)
        o2 = out.view(-1, C)
    r2 = residual.reshape(-1, C) if residual is not None else None
    tl = _lens(t_len)
    T = x.shape[-2] if (tl is not None and x.dim() == 3) else 0
    if out_split is None or out_split is False:
        _lib.call("hfa_layernorm_f32", x2.shape[0], C, _ptr(x2), x2.stride(0), _ptr(r2),
                  r2.stride(0) if r2 is not None else 0, _ptr(gamma), _ptr(beta), float(eps), act, _ptr(o2),
                  o2.stride(0), T, _ptr(tl), _stream(x.device))
        return out
    if out_split is True:
        out_split = torch.empty((2, *x.shape), dtype=torch.float16, device=x.device)
    _need(out_split, torch.float16, "out_split")
    s2 = out_split.view(2, -1, C)
    _lib.call("hfa_layernorm_split", x2.shape[0], C, _ptr(x2), x2.stride(0), _ptr(r2),
              r2.stride(0) if r2 is not None else 0, _ptr(gamma), _ptr(beta), float(eps), act, _ptr(o2),
              o2.stride(0) if o2 is not None else 0, T, _ptr(tl), _ptr(s2), s2.stride(1), s2.stride(0),
              _ptr(split_flag(x.device) if flag is None else flag), _stream(x.device))
    return (None if o2 is None else out), out_split


def groupnorm(x, G, gamma, beta, eps=1e-5, act=ACT_NONE, out=None, t_len=None, out_split=None, flag=None):
    """GroupNorm over channels-last x [B, T, C] (stats over T x C/G per group; over t_len[b] rows if given,
    padding rows -> 0).  ``out_split`` ([2, B, T, C] f16, or True to allocate): write split planes; with
    ``out=False`` the planes only (no f32 output).  Returns the f32 output, the planes, or (f32, planes)."""
    B, T, C = x.shape
    tl = _lens(t_len)
    ws = torch.empty(max(1, int(_lib.lib().hfa_groupnorm_workspace_bytes(B, T, C, G))), dtype=torch.uint8,
                     device=x.device)
    if out_split is None or out_split is False:
        if out is None:
            out = torch.empty_like(x)
        _lib.call("hfa_groupnorm_f32", B, T, C, G, _ptr(x), x.stride(0), x.stride(1), _ptr(gamma), _ptr(beta),
                  float(eps), act, _ptr(out), out.stride(0), out.stride(1), _ptr(tl), _ptr(ws), _stream(x.device))
        return out
    if out_split is True:
        out_split = torch.empty((2, B, T, C), dtype=torch.float16, device=x.device)
    _need(out_split, torch.float16, "out_split", contiguous=False)
    if out is None:
        out = torch.empty_like(x)
    y = None if out is False else out
    _lib.call("hfa_groupnorm_split", B, T, C, G, _ptr(x), x.stride(0), x.stride(1), _ptr(gamma), _ptr(beta),
              float(eps), act, _ptr(y), y.stride(0) if y is not None else 0, y.stride(1) if y is not None else 0,
              _ptr(tl), _ptr(out_split), out_split.stride(1), out_split.stride(2), out_split.stride(0),
              _ptr(split_flag(x.device) if flag is None else flag), _ptr(ws), _stream(x.device))
    return out_split if y is None else (y, out_split)


def conv0(x, w0, *, bias=None, gamma=None, beta=None, eps=1e-5, out=None, workspace=None, t0_len=None,
          out_split=False):
    """First extractor conv (1->512, k10, s5) -> [B, T0, 512]; GroupNorm+GELU when gamma/beta are given
    (statistics over t0_len[b] frames if given).  out_split: the output as split-f16 planes [2, B, T0, 512]."""
    B, N = x.shape
    T0 = (N - 10) // 5 + 1
    if out is None:
        out = torch.empty(((2,) if out_split else ()) + (B, T0, 512),
                          dtype=torch.float16 if out_split else torch.float32, device=x.device)
    norm = gamma is not None
    if norm and workspace is None:
        nbytes = _lib.lib().hfa_conv0_workspace_bytes(B, N)
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    tl = _lens(t0_len)

    def launch():
        if out_split:
            _lib.call("hfa_conv0_split", B, N, _ptr(x), x.stride(0), _ptr(w0), _ptr(bias), 1 if norm else 0,
                      _ptr(gamma), _ptr(beta), float(eps), _ptr(workspace), _ptr(out), out.stride(1), out.stride(0),
                      _ptr(split_flag(x.device)), _ptr(tl), _stream(x.device))
        else:
            _lib.call("hfa_conv0_f32", B, N, _ptr(x), x.stride(0), _ptr(w0), _ptr(bias), 1 if norm else 0,
                      _ptr(gamma), _ptr(beta), float(eps), _ptr(workspace), _ptr(out), out.stride(0), _ptr(tl),
                      _stream(x.device))
    if PROBE is None:
        launch()
    else:                       # wave in (4 B/sample) + activations out (4 B x 512 x T0)
        PROBE("hfa_conv0_split" if out_split else "hfa_conv0_f32", B * (4.0 * N + 4.0 * 512 * T0), launch,
              kind="bytes")
    return out


def units_gather(units, n_frames, T_pad, ratio, out=None, n_frames_b=None, U_b=None):
    B, U, C = units.shape
    if out is None:
        out = torch.empty((B, T_pad, C), dtype=torch.float32, device=units.device)
    nf, ub = _lens(n_frames_b), _lens(U_b)
    _lib.call("hfa_units_gather_f32", B, U, C, _ptr(units), units.stride(0), units.stride(1), n_frames, T_pad,
              float(ratio), _ptr(out), out.stride(0), out.stride(1), _ptr(nf), _ptr(ub), _stream(units.device))
    return out


def mask_rows(x, lens):
    """Zero rows t >= lens[b] of x [B, T, C] (or [B, N] as C = 1), in place."""
    ln = _lens(lens)
    if x.dim() == 2:
        B, T = x.shape
        C, ld = 1, 1
    else:
        B, T, C = x.shape
        ld = x.stride(1)
    _lib.call("hfa_mask_rows_f32", B, T, C, _ptr(x), x.stride(0), ld, _ptr(ln), _stream(x.device))
    return x


def wav_normalize(x, eps=1e-7, out=None, lens=None):
    B, N = x.shape
    if out is None:
        out = torch.empty_like(x)
    ln = _lens(lens)
    ws = torch.empty(max(1, int(_lib.lib().hfa_wav_normalize_workspace_bytes(B))), dtype=torch.uint8,
                     device=x.device)
    _lib.call("hfa_wav_normalize_f32", B, N, _ptr(x), x.stride(0), float(eps), _ptr(out), out.stride(0), _ptr(ln),
              _ptr(ws), _stream(x.device))
    return out


def pad_rows(x, left, n_out, out=None):
    B, N = x.shape
    if out is None:
        out = torch.empty((B, n_out), dtype=torch.float32, device=x.device)
    _lib.call("hfa_pad_rows_f32", B, N, _ptr(x), x.stride(0), left, n_out, _ptr(out), out.stride(0),
              _stream(x.device))
    return out


_lib.register("hfa_flag_take", [_I_, _P_, _P_, _P_])


def flag_take(flag: torch.Tensor) -> torch.Tensor:
    """Snapshot of a device int32 flag tensor, which is cleared (stream-ordered, one launch)."""
    _need(flag, torch.int32, "flag")
    snap = torch.empty_like(flag)
    _lib.call("hfa_flag_take", flag.numel(), _ptr(flag), _ptr(snap), _stream(flag.device))
    return snap


_lib.register("hfa_set_grid_cap", [_I_])


@contextlib.contextmanager
def grid_cap(wgs: int):
    """Launches of the row-streaming kernels (split_f16, LayerNorm, lattice / CTC prologue) made by this thread inside the
    block use at most ``wgs`` workgroups (hfa_set_grid_cap; results identical)."""
    _lib.call("hfa_set_grid_cap", int(wgs))
    try:
        yield
    finally:
        _lib.call("hfa_set_grid_cap", 0)


def add(a, b, out=None):
    if out is None:
        out = torch.empty_like(a)
    _lib.call("hfa_add_f32", a.numel(), _ptr(a), _ptr(b), _ptr(out), _stream(a.device))
    return out


_lib.register("hfa_resample_split_workspace_bytes", [_I_, _I_, _I_, _I_, _I_], ctypes.c_longlong)
_lib.register("hfa_resample_split", [_I_, _I_, _P_, _LL_, _I_, _I_, _P_, _I_, _I_, _I_, _P_, _P_, _LL_, _P_, _P_])


def resample_split(x, orig, new, w_planes, G, width, out=None, workspace=None, flag=None, n_out=None):
    """Sinc resample rows of x [B, N] (row stride free, unit element stride) on the split-f16 GEMM; w_planes
    [2, G, new, Kg] (resample.Resampler builds them).  Returns the [B, ceil(new*N/orig)] view of the output (``n_out``
    columns instead: resample.ChainResampler, whose composite filter's length is the two stages')."""
    _need(x, torch.float32, "x", contiguous=False)
    if x.stride(-1) != 1:
        raise ValueError("resample_split: rows must have unit stride")
    B, N = x.shape
    Kg = w_planes.shape[-1]
    F = N // orig + 1
    cols = F * new if G == 1 else -(-F // 8) * 8 * new
    if out is None:
        out = torch.empty((B, cols), dtype=torch.float32, device=x.device)
    if workspace is None:
        nbytes = _lib.lib().hfa_resample_split_workspace_bytes(B, N, orig, Kg, G)
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    def launch():
        _lib.call("hfa_resample_split", B, N, _ptr(x), x.stride(0), orig, new, _ptr(w_planes), Kg, G, width,
                  _ptr(workspace), _ptr(out), out.stride(0), _ptr(split_flag(x.device) if flag is None else flag),
                  _stream(x.device))
    if PROBE is None:
        launch()
    else:      # (its GEMM shares an instantiation with the encoder's: reported outside the dominant-kernel census)
        rows = F if G == 1 else -(-F // 8)
        PROBE(_split_name(rows, new, Kg, B * G, False, 0, Kg), 2.0 * rows * new * Kg * B * G, launch,
              kind="flops_aux", shape=(rows, new, Kg, B * G),
              label="resampler chain (one pass)" if orig == new else f"resampler {orig} -> {new} (reduced rates)")
    from .resample import target_length
    return out[:, : target_length(N, orig, new) if n_out is None else n_out]


_lib.register("hfa_resample_chain_edges_workspace_bytes", [_I_, _I_, _I_, _I_], restype=_LL_)
_lib.register("hfa_resample_chain_edges", [_I_, _I_, _P_, _P_, _LL_, _I_, _I_, _P_, _I_, _I_, _P_, _I_, _I_, _P_, _P_,
                                            _LL_, _I_, _P_])


def resample_chain_edges(x, lens, P, Q, wu_t, wu_width, wd_t, wd_width, y):
    """Overwrite the edge frames of a composite two-stage resample y [B, >= cols] (hfa_resample_chain_edges): x
    [B, N] the input rows, ``lens`` an int32 device tensor of per-row input lengths or None (all N)."""
    _need(x, torch.float32, "x", contiguous=False)
    _need(y, torch.float32, "y", contiguous=False)
    if x.stride(-1) != 1 or y.stride(-1) != 1:
        raise ValueError("resample_chain_edges: rows must have unit stride")
    B, N = x.shape
    nbytes = _lib.lib().hfa_resample_chain_edges_workspace_bytes(B, Q, wd_t.shape[0], wd_width)
    ws = torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=x.device)
    _lib.call("hfa_resample_chain_edges", B, N, _ptr(lens) if lens is not None else None, _ptr(x), x.stride(0), P, Q,
              _ptr(wu_t), wu_t.shape[0], wu_width, _ptr(wd_t), wd_t.shape[0], wd_width, _ptr(ws), _ptr(y), y.stride(0),
              y.shape[1], _stream(x.device))


def resample(x, orig, new, kernel, width, out=None, workspace=None):
    """Sinc resample rows of x [B, N] (gcd-reduced orig/new rates); returns [B, ceil(new*N/orig)] view."""
    B, N = x.shape
    Kpad = kernel.shape[1]
    F = N // orig + 1
    if out is None:
        out = torch.empty((B, F * new), dtype=torch.float32, device=x.device)
    if workspace is None:
        nbytes = _lib.lib().hfa_resample_workspace_bytes(B, N, orig, Kpad)
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    _lib.call("hfa_resample_f32", B, N, _ptr(x), x.stride(0), orig, new, _ptr(kernel), Kpad, width,
              _ptr(workspace), _ptr(out), out.stride(0), _stream(x.device))
    from .resample import target_length
    return out[:, : target_length(N, orig, new)]


_lib.register("hfa_logmel_split", [_I_, _I_, _P_, _LL_, _P_, _I_, _I_, _I_, _I_, _I_, _P_, _P_, _F_, _I_, _P_, _LL_,
                                   _I_, _P_, _P_])


def logmel_split(x, basis, fb, *, win_length, hop_length, n_fft, n_mels, clamp, lens=None, out=None, flag=None):
    """Log-mel spectrogram of the rows of x [B, N] (row stride free, unit element stride) in one fused kernel
    (hfa_logmel_split); ``basis`` / ``fb`` are the fragment-order split tables melspec.MelSpecExtractor builds
    (fb [2, 8, nb_pad / 32, 64, 8]).  ``lens``: optional int32 device tensor of per-row lengths.  Returns
    [B, n_mels, N // hop_length + 1]; out-of-range magnitudes raise ``flag`` (default: the device's split_flag)."""
    _need(x, torch.float32, "x", contiguous=False)
    if x.dim() != 2 or x.stride(-1) != 1:
        raise ValueError("logmel_split: x must be [B, N] with unit element stride")
    _need(basis, torch.float16, "basis")
    _need(fb, torch.float16, "fb")
    B, N = x.shape
    frames = N // hop_length + 1
    nb_pad, kpad = fb.shape[2] * 32, (win_length + 127) // 128 * 128
    if tuple(fb.shape) != (2, 8, nb_pad // 32, 64, 8) or tuple(basis.shape) != (2, nb_pad // 8, kpad // 32, 64, 8):
        raise ValueError("logmel_split: basis / fb are not the tables of this configuration")   # the kernel trusts them
    if out is None:
        out = torch.empty((B, n_mels, frames), dtype=torch.float32, device=x.device)
    _lib.call("hfa_logmel_split", B, N, _ptr(x), x.stride(0) if B > 1 else 0, _ptr(_lens(lens)), win_length,
              hop_length, n_fft, n_mels, nb_pad, _ptr(basis), _ptr(fb), float(clamp), frames, _ptr(out),
              out.stride(0), out.stride(1),
              _ptr(split_flag(x.device) if flag is None else flag), _stream(x.device))
    return out


# ------------------------------------------------------------------------------------------------------------
# CTC head (ctc.hip): gathered log-softmax + argmax, batched sequence likelihood, greedy decode
# ------------------------------------------------------------------------------------------------------------
_lib.register("hfa_ctc_max_labels", [])
_lib.register("hfa_ctc_prologue", [_I_, _I_, _I_, _I_, _P_, _P_, _P_, _LL_, _LL_, _I_, _I_, _P_, _P_, _P_, _P_])
_lib.register("hfa_ctc_forward", [_I_, _I_, _I_, _P_, _P_, _P_, _P_, _P_, _P_])
_lib.register("hfa_ctc_greedy", [_I_, _I_, _P_, _P_, _P_, _P_, _P_])

CTC_BLANK_COL, CTC_LABEL_OFF = 1, 2      # the head's layout: [edge, ctc blank, frame class 0, class 1 (= ctc 1), ...]
CTC_MAX_V = 1024                         # ctc.hip kMaxV


def ctc_check_targets(T, targets, L, V):
    """Host validation of a CTC batch (the kernels trust it): T / L [B] non-negative ints, targets [B, >= max L] with
    every used id in 1..V-1 (0 is the blank; the binarizer drops it, binarize.py:197-198).  Returns int32 numpy arrays
    (T [B], L [B], targets [B, Lmax]) with Lmax = max L; unused target slots are zeros."""
    import numpy as np
    T = np.asarray(T.cpu() if isinstance(T, torch.Tensor) else T, dtype=np.int64).reshape(-1)
    L = np.asarray(L.cpu() if isinstance(L, torch.Tensor) else L, dtype=np.int64).reshape(-1)
    B = T.shape[0]
    if L.shape[0] != B:
        raise ValueError(f"ctc: T has {B} rows, L has {L.shape[0]}")
    if not 0 < int(V) <= CTC_MAX_V:
        raise ValueError(f"ctc: V = {V} classes is outside 1..{CTC_MAX_V}")
    if B and (T.min() < 0 or L.min() < 0):
        raise ValueError("ctc: negative length")
    Lmax = int(L.max()) if B else 0
    out = np.zeros((B, Lmax), np.int32)
    if isinstance(targets, torch.Tensor):
        targets = targets.cpu().numpy()
    for b in range(B):
        row = np.asarray(targets[b], dtype=np.int64).reshape(-1)
        n = int(L[b])
        if row.shape[0] < n:
            raise ValueError(f"ctc: row {b} has {row.shape[0]} targets, L says {n}")
        row = row[:n]
        if n and (row.min() < 1 or row.max() >= V):
            bad = row[(row < 1) | (row >= V)][0]
            raise ValueError(f"ctc: row {b} has target id {int(bad)} outside 1..{int(V) - 1}")
        out[b, :n] = row
    return T.astype(np.int32), L.astype(np.int32), out


def _ctc_logits(logits, V, blank_col, label_off):
    _need(logits, torch.float32, "logits", contiguous=False)
    if logits.dim() != 3 or logits.stride(2) != 1:
        raise ValueError("ctc: logits must be [B, T, C] with unit stride in the last dim")
    C = logits.shape[2]
    if not 0 < V <= CTC_MAX_V or not 0 <= blank_col < C or label_off < -1 or (V > 1 and V - 1 + label_off >= C):
        raise ValueError(f"ctc: V = {V}, blank_col = {blank_col}, label_off = {label_off} do not fit {C} columns")


def ctc_prologue(logits, T, L, targets, V=None, blank_col=CTC_BLANK_COL, label_off=CTC_LABEL_OFF):
    """log_softmax over the V CTC classes of every frame, gathered to the transcript, and the argmax class
    (hfa_ctc_prologue).  logits [B, Tmax, C] f32 (a strided view is fine; class c in column blank_col if c == 0 else
    c + label_off; V defaults to C - 2, the head's layout), T / L [B] i32, targets [B, Lmax] i32 with ids in 1..V-1
    (NOT checked here: ctc_check_targets / ctc_score do).  Returns (emis [B, Tmax, Lmax + 1] f32, best [B, Tmax] i32);
    rows t >= T[b] and columns j > L[b] are left unwritten."""
    B, Tmax, C = logits.shape
    V = C - 2 if V is None else int(V)
    _ctc_logits(logits, V, blank_col, label_off)
    for t, n in ((T, "T"), (L, "L"), (targets, "targets")):
        _need(t, torch.int32, n)
    if T.shape != (B,) or L.shape != (B,) or targets.dim() != 2 or targets.shape[0] != B:
        raise ValueError("ctc_prologue: T / L must be [B] and targets [B, Lmax]")
    Lmax = targets.shape[1]
    dev = logits.device
    emis = torch.empty((B, Tmax, Lmax + 1), dtype=torch.float32, device=dev)
    best = torch.empty((B, Tmax), dtype=torch.int32, device=dev)
    _lib.call("hfa_ctc_prologue", B, Tmax, V, Lmax, _ptr(T), _ptr(L), _ptr(logits), logits.stride(1),
              logits.stride(0), blank_col, label_off, _ptr(targets) if Lmax else None, _ptr(emis), _ptr(best),
              _stream(dev))
    return emis, best


def ctc_forward(emis, T, L, targets):
    """-log P(targets | frames) per utterance as f64 [B] (hfa_ctc_forward; +inf for an infeasible pair): emis
    [B, Tmax, Lmax + 1] from ctc_prologue, T / L [B] i32, targets [B, Lmax] i32."""
    _need(emis, torch.float32, "emis")
    for t, n in ((T, "T"), (L, "L"), (targets, "targets")):
        _need(t, torch.int32, n)
    B, Tmax, Lp = emis.shape
    if T.shape != (B,) or L.shape != (B,) or tuple(targets.shape) != (B, Lp - 1):
        raise ValueError("ctc_forward: T / L must be [B] and targets [B, Lmax] for emis [B, Tmax, Lmax + 1]")
    nll = torch.empty((B,), dtype=torch.float64, device=emis.device)
    _lib.call("hfa_ctc_forward", B, Tmax, Lp - 1, _ptr(T), _ptr(L), _ptr(emis) if Tmax else None,
              _ptr(targets) if Lp > 1 else None, _ptr(nll), _stream(emis.device))
    return nll


def ctc_greedy(best, T):
    """Greedy CTC collapse of the per-frame argmax (hfa_ctc_greedy; alignment_decoder.py:145-150): best [B, Tmax]
    i32, T [B] i32 -> (ids [B, Tmax] i32, n [B] i32), row b valid up to n[b]."""
    _need(best, torch.int32, "best")
    _need(T, torch.int32, "T")
    B, Tmax = best.shape
    if T.shape != (B,):
        raise ValueError("ctc_greedy: T must be [B]")
    ids = torch.empty((B, Tmax), dtype=torch.int32, device=best.device)
    n = torch.empty((B,), dtype=torch.int32, device=best.device)
    _lib.call("hfa_ctc_greedy", B, Tmax, _ptr(T), _ptr(best) if Tmax else None, _ptr(ids) if Tmax else None, _ptr(n),
              _stream(best.device))
    return ids, n


def ctc_score(logits, T, targets, L, V=None, blank_col=CTC_BLANK_COL, label_off=CTC_LABEL_OFF):
    """Score B transcripts against the head's CTC columns: logits [B, Tmax, C] f32 on the GPU (see ctc_prologue), T /
    L [B] and targets [B, >= max L] as host integers (lists, numpy, CPU tensors; device tensors are copied back to be
    checked).  The ids are validated on the host (1..V-1, else ValueError, before anything touches the GPU) and reach
    the device in one pinned non-blocking copy; the workspace comes from torch's allocator.  Returns (nll f64 [B],
    best i32 [B, Tmax], ids i32 [B, Tmax], n i32 [B]) on the device, stream-ordered."""
    if not isinstance(logits, torch.Tensor) or logits.dim() != 3:
        raise TypeError("ctc_score: logits must be a [B, T, C] tensor")
    Vn = logits.shape[2] - 2 if V is None else int(V)
    T_h, L_h, tg_h = ctc_check_targets(T, targets, L, Vn)
    B, Tmax = logits.shape[:2]
    if T_h.shape[0] != B:
        raise ValueError(f"ctc_score: {B} logit rows, {T_h.shape[0]} lengths")
    if B and int(T_h.max()) > Tmax:
        raise ValueError(f"ctc_score: a row's T = {int(T_h.max())} exceeds the {Tmax} logit frames")
    _ctc_logits(logits, Vn, blank_col, label_off)
    Lmax = tg_h.shape[1]
    if Lmax > int(_lib.lib().hfa_ctc_max_labels()):
        raise _lib.HFAArgumentError(f"ctc_score: {Lmax} labels exceed the kernel's {_lib.lib().hfa_ctc_max_labels()}",
                                    _lib.HFA_EINVAL)
    import numpy as np
    meta = torch.from_numpy(np.concatenate([T_h, L_h, tg_h.ravel()])).pin_memory().to(logits.device, non_blocking=True)
    T_t, L_t, tg_t = meta[:B], meta[B:2 * B], meta[2 * B:].view(B, Lmax)
    emis, best = ctc_prologue(logits, T_t, L_t, tg_t, Vn, blank_col, label_off)
    nll = ctc_forward(emis, T_t, L_t, tg_t)
    ids, n = ctc_greedy(best, T_t)
    return nll, best, ids, n


# ---- CTC forward-backward: state posteriors, the per-label report, the loss gradient -----------
_lib.register("hfa_ctc_forward_alpha", [_I_, _I_, _I_, _P_, _P_, _P_, _P_, _P_, _P_, _P_, _P_])
_lib.register("hfa_ctc_backward", [_I_, _I_, _I_, _P_, _P_, _P_, _P_, _P_, _P_, _P_, _P_, _P_, _P_, _P_, _P_])
_lib.register("hfa_ctc_grad", [_I_, _I_, _I_, _I_, _P_, _P_, _P_, _LL_, _LL_, _I_, _I_, _P_, _P_, _P_, _P_, _P_, _P_,
                               _LL_, _LL_, _P_])


def _ctc_meta(emis, T, L, targets, who):
    _need(emis, torch.float32, "emis")
    for t, n in ((T, "T"), (L, "L"), (targets, "targets")):
        _need(t, torch.int32, n)
    B, Tmax, Lp = emis.shape
    if T.shape != (B,) or L.shape != (B,) or tuple(targets.shape) != (B, Lp - 1):
        raise ValueError(f"{who}: T / L must be [B] and targets [B, Lmax] for emis [B, Tmax, Lmax + 1]")
    return B, Tmax, Lp - 1


def ctc_forward_alpha(emis, T, L, targets):
    """ctc_forward that also keeps every step's alpha row (hfa_ctc_forward_alpha): returns (nll f64 [B], the bits
    ctc_forward gives; alpha [B, Tmax, 2, Lmax + 1] f32, the blank and the label plane, relative to aoff [B, Tmax] f64).
    Rows t >= T[b] and slots past L[b] are left unwritten."""
    B, Tmax, Lmax = _ctc_meta(emis, T, L, targets, "ctc_forward_alpha")
    dev = emis.device
    nll = torch.empty((B,), dtype=torch.float64, device=dev)
    alpha = torch.empty((B, Tmax, 2, Lmax + 1), dtype=torch.float32, device=dev)
    aoff = torch.empty((B, Tmax), dtype=torch.float64, device=dev)
    _lib.call("hfa_ctc_forward_alpha", B, Tmax, Lmax, _ptr(T), _ptr(L), _ptr(emis) if Tmax else None,
              _ptr(targets) if Lmax else None, _ptr(nll), _ptr(alpha) if Tmax else None,
              _ptr(aoff) if Tmax else None, _stream(dev))
    return nll, alpha, aoff


def ctc_backward(emis, T, L, targets, nll, alpha, aoff, out=None):
    """The beta scan and the state posterior (hfa_ctc_backward) from ctc_forward_alpha's results: returns (occ
    [B, Tmax, Lmax + 1] f32: column 0 the blanks' summed posterior, column j label j - 1's; frames, centre, logp
    [B, Lmax] f32: each label's expected frame count, expected position in frames, and posterior-weighted mean
    log-probability).  Zeros past a row's T / L; an infeasible row gives zeros and logp = -inf.  ``out``: the four
    tensors to write into."""
    B, Tmax, Lmax = _ctc_meta(emis, T, L, targets, "ctc_backward")
    dev = emis.device
    _need(nll, torch.float64, "nll")
    _need(alpha, torch.float32, "alpha")
    _need(aoff, torch.float64, "aoff")
    if nll.shape != (B,) or tuple(alpha.shape) != (B, Tmax, 2, Lmax + 1) or tuple(aoff.shape) != (B, Tmax):
        raise ValueError("ctc_backward: nll [B], alpha [B, Tmax, 2, Lmax + 1], aoff [B, Tmax] of ctc_forward_alpha")
    if out is None:
        out = (torch.empty((B, Tmax, Lmax + 1), dtype=torch.float32, device=dev),) + tuple(
            torch.empty((B, Lmax), dtype=torch.float32, device=dev) for _ in range(3))
    occ, frames, centre, logp = out
    _need(occ, torch.float32, "occ")
    if tuple(occ.shape) != (B, Tmax, Lmax + 1):
        raise ValueError("ctc_backward: occ must be [B, Tmax, Lmax + 1]")
    for t, n in ((frames, "frames"), (centre, "centre"), (logp, "logp")):
        _need(t, torch.float32, n)
        if tuple(t.shape) != (B, Lmax):
            raise ValueError(f"ctc_backward: {n} must be [B, Lmax]")
    p = lambda t, on: _ptr(t) if on else None      # noqa: E731
    _lib.call("hfa_ctc_backward", B, Tmax, Lmax, _ptr(T), _ptr(L), p(emis, Tmax), p(targets, Lmax), _ptr(nll),
              p(alpha, Tmax), p(aoff, Tmax), p(occ, Tmax), p(frames, Lmax), p(centre, Lmax), p(logp, Lmax),
              _stream(dev))
    return occ, frames, centre, logp


def ctc_class_index(T, targets, L, V):
    """The target positions of every row grouped by class, for ctc_grad: validates as ctc_check_targets and returns
    int32 numpy arrays (T [B], L [B], targets [B, Lmax], cls_ptr [B, V + 1], cls_idx [B, Lmax]): class c's positions
    in row b are cls_idx[b, cls_ptr[b, c]:cls_ptr[b, c + 1]], ascending (a stable argsort of the row)."""
    import numpy as np
    T_h, L_h, tg_h = ctc_check_targets(T, targets, L, V)
    B, Lmax = tg_h.shape
    cls_ptr = np.zeros((B, int(V) + 1), np.int32)
    cls_idx = np.zeros((B, Lmax), np.int32)
    for b in range(B):
        n = int(L_h[b])
        row = tg_h[b, :n]
        cls_idx[b, :n] = np.argsort(row, kind="stable")
        cls_ptr[b, 1:] = np.cumsum(np.bincount(row, minlength=int(V))[:int(V)])
    return T_h, L_h, tg_h, cls_ptr, cls_idx


def ctc_grad(logits, T, L, occ, nll, cls_ptr, cls_idx, weight=None, V=None, blank_col=CTC_BLANK_COL,
             label_off=CTC_LABEL_OFF, out=None):
    """d (sum_b weight[b] nll[b]) / d logits over the V CTC classes (hfa_ctc_grad): softmax minus the class posterior
    of ctc_backward's occ, times weight[b] (None: 1), written to the classes' columns of ``out`` (default: zeros of
    the logits' shape; its other columns are not touched).  Rows t >= T[b] and infeasible rows (nll = +inf) get
    zeros.  cls_ptr [B, V + 1] / cls_idx [B, Lmax] i32 from ctc_class_index, on the device."""
    B, Tmax, C = logits.shape
    V = C - 2 if V is None else int(V)
    _ctc_logits(logits, V, blank_col, label_off)
    for t, n in ((T, "T"), (L, "L"), (cls_ptr, "cls_ptr"), (cls_idx, "cls_idx")):
        _need(t, torch.int32, n)
    _need(occ, torch.float32, "occ")
    _need(nll, torch.float64, "nll")
    Lmax = occ.shape[2] - 1 if occ.dim() == 3 else -1
    if T.shape != (B,) or L.shape != (B,) or nll.shape != (B,) or tuple(occ.shape) != (B, Tmax, Lmax + 1) or \
            tuple(cls_ptr.shape) != (B, V + 1) or tuple(cls_idx.shape) != (B, Lmax):
        raise ValueError("ctc_grad: T / L / nll [B], occ [B, Tmax, Lmax + 1], cls_ptr [B, V + 1], cls_idx [B, Lmax]")
    if weight is not None:
        _need(weight, torch.float32, "weight")
        if weight.shape != (B,):
            raise ValueError("ctc_grad: weight must be [B]")
    if out is None:
        out = torch.zeros((B, Tmax, C), dtype=torch.float32, device=logits.device)
    _need(out, torch.float32, "grad", contiguous=False)
    if out.shape != logits.shape or out.stride(2) != 1:
        raise ValueError("ctc_grad: out must have the logits' shape and unit stride in the last dim")
    _lib.call("hfa_ctc_grad", B, Tmax, V, Lmax, _ptr(T), _ptr(L), _ptr(logits), logits.stride(1), logits.stride(0),
              blank_col, label_off, _ptr(occ) if Tmax else None, _ptr(nll), _ptr(cls_ptr),
              _ptr(cls_idx) if Lmax else None, None if weight is None else _ptr(weight), _ptr(out), out.stride(1),
              out.stride(0), _stream(logits.device))
    return out


def _ctc_prepare(who, logits, T, targets, L, V, blank_col, label_off):
    """ctc_score's validation plus the class index; one pinned non-blocking copy of all the integers."""
    if not isinstance(logits, torch.Tensor) or logits.dim() != 3:
        raise TypeError(f"{who}: logits must be a [B, T, C] tensor")
    Vn = logits.shape[2] - 2 if V is None else int(V)
    T_h, L_h, tg_h, cp_h, ci_h = ctc_class_index(T, targets, L, Vn)
    B, Tmax = logits.shape[:2]
    if T_h.shape[0] != B:
        raise ValueError(f"{who}: {B} logit rows, {T_h.shape[0]} lengths")
    if B and int(T_h.max()) > Tmax:
        raise ValueError(f"{who}: a row's T = {int(T_h.max())} exceeds the {Tmax} logit frames")
    _ctc_logits(logits, Vn, blank_col, label_off)
    Lmax = tg_h.shape[1]
    if Lmax > int(_lib.lib().hfa_ctc_max_labels()):
        raise _lib.HFAArgumentError(f"{who}: {Lmax} labels exceed the kernel's {_lib.lib().hfa_ctc_max_labels()}",
                                    _lib.HFA_EINVAL)
    import numpy as np
    meta = torch.from_numpy(np.concatenate([T_h, L_h, tg_h.ravel(), ci_h.ravel(), cp_h.ravel()]))
    meta = meta.pin_memory().to(logits.device, non_blocking=True)
    o = 2 * B + 2 * B * Lmax
    return (Vn, meta[:B], meta[B:2 * B], meta[2 * B:2 * B + B * Lmax].view(B, Lmax),
            meta[o:].view(B, Vn + 1), meta[2 * B + B * Lmax:o].view(B, Lmax))


def ctc_posteriors(logits, T, targets, L, V=None, blank_col=CTC_BLANK_COL, label_off=CTC_LABEL_OFF):
    """ctc_score plus the forward-backward report, on one prologue: arguments and validation as ctc_score.  Returns
    (nll f64 [B], occ f32 [B, Tmax, Lmax + 1], frames, centre, logp f32 [B, Lmax], best, ids, n) on the device: see
    ctc_backward for occ and the per-label summaries (exp(logp) is the label's confidence) and ctc_score for the
    rest.  The stored alpha takes B * Tmax * 2 (Lmax + 1) * 4 bytes while this runs."""
    Vn, T_t, L_t, tg_t, _, _ = _ctc_prepare("ctc_posteriors", logits, T, targets, L, V, blank_col, label_off)
    emis, best = ctc_prologue(logits, T_t, L_t, tg_t, Vn, blank_col, label_off)
    nll, alpha, aoff = ctc_forward_alpha(emis, T_t, L_t, tg_t)
    occ, frames, centre, logp = ctc_backward(emis, T_t, L_t, tg_t, nll, alpha, aoff)
    ids, n = ctc_greedy(best, T_t)
    return nll, occ, frames, centre, logp, best, ids, n


class _CTCNLL(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, T, targets, L, V, blank_col, label_off):
        x = logits.detach()
        Vn, T_t, L_t, tg_t, cp_t, ci_t = _ctc_prepare("ctc_nll", x, T, targets, L, V, blank_col, label_off)
        emis, _ = ctc_prologue(x, T_t, L_t, tg_t, Vn, blank_col, label_off)
        nll, alpha, aoff = ctc_forward_alpha(emis, T_t, L_t, tg_t)
        occ = ctc_backward(emis, T_t, L_t, tg_t, nll, alpha, aoff)[0]
        ctx.save_for_backward(x, T_t, L_t, occ, nll, cp_t, ci_t)
        ctx.layout = (Vn, blank_col, label_off)
        return nll.clone()

    @staticmethod
    def backward(ctx, grad_nll):
        x, T_t, L_t, occ, nll, cp_t, ci_t = ctx.saved_tensors
        Vn, blank_col, label_off = ctx.layout
        g = ctc_grad(x, T_t, L_t, occ, nll, cp_t, ci_t, grad_nll.to(torch.float32).contiguous(), Vn, blank_col,
                     label_off)
        return g, None, None, None, None, None, None


def ctc_nll(logits, T, targets, L, V=None, blank_col=CTC_BLANK_COL, label_off=CTC_LABEL_OFF):
    """The CTC loss of forced_alignment.py:256-272 with a gradient: logits [B, Tmax, C] f32 on the GPU in the head's
    layout (arguments and validation as ctc_score) -> nll f64 [B], differentiable with respect to the logits.  The
    backward is one hfa_ctc_grad call with weight = grad_output, into zeros of the logits' shape: the columns that
    are no CTC class get no gradient.  An infeasible row keeps nll = +inf and contributes a zero gradient, which is
    nn.CTCLoss's zero_infinity for the gradient only."""
    return _CTCNLL.apply(logits, T, targets, L, V, blank_col, label_off)


# ------------------------------------------------------------------------------------------------------------
# Full-label alignment losses (loss.hip): the four full-label terms of the reference's _get_loss, their gradient
# with respect to the head logits and the counts behind the GHM tables
# ------------------------------------------------------------------------------------------------------------
_lib.register("hfa_fa_frame_loss", [_I_, _I_, _I_, _I_, ctypes.c_double, _P_, _P_, _P_, _LL_, _LL_, _P_, _P_, _P_, _P_, _P_, _P_,
                                    _P_, _P_, _P_, _LL_, _LL_, _P_])
_lib.register("hfa_fa_emd", [_I_, _I_, _P_, _P_, _P_, _LL_, _LL_, _P_, _P_, _P_, _P_])
_lib.register("hfa_fa_loss_reduce", [_I_, _I_, _I_, _I_, _P_, _P_, _P_, _P_, _P_, _P_, _P_, _P_, _P_, _P_, _P_])

FA_LOSS_NAMES = ("ph_frame_GHM_loss", "ph_edge_GHM_loss", "ph_edge_EMD_loss", "ph_edge_diff_loss")
FA_MAX_BINS = 64                         # loss.hip kMaxBins


def fa_table_slices(V: int, num_bins: int) -> dict:
    """Where the reference's six GHM buffers sit in the packed ``tables`` / ``hist`` array of the loss kernels."""
    V, nb = int(V), int(num_bins)
    o = [0, V, V + nb, V + 2 * nb, V + 2 * nb + 3, V + 3 * nb + 3, V + 3 * nb + 6]
    names = ("ph_frame_GHM_loss_fn.class_ema", "ph_frame_GHM_loss_fn.GD_ema", "ph_edge_GHM_loss_fn.GD_stat_ema",
             "ph_edge_GHM_loss_fn.label_stat_ema_each_class", "ph_edge_diff_GHM_loss_fn.GD_stat_ema",
             "ph_edge_diff_GHM_loss_fn.label_stat_ema_each_class")
    return {n: slice(o[i], o[i + 1]) for i, n in enumerate(names)}


def _fa_i32(x, device, name):
    if not isinstance(x, torch.Tensor):
        import numpy as np
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(x)))
    if x.device.type != "cuda":
        x = x.to(device)
    if x.dtype != torch.int32:
        if x.dtype.is_floating_point:
            raise TypeError(f"{name}: expected an integer (or bool) tensor, got {x.dtype}")
        x = x.to(torch.int32)
    return x.contiguous()


def _fa_check(who, logits, T, label_type, ph_frame=None, ph_edge=None, ph_mask=None):
    if not isinstance(logits, torch.Tensor) or logits.dim() != 3:
        raise TypeError(f"{who}: logits must be a [B, T, V + 2] tensor")
    _need(logits, torch.float32, f"{who}: logits", contiguous=False)
    B, Tmax, C = logits.shape
    V = C - 2
    if logits.stride(2) != 1 and C > 1:
        raise ValueError(f"{who}: logits need unit stride in the last dim")
    if V < 1 or V > CTC_MAX_V:
        raise ValueError(f"{who}: V = {V} frame classes is outside 1..{CTC_MAX_V}")
    for t, n in ((T, "T"), (label_type, "label_type")):
        _need(t, torch.int32, f"{who}: {n}")
        if t.shape != (B,):
            raise ValueError(f"{who}: {n} must be [B]")
    if ph_frame is not None:
        _need(ph_frame, torch.int32, f"{who}: ph_frame")
        if tuple(ph_frame.shape) != (B, Tmax):
            raise ValueError(f"{who}: ph_frame must be [B, Tmax]")
    if ph_edge is not None:
        _need(ph_edge, torch.float32, f"{who}: ph_edge")
        if tuple(ph_edge.shape) != (B, Tmax):
            raise ValueError(f"{who}: ph_edge must be [B, Tmax]")
    if ph_mask is not None:
        _need(ph_mask, torch.int32, f"{who}: ph_mask")
        if tuple(ph_mask.shape) != (B, V):
            raise ValueError(f"{who}: ph_mask must be [B, V]")
    return B, Tmax, V


def fa_frame_loss(logits, T, label_type, ph_frame, ph_edge, ph_mask, tables, num_bins, label_smoothing=0.0,
                  coef=None, emd_fac=None, grad=None, terms=None, bins=None):
    """The frame, edge and edge-difference terms of every frame (hfa_fa_frame_loss): logits [B, Tmax, V + 2] f32 (a
    strided view is fine), T / label_type [B] i32, ph_frame [B, Tmax] i32, ph_edge [B, Tmax] f32, ph_mask [B, V] i32,
    tables f32 [V + 3 num_bins + 6] (fa_table_slices), all on the device.  Returns (terms [B, Tmax, 3] f32, bins
    [B, Tmax, 5] i32); with ``coef`` ([4] f32 on the device: upstream / normaliser per loss, in FA_LOSS_NAMES' order)
    also the gradient, written to column 0 and columns 2.. of ``grad`` (default: zeros of the logits' shape), the EMD's
    share included when ``emd_fac`` (fa_emd) is given."""
    B, Tmax, V = _fa_check("fa_frame_loss", logits, T, label_type, ph_frame, ph_edge, ph_mask)
    nb = int(num_bins)
    _need(tables, torch.float32, "fa_frame_loss: tables")
    if tables.shape != (V + 3 * nb + 6,):
        raise ValueError(f"fa_frame_loss: tables must be [{V + 3 * nb + 6}] for V = {V}, num_bins = {nb}")
    dev = logits.device
    if terms is None:
        terms = torch.empty((B, Tmax, 3), dtype=torch.float32, device=dev)
    if bins is None:
        bins = torch.empty((B, Tmax, 5), dtype=torch.int32, device=dev)
    _need(terms, torch.float32, "fa_frame_loss: terms")
    _need(bins, torch.int32, "fa_frame_loss: bins")
    if tuple(terms.shape) != (B, Tmax, 3) or tuple(bins.shape) != (B, Tmax, 5):
        raise ValueError("fa_frame_loss: terms must be [B, Tmax, 3] and bins [B, Tmax, 5]")
    g_ld = g_bs = 0
    if coef is not None:
        _need(coef, torch.float32, "fa_frame_loss: coef")
        if coef.shape != (4,):
            raise ValueError("fa_frame_loss: coef must be [4]")
        if grad is None:
            grad = torch.zeros(logits.shape, dtype=torch.float32, device=dev)
        _need(grad, torch.float32, "fa_frame_loss: grad", contiguous=False)
        if grad.shape != logits.shape or grad.stride(2) != 1:
            raise ValueError("fa_frame_loss: grad must have the logits' shape and unit stride in the last dim")
        g_ld, g_bs = grad.stride(1), grad.stride(0)
        if emd_fac is not None:
            _need(emd_fac, torch.int32, "fa_frame_loss: emd_fac")
            if tuple(emd_fac.shape) != (B, Tmax):
                raise ValueError("fa_frame_loss: emd_fac must be [B, Tmax]")
    elif grad is not None or emd_fac is not None:
        raise ValueError("fa_frame_loss: grad / emd_fac need coef")
    _lib.call("hfa_fa_frame_loss", B, Tmax, V, nb, float(label_smoothing), _ptr(T), _ptr(label_type), _ptr(logits),
              logits.stride(1), logits.stride(0), _ptr(ph_frame), _ptr(ph_edge), _ptr(ph_mask), _ptr(tables),
              _ptr(terms), _ptr(bins), _ptr(coef), _ptr(emd_fac), _ptr(grad), g_ld, g_bs, _stream(dev))
    return (terms, bins) if coef is None else (terms, bins, grad)


def fa_emd(logits, T, label_type, ph_edge):
    """The EMD term's scans (hfa_fa_emd) over the edge column of logits [B, Tmax, V + 2]: returns (sums [B, 3] f64 =
    sum |forward cumsum| and sum |reverse cumsum| over the row's own frames and |sum d|, what each padding column adds
    to the first; fac [B, Tmax] i32 = the gradient's sign
    counts per frame)."""
    B, Tmax, _ = _fa_check("fa_emd", logits, T, label_type, None, ph_edge)
    sums = torch.empty((B, 3), dtype=torch.float64, device=logits.device)
    fac = torch.empty((B, Tmax), dtype=torch.int32, device=logits.device)
    _lib.call("hfa_fa_emd", B, Tmax, _ptr(T), _ptr(label_type), _ptr(logits), logits.stride(1), logits.stride(0),
              _ptr(ph_edge), _ptr(sums), _ptr(fac) if Tmax else None, _stream(logits.device))
    return sums, fac


def fa_loss_reduce(T, label_type, terms, bins, ph_frame, emd_sums, V, num_bins):
    """Sums, normalisers and counts (hfa_fa_loss_reduce) of fa_frame_loss's and fa_emd's results: returns (row_terms
    [B, 4] f64 unnormalised, losses [4] f64, norm [4] f64, hist i32 [V + 3 num_bins + 6] in tables' layout)."""
    _need(terms, torch.float32, "fa_loss_reduce: terms")
    _need(bins, torch.int32, "fa_loss_reduce: bins")
    _need(ph_frame, torch.int32, "fa_loss_reduce: ph_frame")
    _need(emd_sums, torch.float64, "fa_loss_reduce: emd_sums")
    _need(T, torch.int32, "fa_loss_reduce: T")
    _need(label_type, torch.int32, "fa_loss_reduce: label_type")
    if terms.dim() != 3 or terms.shape[2] != 3:
        raise ValueError("fa_loss_reduce: terms must be [B, Tmax, 3]")
    B, Tmax = terms.shape[:2]
    if tuple(bins.shape) != (B, Tmax, 5) or tuple(ph_frame.shape) != (B, Tmax) or tuple(emd_sums.shape) != (B, 3) or \
            T.shape != (B,) or label_type.shape != (B,):
        raise ValueError("fa_loss_reduce: bins [B, Tmax, 5], ph_frame [B, Tmax], emd_sums [B, 3], T / label_type [B]")
    V, nb = int(V), int(num_bins)
    dev = terms.device
    row_terms = torch.empty((B, 4), dtype=torch.float64, device=dev)
    out = torch.empty(8, dtype=torch.float64, device=dev)
    hist = torch.empty(V + 3 * nb + 6, dtype=torch.int32, device=dev)
    _lib.call("hfa_fa_loss_reduce", B, Tmax, V, nb, _ptr(T), _ptr(label_type), _ptr(terms), _ptr(bins),
              _ptr(ph_frame), _ptr(emd_sums), _ptr(row_terms), _ptr(out), _P(out.data_ptr() + 32), _ptr(hist),
              _stream(dev))
    return row_terms, out[:4], out[4:], hist


_FA_HALF_EMD = (1.0, 1.0, 0.5, 1.0)
_FA_HALF = {}                            # the same on each device, made once


class _FALoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, T, label_type, ph_frame, ph_edge, ph_mask, tables, num_bins, label_smoothing):
        x = logits.detach()
        V = x.shape[2] - 2
        sums, fac = fa_emd(x, T, label_type, ph_edge)
        terms, bins = fa_frame_loss(x, T, label_type, ph_frame, ph_edge, ph_mask, tables, num_bins, label_smoothing)
        row_terms, losses, norm, hist = fa_loss_reduce(T, label_type, terms, bins, ph_frame, sums, V, num_bins)
        # upstream -> coef without a host synchronisation: 1 / normaliser (1/2 of it for the EMD), 0 where none
        half = _FA_HALF.get(x.device)
        if half is None:
            half = _FA_HALF[x.device] = torch.tensor(_FA_HALF_EMD, dtype=torch.float64, device=x.device)
        inv = torch.where(norm > 0, half / norm.clamp_min(1.0), torch.zeros_like(norm))
        ctx.save_for_backward(x, T, label_type, ph_frame, ph_edge, ph_mask, tables, fac, inv, terms, bins)
        ctx.cfg = (int(num_bins), float(label_smoothing))
        ctx.mark_non_differentiable(row_terms, norm, hist, sums)
        return losses.clone(), row_terms, norm, hist, sums

    @staticmethod
    def backward(ctx, g_losses, _g_rows, _g_norm, _g_hist, _g_sums):
        x, T, label_type, ph_frame, ph_edge, ph_mask, tables, fac, inv, terms, bins = ctx.saved_tensors
        nb, ls = ctx.cfg
        coef = (g_losses.to(torch.float64) * inv).to(torch.float32)
        grad = torch.empty(x.shape, dtype=torch.float32, device=x.device)
        grad[:, :, 1] = 0                                    # the kernel writes every other column of every frame
        g = fa_frame_loss(x, T, label_type, ph_frame, ph_edge, ph_mask, tables, nb, ls, coef=coef, emd_fac=fac,
                          grad=grad, terms=terms, bins=bins)[2]
        return g, None, None, None, None, None, None, None, None


def fa_loss(logits, T, label_type, ph_frame, ph_edge, ph_mask, tables, num_bins=10, label_smoothing=0.0,
            stats=False, check=True):
    """The four full-label losses of the reference's _get_loss (forced_alignment.py:188-254) over the rows with
    label_type >= 2, in FA_LOSS_NAMES' order, as an f64 [4] device tensor that is differentiable with respect to the
    logits: logits [B, Tmax, V + 2] f32 on the GPU in the head's layout (a strided view is fine; Tmax is the view's, as
    the reference's EMD mean runs over it), T / label_type [B], ph_frame [B, Tmax] integer, ph_edge [B, Tmax] f32,
    ph_mask [B, V] integer or bool, tables f32 [V + 3 num_bins + 6] (fa_table_slices; constants for the gradient).
    The backward is one hfa_fa_frame_loss launch with device-resident coefficients: a gradient of the logits' shape,
    zeros in column 1 and wherever a row or frame does not take part.  ``stats``: also (row_terms [B, 4] f64
    unnormalised, norm [4] f64, hist i32 in tables' layout, fa_emd's sums [B, 3]).  ``check`` (one host synchronisation): T within the view
    and the taking-part frames' ph_frame within 0..V-1."""
    if not isinstance(logits, torch.Tensor) or logits.device.type != "cuda":
        raise _lib.HFALibraryError("fa_loss: logits must be a GPU tensor (no CPU fallback)")
    dev = logits.device
    T = _fa_i32(T, dev, "T")
    label_type = _fa_i32(label_type, dev, "label_type")
    ph_frame = _fa_i32(ph_frame, dev, "ph_frame")
    ph_mask = _fa_i32(ph_mask, dev, "ph_mask")
    if not isinstance(ph_edge, torch.Tensor):
        import numpy as np
        ph_edge = torch.from_numpy(np.ascontiguousarray(np.asarray(ph_edge, dtype=np.float32)))
    ph_edge = ph_edge.to(dev, torch.float32).contiguous()
    tables = tables.detach().to(dev, torch.float32).contiguous()
    B, Tmax, V = _fa_check("fa_loss", logits, T, label_type, ph_frame, ph_edge, ph_mask)
    if not 0 < int(num_bins) <= FA_MAX_BINS:
        raise ValueError(f"fa_loss: num_bins = {num_bins} is outside 1..{FA_MAX_BINS}")
    if check and B and Tmax:
        part = (torch.arange(Tmax, device=dev)[None, :] < T[:, None]) & (label_type[:, None] >= 2)
        bad = torch.stack([(T > Tmax).any() | (T < 0).any(), (((ph_frame < 0) | (ph_frame >= V)) & part).any()])
        bad = bad.tolist()
        if bad[0]:
            raise ValueError(f"fa_loss: a row's T is outside 0..{Tmax}")
        if bad[1]:
            raise ValueError(f"fa_loss: a ph_frame id is outside 0..{V - 1}")
    out = _FALoss.apply(logits, T, label_type, ph_frame, ph_edge, ph_mask, tables, int(num_bins),
                        float(label_smoothing))
    return out if stats else out[0]


# ------------------------------------------------------------------------------------------------------------
# Head fine-tuning (train.hip): the Linear weight gradient and the clipped AdamW step
# ------------------------------------------------------------------------------------------------------------
_D_ = ctypes.c_double
_lib.register("hfa_wgrad_workspace_bytes", [_I_, _I_, _I_, _I_], ctypes.c_longlong)
_lib.register("hfa_wgrad_chunk_rows", [])
_lib.register("hfa_wgrad_f32", [_I_, _I_, _I_, _I_, _P_, _LL_, _LL_, _P_, _LL_, _LL_, _P_, _P_, _LL_, _P_, _P_, _P_, _P_])
_lib.register("hfa_adamw_f32", [_LL_, _P_, _P_, _P_, _P_, _P_, _D_, _D_, _D_, _D_, _D_, _D_, _D_, _D_, _P_, _P_])


def wgrad_workspace(B, Tmax, N, C, device) -> torch.Tensor:
    """The workspace hfa_wgrad_f32 needs for these sizes (uint8, 8-byte aligned as every torch allocation is)."""
    n = _lib.lib().hfa_wgrad_workspace_bytes(int(B), int(Tmax), int(N), int(C))
    if n < 0:
        _lib.check(int(n), "hfa_wgrad_workspace_bytes")
    return torch.empty(max(int(n), 8), dtype=torch.uint8, device=device)


def wgrad(G, X, lens, dW=None, db=None, sumsq=None, workspace=None):
    """The weight gradient of y = x W^T + b over a variable-length batch (hfa_wgrad_f32): G [B, Tmax, N] f32 = d loss /
    d y and X [B, Tmax, C] f32 (strided views with unit stride in the last dim are fine), lens [B] i32 on the device; rows
    t >= lens[b] never reach a result.  Returns (dW [N, C] f32, db [N] f32, sumsq 0-d f64 = sum dW^2 + sum db^2), written
    into ``dW`` (a row-strided view is fine) / ``db`` / ``sumsq`` where given.  C % 8 == 0.  Deterministic: the same bits
    on every run and under grid_cap."""
    for t, n in ((G, "G"), (X, "X")):
        _need(t, torch.float32, f"wgrad: {n}", contiguous=False)
        if t.dim() != 3 or (t.stride(2) != 1 and t.shape[2] > 1):
            raise ValueError(f"wgrad: {n} must be [B, Tmax, width] with unit stride in the last dim")
    B, Tmax, N = G.shape
    C = X.shape[2]
    if tuple(X.shape[:2]) != (B, Tmax):
        raise ValueError("wgrad: G and X must share [B, Tmax]")
    if N < 1 or C < 8 or C % 8:
        raise ValueError(f"wgrad: N = {N} must be >= 1 and C = {C} a positive multiple of 8")
    _need(lens, torch.int32, "wgrad: lens")
    if lens.shape != (B,):
        raise ValueError("wgrad: lens must be [B]")
    dev = G.device
    if dW is None:
        dW = torch.empty((N, C), dtype=torch.float32, device=dev)
    if db is None:
        db = torch.empty(N, dtype=torch.float32, device=dev)
    if sumsq is None:
        sumsq = torch.empty((), dtype=torch.float64, device=dev)
    _need(dW, torch.float32, "wgrad: dW", contiguous=False)
    _need(db, torch.float32, "wgrad: db")
    _need(sumsq, torch.float64, "wgrad: sumsq")
    if tuple(dW.shape) != (N, C) or dW.stride(1) != 1 or (N > 1 and dW.stride(0) < C) or db.shape != (N,) or \
            sumsq.numel() != 1:
        raise ValueError("wgrad: dW must be [N, C] (rows at least C apart), db [N], sumsq one f64")
    if workspace is None:
        workspace = wgrad_workspace(B, Tmax, N, C, dev)
    _need(workspace, torch.uint8, "wgrad: workspace")
    if workspace.numel() < _lib.lib().hfa_wgrad_workspace_bytes(B, Tmax, N, C):
        raise ValueError("wgrad: workspace too small (wgrad_workspace)")
    # (a size-1 dim's stride is arbitrary in torch: pass the width instead)
    ldg = G.stride(1) if Tmax > 1 else max(N, G.stride(1))
    ldx = X.stride(1) if Tmax > 1 else max(C, X.stride(1))
    _lib.call("hfa_wgrad_f32", B, Tmax, N, C, _ptr(G), ldg, G.stride(0) if B > 1 else 0, _ptr(X), ldx,
              X.stride(0) if B > 1 else 0, _ptr(lens), _ptr(dW), dW.stride(0) if N > 1 else C, _ptr(db), _ptr(sumsq),
              _ptr(workspace), _stream(dev))
    return dW, db, sumsq


def adamw_step(p, m, v, g, sumsq, skipped, *, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-2, step=None,
               bc1=None, bc2=None, max_norm=0.0):
    """clip_grad_norm_(max_norm) + one torch.optim.AdamW step over flat f32 buffers, in place (hfa_adamw_f32): p, m
    (exp_avg), v (exp_avg_sq), g [n]; sumsq the 0-d f64 device scalar wgrad wrote (the gradient's squared norm);
    ``skipped`` i32 [1] on the device, incremented instead of stepping when sumsq is not finite.  ``step`` (1-based)
    gives the bias corrections 1 - beta^step unless ``bc1`` / ``bc2`` are passed; max_norm <= 0: no clipping.  Nothing
    here waits for the device."""
    for t, n in ((p, "p"), (m, "m"), (v, "v"), (g, "g")):
        _need(t, torch.float32, f"adamw_step: {n}")
        if t.dim() != 1 or t.numel() != p.numel():
            raise ValueError(f"adamw_step: {n} must be a flat buffer of p's size")
    _need(sumsq, torch.float64, "adamw_step: sumsq")
    _need(skipped, torch.int32, "adamw_step: skipped")
    if sumsq.numel() != 1 or skipped.numel() != 1:
        raise ValueError("adamw_step: sumsq and skipped hold one element each")
    if bc1 is None or bc2 is None:
        if step is None or int(step) < 1:
            raise ValueError("adamw_step: step (>= 1) or bc1 and bc2")
        bc1 = 1.0 - float(beta1) ** int(step) if bc1 is None else bc1
        bc2 = 1.0 - float(beta2) ** int(step) if bc2 is None else bc2
    _lib.call("hfa_adamw_f32", p.numel(), _ptr(p), _ptr(m), _ptr(v), _ptr(g), _ptr(sumsq), float(max_norm), float(lr),
              float(beta1), float(beta2), float(eps), float(weight_decay), float(bc1), float(bc2), _ptr(skipped),
              _stream(p.device))


class _HeadLinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, ys, W, Ws, b, lens, flag, grad_out):
        if Ws is not None:
            out = linear_split(ys if ys is not None else split(y, flag=flag), Ws, b, flag=flag)
        else:
            out = linear(y, W, b)
        ctx.save_for_backward(y, lens)
        ctx.grad_out = grad_out
        ctx.wshape = tuple(W.shape)
        return out

    @staticmethod
    def backward(ctx, g):
        y, lens = ctx.saved_tensors
        N, C = ctx.wshape
        dW, db, sumsq = ctx.grad_out if ctx.grad_out is not None else (None, None, None)
        if g.stride(-1) != 1:
            g = g.contiguous()
        dW, db, _ = wgrad(g, y, lens, dW, db, sumsq)
        return None, None, dW, None, db, None, None, None


def head_linear(y, ys, Wp, Ws, bp, lens, flag=None, grad_out=None):
    """The head's nn.Linear (forced_alignment.py:53-55) as LatticeHead.logits runs it, differentiable with respect to its
    weight and bias only (the backbone is frozen: no gradient to ``y``): y [B, T, C] f32 and, on the split path, its
    planes ``ys`` (None: split here) with the padded weight's planes ``Ws`` -- linear_split; Ws None: ops.linear on the
    f32 weight.  Wp [n, C], bp [n]; returns logits [B, T, n] (the caller slices the padded columns off).  Backward is one
    ops.wgrad over the rows t < lens[b] (lens [B] i32 on the device); ``grad_out`` = (dW [n, C], db [n], sumsq): write
    the gradient there (the trainer's flat buffer) instead of into new tensors."""
    _need(y, torch.float32, "head_linear: y", contiguous=False)
    _need(Wp, torch.float32, "head_linear: Wp")
    _need(bp, torch.float32, "head_linear: bp")
    _need(lens, torch.int32, "head_linear: lens")
    if y.dim() != 3 or Wp.dim() != 2 or Wp.shape[1] != y.shape[2] or bp.shape != (Wp.shape[0],) or \
            lens.shape != (y.shape[0],):
        raise ValueError("head_linear: y [B, T, C], Wp [n, C], bp [n], lens [B]")
    if Ws is not None and tuple(Ws.shape) != (2, *Wp.shape):
        raise ValueError("head_linear: Ws must be Wp's split planes [2, n, C]")
    return _HeadLinear.apply(y, ys, Wp, Ws, bp, lens, flag, grad_out)
