"""Drop-in ``AlignmentDecoder`` (reference: tools/alignment_decoder.py) running its hot path on the GPU.

Same constructor, same ``decode``/``_decode``/``forward_pass`` signatures and return values, same attributes
(``ph_seq_id``, ``ph_idx_seq``, ``ph_frame_pred``, ``ph_time_int_pred``, ``edge_prob``, ``ph_pred_seq``,
``ph_intervals_pred``, ``frame_confidence``, ``ctc_logits``).  The per-frame work (mask, log_softmax, edge
sigmoid, lattice gather), the monotonic DP and the backtrack are HIP kernels (csrc/viterbi.hip); the host keeps
only the O(#phones) interval/word assembly, in numpy, with the reference's dtypes.

``decode_batch`` is the batched entry used by the pipeline: B utterances, one kernel launch per stage.
"""
from __future__ import annotations

import functools
import time

import numpy as np
import torch

from . import _lib, ops
from .intervals import assemble_intervals, batch_results, total_confidence, utterance_result  # noqa: F401 (public names)


def _device(t: torch.Tensor) -> torch.device:
    if t.device.type == "cuda":
        return t.device
    return torch.device("cuda", torch.cuda.current_device())


class AlignmentDecoder:
    """GPU alignment decoder with the reference's API (tools/alignment_decoder.py:8-24)."""

    def __init__(self, vocab, melspec_config):
        self.vocab = vocab
        self.melspec_config = melspec_config
        self.frame_length = self.melspec_config["hop_length"] / (self.melspec_config["sample_rate"])
        self.ctc_logits = None
        self.ph_seq_id = None
        self.ph_idx_seq = None
        self.ph_frame_pred = None
        self.ph_time_int_pred = None
        self.ph_intervals_pred = None
        self.edge_prob = None
        self.ph_pred_seq = None
        self.frame_confidence = None

    # -- frame trimming (alignment_decoder.py:45-50) ------------------------------------------------------
    def num_frames(self, wav_length: float | None, n_logit_frames: int) -> int:
        if wav_length is None:
            return n_logit_frames
        n = int((wav_length * self.melspec_config["sample_rate"] + 0.5) / self.melspec_config["hop_length"])
        return min(n, n_logit_frames)

    def ph_ids(self, ph_seq) -> np.ndarray:
        return np.array([self.vocab["vocab"][ph] for ph in ph_seq])  # KeyError on OOV, as (:35)

    # -- single utterance, reference signature (alignment_decoder.py:26-143) ------------------------------
    def decode(self, ph_frame_logits, ph_edge_logits, ctc_logits, wav_length: float | None, ph_seq: list[str],
               word_seq: list[str] = None, ph_idx_to_word_idx: list[int] = None):
        ph_seq_id = self.ph_ids(ph_seq)
        self.ph_seq_id = ph_seq_id
        if word_seq is None:
            word_seq = ph_seq
            ph_idx_to_word_idx = np.arange(len(ph_seq))
        res = self.decode_batch(ph_frame_logits, ph_edge_logits, [wav_length], [ph_seq], [word_seq],
                                [ph_idx_to_word_idx], keep_frame_probs=True)[0]
        T = res["T"]
        self.ctc_logits = ctc_logits[:, :T, :].float().squeeze(0).cpu().numpy().astype("float32")
        self.ph_frame_pred = res["ph_frame_pred"]
        self.edge_prob = res["edge_prob"]
        self.ph_idx_seq = res["ph_idx_seq"]
        self.ph_time_int_pred = res["ph_time_int"]
        self.frame_confidence = res["frame_confidence"]
        self.ph_pred_seq = res["ph_seq"]
        self.ph_intervals_pred = res["ph_intervals"]
        return res["ph_seq"], res["ph_intervals"], res["word_seq"], res["word_intervals"], res["confidence"]

    # -- batched path ---------------------------------------------------------------------------------------
    def decode_batch(self, frame_logits, edge_logits, wav_lengths, ph_seqs, word_seqs=None, p2ws=None,
                     keep_frame_probs: bool = False, host: bool = True, dp_ranges=None):
        """Decode B utterances: frame_logits [B,Tl,V], edge_logits [B,Tl] (GPU tensors, strided views OK).

        Returns one dict per utterance with the reference decode() outputs (+ raw path arrays).  With
        ``host=False`` the device outputs instead; ``dp_ranges`` (callable (Tmax, Smax) -> n, host=False only):
        when it returns n > 1 the forward DP is not enqueued here but left as n step-range closures plus the
        backtrack under ``dev_out["deferred"]``, to be called in order on one stream (task.submit runs them beside
        the next batch's attention kernels); the outputs are complete when the last one has run.
        """
        dev = _device(frame_logits)
        frame_logits = frame_logits.to(dev).float()
        edge_logits = edge_logits.to(dev).float()
        if frame_logits.stride(2) != 1:
            frame_logits = frame_logits.contiguous()
        B, Tl, V = frame_logits.shape
        Ts = [self.num_frames(w, Tl) for w in wav_lengths]
        ids = [self.ph_ids(p) for p in ph_seqs]
        # state pitch padded to a multiple of 8 so the DP kernel moves each lane's states as vectors
        Smax = -(-max(len(i) for i in ids) // 8) * 8
        ids_pad = np.zeros((B, Smax), np.int32)
        for b, i in enumerate(ids):
            ids_pad[b, :len(i)] = i
        # one pinned staging buffer -> one async H2D copy (keeps the stream free-running); T, S and the ids are
        # contiguous slices of it (no copy kernels)
        meta = np.concatenate([np.asarray(Ts, np.int32), np.array([len(i) for i in ids], np.int32), ids_pad.ravel()])
        meta_t = torch.from_numpy(meta).pin_memory().to(dev, non_blocking=True)
        T_t, S_t, ids_t = meta_t[:B], meta_t[B:2 * B], meta_t[2 * B:].view(B, Smax)
        # the lattice prologue also writes _decode's dp / curr initialisation (one launch, no ATen glue)
        lat = ops.lattice_prologue(frame_logits, edge_logits, ids_t, T_t, S_t, want_frame_probs=keep_frame_probs,
                                   init_dp=True)
        dp, bt, curr = lat.pop("dp"), lat.pop("bt"), lat.pop("curr")
        dev_out = dict(edge_diff=lat["edge_diff"], T=Ts, lattice=lat)
        Tmax = dp.shape[1]

        def forward(t0=None, t1=None):
            ops.viterbi_forward(lat["prob_log"], lat["not_edge_log"], lat["edge_log"], curr, dp, bt, ids_t, T_t, S_t,
                                steps=None if t0 is None else (t0, t1))

        def backtrack():
            idx, tint, n, fc = ops.viterbi_backtrack(dp, bt, ids_t, T_t, S_t)
            dev_out.update(ph_idx_seq=idx, ph_time_int=tint, n=n, frame_confidence=fc)
        # past the library's range limit (the segmented-state form) the DP runs whole lattices only
        n_rng = 1 if host or dp_ranges is None or Smax > _lib.lib().hfa_viterbi_range_max_states() \
            else max(1, int(dp_ranges(Tmax, Smax)))
        if n_rng > 1:
            cuts = np.linspace(1, Tmax, n_rng + 1).round().astype(int)
            dev_out["deferred"] = [functools.partial(forward, int(a), int(c)) for a, c in zip(cuts[:-1], cuts[1:])]
            dev_out["deferred"].append(backtrack)
            return dev_out
        forward()
        backtrack()
        if not host:
            return dev_out
        return self.assemble(dev_out, ph_seqs, word_seqs, p2ws, keep_frame_probs)

    _FETCH_KEYS = ("ph_idx_seq", "ph_time_int", "n", "frame_confidence", "edge_diff")

    def fetch(self, dev_out, keep_frame_probs: bool = False):
        """Enqueue the D2H copies of a batch's boundary arrays into pinned memory; returns a handle that
        ``assemble`` completes.  Lets the host assemble batch i while the GPU runs batch i+1."""
        keys = list(self._FETCH_KEYS)
        src = {k: dev_out[k] for k in keys}
        if keep_frame_probs:
            src["edge_prob"] = dev_out["lattice"]["edge_prob"]
            src["ph_frame_pred"] = dev_out["lattice"]["ph_frame_pred"]
        for k in ("split_oflow", "split_oflow_head"):      # the split-precision range guard (task._guard)
            if k in dev_out:
                src[k] = dev_out[k]
        host = {}
        for k, t in src.items():
            h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
            h.copy_(t, non_blocking=True)
            host[k] = h
        ev = torch.cuda.Event()
        ev.record()
        out = {"T": dev_out["T"], "host": host, "event": ev}
        if "redo" in dev_out:
            out["redo"] = dev_out["redo"]
        return out

    def assemble(self, dev_out, ph_seqs, word_seqs=None, p2ws=None, keep_frame_probs: bool = False,
                 intervals: bool = True):
        """Host half of decode for a batch (from ``decode_batch(host=False)`` or ``fetch``): per-utterance
        interval/word assembly.  ``intervals=False`` returns the raw boundary records only (T, ph_idx_seq,
        ph_time_int, frame_confidence, edge_diff), for callers that assemble them elsewhere (``utterance_result``:
        the CLI's export workers, rank 0 after the multi-GPU gather)."""
        resolve = dev_out.get("resolve")
        if resolve is not None:              # a pipelined handle whose DP steps are still held (task.submit)
            resolve()                        # (raises a held step's error, again on every retry: ADVICE r05)
            dev_out.pop("resolve", None)
        if "host" not in dev_out:
            dev_out = self.fetch(dev_out, keep_frame_probs)
        ev = dev_out["event"]
        while not ev.query():          # poll and sleep: a HIP event wait spins a core (~12 ms of CPU per 15.6 ms
            time.sleep(2e-4)           # step); the batch lands while the GPU runs the next one, so 0.2 ms is slack
        hd = {k: v.numpy() for k, v in dev_out["host"].items()}
        if "redo" in dev_out and any(int(hd[k][0]) for k in ("split_oflow", "split_oflow_head") if k in hd):
            # a split-f16 operand left f16 range: this batch is recomputed with f32 GEMMs
            return dev_out["redo"]()
        Ts = dev_out["T"]
        idx_h, tint_h, n_h, fc_h, ed_h = (hd[k] for k in self._FETCH_KEYS)
        ep_h = hd.get("edge_prob") if keep_frame_probs else None
        fp_h = hd.get("ph_frame_pred") if keep_frame_probs else None
        if intervals:        # the batch's fractional boundaries in one set of array operations (intervals.py)
            out = batch_results(Ts, idx_h, tint_h, n_h, fc_h, ed_h, ph_seqs, word_seqs, p2ws, self.frame_length,
                                tables=dev_out.get("tables"))
        else:
            out = []
            for b in range(len(ph_seqs)):
                T, k = Ts[b], int(n_h[b])
                out.append(dict(T=T, ph_idx_seq=idx_h[b, :k].astype(np.int64),
                                ph_time_int=tint_h[b, :k].astype(np.int64), frame_confidence=fc_h[b, :T].copy(),
                                edge_diff=ed_h[b, :T].copy()))
        if keep_frame_probs:
            for b, r in enumerate(out):
                r["edge_prob"] = ep_h[b, :Ts[b]].copy()
                r["ph_frame_pred"] = fp_h[b, :Ts[b]].copy()
        return out

    # -- reference static/numpy API on the GPU --------------------------------------------------------------
    @staticmethod
    def forward_pass(T, S, prob_log, not_edge_prob_log, edge_prob_log, curr_ph_max_prob_log, dp, backtrack_s,
                     ph_seq_id, prob3_pad_len):
        """numpy in/out with the reference's in-place semantics (alignment_decoder.py:170-230)."""
        dev = torch.device("cuda", torch.cuda.current_device())
        Smax = prob_log.shape[1]
        pl = torch.from_numpy(np.ascontiguousarray(prob_log, np.float32))[None].to(dev)
        nE = torch.from_numpy(np.ascontiguousarray(not_edge_prob_log, np.float32))[None].to(dev)
        E = torch.from_numpy(np.ascontiguousarray(edge_prob_log, np.float32))[None].to(dev)
        cu = torch.from_numpy(np.ascontiguousarray(curr_ph_max_prob_log, np.float64))[None].to(dev)
        d = torch.from_numpy(np.ascontiguousarray(dp, np.float32))[None].to(dev)
        bt = torch.from_numpy(np.ascontiguousarray(backtrack_s).astype(np.int8))[None].to(dev)
        ids = torch.from_numpy(np.ascontiguousarray(ph_seq_id).astype(np.int32))[None].to(dev)
        T_t = torch.tensor([T], dtype=torch.int32, device=dev)
        S_t = torch.tensor([S], dtype=torch.int32, device=dev)
        pad = torch.tensor([prob3_pad_len], dtype=torch.int32, device=dev)
        assert Smax == S
        ops.viterbi_forward(pl, nE, E, cu, d, bt, ids, T_t, S_t, pad)
        dp[...] = d[0].cpu().numpy()
        bt_h = bt[0].cpu().numpy().astype(np.int32)
        bt_h[0] = backtrack_s[0]
        backtrack_s[...] = bt_h
        curr_ph_max_prob_log[...] = cu[0].cpu().numpy()
        return dp, backtrack_s, curr_ph_max_prob_log

    def _decode(self, ph_seq_id, ph_prob_log, edge_prob):
        """(ph_idx_seq, ph_time_int, frame_confidence) from a host lattice (alignment_decoder.py:232-294)."""
        dev = torch.device("cuda", torch.cuda.current_device())
        ph_seq_id = np.asarray(ph_seq_id)
        T = ph_prob_log.shape[0]
        S = len(ph_seq_id)
        prob_log = np.ascontiguousarray(ph_prob_log[:, ph_seq_id], np.float32)
        E = np.log(edge_prob + 1e-6).astype("float32")  # numpy dtype rules of (:241-242)
        nE = np.log(1 - edge_prob + 1e-6).astype("float32")
        pl = torch.from_numpy(prob_log)[None].to(dev)
        ids = torch.from_numpy(ph_seq_id.astype(np.int32))[None].to(dev)
        T_t = torch.tensor([T], dtype=torch.int32, device=dev)
        S_t = torch.tensor([S], dtype=torch.int32, device=dev)
        dp, bt, curr = ops.viterbi_init(pl, ids, T_t, S_t)
        ops.viterbi_forward(pl, torch.from_numpy(nE)[None].to(dev), torch.from_numpy(E)[None].to(dev), curr, dp,
                            bt, ids, T_t, S_t)
        idx, tint, n, fc = ops.viterbi_backtrack(dp, bt, ids, T_t, S_t)
        k = int(n[0])
        return (idx[0, :k].cpu().numpy().astype(np.int64), tint[0, :k].cpu().numpy().astype(np.int64),
                fc[0].cpu().numpy())

    def plot(self, melspec):
        """Validation figure of the last decode() (alignment_decoder.py:152-168; hubertfa_amd/plot.py): ``melspec``
        [1, n_mels, T] (a torch tensor, as MelSpecExtractor returns it); returns the matplotlib figure."""
        from .plot import phone_index_per_frame, plot_for_valid
        ph_intervals_int = (self.ph_intervals_pred / self.frame_length).round().astype("int32")
        ph_idx_frame = phone_index_per_frame(self.ph_idx_seq, self.ph_time_int_pred, self.ph_frame_pred.shape[0])
        mel = melspec.cpu().numpy() if isinstance(melspec, torch.Tensor) else np.asarray(melspec)
        return plot_for_valid(mel, self.ph_pred_seq, ph_intervals_int, self.frame_confidence,
                              self.ph_frame_pred[:, self.ph_seq_id], ph_idx_frame, self.edge_prob)

    def ctc(self):
        """Greedy CTC collapse (alignment_decoder.py:145-150); validation-only helper, host numpy."""
        ctc = np.argmax(self.ctc_logits, axis=-1)
        ctc_index = np.concatenate([[0], ctc])
        ctc_index = (ctc_index[1:] != ctc_index[:-1]) * ctc != 0
        ctc = ctc[ctc_index]
        return np.array([ph_id for ph_id in ctc if ph_id != 0])

    # -- batched CTC scoring on the GPU (csrc/ctc.hip) ------------------------------------------------------
    def ctc_targets(self, ph_seq) -> np.ndarray:
        """The CTC target of a transcript: its phoneme ids with id 0 (SP and the ignored phonemes) dropped
        (binarize.py:197-198).  KeyError on a phoneme outside the vocabulary."""
        ids = self.ph_ids(ph_seq).astype(np.int64).reshape(-1)
        return ids[ids != 0]

    def id_to_phone(self) -> dict:
        """id -> phoneme name (the first name the vocabulary gives an id; id 0 is "SP")."""
        inv = {}
        for ph, i in self.vocab["vocab"].items():
            inv.setdefault(int(i), ph)
        inv[0] = "SP"
        return inv

    def ctc_batch(self, logits, n_frames, ph_seqs, host: bool = True, posteriors: bool = False):
        """Score B transcripts against the head's CTC columns and greedy-decode them, on the GPU.

        logits [B, Tl, V + 2]: the head's logits (column 0 the edge, 1 the CTC blank, 3.. the CTC labels); n_frames:
        the frame count ``decode`` keeps (:45-50: ``num_frames`` of the row's wav length), an int or one per row,
        clipped to Tl.  Returns one
        dict per utterance: ``ctc_nll`` = -log P(transcript | audio) (forced_alignment.py:256-272; inf when the
        transcript does not fit the frames), ``ctc_confidence`` = clip(exp(-nll / T), 1e-6, 1 - 1e-6) (GHMLoss.py:35-37),
        ``ctc_phones`` the greedy decode (:145-150) as phoneme names and ``ctc_phone_ids`` as ids.  ``host=False``:
        the device tensors instead (dict with nll, best, ids, n, T), stream-ordered; ``ctc_results`` completes them.

        ``posteriors``: the CTC forward-backward as well (ops.ctc_posteriors).  Every result also
        carries, aligned with ``ctc_targets(ph_seq)`` (the transcript's non-SP phones), ``ctc_phone_confidence`` =
        exp of the posterior-weighted mean log-probability of the phone where the model places it (f64 array; 0 for
        an infeasible transcript), ``ctc_phone_centre_s`` its expected position in seconds and ``ctc_phone_frames``
        its expected frame count; ``host=False`` adds occ, frames, centre, logp and L to the device dict."""
        tgs = [self.ctc_targets(p) for p in ph_seqs]          # (first: an unknown phoneme raises before any GPU work)
        dev = _device(logits)
        logits = logits.to(dev).float()
        if logits.stride(2) != 1:
            logits = logits.contiguous()
        B, Tl = logits.shape[:2]
        if isinstance(n_frames, (list, tuple, np.ndarray)):
            Ts = [min(int(t), Tl) for t in n_frames]
        else:
            Ts = [min(int(n_frames), Tl)] * B
        if len(Ts) != B or len(ph_seqs) != B:
            raise ValueError(f"ctc_batch: {B} logit rows, {len(Ts)} frame counts, {len(ph_seqs)} transcripts")
        Ls = [len(t) for t in tgs]
        if posteriors:
            nll, occ, frames, centre, logp, best, ids, n = ops.ctc_posteriors(logits, Ts, tgs, Ls)
            dev_out = dict(nll=nll, best=best, ids=ids, n=n, T=Ts, occ=occ, frames=frames, centre=centre, logp=logp,
                           L=Ls)
        else:
            nll, best, ids, n = ops.ctc_score(logits, Ts, tgs, Ls)
            dev_out = dict(nll=nll, best=best, ids=ids, n=n, T=Ts)
        return self.ctc_results(dev_out) if host else dev_out

    def ctc_results(self, dev_out) -> list:
        """Host half of ctc_batch: the device tensors of ``ctc_batch(host=False)`` -> one dict per utterance."""
        nll = dev_out["nll"].cpu().numpy()
        ids, n = dev_out["ids"].cpu().numpy(), dev_out["n"].cpu().numpy()
        inv = self.id_to_phone()
        out = []
        for b, T in enumerate(dev_out["T"]):
            v = float(nll[b])
            with np.errstate(over="ignore"):
                conf = float(np.exp(-v / T)) if T > 0 else (1.0 if v == 0.0 else 0.0)
            k = ids[b, :int(n[b])].astype(np.int64)
            out.append(dict(ctc_nll=v, ctc_confidence=float(np.clip(conf, 1e-6, 1 - 1e-6)),
                            ctc_phones=[inv.get(int(i), str(int(i))) for i in k], ctc_phone_ids=k))
        if "logp" in dev_out:
            frames, centre, logp = (dev_out[k].cpu().numpy().astype(np.float64) for k in ("frames", "centre", "logp"))
            for b, (r, L) in enumerate(zip(out, dev_out["L"])):
                r["ctc_phone_confidence"] = np.exp(logp[b, :L])
                r["ctc_phone_centre_s"] = centre[b, :L] * self.frame_length
                r["ctc_phone_frames"] = frames[b, :L]
        return out


def ctc_ghm_loss(nll, T, ema):
    """The reference's ``CTCGHMLoss.forward(valid=True)`` weighting (networks/loss/GHMLoss.py:21-52) of per-utterance
    CTC losses: each ``nll[b]`` (ops.ctc_score / ``ctc_batch(host=False)["nll"]``, or any tensor-like) is divided by
    the EMA bin count of its per-frame confidence clip(exp(-nll / T), 1e-6, 1 - 1e-6), and the batch is averaged.
    ``ema``: the checkpoint's ``CTC_GHM_loss_fn.ema`` buffer (num_bins values); it is not updated (valid=True).
    Returns a 0-d tensor of nll's dtype on nll's device (0 for an empty batch, as the reference)."""
    nll = torch.as_tensor(nll)
    if nll.numel() == 0:
        return torch.tensor(0.0, device=nll.device)
    T = torch.as_tensor(T, device=nll.device)
    ema = torch.as_tensor(ema, device=nll.device).to(nll.dtype)
    bins = ema.numel()
    conf = (-nll / T).exp().clamp(1e-6, 1 - 1e-6)
    idx = torch.floor(conf * bins).long().clamp(0, bins - 1)
    return (nll / (ema[idx] + 1e-10)).mean()
