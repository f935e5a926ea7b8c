"""FALoss: the reference's _get_loss (networks/task/forced_alignment.py:188-282) on the device kernels.

The four full-label terms run as ops.fa_loss (csrc/loss.hip), the weak-label term as ops.ctc_nll (csrc/ctc.hip) weighted
as CTCGHMLoss.forward (networks/loss/GHMLoss.py:21-56); all five are differentiable with respect to the head logits.  The
seven EMA tables live on the device under the reference's buffer names and are updated, when ``valid`` is False, by
update_ema (GHMLoss.py:5-9) from the kernels' integer counts; the loss always uses the tables as they were before.
``total`` applies the plain weights; the ramp-up schedulers (forced_alignment.py:70-79) are hubertfa_amd/schedulers.py's,
applied by train.HeadTrainer.
"""
from __future__ import annotations

import torch

from . import ops

LOSS_NAMES = ops.FA_LOSS_NAMES + ("ctc_GHM_loss",)
CTC_TABLE = "CTC_GHM_loss_fn.ema"
CTC_BINS, CTC_ALPHA = 10, 1 - 1e-3           # CTCGHMLoss(alpha=1 - 1e-3), forced_alignment.py:108


def update_ema(ema, alpha, num_bins, hist):
    """GHMLoss.py:5-9, line for line."""
    hist = hist / (torch.sum(hist) + 1e-10) * num_bins
    ema = ema * alpha + (1 - alpha) * hist
    ema = ema / (torch.sum(ema) + 1e-10) * num_bins
    return ema


class FALoss:
    def __init__(self, vocab_size, num_bins=10, alpha=1 - 1e-6, label_smoothing=0.0, weights=None, device="cuda"):
        self.vocab_size, self.num_bins = int(vocab_size), int(num_bins)
        self.alpha, self.label_smoothing = float(alpha), float(label_smoothing)
        self.device = torch.device(device)
        self.weights = torch.tensor([1.0] * 5 if weights is None else [float(w) for w in weights],
                                    dtype=torch.float64, device=self.device)
        if self.weights.shape != (5,):
            raise ValueError("FALoss: five loss weights, in LOSS_NAMES' order")
        self._slices = ops.fa_table_slices(self.vocab_size, self.num_bins)
        self.tables = {n: torch.ones(s.stop - s.start, dtype=torch.float32, device=self.device)
                       for n, s in self._slices.items()}
        self.tables[CTC_TABLE] = torch.ones(CTC_BINS, dtype=torch.float32, device=self.device)

    # -- checkpoint ---------------------------------------------------------------------------------------------
    @classmethod
    def from_checkpoint(cls, state_dict, loss_config, vocab_size=None, device="cuda"):
        """``state_dict``: a Lightning checkpoint's (the loss modules' buffers under their attribute names);
        ``loss_config``: its hyper_parameters["loss_config"] (function.num_bins / alpha / label_smoothing,
        losses.weights).  Buffers the checkpoint lacks stay at ones, as the reference initialises them."""
        fn = loss_config["function"]
        if vocab_size is None:
            vocab_size = state_dict["ph_frame_GHM_loss_fn.class_ema"].numel()
        self = cls(vocab_size, fn["num_bins"], fn["alpha"], fn["label_smoothing"],
                   loss_config.get("losses", {}).get("weights"), device)
        for n, t in self.tables.items():
            if n in state_dict:
                v = torch.as_tensor(state_dict[n]).to(self.device, torch.float32)
                if v.shape != t.shape:
                    raise ValueError(f"FALoss: checkpoint buffer {n} has shape {tuple(v.shape)}, expected "
                                     f"{tuple(t.shape)}")
                self.tables[n] = v.clone()
        return self

    def state_dict(self):
        return {n: t.detach().cpu().clone() for n, t in self.tables.items()}

    def packed_tables(self):
        return torch.cat([self.tables[n] for n in self._slices])

    # -- the losses ---------------------------------------------------------------------------------------------
    def __call__(self, logits, T, ph_frame, ph_edge, ph_id_seq, L, ph_mask, label_type, valid=False, stats=False, check=True):
        """The five losses in _get_loss's order (a list of 0-d f64 device tensors): logits [B, Tmax, V + 2] on the GPU;
        T, L, label_type [B] host integers (lists, numpy or CPU tensors); ph_frame / ph_edge [B, Tmax], ph_mask [B, V];
        ph_id_seq: the rows' target id lists (or a padded [B, Lmax] array with L).  ``valid`` False: the tables are
        updated after the losses are formed.  ``stats``: also a dict with row_terms [B, 4] (unnormalised), norm [4],
        ctc_nll [B] (NaN where the row has no weak label), hist, emd_sums [B, 3] (ops.fa_emd).  ``check`` False: skip
        ops.fa_loss's validation of T and ph_frame, which waits for the device (a caller that validated its targets once,
        as train.HeadTrainer does when it caches them)."""
        import numpy as np
        dev = logits.device
        T_h = np.asarray(torch.as_tensor(T).cpu() if isinstance(T, torch.Tensor) else T, dtype=np.int64).reshape(-1)
        lt_h = np.asarray(torch.as_tensor(label_type).cpu() if isinstance(label_type, torch.Tensor) else label_type,
                          dtype=np.int64).reshape(-1)
        L_h = np.asarray(torch.as_tensor(L).cpu() if isinstance(L, torch.Tensor) else L, dtype=np.int64).reshape(-1)
        B = logits.shape[0]
        losses4, row_terms, norm, hist, emd_sums = ops.fa_loss(
            logits, T_h.astype(np.int32), lt_h.astype(np.int32), ph_frame, ph_edge, ph_mask, self.packed_tables(),
            self.num_bins, self.label_smoothing, stats=True, check=check)
        # the weak-label term: CTCGHMLoss.forward (GHMLoss.py:21-56) over the rows with label_type >= 1
        weak = np.nonzero(lt_h >= 1)[0]
        ctc = torch.zeros((), dtype=torch.float64, device=dev)
        nll_all = torch.full((B,), float("nan"), dtype=torch.float64, device=dev)
        conf = None
        if len(weak):
            seqs = [np.asarray(ph_id_seq[b], dtype=np.int64).reshape(-1)[:int(L_h[b])] for b in weak]
            widx = torch.as_tensor(weak, device=dev)
            wl = logits if len(weak) == B else logits[widx]
            nll = ops.ctc_nll(wl, T_h[weak].astype(np.int32), seqs, L_h[weak].astype(np.int32))
            Tw = torch.as_tensor(T_h[weak], device=dev).to(torch.float64)
            ema = self.tables[CTC_TABLE].to(torch.float64)
            conf = (-nll.detach() / Tw).exp().clamp(1e-6, 1 - 1e-6)
            idx = torch.floor(conf * CTC_BINS).long().clamp(0, CTC_BINS - 1)
            ctc = (nll / (ema[idx] + 1e-10)).mean()
            nll_all[widx] = nll.detach()
        if not valid:
            self._update(hist, conf)
        out = [losses4[0], losses4[1], losses4[2], losses4[3], ctc]
        if stats:
            return out, dict(row_terms=row_terms, norm=norm, ctc_nll=nll_all, hist=hist, emd_sums=emd_sums)
        return out

    @torch.no_grad()
    def _update(self, hist, conf):
        """The EMA updates of GHMLoss.py:181-209 and :278-300 (alpha from loss_config) and :52-54 (alpha 1 - 1e-3): a
        table whose loss did not run this step (no full-label row, no difference pair, no weak row) stays as it is."""
        h = hist.to(torch.float32)
        for n, s in self._slices.items():
            hs = h[s]
            new = update_ema(self.tables[n], self.alpha, hs.numel(), hs)
            self.tables[n] = torch.where(hs.sum() > 0, new, self.tables[n])
        if conf is not None:
            ch = torch.histc(conf.to(torch.float32), bins=CTC_BINS, min=0, max=1)
            self.tables[CTC_TABLE] = update_ema(self.tables[CTC_TABLE], CTC_ALPHA, CTC_BINS, ch)

    def total(self, losses):
        """sum_k weights[k] losses[k] (forced_alignment.py:68's weights; no ramp-up schedule)."""
        return sum(w * l for w, l in zip(self.weights, losses))
