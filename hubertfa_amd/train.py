"""Head fine-tuning on the GPU: the reference's training step (networks/task/forced_alignment.py:296-334) for the one
case where only the head's nn.Linear trains -- a checkpoint's backbone kept frozen (optimizer_config.freeze,
forced_alignment.py:499-501) under a new head for another phoneme set, or the old head continued on new labels
(load_pretrained, forced_alignment.py:118-125).

With the encoder and the UNet frozen, a file's backbone output y [T, hidden] never changes: ``HeadTrainer.cache`` computes
it once on the inference path and keeps it, with the file's targets, on the device.  A step is then the head GEMM
(ops.head_linear), losses.FALoss, the weight gradient (ops.wgrad, csrc/train.hip) and the clipped AdamW update
(ops.adamw_step) under OneCycleLR's learning rate and beta1 (schedulers.one_cycle); nothing in it waits for the device.
Out of scope: the UNet's and the encoder's backward, validation metrics, multi-GPU training, HDF5 datasets.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import yaml

from . import ops
from .alignment_decoder import AlignmentDecoder
from .hubert import dev_lengths
from .labels import make_ph_data
from .losses import LOSS_NAMES, FALoss
from .schedulers import GaussianRampUp, NoneScheduler, one_cycle

BETA2, EPS = 0.999, 1e-8                     # torch.optim.AdamW's defaults, which forced_alignment.py:473-486 leaves


def init_head(N, C, seed):
    """A new head's (weight [N, C], bias [N]) on the host: U(-1/sqrt(C), 1/sqrt(C)) for both, nn.Linear's range, drawn from
    ``seed`` alone (weight first), so a run can be repeated anywhere."""
    gen = torch.Generator().manual_seed(int(seed))
    k = 1.0 / math.sqrt(C)
    return (torch.empty(N, C).uniform_(-k, k, generator=gen), torch.empty(N).uniform_(-k, k, generator=gen))


class HeadTrainer:
    """``task``: a ForcedAlignmentTask (its head, vocabulary and decoder are replaced in place, so the task aligns with the
    head being trained).  ``optimizer_config``: lr (a float, or the reference's {"backbone", "head"} of which "head" is
    used), weight_decay, total_steps.  ``loss_config``: losses.weights [5], losses.enable_RampUpScheduler [5] (absent:
    none), function.{num_bins, alpha, label_smoothing}.  ``gradient_clip_val``: the norm clip (<= 0 or None: none).
    ``vocab``: a new vocabulary (the dict of vocab.yaml, or its text); a vocab_size other than the checkpoint's gives a
    new head, U(-1/sqrt(C), 1/sqrt(C)) for weight and bias (nn.Linear's range) from ``seed``, and fresh GHM tables;
    otherwise the checkpoint's head and tables continue.  ``state_dict``: the checkpoint's (its loss buffers for a
    continued head, its backbone.* for ``save``); default: re-read from the file the task was loaded from, so a task that
    never trains holds no host copy of its checkpoint."""

    def __init__(self, task, optimizer_config, loss_config, gradient_clip_val=None, vocab=None, seed=0, state_dict=None):
        self.task = task
        self._state_dict = state_dict
        self.device = dev = task.device
        self.optimizer_config, self.loss_config = optimizer_config, loss_config
        lr = optimizer_config["lr"]
        self.max_lr = float(lr["head"] if isinstance(lr, dict) else lr)
        self.weight_decay = float(optimizer_config.get("weight_decay", 1e-2))
        self.total_steps = int(optimizer_config["total_steps"])
        self.max_norm = float(gradient_clip_val or 0.0)
        self.seed = int(seed)
        if isinstance(vocab, str):
            vocab = yaml.safe_load(vocab)
        head = task.head
        old_V = head.vocab_size
        C = head.head_w.shape[1]
        new_head = vocab is not None and int(vocab["vocab_size"]) != old_V
        if vocab is not None:
            task.vocab = vocab
            task.ignored_phones = vocab.get("ignored_phonemes", [])
            task.hparams["vocab_text"] = yaml.safe_dump(vocab)
            task.decoder = AlignmentDecoder(vocab, task.melspec_config)
        self.V = V = int(task.vocab["vocab_size"])
        self.N, self.C = V + 2, C
        self.n4 = n4 = -(-self.N // 4) * 4
        # the flat buffers: the padded weight [n4, C], then the padded bias [n4]; the padding rows stay zero in all four
        n = n4 * C + n4
        self.p = torch.zeros(n, dtype=torch.float32, device=dev)
        self.m, self.v, self.g = (torch.zeros_like(self.p) for _ in range(3))
        Wp, bp = self._planes_of(self.p)
        if new_head:
            W0, b0 = init_head(self.N, C, self.seed)
            Wp[:self.N], bp[:self.N] = W0.to(dev), b0.to(dev)
        else:
            Wp[:self.N] = head.head_w
            bp[:self.N] = head.head_b
        self.Wp, self.bp = Wp.requires_grad_(), bp.requires_grad_()
        self.gW, self.gb = self._planes_of(self.g)
        self.sumsq = torch.zeros((), dtype=torch.float64, device=dev)
        self.skipped = torch.zeros(1, dtype=torch.int32, device=dev)
        # the task's head becomes views of the flat buffer (and the planes re-split from it after every step)
        head.head_wp, head.head_bp = Wp.detach(), bp.detach()
        head.head_w, head.head_b = head.head_wp[:self.N], head.head_bp[:self.N]
        head.vocab_size = V
        head.arch.vocab_size = V
        # (LatticeHead's one-time |w| < 16 test of the planes would wait for the device every step: a weight that
        # outgrows the split GEMM's range raises the head's flag instead, which check_range reads)
        self.split = head.ctx.precision == "split" and C % 32 == 0
        head.head_ws = torch.empty((2, n4, C), dtype=torch.float16, device=dev) if self.split else None
        self._resplit()
        # losses, tables and schedules
        state = self._checkpoint_state() if not new_head else {}
        self.loss = FALoss.from_checkpoint(state, loss_config, vocab_size=V, device=dev)
        task._fa_loss = self.loss
        task.hparams["loss_config"], task.hparams["optimizer_config"] = loss_config, optimizer_config
        self.weights = [float(w) for w in self.loss.weights.tolist()]
        ramp = loss_config.get("losses", {}).get("enable_RampUpScheduler") or [False] * 5
        self.schedulers = [GaussianRampUp(self.total_steps) if on else NoneScheduler() for on in ramp]
        if len(self.schedulers) != 5:
            raise ValueError("HeadTrainer: losses.enable_RampUpScheduler holds five flags")
        self.step_count = 0
        self.rows = []
        self.frame_length = task.melspec_config["hop_length"] / task.melspec_config["sample_rate"]

    def _checkpoint_state(self):
        """The source checkpoint's state_dict on the host: the one passed in, else the task's file, read when asked."""
        if self._state_dict is not None:
            return self._state_dict
        path = getattr(self.task, "checkpoint_path", None)
        if path is None:
            return {}
        return torch.load(path, map_location="cpu", weights_only=True)["state_dict"]

    def _planes_of(self, flat):
        n4, C = self.n4, self.C
        return flat[:n4 * C].view(n4, C), flat[n4 * C:]

    def _resplit(self):
        if self.split:
            ops.split(self.task.head.head_wp, out=self.task.head.head_ws, flag=self.task.head.flag)

    # -- the feature cache --------------------------------------------------------------------------------------
    def add_features(self, y, item):
        """One precomputed row: y [T, C] (the backbone's output over the row's own frames) and its labels -- ``item`` as
        labels.read_transcriptions gives them (ph_seq names, ph_dur seconds or empty: a weak label), or the targets
        themselves (label_type, ph_id_seq, ph_edge [T], ph_frame [T], ph_mask [V]).  Returns the row's index."""
        dev = self.device
        y = torch.as_tensor(y, dtype=torch.float32).to(dev).contiguous()
        if y.dim() != 2 or y.shape[1] != self.C:
            raise ValueError(f"add_features: y must be [T, {self.C}]")
        T = y.shape[0]
        if "ph_mask" in item:
            lt = int(item["label_type"])
            seq, edge, frame, mask = item["ph_id_seq"], item["ph_edge"], item["ph_frame"], item["ph_mask"]
        else:
            durs = list(item.get("ph_dur") or [])
            lt = 2 if durs else 1
            ids = [self.task.vocab["vocab"][p] for p in item["ph_seq"]]
            seq, edge, frame, mask, _ = make_ph_data(self.task.vocab, T, lt, ids, durs, self.frame_length)
            if seq is None:
                raise ValueError(f"add_features: item {item.get('name', len(self.rows))} has no phone but SP")
        seq = np.asarray(seq, np.int64).reshape(-1)
        frame = np.asarray(frame, np.int32).reshape(-1)
        edge = np.asarray(edge, np.float32).reshape(-1)
        mask = np.asarray(mask, np.int32).reshape(-1)
        # validated here, once, on the host: the step passes check=False and never waits for the device
        if frame.shape != (T,) or edge.shape != (T,) or mask.shape != (self.V,):
            raise ValueError("add_features: ph_frame / ph_edge must be [T] and ph_mask [V]")
        if T and (frame.min() < 0 or frame.max() >= self.V):
            raise ValueError(f"add_features: a ph_frame id is outside 0..{self.V - 1}")
        if len(seq) and (seq.min() < 1 or seq.max() >= self.V):
            raise ValueError(f"add_features: a ph_id_seq id is outside 1..{self.V - 1}")
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        self.rows.append(dict(y=y, T=T, label_type=lt, seq=seq, ph_frame=up(frame), ph_edge=up(edge),
                              ph_mask=up(mask), name=item.get("name")))
        return len(self.rows) - 1

    @torch.no_grad()
    def cache(self, waves, items, wav_sr=None, lengths=None):
        """Encode B labelled waves once (waves / ``wav_sr`` / ``lengths`` as ForcedAlignmentTask.loss_batch) and keep each
        row's backbone output over its own frames with its targets.  Range guard as loss_batch: a split-f16 operand out
        of range re-runs the batch on the f32 GEMMs.  Returns the rows' indices."""
        task, head = self.task, self.task.head

        def run():
            feats, n_frames, wl = task.encode_batch(waves, wav_sr, lengths)
            if isinstance(n_frames, (list, tuple)):
                y = head.backbone(feats, [head.padded_len(int(t)) for t in n_frames], want_split=True)
            else:
                y = head.backbone(feats, want_split=True)
            flag = ops.flag_take(head.flag) if head.precision == "split" else None
            return y[0], [task.decoder.num_frames(w, y[0].shape[1]) for w in wl], flag
        y, Ts, flag = run()
        enc = getattr(task.unitsEncoder, "model", None)
        bad = flag is not None and int(flag.item())
        if getattr(enc, "precision", "f32") == "split":
            bad = int(ops.flag_take(ops.split_flag(self.device)).item()) or bad
        if bad:
            y, Ts, _ = task._f32(run)
            self._use_f32_head()              # features beyond f16 range: the head trains on the f32 GEMM
        if len(items) != len(Ts):
            raise ValueError(f"cache: {len(Ts)} waves, {len(items)} items")
        return [self.add_features(y[b, :Ts[b]].clone(), it) for b, it in enumerate(items)]

    def _use_f32_head(self):
        self.split = False
        self.task.head.head_ws = None          # LatticeHead.logits then takes ops.linear

    def check_range(self):
        """Read (and clear) the head's split-f16 range flag; one wait for the device.  The trainer skips LatticeHead's
        one-time |w| < 16 test of the weight planes, so a feature row or a weight that left the split GEMM's range since
        the last call shows here: the steps since then trained on wrong logits, and this raises instead of letting them
        be saved.  Called by ``save`` and by finetune_head.py wherever it reads the losses back."""
        if self.split and int(ops.flag_take(self.task.head.flag)):
            self._use_f32_head()
            raise RuntimeError("HeadTrainer: a feature or a head weight left the split-f16 GEMM's range (|x| < 65504, "
                               "|w| < 32) since the last check; the steps since then are not valid.  This trainer now "
                               "runs the head on the f32 GEMM: load_state() the last good state and go on, or start "
                               "over with task.head.precision = 'f32'")

    # -- a step -------------------------------------------------------------------------------------------------
    def _batch(self, indices):
        rows = [self.rows[int(i)] for i in indices]
        if not rows:
            raise ValueError("HeadTrainer: an empty batch")
        dev = self.device
        Ts = [r["T"] for r in rows]
        pad = torch.nn.utils.rnn.pad_sequence                 # zero rows past each row's T
        y = pad([r["y"] for r in rows], batch_first=True)
        ph_frame = pad([r["ph_frame"] for r in rows], batch_first=True)
        ph_edge = pad([r["ph_edge"] for r in rows], batch_first=True)
        ph_mask = torch.stack([r["ph_mask"] for r in rows])
        return dict(y=y, lens=dev_lengths(Ts, dev), T=np.asarray(Ts, np.int32), ph_frame=ph_frame, ph_edge=ph_edge,
                    ph_mask=ph_mask, seqs=[r["seq"] for r in rows], L=[len(r["seq"]) for r in rows],
                    label_type=[r["label_type"] for r in rows])

    def logits(self, batch, grad=False):
        """The head's logits [B, Tmax, V + 2] of a gathered batch, as LatticeHead.logits forms them."""
        head = self.task.head
        out = ops.head_linear(batch["y"], None, self.Wp if grad else head.head_wp, head.head_ws if self.split else None,
                              self.bp if grad else head.head_bp, batch["lens"], flag=head.flag,
                              grad_out=(self.gW, self.gb, self.sumsq) if grad else None)
        return out[:, :, :self.N]

    def _losses(self, batch, valid, grad):
        losses = self.loss(self.logits(batch, grad), batch["T"], batch["ph_frame"], batch["ph_edge"], batch["seqs"],
                           batch["L"], batch["ph_mask"], batch["label_type"], valid=valid, check=False)
        coef = [w * float(s()) for w, s in zip(self.weights, self.schedulers)]
        total = sum(l * c for l, c in zip(losses, coef))      # forced_alignment.py:330-334
        return losses, total

    def schedule(self):
        """(lr, beta1) of the step about to run."""
        return one_cycle(self.step_count, self.total_steps, self.max_lr)

    def step(self, indices):
        """One training step over the cached rows ``indices``.  Returns the five losses of LOSS_NAMES and the total as
        0-d f64 device tensors (detached); nothing is read back."""
        if self.step_count >= self.total_steps:
            raise ValueError(f"HeadTrainer: total_steps = {self.total_steps} steps have run")
        batch = self._batch(indices)
        lr, beta1 = self.schedule()
        with torch.enable_grad():
            self.Wp.grad = self.bp.grad = None
            losses, total = self._losses(batch, valid=False, grad=True)
            total.backward()                               # ... -> ops.wgrad into the flat gradient buffer
        k = self.step_count + 1
        ops.adamw_step(self.p, self.m, self.v, self.g, self.sumsq, self.skipped, lr=lr, beta1=beta1, beta2=BETA2,
                       eps=EPS, weight_decay=self.weight_decay, bc1=1.0 - beta1 ** k, bc2=1.0 - BETA2 ** k,
                       max_norm=self.max_norm)
        self._resplit()
        for s in self.schedulers:
            s.step()
        self.step_count = k
        return [l.detach() for l in losses] + [total.detach()]

    @torch.no_grad()
    def evaluate(self, indices):
        """The same five losses and total with valid=True: no gradient, no table update, no step."""
        losses, total = self._losses(self._batch(indices), valid=True, grad=False)
        return [l.detach() for l in losses] + [total.detach()]

    # -- state --------------------------------------------------------------------------------------------------
    def state(self):
        """Host copies: step, the unpadded head weight / bias, the padded m / v / last gradient planes, the GHM tables,
        the skipped-step count."""
        W, b = self._planes_of(self.p)
        mW, mb = self._planes_of(self.m)
        vW, vb = self._planes_of(self.v)
        c = lambda t: t.detach().cpu().clone()  # noqa: E731
        return dict(step=self.step_count, weight=c(W[:self.N]), bias=c(b[:self.N]), padded_weight=c(W), padded_bias=c(b),
                    exp_avg=(c(mW), c(mb)), exp_avg_sq=(c(vW), c(vb)), grad=(c(self.gW), c(self.gb)),
                    sumsq=float(self.sumsq), tables=self.loss.state_dict(), skipped=int(self.skipped))

    def load_state(self, state):
        """Continue from ``state()``'s dict (or one shaped like it: step, weight [N, C], bias [N], exp_avg and
        exp_avg_sq as (weight-shaped, bias-shaped) pairs, padded or not, tables under the reference's names): the head,
        AdamW's moments, the GHM tables, the step count and the schedules."""
        dev, N = self.device, self.N
        up = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32).to(dev)  # noqa: E731
        with torch.no_grad():
            for flat, (w, b) in ((self.p, (state["weight"], state["bias"])), (self.m, state["exp_avg"]),
                                 (self.v, state["exp_avg_sq"])):
                W, B = self._planes_of(flat)
                w, b = up(w), up(b)
                if w.shape[0] < N or w.shape[1] != self.C or b.shape[0] < N:
                    raise ValueError(f"load_state: expected [{N}, {self.C}] and [{N}] arrays")
                flat.zero_()
                W[:N], B[:N] = w[:N], b[:N]
        for n, t in state.get("tables", {}).items():
            if n in self.loss.tables:
                t = up(t)
                if t.shape != self.loss.tables[n].shape:
                    raise ValueError(f"load_state: table {n} has shape {tuple(t.shape)}")
                self.loss.tables[n] = t.clone()
        self.step_count = int(state["step"])
        for s in self.schedulers:
            s.resume(self.step_count)
        self._resplit()

    def save(self, path=None):
        """A Lightning-layout checkpoint that ForcedAlignmentTask.load_from_checkpoint and FALoss.from_checkpoint load
        unchanged: the input's backbone.*, the new head.weight / head.bias (unpadded), FALoss's tables under the
        reference's buffer names; hyper_parameters with the new vocab_text and both configs.  Raises (check_range) if the
        head left the split GEMM's range."""
        self.check_range()
        st = self.state()
        sd = {k: torch.as_tensor(v).detach().cpu() for k, v in self._checkpoint_state().items()
              if k.startswith("backbone.")}
        if not sd:
            raise ValueError("HeadTrainer.save: no backbone.* to carry over (pass state_dict, or load the task with "
                             "load_from_checkpoint)")
        sd["head.weight"], sd["head.bias"] = st["weight"], st["bias"]
        sd.update(st["tables"])
        ckpt = {"state_dict": sd, "hyper_parameters": dict(self.task.hparams), "global_step": self.step_count}
        if path is not None:
            torch.save(ckpt, path)
        return ckpt


__all__ = ["HeadTrainer", "LOSS_NAMES"]
