"""Times of the head fine-tuning step at config-2 geometry: 32 rows x 861 frames x (63 + 2) logits,
hidden 192.  HIP events after warm-up, the median of 50:

  * hfa_wgrad_f32 and hfa_adamw_f32 alone (ops.wgrad, ops.adamw_step);
  * a whole HeadTrainer.step and its parts (gather, head GEMM, FALoss forward and backward, wgrad, AdamW, re-split), as the device
    sees it (events around the step) and as the host sees it (the wall time step() takes to return, nothing awaited):
    where the two agree, the step is bound by the host's launches, not by its kernels;
  * the torch op chain for the same update on the same box: G.flatten(0,1).t() @ X.flatten(0,1) (+ the column sums),
    clip_grad_norm_ and torch.optim.AdamW.

    python scripts/head_train_bench.py [--reps 50] > profiles/train/head_train_bench.txt
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, T, V, C = 32, 861, 63, 192


def timed(fn, reps, warmup=5):
    """Median and least event time of ``fn`` in ms."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        ms.append(s.elapsed_time(e))
    return statistics.median(ms), min(ms)


def rows(seed):
    r = np.random.default_rng(seed)
    out = []
    for b in range(B):
        L = 12
        seq = r.choice(np.arange(1, V), L, replace=False).astype(np.int32)
        mask = np.zeros(V, np.int32)
        mask[seq], mask[0] = 1, 1
        cuts = np.sort(r.choice(np.arange(1, T), L + 1, replace=False))
        frame = np.zeros(T, np.int32)
        for j in range(L):
            frame[cuts[j]:cuts[j + 1]] = seq[j]
        full = b % 4 != 3
        out.append(dict(y=r.standard_normal((T, C)).astype(np.float32), label_type=2 if full else 1, ph_id_seq=seq,
                        ph_frame=frame if full else np.zeros(T, np.int32), ph_mask=mask,
                        ph_edge=r.uniform(0.02, 0.98, T).astype(np.float32) if full else np.zeros(T, np.float32)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    from hubertfa_amd import ops
    from hubertfa_amd.task import ForcedAlignmentTask, synth_checkpoint
    from hubertfa_amd.train import HeadTrainer
    dev = torch.device("cuda")
    N = V + 2
    print(f"head fine-tuning step, {B} x {T} x ({V} + 2), hidden {C}; {torch.cuda.get_device_name(0)}; median (least) of "
          f"{a.reps}, ms")
    g = torch.Generator(device="cpu").manual_seed(0)
    G = (torch.randn(B, T, N, generator=g) * 1e-5).to(dev)
    X = torch.randn(B, T, C, generator=g).to(dev)
    lens = torch.full((B,), T, dtype=torch.int32, device=dev)
    dW, db = torch.empty(N, C, device=dev), torch.empty(N, device=dev)
    ss = torch.zeros((), dtype=torch.float64, device=dev)
    ws = ops.wgrad_workspace(B, T, N, C, dev)
    med, least = timed(lambda: ops.wgrad(G, X, lens, dW, db, ss, ws), a.reps)
    nbytes = 4 * B * T * (N + C)
    print(f"hfa_wgrad_f32            {med:8.4f} ({least:.4f})   {nbytes / 1e6:.1f} MB of input: {nbytes / med / 1e6:.0f} GB/s; "
          f"workspace {ws.numel() / 1e6:.1f} MB")
    med_t, least_t = timed(lambda: (G.flatten(0, 1).t() @ X.flatten(0, 1), G.sum(dim=(0, 1))), a.reps)
    print(f"torch G^T X + column sum {med_t:8.4f} ({least_t:.4f})")
    err = ((G.flatten(0, 1).double().t() @ X.flatten(0, 1).double()) - dW.double()).abs().max().item()
    print(f"  (hfa_wgrad_f32 against the float64 product: max |error| {err:.3g}, max |dW| {dW.abs().max().item():.3g})")

    n = N * C + N
    p, m, v = torch.randn(n, device=dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    gr = torch.cat([dW.flatten(), db])
    skipped = torch.zeros(1, dtype=torch.int32, device=dev)
    med, least = timed(lambda: ops.adamw_step(p, m, v, gr, ss, skipped, lr=1e-3, beta1=0.9, weight_decay=0.1, step=3,
                                              max_norm=0.5), a.reps)
    print(f"hfa_adamw_f32            {med:8.4f} ({least:.4f})   n = {n}")
    lin = torch.nn.Linear(C, N).to(dev)
    opt = torch.optim.AdamW(lin.parameters(), lr=1e-3, weight_decay=0.1)

    def torch_update():
        lin.weight.grad, lin.bias.grad = dW.clone(), db.clone()
        torch.nn.utils.clip_grad_norm_(lin.parameters(), 0.5)
        opt.step()
    med_t, least_t = timed(torch_update, a.reps)
    print(f"torch clip + AdamW       {med_t:8.4f} ({least_t:.4f})")

    with tempfile.TemporaryDirectory() as td:
        ckpt = os.path.join(td, "m.ckpt")
        state_dict = synth_checkpoint(ckpt)["state_dict"]
        task = ForcedAlignmentTask.load_from_checkpoint(ckpt)
    loss_config = {"losses": {"weights": [8.0, 0.1, 0.01, 0.1, 2.0], "enable_RampUpScheduler": [False] * 5},
                   "function": {"num_bins": 10, "alpha": 0.999, "label_smoothing": 0.08}}
    trainer = HeadTrainer(task, {"lr": 1e-3, "weight_decay": 0.1, "total_steps": 100000}, loss_config,
                          gradient_clip_val=0.5, state_dict=state_dict)
    for r in rows(1):
        trainer.add_features(r["y"], r)
    idx = list(range(B))
    host = []

    def step():
        t0 = time.perf_counter()
        trainer.step(idx)
        host.append((time.perf_counter() - t0) * 1e3)
    med, least = timed(step, a.reps)
    h = statistics.median(host[-a.reps:])
    print(f"HeadTrainer.step         {med:8.4f} ({least:.4f})   host time to enqueue it {h:.4f}: "
          f"{'host-bound' if h > 0.8 * med else 'device-bound'}; skipped {int(trainer.skipped)}")

    batch = trainer._batch(idx)
    med_b, _ = timed(lambda: trainer._batch(idx), a.reps)
    med_f, _ = timed(lambda: trainer.logits(batch), a.reps)
    print(f"  gather of the batch    {med_b:8.4f}")
    print(f"  head GEMM (+ split)    {med_f:8.4f}")

    def forward_backward():
        with torch.enable_grad():
            trainer.Wp.grad = trainer.bp.grad = None
            _, total = trainer._losses(batch, valid=False, grad=True)
            total.backward()
    med_l, _ = timed(forward_backward, a.reps)
    print(f"  head GEMM, FALoss (five terms, table update), backward, wgrad: {med_l:8.4f}")


if __name__ == "__main__":
    main()
