"""Time the CTC kernels (csrc/ctc.hip) and align_batch(ctc=True) on the MI355X.

    python scripts/ctc_bench.py [--rows 32] [--frames 861] [--phones 45] [--iters 50] [--out FILE] [--no-task]
                                [--backward]

At config-2 geometry (32 rows x 861 frames, V = 63, about 45 non-SP phones per row) on seeded Gaussian logits in the
head's layout: HIP-event time of hfa_ctc_prologue, hfa_ctc_forward and hfa_ctc_greedy after warm-up (median and
minimum over ``--iters`` launches timed one by one, plus one back-to-back window), the Viterbi forward DP on a lattice
of the same (rows, frames, 2 phones + 1 states) for comparison, and wider transcripts (one row each) through the
multi-wave forms.  Then, on the synthetic Hubert-base task, the wall difference align_batch(ctc=True) - align_batch()
for 32 x 10 s waves.  ``--backward`` adds the forward-backward kernels at the same shapes: hfa_ctc_forward_alpha (beside
the plain forward it must not slow down), hfa_ctc_backward and hfa_ctc_grad.  Needs a GPU: there is no CPU path.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def event_times(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    each = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        each.append(a.elapsed_time(b))
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return statistics.median(each), min(each), a.elapsed_time(b) / iters


def wall_times(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=32)
    ap.add_argument("--frames", type=int, default=861)
    ap.add_argument("--phones", type=int, default=45)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-task", action="store_true")
    ap.add_argument("--backward", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ctc_bench: no GPU (timings come from the MI355X only)")
    from hubertfa_amd import ops
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    B, T, V, L = args.rows, args.frames, 63, args.phones
    rng = np.random.default_rng(11)
    i32 = lambda a: torch.as_tensor(np.asarray(a, np.int32)).cuda()      # noqa: E731

    def kernels(B, T, L, iters):
        logits = (torch.randn(B, T, V + 2, generator=torch.Generator().manual_seed(3)) * 3).cuda()
        T_t, L_t = i32([T] * B), i32([L] * B)
        tg = i32(rng.integers(1, V, (B, L)))
        emis, best = ops.ctc_prologue(logits, T_t, L_t, tg)
        pro = event_times(lambda: ops.ctc_prologue(logits, T_t, L_t, tg), iters)
        fwd = event_times(lambda: ops.ctc_forward(emis, T_t, L_t, tg), iters)
        gre = event_times(lambda: ops.ctc_greedy(best, T_t), iters)
        return pro, fwd, gre

    def fb_kernels(B, T, L, iters):
        logits = (torch.randn(B, T, V + 2, generator=torch.Generator().manual_seed(3)) * 3).cuda()
        tg_h = np.random.default_rng(12).integers(1, V, (B, L))
        _, _, _, cp, ci = ops.ctc_class_index([T] * B, tg_h, [L] * B, V)
        T_t, L_t, tg, cp, ci = i32([T] * B), i32([L] * B), i32(tg_h), i32(cp), i32(ci)
        emis, _ = ops.ctc_prologue(logits, T_t, L_t, tg)
        nll, alpha, aoff = ops.ctc_forward_alpha(emis, T_t, L_t, tg)
        out = ops.ctc_backward(emis, T_t, L_t, tg, nll, alpha, aoff)
        grad = torch.zeros_like(logits)
        fwd = event_times(lambda: ops.ctc_forward(emis, T_t, L_t, tg), iters)
        fwa = event_times(lambda: ops.ctc_forward_alpha(emis, T_t, L_t, tg), iters)
        bwd = event_times(lambda: ops.ctc_backward(emis, T_t, L_t, tg, nll, alpha, aoff, out=out), iters)
        grd = event_times(lambda: ops.ctc_grad(logits, T_t, L_t, out[0], nll, cp, ci, out=grad), iters)
        return fwd, fwa, bwd, grd

    pro, fwd, gre = kernels(B, T, L, args.iters)
    say(f"ctc {B} x {T} frames, V = {V}, {L} labels ({2 * L + 1} states), one wave per utterance:")
    for name, t in (("prologue", pro), ("forward ", fwd), ("greedy  ", gre)):
        say(f"  {name}: median {t[0] * 1e3:.0f} us, min {t[1] * 1e3:.0f} us, back-to-back {t[2] * 1e3:.0f} us"
            + (f"  ({t[0] * 1e3 / T:.3f} us per step)" if name.startswith("forward") else ""))

    # the Viterbi forward DP on the same (rows, frames, states): SP-framed transcripts, 2 L + 1 states
    S = 2 * L + 1
    Smax = -(-S // 8) * 8
    ids = np.zeros((B, Smax), np.int32)
    ids[:, 1:S:2] = rng.integers(1, V, (B, L))
    g = torch.Generator().manual_seed(4)
    frame = (torch.randn(B, T, V, generator=g) * 3).cuda()
    edge = torch.randn(B, T, generator=g).cuda()
    T_t, S_t, ids_t = i32([T] * B), i32([S] * B), i32(ids)
    lat = ops.lattice_prologue(frame, edge, ids_t, T_t, S_t, init_dp=True)
    vit = event_times(lambda: ops.viterbi_forward(lat["prob_log"], lat["not_edge_log"], lat["edge_log"], lat["curr"],
                                                  lat["dp"], lat["bt"], ids_t, T_t, S_t), args.iters)
    say(f"  viterbi forward, {S} states: median {vit[0] * 1e3:.0f} us, min {vit[1] * 1e3:.0f} us "
        f"({vit[0] * 1e3 / T:.3f} us per step) -> the CTC forward takes {fwd[0] / vit[0]:.2f} x")

    for Lw, Tw in ((300, 3000), (1000, 3000), (4000, 9000), (8191, 9000)):
        _, f, _ = kernels(1, Tw, Lw, max(5, args.iters // 5))
        say(f"ctc forward 1 x {Tw} frames, {Lw} labels: median {f[0] * 1e3:.0f} us ({f[0] * 1e3 / Tw:.3f} us per step)")

    if args.backward:
        shapes = [(B, T, L, args.iters)] + [(1, Tw, Lw, max(5, args.iters // 5))
                                            for Lw, Tw in ((300, 3000), (1000, 3000), (4000, 9000), (8191, 9000))]
        for Bb, Tb, Lb, it in shapes:
            fwd, fwa, bwd, grd = fb_kernels(Bb, Tb, Lb, it)
            say(f"ctc forward-backward {Bb} x {Tb} frames, {Lb} labels (median us, us per step): "
                f"forward {fwd[0] * 1e3:.0f} ({fwd[0] * 1e3 / Tb:.3f}), "
                f"forward_alpha {fwa[0] * 1e3:.0f} ({fwa[0] * 1e3 / Tb:.3f}, {fwa[0] / fwd[0]:.2f} x), "
                f"backward {bwd[0] * 1e3:.0f} ({bwd[0] * 1e3 / Tb:.3f}, {bwd[0] / fwd[0]:.2f} x), "
                f"grad {grd[0] * 1e3:.0f}")

    if not args.no_task:
        from hubertfa_amd import synth
        from hubertfa_amd.task import ForcedAlignmentTask, synth_checkpoint
        ck = synth_checkpoint()
        hp = ck["hyper_parameters"]
        task = ForcedAlignmentTask(hp["vocab_text"], hp["vowel_text"], hp["model_config"], hp["hubert_config"],
                                   hp["melspec_config"], state_dict=ck["state_dict"], device="cuda")
        task.on_predict_start()
        n = (T - 1) * 512 + 200                                   # 861 frames at hop 512
        waves = torch.from_numpy(np.stack([synth.synth_audio(n, 44100, seed=20 + b) for b in range(B)])).cuda()
        names = [p for p, i in task.vocab["vocab"].items() if i != 0]
        seqs = [["SP"] + [names[int(i)] for i in rng.integers(0, len(names), L)] + ["SP"] for _ in range(B)]
        it = max(5, args.iters // 5)
        plain = wall_times(lambda: task.align_batch(waves, seqs), it)
        both = wall_times(lambda: task.align_batch(waves, seqs, ctc=True), it)
        only = wall_times(lambda: task.ctc_score_batch(waves, seqs), it)
        say(f"align_batch {B} x {n} samples ({T} frames), wall: median {plain[0]:.2f} ms;  align_batch(ctc=True): "
            f"median {both[0]:.2f} ms  (+{both[0] - plain[0]:.2f} ms, {100 * (both[0] / plain[0] - 1):.1f} %; min "
            f"{plain[1]:.2f} -> {both[1]:.2f} ms);  ctc_score_batch alone: median {only[0]:.2f} ms")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w", encoding="utf-8") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
