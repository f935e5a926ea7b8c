"""Time the fused log-mel kernel (csrc/melspec.hip) and make_input_feature on the MI355X.

    python scripts/melspec_bench.py [--rows 32] [--samples 441000] [--iters 50] [--out FILE] [--accuracy]

HIP-event time per batch of ``rows`` x ``samples`` (config 2: 32 x 441 000, 27 592 frames) after warm-up, on seeded
Gaussian waves (not zeros: data changes the clock), median and minimum over ``--iters`` launches timed one by one plus
one window of all of them, and the implied share of the three-product f16 roofline (838.9 TF/s of useful MACs, as
profiles/shape_roofline.csv): useful work = 2 F (2 bins win_length + bins n_mels) FLOP over the needed bins.  Then the
cost of ``make_input_feature`` over ``encode_batch`` alone on the synthetic Hubert-base task.  ``--accuracy`` prints
e_hip / e_torch_f32 of the test cases (tests/melspec_ref.py's metric).  Needs a GPU: there is no CPU path.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

ROOFLINE_TFS = 838.9


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=32)
    ap.add_argument("--samples", type=int, default=441000)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--accuracy", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("melspec_bench: no GPU (timings come from the MI355X only)")
    import melspec_ref as ref
    from hubertfa_amd.melspec import MelSpecExtractor, mel_filterbank, needed_bins
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    cfg = ref.DEFAULT
    ex = MelSpecExtractor(**cfg, device="cuda")
    g = torch.Generator().manual_seed(3)
    x = (0.1 * torch.randn(args.rows, args.samples, generator=g)).cuda()
    out = ex.batch(x)
    frames = out.shape[0] * out.shape[2]
    lo, hi = needed_bins(mel_filterbank(cfg))
    flop = 2.0 * frames * (2 * (hi - lo) * cfg["win_length"] + (hi - lo) * cfg["n_mels"])
    med, best, window = event_times(lambda: ex.batch(x), args.iters)
    say(f"logmel {args.rows} x {args.samples} ({frames} frames, bins {lo}..{hi - 1}): median {med * 1e3:.0f} us, "
        f"min {best * 1e3:.0f} us, back-to-back {window * 1e3:.0f} us per batch over {args.iters} launches")
    say(f"  useful work {flop / 1e12:.3f} TFLOP -> {flop / (med * 1e-3) / 1e12:.1f} TF/s at the median = "
        f"{100 * flop / (med * 1e-3) / 1e12 / ROOFLINE_TFS:.1f} % of the three-product f16 roofline "
        f"({ROOFLINE_TFS} TF/s; compute-bound: {args.rows * args.samples * 4 / 1e6:.0f} MB in, "
        f"{frames * cfg['n_mels'] * 4 / 1e6:.0f} MB out)")
    assert not ex.overflowed()

    if args.accuracy:
        import math
        cases = [("gauss", n) for n in (1, 511, 512, 513, 1023, 1536, 4097, 32768)] + \
                [("zeros", 4096), ("sign", 8192), ("sine", 44100)]
        for kind, n in cases:
            gg = torch.Generator().manual_seed(1000 + n)
            w = {"gauss": lambda: 0.1 * torch.randn(n, generator=gg), "zeros": lambda: torch.zeros(n),
                 "sign": lambda: torch.randint(0, 2, (n,), generator=gg).float() * 2.0 - 1.0,
                 "sine": lambda: 0.5 * torch.sin(2.0 * math.pi * 440.0 * torch.arange(n, dtype=torch.float64)
                                                 / 44100.0).float()}[kind]()
            mel64, e32, bound = ref.bar(w, cfg)
            e = ref.error(torch.exp(ex(w.cuda())[0].double().cpu()), mel64, cfg)
            say(f"accuracy default {kind:5s} N={n:6d}: e_hip {e:.2e}  e_torch_f32 {e32:.2e}  bound {bound:.2e}")
        ex2 = MelSpecExtractor(**ref.SECOND, device="cuda")
        w = 0.1 * torch.randn(3000, generator=torch.Generator().manual_seed(4000))
        mel64, e32, bound = ref.bar(w, ref.SECOND)
        e = ref.error(torch.exp(ex2(w.cuda())[0].double().cpu()), mel64, ref.SECOND)
        say(f"accuracy second  gauss N=  3000: e_hip {e:.2e}  e_torch_f32 {e32:.2e}  bound {bound:.2e}")

    # make_input_feature over encode_batch alone (synthetic Hubert-base, the same batch at the melspec rate)
    from hubertfa_amd.task import ForcedAlignmentTask, synth_checkpoint
    ck = synth_checkpoint()
    hp = ck["hyper_parameters"]
    task = ForcedAlignmentTask(hp["vocab_text"], hp["vowel_text"], hp["model_config"], hp["hubert_config"],
                               hp["melspec_config"], state_dict=ck["state_dict"], device="cuda")
    task.on_predict_start()
    it = max(3, args.iters // 5)
    enc = event_times(lambda: task.encode_batch(x), it, warmup=2)
    mif = event_times(lambda: task.make_input_feature(x), it, warmup=2)
    say(f"encode_batch alone: median {enc[0]:.2f} ms;  make_input_feature (units + mel + flag reads + per-row views): "
        f"median {mif[0]:.2f} ms  (+{mif[0] - enc[0]:.2f} ms, {100 * (mif[0] / enc[0] - 1):.1f} %)")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w", encoding="utf-8") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
