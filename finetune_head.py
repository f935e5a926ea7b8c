"""Fine-tune the head of a checkpoint on a labelled folder, the backbone frozen (reference: the training step of
networks/task/forced_alignment.py:296-334 with optimizer_config.freeze on the backbone, :499-501, and load_pretrained's
new head for another vocabulary, :118-125), one GPU.

    python finetune_head.py -c model.ckpt -f folder [--vocab vocab.yaml] [--steps 200] [--batch_seconds 60] [--lr 1e-3]
        [--weight_decay 0.1] [--clip 0.5] [--seed 0] [--hubert_path synth:0] -o out.ckpt [--log run.jsonl]

``folder`` is score_labels.py's: ``transcriptions.csv`` (``name``, ``ph_seq``, ``ph_dur``; a blank ``ph_dur`` is a weak
label) and the ``<name>.wav`` files, beside it or under ``wavs/``.  Every file runs through the encoder and the UNet once
(hubertfa_amd.train.HeadTrainer.cache, batched per sample rate as score_labels.py batches them); then ``--steps`` seeded
random batches of at most ``--batch_seconds`` of audio train the head under OneCycleLR, AdamW and the norm clip.  The
log gets one JSON line per step (the five losses, the total, lr, beta1), read back from the device every ``--log_every``
steps, so the loop itself never waits for the GPU.  ``--vocab`` with another vocab_size starts a new head; otherwise the
checkpoint's head and GHM tables continue.  The loss weights and functions are the checkpoint's loss_config (absent: the
reference's train_config defaults).  Writes a checkpoint infer.py and score_labels.py load.
"""
from __future__ import annotations

import json
import pathlib

import click

DEFAULT_LOSS_CONFIG = {"losses": {"weights": [8.0, 0.1, 0.01, 0.1, 2.0], "enable_RampUpScheduler": [False, False, False, True, True]},
                       "function": {"num_bins": 10, "alpha": 0.999, "label_smoothing": 0.08}}


def batch_plan(durations, steps, batch_seconds, seed):
    """``steps`` lists of row indices: each step a fresh seeded permutation's leading rows, as many as fit into
    ``batch_seconds`` (one at the least)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    plan = []
    for _ in range(steps):
        rows, total = [], 0.0
        for i in rng.permutation(len(durations)):
            if rows and total + durations[i] > batch_seconds:
                break
            rows.append(int(i))
            total += durations[i]
        plan.append(rows)
    return plan


@click.command()
@click.option("--ckpt", "-c", required=True, type=str, help="path to the checkpoint")
@click.option("--folder", "-f", required=True, type=str, help="folder with transcriptions.csv and its wavs")
@click.option("--vocab", default=None, type=str, help="vocab.yaml of the new phoneme set (default: the checkpoint's)")
@click.option("--steps", default=200, type=int, help="optimiser steps (OneCycleLR's total_steps)")
@click.option("--batch_seconds", default=60.0, type=float, help="audio per step at the most")
@click.option("--batch_size", default=16, type=int, help="max files per encoder batch while caching")
@click.option("--lr", default=1e-3, type=float, help="OneCycleLR's max_lr of the head")
@click.option("--weight_decay", default=0.1, type=float)
@click.option("--clip", default=0.5, type=float, help="gradient norm clip (0: none)")
@click.option("--seed", default=0, type=int)
@click.option("--hubert_path", default=None, type=str, help="override hubert_config.model_path")
@click.option("--out", "-o", required=True, type=str, help="the checkpoint to write")
@click.option("--log", default=None, type=str, help="JSON lines, one per step")
@click.option("--log_every", default=50, type=int, help="read the losses back every this many steps")
def main(ckpt, folder, vocab, steps, batch_seconds, batch_size, lr, weight_decay, clip, seed, hubert_path, out, log,
         log_every):
    import numpy as np
    import torch
    import yaml
    from hubertfa_amd.labels import read_transcriptions
    from hubertfa_amd.task import ForcedAlignmentTask
    from hubertfa_amd.train import LOSS_NAMES, HeadTrainer
    from hubertfa_amd.wav_io import read_wav

    root = pathlib.Path(folder)
    task = ForcedAlignmentTask.load_from_checkpoint(ckpt, device=torch.device("cuda"), hubert_model_path=hubert_path)
    loss_config = task.hparams.get("loss_config") or {}
    if not loss_config.get("function"):
        loss_config = DEFAULT_LOSS_CONFIG
    optimizer_config = {"lr": {"backbone": 0.0, "head": lr}, "weight_decay": weight_decay, "total_steps": steps,
                        "freeze": {"backbone": True, "head": False}}
    new_vocab = yaml.safe_load(open(vocab, encoding="utf-8")) if vocab else None
    trainer = HeadTrainer(task, optimizer_config, loss_config, gradient_clip_val=clip, vocab=new_vocab, seed=seed)

    loaded = []
    for it in read_transcriptions(root):
        path = next((p for p in (root / f"{it['name']}.wav", root / "wavs" / f"{it['name']}.wav") if p.exists()), None)
        if path is None:
            raise SystemExit(f"{it['name']}: no wav beside transcriptions.csv or under wavs/")
        x, sr = read_wav(str(path))
        loaded.append((it, x[0], sr))
    if not loaded:
        raise SystemExit("transcriptions.csv lists no file")
    for sr in sorted({sr for _, _, sr in loaded}):
        group = [(it, x) for it, x, s in loaded if s == sr]
        for i in range(0, len(group), batch_size):
            part = group[i:i + batch_size]
            lens = [len(x) for _, x in part]
            wav = np.zeros((len(part), max(lens)), np.float32)
            for r, (_, x) in enumerate(part):
                wav[r, :len(x)] = x
            trainer.cache(task.upload(wav), [it for it, _ in part], wav_sr=sr, lengths=lens if len(part) > 1 else None)
    durations = [r["T"] * trainer.frame_length for r in trainer.rows]

    pending = []
    fh = open(log, "w", encoding="utf-8") if log else None

    def flush():
        trainer.check_range()                                 # (a head outside the split GEMM's range stops the run)
        for k, lr_k, b1_k, vals in pending:                   # (the only reads from the device)
            rec = {"step": k, "lr": lr_k, "beta1": b1_k}
            rec.update({n: float(v) for n, v in zip(LOSS_NAMES + ("total_loss",), vals)})
            if fh is not None:
                fh.write(json.dumps(rec) + "\n")
        pending.clear()
        if fh is not None:
            fh.flush()

    for k, rows in enumerate(batch_plan(durations, steps, batch_seconds, seed)):
        lr_k, b1_k = trainer.schedule()
        pending.append((k, lr_k, b1_k, trainer.step(rows)))
        if len(pending) >= max(log_every, 1):
            flush()
    flush()
    if fh is not None:
        fh.close()
    trainer.save(out)
    print(f"{len(trainer.rows)} file(s), {steps} step(s), {int(trainer.skipped)} skipped -> {out}")


if __name__ == "__main__":
    main()
