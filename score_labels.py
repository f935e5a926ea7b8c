"""Rank a labelled folder's files by how badly the model explains their labels (reference: the full-label terms of
_get_loss, networks/task/forced_alignment.py:188-254, on targets built as binarize.py:179-271 builds them), one GPU.

    python score_labels.py -c model.ckpt -f folder [--batch_size 16] [--hubert_path synth:0]

``folder`` holds ``transcriptions.csv`` (``name``, ``ph_seq``, ``ph_dur``, the reference's training layout) and the
``<name>.wav`` files it lists, beside it or under ``wavs/``.  Writes ``<folder>/label_losses.csv``, one row per file:
``name``, the four full-label losses over the file's own frames (ph_frame_GHM_loss, ph_edge_GHM_loss, ph_edge_EMD_loss,
ph_edge_diff_loss), ``total`` (their sum under the checkpoint's loss weights), ``ctc_nll`` and ``frames``; the worst
``total`` first, then a ``MEAN`` row of the corpus means.  It is a loop over ForcedAlignmentTask.loss_batch: files are
batched in the CSV's order per sample rate, rows zero-padded with per-row lengths, so a file's row is the one it gives
alone.  The GHM tables are the checkpoint's (ones where it has none) and are not updated.
"""
from __future__ import annotations

import csv
import math
import pathlib

import click

LOSSES = ("ph_frame_GHM_loss", "ph_edge_GHM_loss", "ph_edge_EMD_loss", "ph_edge_diff_loss")
COLUMNS = ("name",) + LOSSES + ("total", "ctc_nll", "frames")


@click.command()
@click.option("--ckpt", "-c", required=True, type=str, help="path to the checkpoint")
@click.option("--folder", "-f", required=True, type=str, help="folder with transcriptions.csv and its wavs")
@click.option("--batch_size", default=16, type=int, help="max files per GPU batch (results equal B=1)")
@click.option("--hubert_path", default=None, type=str, help="override hubert_config.model_path")
def main(ckpt, folder, batch_size, hubert_path):
    import numpy as np
    import torch
    from hubertfa_amd.labels import read_transcriptions
    from hubertfa_amd.losses import FALoss
    from hubertfa_amd.task import ForcedAlignmentTask
    from hubertfa_amd.wav_io import read_wav

    root = pathlib.Path(folder)
    task = ForcedAlignmentTask.load_from_checkpoint(ckpt, device=torch.device("cuda"), hubert_model_path=hubert_path)
    cfg = task.hparams.get("loss_config") or {}
    if cfg.get("function"):                                   # the checkpoint's own tables, where it carries them
        sd = torch.load(ckpt, map_location="cpu", weights_only=True)["state_dict"]
        task._fa_loss = FALoss.from_checkpoint(sd, cfg, vocab_size=task.vocab["vocab_size"], device=task.device)
    weights = task.fa_loss.weights.tolist()[:4]

    loaded = []
    for it in read_transcriptions(root):
        path = next((p for p in (root / f"{it['name']}.wav", root / "wavs" / f"{it['name']}.wav") if p.exists()), None)
        if path is None:
            raise SystemExit(f"{it['name']}: no wav beside transcriptions.csv or under wavs/")
        x, sr = read_wav(str(path))
        loaded.append((it, x[0], sr))
    rows = []
    for sr in sorted({sr for _, _, sr in loaded}):
        group = [(it, x) for it, x, s in loaded if s == sr]
        for i in range(0, len(group), batch_size):
            part = group[i:i + batch_size]
            lens = [len(x) for _, x in part]
            wav = np.zeros((len(part), max(lens)), np.float32)
            for r, (_, x) in enumerate(part):
                wav[r, :len(x)] = x
            res = task.loss_batch(task.upload(wav), [it for it, _ in part], wav_sr=sr,
                                  lengths=lens if len(part) > 1 else None)
            for (it, _), r in zip(part, res["rows"]):
                r = dict(r, name=it["name"])
                r["total"] = sum(w * r[k] for w, k in zip(weights, LOSSES))
                rows.append(r)
    rows.sort(key=lambda r: (-r["total"] if not math.isnan(r["total"]) else math.inf, r["name"]))
    mean = {"name": "MEAN", "frames": sum(r["frames"] for r in rows)}
    for k in LOSSES + ("total", "ctc_nll"):
        v = [r[k] for r in rows if not math.isnan(r[k])]
        mean[k] = sum(v) / len(v) if v else float("nan")
    out = root / "label_losses.csv"
    with open(out, "w", newline="", encoding="utf-8") as f:
        w = csv.writer(f)
        w.writerow(COLUMNS)
        for r in rows + [mean]:
            w.writerow([repr(r[c]) if isinstance(r[c], float) else r[c] for c in COLUMNS])
    print(f"{len(rows)} file(s) scored -> {out}")


if __name__ == "__main__":
    main()
