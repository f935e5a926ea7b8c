"""Training-prep features of a folder of WAVs (reference: binarize.py:273-302 make_input_feature), one GPU.

    python extract_features.py -c model.ckpt -f segments [--batch_size 32] [--hubert_path synth:0]

For every ``*.wav`` under the folder: the Hubert units on the melspec frame grid and the log-mel spectrogram, written
to ``<wav dir>/features/<name>.npz`` with keys ``input_feature`` [1, C, T], ``melspec`` [1, n_mels, T] and
``wav_length`` (seconds).  Files are read and batched as infer.py does (headers first, per sample rate, sorted by
length, rows zero-padded and processed with per-row lengths), so every file's arrays equal the ones it gives alone.
No transcripts, no G2P, no multi-GPU.
"""
from __future__ import annotations

import pathlib

import click


@click.command()
@click.option("--ckpt", "-c", default=None, required=True, type=str, help="path to the checkpoint")
@click.option("--folder", "-f", default="segments", type=str, help="path to the input folder")
@click.option("--batch_size", default=32, type=int, help="max files per GPU batch (variable lengths; results equal B=1)")
@click.option("--hubert_path", default=None, type=str, help="override hubert_config.model_path")
def main(ckpt, folder, batch_size, hubert_path):
    import numpy as np
    import torch
    from hubertfa_amd.batching import plan_batches
    from hubertfa_amd.task import ForcedAlignmentTask
    from hubertfa_amd.wav_io import read_wav_into, wav_info

    torch.set_grad_enabled(False)
    task = ForcedAlignmentTask.load_from_checkpoint(ckpt, device=torch.device("cuda"), hubert_model_path=hubert_path)
    task.on_predict_start()
    sr = task.melspec_config["sample_rate"]
    items, errors = {}, []
    for path in sorted(pathlib.Path(folder).rglob("*.wav")):
        try:
            n, file_sr, _ = wav_info(path)
            items[path] = (n, file_sr)
        except (OSError, ValueError) as e:
            errors.append((path, e))
    plan = plan_batches([(k, n, fsr) for k, (n, fsr) in items.items()], batch_size, sr,
                        task.unitsEncoder.encoder_sample_rate)
    done = 0
    for file_sr, paths in plan:
        lens = [items[p][0] for p in paths]
        wav_h = torch.zeros((len(paths), max(lens)), dtype=torch.float32, pin_memory=True)
        wav_np = wav_h.numpy()
        try:
            for r, p in enumerate(paths):
                got, _ = read_wav_into(p, wav_np[r], channel=0)          # channel 0, as the reference's waveform[0]
                if got != lens[r]:
                    raise ValueError(f"{p}: {got} samples read, the header said {lens[r]}")
            rows = task.make_input_feature(task.upload(wav_h), wav_sr=file_sr,
                                           lengths=lens if len(paths) > 1 else None)
        except ValueError as e:                                          # one input's failure: logged, the run goes on
            errors += [(p, e) for p in paths]
            continue
        for p, (units, mel, wav_length) in zip(paths, rows):
            out = p.parent / "features"
            out.mkdir(exist_ok=True)
            np.savez(out / (p.stem + ".npz"), input_feature=units.cpu().numpy(), melspec=mel.cpu().numpy(),
                     wav_length=np.float64(wav_length))
            done += 1
    for p, e in errors:
        print(f"[error] {p}: {e}")
    print(f"{done} feature file(s) written under <wav dir>/features ({len(errors)} error(s)).")
    if errors:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
