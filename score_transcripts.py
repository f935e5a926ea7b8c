"""Score a folder's transcripts against its audio with the CTC head (reference: the weak-label CTC likelihood of
networks/task/forced_alignment.py:256-272 and the greedy decode of tools/alignment_decoder.py:145-150), one GPU.

    python score_transcripts.py -c model.ckpt -f segments -g Dictionary -d dict.txt [--batch_size 32]
                                [--hubert_path synth:0] [--phones]

Pairs every ``*.wav`` under the folder with its ``*.lab`` through the G2P plugins exactly as infer.py does, and writes
``<folder>/ctc_scores.csv`` with one row per file: ``name``, ``n_frames``, ``n_phones`` (the transcript's non-SP
phones), ``ctc_nll`` = -log P(transcript | audio), ``ctc_confidence`` = clip(exp(-nll / n_frames), 1e-6, 1 - 1e-6),
``ctc_phones`` (the transcript-free greedy decode, space-joined) and ``phone_edit_distance`` (Levenshtein between
``ctc_phones`` and the transcript's non-SP phones).  Rows are sorted by ``ctc_confidence`` ascending: the files whose
transcript least belongs to their audio come first.  Files are read and batched as infer.py does (headers first, per
sample rate, sorted by length, rows zero-padded and processed with per-row lengths), so every file's row equals the
one it gives alone.  A batch that fails on one input is re-run file by file; a file that fails alone is logged and
skipped.  No alignment, no multi-GPU.

``--phones`` also writes ``<folder>/ctc_phone_scores.csv`` from the CTC forward-backward (ops.ctc_posteriors), one row
per (file, non-SP transcript phone): ``name``, ``index`` (among the file's non-SP phones), ``phone``, ``centre_s`` (the
phone's expected position), ``frames`` (its expected frame count) and ``confidence`` = exp of the posterior-weighted
mean log-probability of the phone where the model places it: the phone that is wrong stands out as the file's lowest.
Files come in ``ctc_scores.csv``'s order, phones in transcript order; a file whose transcript does not fit its frames
gets its rows with confidence 0.  ``ctc_scores.csv`` has the same bytes with and without the flag.
"""
from __future__ import annotations

import csv
import pathlib

import click

COLUMNS = ("name", "n_frames", "n_phones", "ctc_nll", "ctc_confidence", "ctc_phones", "phone_edit_distance")


def edit_distance(a, b) -> int:
    """Levenshtein distance between two sequences (insertions, deletions, substitutions, each 1)."""
    a, b = list(a), list(b)
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i]
        for j, y in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (x != y)))
        prev = cur
    return prev[-1]


def score_row(name, result, ph_seq, vocab) -> dict:
    """One CSV row from a file's ctc_score_batch result and its transcript (``vocab``: phoneme -> id; id 0 is SP)."""
    phones = [p for p in ph_seq if vocab[p] != 0]
    return dict(name=name, n_frames=int(result["T"]), n_phones=len(phones), ctc_nll=float(result["ctc_nll"]),
                ctc_confidence=float(result["ctc_confidence"]), ctc_phones=" ".join(result["ctc_phones"]),
                phone_edit_distance=edit_distance(result["ctc_phones"], phones))


PHONE_COLUMNS = ("name", "index", "phone", "centre_s", "frames", "confidence")


def phone_rows(name, result, ph_seq, vocab) -> list:
    """The ``--phones`` rows of one file from its ctc_score_batch(posteriors=True) result and its transcript."""
    phones = [p for p in ph_seq if vocab[p] != 0]
    return [dict(name=name, index=j, phone=p, centre_s=float(result["ctc_phone_centre_s"][j]),
                 frames=float(result["ctc_phone_frames"][j]), confidence=float(result["ctc_phone_confidence"][j]))
            for j, p in enumerate(phones)]


def write_phone_csv(path, names, rows_by_name) -> None:
    """Write the phone rows of the files ``names`` in that order (write_csv's), each file's in transcript order."""
    with open(path, "w", newline="", encoding="utf-8") as f:
        w = csv.writer(f)
        w.writerow(PHONE_COLUMNS)
        for n in names:
            for r in rows_by_name[n]:
                w.writerow([repr(r[c]) if isinstance(r[c], float) else r[c] for c in PHONE_COLUMNS])


def write_csv(path, rows) -> list:
    """Write ``rows`` (dicts with COLUMNS) sorted by ctc_confidence ascending (ties by name); returns them sorted.
    Floats are written with repr, so reading them back gives the same values."""
    rows = sorted(rows, key=lambda r: (r["ctc_confidence"], r["name"]))
    with open(path, "w", newline="", encoding="utf-8") as f:
        w = csv.writer(f)
        w.writerow(COLUMNS)
        for r in rows:
            w.writerow([repr(r[c]) if isinstance(r[c], float) else r[c] for c in COLUMNS])
    return rows


@click.command()
@click.option("--ckpt", "-c", default=None, required=True, type=str, help="path to the checkpoint")
@click.option("--folder", "-f", default="segments", type=str, help="path to the input folder")
@click.option("--g2p", "-g", default="Dictionary", type=str, help="name of the g2p class")
@click.option("--dictionary", "-d", default="dictionary/opencpop-extension.txt", type=str,
              help="(only used when --g2p=='Dictionary') path to the dictionary")
@click.option("--batch_size", default=32, type=int, help="max files per GPU batch (variable lengths; results equal B=1)")
@click.option("--hubert_path", default=None, type=str, help="override hubert_config.model_path")
@click.option("--phones", is_flag=True, help="also write ctc_phone_scores.csv: one row per non-SP transcript phone")
def main(ckpt, folder, g2p, batch_size, hubert_path, phones, **kwargs):
    import torch
    import hubertfa_amd.g2p as g2p_mod
    from hubertfa_amd._lib import HFAArgumentError
    from hubertfa_amd.batching import plan_batches
    from hubertfa_amd.task import ForcedAlignmentTask
    from hubertfa_amd.wav_io import read_wav_into, wav_info

    if not g2p.endswith("G2P"):
        g2p += "G2P"
    grapheme_to_phoneme = getattr(g2p_mod, g2p)(**kwargs)
    grapheme_to_phoneme.set_in_format("lab")
    dataset = list(grapheme_to_phoneme.get_dataset(sorted(pathlib.Path(folder).rglob("*.wav"))))

    torch.set_grad_enabled(False)
    task = ForcedAlignmentTask.load_from_checkpoint(ckpt, device=torch.device("cuda"), hubert_model_path=hubert_path)
    task.on_predict_start()
    sr = task.melspec_config["sample_rate"]
    vocab = task.vocab["vocab"]
    items, errors = {}, []
    for wav_path, ph_seq, _, _ in dataset:
        path = pathlib.Path(wav_path)
        try:
            n, file_sr, _ = wav_info(path)
            items[path] = (n, file_sr, ph_seq)
        except (OSError, ValueError) as e:
            errors.append((path, e))
    plan = plan_batches([(k, n, fsr) for k, (n, fsr, _) in items.items()], batch_size, sr,
                        task.unitsEncoder.encoder_sample_rate)
    recoverable = (HFAArgumentError, ValueError, KeyError, IndexError)   # one input's failure: the GPU stays healthy
    root = pathlib.Path(folder)
    rows, by_name = [], {}
    kw = dict(posteriors=True) if phones else {}

    def score(paths, file_sr):
        lens = [items[p][0] for p in paths]
        wav_h = torch.zeros((len(paths), max(lens)), dtype=torch.float32, pin_memory=True)
        wav_np = wav_h.numpy()
        for r, p in enumerate(paths):
            got, _ = read_wav_into(p, wav_np[r], channel=0)              # channel 0, as the reference's waveform[0]
            if got != lens[r]:
                raise ValueError(f"{p}: {got} samples read, the header said {lens[r]}")
        res = task.ctc_score_batch(task.upload(wav_h), [items[p][2] for p in paths], wav_sr=file_sr,
                                   lengths=lens if len(paths) > 1 else None, **kw)
        names = [str(p.relative_to(root).with_suffix("")) for p in paths]
        if phones:
            for n, p, r in zip(names, paths, res):
                by_name[n] = phone_rows(n, r, items[p][2], vocab)
        return [score_row(n, r, items[p][2], vocab) for n, p, r in zip(names, paths, res)]

    for file_sr, paths in plan:
        try:
            rows += score(paths, file_sr)
        except recoverable as e:
            if len(paths) == 1:
                errors.append((paths[0], e))
                continue
            for p in paths:                                              # re-run file by file: one bad input
                try:
                    rows += score([p], file_sr)
                except recoverable as e1:
                    errors.append((p, e1))
    out = root / "ctc_scores.csv"
    rows = write_csv(out, rows)
    if phones:
        write_phone_csv(root / "ctc_phone_scores.csv", [r["name"] for r in rows], by_name)
    for p, e in errors:
        print(f"[error] {p}: {e!r}")
    print(f"{len(rows)} transcript(s) scored -> {out} ({len(errors)} error(s)).")
    if errors:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
