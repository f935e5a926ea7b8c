"""Labels -> training targets: the reference's ForcedAlignmentBinarizer.make_ph_data (binarize.py:179-271) and a reader
for its ``transcriptions.csv`` (name, ph_seq, ph_dur), so a labelled corpus can be fed to hubertfa_amd.losses.FALoss.

Host-side numpy; nothing here touches the GPU.
"""
from __future__ import annotations

import csv
import os

import numpy as np

LABEL_TYPES = {"no_label": 0, "weak_label": 1, "full_label": 2, "evaluate": 3}


def make_ph_data(vocab, T, label_type_id, ph_id_seq, ph_dur, frame_length):
    """binarize.py:179-271 restated, quirks included.  ``vocab``: a dict with "vocab_size" (or the size itself); T: the
    item's frame count; label_type_id 0 none / 1 weak (phones only) / >= 2 full (phones and durations in seconds);
    frame_length: seconds per frame (hop_length / sample_rate).  Returns (ph_id_seq [S] i32 without SP, ph_edge [T]
    f32, ph_frame [T] i32, ph_mask [vocab_size] i32, ph_time) or five Nones (binarize.py:201, :237, :270: a weak item
    of SP only, and a negative label type).  As in the reference, boundaries are deduplicated and sorted by np.unique,
    rounded half to even by np.round, a boundary within half a frame of 0 or T is dropped, and the soft edge is
    0.1 + 0.8 (0.5 +- fraction) on the two frames around each boundary; a FULL item whose phones are all SP raises
    IndexError (binarize.py:233 indexes the empty boundary list before :237 can return)."""
    V = int(vocab["vocab_size"]) if isinstance(vocab, dict) else int(vocab)
    T = int(T)
    if label_type_id == 0:
        return (np.array([]).astype("int32"), np.zeros([T], dtype="float32"), np.zeros(T, dtype="int32"),
                np.ones(V, dtype="int32"), np.zeros(T, dtype="float32"))
    if label_type_id == 1:
        ids = np.array(ph_id_seq).astype("int32")
        ids = ids[ids != 0]
        if len(ids) <= 0:
            return None, None, None, None, None
        ph_mask = np.zeros(V, dtype="int32")
        ph_mask[ids] = 1
        ph_mask[0] = 1
        return ids, np.zeros([T], dtype="float32"), np.zeros(T, dtype="int32"), ph_mask, np.zeros(T, dtype="float32")
    if not label_type_id >= 2:
        return None, None, None, None, None

    ids = np.array(ph_id_seq).astype("int32")
    not_sp = ids != 0
    ids = ids[not_sp]
    dur = np.array(ph_dur).astype("float32")
    ph_time = np.array(np.concatenate(([0], dur))).cumsum()              # float64 sums of the float32 durations
    pos = ph_time / frame_length
    interval = np.stack((pos[:-1], pos[1:]))[:, not_sp]
    ph_time = ph_time[:-1][not_sp]
    bounds = np.unique(interval.flatten())
    if bounds[-1] >= T:
        bounds = bounds[:-1]
    if len(ids) <= 0:
        return None, None, None, None, None
    ph_edge = np.zeros([T], dtype="float32")
    if bounds[-1] + 0.5 > T:
        bounds = bounds[:-1]
    if bounds[0] - 0.5 < 0:
        bounds = bounds[1:]
    at = np.round(bounds).astype("int32")
    frac = bounds - at
    ph_edge[at] = 0.5 + frac
    ph_edge[at - 1] = 0.5 - frac
    ph_edge = ph_edge * 0.8 + 0.1
    ph_frame = np.zeros(T, dtype="int32")
    for ph_id, st, ed in zip(ids, interval[0], interval[1]):
        st, ed = max(st, 0), min(ed, T)
        ph_frame[int(np.round(st)): int(np.round(ed))] = ph_id
    ph_mask = np.zeros(V, dtype="int32")
    ph_mask[ids] = 1
    ph_mask[0] = 1
    return ids, ph_edge, ph_frame, ph_mask, ph_time


def read_transcriptions(path):
    """The rows of a reference ``transcriptions.csv``: a list of dicts name, ph_seq (list of phone names), ph_dur (list
    of seconds, empty when the column is absent or blank: a weak label).  ``path``: the file or its folder."""
    if os.path.isdir(path):
        path = os.path.join(path, "transcriptions.csv")
    rows = []
    with open(path, newline="", encoding="utf-8") as fh:
        for r in csv.DictReader(fh):
            if not r.get("name"):
                continue
            ph_seq = (r.get("ph_seq") or "").split()
            durs = [float(d) for d in (r.get("ph_dur") or "").split()]
            if durs and len(durs) != len(ph_seq):
                raise ValueError(f"{path}: {r['name']}: {len(ph_seq)} phones, {len(durs)} durations")
            rows.append({"name": r["name"], "ph_seq": ph_seq, "ph_dur": durs})
    return rows
