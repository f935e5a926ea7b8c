"""Record tests/golden/fa_loss.npz by running the reference's own loss modules and label conversion on the CPU.

Run:  python tests/golden/gen_fa_loss.py        (needs the reference checkout; skips itself otherwise)

What runs is the reference's code: LitForcedAlignmentTask._get_loss (networks/task/forced_alignment.py:188-282) on an
object that carries its GHMLoss, MultiLabelGHMLoss, BinaryEMDLoss and CTCGHMLoss instances, once in float64 and once in
float32, with valid=False (the tables after one update are recorded) and valid=True (they must not move); the gradient is
autograd's.  ForcedAlignmentBinarizer.make_ph_data (binarize.py:179-271) runs on an object that carries frame_length.
Imports that are absent here (lightning, textgrid, torchaudio, h5py, numba) are stubbed the way gen_golden.py stubs numba:
none of them is touched by what runs.

Inputs come from tests/fa_loss_ref.py's draw_case, i.e. from seeds that keep the margin from every bin edge and sign
change.  Everything written is DATA (inputs + expected outputs).  No reference source is copied.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, os.path.dirname(HERE))          # tests/ (fa_loss_ref)

import fa_loss_ref as ref  # noqa: E402

V, NB, ALPHA = 20, 10, 0.9
CASES = [  # name, Ts, label types, label smoothing, seed
    ("ls0", (200, 131, 64), (2, 2, 2), 0.0, 11),
    ("ls01", (200, 131, 64), (2, 3, 2), 0.1, 12),
    ("mixed", (180, 200, 97, 150), (0, 1, 2, 3), 0.1, 13),
]
PH_CASES = [  # name, T, label_type_id, ph ids, durations (s)
    ("sp_inside", 60, 2, [3, 0, 5, 7, 0], [0.113, 0.05, 0.2049, 0.131, 0.1]),
    ("ends_at_T", 50, 2, [4, 9, 2], [0.15, 0.25, 0.10]),
    ("beyond_T", 40, 2, [6, 1, 8, 3], [0.123, 0.2, 0.15, 0.3]),
    ("half_frames", 30, 2, [2, 3, 4, 5], [0.025, 0.045, 0.055, 0.1]),
    ("leading_sp", 45, 3, [0, 11, 12], [0.0837, 0.2, 0.15]),
    ("all_sp_full", 20, 2, [0, 0], [0.1, 0.1]),
    ("all_sp_weak", 20, 1, [0], [0.2]),
    ("weak", 33, 1, [5, 0, 6, 5], [0.1, 0.1, 0.1, 0.03]),
    ("none", 25, 0, [1, 2], [0.1, 0.15]),
    ("negative_type", 25, -1, [1, 2], [0.1, 0.15]),
]


class _Anything:
    def __init__(self, *a, **k):
        pass


class _Stub(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Anything


def _import_reference():
    import transformers  # noqa: F401  (it probes torchaudio's presence: imported before the stub exists)
    from transformers import Wav2Vec2FeatureExtractor, HubertModel  # noqa: F401
    for n in ("lightning", "textgrid", "torchaudio", "torchaudio.transforms", "h5py", "numba"):
        try:
            __import__(n)
        except ImportError:
            sys.modules[n] = _Stub(n)
    if isinstance(sys.modules.get("numba"), _Stub):
        sys.modules["numba"].jit = lambda f=None, **kw: f if f is not None else (lambda g: g)
    sys.path.insert(0, REF)
    from networks.task.forced_alignment import LitForcedAlignmentTask
    from networks.loss.GHMLoss import CTCGHMLoss, GHMLoss, MultiLabelGHMLoss
    from networks.loss.BinaryEMDLoss import BinaryEMDLoss
    from binarize import ForcedAlignmentBinarizer
    return LitForcedAlignmentTask, GHMLoss, MultiLabelGHMLoss, BinaryEMDLoss, CTCGHMLoss, ForcedAlignmentBinarizer


def _owner(mods, tables, ls, dtype):
    _, GHMLoss, MultiLabelGHMLoss, BinaryEMDLoss, CTCGHMLoss, _ = mods
    o = types.SimpleNamespace()
    o.ph_frame_GHM_loss_fn = GHMLoss(V, NB, ALPHA, ls)
    o.ph_edge_GHM_loss_fn = MultiLabelGHMLoss(1, NB, ALPHA, label_smoothing=0.0)
    o.ph_edge_diff_GHM_loss_fn = MultiLabelGHMLoss(1, NB, ALPHA, label_smoothing=0.0)
    o.EMD_loss_fn = BinaryEMDLoss()
    o.CTC_GHM_loss_fn = CTCGHMLoss(alpha=1 - 1e-3)
    for name, v in tables.items():
        fn, buf = name.split(".")
        setattr(getattr(o, fn), buf, torch.tensor(np.asarray(v, np.float64)).to(dtype))
    return o


def _tables_of(o, names):
    return {n: getattr(getattr(o, n.split(".")[0]), n.split(".")[1]).detach().double().numpy() for n in names}


def gen_losses(mods, arrays):
    Task = mods[0]
    names = ref.TABLES + (ref.CTC_TABLE,)
    for name, Ts, lts, ls, seed in CASES:
        B, Tmax = len(Ts), 200
        inp, out = ref.draw_case(B, Tmax, V, Ts, lts, seed, NB, ls)
        assert ref.margins_ok(out)
        r = np.random.default_rng(seed + 99)
        Ls = [0 if lt == 0 else int(r.integers(3, 30)) for lt in lts]
        seq = np.zeros((B, max(Ls)), np.int64)
        for b, L in enumerate(Ls):
            seq[b, :L] = r.integers(1, V, L)
        p = f"{name}_"
        for k in ("logits", "T", "label_type", "ph_frame", "ph_edge", "ph_mask"):
            arrays[p + k] = inp[k]
        arrays[p + "ph_id_seq"], arrays[p + "L"] = seq.astype(np.int32), np.asarray(Ls, np.int32)
        arrays[p + "cfg"] = np.asarray([NB, ALPHA, ls, inp["seed"]], np.float64)
        for n in names:
            arrays[p + "in." + n] = inp["tables"][n]
        for tag, dtype in (("f64", torch.float64), ("f32", torch.float32)):
            for valid in (False, True):
                o = _owner(mods, inp["tables"], ls, dtype)
                x = torch.tensor(inp["logits"]).to(dtype).requires_grad_(True)
                time_len = torch.tensor(inp["T"]).long()
                losses = Task._get_loss(
                    o, x[:, :, 2:], x[:, :, 0], torch.cat([x[:, :, 1:2], x[:, :, 3:]], dim=-1),
                    torch.tensor(inp["ph_frame"]).long(), torch.tensor(inp["ph_edge"]).to(dtype), torch.tensor(seq),
                    torch.tensor(Ls).long(), torch.tensor(inp["ph_mask"]).to(dtype), time_len,
                    torch.tensor(inp["label_type"]).long(), valid)
                w = torch.tensor([1.0, 0.7, 1.3, 0.4, 0.9], dtype=torch.float64).to(dtype)
                sum(wi * li for wi, li in zip(w[:4], losses[:4])).backward(retain_graph=True)
                grad4 = x.grad.double().numpy().copy()           # the four full-label terms alone
                (w[4] * losses[4]).backward()
                after = _tables_of(o, names)
                if valid:
                    for n in names:               # valid=True leaves every table alone
                        assert np.array_equal(after[n], np.asarray(inp["tables"][n], np.float64).astype(
                            np.float32 if tag == "f32" else np.float64).astype(np.float64)), n
                    arrays[p + tag + "_losses_valid"] = np.asarray([float(v.detach()) for v in losses], np.float64)
                    continue
                arrays[p + tag + "_losses"] = np.asarray([float(v.detach()) for v in losses], np.float64)
                arrays[p + tag + "_grad"] = x.grad.double().numpy()
                arrays[p + tag + "_grad4"] = grad4
                for n in names:
                    arrays[p + tag + "_after." + n] = after[n]
        arrays[p + "grad_weights"] = np.asarray([1.0, 0.7, 1.3, 0.4, 0.9])
        e = np.abs(arrays[p + "f32_losses"] - arrays[p + "f64_losses"])
        print(name, "losses f64", arrays[p + "f64_losses"], "f32 err", e, "grad f32 err",
              np.abs(arrays[p + "f32_grad4"] - arrays[p + "f64_grad4"]).max(), "max |g|",
              np.abs(arrays[p + "f64_grad4"]).max())


def gen_ph_data(mods, arrays):
    Binarizer = mods[5]
    me = types.SimpleNamespace(frame_length=441 / 44100)
    arrays["ph_names"] = np.asarray([c[0] for c in PH_CASES])
    arrays["ph_frame_length"] = np.asarray(me.frame_length)
    for name, T, lt, ids, durs in PH_CASES:
        p = f"ph_{name}_"
        arrays[p + "T"], arrays[p + "type"] = np.asarray(T), np.asarray(lt)
        arrays[p + "ids"], arrays[p + "durs"] = np.asarray(ids, np.int64), np.asarray(durs, np.float64)
        try:
            out = Binarizer.make_ph_data(me, {"vocab_size": V}, T, lt, ids, durs)
        except IndexError:                        # full labels that are all SP: binarize.py:233 indexes an empty array
            arrays[p + "raises"] = np.asarray(True)
            print(name, "IndexError")
            continue
        arrays[p + "raises"] = np.asarray(False)
        arrays[p + "none"] = np.asarray(out[0] is None)
        if out[0] is not None:
            for k, v in zip(("ph_id_seq", "ph_edge", "ph_frame", "ph_mask", "ph_time"), out):
                arrays[p + k] = np.asarray(v)
        print(name, "None" if out[0] is None else [np.asarray(v).shape for v in out])


def main():
    if not os.path.isdir(REF):
        print("reference absent: fixtures are generated only where it is checked out; skipping")
        return
    torch.manual_seed(0)
    mods = _import_reference()
    arrays = {}
    gen_losses(mods, arrays)
    gen_ph_data(mods, arrays)
    path = os.path.join(HERE, "fa_loss.npz")
    np.savez_compressed(path, **arrays)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
