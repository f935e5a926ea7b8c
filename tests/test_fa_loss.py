"""The alignment-loss yardstick and the host-side pieces, without a GPU: tests/fa_loss_ref.py (the float64 restatement
that test_fa_loss_gpu.py holds the kernels to) against tests/golden/fa_loss.npz, which records what the reference's own
GHMLoss / MultiLabelGHMLoss / BinaryEMDLoss / CTCGHMLoss and make_ph_data computed (tests/golden/gen_fa_loss.py);
hubertfa_amd.labels.make_ph_data against the same fixture, exactly; FALoss's table update and checkpoint round trip."""
import json
import os

import numpy as np
import pytest

import fa_loss_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ("ls0", "ls01", "mixed")


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "fa_loss.npz"))


def load_case(fx, name):
    p = name + "_"
    inp = {k: fx[p + k] for k in ("logits", "T", "label_type", "ph_frame", "ph_edge", "ph_mask", "ph_id_seq", "L")}
    nb, alpha, ls, _seed = fx[p + "cfg"]
    inp.update(num_bins=int(nb), alpha=float(alpha), label_smoothing=float(ls), weights=fx[p + "grad_weights"],
               tables={n: fx[p + "in." + n] for n in ref.TABLES + (ref.CTC_TABLE,)})
    return inp


def restate(inp, dtype=np.float64):
    out = ref.run(inp["logits"], inp["T"], inp["label_type"], inp["ph_frame"], inp["ph_edge"], inp["ph_mask"],
                  inp["tables"], inp["num_bins"], inp["label_smoothing"], dtype)
    seqs = [inp["ph_id_seq"][b, :inp["L"][b]] for b in range(len(inp["L"]))]
    out["ctc"] = ref.ctc_term(inp["logits"], inp["T"], inp["label_type"], seqs, inp["tables"][ref.CTC_TABLE])
    return out


def tables_after(inp, out, dtype=np.float64):
    """One update (valid=False) of every table from the restatement's counts."""
    after = {}
    for n in ref.TABLES:
        h = out["hist"][n]
        hd = np.float32 if n.startswith("ph_edge_GHM_loss_fn") else None     # (see fa_loss_ref.update_ema)
        after[n] = ref.update_ema(inp["tables"][n], inp["alpha"], len(h), h, dtype, hd) if h.sum() else \
            np.asarray(inp["tables"][n], dtype)
    h = out["ctc"][2]
    after[ref.CTC_TABLE] = ref.update_ema(inp["tables"][ref.CTC_TABLE], 1 - 1e-3, len(h), h, dtype) if h.sum() else \
        np.asarray(inp["tables"][ref.CTC_TABLE], dtype)
    return after


@pytest.mark.parametrize("name", CASES)
def test_restatement_matches_reference_f64(fx, name):
    inp = load_case(fx, name)
    out = restate(inp)
    assert ref.margins_ok(out), out["margin"]
    p = name + "_"
    want = fx[p + "f64_losses"]
    got = np.concatenate([out["losses"], [out["ctc"][0]]])
    print(name, "losses", got, "|err|", np.abs(got - want))
    assert np.all(np.abs(got - want) <= 1e-10 * np.maximum(1, np.abs(want)))
    assert np.array_equal(fx[p + "f64_losses_valid"], want)          # valid=True: the same losses
    w = inp["weights"]
    g4 = np.tensordot(w[:4], out["grads"], axes=1)
    assert np.abs(g4 - fx[p + "f64_grad4"]).max() <= 1e-10
    assert np.abs(g4 + w[4] * out["ctc"][1] - fx[p + "f64_grad"]).max() <= 1e-10
    for n, v in tables_after(inp, out).items():
        assert np.abs(v - fx[p + "f64_after." + n]).max() <= 1e-10, n


@pytest.mark.parametrize("name", CASES)
def test_restatement_f32_is_as_close_as_the_reference_f32(fx, name):
    """The float32 run of the restatement (the e_f32 of shapes outside the fixture) errs like the reference's own
    float32 run: within 4x of it, or under the 1e-6 floor."""
    inp = load_case(fx, name)
    p = name + "_"
    o64, o32 = restate(inp), restate(inp, np.float32)
    e_ref = np.abs(fx[p + "f32_losses"][:4] - fx[p + "f64_losses"][:4]) / np.abs(fx[p + "f64_losses"][:4]).clip(1e-30)
    e_own = np.abs(o32["losses"] - o64["losses"]) / np.abs(o64["losses"]).clip(1e-30)
    print(name, "relative f32 error: reference", e_ref, "restatement", e_own)
    assert np.all(e_own <= np.maximum(4 * e_ref, 1e-6))
    assert np.array_equal(o32["bins"], o64["bins"])                 # the margin keeps every bin


def test_make_ph_data_matches_reference(fx):
    from hubertfa_amd.labels import make_ph_data
    fl = float(fx["ph_frame_length"])
    keys = ("ph_id_seq", "ph_edge", "ph_frame", "ph_mask", "ph_time")
    nones = 0
    for name in fx["ph_names"]:
        p = f"ph_{name}_"
        args = ({"vocab_size": 20}, int(fx[p + "T"]), int(fx[p + "type"]), fx[p + "ids"].tolist(),
                fx[p + "durs"].tolist(), fl)
        if bool(fx[p + "raises"]):
            with pytest.raises(IndexError):
                make_ph_data(*args)
            continue
        got = make_ph_data(*args)
        if bool(fx[p + "none"]):
            assert got == (None,) * 5, name
            nones += 1
            continue
        for k, g in zip(keys, got):
            want = fx[p + k]
            assert g.dtype == want.dtype and g.shape == want.shape and np.array_equal(g, want), (name, k)
    assert nones >= 2


def test_read_transcriptions(tmp_path):
    from hubertfa_amd.labels import read_transcriptions
    (tmp_path / "transcriptions.csv").write_text("name,ph_seq,ph_dur\na,SP k a,0.1 0.05 0.2\nb,k a,\n")
    rows = read_transcriptions(str(tmp_path))
    assert rows == [{"name": "a", "ph_seq": ["SP", "k", "a"], "ph_dur": [0.1, 0.05, 0.2]},
                    {"name": "b", "ph_seq": ["k", "a"], "ph_dur": []}]
    (tmp_path / "bad.csv").write_text("name,ph_seq,ph_dur\na,k a,0.1\n")
    with pytest.raises(ValueError):
        read_transcriptions(str(tmp_path / "bad.csv"))


@pytest.mark.parametrize("name", CASES)
def test_faloss_table_update_matches_reference(fx, name):
    """FALoss._update (update_ema as torch ops, float32 tables as the reference's buffers) from the restatement's
    counts against the reference's float32 tables after one step; valid=True is the caller not updating."""
    torch = pytest.importorskip("torch")
    from hubertfa_amd.losses import CTC_TABLE, FALoss
    inp = load_case(fx, name)
    out = restate(inp)
    loss = FALoss(20, inp["num_bins"], inp["alpha"], inp["label_smoothing"], device="cpu")
    for n in loss.tables:
        loss.tables[n] = torch.tensor(inp["tables"][n])
    hist = torch.tensor(np.concatenate([out["hist"][n] for n in ref.TABLES]).astype(np.int32))
    weak = inp["label_type"] >= 1
    conf = None
    if weak.any():
        # the clipped per-frame confidences, from the restatement's nll
        nll = [ref.ctc_fb_ref.oracle(np.concatenate([inp["logits"][b, :inp["T"][b], 1:2],
                                                     inp["logits"][b, :inp["T"][b], 3:]], axis=1).astype(np.float64),
                                     inp["ph_id_seq"][b, :inp["L"][b]])["nll"] for b in np.nonzero(weak)[0]]
        conf = torch.tensor(np.clip(np.exp(-np.asarray(nll) / inp["T"][weak]), 1e-6, 1 - 1e-6))
    loss._update(hist, conf)
    p = name + "_"
    for n, t in loss.tables.items():
        want = fx[p + "f32_after." + n]
        assert np.abs(t.numpy().astype(np.float64) - want).max() <= 1e-6, n
    assert CTC_TABLE in loss.tables


def test_faloss_checkpoint_round_trip(tmp_path):
    torch = pytest.importorskip("torch")
    import ckpt_files
    from hubertfa_amd.losses import FALoss
    meta = json.load(open(os.path.join(HERE, "golden", "loaders.json")))
    path = str(tmp_path / "m.ckpt")
    ck = ckpt_files.write_lightning_ckpt(path, meta)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    cfg = ck["hyper_parameters"]["loss_config"]
    loss = FALoss.from_checkpoint(ck["state_dict"], cfg, device="cpu")
    assert loss.vocab_size == 63 and loss.num_bins == 10 and loss.alpha == 0.999 and loss.label_smoothing == 0.08
    assert loss.weights.tolist() == [8.0, 0.1, 0.01, 0.1, 2.0]
    assert all(bool((t == 1).all()) for t in loss.tables.values())
    assert sorted(loss.tables) == sorted(k for k in meta["loss_buffers"] if not k.startswith("pseudo_label"))
    tables = ref.make_tables(63, 10, 3)
    for n in loss.tables:
        loss.tables[n] = torch.tensor(tables[n])
    ck["state_dict"].update(loss.state_dict())
    torch.save(ck, path)
    again = FALoss.from_checkpoint(torch.load(path, map_location="cpu", weights_only=True)["state_dict"], cfg,
                                   device="cpu")
    for n in loss.tables:
        assert torch.equal(again.tables[n], loss.tables[n]), n
    total = again.total([torch.tensor(float(k + 1), dtype=torch.float64) for k in range(5)])
    assert abs(float(total) - (8.0 + 0.2 + 0.03 + 0.4 + 10.0)) < 1e-12
