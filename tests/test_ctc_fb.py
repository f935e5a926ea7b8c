"""Host side of the CTC forward-backward: the float64 oracle of tests/ctc_fb_ref.py against torch's
own float64 autograd, the float32 emulation of the kernels' scheme against the oracle, the argument envelope of
hfa_ctc_forward_alpha / hfa_ctc_backward / hfa_ctc_grad, ops.ctc_class_index, score_transcripts.py's phone CSV, and
the localisation fixture the GPU test reuses."""
import csv
import ctypes
import functools
import os

import numpy as np
import pytest

import ctc_fb_ref as ref

torch = pytest.importorskip("torch")
F = torch.nn.functional
P = ctypes.c_void_p

SHAPES = [(861, 63, 45, 1), (861, 63, 45, 6), (70, 5, 33, 2), (400, 63, 40, 30), (23, 63, 11, 2), (600, 63, 300, 4)]


@functools.lru_cache(maxsize=None)
def _case(T, V, L, scale):
    r = np.random.default_rng(1000 + T + L)
    x = (r.standard_normal((T, V)) * scale).astype(np.float32)
    tg = r.integers(1, V, L)
    tg[1] = tg[0]                                        # an adjacent repeat: the skip rule matters
    return x, tg, ref.oracle(x, tg)


@pytest.mark.parametrize("T,V,L,scale", SHAPES)
def test_oracle_matches_torch_float64_autograd(T, V, L, scale):
    """The gradient with respect to the LOGITS (log_softmax inside the graph): softmax - Gamma.  Measured: nll equal to
    every printed digit, the gradient within 2e-12 .. 5e-11, gamma's row sums within 2e-11 of 1; the asserts leave an
    order of magnitude for another BLAS or libm."""
    x, tg, want = _case(T, V, L, scale)
    xt = torch.from_numpy(x).double().requires_grad_(True)
    with torch.enable_grad():                            # (other tests' CLIs switch autograd off process-wide)
        lp = F.log_softmax(xt, dim=-1).unsqueeze(1)
        nll = F.ctc_loss(lp, torch.from_numpy(tg).view(1, -1), [T], [L], blank=0, reduction="sum", zero_infinity=False)
        nll.backward()
    nll = float(nll.detach())
    assert abs(want["nll"] - nll) <= 1e-11 * abs(nll)
    e = float(np.max(np.abs(want["grad"] - xt.grad.numpy())))
    rs = float(np.max(np.abs(want["occ"].sum(axis=1) - 1)))
    print(f"[oracle T={T} V={V} L={L} scale={scale}] grad err {e:.1e}  row sums {rs:.1e}")
    assert e <= 5e-10 and rs <= 2e-10
    assert np.all(want["frames"] >= 1 - 1e-9)            # every path emits every label at least once


@pytest.mark.parametrize("T,V,L,scale", SHAPES)
def test_emulation_nll_matches_oracle(T, V, L, scale):
    x, tg, want = _case(T, V, L, scale)
    emu = ref.emulate(x, tg)
    e = abs(emu["nll"] - want["nll"]) / want["nll"]
    eg = float(np.max(np.abs(emu["occ"] - want["occ"])))
    print(f"[emulation T={T} V={V} L={L} scale={scale}] nll rel {e:.1e}  occ abs {eg:.1e}")
    assert e <= 1e-6
    assert eg <= 1e-2                                    # (a sanity limit only: its measured value sets the device's bar)


def test_oracle_infeasible_and_empty():
    x = np.random.default_rng(3).standard_normal((4, 9))
    for o in (ref.oracle(x, [1, 1, 2, 2]), ref.emulate(x, [1, 1, 2, 2]), ref.oracle(x[:0], [3, 4])):
        assert o["nll"] == np.inf and not o["occ"].any() and not o["grad"].any() and not o["frames"].any()
        assert np.all(np.isneginf(o["logp"]))
    o = ref.oracle(x[:0], [])
    assert o["nll"] == 0.0 and o["occ"].shape == (0, 1)
    o = ref.oracle(x, [])                                # L = 0: all mass on the one blank state
    assert np.allclose(o["occ"], 1.0) and np.allclose(o["Gam"][:, 0], 1.0)


# ---- the C entries' envelope ---------------------------------------------------------------------------------------
def _lib():
    from hubertfa_amd import _lib, ops  # noqa: F401  (ops registers the signatures)
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libhfa.so not built (run __graft_entry__.build())")
    return _lib


def _alpha(M, **kw):
    a = dict(B=1, Tmax=8, Lmax=4, T=0x10000, L=0x20000, emis=0x30000, targets=0x40000, nll=0x50000, alpha=0x60000,
             aoff=0x70000)
    a.update(kw)
    return M.lib().hfa_ctc_forward_alpha(a["B"], a["Tmax"], a["Lmax"], P(a["T"]), P(a["L"]), P(a["emis"]),
                                         P(a["targets"]), P(a["nll"]), P(a["alpha"]), P(a["aoff"]), P(0))


def _backward(M, **kw):
    a = dict(B=1, Tmax=8, Lmax=4, T=0x10000, L=0x20000, emis=0x30000, targets=0x40000, nll=0x50000, alpha=0x60000,
             aoff=0x70000, occ=0x80000, frames=0x90000, centre=0xa0000, logp=0xb0000)
    a.update(kw)
    return M.lib().hfa_ctc_backward(a["B"], a["Tmax"], a["Lmax"], P(a["T"]), P(a["L"]), P(a["emis"]), P(a["targets"]),
                                    P(a["nll"]), P(a["alpha"]), P(a["aoff"]), P(a["occ"]), P(a["frames"]),
                                    P(a["centre"]), P(a["logp"]), P(0))


def _grad(M, **kw):
    a = dict(B=1, Tmax=8, V=63, Lmax=4, T=0x10000, L=0x20000, logits=0x30000, ld=65, bs=8 * 65, blank_col=1,
             label_off=2, occ=0x40000, nll=0x50000, cls_ptr=0x60000, cls_idx=0x70000, weight=0x80000, grad=0x90000,
             g_ld=65, g_bs=8 * 65)
    a.update(kw)
    return M.lib().hfa_ctc_grad(a["B"], a["Tmax"], a["V"], a["Lmax"], P(a["T"]), P(a["L"]), P(a["logits"]), a["ld"],
                                a["bs"], a["blank_col"], a["label_off"], P(a["occ"]), P(a["nll"]), P(a["cls_ptr"]),
                                P(a["cls_idx"]), P(a["weight"]), P(a["grad"]), a["g_ld"], a["g_bs"], P(0))


_A, _B, _G = "hfa_ctc_forward_alpha", "hfa_ctc_backward", "hfa_ctc_grad"
ENVELOPE = (
    [(_alpha, _A, d) for d in (dict(Lmax=8192), dict(Lmax=-1), dict(B=-1), dict(Tmax=-1), dict(emis=0), dict(nll=0),
                               dict(targets=0), dict(L=0), dict(T=0), dict(alpha=0), dict(aoff=0), dict(nll=0x50004),
                               dict(aoff=0x70004), dict(alpha=0x60002), dict(emis=0x30002))] +
    [(_backward, _B, d) for d in (dict(Lmax=8192), dict(Lmax=-1), dict(B=-1), dict(Tmax=-1), dict(emis=0),
                                  dict(nll=0), dict(targets=0), dict(L=0), dict(T=0), dict(alpha=0), dict(aoff=0),
                                  dict(occ=0), dict(frames=0), dict(centre=0), dict(logp=0), dict(nll=0x50004),
                                  dict(aoff=0x70004), dict(occ=0x80002), dict(logp=0xb0001))] +
    [(_grad, _G, d) for d in (dict(V=1025), dict(V=0), dict(Lmax=8192), dict(Lmax=-1), dict(B=-1), dict(Tmax=-1),
                              dict(blank_col=-1), dict(label_off=-2), dict(ld=-1), dict(g_ld=-1), dict(g_bs=-1),
                              dict(logits=0), dict(occ=0), dict(nll=0), dict(cls_ptr=0), dict(cls_idx=0),
                              dict(grad=0), dict(T=0), dict(L=0), dict(nll=0x50004), dict(weight=0x80002),
                              dict(grad=0x90001), dict(cls_ptr=0x60002))])


@pytest.mark.parametrize("call,name,bad", ENVELOPE, ids=[f"{n}-{k}={v}" for _, n, d in ENVELOPE for k, v in d.items()])
def test_ctc_fb_entries_reject_outside_envelope(call, name, bad):
    """Validation precedes any HIP call, so on a host without a GPU each entry answers HFA_EINVAL (never a HIP error)
    with its own name in hfa_last_error(); the pointers are never dereferenced."""
    L = _lib()
    rc = call(L, **bad)
    assert rc == L.HFA_EINVAL, L.lib().hfa_last_error()
    assert name.encode() in L.lib().hfa_last_error()


def test_ctc_fb_abi_is_additive():
    L = _lib()
    assert L.lib().hfa_abi_version() == 2
    assert _grad(L, weight=0, B=0) == 0 and _backward(L, B=0) == 0 and _alpha(L, B=0) == 0      # nothing to do


# ---- ops.ctc_class_index -------------------------------------------------------------------------------------------
def test_ctc_class_index():
    from hubertfa_amd import ops
    tg = [[3, 1, 3, 2, 3, -1], [2, 2, -1, -1, -1, -1], [-1] * 6, [4, 3, 2, 1, 4, 4]]
    T, L, out, cp, ci = ops.ctc_class_index([9, 3, 0, 7], tg, [5, 2, 0, 6], 5)
    assert cp.dtype == ci.dtype == np.int32 and cp.shape == (4, 6) and ci.shape == (4, 6)
    assert out.tolist()[0] == [3, 1, 3, 2, 3, 0] and out.tolist()[2] == [0] * 6          # padding is not looked at
    assert cp.tolist() == [[0, 0, 1, 2, 5, 5], [0, 0, 0, 2, 2, 2], [0] * 6, [0, 0, 1, 2, 3, 6]]
    assert ci[0, :5].tolist() == [1, 3, 0, 2, 4]         # class 1, class 2, then class 3's positions ascending
    assert ci[1, :2].tolist() == [0, 1] and ci[3].tolist() == [3, 2, 1, 0, 4, 5]
    for b in range(4):                                   # every class's slice holds exactly its positions
        for c in range(5):
            want = [j for j in range(int(L[b])) if out[b, j] == c]
            assert ci[b, cp[b, c]:cp[b, c + 1]].tolist() == want
    with pytest.raises(ValueError, match="outside 1..4"):
        ops.ctc_class_index([3], [[5]], [1], 5)
    T, L, out, cp, ci = ops.ctc_class_index([], [], [], 5)
    assert cp.shape == (0, 6) and ci.shape == (0, 0)


# ---- the phone CSV -------------------------------------------------------------------------------------------------
def test_phone_csv_writer(tmp_path):
    from score_transcripts import PHONE_COLUMNS, phone_rows, score_row, write_csv, write_phone_csv
    vocab = {"SP": 0, "AP": 0, "a": 1, "b": 2, "c": 3}
    res = [dict(T=10, ctc_nll=12.5, ctc_confidence=0.2865047968601901, ctc_phones=["a", "c"],
                ctc_phone_confidence=np.array([0.9, 0.1234567890123456, 1 / 3]),
                ctc_phone_centre_s=np.array([0.011609977324263039, 0.05, 0.1]), ctc_phone_frames=np.array([1.5, 2, 6.5])),
           dict(T=1, ctc_nll=float("inf"), ctc_confidence=1e-6, ctc_phones=[],                  # infeasible
                ctc_phone_confidence=np.exp(np.full(2, -np.inf)), ctc_phone_centre_s=np.zeros(2),
                ctc_phone_frames=np.zeros(2))]
    seqs = [["SP", "a", "b", "c", "SP"], ["SP", "a", "AP", "b"]]
    rows = write_csv(tmp_path / "ctc_scores.csv", [score_row(f"u{i}", r, s, vocab)
                                                   for i, (r, s) in enumerate(zip(res, seqs))])
    by_name = {f"u{i}": phone_rows(f"u{i}", r, s, vocab) for i, (r, s) in enumerate(zip(res, seqs))}
    write_phone_csv(tmp_path / "ctc_phone_scores.csv", [r["name"] for r in rows], by_name)
    back = list(csv.reader(open(tmp_path / "ctc_phone_scores.csv", newline="", encoding="utf-8")))
    assert tuple(back[0]) == PHONE_COLUMNS == ("name", "index", "phone", "centre_s", "frames", "confidence")
    assert [(r[0], r[1], r[2]) for r in back[1:]] == [("u1", "0", "a"), ("u1", "1", "b"), ("u0", "0", "a"),
                                                      ("u0", "1", "b"), ("u0", "2", "c")]      # the worst file first
    assert [float(r[5]) for r in back[1:3]] == [0.0, 0.0] and [float(r[4]) for r in back[1:3]] == [0.0, 0.0]
    got = back[3:]
    assert [float(r[5]) for r in got] == res[0]["ctc_phone_confidence"].tolist()                 # repr round-trips
    assert [float(r[3]) for r in got] == res[0]["ctc_phone_centre_s"].tolist()
    assert [float(r[4]) for r in got] == [1.5, 2.0, 6.5]


# ---- localisation --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 5, 11])
def test_localisation_on_the_oracle(k):
    """One wrong phone in a clean transcript: its confidence collapses, every other phone keeps its own, and the
    expected positions stay on the phones' frames."""
    x, tg = ref.localisation_fixture(k)
    o = ref.oracle(x, tg)
    conf = np.exp(o["logp"])
    others = np.delete(conf, k)
    print(f"[k={k}] confidence at k {conf[k]:.4f}, others {others.min():.4f} .. {others.max():.4f}")
    assert int(np.argmin(conf)) == k and abs(conf[k] - 0.006) < 5e-4
    assert others.min() > 0.875 and others.max() < 0.883
    right = ref.oracle(*ref.localisation_fixture(None))
    assert np.allclose(right["centre"], 8 * np.arange(12) + 2.5, atol=0.05)
    assert np.allclose(np.delete(o["centre"], k), np.delete(8 * np.arange(12) + 2.5, k), atol=0.5)
