"""Head fine-tuning without a GPU: the schedules of hubertfa_amd/schedulers.py against torch's own, the invalid-argument
paths of hfa_wgrad_f32 / hfa_adamw_f32 (nothing launches), and the float64 yardstick of test_train_gpu.py,
tests/train_ref.py, against torch.optim.AdamW + clip_grad_norm_ + OneCycleLR on a float64 nn.Linear."""
import ctypes
import math
import os

import numpy as np
import pytest

import fa_loss_ref as ref
import train_ref

torch = pytest.importorskip("torch")


@pytest.fixture(autouse=True)
def _autograd_on():
    with torch.enable_grad():                            # (other tests' CLIs switch autograd off process-wide)
        yield


@pytest.mark.parametrize("total", (10, 100, 1000))
def test_one_cycle_equals_torch(total):
    from hubertfa_amd.schedulers import one_cycle
    max_lr = 3e-3
    p = torch.nn.Parameter(torch.zeros(3))
    opt = torch.optim.AdamW([p], lr=1e-3)
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=max_lr, total_steps=total)
    worst = 0.0
    for k in range(total):
        lr, beta1 = one_cycle(k, total, max_lr)
        g = opt.param_groups[0]
        worst = max(worst, abs(lr - g["lr"]) / g["lr"], abs(beta1 - g["betas"][0]) / g["betas"][0])
        p.grad = torch.ones(3)
        opt.step()
        if k + 1 < total:
            sched.step()
    print(f"one_cycle total_steps {total}: worst relative difference {worst:.3g}")
    assert worst <= 1e-14
    with pytest.raises(ValueError):
        one_cycle(total, total, max_lr)


def test_gaussian_ramp_up():
    from hubertfa_amd.schedulers import GaussianRampUp, NoneScheduler
    s = GaussianRampUp(100, start_steps=10, end_steps=60)
    seen = []
    for k in range(80):
        seen.append(s())
        s.step()
    assert all(v == 0 for v in seen[:10])
    for k in range(10, 60):
        assert seen[k] == pytest.approx(math.exp(-5 * (1 - (k - 10) / 50) ** 2), rel=1e-15)
    assert all(v == 1 for v in seen[60:])
    s.resume(35)
    assert s() == pytest.approx(math.exp(-5 * 0.25), rel=1e-15)
    d = GaussianRampUp(8)                                 # the defaults the reference uses: 0 .. max_steps
    assert d() == pytest.approx(math.exp(-5.0)) and d.start_steps == 0 and d.end_steps == 8
    n = NoneScheduler()
    n.step()
    n.resume(5)
    assert n() == 1


def test_kernels_refuse_bad_arguments():
    from hubertfa_amd import _lib, ops  # noqa: F401  (ops registers the signatures)
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libhfa.so not built")
    L = _lib.lib()
    E = _lib.HFA_EINVAL
    buf = (ctypes.c_double * 64)()                        # host memory: never dereferenced, nothing launches
    P = ctypes.c_void_p(ctypes.addressof(buf))
    NULL = ctypes.c_void_p(0)

    def wgrad(B=2, T=5, N=3, C=8, G=P, ldg=3, X=P, ldx=8, lens=P, dW=P, ldw=8, db=P, ss=P, ws=P):
        return L.hfa_wgrad_f32(B, T, N, C, G, ldg, 15, X, ldx, 40, lens, dW, ldw, db, ss, ws, NULL)
    for kw in (dict(G=NULL), dict(X=NULL), dict(lens=NULL), dict(dW=NULL), dict(db=NULL), dict(ss=NULL), dict(ws=NULL),
               dict(C=12, ldx=12, ldw=12), dict(C=0), dict(N=0), dict(N=-1), dict(ldg=2), dict(ldx=7), dict(ldw=7),
               dict(B=-1), dict(T=-1), dict(G=ctypes.c_void_p(P.value + 2)), dict(ss=ctypes.c_void_p(P.value + 4))):
        assert wgrad(**kw) == E, kw
        assert L.hfa_last_error()
    assert L.hfa_wgrad_workspace_bytes(2, 5, 0, 8) == E and L.hfa_wgrad_workspace_bytes(2, 5, 3, 12) == E
    rows = L.hfa_wgrad_chunk_rows()
    assert rows > 0 and rows % 16 == 0
    n_out = 65 * 192 + 65
    assert L.hfa_wgrad_workspace_bytes(32, 861, 65, 192) == \
        8 * -(-n_out // 256) + 32 * -(-861 // rows) * (8 * 65 + 4 * 65 * 192)

    def adamw(n=4, p=P, m=P, v=P, g=P, ss=P, sk=P, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.1, bc1=0.1, bc2=1e-3):
        return L.hfa_adamw_f32(n, p, m, v, g, ss, 0.5, lr, b1, b2, eps, wd, bc1, bc2, sk, NULL)
    for kw in (dict(n=-1), dict(p=NULL), dict(m=NULL), dict(v=NULL), dict(g=NULL), dict(ss=NULL), dict(sk=NULL),
               dict(b1=1.0), dict(b2=-0.1), dict(bc1=0.0), dict(lr=float("nan")),
               dict(p=ctypes.c_void_p(P.value + 1))):
        assert adamw(**kw) == E, kw
    assert adamw(n=0) == 0                                # nothing to do: no launch


def test_ops_refuse_cpu_tensors():
    from hubertfa_amd import _lib, ops
    G, X = torch.zeros(1, 4, 3), torch.zeros(1, 4, 8)
    with pytest.raises(_lib.HFALibraryError):
        ops.wgrad(G, X, torch.ones(1, dtype=torch.int32))
    z = torch.zeros(4)
    with pytest.raises(_lib.HFALibraryError):
        ops.adamw_step(z, z, z, z, torch.zeros((), dtype=torch.float64), torch.zeros(1, dtype=torch.int32), lr=1e-3,
                       step=1)
    with pytest.raises(_lib.HFALibraryError):
        ops.head_linear(X, None, torch.zeros(4, 8), None, torch.zeros(4), torch.ones(1, dtype=torch.int32))


# ---- the float64 yardstick ---------------------------------------------------------------------------------------------
C, V, TOTAL, MAX_LR, WD = 8, 6, 10, 2e-2, 0.1
WEIGHTS, RAMP = (8.0, 0.1, 0.01, 0.1, 2.0), (False, False, False, True, True)


def _trainer(max_norm, dtype=np.float64, seed=5, ramp=RAMP):
    from hubertfa_amd.schedulers import one_cycle
    rows = train_ref.draw_rows(seed, (14, 19, 11), (2, 1, 2), C, V)
    r = np.random.default_rng(seed + 1)
    W, b = r.uniform(-0.35, 0.35, (V + 2, C)), r.uniform(-0.35, 0.35, V + 2)
    return train_ref.RefTrainer(rows, W, b, ref.make_tables(V, 10, seed), WEIGHTS, ramp, TOTAL,
                                lambda k: one_cycle(k, TOTAL, MAX_LR), WD, max_norm, 10, 0.999, 0.08, dtype)


@pytest.mark.parametrize("max_norm", (0.0, 0.05, 1e3))
def test_restatement_step_equals_torch(max_norm):
    """Two steps of RefTrainer against a float64 nn.Linear under clip_grad_norm_, AdamW and OneCycleLR; the gradient of
    the total with respect to the logits (the restatement's, held to the reference by test_fa_loss.py) enters both."""
    tr = _trainer(max_norm)
    lin = torch.nn.Linear(C, V + 2).double()
    with torch.no_grad():
        lin.weight.copy_(torch.from_numpy(tr.W))
        lin.bias.copy_(torch.from_numpy(tr.b))
    opt = torch.optim.AdamW(lin.parameters(), lr=1e-3, weight_decay=WD)
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=MAX_LR, total_steps=TOTAL)
    idx = ((0, 1, 2), (2, 0))
    for k in range(2):
        _, _, G, fw = tr.gradients(idx[k])
        y = torch.from_numpy(fw[0]["y"]).double()
        opt.zero_grad()
        lin(y).backward(torch.from_numpy(G))
        if max_norm > 0:
            torch.nn.utils.clip_grad_norm_(lin.parameters(), max_norm)
        opt.step()
        sched.step()
        tr.step(idx[k])
        st = opt.state[lin.weight]
        err = max(np.abs(tr.W - lin.weight.detach().numpy()).max(), np.abs(tr.b - lin.bias.detach().numpy()).max(),
                  np.abs(tr.mW - st["exp_avg"].numpy()).max(), np.abs(tr.vW - st["exp_avg_sq"].numpy()).max())
        print(f"restatement step {k} (max_norm {max_norm}): clipped {tr.clipped[-1]}, norm {tr.norms[-1]:.4g}, "
              f"|difference| {err:.3g}")
        assert err <= 1e-12
    if max_norm == 0.05:
        assert all(tr.clipped)
    else:
        assert not any(tr.clipped)


def test_restatement_learns_and_f32_run_stays_close():
    """(ramps off: a loss weight that grows with the step would hide the descent in the total)"""
    off = (False,) * 5
    tr, tr32 = _trainer(0.5, ramp=off), _trainer(0.5, np.float32, ramp=off)
    first = tr.evaluate((0, 1, 2))[1]
    for k in range(5):
        l64, t64 = tr.step((0, 1, 2))
        l32, t32 = tr32.step((0, 1, 2))
        assert np.all(np.isfinite(l64)) and abs(t32 - t64) <= 1e-4 * abs(t64)
    assert min(tr.margins) > 0
    last = tr.evaluate((0, 1, 2))[1]
    print(f"restatement: evaluate total {first:.6g} -> {last:.6g}; float32 |dW| {np.abs(tr32.W - tr.W).max():.3g}")
    assert last < first
    assert tr32.W.dtype == np.float32 and np.abs(tr32.W - tr.W).max() <= 1e-4
    assert tr.ramp_weight(True) == pytest.approx(math.exp(-5 * (1 - 5 / TOTAL) ** 2)) and tr.ramp_weight(False) == 1
