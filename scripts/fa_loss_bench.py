"""Time the fused full-label alignment losses (csrc/loss.hip) against the same arithmetic as plain torch ops.

    python scripts/fa_loss_bench.py [--B 32 --T 861 --V 63 --iters 50]

HIP events after warm-up, the median of ``--iters`` runs, seeded logits, every row full-label and full length.  Reports
microseconds per kernel (hfa_fa_emd, hfa_fa_frame_loss without and with the gradient, hfa_fa_loss_reduce), the loss-only
and loss-plus-gradient totals through ops.fa_loss, GB/s of algorithmic bytes (the logits, targets and mask read once, the
terms and bins written once, the gradient written once), and the reference's _get_loss restated as torch ops on the same
device (forced_alignment.py:216-254 with GHMLoss.py:117-302 and BinaryEMDLoss.py:4-15, valid=False so the bincounts run;
autograd for the gradient).  Record: profiles/loss/fa_loss_bench.txt.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hubertfa_amd import ops  # noqa: E402


def timed(fn, iters, warm=10):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return float(np.median(ts))


def torch_get_loss(x, T, ph_frame, ph_edge, ph_mask, tab, nb, ls):
    """The four full-label terms as the reference's op chain (every row full-label), float32, with the bincounts."""
    B, Tmax, C = x.shape
    V = C - 2
    frame, edge = x[:, :, 2:], x[:, :, 0]
    tm = (torch.arange(Tmax, device=x.device)[None, :] < T[:, None]).float()

    def multilabel(logit, target, mask, gd_ema, lab_ema):
        raw = torch.nn.functional.binary_cross_entropy_with_logits(logit, target, reduction="none")
        p = torch.sigmoid(logit)
        gi = torch.floor((p - target).abs() * nb).long().clamp(0, nb - 1)
        li = torch.floor(target * 3).long().clamp(0, 2)
        w = torch.sqrt((1 / gd_ema[gi] + 1e-3) * (1 / lab_ema[li] + 1e-3))
        loss = torch.sum(raw * w * mask) / torch.sum(mask)
        torch.bincount(gi.flatten(), weights=mask.flatten(), minlength=nb)
        torch.bincount(li.flatten(), weights=mask.flatten(), minlength=3)
        return loss

    dgt = (ph_edge[:, 1:] - ph_edge[:, :-1] + 1) / 2
    dpr = (torch.sigmoid(edge[:, 1:]) - torch.sigmoid(edge[:, :-1]) + 1) / 2
    l_diff = multilabel(dpr, dgt, (tm[:, 1:] > 0).float(), tab["dgd"], tab["dlab"])
    mask = ph_mask[:, None, :].float() * tm[:, :, None]
    time_mask = mask.any(dim=-1)
    xl = frame - 1e9 * mask.logical_not().float()
    tp = torch.nn.functional.one_hot(ph_frame.long(), num_classes=V).float().clamp(ls, 1 - ls) * mask
    raw = torch.nn.functional.cross_entropy(xl.transpose(1, 2), tp.transpose(1, 2), reduction="none")
    pp = torch.softmax(xl, dim=-1).detach()
    gd = torch.gather((pp - tp).abs(), -1, ph_frame.long().unsqueeze(-1)).squeeze(-1)
    gi = torch.floor(gd * nb).long().clamp(0, nb - 1)
    w = torch.sqrt(tab["class"][ph_frame.long()] * tab["gd"][gi])
    l_frame = torch.sum(raw / w * time_mask.float()) / torch.sum(time_mask.float())
    torch.bincount(ph_frame.long().flatten(), weights=time_mask.flatten().float(), minlength=V)
    torch.bincount(gi.flatten(), weights=time_mask.flatten().float(), minlength=nb)
    l_edge = multilabel(edge, ph_edge, tm, tab["egd"], tab["elab"])
    a, b = torch.sigmoid(edge) * tm, ph_edge * tm
    l1 = torch.nn.functional.l1_loss
    l_emd = (l1(a.cumsum(-1), b.cumsum(-1)) + l1(a.flip([-1]).cumsum(-1), b.flip([-1]).cumsum(-1))) / 2
    return torch.stack([l_frame, l_edge, l_emd, l_diff])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--T", type=int, default=861)
    ap.add_argument("--V", type=int, default=63)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    B, Tm, V, nb, ls = a.B, a.T, a.V, 10, 0.08
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(B, Tm, V + 2, generator=g) * 2).cuda()
    T = torch.full((B,), Tm, dtype=torch.int32).cuda()
    lt = torch.full((B,), 2, dtype=torch.int32).cuda()
    pf = torch.randint(0, V, (B, Tm), generator=g, dtype=torch.int32).cuda()
    pe = (torch.rand(B, Tm, generator=g) * 0.96 + 0.02).cuda()
    pm = torch.ones(B, V, dtype=torch.int32).cuda()
    packed = (torch.rand(V + 3 * nb + 6, generator=g) + 0.5).cuda()
    sl = list(ops.fa_table_slices(V, nb).values())
    tab = {k: packed[s] for k, s in zip(("class", "gd", "egd", "elab", "dgd", "dlab"), sl)}
    coef = torch.full((4,), 1e-4).cuda()

    sums, fac = ops.fa_emd(x, T, lt, pe)
    terms, bins = ops.fa_frame_loss(x, T, lt, pf, pe, pm, packed, nb, ls)
    grad = torch.zeros_like(x)
    k = {
        "hfa_fa_emd": lambda: ops.fa_emd(x, T, lt, pe),
        "hfa_fa_frame_loss": lambda: ops.fa_frame_loss(x, T, lt, pf, pe, pm, packed, nb, ls, terms=terms, bins=bins),
        "hfa_fa_frame_loss+grad": lambda: ops.fa_frame_loss(x, T, lt, pf, pe, pm, packed, nb, ls, coef=coef,
                                                            emd_fac=fac, grad=grad, terms=terms, bins=bins),
        "hfa_fa_loss_reduce": lambda: ops.fa_loss_reduce(T, lt, terms, bins, pf, sums, V, nb),
    }
    us = {n: timed(f, a.iters) for n, f in k.items()}
    xg = x.clone().requires_grad_(True)
    up = torch.ones(4, dtype=torch.float64).cuda()

    def fused(backward):
        losses = ops.fa_loss(xg if backward else x, T, lt, pf, pe, pm, packed, nb, ls, check=False)
        if backward:
            xg.grad = None
            (losses * up).sum().backward()

    def chain(backward):
        losses = torch_get_loss(xg if backward else x, T, pf, pe, pm, tab, nb, ls)
        if backward:
            xg.grad = None
            losses.sum().backward()

    with torch.no_grad():
        f_loss, t_loss = timed(lambda: fused(False), a.iters), timed(lambda: chain(False), a.iters)
    f_both, t_both = timed(lambda: fused(True), a.iters), timed(lambda: chain(True), a.iters)
    with torch.no_grad():
        got = ops.fa_loss(x, T, lt, pf, pe, pm, packed, nb, ls).cpu().numpy()
        want = torch_get_loss(x, T, pf, pe, pm, tab, nb, ls).double().cpu().numpy()
    rd = B * Tm * ((V + 2) * 4 + 8) + B * V * 4
    wr = B * Tm * (12 + 20)
    gw = B * Tm * (V + 1) * 4
    print(f"fa_loss_bench B={B} T={Tm} V={V} (+2 columns), median of {a.iters}, {torch.cuda.get_device_name(0)}")
    for n, v in us.items():
        print(f"  {n:26s} {v:8.1f} us")
    kl = us["hfa_fa_emd"] + us["hfa_fa_frame_loss"] + us["hfa_fa_loss_reduce"]
    kg = kl + us["hfa_fa_frame_loss+grad"]
    print(f"  kernels, loss only         {kl:8.1f} us   {(rd + wr) / kl / 1e3:7.1f} GB/s algorithmic")
    print(f"  kernels, loss + gradient   {kg:8.1f} us   {(2 * rd + 2 * wr + gw) / kg / 1e3:7.1f} GB/s algorithmic")
    print(f"  ops.fa_loss, loss only     {f_loss:8.1f} us   torch op chain {t_loss:8.1f} us   x{t_loss / f_loss:.1f}")
    print(f"  ops.fa_loss, loss + grad   {f_both:8.1f} us   torch op chain {t_both:8.1f} us   x{t_both / f_both:.1f}")
    print(f"  losses fused {got}  torch f32 {want}  max rel diff {np.max(np.abs(got - want) / np.abs(want)):.2e}")


if __name__ == "__main__":
    main()
