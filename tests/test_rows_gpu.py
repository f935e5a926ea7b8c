"""The row kernels every alignment runs through -- LayerNorm (norm.hip), f32 and split attention with per-row lengths
(attention.hip), the small kernels of misc.hip and the lattice prologue (viterbi.hip) -- on their secondary paths
(residual, row strides, in place, t_len / key_len, every LayerNorm instantiation, ragged batches) against the plain
float64 restatements of tests/rows_ref.py.  Padding is poisoned with NaN where the kernel is written never to read it,
outputs are pre-filled with NaN or a canary, and "the same bits as the row alone" is asserted next to the float64
comparison, never instead of it.

The tests marked gpu need the device; the un-marked ones check the restatements and the LayerNorm statistics bound on
the CPU (torch's own float32 LayerNorm meets the bound, a one-pass variance misses it by orders of magnitude).
"""
import contextlib
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import rows_ref as ref  # noqa: E402

F = torch.nn.functional
gpu = pytest.mark.gpu
NAN = float("nan")


def _dev():
    return torch.device("cuda")


def _lens(values):
    return torch.tensor([int(v) for v in values], dtype=torch.int32, device=_dev())


def _decode(planes):
    return planes[0].float() + planes[1].float() / 2048.0


# ---- 1. LayerNorm ------------------------------------------------------------------------------------------------
LN_TOL = (1e-5, 2e-5)                      # tests/test_kernels_gpu.py::test_layernorm


def _ln_params(C, seed=10):
    return ref.randn(C, seed=seed) * 0.1 + 1, ref.randn(C, seed=seed + 1) * 0.1


@gpu
@pytest.mark.parametrize("C", [4, 252, 256, 260, 516, 1028, 2048, 2052, 4096])
def test_layernorm_every_instantiation_vs_f64(C):
    """VPL 1, 1, 1, 2, 3, 8, 8, 16, 16 (the c < C guard hit in the last slot), rows fewer than one workgroup's four
    waves and not a multiple of four, every activation, through hfa_layernorm_f32 and hfa_layernorm_split."""
    from hubertfa_amd import ops
    d = _dev()
    g, b = _ln_params(C)
    for rows in (1, 7):
        x = ref.randn(rows, C, seed=9 + rows, scale=3.0) + 0.5
        for act in (ops.ACT_NONE, ops.ACT_GELU, ops.ACT_HARDSWISH):
            want = ref.layernorm(x, g, b, 1e-5, act)
            got = ops.layernorm(x.to(d), g.to(d), b.to(d), 1e-5, act=act)
            ref.close(got, want, *LN_TOL)
            y, ys = ops.layernorm(x.to(d), g.to(d), b.to(d), 1e-5, act=act, out_split=True)
            ref.close(y, want, *LN_TOL)
            assert torch.equal(y, got), (rows, act)
            assert torch.equal(ys.cpu(), ref.split_planes(y.cpu())), (rows, act)


@gpu
@pytest.mark.parametrize("C", [192, 768, 2052])
@pytest.mark.parametrize("out_split", [False, True])
def test_layernorm_residual_and_row_pitches_vs_f64(C, out_split):
    """x, residual and out as column-slice views of wider buffers with three different row pitches; the statistics
    are those of x + residual; the slack columns of out keep their canary.  With out_split the planes are those of
    the f32 output bit for bit (hi = f16(y), lo = f16((y - hi) 2^11), so hi + lo / 2048 is y to 22 bits), and that
    f32 output meets the float64 tolerance too.  In place (out = x) gives the out-of-place bits."""
    from hubertfa_amd import ops
    d = _dev()
    rows = 7
    g, b = _ln_params(C, seed=30)
    xb = (ref.randn(rows, C + 4, seed=31, scale=3.0) + 0.5).to(d)
    rb = (ref.randn(rows, C + 8, seed=32, scale=2.0) - 1.0).to(d)
    ob = torch.full((rows, C + 12), 7.0, device=d)
    x, r, o = xb[:, 4:], rb[:, 4:C + 4], ob[:, 4:C + 4]
    assert x.stride(0) == C + 4 and r.stride(0) == C + 8 and o.stride(0) == C + 12
    for act in (ops.ACT_NONE, ops.ACT_GELU, ops.ACT_HARDSWISH):
        want = ref.layernorm(x.cpu(), g, b, 1e-5, act, residual=r.cpu())
        ob.fill_(7.0)
        res = ops.layernorm(x, g.to(d), b.to(d), 1e-5, act=act, out=o, residual=r, out_split=out_split or None)
        y = res[0] if out_split else res
        assert y.data_ptr() == o.data_ptr()
        ref.close(o, want, *LN_TOL)
        assert bool((ob[:, :4] == 7.0).all()) and bool((ob[:, C + 4:] == 7.0).all()), "wrote outside the row"
        if out_split:
            planes = res[1].cpu()
            assert torch.equal(planes, ref.split_planes(o.cpu())), act
            dec = _decode(planes).double()
            assert bool(((dec - o.cpu().double()).abs() <= 2.0 ** -22 * o.cpu().double().abs() + 2.0 ** -36).all())
        # in place, as hubert.py and unet.py call it
        x2 = x.clone()                       # contiguous copy: out = x
        ops.layernorm(x2, g.to(d), b.to(d), 1e-5, act=act, out=x2, residual=r)
        assert torch.equal(x2, o), act
        xw = xb.clone()
        xv = xw[:, 4:]                       # and in place on the pitched view
        ops.layernorm(xv, g.to(d), b.to(d), 1e-5, act=act, out=xv, residual=r)
        assert torch.equal(xv, o) and torch.equal(xw[:, :4], xb[:, :4]), act


@gpu
def test_layernorm_t_len_vs_f64():
    """Per-row lengths: rows t >= len of x and of the residual are NaN and never read; valid rows meet the float64
    tolerance; padding rows are exactly 0 in f32 and in both planes (all pre-filled with NaN); no range flag."""
    from hubertfa_amd import ops
    d = _dev()
    B, T, C = 5, 9, 260
    lens = [9, 0, 1, 8, 4]
    g, b = _ln_params(C, seed=40)
    x = ref.randn(B, T, C, seed=41, scale=3.0) + 0.5
    r = ref.randn(B, T, C, seed=42)
    want = ref.layernorm(x, g, b, 1e-5, 1, residual=r)
    xp, rp = x.clone(), r.clone()
    for i, n in enumerate(lens):
        xp[i, n:] = NAN
        rp[i, n:] = NAN
    for split in (False, True):
        out = torch.full((B, T, C), NAN, device=d)
        planes = torch.full((2, B, T, C), NAN, dtype=torch.float16, device=d) if split else None
        flag = torch.zeros(1, dtype=torch.int32, device=d)
        ops.layernorm(xp.to(d), g.to(d), b.to(d), 1e-5, act=1, out=out, residual=rp.to(d), t_len=_lens(lens),
                      out_split=planes, flag=flag)
        for i, n in enumerate(lens):
            ref.close(out[i, :n], want[i, :n], *LN_TOL)
            assert bool((out[i, n:] == 0).all()), i
            if split:
                assert bool((planes[:, i, n:] == 0).all()), i
                assert torch.equal(planes[:, i, :n].cpu(), ref.split_planes(out[i, :n].cpu())), i
        assert int(flag.item()) == 0


STAT_C = [4, 260, 768, 2052, 4096]


@functools.lru_cache(maxsize=None)
def _stat_case(C):
    x = 1000.0 + ref.randn(64, C, seed=50 + C)
    g, b = _ln_params(C, seed=60)
    want = ref.layernorm(x, g, b, 1e-5)
    return x, g, b, want, ref.layernorm_stat_bound(x, g, want)


@pytest.mark.parametrize("C", STAT_C)
def test_layernorm_statistics_bound_is_reachable_in_f32(C):
    """The bound of test_layernorm_large_mean_statistics, without the kernel: torch's float32 CPU layer_norm meets it
    on the same input, and a one-pass E[x^2] - mean^2 variance in float32 misses it by orders of magnitude."""
    x, g, b, want, bound = _stat_case(C)
    err = (F.layer_norm(x, (C,), g, b, 1e-5).double() - want).abs()
    ratio = float((err / bound).max())
    print(f"C={C}: torch f32 layer_norm worst err/bound {ratio:.3f}")
    assert ratio <= 1.0
    mean = x.mean(-1, keepdim=True)
    var1 = ((x * x).mean(-1, keepdim=True) - mean * mean).clamp_min(0)
    one_pass = (x - mean) / torch.sqrt(var1 + 1e-5) * g + b
    assert float(((one_pass.double() - want).abs() / bound).max()) > 30.0


@gpu
@pytest.mark.parametrize("C", STAT_C)
def test_layernorm_large_mean_statistics(C):
    """x = 1000 + N(0, 1): per element within 2e-5 + 1e-5 |ref| + 4 * 2^-24 * max_c |x| * rstd * |gamma_c| (the last
    term: the rounding of a float32 mean of values of that size, carried through the normalisation)."""
    from hubertfa_amd import ops
    d = _dev()
    x, g, b, want, bound = _stat_case(C)
    got = ops.layernorm(x.to(d), g.to(d), b.to(d), 1e-5)
    err = (got.cpu().double() - want).abs()
    ratio = float((err / bound).max())
    print(f"C={C}: kernel worst err/bound {ratio:.3f}")
    assert bool((err <= bound).all()), f"worst err/bound {ratio:.3f}, max err {float(err.max()):.3e}"


# ---- 2. attention with per-row lengths -------------------------------------------------------------------------------
ATTN_TOL = (1e-4, 2e-5)                    # tests/test_kernels_gpu.py::test_attention


def _attn_f32(q, k, v, B, H, L, D, key_len=None):
    """ops.attention on three contiguous [B, L, H * D] device tensors; the output pre-filled with NaN."""
    from hubertfa_amd import ops
    out = torch.full((B, L, H * D), NAN, device=q.device)
    ld = H * D
    ops.attention(q, k, v, out, B=B, H=H, L=L, head_dim=D, scale=D ** -0.5, q_bs=L * ld, q_ld=ld, k_bs=L * ld,
                  k_ld=ld, v_bs=L * ld, v_ld=ld, o_bs=L * ld, o_ld=ld, key_len=key_len)
    return out


@gpu
def test_attention_f32_key_len_vs_f64():
    """attn_fwd_f32_kernel (32-key tiles, 128 queries per workgroup) with lengths on and around the tile and workgroup
    edges.  Rows >= len of Q, K and V are NaN: the kernel never reads them, so NaN in an output means the masking
    multiplies where it should select.  Valid rows meet the float64 tolerance, rows in [len, L) are exactly 0 (whole
    workgroups of padding and partly active ones), and each row equals the same row run alone, bit for bit."""
    B, H, D, L = 10, 2, 64, 200
    lens = [0, 1, 31, 32, 33, 64, 127, 128, 129, 200]
    d = _dev()
    q, k, v = (ref.randn(B, L, H * D, seed=70 + i, scale=1.5) for i in range(3))
    want = ref.attention(q, k, v, H, D, lens)
    qp, kp, vp = q.clone(), k.clone(), v.clone()
    for b, n in enumerate(lens):
        for t in (qp, kp, vp):
            t[b, n:] = NAN
    qd, kd, vd = qp.to(d), kp.to(d), vp.to(d)
    out = _attn_f32(qd, kd, vd, B, H, L, D, key_len=_lens(lens))
    assert not bool(torch.isnan(out).any()), "NaN from padding rows reached an output (or a row was not written)"
    for b, n in enumerate(lens):
        ref.close(out[b, :n], want[b, :n], *ATTN_TOL)
        assert bool((out[b, n:] == 0).all()), b
        if n:
            alone = _attn_f32(qd[b:b + 1, :n].contiguous(), kd[b:b + 1, :n].contiguous(),
                              vd[b:b + 1, :n].contiguous(), 1, H, n, D)
            assert torch.equal(alone[0], out[b, :n]), b


def _pitched(vals, ld, bs_pad, fill):
    """vals [B, L, W] in a flat buffer with row pitch ld and batch stride L * ld + bs_pad, every other element fill.
    Returns (flat buffer, the strided view, batch stride)."""
    B, L, W = vals.shape
    bs = L * ld + bs_pad
    flat = torch.full((B * bs,), fill, dtype=vals.dtype, device=vals.device)
    view = flat.as_strided((B, L, W), (bs, ld, 1))
    view.copy_(vals)
    return flat, view, bs


@gpu
@pytest.mark.parametrize("lens", [None, [70, 33]])
def test_attention_f32_distinct_strides_vs_f64(lens):
    """q, k, v and o in four separate buffers with four different row pitches and batch strides (a swapped k_ld / v_ld
    or k_bs / v_bs cannot hide); everything between the rows is NaN on the inputs and must stay untouched on o."""
    from hubertfa_amd import ops
    B, H, D, L = 2, 2, 64, 70
    W = H * D
    d = _dev()
    q, k, v = (ref.randn(B, L, W, seed=80 + i, scale=1.5) for i in range(3))
    want = ref.attention(q, k, v, H, D, lens)
    qp, kp, vp = q.clone(), k.clone(), v.clone()
    for b, n in enumerate(lens or []):
        for t in (qp, kp, vp):
            t[b, n:] = NAN
    (_, qv, q_bs), (_, kv, k_bs), (_, vv, v_bs) = (_pitched(t.to(d), W + 4 * i, 16 * (i + 1), NAN)
                                                    for i, t in enumerate((qp, kp, vp)))
    oflat, ov, o_bs = _pitched(torch.full((B, L, W), NAN, device=d), W + 12, 64, 7.0)
    owned = torch.zeros_like(oflat, dtype=torch.bool)
    owned.as_strided((B, L, W), (o_bs, W + 12, 1)).fill_(True)
    ops.attention(qv, kv, vv, ov, B=B, H=H, L=L, head_dim=D, scale=D ** -0.5, q_bs=q_bs, q_ld=W, k_bs=k_bs,
                  k_ld=W + 4, v_bs=v_bs, v_ld=W + 8, o_bs=o_bs, o_ld=W + 12,
                  key_len=None if lens is None else _lens(lens))
    assert bool((oflat[~owned] == 7.0).all()), "wrote between the rows of o"
    assert not bool(torch.isnan(ov).any())
    for b in range(B):
        n = L if lens is None else lens[b]
        ref.close(ov[b, :n], want[b, :n], *ATTN_TOL)
        assert bool((ov[b, n:] == 0).all()), b


@contextlib.contextmanager
def _attn_form(form):
    from hubertfa_amd import _lib
    _lib.call("hfa_attention_split_form", form)
    try:
        yield
    finally:
        _lib.call("hfa_attention_split_form", 0)


@gpu
@pytest.mark.parametrize("form", [16, 32])
def test_attention_split_key_len_tile_edges_vs_f64(form):
    """Split attention (64-key tiles) with lengths 0, 1 and on both sides of one and two tiles, both MFMA forms.  The
    padding rows of the input planes hold finite garbage (1e3); valid rows meet the float64 tolerance, padding rows of
    the output are 0 in both planes, and every row has the bits of the run with zeros in the padding."""
    from hubertfa_amd import ops
    B, H, D, L = 7, 2, 64, 300
    lens = [0, 1, 63, 64, 65, 128, 300]
    d = _dev()
    qkv = ref.randn(B, L, 3 * H * D, seed=90, scale=2.0)
    want = ref.attention(*qkv.split(H * D, dim=-1), H, D, lens)
    outs = []
    for garbage in (1e3, 0.0):
        x = qkv.clone()
        for b, n in enumerate(lens):
            x[b, n:] = garbage
        out = torch.full((2, B, L, H * D), NAN, dtype=torch.float16, device=d)
        with _attn_form(form):
            ops.attention_split(ops.split(x.to(d)), out, B=B, H=H, L=L, head_dim=D, scale=D ** -0.5,
                                key_len=_lens(lens))
        outs.append(out)
    got = _decode(outs[0])
    for b, n in enumerate(lens):
        ref.close(got[b, :n], want[b, :n], *ATTN_TOL)
        assert bool((outs[0][:, b, n:] == 0).all()), b
    assert torch.equal(outs[0], outs[1])


# ---- 3. the small row kernels of misc.hip ------------------------------------------------------------------------------
@gpu
def test_mask_rows_equals_numpy_where():
    from hubertfa_amd import ops
    d = _dev()
    B, T, C, ld = 3, 50, 192, 200
    lens = [0, 1, T]
    buf = ref.randn(B, T, ld, seed=100) + 3.0                     # (no zeros in the data)
    bd = buf.to(d)
    ops.mask_rows(bd[:, :, :C], _lens(lens))
    want = buf.numpy().copy()
    want[:, :, :C] = ref.mask_rows(want[:, :, :C], lens)
    assert np.array_equal(bd.cpu().numpy(), want)                  # rows zeroed, slack columns untouched
    N, pitch = 1000, 1003
    buf2 = ref.randn(B, pitch, seed=101) + 3.0
    b2 = buf2.to(d)
    lens2 = [0, 1, N]
    ops.mask_rows(b2[:, :N], _lens(lens2))
    want2 = buf2.numpy().copy()
    want2[:, :N] = ref.mask_rows(want2[:, :N], lens2)
    assert np.array_equal(b2.cpu().numpy(), want2)


@gpu
@pytest.mark.parametrize("N,left,N_out", [(100, 0, 100), (100, 40, 180), (100, 40, 120), (5, 7, 300000)])
def test_pad_rows_equals_numpy(N, left, N_out):
    """Plain copy, padding on both sides, a truncating pad, and a row longer than the capped 1024-block grid covers in
    one sweep (its stride loop); row-strided x and out, canaries past N_out."""
    from hubertfa_amd import ops
    d = _dev()
    B = 2
    xb = ref.randn(B, N + 3, seed=110) + 3.0
    ob = torch.full((B, N_out + 5), 7.0, device=d)
    ops.pad_rows(xb.to(d)[:, :N], left, N_out, out=ob[:, :N_out])
    got = ob.cpu().numpy()
    assert np.array_equal(got[:, :N_out], ref.pad_rows(xb.numpy()[:, :N], left, N_out))
    assert np.all(got[:, N_out:] == 7.0)


@gpu
@pytest.mark.parametrize("n", [4, 1028, 8192 * 256 * 4 + 4])
def test_add_equals_float32_sum(n):
    """One float4, a tail block, and more float4s than the capped 8192-block grid covers in one sweep."""
    from hubertfa_amd import ops
    d = _dev()
    a, b = ref.randn(n, seed=120), ref.randn(n, seed=121, scale=100.0)
    got = ops.add(a.to(d), b.to(d))
    assert torch.equal(got.cpu(), a + b)


@gpu
def test_add_rejects_unaligned():
    from hubertfa_amd import ops, _lib
    d = _dev()
    a = torch.zeros(16, device=d)
    with pytest.raises(_lib.HFALibraryError):
        ops.add(a[:6], a[8:14])                                     # n % 4 != 0
    with pytest.raises(_lib.HFALibraryError):
        ops.add(a[1:9], a[4:12], out=torch.empty(8, device=d))      # a pointer offset by one float


@gpu
@pytest.mark.parametrize("C", [4, 260, 768])
@pytest.mark.parametrize("ratio", [0.5, 1.5, (512 / 44100) / (320 / 16000)])
def test_units_gather_per_row_lengths(C, ratio):
    """n_frames_b / U_b: every row gathers with its own frame count and clamps to its own last unit (rows >= U_b[b] of
    units are NaN and never read); ratios 0.5 and 1.5 put ratio * k on exact halves (round half to even decides);
    rows k >= n_frames_b[b] are exactly 0; each row equals the single-row call."""
    from hubertfa_amd import ops
    d = _dev()
    B, U, T_pad = 4, 40, 64
    U_b, nf = [40, 1, 17, 33], [T_pad, 0, 5, 60]
    ub = ref.randn(B, U, C + 4, seed=130) + 3.0
    for b in range(B):
        ub[b, U_b[b]:] = NAN
    units = ub.to(d)[:, :, :C]
    assert units.stride(1) == C + 4
    out = torch.full((B, T_pad, C), NAN, device=d)
    ops.units_gather(units, max(nf), T_pad, ratio, out=out, n_frames_b=_lens(nf), U_b=_lens(U_b))
    got = out.cpu().numpy()
    assert not np.isnan(got).any()
    want = ref.units_gather(ub.numpy()[:, :, :C], nf, U_b, T_pad, ratio)
    assert np.array_equal(got, want)
    for b in range(B):
        assert np.all(got[b, nf[b]:] == 0)
        alone = ops.units_gather(units[b:b + 1, :U_b[b]], nf[b], T_pad, ratio)
        assert torch.equal(alone[0], out[b]), b


def test_gather_index_rounds_half_to_even():
    """The restated index on exact halves (0.5, 1.5, 2.5, 3.5 -> 0, 2, 2, 4) and the clamp to U - 1."""
    assert ref.gather_index(8, 0.5, 40).tolist() == [0, 0, 1, 2, 2, 2, 3, 4]
    assert ref.gather_index(6, 1.5, 40).tolist() == [0, 2, 3, 4, 6, 8]
    assert ref.gather_index(6, 1.5, 5).tolist() == [0, 2, 3, 4, 4, 4]


@gpu
@pytest.mark.parametrize("N", [1, 5, 63, 4097])
def test_wav_normalize_short_and_unaligned_vs_f64(N):
    """Fewer samples than the 64 partial chunks, one sample, a tail past the last float4, each once 16-byte aligned
    (the float4 path) and once as buf[:, 1:] (the scalar path): both against float64, the same bits from both, zeros
    past each row's length, exactly 0 for N = 1 and for len <= 1."""
    from hubertfa_amd import ops
    d = _dev()
    B = 3
    pitch = (N + 8) // 4 * 4
    x = ref.randn(B, N, seed=140 + N, scale=0.3) + 0.01
    for lens in (None, [N, 0, 1]):
        want = ref.wav_normalize(x, lens)
        got = []
        for off in (0, 1):
            xb = torch.full((B, pitch), 5.0, device=d)
            ob = torch.full((B, pitch), NAN, device=d)
            xv, ov = xb[:, off:off + N], ob[:, off:off + N]
            xv.copy_(x)
            assert xv.data_ptr() % 16 == 4 * off
            ops.wav_normalize(xv, out=ov, lens=None if lens is None else _lens(lens))
            ref.close(ov, want, 1e-5, 1e-5)
            assert bool(torch.isnan(ob[:, :off]).all()) and bool(torch.isnan(ob[:, off + N:]).all())
            got.append(ov.clone())
            for b in range(B):
                n = N if lens is None else lens[b]
                assert bool((ov[b, n:] == 0).all()), b
                if n <= 1:
                    assert bool((ov[b] == 0).all()), b
        assert torch.equal(got[0], got[1])


# ---- 4. lattice prologue on a ragged batch ---------------------------------------------------------------------------
PRO_T, PRO_S, PRO_TL, PRO_SMAX = [300, 1, 0, 37, 299], [70, 1, 2, 64, 65], 300, 72


@functools.lru_cache(maxsize=None)
def _prologue_case(V):
    """logits [B, Tl, V + 2] (the head's layout), ids [B, Smax], and the float64 restatement per row."""
    B = len(PRO_T)
    r = np.random.default_rng(7)
    edge = r.normal(0, 3, (4, PRO_TL))                             # (drawn first: the same edges for every V)
    edge = np.concatenate([edge, r.normal(0, 3, (B - 4, PRO_TL))])
    edge[:, ::10] = 30.0
    edge[:, 5::10] = -30.0
    logits = np.empty((B, PRO_TL, V + 2), np.float32)
    logits[:, :, 2:] = r.normal(0, 3, (B, PRO_TL, V))
    logits[:, :, 1] = r.normal(0, 3, (B, PRO_TL))
    logits[:, :, 0] = edge
    ids = np.full((B, PRO_SMAX), -1, np.int32)
    for b, S in enumerate(PRO_S):
        row = r.integers(0, V, S)
        row[::3] = 0                                               # some id 0 (the first included)
        row[1::7] = row[(1 + 3) % S] if S > 1 else row[0]          # repeated phones
        ids[b, :S] = row
    if PRO_S[4] > 1:
        ids[4, 0] = min(1, V - 1)                                  # one row whose first phone is not id 0 (V > 1)
    lt = torch.from_numpy(logits)
    rows = [ref.lattice_prologue(lt[b], ids[b], PRO_T[b], PRO_S[b]) for b in range(B)]
    return logits, ids, rows


def _band_share(rows):
    valid = sum(len(r["edge_prob"]) for r in rows)
    return sum(int(ref.edge_band(r["edge_prob"]).sum()) for r in rows) / valid


@pytest.mark.parametrize("V", [2, 63, 65, 1024])
def test_prologue_case_is_well_posed(V):
    """The restatement on the test's own input: saturated edge logits clamp to exactly 0 and 1, edge_diff is 0 at each
    row's own last frame, fewer than 2 % of the valid frames fall in the band where log(p + 1e-6) amplifies float32
    rounding, ids repeat and contain 0, and the softmax of every frame sums to 1."""
    logits, ids, rows = _prologue_case(V)
    assert _band_share(rows) < 0.02
    for b, r in enumerate(rows):
        T, S = PRO_T[b], PRO_S[b]
        assert r["prob_log"].shape == (T, S)
        if T == 0:
            continue
        assert np.all(r["e"][0::10] == 1.0) and np.all(r["e"][5::10] == 0.0)
        assert r["edge_diff"][T - 1] == 0.0
        assert np.allclose(r["ph_frame_pred"].sum(-1), 1.0, atol=1e-12)
        assert np.all(r["ph_prob_log"][:, ~r["allowed"]] < -1e8)
        if T > 1:
            assert r["edge_diff"][0] == r["e"][1] - r["e"][0]
    assert (ids[0, :PRO_S[0]] == 0).sum() > 1 and len(set(ids[0, :PRO_S[0]].tolist())) < PRO_S[0]
    assert np.all(ids[3, PRO_S[3]:] == -1)


@gpu
@pytest.mark.parametrize("V", [2, 63, 65, 1024])
def test_prologue_ragged_batch_vs_f64(V):
    """Per-row T and S (T = 0 and 1, S on both sides of 64), V at the 64-lane loop's tail and at kMaxV, strided logit
    views, NaN logit rows past T, -1 ids past S.  Tolerances: tests/test_viterbi_gpu.py::
    test_prologue_logprobs_within_tolerance (log-probs atol 1e-5 on the allowed classes -- a masked class sits at -1e9,
    where one float32 ulp is 64 --, softmax and edge_prob atol 1e-6, edge_log / not_edge_log atol 2e-4 + rtol 1e-5);
    edge_diff atol 1e-6 (two float32 sigmoids, each rounded at ~1e-7, divided by 0.8).  Frames whose edge_prob p has p
    or 1 - p in (0, 1e-3) are left out of the edge_log / not_edge_log comparison only (under 2 % of the frames)."""
    from hubertfa_amd import ops
    d = _dev()
    logits, ids, rows = _prologue_case(V)
    assert _band_share(rows) < 0.02
    lg = logits.copy()
    for b, T in enumerate(PRO_T):
        lg[b, T:] = np.nan
    lg = torch.from_numpy(lg).to(d)
    out = ops.lattice_prologue(lg[:, :, 2:], lg[:, :, 0], torch.from_numpy(ids).to(d), _lens(PRO_T), _lens(PRO_S),
                               want_frame_probs=True, init_dp=True)
    o = {k: v.cpu().numpy() for k, v in out.items() if v is not None}
    at = np.testing.assert_allclose
    for b, r in enumerate(rows):
        T, S = PRO_T[b], PRO_S[b]
        al = r["allowed"]
        at(o["ph_prob_log"][b, :T][:, al], r["ph_prob_log"][:, al], atol=1e-5, rtol=0, err_msg=f"row {b}")
        assert np.all(o["ph_prob_log"][b, :T][:, ~al] < -1e8)
        at(o["ph_frame_pred"][b, :T], r["ph_frame_pred"], atol=1e-6, rtol=0, err_msg=f"row {b}")
        at(o["prob_log"][b, :T, :S], r["prob_log"], atol=1e-5, rtol=0, err_msg=f"row {b}")
        at(o["edge_prob"][b, :T], r["edge_prob"], atol=1e-6, rtol=0, err_msg=f"row {b}")
        at(o["edge_diff"][b, :T], r["edge_diff"], atol=1e-6, rtol=0, err_msg=f"row {b}")
        keep = ~ref.edge_band(r["edge_prob"])
        at(o["edge_log"][b, :T][keep], r["edge_log"][keep], atol=2e-4, rtol=1e-5, err_msg=f"row {b}")
        at(o["not_edge_log"][b, :T][keep], r["not_edge_log"][keep], atol=2e-4, rtol=1e-5, err_msg=f"row {b}")
        # the DP's initialisation, from the restated lattice's own row 0
        row0 = ref.dp_row0(r["prob_log"], ids[b], T, S, PRO_SMAX)
        dp0, cu = o["dp"][b, 0], o["curr"][b]
        fin = np.isfinite(row0)
        assert np.array_equal(np.isneginf(dp0), ~fin) and np.array_equal(np.isneginf(cu), ~fin), b
        at(dp0[fin], row0[fin], atol=1e-5, rtol=0, err_msg=f"row {b}")
        assert np.array_equal(cu, dp0.astype(np.float64)), b
        if T:
            assert np.array_equal(dp0[fin], o["prob_log"][b, 0, :S][fin[:S]]), b
