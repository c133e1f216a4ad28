"""GPU parity tests, kernel by kernel: every libgimhip entry point (through the C ABI / ctypes) against
the CPU oracle or the torch fp32 op it replaces, on the same seeded inputs.

Tolerances: fp32 mode (fp32 MFMA = fmaf chain) 2e-5 relative to the output scale -- summation order is
the only difference; bf16 mode is compared against the fp32 reference evaluated on bf16-rounded
operands, 1.5e-2 (output rounding 2^-9 + accumulation order).  Integer outputs: exact.
The conv cases here have at most 30 tiles, one per workgroup; launches whose workgroups walk several tiles: test_gpu_conv_many_tiles.py."""
import pytest
import torch
import torch.nn.functional as F

import loftr_oracle as O

pytestmark = pytest.mark.gpu

DTS = ["fp32", "bf16", "fp16"]   # fp16: the second 16-bit flavour of every gim_loftr kernel (csrc/gim_common.h)


def _dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda:0")


def _gim(dt):
    from gim_amd import _lib
    return {"bf16": _lib.GIM_BF16, "fp16": _lib.GIM_F16, "fp32": _lib.GIM_F32}[dt]


def _tdt(dt):
    return {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[dt]


def _rnd(t, dt):
    """round like the kernel's operand dtype, keep fp32 container"""
    return t.to(_tdt(dt)).float()


def _tol(dt):
    return {"bf16": 1.5e-2, "fp16": 2e-3, "fp32": 2e-5}[dt]


def _ht(dt, half, full):
    """tolerance of a memory-bound kernel: `half` for bf16 outputs, an eighth of it for fp16 (3 more bits), `full` for fp32"""
    return {"bf16": half, "fp16": half / 8, "fp32": full}[dt]


def _assert_close(got, ref, tol, what=""):
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    scale = max(1e-6, ref.abs().max().item())
    err = (got - ref).abs().max().item()
    assert err <= tol * scale, f"{what}: max|err|={err:.3e} scale={scale:.3e} rel={err / scale:.3e} tol={tol}"


def _to_nhwc(x, cs, dt, dev):
    """[B,C,H,W] fp32 cpu -> [B,H,W,cs] device tensor of compute dtype (host-side test plumbing)"""
    B, C, H, W = x.shape
    y = torch.zeros(B, H, W, cs)
    y[..., :C] = x.permute(0, 2, 3, 1)
    return y.to(_tdt(dt)).to(dev).contiguous()


CONV_CASES = [
    # (B, Cin, H, W, Cout, k, stride, bn, act, residual)
    (2, 64, 24, 40, 64, 1, 1, True, "relu", False),      # 256x64 tile config
    (2, 64, 24, 40, 256, 1, 1, True, "relu", True),      # 128x128 config + residual
    (1, 64, 17, 23, 64, 3, 1, True, "relu", False),      # ragged M, spatial padding
    (2, 128, 20, 28, 128, 3, 2, True, "relu", False),    # stride 2
    (1, 256, 12, 16, 512, 1, 2, True, "none", False),    # strided 1x1 (downsample)
    (2, 3, 32, 48, 64, 7, 2, True, "relu", False),       # stem
    (1, 256, 10, 14, 196, 3, 1, False, "none", False),   # 196 outputs (n_store 196/200)
    (1, 196, 10, 14, 196, 3, 1, True, "leaky", False),   # 196 inputs (cin_pad 196/200)
    (1, 196, 9, 11, 128, 3, 1, False, "none", False),
    (1, 1024, 6, 8, 256, 1, 1, False, "none", False),    # long K
    (2, 144, 37, 45, 144, 1, 1, False, "relu", False),   # npad 192: the 256 x 192 tile (16-bit, round 4), ragged M
    (1, 96, 20, 28, 160, 3, 1, True, "leaky", False),    # npad 192 again, 3x3, N = 160 (the last 32-channel fragment empty)
]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("dma", [True, False])
@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_conv2d_bn_act(case, dt, dma):
    from gim_amd import ops
    from gim_amd.packing import cstore, pack_conv
    dev = _dev()
    B, Cin, H, W, Cout, k, stride, use_bn, act, use_res = case
    g = torch.Generator().manual_seed(1000 + CONV_CASES.index(case))
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) * (2.0 / (Cin * k * k)) ** 0.5
    bn = None
    if use_bn:
        bn = (0.75 + 0.5 * torch.rand(Cout, generator=g), 0.1 * torch.randn(Cout, generator=g),
              0.1 * torch.randn(Cout, generator=g), 0.5 + torch.rand(Cout, generator=g), 1e-5)
    gd = _gim(dt)
    pk = pack_conv(w, bn, gd, dev, stride=stride, pad=k // 2, cin_pad=cstore(Cin, gd))
    xd = _to_nhwc(x, pk.cin_pad, dt, dev)
    Ho, Wo = (H + 2 * (k // 2) - k) // stride + 1, (W + 2 * (k // 2) - k) // stride + 1
    res = torch.randn(B, Cout, Ho, Wo, generator=g) if use_res else None
    resd = _to_nhwc(res, pk.n_store, dt, dev) if use_res else None
    actc = {"none": ops.ACT_NONE, "relu": ops.ACT_RELU, "leaky": ops.ACT_LEAKY}[act]
    y = ops.conv2d(xd, pk, actc, res=resd, lds_dma=dma)
    torch.cuda.synchronize()
    assert y.shape == (B, Ho, Wo, pk.n_store)
    # reference: same folded weights (rounded like the kernel's operands), fp32 math on the CPU
    from gim_amd.packing import fold_bn
    wf, bf = fold_bn(w, bn)
    ref = F.conv2d(_rnd(x, dt), _rnd(wf, dt), bf, stride=stride, padding=k // 2)
    if use_res:
        ref = ref + _rnd(res, dt)
    ref = {"none": lambda v: v, "relu": F.relu, "leaky": lambda v: F.leaky_relu(v, 0.01)}[act](ref)
    got = y.float().cpu()[..., :Cout].permute(0, 3, 1, 2)
    _assert_close(got, ref, _tol(dt), f"conv {case} {dt} dma={dma}")
    if pk.n_store > Cout:  # padded channels must be exact zeros (next layer reads them)
        assert (y.float().cpu()[..., Cout:] == 0).all()


@pytest.mark.parametrize("dt", DTS)
def test_linear_strided_views_and_elu(dt):
    """nn.Linear via the conv kernel on column-sliced row views (the transformer's concat buffer)."""
    from gim_amd import ops
    from gim_amd.packing import pack_conv
    dev = _dev()
    g = torch.Generator().manual_seed(3)
    R, C = 333, 256
    cat = torch.randn(R, 2 * C, generator=g)
    wq = torch.randn(C, C, generator=g) / C ** 0.5
    w0 = torch.randn(2 * C, 2 * C, generator=g) / (2 * C) ** 0.5
    gd = _gim(dt)
    catd = cat.to(_tdt(dt)).to(dev)
    q = torch.full((R, C), float("nan"), dtype=_tdt(dt), device=dev)
    ops.linear(catd[:, :C], pack_conv(wq, None, gd, dev), q, ops.ACT_ELU1)
    hid = torch.full((R + 5, 2 * C), float("nan"), dtype=torch.float32, device=dev)
    ops.linear(catd, pack_conv(w0, None, gd, dev), hid[:R], ops.ACT_RELU)
    torch.cuda.synchronize()
    ref_q = F.elu(F.linear(_rnd(cat[:, :C], dt), _rnd(wq, dt))) + 1
    ref_h = F.relu(F.linear(_rnd(cat, dt), _rnd(w0, dt)))
    _assert_close(q, ref_q, _tol(dt), "q_proj+elu1")
    _assert_close(hid[:R], ref_h, _tol(dt), "mlp0+relu")
    assert torch.isnan(hid[R:]).all(), "rows beyond M were written"


@pytest.mark.parametrize("dt", DTS)
def test_layout_roundtrip_and_upsample_posenc(dt):
    from gim_amd import ops
    from gim_amd.packing import cstore
    dev = _dev()
    gd = _gim(dt)
    g = torch.Generator().manual_seed(5)
    x = torch.rand(3, 3, 20, 28, generator=g)
    cs = cstore(3, gd)
    buf = torch.full((5, 20, 28, cs), float("nan"), dtype=_tdt(dt), device=dev)
    ops.nchw_to_nhwc(x[:2].to(dev), buf, 0)
    ops.nchw_to_nhwc(x[2:].to(dev), buf, 2)
    back = ops.nhwc_to_nchw(buf[:3], 3)
    torch.cuda.synchronize()
    _assert_close(back, _rnd(x, dt), 0.0, "nchw->nhwc->nchw")
    assert (buf[:3, ..., 3:].float() == 0).all()
    # upsample (align_corners=True) + add
    lo = torch.randn(2, 196, 7, 9, generator=g)
    hi = torch.randn(2, 196, 14, 18, generator=g)
    c2 = cstore(196, gd)
    lod, hid_ = _to_nhwc(lo, c2, dt, dev), _to_nhwc(hi, c2, dt, dev)
    ops.upsample2x_add(lod, hid_)
    ref = _rnd(hi, dt) + F.interpolate(_rnd(lo, dt), scale_factor=2.0, mode="bilinear", align_corners=True)
    torch.cuda.synchronize()
    _assert_close(hid_.float().cpu()[..., :196].permute(0, 3, 1, 2), ref, _ht(dt, 1e-2, 1e-6), "upsample2x_add")
    # posenc
    pe = O.position_encoding(256, 6, 8)[0]  # [C,h,w]
    feat = torch.randn(2, 256, 6, 8, generator=g)
    fd = _to_nhwc(feat, 256, dt, dev)
    out32 = torch.empty(2 * 48, 256, device=dev)
    outt = torch.empty(2 * 48, 512, dtype=_tdt(dt), device=dev)
    ops.posenc_add(fd.view(-1, 256), pe.permute(1, 2, 0).reshape(48, 256).contiguous().to(dev), out32, outt[:, :256])
    torch.cuda.synchronize()
    ref = (_rnd(feat, dt) + pe[None]).flatten(2).transpose(1, 2).reshape(96, 256)
    _assert_close(out32, ref, 1e-6, "posenc f32")
    _assert_close(outt[:, :256], ref, _ht(dt, 1e-2, 1e-6), "posenc T")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("C", [256, 128])
def test_layernorm_residual(dt, C):
    from gim_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(7)
    R = 203
    x = torch.randn(R, C, generator=g) * 3 + 0.5
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.1
    res = torch.randn(R, C, generator=g)
    o32 = torch.empty(R, C, device=dev)
    ot = torch.empty(R, 2 * C, dtype=_tdt(dt), device=dev)
    ops.layernorm_residual(x.to(dev), gamma.to(dev), beta.to(dev), res.to(dev), o32, ot[:, C:])
    ops.layernorm_residual(x.to(dev), gamma.to(dev), beta.to(dev), None, None, ot[:, :C])
    torch.cuda.synchronize()
    ref = F.layer_norm(x, (C,), gamma, beta, 1e-5)
    _assert_close(o32, ref + res, 1e-5, "ln+res f32")
    _assert_close(ot[:, C:], ref + res, _ht(dt, 1e-2, 1e-5), "ln+res T")
    _assert_close(ot[:, :C], ref, _ht(dt, 1e-2, 1e-5), "ln T")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shape", [(3, 300, 300, 8, 32), (2, 77, 150, 8, 32), (5, 25, 25, 8, 16), (6, 40, 33, 8, 32),
                                   (9, 25, 25, 8, 16)],
                         ids=lambda s: "x".join(map(str, s)))
def test_linear_attention(dt, shape):
    """against oracle linear_attention (attentions.py:20-47); q/k pre-mapped by elu+1 like the GEMM epilogue"""
    from gim_amd import ops
    dev = _dev()
    nb, L, S, H, D = shape
    g = torch.Generator().manual_seed(11)
    q = torch.randn(nb, L, H, D, generator=g)
    k = torch.randn(nb, S, H, D, generator=g)
    v = torch.randn(nb, S, H, D, generator=g)
    Qe, Ke = _rnd(F.elu(q) + 1, dt), _rnd(F.elu(k) + 1, dt)
    vr = _rnd(v, dt)
    # oracle on the rounded, already-mapped operands: undo the map (elu(x)+1 == y  <=>  feed y-1 for y>=1 ...)
    # simpler: restate with the mapped tensors directly
    vl = vr / S
    KV = torch.einsum("nshd,nshv->nhdv", Ke, vl)
    Z = 1 / (torch.einsum("nlhd,nhd->nlh", Qe, Ke.sum(dim=1)) + 1e-6)
    ref = torch.einsum("nlhd,nhdv,nlh->nlhv", Qe, KV, Z) * S
    # sanity: same as the oracle function on raw q,k when no rounding is involved
    if dt == "fp32":
        assert (ref - O.linear_attention(q, k, v)).abs().max() < 1e-4
    C = H * D
    out = torch.empty(nb * L, C, dtype=_tdt(dt), device=dev)
    ops.linear_attention(Qe.reshape(nb * L, C).to(_tdt(dt)).to(dev), Ke.reshape(nb * S, C).to(_tdt(dt)).to(dev),
                         vr.reshape(nb * S, C).to(_tdt(dt)).to(dev), out, nb, L, nb, S, H)
    torch.cuda.synchronize()
    _assert_close(out.view(nb, L, H, D), ref, _ht(dt, 1e-2, 1e-5), f"linear attention {shape}")


COARSE_CASES = [
    # (N, h0c, w0c, h1c, w1c, sigma, eps, scaled)
    (2, 12, 16, 12, 16, 1.0, 0.5, False),
    (2, 12, 16, 12, 16, 1.0, 0.5, True),
    (1, 15, 20, 15, 20, 2.0, 0.1, False),     # L=S=300: ragged 128-tiles
    (3, 9, 13, 9, 13, 1.0, 0.3, True),
    (1, 30, 40, 30, 40, 1.0, 0.5, False),     # 1200 cells, 10x10 tiles
]


@pytest.mark.parametrize("case", COARSE_CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_coarse_match(case):
    """bit-exact (b,i,j) + ordering, mconf / mkpts within 1e-5, against the oracle (coarse_matching.py)"""
    from gim_amd import ops
    dev = _dev()
    N, h0, w0, h1, w1, sigma, eps, scaled = case
    f0, f1, _ = O.planted_coarse_features(N, (h0, w0), sigma=sigma, eps=eps, seed=101)
    s0 = s1 = None
    if scaled:
        g = torch.Generator().manual_seed(1)
        s0, s1 = 0.5 + 2 * torch.rand(N, 2, generator=g), 0.5 + 2 * torch.rand(N, 2, generator=g)
    hw_i = (h0 * 8, w0 * 8)
    conf = O.conf_matrix_dual_softmax(f0, f1, 0.1)
    ref = O.get_coarse_match(conf, hw_i, hw_i, (h0, w0), (h1, w1), 0.2, 2, s0, s1)
    r = ops.coarse_match(f0.to(dev), f1.to(dev), (h0, w0), (h1, w1), 8.0, 0.1, 0.2, 2,
                         s0.to(dev) if scaled else None, s1.to(dev) if scaled else None)
    cnt = r.count.cpu()
    M = int(cnt[0])
    assert ref["b_ids"].numel() > 20, "test input produced too few matches"
    assert M == ref["b_ids"].numel(), f"M={M} ref={ref['b_ids'].numel()}"
    assert int(cnt[1]) == 0                                                             # health word: finite similarities
    assert cnt[2:].tolist() == torch.bincount(ref["b_ids"], minlength=N).tolist()
    for k in ("b_ids", "i_ids", "j_ids"):
        got = getattr(r, k)[:M].cpu()
        assert got.dtype == torch.int64
        assert torch.equal(got, ref[k]), k
    _assert_close(r.mconf[:M], ref["mconf"], 1e-5, "mconf")
    _assert_close(r.mkpts0_c[:M], ref["mkpts0_c"], 1e-6, "mkpts0_c")
    _assert_close(r.mkpts1_c[:M], ref["mkpts1_c"], 1e-6, "mkpts1_c")
    cm = ops.coarse_conf_matrix(r)
    _assert_close(cm, conf, 1e-5, "conf_matrix")


def test_coarse_match_different_shapes_and_empty():
    from gim_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(9)
    # L != S
    f0 = torch.randn(2, 8 * 10, 256, generator=g)
    f1 = torch.cat([f0[:, torch.randperm(80, generator=g)], torch.randn(2, 40, 256, generator=g)], 1) \
        + 0.2 * torch.randn(2, 120, 256, generator=g)
    conf = O.conf_matrix_dual_softmax(f0, f1, 0.1)
    ref = O.get_coarse_match(conf, (64, 80), (80, 96), (8, 10), (10, 12), 0.2, 2)
    r = ops.coarse_match(f0.to(dev), f1.to(dev), (8, 10), (10, 12), 8.0)
    M = int(r.count[0])
    assert M == ref["b_ids"].numel() and M > 0
    for k in ("b_ids", "i_ids", "j_ids"):
        assert torch.equal(getattr(r, k)[:M].cpu(), ref[k])
    # no match at all: uniform features
    z = torch.zeros(1, 48, 256)
    r = ops.coarse_match(z.to(dev), z.to(dev), (6, 8), (6, 8), 8.0)
    assert int(r.count[0]) == 0


@pytest.mark.parametrize("tdt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_coarse_match_bf16_features_strided(tdt):
    """16-bit features (the throughput mode's token buffers, rows strided inside a wider buffer): the bf16 MFMA computes exact
    products with fp32 accumulation, so against the oracle evaluated on the SAME bf16-valued features the indices are
    exact and the confidences differ by summation order only"""
    from gim_amd import ops
    dev = _dev()
    N, h0, w0 = 2, 15, 20
    f0, f1, _ = O.planted_coarse_features(N, (h0, w0), sigma=1.0, eps=0.5, seed=33)
    b0, b1 = f0.to(tdt), f1.to(tdt)
    conf = O.conf_matrix_dual_softmax(b0.float(), b1.float(), 0.1)
    ref = O.get_coarse_match(conf, (h0 * 8, w0 * 8), (h0 * 8, w0 * 8), (h0, w0), (h0, w0), 0.2, 2)
    C = 256
    buf = torch.zeros(2 * N * h0 * w0, 2 * C, dtype=tdt, device=dev)           # [x | other columns], like T.CAT
    buf[:N * h0 * w0, :C] = b0.reshape(-1, C).to(dev)
    buf[N * h0 * w0:, :C] = b1.reshape(-1, C).to(dev)
    buf[:, C:] = 7.0                                                                          # must never be read
    v0 = buf[:N * h0 * w0].view(N, h0 * w0, 2 * C)[:, :, :C]
    v1 = buf[N * h0 * w0:].view(N, h0 * w0, 2 * C)[:, :, :C]
    r = ops.coarse_match(v0, v1, (h0, w0), (h0, w0), 8.0, 0.1, 0.2, 2)
    M = int(r.count[0])
    assert ref["b_ids"].numel() > 100 and M == ref["b_ids"].numel()
    for k in ("b_ids", "i_ids", "j_ids"):
        assert torch.equal(getattr(r, k)[:M].cpu(), ref[k]), k
    _assert_close(r.mconf[:M], ref["mconf"], 1e-5, "mconf")
    _assert_close(ops.coarse_conf_matrix(r), conf, 1e-5, "conf_matrix")


@pytest.mark.parametrize("dt", DTS)
def test_fine_gather_and_match(dt):
    """fine_preprocess.py:40-47 windows (incl. zero padded border cells) and fine_matching.py:43-74"""
    from gim_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(13)
    bs, hc, wc, stride, W, C = 2, 6, 8, 4, 5, 128
    hf, wf = hc * stride, wc * stride
    ff0, ff1 = torch.randn(bs, C, hf, wf, generator=g), torch.randn(bs, C, hf, wf, generator=g)
    M = 37
    b_ids = torch.randint(0, bs, (M,), generator=g).sort()[0]
    i_ids = torch.randint(0, hc * wc, (M,), generator=g)
    j_ids = torch.randint(0, hc * wc, (M,), generator=g)
    i_ids[:4] = torch.tensor([0, wc - 1, wc * (hc - 1), hc * wc - 1])  # corners -> zero padding
    u0, u1 = O.fine_preprocess(_rnd(ff0, dt), _rnd(ff1, dt), b_ids, i_ids, j_ids, (hc, wc), (hf, wf), W)
    fd0, fd1 = _to_nhwc(ff0, C, dt, dev), _to_nhwc(ff1, C, dt, dev)
    o32 = torch.empty(2 * M * W * W, C, device=dev)
    ot = torch.empty(2 * M * W * W, 2 * C, dtype=_tdt(dt), device=dev)
    ops.fine_gather(fd0, fd1, b_ids.to(dev), i_ids.to(dev), j_ids.to(dev), M, wc, wc, stride, W, o32, ot[:, :C])
    torch.cuda.synchronize()
    ref = torch.cat([u0, u1], 0).reshape(-1, C)
    _assert_close(o32, ref, 0.0, "fine gather f32")
    _assert_close(ot[:, :C], ref, 0.0, "fine gather T")
    # fine matching on fp32 windows
    t0, t1 = torch.randn(M, W * W, C, generator=g), torch.randn(M, W * W, C, generator=g)
    mk1c = torch.rand(M, 2, generator=g) * 100
    s1 = 0.5 + torch.rand(bs, 2, generator=g)
    for has in (False, True):
        refm = O.fine_matching(t0, t1, mk1c.clone(), mk1c, b_ids, M, (hc * 8, wc * 8), (hf, wf), s1, has)
        e, m1 = ops.fine_match(t0.reshape(-1, C).to(dev), t1.reshape(-1, C).to(dev), mk1c.to(dev),
                               b_ids.to(dev), s1.to(dev), M, W * W, 2.0, has)
        torch.cuda.synchronize()
        _assert_close(e, refm["expec_f"], 1e-5, "expec_f")
        _assert_close(m1, refm["mkpts1_f"], 1e-6, "mkpts1_f")


def test_coarse_match_precandidate_overflow_fallback():
    """with NO pre-candidate buffer (gim_coarse_args.precand_per_row = -1; until round 5 an environment hook of the library) the device-side
    overflow flag must route to the recompute pass and give the same exact result"""
    from gim_amd import ops
    f0, f1, _ = O.planted_coarse_features(1, (30, 40), sigma=1.0, eps=0.5, seed=7)
    conf = O.conf_matrix_dual_softmax(f0, f1, 0.1)
    ref = O.get_coarse_match(conf, (240, 320), (240, 320), (30, 40), (30, 40), 0.2, 2)
    for per_row in (-1, 1, 0):
        r = ops.coarse_match(f0.cuda(), f1.cuda(), (30, 40), (30, 40), 8.0, precand_per_row=per_row)
        M = int(r.count[0])
        assert M == ref['b_ids'].numel() and M > 600, (per_row, M, ref['b_ids'].numel())
        assert torch.equal(r.i_ids[:M].cpu(), ref['i_ids']) and torch.equal(r.j_ids[:M].cpu(), ref['j_ids']), per_row
        assert (r.mconf[:M].cpu() - ref['mconf']).abs().max() < 1e-5, per_row


def test_conv_big_tile_forced():
    """the 256 x 256 / 8-wave tile is picked by a size heuristic (>= 1024 tiles, >= 4 K slabs): force it onto every eligible conv / linear
    case of this file (gim_conv_args.use_lds_dma = 3 through GIM_FLAGS=force_big_tile=1; read once per process -> subprocess)"""
    env = {"GIM_FLAGS": "force_big_tile=1"}
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_kernels.py", "-m", "gpu", "-q", "-x",
                          "-k", "conv2d_bn_act or linear_strided", "-p", "no:cacheprovider"],
                         cwd=root, capture_output=True, text=True, env={**os.environ, **env}, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]


@pytest.mark.parametrize("shape", [(4, 25, 25, 8, 16), (2, 200, 140, 8, 32)], ids=["short", "long"])
def test_linear_attention_masks(shape):
    """q_mask / kv_mask (attentions.py:35-39) on both the fused short-sequence kernel and the chunked one"""
    from gim_amd import ops
    dev = _dev()
    nb, L, S, H, D = shape
    g = torch.Generator().manual_seed(17)
    q, k, v = (torch.randn(nb, n, H, D, generator=g) for n in (L, S, S))
    qm = torch.rand(nb, L, generator=g) > 0.3
    km = torch.rand(nb, S, generator=g) > 0.3
    ref = O.linear_attention(q, k, v, qm, km)
    C = H * D
    Qe, Ke = F.elu(q) + 1, F.elu(k) + 1
    out = torch.empty(nb * L, C, device=dev)
    ops.linear_attention(Qe.reshape(nb * L, C).to(dev), Ke.reshape(nb * S, C).to(dev), v.reshape(nb * S, C).to(dev), out,
                         nb, L, nb, S, H, None, qm.reshape(-1).to(torch.uint8).to(dev), km.reshape(-1).to(torch.uint8).to(dev))
    torch.cuda.synchronize()
    _assert_close(out.view(nb, L, H, D), ref, 1e-5, f"masked linear attention {shape}")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shape", [(16, 4800, True, False), (3, 1000, False, True), (2, 257, True, True)],
                         ids=["coarse16x4800-strided", "3x1000-masked", "2x257-strided-masked"])
def test_linear_attention_state(dt, shape):
    """gim_linear_attention_kv alone (the MFMA kernels of the coarse level: D = 32, H = 8): the final KV / Ksum state against a float64
    einsum on the rounded operands -- at the benchmark's size with K / V as column blocks of a [rows, 3C] projection buffer (the
    layout gim_token_mlp_emit writes), on ragged last chunks, and with kv_mask (attentions.py:38-43)."""
    from gim_amd import ops
    dev = _dev()
    nb, S, strided, masked = shape
    H, D, C = 8, 32, 256
    g = torch.Generator().manual_seed(23)
    k = _rnd(F.elu(torch.randn(nb * S, C, generator=g)) + 1, dt)
    v = _rnd(torch.randn(nb * S, C, generator=g), dt)
    km = (torch.rand(nb * S, generator=g) > 0.25) if masked else None
    buf = torch.zeros(nb * S, 3 * C if strided else 2 * C, dtype=_tdt(dt))
    buf[:, -2 * C:-C], buf[:, -C:] = k.to(_tdt(dt)), v.to(_tdt(dt))
    bd = buf.to(dev)
    ws, need = ops.linear_attention_state(bd[:, -2 * C:-C], bd[:, -C:], nb, S, H,
                                          kv_mask=km.to(torch.uint8).to(dev) if masked else None)
    torch.cuda.synchronize()
    got = ws[:nb * H * (D * D + D)].view(nb, H, D * D + D).cpu().double()
    kd, vd = k.double().view(nb, S, H, D), v.double().view(nb, S, H, D)
    if masked:
        kd, vd = kd * km.view(nb, S, 1, 1), vd * km.view(nb, S, 1, 1)
    KV = torch.einsum("nshd,nshv->nhdv", kd, vd / S)
    ref = torch.cat([KV.reshape(nb, H, D * D), kd.sum(1)], -1)
    # fp32 accumulation of S products: error ~ sqrt(S) * 2^-24 of the running sums (a wrong row, mask or head shows at 1e-2)
    _assert_close(got[..., :D * D], ref[..., :D * D], 1e-5, f"KV state {shape}")
    _assert_close(got[..., D * D:], ref[..., D * D:], 1e-5, f"Ksum {shape}")


@pytest.mark.parametrize("dt", [d for d in DTS if d != "fp32"])
@pytest.mark.parametrize("shape", [(16, 4800), (66, 1000), (130, 257)], ids=["16x4800", "66x1000-ragged", "130x257-ragged"])
def test_linear_attention_state_is_batch_invariant(dt, shape):
    """A sequence's KV / Ksum state must not depend on the batch it travels in: large batches run la_kv_h16_kernel with 512 rows
    per workgroup, small ones with 256 -- both write the partials of 256-row chunks with the same association, so the state of the same
    sequences computed alone (nb = 2: the 256-row shape) is BIT-identical to its rows of the large call (the 512-row shape), also where the
    last chunk is ragged (S % 512 <= 256: the 512-row shape's last half chunk does not exist)."""
    from gim_amd import ops
    dev = _dev()
    nb, S = shape
    H, D, C = 8, 32, 256
    g = torch.Generator().manual_seed(29)
    k = (F.elu(torch.randn(nb * S, C, generator=g)) + 1).to(_tdt(dt)).to(dev)
    v = torch.randn(nb * S, C, generator=g).to(_tdt(dt)).to(dev)
    assert nb * ((S + 255) // 256) * 2 > 512 and 2 * ((S + 255) // 256) * 2 <= 512   # the large call takes the 512-row shape, the small one not
    ws, _ = ops.linear_attention_state(k, v, nb, S, H)
    per = H * (D * D + D)
    big = ws[:nb * per].view(nb, per).clone()
    for b0 in (0, nb - 2):
        ws2, _ = ops.linear_attention_state(k[b0 * S:(b0 + 2) * S], v[b0 * S:(b0 + 2) * S], 2, S, H)
        torch.cuda.synchronize()
        assert torch.equal(ws2[:2 * per].view(2, per), big[b0:b0 + 2]), (shape, b0, (ws2[:2 * per].view(2, per) - big[b0:b0 + 2]).abs().max().item())


@pytest.mark.parametrize("mode", ["tile256", "tile128"], ids=["rows256x128-2wg", "tile128-kernel-via-masks"])
@pytest.mark.parametrize("kind", ["bf16", "fp16"])
def test_coarse_match_tile256_statistics(mode, kind):
    """The persistent 256-row statistics kernel (16-bit features, no masks; round 4: row / column maxima and sums straight from the
    accumulators; two 4-wave workgroups per CU on 256 x 128 tiles) against the oracle evaluated on the SAME 16-bit-valued features: exact
    indices and order, confidences to 1e-5 -- on sizes with ragged last tiles in both directions, unequal L / S, several pairs (8: pair =
    tile % N walks every pair), a wide logit range (sigma = 3: similarities of ~90 beside rows that peak at ~15).  `tile128`: the same
    cases through the 128 x 128 tile-per-workgroup kernel, which takes 16-bit features when padding masks are given -- all-valid masks
    here, so the answer is the same (coarse_matching.py:118-123, 149-172: masked_fill / mask_border_with_padding are no-ops then)."""
    from gim_amd import ops
    tdt = torch.bfloat16 if kind == "bf16" else torch.float16

    def run(b0, b1, hw0, hw1):
        if mode == "tile128":
            N = b0.shape[0]
            m0 = torch.ones(N * hw0[0] * hw0[1], dtype=torch.uint8, device="cuda")
            m1 = torch.ones(N * hw1[0] * hw1[1], dtype=torch.uint8, device="cuda")
            return ops.coarse_match(b0.cuda(), b1.cuda(), hw0, hw1, 8.0, 0.1, 0.2, 2, mask0=m0, mask1=m1)
        return ops.coarse_match(b0.cuda(), b1.cuda(), hw0, hw1, 8.0, 0.1, 0.2, 2)

    for (N, hw0, hw1, sigma, eps, seed) in ((2, (30, 40), (30, 40), 1.0, 0.5, 3), (1, (36, 45), (36, 45), 2.0, 0.1, 4), (3, (25, 31), (25, 31), 1.0, 0.3, 5),
                                            (1, (60, 80), (60, 80), 1.0, 0.5, 6), (1, (30, 40), (30, 40), 3.0, 0.1, 8), (8, (17, 23), (17, 23), 1.0, 0.5, 11)):
        f0, f1, _ = O.planted_coarse_features(N, hw0, sigma=sigma, eps=eps, seed=seed)
        b0, b1 = f0.to(tdt), f1.to(tdt)
        conf = O.conf_matrix_dual_softmax(b0.float(), b1.float(), 0.1)
        ref = O.get_coarse_match(conf, (hw0[0] * 8, hw0[1] * 8), (hw1[0] * 8, hw1[1] * 8), hw0, hw1, 0.2, 2)
        r = run(b0, b1, hw0, hw1)
        M = int(r.count[0])
        assert M == ref['b_ids'].numel() and M > 200, (M, ref['b_ids'].numel())
        for k in ('b_ids', 'i_ids', 'j_ids'):
            assert torch.equal(getattr(r, k)[:M].cpu(), ref[k]), k
        assert (r.mconf[:M].cpu() - ref['mconf']).abs().max() < 1e-5
        cm = ops.coarse_conf_matrix(r).cpu()
        assert (cm - conf).abs().max() < 1e-5 * conf.abs().max().clamp_min(1e-6) + 1e-7
    # unequal map sizes (L != S), ragged in both directions
    f0, f1, _ = O.planted_coarse_features(2, (30, 40), sigma=1.0, eps=0.5, seed=9)
    f1 = f1[:, :29 * 40].contiguous()
    b0, b1 = f0.to(tdt), f1.to(tdt)
    conf = O.conf_matrix_dual_softmax(b0.float(), b1.float(), 0.1)
    ref = O.get_coarse_match(conf, (240, 320), (232, 320), (30, 40), (29, 40), 0.2, 2)
    r = run(b0, b1, (30, 40), (29, 40))
    M = int(r.count[0])
    assert M == ref['b_ids'].numel() and torch.equal(r.j_ids[:M].cpu(), ref['j_ids']) and torch.equal(r.i_ids[:M].cpu(), ref['i_ids'])
