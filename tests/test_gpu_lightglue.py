"""GPU parity tests of the gim_lightglue path (SuperPoint + LightGlue + adapter), through the C ABI, against
oracle/lightglue_oracle.py on the same seeded inputs and against the golden vectors recorded from the
reference's own modules (tests/golden/lg_*.npz).

Bars: keypoint coordinates, arg-max / match indices: exact in fp32 mode (fp32 MFMA); floats 2e-5 of the
output scale in fp32 mode (summation order only); bf16 mode: 6.5e-3 = 2 x the largest value measured on MI355X (3.2e-3 of scale, one
bf16 output rounding; profiles/r04_secondary_measured.txt -- the bound was 1.5e-2 ... 2.5e-2 through round 3); fp16 kernels: the bf16
bar / 6 (three more significand bits; tests/test_gpu_dkm.py::_t16) = 1.08e-3 of scale.  For sdpa that bar rests on the fp64 emulation of
the kernel's own roundings (_attention64 with kinds: P and the output rounded where the kernel rounds them), which the tests assert to
stay below HALF of it on their inputs.

Largest fraction of scale measured on MI355X per kernel, bf16 / fp16 (bars 6.5e-3 / 1.08e-3 unless noted):
  sdpa D=64, all of test_sdpa*          3.24e-3 (2048 x 2048) / 4.09e-4 (256 x 128)   -- equal to the emulation to 3 digits: the kernel
                                        adds nothing measurable to its roundings
  sdpa 16-bit operands -> fp32 out      6.7e-4, 9.2e-4 (D=128) / 8.4e-5, 9.9e-5 (D=128)
  sdpa fp32 operands -> 16-bit out      2.6e-3 / 3.1e-4
  sdpa late maximum (keys 195, 70)      0 / 0 (the output is v[planted], a 16-bit value); fp32 8.2e-8
  layernorm_act (bars 5e-3 / 8.3e-4)    2.2e-3 / 3.5e-4
  lg_rotary vs the once-rounded fp64    5.6e-5 / 1.1e-4 of scale; 5.9e-5 / 3.9e-5 of the elements differ at all (one unit)
  maxpool2x2, lg_transpose, cast_rows, sp_sample_desc's out_t: bit-exact; fp32 outputs (bars 2e-6), any kind: sp_scores 5.4e-7, sp_sample_desc 5.0e-7."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lightglue_oracle as O

pytestmark = pytest.mark.gpu
DTS = ["fp32", "bf16", "fp16"]   # fp16: the IEEE-fp16 flavour of every kernel (GIM_HALF_KIND = 1 objects)
H16 = ["bf16", "fp16"]


def _dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda:0")


def _tdt(dt):
    return {"bf16": torch.bfloat16, "fp16": torch.float16}.get(dt, torch.float32)


def _t16(dt, bf16_tol, fp32_tol):
    """tolerance of a kernel test by operand kind (tests/test_gpu_dkm.py): fp16 keeps 3 more significand bits than bf16"""
    return {"bf16": bf16_tol, "fp16": bf16_tol / 6}.get(dt, fp32_tol)


def _tol(dt):
    return _t16(dt, 6.5e-3, 2e-5)


def _close(got, ref, tol, what=""):
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    scale = max(1e-6, ref.abs().max().item())
    err = (got - ref).abs().max().item()
    print(f"[close] {what}: {err / scale:.3e} of scale (tol {tol:g})")   # pytest -s: the measured value the tolerance is set from
    assert err <= tol * scale, f"{what}: max|err|={err:.3e} scale={scale:.3e} tol={tol}"


# ------------------------------------------------------------------------------------------- SuperPoint glue
@pytest.mark.parametrize("dt", DTS)
def test_maxpool2x2(dt):
    from gim_amd import ops
    dev = _dev()
    x = torch.randn(2, 12, 20, 64, generator=torch.Generator().manual_seed(1)).to(_tdt(dt))
    y = ops.maxpool2x2(x.to(dev))
    ref = F.max_pool2d(x.float().permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)
    assert torch.equal(y.float().cpu(), ref)


@pytest.mark.parametrize("dt", DTS)
def test_sp_scores(dt):
    from gim_amd import ops
    dev = _dev()
    B, h, w = 2, 5, 7
    logits = (3 * torch.randn(B * h * w, 72, generator=torch.Generator().manual_seed(2))).to(_tdt(dt))
    got = ops.sp_scores(logits.to(dev), B, h, w)
    lg = logits.float()[:, :65].reshape(B, h, w, 65).permute(0, 3, 1, 2)
    prob = F.softmax(lg, 1)[:, :-1]
    ref = prob.permute(0, 2, 3, 1).reshape(B, h, w, 8, 8).permute(0, 1, 3, 2, 4).reshape(B, h * 8, w * 8)
    _close(got, ref, 2e-6, "sp_scores")


def _score_map(B, H, W, seed, plateau=False):
    g = torch.Generator().manual_seed(seed)
    s = torch.rand(B, H, W, generator=g) * 0.05
    s = F.avg_pool2d(s[:, None], 3, 1, 1)[:, 0].contiguous()      # smooth: maxima spaced like real score maps
    if plateau:
        s[:, 10:14, 20:30] = 0.04                                  # equal neighbours both survive (superpoint.py:63)
    return s


@pytest.mark.parametrize("radius,border,plateau", [(3, 4, False), (4, 4, True), (1, 0, False)])
def test_sp_nms(radius, border, plateau):
    from gim_amd import ops
    dev = _dev()
    s = _score_map(2, 48, 72, 3, plateau)
    got = ops.sp_nms(s.to(dev), radius, border).cpu()
    ref = O.simple_nms(s, radius)
    if border:
        ref = O.mask_borders(ref, torch.tensor([[72, 48]] * 2), border)
    assert torch.equal(got, ref)


@pytest.mark.parametrize("k,thr", [(64, 0.0), (200, 0.0), (4096, 0.0), (50, 0.02)])
def test_sp_topk(k, thr):
    """top-k (sorted, descending) when there are more than k candidates, torch.where order when fewer."""
    from gim_amd import ops
    dev = _dev()
    s = _score_map(3, 64, 96, 4)
    nms = O.mask_borders(O.simple_nms(s, 3), torch.tensor([[96, 64]] * 3), 4)
    kpts, ksc, nv = ops.sp_topk(nms.to(dev), k, thr)
    ref_k, ref_s = O.select_keypoints(nms, thr, k)
    for b in range(3):
        n = len(ref_k[b])
        assert int(nv[b]) == n
        assert torch.equal(kpts[b, :n].cpu(), ref_k[b]), b
        assert torch.equal(ksc[b, :n].cpu(), ref_s[b])
        assert (kpts[b, n:] == 0).all() and (ksc[b, n:] == 0).all()


def test_sp_topk_ties_and_plateau():
    """equal scores: lower flat index first (deterministic); a constant plateau keeps every pixel a candidate"""
    from gim_amd import ops
    dev = _dev()
    nms = torch.zeros(1, 32, 32)
    nms[0, 5:9, 5:9] = 0.5
    nms[0, 20, 3] = 0.7
    kpts, ksc, nv = ops.sp_topk(nms.to(dev), 8, 0.0)
    assert int(nv[0]) == 8
    assert kpts[0, 0].tolist() == [3.0, 20.0] and float(ksc[0, 0]) == pytest.approx(0.7)
    exp = [[5.0 + i, 5.0] for i in range(4)] + [[5.0 + i, 6.0] for i in range(3)]
    assert kpts[0, 1:].tolist() == exp


@pytest.mark.parametrize("dt", DTS)
def test_sp_sample_desc(dt):
    """the dense map in every kind (the 16-bit ld4), both outputs at once: out_f32 against the oracle on the rounded map, out_t = out_f32
    rounded once to the kind, in rows wider than 256 whose padding stays untouched"""
    from gim_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(5)
    B, h, w, K = 2, 8, 12, 70
    dense = torch.randn(B, 256, h, w, generator=g).to(_tdt(dt)).float()
    kp = torch.stack([torch.randint(0, w * 8, (B, K), generator=g), torch.randint(0, h * 8, (B, K), generator=g)], -1).float()
    kp[0, 0] = torch.tensor([0.0, 0.0]); kp[0, 1] = torch.tensor([w * 8 - 1.0, h * 8 - 1.0])   # outside the sample grid
    ref = O.sample_descriptors_legacy(kp.clone(), F.normalize(dense, p=2, dim=1), 8).transpose(-1, -2)
    rows = dense.permute(0, 2, 3, 1).reshape(B * h * w, 256).contiguous().to(_tdt(dt)).to(dev)
    out = torch.empty(B * K, 256, device=dev)
    out_t = torch.full((B * K, 320), 7.0, dtype=_tdt(dt), device=dev)
    ops.sp_sample_desc(rows, kp.to(dev), h, w, out, out_t[:, :256])
    _close(out.view(B, K, 256), ref, 2e-6, "sample_desc")
    assert torch.equal(out_t[:, :256], out.to(_tdt(dt)))
    assert (out_t[:, 256:] == 7.0).all()


# ------------------------------------------------------------------------------------------- LightGlue pieces
def test_posenc_rotary():
    from gim_amd import ops
    dev = _dev()
    _, lg = O.make_state_dicts(0)
    g = torch.Generator().manual_seed(6)
    B, K = 2, 50
    kp = torch.rand(B, K, 2, generator=g) * torch.tensor([640.0, 480.0])
    size = torch.tensor([[640.0, 480.0], [500.0, 480.0]])
    enc_ref = O.fourier_encoding(lg, O.normalize_keypoints(kp, size))            # [2,B,1,K,64]
    enc = ops.lg_posenc(kp.to(dev), size.to(dev), lg["posenc.Wr.weight"].to(dev))
    _close(enc.view(B, K, 64)[..., :32], enc_ref[0, :, 0, :, 0::2], 1e-5, "cos")
    _close(enc.view(B, K, 64)[..., 32:], enc_ref[1, :, 0, :, 0::2], 1e-5, "sin")
    q = torch.randn(B, K, 768, generator=g)
    x = q.view(B * K, 768).clone().to(dev)
    ops.lg_rotary(x, enc, 512)
    ref = q.clone()
    for h in range(8):
        ref[..., h * 64:(h + 1) * 64] = O._rotary(enc_ref[:, :, 0], q[..., h * 64:(h + 1) * 64])
    _close(x.view(B, K, 768), ref, 1e-5, "rotary")
    assert torch.equal(x.view(B, K, 768)[..., 512:].cpu(), q[..., 512:])


@pytest.mark.parametrize("dt", H16)
def test_rotary_16bit(dt):
    """lg_rotary in place on 16-bit rows (ElemIO ld4 / st4) vs the fp64 rotation of the same 16-bit values with the kernel's own fp32
    cos / sin table, rounded ONCE to the kind.  The kernel rounds its fp32 result a second time: it lands on the neighbouring 16-bit value
    only when the exact one lies within the fp32 error (three roundings of 2^-24) of a tie of a grid 2^13 (fp16) / 2^16 (bf16) times
    coarser -- the same formula in torch fp32 on the CPU differs from the once-rounded value in 2.1e-4 (fp16) / 0.8e-4 (bf16) of 51200
    elements, so at most 0.1 % may differ at all, and those by one unit of the kind (inside the 16-bit bar of the file).  Columns
    [512, 768) and, on the row view with ld = 1024, everything outside the view: bit-identical."""
    from gim_amd import ops
    dev = _dev()
    _, lg = O.make_state_dicts(0)
    g = torch.Generator().manual_seed(6)
    B, K = 2, 50
    kp = torch.rand(B, K, 2, generator=g) * torch.tensor([640.0, 480.0])
    size = torch.tensor([[640.0, 480.0], [500.0, 480.0]])
    enc = ops.lg_posenc(kp.to(dev), size.to(dev), lg["posenc.Wr.weight"].to(dev))      # [B*K, 64] = cos | sin, pinned by test_posenc_rotary
    q = torch.randn(B * K, 768, generator=g).to(_tdt(dt))
    t = q.double()[:, :512].reshape(B * K, 8, 32, 2)
    c, s_ = enc.cpu().double()[:, None, :32], enc.cpu().double()[:, None, 32:]
    rot = torch.stack([t[..., 0] * c - t[..., 1] * s_, t[..., 1] * c + t[..., 0] * s_], -1).reshape(B * K, 512)
    ref = torch.cat([rot.to(_tdt(dt)), q[:, 512:]], 1)
    x = q.clone().to(dev)
    ops.lg_rotary(x, enc, 512)
    wide = torch.full((B * K, 1024), 7.0, dtype=_tdt(dt), device=dev)
    wide[:, 128:896] = q.to(dev)
    ops.lg_rotary(wide[:, 128:896], enc, 512)
    for got, what in ((x.cpu(), f"rotary {dt}"), (wide[:, 128:896].cpu(), f"rotary {dt} ld=1024")):
        _close(got[:, :512], ref[:, :512], _tol(dt), what)
        differ = (got[:, :512] != ref[:, :512]).float().mean().item()
        print(f"[differ] {what}: {differ:.2e} of the elements are not the once-rounded value")
        assert differ <= 1e-3, (what, differ)
        assert torch.equal(got[:, 512:], q[:, 512:])
    assert (wide[:, :128] == 7.0).all() and (wide[:, 896:] == 7.0).all()


@pytest.mark.parametrize("dt", DTS)
def test_transpose_and_cast(dt):
    from gim_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(7)
    nb, S, C = 3, 100, 256
    Sp = 128
    src = torch.randn(nb * S, 768, generator=g).to(_tdt(dt))
    dst = torch.full((nb, C, Sp), 7.0, dtype=_tdt(dt), device=dev)
    ops.lg_transpose(src.to(dev)[:, 512:], dst, nb, S, Sp, C)
    ref = torch.zeros(nb, C, Sp)
    ref[:, :, :S] = src.float()[:, 512:].reshape(nb, S, C).transpose(1, 2)
    assert torch.equal(dst.float().cpu(), ref)
    x = torch.randn(40, 256, generator=g)
    out = torch.empty(40, 512, dtype=_tdt(dt), device=dev)
    ops.cast_rows(x.to(dev), out[:, :256])
    assert torch.equal(out[:, :256].float().cpu(), x.to(_tdt(dt)).float())


def _rnd(x, dt):
    return x if dt == "fp32" else x.to(_tdt(dt)).double()


def _attention64(qq, kk, vv, D, dt_in="fp32", dt_out="fp32"):
    """softmax(q k^T / sqrt(D)) v in fp64 on [..., L / S, D] operands.  With the defaults: the exact result.  With kinds: the roundings
    of the kernel ON TOP of it -- 16-bit operands make it round P to their kind for the second MFMA (the row sum keeps the unrounded
    P), a 16-bit output is rounded once -- i.e. what a kernel without any error of its own returns."""
    sc = qq @ kk.transpose(-1, -2) / math.sqrt(D)
    p = torch.exp(sc - sc.amax(-1, keepdim=True))
    return _rnd(_rnd(p, dt_in) @ vv / p.sum(-1, keepdim=True), dt_out)


def _sdpa_tol(dt_in, dt_out):
    """1e-5 of scale between fp32 operands and an fp32 output, else the 16-bit bar of the 16-bit kind involved"""
    return _t16(dt_in if dt_in != "fp32" else dt_out, 6.5e-3, 1e-5)


def _sdpa_check(out, qq, kk, vv, D, dt_in, dt_out, what):
    """out rows [nb*L, H*D] vs the fp64 attention of qq / kk / vv [nb, H, L / S, D] (fp64 copies of the kernel's operands); the
    emulated roundings alone must stay below HALF the bar, so that a change of inputs cannot quietly eat the margin for real errors"""
    nb, H, L, _ = qq.shape
    ref = _attention64(qq, kk, vv, D)
    tol = _sdpa_tol(dt_in, dt_out)
    if (dt_in, dt_out) != ("fp32", "fp32"):
        emu = (_attention64(qq, kk, vv, D, dt_in, dt_out) - ref).abs().max().item() / ref.abs().max().item()
        print(f"[emulated] {what}: roundings alone {emu:.3e} of scale (half the bar: {tol / 2:g})")
        assert emu < tol / 2, (what, emu, tol)
    _close(out, ref.transpose(1, 2).reshape(nb * L, H * D).float(), tol, what)


def _heads(x, nb, n, H, D, shift=0):
    """rows [nb*n, H*D] -> fp64 [nb, H, n, D], sequences rolled the way kv_shift pairs them"""
    return x.double().reshape(nb, n, H, D).transpose(1, 2).roll(-shift, 0)


def _sdpa_run(q, k, v, nb, H, D, L, S, dt_out, shift=0, ld=None, extra_rows=3):
    """q [nb*L, H*D], k / v [nb*S, H*D]: CPU tensors of the operand kind.  V^T goes into a buffer of NaNs (the padding keys must be
    zeros lg_transpose wrote), q / k / out are column windows of buffers with row strides `ld` (default: H*D + 64), out's buffer is
    `extra_rows` longer: everything of it outside the window must keep its sentinel.  -> out [nb*L, H*D] on the device"""
    from gim_amd import ops
    dev = _dev()
    C = H * D
    Sp = (S + 63) // 64 * 64
    vt = torch.full((nb, C, Sp), float("nan"), dtype=q.dtype, device=dev)
    ops.lg_transpose(v.to(dev), vt, nb, S, Sp, C)
    views = []
    for t, w, fill, rows in ((q, (ld or (C + 64,) * 3)[0], 0.0, nb * L), (k, (ld or (C + 64,) * 3)[1], 0.0, nb * S),
                             (None, (ld or (C + 64,) * 3)[2], 7.0, nb * L + extra_rows)):
        buf = torch.full((rows, w), fill, dtype=_tdt(dt_out) if t is None else t.dtype, device=dev)
        off = (w - C) // 2 // 8 * 8
        if t is not None:
            buf[:, off:off + C] = t.to(dev)
        views.append((buf, off))
    (qb, qo), (kb, ko), (ob, oo) = views
    out = ob[:nb * L, oo:oo + C]
    ops.sdpa(qb[:, qo:qo + C], kb[:, ko:ko + C], vt, out, nb, H, L, S, Sp, kv_shift=shift, D=D)
    rest = ob.clone()
    rest[:nb * L, oo:oo + C] = 7.0
    assert (rest == 7.0).all(), "sdpa wrote outside its nb*L rows / H*D columns"
    return out


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("L,S,cross", [(128, 128, False), (100, 77, True), (300, 2048, True), (2048, 2048, False), (1, 5, True)])
def test_sdpa(dt, L, S, cross):
    """flash SDPA vs softmax(q k^T / 8) v in fp64 on the kernel's operand precision"""
    from gim_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(8)
    nb, H = 2, 4
    tdt = _tdt(dt)
    q = torch.randn(nb * L, 768, generator=g).to(tdt)
    kv = torch.randn(nb * S, 768, generator=g).to(tdt)
    kv[:, 256:512] *= 2.0          # sharper softmax
    Sp = (S + 63) // 64 * 64
    vt = torch.empty(nb, 256, Sp, dtype=tdt, device=dev)
    kvd = kv.to(dev)
    ops.lg_transpose(kvd[:, 512:], vt, nb, S, Sp, 256)
    out = torch.empty(nb * L, 256, dtype=tdt, device=dev)
    shift = 1 if cross else 0
    ops.sdpa(q.to(dev)[:, :256], kvd[:, 256:512], vt, out, nb, H, L, S, Sp, kv_shift=shift)
    qq = q.double()[:, :256].reshape(nb, L, H, 64).transpose(1, 2)
    kk = kv.double()[:, 256:512].reshape(nb, S, H, 64).transpose(1, 2).roll(-shift, 0)
    vv = kv.double()[:, 512:].reshape(nb, S, H, 64).transpose(1, 2).roll(-shift, 0)
    ref = (torch.softmax(qq @ kk.transpose(-1, -2) / 8.0, -1) @ vv).transpose(1, 2).reshape(nb * L, 256)
    _close(out, ref.float(), _t16(dt, 6.5e-3, 1e-5), f"sdpa L={L} S={S}")
    if dt != "fp32":   # the fp16 bar leaves the kernel half of itself: the roundings of an error-free kernel stay below the other half
        emu = (_attention64(qq, kk, vv, 64, dt, dt).transpose(1, 2).reshape(nb * L, 256) - ref).abs().max().item() / ref.abs().max().item()
        print(f"[emulated] sdpa {dt} L={L} S={S}: roundings alone {emu:.3e} of scale")
        # (bf16: printed only -- its bar is 2 x the MEASURED error, and at 2048 x 2048 the emulation sits at 3.24e-3, half of it)
        assert dt == "bf16" or emu < _t16(dt, 6.5e-3, 1e-5) / 2, emu


def _qkv(nb, L, S, C, dt, seed, ksharp=2.0):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(nb * L, C, generator=g).to(_tdt(dt))
    k = (ksharp * torch.randn(nb * S, C, generator=g)).to(_tdt(dt))
    v = torch.randn(nb * S, C, generator=g).to(_tdt(dt))
    return q, k, v


@pytest.mark.parametrize("D,L,S", [(64, 100, 77), (128, 80, 80)])
@pytest.mark.parametrize("dt_in,dt_out", [("fp16", "fp32"), ("bf16", "fp32"), ("fp32", "fp16"), ("fp32", "bf16")])
def test_sdpa_mixed_kinds(dt_in, dt_out, D, L, S):
    """launch_sdpa<true, false, D> (16-bit operands, fp32 output) and <false, true, D> (fp32 operands and MFMA, 16-bit output), in the
    flavour the 16-bit tag routes to"""
    nb, H = 2, 256 // D
    q, k, v = _qkv(nb, L, S, H * D, dt_in, 14, 2.0 if D == 64 else 1.5)
    out = _sdpa_run(q, k, v, nb, H, D, L, S, dt_out)
    assert out.dtype == _tdt(dt_out)
    _sdpa_check(out, _heads(q, nb, L, H, D), _heads(k, nb, S, H, D), _heads(v, nb, S, H, D), D, dt_in, dt_out,
                f"sdpa {dt_in}->{dt_out} D={D}")


@pytest.mark.parametrize("dt", ["fp32", "fp16"])
@pytest.mark.parametrize("L,S", [(128, 64), (129, 65), (127, 63), (256, 128), (1, 1)])
def test_sdpa_tile_edges(dt, L, S):
    """L on / one past / one short of the 128-query workgroup tile, S of the 64-key tile; the padding keys of V^T are the zeros of
    lg_transpose (the buffer held NaNs), the rows behind nb*L and the columns beside H*D keep their sentinel (_sdpa_run)"""
    nb, H, D = 2, 2, 64
    q, k, v = _qkv(nb, L, S, H * D, dt, 15)
    out = _sdpa_run(q, k, v, nb, H, D, L, S, dt, shift=1)
    _sdpa_check(out, _heads(q, nb, L, H, D), _heads(k, nb, S, H, D, 1), _heads(v, nb, S, H, D, 1), D, dt, dt, f"sdpa {dt} edge L={L} S={S}")


@pytest.mark.parametrize("dt", ["fp32", "fp16"])
@pytest.mark.parametrize("shift", [1, 2])
def test_sdpa_kv_shift_wraps(dt, shift):
    """sequence s attends to sequence (s + kv_shift) % nb: nb = 3, so that both shifts wrap at a different sequence"""
    nb, H, D, L, S = 3, 4, 64, 100, 77
    q, k, v = _qkv(nb, L, S, H * D, dt, 16)
    out = _sdpa_run(q, k, v, nb, H, D, L, S, dt, shift=shift)
    _sdpa_check(out, _heads(q, nb, L, H, D), _heads(k, nb, S, H, D, shift), _heads(v, nb, S, H, D, shift), D, dt, dt,
                f"sdpa {dt} nb=3 kv_shift={shift}")


@pytest.mark.parametrize("dt", ["fp32", "fp16"])
def test_sdpa_strides_and_16_heads(dt):
    """q, k and out in three buffers with three row strides (1536 / 1280 / 1096), 16 heads of 64: DINOv2's geometry"""
    nb, H, D, L, S = 1, 16, 64, 70, 130
    q, k, v = _qkv(nb, L, S, H * D, dt, 17)
    out = _sdpa_run(q, k, v, nb, H, D, L, S, dt, ld=(1536, 1280, 1096))
    assert (out.stride(0), out.shape) == (1096, (L, 1024))
    _sdpa_check(out, _heads(q, nb, L, H, D), _heads(k, nb, S, H, D), _heads(v, nb, S, H, D), D, dt, dt, f"sdpa {dt} H=16 strided")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("planted", [195, 70])
def test_sdpa_late_maximum(dt, planted):
    """the online-softmax rescale: one key per head beats every other score of every query by more than 20 (after the 1 / sqrt(D)
    scale), and it arrives in the LAST tile, which holds 8 valid keys of 64 (key 195 of 200: the rescale branch next to the -inf
    masking), or in tile 1 of 4 (key 70).  Everything accumulated before it must shrink by exp(-20) or more: a rescale that is
    skipped, or applied to one half of the lanes only, leaves the output orders of magnitude away from v[planted]."""
    nb, H, D, L, S = 1, 4, 64, 130, 200
    g = torch.Generator().manual_seed(18)
    u = F.normalize(torch.randn(H, D, generator=g), dim=-1)                       # one direction per head
    q = (torch.randn(L, H, D, generator=g) + 24.0 * u).reshape(L, H * D).to(_tdt(dt))
    k = torch.randn(S, H, D, generator=g)
    k[:192] *= 0.25
    k[planted] = 16.0 * u
    k = k.reshape(S, H * D).to(_tdt(dt))
    v = torch.randn(S, H * D, generator=g).to(_tdt(dt))
    qq, kk, vv = _heads(q, nb, L, H, D), _heads(k, nb, S, H, D), _heads(v, nb, S, H, D)
    sc = qq @ kk.transpose(-1, -2) / 8.0
    others = sc.clone()
    others[..., planted] = -math.inf
    margin = (sc[..., planted] - others.amax(-1)).min().item()
    assert margin > 20.0, margin
    out = _sdpa_run(q, k, v, nb, H, D, L, S, dt)
    _sdpa_check(out, qq, kk, vv, D, dt, dt, f"sdpa {dt} late maximum at key {planted} (margin {margin:.1f})")


def test_sdpa_refuses_two_16bit_kinds():
    """fp16 operands with a bf16 output: refused in Python before any launch (the library refuses the tags too: GIM_ROUTE_ANY2,
    tests/test_dtype_dispatch_cpu.py); out keeps its sentinel"""
    from gim_amd import ops
    dev = _dev()
    nb, H, L, S, Sp = 1, 4, 8, 8, 64
    q = torch.randn(nb * L, 256, dtype=torch.float16, device=dev)
    vt = torch.zeros(nb, 256, Sp, dtype=torch.float16, device=dev)
    out = torch.full((nb * L, 256), 7.0, dtype=torch.bfloat16, device=dev)
    with pytest.raises(AssertionError):
        ops.sdpa(q, q, vt, out, nb, H, L, S, Sp)
    torch.cuda.synchronize()
    assert (out == 7.0).all()


@pytest.mark.parametrize("dt", DTS)
def test_layernorm_gelu(dt):
    from gim_amd import ops
    from gim_amd._lib import ACT_GELU, ACT_NONE
    dev = _dev()
    g = torch.Generator().manual_seed(9)
    x = 2 * torch.randn(77, 512, generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(512, generator=g), 0.1 * torch.randn(512, generator=g)
    for act in (ACT_GELU, ACT_NONE):
        out = torch.empty(77, 512, dtype=_tdt(dt), device=dev)
        ops.layernorm_act(x.to(dev), gamma.to(dev), beta.to(dev), out, act)
        ref = F.layer_norm(x, (512,), gamma, beta)
        ref = F.gelu(ref) if act == ACT_GELU else ref
        _close(out, ref, _t16(dt, 5e-3, 2e-6), "layernorm_act")


def _assign_inputs(B, M, N, seed):
    _, lg = O.make_state_dicts(0)
    g = torch.Generator().manual_seed(seed)
    d0 = torch.randn(B, M, 256, generator=g)
    d1 = torch.randn(B, N, 256, generator=g)
    nm = min(M, N) // 2
    for b in range(B):   # plant correspondences so that many rows have a confident mutual match
        perm = torch.randperm(N, generator=g)[:nm]
        d1[b, perm] = d0[b, :nm] + 0.05 * torch.randn(nm, 256, generator=g)
    return lg, d0, d1


@pytest.mark.parametrize("B,M,N", [(2, 128, 128), (1, 300, 170), (2, 2048, 2048)])
def test_lg_assign(B, M, N):
    """fused assignment vs oracle log_assignment + filter_matches: indices exact, scores 1e-5, lazy matrix 2e-5"""
    from gim_amd import ops
    dev = _dev()
    lg, d0, d1 = _assign_inputs(B, M, N, 10)
    i = 8
    p = f"log_assignment.{i}"
    lg[p + ".final_proj.weight"] = lg[p + ".final_proj.weight"] * 0.1      # keep exp() in range for random descriptors
    scores, _ = O.log_assignment(lg, i, d0, d1)
    m0, m1, ms0, ms1 = O.filter_matches(scores, 0.1)
    md0 = F.linear(d0, lg[p + ".final_proj.weight"], lg[p + ".final_proj.bias"])
    md1 = F.linear(d1, lg[p + ".final_proj.weight"], lg[p + ".final_proj.bias"])
    r = ops.lg_assign(d0.to(dev), d1.to(dev), md0.to(dev).contiguous(), md1.to(dev).contiguous(),
                      lg[p + ".matchability.weight"].reshape(-1).to(dev), lg[p + ".matchability.bias"].to(dev), 0.1)
    assert (m0 > -1).sum() > B * min(M, N) // 8, "test inputs must be match-rich"
    assert torch.equal(r.matches0.cpu(), m0) and torch.equal(r.matches1.cpu(), m1)
    _close(r.mscores0, ms0, 2e-5, "mscores0")
    _close(r.mscores1, ms1, 2e-5, "mscores1")
    assert r.count.tolist() == [(m0[b] > -1).sum().item() for b in range(B)]
    la = ops.lg_log_assignment(r)
    _close(la, scores, 2e-5, "log_assignment")
    total = sum(r.count.tolist())
    kp0, kp1 = torch.rand(B, M, 2) * 600, torch.rand(B, N, 2) * 600
    sc0, sc1 = torch.tensor([[1.5, 2.0]] * B), torch.tensor([[0.5, 1.25]] * B)
    matches, sc, mk0, mk1, bids = ops.lg_emit_matches(r, total, kp0.to(dev), kp1.to(dev), sc0.to(dev), sc1.to(dev))
    exp_m = torch.cat([torch.stack([torch.where(m0[b] > -1)[0], m0[b][m0[b] > -1]], -1) for b in range(B)])
    assert torch.equal(matches.cpu(), exp_m)
    exp_b = torch.cat([torch.full(((m0[b] > -1).sum().item(),), b) for b in range(B)])
    assert torch.equal(bids.cpu(), exp_b)
    exp0 = torch.cat([kp0[b][torch.where(m0[b] > -1)[0]] * sc0[b] for b in range(B)])
    exp1 = torch.cat([kp1[b][m0[b][m0[b] > -1]] * sc1[b] for b in range(B)])
    assert torch.equal(mk0.cpu(), exp0) and torch.equal(mk1.cpu(), exp1)
    _close(sc, torch.cat([ms0[b][m0[b] > -1] for b in range(B)]), 2e-5, "scores list")


# ------------------------------------------------------------------------------------------- whole modules
def _models(precision, K):
    from gim_amd.lightglue import LightGlue, SuperPoint
    sp_sd, lg_sd = O.make_state_dicts(0)
    det = SuperPoint({"max_num_keypoints": K, "force_num_keypoints": True, "detection_threshold": 0.0, "nms_radius": 3,
                      "trainable": False, "precision": precision})
    lg = LightGlue({"filter_threshold": 0.1, "flash": False, "checkpointed": True, "precision": precision})
    det.load_state_dict(sp_sd)
    lg.load_state_dict(lg_sd)
    return det.eval(), lg.eval(), sp_sd, lg_sd


def test_superpoint_golden_fp32(golden_dir):
    """engine (fp32 mode) vs the reference's own SuperPoint outputs"""
    g = np.load(os.path.join(golden_dir, "lg_superpoint.npz"))
    det, _, _, _ = _models("fp32", int(g["K"]))
    b, h, w = (int(v) for v in g["shape"])
    img = O.seeded_gray(b, h, w, int(g["seed"]))
    out = det({"image": img.to(_dev())})
    _close(det._debug["scores"], torch.as_tensor(g["dense_scores"]), 2e-5, "dense scores")
    kp, ref = out["keypoints"].cpu(), torch.as_tensor(g["keypoints"])
    same = (kp == ref).all(-1).float().mean().item()
    # keypoint order is a sort on fp32 scores that agree to ~1e-7 relative: allow a handful of swaps
    assert same >= 0.97, same
    for i in range(b):
        a = set(map(tuple, kp[i].tolist())); r = set(map(tuple, ref[i].tolist()))
        assert len(a & r) >= 0.98 * len(r)
    keep = (kp == ref).all(-1)
    _close(out["descriptors"].cpu()[keep], torch.as_tensor(g["descriptors"])[keep], 5e-5, "descriptors")


def test_superpoint_rgb_and_bf16(golden_dir):
    g = np.load(os.path.join(golden_dir, "lg_superpoint_rgb.npz"))
    det, _, _, _ = _models("fp32", 32)
    rgb = torch.rand(1, 3, 64, 96, generator=torch.Generator().manual_seed(int(g["seed"])))
    out = det({"image": rgb.to(_dev())})
    kp, ref = out["keypoints"].cpu(), torch.as_tensor(g["keypoints"])
    assert (kp == ref).all(-1).float().mean().item() >= 0.9
    det16, _, _, _ = _models("bf16", 32)
    out16 = det16({"image": rgb.to(_dev())})
    assert out16["keypoints"].shape == (1, 32, 2) and torch.isfinite(out16["descriptors"]).all()
    _close(det16._debug["scores"], det._debug["scores"], 0.1, "bf16 score map")


def test_superpoint_few_keypoints_padding():
    """fewer candidates than K: found points first (torch.where order), the rest uniform random inside their
    bounding box, zero scores (pad_and_stack 'random_c', misc.py:44-55)"""
    det, _, _, _ = _models("fp32", 2048)
    img = O.seeded_gray(1, 64, 96, 3)
    out = det({"image": img.to(_dev())})
    n = det._debug["nvalid"][0]
    assert 0 < n < 2048 and out["keypoints"].shape == (1, 2048, 2)
    found = out["keypoints"][0, :n].cpu() - 0.5
    flat = found[:, 1] * 96 + found[:, 0]
    assert (flat[1:] > flat[:-1]).all()                        # torch.where order
    pad = out["keypoints"][0, n:].cpu() - 0.5
    assert (pad[:, 0] >= found[:, 0].min()).all() and (pad[:, 0] <= found[:, 0].max()).all()
    assert (det._debug["keypoint_scores"][0, n:] == 0).all()
    assert torch.isfinite(out["descriptors"]).all()


def test_lightglue_golden_fp32(golden_dir):
    """engine (fp32 mode) vs the reference's own LightGlue outputs on planted descriptors: indices exact"""
    g = np.load(os.path.join(golden_dir, "lg_lightglue.npz"))
    _, lg, _, _ = _models("fp32", 128)
    dev = _dev()
    kp0, d0, kp1, d1 = O.planted_descriptors(2, int(g["K"]), seed=int(g["seed"]))
    rs = torch.tensor([[480, 640], [480, 640]])
    pred = lg({"keypoints0": kp0.to(dev), "keypoints1": kp1.to(dev), "descriptors0": d0.to(dev), "descriptors1": d1.to(dev),
               "resize0": rs.to(dev), "resize1": rs.to(dev)})
    _close(pred["ref_descriptors0"][:, 0], torch.as_tensor(g["ref_descriptors0"]), 1e-4, "ref_descriptors0")
    _close(pred["ref_descriptors1"][:, 0], torch.as_tensor(g["ref_descriptors1"]), 1e-4, "ref_descriptors1")
    assert np.array_equal(pred["matches0"].cpu().numpy(), g["matches0"])
    assert np.array_equal(pred["matches1"].cpu().numpy(), g["matches1"])
    _close(pred["matching_scores0"], torch.as_tensor(g["matching_scores0"]), 5e-3, "matching_scores0")
    _close(pred["log_assignment"].get(), torch.as_tensor(g["log_assignment"]), 2e-4, "log_assignment")
    assert pred["stop"] == 9 and len(pred["matches"]) == 2
    for b in range(2):
        m = g["matches0"][b]
        exp = np.stack([np.nonzero(m > -1)[0], m[m > -1]], -1)
        assert np.array_equal(pred["matches"][b].cpu().numpy(), exp)
    assert pred["prune0"].shape == (2, 128) and float(pred["prune0"][0, 0]) == 9.0


def test_lightglue_unequal_counts_and_bf16():
    """M != N (the stacked row block handles both sets), bf16 mode agrees with the fp32 oracle on most matches"""
    _, lg_sd = O.make_state_dicts(0)
    dev = _dev()
    kp0, d0, kp1, d1 = O.planted_descriptors(1, 192, seed=33)
    kp1, d1 = kp1[:, :150].contiguous(), d1[:, :150].contiguous()
    rs = torch.tensor([[480, 640]])
    data = {"keypoints0": kp0, "keypoints1": kp1, "descriptors0": d0, "descriptors1": d1, "resize0": rs, "resize1": rs}
    ref = O.lightglue_forward(lg_sd, data)
    for prec, need in (("fp32", 1.0), ("bf16", 0.985), ("fp16", 0.99)):   # bf16 measured 0.9948 (one of 192 keypoints differs): 2 x the disagreement; fp16: round 5
        _, lg, _, _ = _models(prec, 128)
        pred = lg({k: v.to(dev) for k, v in data.items()})
        agree = (pred["matches0"].cpu() == ref["matches0"]).float().mean().item()
        print(f"[agree] lightglue {prec} matches0 agreement with the fp32 oracle: {agree:.4f}")
        assert agree >= need, (prec, agree)
        assert pred["matches1"].shape == (1, 150)
    assert (ref["matches0"] > -1).sum() > 50


def test_e2e_pipeline_golden(golden_dir):
    """detector + matcher + adapter (trainer/lightning.py:161-193) vs the golden run of the reference modules"""
    from gim_amd.lightglue import gim_lightglue_inference
    g = np.load(os.path.join(golden_dir, "lg_e2e.npz"))
    det, lg, _, _ = _models("fp32", int(g["K"]))
    dev = _dev()
    img0 = O.seeded_gray(2, 96, 128, int(g["seeds"][0]))
    img1 = torch.roll(img0, shifts=tuple(int(x) for x in g["shift"]), dims=(2, 3)).contiguous()
    rs = torch.tensor([[96, 128], [96, 128]])
    scale = torch.as_tensor(g["scale"])
    data = {"image0": img0.to(dev), "image1": img1.to(dev), "resize0": rs.to(dev), "resize1": rs.to(dev),
            "scale0": scale.to(dev), "scale1": scale.to(dev)}
    pred = gim_lightglue_inference(det, lg, data)
    for k in ("hw0_i", "hw1_i", "mkpts0_f", "mkpts1_f", "m_bids", "mconf"):
        assert k in data
    assert tuple(data["hw0_i"]) == (96, 128)
    same0 = (pred["keypoints0"].cpu() == torch.as_tensor(g["keypoints0"])).all(-1).float().mean().item()
    assert same0 >= 0.95
    # the adapter outputs are consistent with the engine's own matches (exact gather + scale)
    m0 = pred["matches0"].cpu()
    exp0 = torch.cat([pred["keypoints0"][b].cpu()[m0[b] > -1] * scale[b] for b in range(2)])
    exp1 = torch.cat([pred["keypoints1"][b].cpu()[m0[b][m0[b] > -1]] * scale[b] for b in range(2)])
    assert torch.equal(data["mkpts0_f"].cpu(), exp0) and torch.equal(data["mkpts1_f"].cpu(), exp1)
    assert torch.equal(data["m_bids"].cpu(), torch.cat([torch.full(((m0[b] > -1).sum().item(),), b) for b in range(2)]))
    assert data["mconf"].shape[0] == exp0.shape[0]
    if same0 == 1.0 and (pred["keypoints1"].cpu() == torch.as_tensor(g["keypoints1"])).all():
        assert np.array_equal(m0.numpy(), g["matches0"])
        _close(data["mkpts0_f"], torch.as_tensor(g["mkpts0_f"]), 1e-6, "mkpts0_f")


def test_no_cpu_fallback():
    from gim_amd._lib import GimHipError
    det, lg, _, _ = _models("fp32", 32)
    with pytest.raises(GimHipError):
        det({"image": torch.rand(1, 1, 64, 64)})
    with pytest.raises(GimHipError):
        lg({"keypoints0": torch.rand(1, 8, 2), "keypoints1": torch.rand(1, 8, 2), "descriptors0": torch.rand(1, 8, 256),
            "descriptors1": torch.rand(1, 8, 256), "resize0": torch.tensor([[480, 640]]), "resize1": torch.tensor([[480, 640]])})
