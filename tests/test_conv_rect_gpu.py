"""Rectangular filters (R != S) and non-square images (H != W) through every conv kernel family,
against float64 ``F.conv2d`` and its autograd per MC group (16-bit: on the same 16-bit-rounded
operands).  Every entry point carries R, S and H, W separately through its tap decomposition,
stage count, parity classes and slab layout; a transposition in any of them fails here.

Kernel serving each case, read from the launch predicates (conv_gemm.hip, conv_split.hip,
conv_gemm16.hip, conv_pipe16.hip); cases are numbered from 1 in CASES' order:

fp32, f32_math = "exact": conv_gemm_f32 (f32 MFMA) for forward, data and weight gradient of
every case (vector loaders where Cin % 32 / K % 4 / Cout % 32 / Cin % 4 allow, else scalar).
fp32, f32_math = "split" (the default):
  forward        cases 1-5, 9-14: conv_split_f32 (pipelined; its short-K form where M, N > 64
                 and K <= 256); case 15: conv_split_f32's stem form (Cin == 4, N == 64);
                 cases 6-8, 16, 17 (Cin % 32 != 0): conv_gemm_f32 with register-staged planes
  data gradient  cases 1-15: conv_split_f32, one launch per parity class (LDS-staged epilogue for
                 the addend); cases 16, 17 (Cout % 32 != 0): conv_gemm_f32
  weight grad.   cases 1-15: conv_split_f32; cases 16, 17 (Cout or Cin % 4 != 0): conv_gemm_f32
bf16 / f16 (cases 1-14):
  forward        cases 6, 7: conv_pipe16's stem form (Cin == 8, S <= 8); cases 5 (Cin = 96) and 8
                 (Cin == 8, S = 9: the stem form declines): conv_gemm_h16 (register-staged);
                 all others: conv_pipe16 (the halo, chunked-halo, expand and 256-row kernels
                 decline: none is 3x3 / stride 1 / pad 1 or 1x1 / stride 1 / pad 0)
  data gradient  case 5 (Cout = 96): conv_gemm_h16; all others: conv_pipe16
  weight grad.   conv_pipe16 for every case

Largest measured error over bar on an MI355X (this file, all cases):
  fp32 split bar (2 x exact error + 2^-24 max|ref|)   y 0.55 (c3)  dx 0.53 (c15)  dW 0.55 (c9)
  fp32 exact bar (1e-4 max|ref| + 1e-5)               y 0.016  dx 0.007  dW 0.004
  16-bit forward (2 ulp)         bf16 0.35 (c7)   f16 0.41 (c2)
  16-bit data gradient (4 ulp)   bf16 0.21 (c3)   f16 0.19 (c7)
  16-bit slabs (1e-4)            bf16 0.001       f16 0.002
  BN on load: y as above (0.27), slabs, mean and variance <= 0.005 of their bars in every type;
  BN-backward partials <= 0.002 of 1e-4 max + 1e-3
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

dev = "cuda"
ULP32 = 2.0 ** -24
ULP = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
H16 = [torch.bfloat16, torch.float16]
DT_IDS = {torch.float32: "fp32", torch.bfloat16: "bf16", torch.float16: "f16"}

CASES = [
    # G, B, H, W, Cin, Cout, R, S, stride, pad
    (2, 2, 7, 10, 64, 64, 1, 3, 1, 1),      # 1: 1x3, output taller than input (9 x 10)
    (2, 2, 9, 6, 64, 128, 3, 1, 1, 1),      # 2: 3x1 (9 x 8)
    (1, 3, 9, 11, 128, 64, 3, 5, 2, 2),     # 3: stride 2: parity classes with nr != ns
    (2, 2, 8, 11, 64, 64, 2, 3, 2, 1),      # 4: even filter side, stride 2
    (1, 2, 6, 9, 96, 96, 5, 3, 1, 1),       # 5: Cin, Cout % 64 != 0: register-staged 16-bit
    (2, 2, 8, 5, 8, 64, 1, 7, 1, 3),        # 6: 16-bit stem form with R = 1 (14 x 5)
    (1, 2, 9, 6, 8, 64, 7, 2, 2, 1),        # 7: the same form, 7 filter rows of 2 taps
    (1, 2, 4, 12, 8, 64, 1, 9, 1, 4),       # 8: S = 9 > 8: the stem form must decline
    (2, 3, 9, 13, 64, 128, 3, 3, 2, 1),     # 9: square filter, H != W, ragged tiles, odd extents
    (1, 2, 5, 12, 256, 512, 1, 1, 2, 0),    # 10: strided 1x1, H != W, tapless parity classes
    (1, 2, 6, 7, 64, 64, 1, 1, 1, 1),       # 11: pad > R/2: border outputs are zero
    (2, 2, 8, 9, 64, 64, 3, 3, 1, 0),       # 12: pad = 0 under a 3x3
    (1, 1, 1, 17, 64, 64, 1, 3, 1, 1),      # 13: one-row image (3 x 17)
    (1, 4, 12, 20, 64, 64, 3, 1, 1, 1),     # 14: split-K slabs (wgrad_splits >= 2)
    (2, 2, 7, 6, 4, 64, 5, 2, 1, 2),        # 15: fp32 split stem form, nt = R*ceil(S/4)
    (1, 2, 5, 7, 3, 10, 2, 3, 1, 0),        # 16: fp32: K % 4 != 0, fully scalar tiles
    (1, 2, 6, 5, 6, 12, 3, 2, 2, 1),        # 17: fp32: Cin % 4 != 0 with stride 2
]
# Ho x Wo of each case (F.conv2d's, listed so a wrong extent in the table fails loudly)
OUT_HW = [(9, 10), (9, 8), (6, 6), (5, 6), (4, 9), (14, 5), (3, 4), (12, 12), (5, 7), (3, 6),
          (8, 9), (6, 7), (3, 17), (12, 22), (7, 9), (4, 5), (3, 3)]
N16 = 14    # the 16-bit tests run the first 14 (Cin, Cout % 8 == 0, Cout % 32 == 0)
IDS = [f"c{i + 1}" for i in range(len(CASES))]


@pytest.fixture
def f32_math():
    from mauv import ops
    prev = ops.f32_math()
    yield ops.set_f32_math
    ops.set_f32_math(prev)


def _ref_all(x, w, dy, st, pad):
    """float64 (y, dx, dW) per MC group: x [G,B,H,W,Cin], w [G,Cout,R,S,Cin], dy [G,B,Ho,Wo,Cout];
    padding=pad on both axes."""
    ys, dxs, dws = [], [], []
    for g in range(w.shape[0]):
        xg = x[g].permute(0, 3, 1, 2).double().requires_grad_(True)
        wg = w[g].permute(0, 3, 1, 2).double().requires_grad_(True)
        yg = F.conv2d(xg, wg, stride=st, padding=pad)
        yg.backward(dy[g].permute(0, 3, 1, 2).double())
        ys.append(yg.detach().permute(0, 2, 3, 1))
        dxs.append(xg.grad.permute(0, 2, 3, 1))
        dws.append(wg.grad.permute(0, 2, 3, 1))
    return torch.stack(ys), torch.stack(dxs), torch.stack(dws)


_DATA = {}


def _data(i, dt):
    """Operands of case i rounded to dt, and their float64 references; computed once per
    (case, dtype), shared by every test and never modified."""
    if (i, dt) not in _DATA:
        from mauv import ops
        G, B, H, W, Cin, Cout, R, S, st, pad = CASES[i]
        Ho, Wo = ops.out_hw(H, R, st, pad), ops.out_hw(W, S, st, pad)
        assert (Ho, Wo) == OUT_HW[i]
        gen = torch.Generator().manual_seed(1000 + i)
        x = torch.randn(G, B, H, W, Cin, generator=gen).to(dt)
        w = (torch.randn(G, Cout, R, S, Cin, generator=gen) / math.sqrt(R * S * Cin)).to(dt)
        dy = torch.randn(G, B, Ho, Wo, Cout, generator=gen).to(dt)
        addend = torch.randn(G, B, H, W, Cin, generator=gen).to(dt)
        y_ref, dx_ref, dw_ref = _ref_all(x, w, dy, st, pad)
        assert tuple(y_ref.shape) == (G, B, Ho, Wo, Cout)
        _DATA[i, dt] = dict(x=x, w=w, dy=dy, addend=addend, Ho=Ho, Wo=Wo, y=y_ref,
                            dx=dx_ref + addend.double(), dw=dw_ref)
    return _DATA[i, dt]


def _nan(*shape, dt=torch.float32):
    return torch.full(shape, float("nan"), device=dev, dtype=dt)


def _err(got, ref):
    """(max |got - ref|, max |ref|) in float64; an unwritten (NaN) output is an infinite error."""
    d = (got.detach().double().cpu() - ref).abs().max().item()
    return (d if d == d else float("inf")), ref.abs().max().item()


def _bar(label, err, lim):
    print(f"{label}: err {err:.3e} bar {lim:.3e} ratio {err / lim if lim else float('nan'):.3f}")
    assert err <= lim, f"{label}: max err {err:.3e} > {lim:.3e}"


def _close(label, got, ref, rtol, atol=0.0):
    e, scale = _err(got, ref)
    _bar(label, e, atol + rtol * scale)


def _run(i, dt, addend=True):
    """Forward, data gradient (+ addend) and weight-gradient slabs of case i on the GPU; every
    output is NaN before its kernel runs."""
    from mauv import ops
    G, B, H, W, Cin, Cout, R, S, st, pad = CASES[i]
    d = _data(i, dt)
    Ho, Wo = d["Ho"], d["Wo"]
    x, w, dy = d["x"].to(dev), d["w"].to(dev), d["dy"].to(dev)
    y = _nan(G, B, Ho, Wo, Cout, dt=dt)
    ops.conv2d_fwd(x, w, y, G, B, H, W, Cin, Cout, (R, S), st, pad)
    dx = _nan(G, B, H, W, Cin, dt=dt)
    ops.conv2d_bwd_data(dy, w, dx, G, B, H, W, Cin, Cout, (R, S), st, pad,
                        addend=d["addend"].to(dev) if addend else None)
    splits = ops.wgrad_splits(G, B, H, W, Cin, Cout, (R, S), st, pad)
    ws = _nan(splits, G, Cout, R * S * Cin)
    ops.conv2d_bwd_weight(x, dy, ws, splits, G, B, H, W, Cin, Cout, (R, S), st, pad)
    torch.cuda.synchronize()
    return y, dx, ws, splits


def _dw(ws, i):
    G, B, H, W, Cin, Cout, R, S, st, pad = CASES[i]
    return ws.sum(0).view(G, Cout, R, S, Cin)


_F32_ERR = {}


def _f32_errors(i, mode, set_mode):
    """[(err, scale)] of (y, dx, dW) of case i under an fp32 arithmetic, measured once."""
    if (i, mode) not in _F32_ERR:
        set_mode(mode)
        y, dx, ws, splits = _run(i, torch.float32)
        d = _data(i, torch.float32)
        _F32_ERR[i, mode] = [_err(y, d["y"]), _err(dx, d["dx"]), _err(_dw(ws, i), d["dw"])], splits
    return _F32_ERR[i, mode]


@pytest.mark.parametrize("mode", ["exact", "split"])
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_rect_f32(i, mode, f32_math):
    """exact: close(rtol=1e-4, atol=1e-5) to float64.  split: error <= 2 x the exact mode's error
    on the same inputs + 2^-24 max|ref| (the bar of test_split_as_accurate_as_exact)."""
    errs, splits = _f32_errors(i, mode, f32_math)
    if i == 13:
        assert splits >= 2, splits    # case 14: the slabs are summed over split-K slices
    if mode == "exact":
        for what, (e, scale) in zip(("y", "dx", "dW"), errs):
            _bar(f"f32 exact c{i + 1} {what}", e, 1e-5 + 1e-4 * scale)
        return
    exact, _ = _f32_errors(i, "exact", f32_math)
    for what, (e, scale), (e_x, _) in zip(("y", "dx", "dW"), errs, exact):
        _bar(f"f32 split c{i + 1} {what} (exact err {e_x:.3e})", e, 2.0 * e_x + ULP32 * scale)


@pytest.mark.parametrize("dt", H16, ids=["bf16", "f16"])
@pytest.mark.parametrize("i", range(N16), ids=IDS[:N16])
def test_rect_h16(i, dt):
    """Forward 2 ulp, data gradient with an addend 4 ulp, slabs 1e-4, relative to max|ref| (the
    bars of test_conv16_fwd_dgrad_wgrad); Cout % 64 != 0: the register-staged data gradient is
    bit-identical to the pipelined kernel's on Cout zero-padded to 64."""
    from mauv import ops
    G, B, H, W, Cin, Cout, R, S, st, pad = CASES[i]
    d = _data(i, dt)
    y, dx, ws, splits = _run(i, dt)
    tag = f"{DT_IDS[dt]} c{i + 1}"
    _close(f"{tag} y", y, d["y"], 2 * ULP[dt])
    _close(f"{tag} dx", dx, d["dx"], 4 * ULP[dt])
    _close(f"{tag} dW", _dw(ws, i), d["dw"], 1e-4)
    if i == 13:
        assert splits >= 2, splits
    if Cout % 64:
        Cp = -(-Cout // 64) * 64
        dyp = F.pad(d["dy"], (0, Cp - Cout)).to(dev)
        wp = F.pad(d["w"], (0, 0, 0, 0, 0, 0, 0, Cp - Cout)).to(dev)
        dxp = _nan(G, B, H, W, Cin, dt=dt)
        ops.conv2d_bwd_data(dyp, wp, dxp, G, B, H, W, Cin, Cp, (R, S), st, pad,
                            addend=d["addend"].to(dev))
        assert torch.equal(dx, dxp)


@pytest.mark.parametrize("dt", [torch.float32] + H16, ids=["fp32", "bf16", "f16"])
@pytest.mark.parametrize("i", [0, 2, 8], ids=["c1", "c3", "c9"])
def test_rect_lazy_bn_input_and_stats(i, dt):
    """x' = relu(x*scale + shift) on load (forward and weight gradient) with every shift
    positive — a padded tap that received relu(shift) instead of 0 shows in y and the slabs — and
    the epilogue's statistics partials: all written, counts summing to B*Ho*Wo, merged mean and
    variance against float64 (bars of test_conv_lazy_bn_input_and_stats, fp32, and
    test_conv16_lazy_bn_input_and_stats, 16-bit)."""
    from mauv import ops
    G, B, H, W, Cin, Cout, R, S, st, pad = CASES[i]
    d = _data(i, dt)
    Ho, Wo = d["Ho"], d["Wo"]
    gen = torch.Generator().manual_seed(2000 + i)
    sc = torch.rand(G, Cin, generator=gen) + 0.5
    sh = torch.randn(G, Cin, generator=gen).abs() * 0.3 + 0.1
    # the operand x' the kernels form: the fp32 value of x*scale + shift, correctly rounded (they
    # use one fma), then one rounding to the 16-bit format.  float64 gives that fp32 value;
    # torch's unfused fp32 multiply-then-add is an fp32 ulp off now and then, which flips the
    # 16-bit rounding of about one element in 2^15 (1 of case 9's 44,928 in bf16), and one
    # flipped x' moves a slab entry by ulp16(x') * |dy| = 1.1e-2 there, twice the 1e-4 bar
    xt = torch.relu(d["x"].double() * sc.double()[:, None, None, None] +
                    sh.double()[:, None, None, None]).float().to(dt)
    y_ref, _, dw_ref = _ref_all(xt, d["w"], d["dy"], st, pad)
    x, w, dy = d["x"].to(dev), d["w"].to(dev), d["dy"].to(dev)
    xbn = (sc.to(dev), sh.to(dev), 1)
    nblk = ops.fwd_stat_blocks(G, B, H, W, Cin, Cout, (R, S), st, pad)
    pm, pm2, pc = _nan(G, nblk, Cout), _nan(G, nblk, Cout), _nan(G, nblk)
    y = _nan(G, B, Ho, Wo, Cout, dt=dt)
    ops.conv2d_fwd(x, w, y, G, B, H, W, Cin, Cout, (R, S), st, pad, x_bn=xbn, stats=(pm, pm2, pc))
    splits = ops.wgrad_splits(G, B, H, W, Cin, Cout, (R, S), st, pad)
    ws = _nan(splits, G, Cout, R * S * Cin)
    ops.conv2d_bwd_weight(x, dy, ws, splits, G, B, H, W, Cin, Cout, (R, S), st, pad, x_bn=xbn)
    torch.cuda.synchronize()
    tag = f"bn-on-load {DT_IDS[dt]} c{i + 1}"
    f32 = dt == torch.float32
    if f32:
        _close(f"{tag} y", y, y_ref, 1e-4, 1e-5)
        _close(f"{tag} dW", _dw(ws, i), dw_ref, 1e-4, 1e-5)
    else:
        _close(f"{tag} y", y, y_ref, 2 * ULP[dt])
        _close(f"{tag} dW", _dw(ws, i), dw_ref, 1e-4)
    assert torch.isfinite(pm).all() and torch.isfinite(pm2).all() and torch.isfinite(pc).all()
    n = pc.double().cpu()
    assert n.sum(1).eq(B * Ho * Wo).all(), n
    mu = (pm.double().cpu() * n[..., None]).sum(1) / n.sum(1, keepdim=True)
    m2 = (pm2.double().cpu() + n[..., None] * (pm.double().cpu() - mu[:, None]) ** 2).sum(1)
    r = y_ref.reshape(G, -1, Cout)
    if f32:
        _close(f"{tag} mean", mu, r.mean(1), 1e-4, 1e-5)
        _close(f"{tag} var", m2 / r.shape[1], r.var(1, unbiased=False), 1e-4, 1e-5)
    else:
        _close(f"{tag} mean", mu, r.mean(1), 1e-4)
        _close(f"{tag} var", m2 / r.shape[1], r.var(1, unbiased=False), 1e-3)


@pytest.mark.parametrize("dt", [torch.float32] + H16, ids=["fp32", "bf16", "f16"])
@pytest.mark.parametrize("i,src,res", [(0, "lazy", False), (2, "mask", True)], ids=["c1", "c3"])
def test_rect_dgrad_bn_partials_epilogue(i, src, res, dt):
    """BN-backward partials from the data-gradient epilogue: dx bit-identical to the plain data
    gradient, every partial written, and their sums over blocks against the float64 sums of dz and
    dz * xhat computed from that dx within 1e-4 max + 1e-3 (test_conv16_dgrad_bn_partials_epilogue).
    c1: ReLU mask from y*scale + shift; c3 (stride 2, four parity classes of different extents):
    mask bits and a residual addend."""
    from mauv import ops
    G, B, H, W, Cin, Cout, R, S, st, pad = CASES[i]
    d = _data(i, dt)
    C, M = Cin, B * H * W
    gen = torch.Generator().manual_seed(3000 + i)
    y = torch.randn(G, B, H, W, C, generator=gen).to(dt).to(dev)
    mean = (torch.randn(G, C, generator=gen) * 0.1).to(dev)
    invstd = (torch.rand(G, C, generator=gen) + 0.5).to(dev)
    sc = (torch.rand(G, C, generator=gen) + 0.5).to(dev)
    sh = (torch.randn(G, C, generator=gen) * 0.1).to(dev)
    w, dy = d["w"].to(dev), d["dy"].to(dev)
    addend = d["addend"].to(dev) if res else None
    mask = None
    if src == "mask":
        out = torch.empty_like(y)
        mask = torch.empty(G * M * C // 8, dtype=torch.uint8, device=dev)
        ops.bn_apply_mask(y, sc, sh, None, out, mask, G, M, C)
        pre_act = out.double().view(G, M, C)      # the bits are of the stored (rounded) output
    else:
        pre_act = y.double().view(G, M, C) * sc.double()[:, None] + sh.double()[:, None]
    dx_plain = _nan(G, B, H, W, C, dt=dt)
    ops.conv2d_bwd_data(dy, w, dx_plain, G, B, H, W, Cin, Cout, (R, S), st, pad, addend=addend)
    nblk = ops.dgrad_stat_blocks(G, B, H, W, Cin, Cout, (R, S), st, pad)
    p1, p2 = _nan(G, nblk, C), _nan(G, nblk, C)
    dx = _nan(G, B, H, W, C, dt=dt)
    bn = dict(y=y, out=None, mask=mask, scale=sc, shift=sh, mean=mean, invstd=invstd, relu=True,
              p1=p1, p2=p2)
    ops.conv2d_bwd_data(dy, w, dx, G, B, H, W, Cin, Cout, (R, S), st, pad, addend=addend, bn=bn)
    torch.cuda.synchronize()
    assert torch.isfinite(dx).all() and torch.equal(dx, dx_plain)
    assert torch.isfinite(p1).all() and torch.isfinite(p2).all()    # every block written
    dz = dx.double().view(G, M, C) * (pre_act > 0)
    xh = (y.double().view(G, M, C) - mean.double()[:, None]) * invstd.double()[:, None]
    tag = f"bn-partials {DT_IDS[dt]} c{i + 1}"
    _close(f"{tag} sum dz", p1.double().sum(1), dz.sum(1).cpu(), 1e-4, 1e-3)
    _close(f"{tag} sum dz*xhat", p2.double().sum(1), (dz * xh).sum(1).cpu(), 1e-4, 1e-3)


@pytest.mark.parametrize("dt", H16, ids=["bf16", "f16"])
@pytest.mark.parametrize("i", [1, 8], ids=["c2", "c9"])
def test_rect_every_route_same_bits(i, dt):
    """include/mauv.h promises the same bits from every route: with the halo, chunked-halo,
    expand and 256-row kernels switched off the outputs equal the default route's (a route whose
    predicate took a 3x1 filter or a strided 3x3 for its 3x3 / stride-1 shape would not)."""
    from mauv import ops
    default = _run(i, dt)[:3]
    prev = ops.set_route(halo3=0, haloc16=0, expand16=0, big16=0)
    try:
        plain = _run(i, dt)[:3]
    finally:
        ops.set_route(**prev)
    for what, a, b in zip(("y", "dx", "slabs"), default, plain):
        assert torch.isfinite(a).all() and torch.equal(a, b), what
