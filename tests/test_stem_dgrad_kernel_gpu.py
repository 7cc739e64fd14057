"""The two kernels of the stems' data gradient (stem_dgrad.hip) against float64, with derived bounds.

  stem_col2im    against F.fold in float64 on the same fp32 rows (torch's unfold order is
                 c*R*S + r*S + s, the rows' own).  A pixel sums at most T taps sequentially in
                 fp32: |err| <= T 2^-24 fold(|drows|) elementwise, T the largest tap count of the
                 shape; bit-equal where exactly one tap reaches the pixel.  The padded columns
                 k >= K hold NaN: they are never read.
  adjoint        <im2col(x), c> = <x, col2im(c)> with the existing ops.stem_im2col (an exact
                 gather), evaluated in float64 from the kernels' outputs: the same bound summed
                 against |x|.
  stem_bwd_rows  against float64 on the same operands (rounded to the storage type first for
                 16-bit): |err| <= (G Cout + 2) 2^-23 (|dy| . |w|) elementwise — a sequential
                 fp32 accumulation of G*Cout exact products (bf16 / f16 products are exact in
                 fp32; the fp32 kernel uses the exact f32 MFMA, one rounding per product and sum).
                 The reference sums the G per-sample products: the sum over samples is proven at
                 G = 2, 3.  Padded columns come out exactly 0.
  Both kernels give equal bits on two runs and leave the NaN tails behind drows / dx untouched.

Worst observed ratios to the bounds (MI355X, pytest -rP): DESIGN.md §2.40."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# (B, C, H, W, R, stride, pad, G, Cout)
SHAPES = [
    (2, 3, 9, 12, 7, 2, 3, 3, 64),    # M = 60: one partial tile, H != W, odd and even extents
    (2, 1, 23, 18, 7, 2, 3, 1, 64),   # M = 216: more than one row tile, C = 1, Kp 49 -> 64
    (1, 3, 7, 7, 7, 2, 3, 2, 64),     # every pixel touches padding
    (1, 5, 6, 7, 3, 1, 1, 2, 64),     # a non-stem geometry, K = 45
    (2, 3, 9, 12, 7, 2, 3, 1, 16),    # Cout = 16 instead of 64
    # the 128-column tiles of stem_bwd_rows (taken where 64-column tiles waste no fewer columns
    # of Kp; the shapes above have Kp = 64, 160, 192: all 64-column):
    (2, 4, 9, 12, 7, 2, 3, 2, 64),    # K = 196: Kp = 224 fp32 (a 96-column partial tile), 256 16-bit
    (2, 2, 23, 18, 7, 2, 3, 2, 64),   # K = 98: Kp = 128, one full tile, more than one row tile
]
IDS = ["M60_G3", "M216_C1", "all_padding", "3x3_s1_K45", "Cout16", "C4_Kp224_256", "C2_Kp128"]
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
DT_IDS = ["fp32", "bf16", "f16"]
GUARD = 4096


def _guarded(n):
    """n fp32 elements followed by GUARD NaN sentinels in one allocation."""
    buf = torch.full((n + GUARD,), float("nan"), device="cuda")
    return buf, buf[:n]


def _tail_ok(buf, n):
    return bool(torch.isnan(buf[n:]).all().item())


def _geo(shape, dt):
    from mauv import ops
    B, C, H, W, R, st, pd, G, Cout = shape
    K = C * R * R
    Ho, Wo = ops.out_hw(H, R, st, pd), ops.out_hw(W, R, st, pd)
    return K, ops.stem_kp(dt, K), Ho, Wo, B * Ho * Wo


def _fold64(rows, shape, K, Ho, Wo):
    """F.fold in float64 of rows[M][>= K] (columns k < K)."""
    B, C, H, W, R, st, pd = shape[:7]
    cols = rows[:, :K].double().reshape(B, Ho * Wo, K).transpose(1, 2)
    return F.fold(cols, (H, W), kernel_size=R, padding=pd, stride=st)


def _col2im(drows, shape, Kp):
    from mauv import ops
    B, C, H, W, R, st, pd = shape[:7]
    n = B * C * H * W
    buf, dx = _guarded(n)
    ops.stem_col2im(drows, B, C, H, W, R, st, pd, Kp, dx.view(B, C, H, W))
    torch.cuda.synchronize()
    assert _tail_ok(buf, n), "stem_col2im wrote past dx"
    return dx.view(B, C, H, W).clone()


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_col2im_against_fold(shape, dt):
    K, Kp, Ho, Wo, M = _geo(shape, dt)
    torch.manual_seed(11)
    rows = torch.randn(M, Kp)
    rows[:, K:] = float("nan")     # padded columns are never read
    dx = _col2im(rows.cuda(), shape, Kp)
    ref = _fold64(rows, shape, K, Ho, Wo)
    taps = _fold64(torch.ones(M, Kp), shape, K, Ho, Wo)
    T = int(taps.max().item())
    assert T == {(7, 2): 16, (3, 1): 9}[(shape[4], shape[5])]
    err = (dx.double().cpu() - ref).abs()
    bound = T * 2.0 ** -24 * _fold64(rows.abs(), shape, K, Ho, Wo)
    assert torch.isfinite(dx).all().item()
    ratio = (err / bound.clamp_min(1e-300)).max().item()
    print(f"col2im {shape} Kp={Kp}: worst err/bound = {ratio:.3f} (T = {T})")
    assert bool((err <= bound).all())
    one = taps == 1
    assert torch.equal(dx.double().cpu()[one], ref[one])
    # determinism: a second run gives the same bits
    assert torch.equal(_col2im(rows.cuda(), shape, Kp), dx)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_col2im_is_the_adjoint_of_im2col(shape):
    from mauv import ops
    B, C, H, W, R, st, pd = shape[:7]
    K, Kp, Ho, Wo, M = _geo(shape, torch.float32)
    torch.manual_seed(12)
    x = torch.randn(B, C, H, W)
    c = torch.randn(M, Kp)
    cols = torch.empty(M, Kp, device="cuda")
    ops.stem_im2col(x.cuda(), B, C, H, W, R, st, pd, Kp, cols)
    dx = _col2im(c.cuda(), shape, Kp)
    lhs = (cols.double().cpu()[:, :K] * c.double()[:, :K]).sum().item()
    rhs = (x.double() * dx.double().cpu()).sum().item()
    T = int(_fold64(torch.ones(M, Kp), shape, K, Ho, Wo).max().item())
    bound = (x.double().abs() * T * 2.0 ** -24 * _fold64(c.abs(), shape, K, Ho, Wo)).sum().item()
    print(f"adjoint {shape}: |lhs - rhs| = {abs(lhs - rhs):.3e}, bound = {bound:.3e}")
    assert abs(lhs - rhs) <= bound


def _rows(dy, w, G, M, Kp, Cout, K):
    from mauv import ops
    buf, drows = _guarded(M * Kp)
    ops.stem_bwd_rows(dy, w, drows.view(M, Kp), G, M, Kp, Cout, K)
    torch.cuda.synchronize()
    assert _tail_ok(buf, M * Kp), "stem_bwd_rows wrote past drows"
    return drows.view(M, Kp).clone()


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_rows_gemm_against_float64(shape, dt):
    G, Cout = shape[7], shape[8]
    K, Kp, Ho, Wo, M = _geo(shape, dt)
    torch.manual_seed(13)
    dy = torch.randn(G, M, Cout).to(dt)
    w = torch.zeros(G, Cout, Kp)
    w[:, :, :K] = 0.1 * torch.randn(G, Cout, K)
    w = w.to(dt)
    got = _rows(dy.cuda(), w.cuda(), G, M, Kp, Cout, K)
    dy64, w64 = dy.double(), w.double()
    ref = sum(dy64[g] @ w64[g] for g in range(G))           # the float64 sum of the samples
    mag = sum(dy64[g].abs() @ w64[g].abs() for g in range(G))
    bound = (G * Cout + 2) * 2.0 ** -23 * mag
    err = (got.double().cpu() - ref).abs()
    ratio = (err / bound.clamp_min(1e-300))[:, :K].max().item()
    print(f"rows {shape} {dt} Kp={Kp}: worst err/bound = {ratio:.4f}")
    assert torch.isfinite(got).all().item()
    assert bool((err <= bound).all())
    assert bool((got[:, K:] == 0).all()), "padded columns of drows must be exactly 0"
    if G > 1:   # one sample alone is not the answer: the kernel did sum over g
        assert not bool(((got.double().cpu() - dy64[0] @ w64[0]).abs() <= bound).all())
    assert torch.equal(_rows(dy.cuda(), w.cuda(), G, M, Kp, Cout, K), got)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_rows_then_col2im_is_conv_transpose(dt):
    """Both stages together against autograd's own data gradient of the stem convolution in
    float64, summed over the samples (the composition the engine runs)."""
    shape = SHAPES[0]
    B, C, H, W, R, st, pd, G, Cout = shape
    K, Kp, Ho, Wo, M = _geo(shape, dt)
    torch.manual_seed(14)
    dy = torch.randn(G, M, Cout).to(dt)
    w = torch.zeros(G, Cout, Kp)
    w[:, :, :K] = 0.1 * torch.randn(G, Cout, K)
    w = w.to(dt)
    dx = _col2im(_rows(dy.cuda(), w.cuda(), G, M, Kp, Cout, K), shape, Kp)
    x = torch.zeros(B, C, H, W, dtype=torch.float64, requires_grad=True)
    tot = 0.0
    for g in range(G):
        y = F.conv2d(x, w[g, :, :K].double().reshape(Cout, C, R, R), stride=st, padding=pd)
        tot = tot + (y * dy[g].double().reshape(B, Ho, Wo, Cout).permute(0, 3, 1, 2)).sum()
    ref, = torch.autograd.grad(tot, x)
    # 16 taps of rows, each within (G Cout + 2) 2^-23 of its magnitude, plus the tap sum's own
    # 16 2^-24: (G Cout + 2 + 8) 2^-23 of the magnitude sum, bounded here by its maximum
    mag = sum(dy[g].double().abs() @ w[g].double().abs() for g in range(G))
    bound = (G * Cout + 10) * 2.0 ** -23 * _fold64(mag, shape, K, Ho, Wo)
    err = (dx.double().cpu() - ref).abs()
    print(f"rows+col2im {dt}: worst err/bound = {(err / bound.clamp_min(1e-300)).max().item():.4f}")
    assert bool((err <= bound).all())
