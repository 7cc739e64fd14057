"""The frozen-BatchNorm kernels (mauv_bn_eval_stats, mauv_bn_bwd_frozen) against float64 on the
same rounded operands, and against mauv_bn_bwd_ex where they must give its bits.

Shapes (G, M, C): one thread per row (C = 8: 256 rows in parallel) up to 256 threads a row
(C = 2048: one row at a time), with M below, at a multiple of and one past the rows a block
walks.  The row walk gives a block 2 * 256 / (C / 8) rows: (1, 1, 8) and (3, 5, 8) leave most
threads of one block without a row, (2, 513, 64) is 8 full 64-row blocks and one row, (2, 33, 256)
two 16-row blocks and one row, (1, 3, 2048) and (3, 7, 2048) 2-row blocks with an odd last one.
The summing kernel gives a block 32 * 256 / (C / 8) rows in steps of 4 rows a thread: every shape
of the issue is one block per group there (3 and 7 rows of 2048 channels: a ragged 4-row step);
(2, 300, 256), added here, is two blocks per group, the second ragged.

Bars: dres is dout or zero, so exact.  dy = store(scale * dz) is one fp32 product (2^-24
relative) and one rounding to the storage type (h = 0 / 2^-8 / 2^-11 for fp32 / bf16 / f16, f16
also half its subnormal spacing 2^-25): |err| <= (2^-23 + h) |ref| — the bound
tests/helpers.check_avgpool uses for the same two roundings.  dgamma / dbeta are the bits
mauv_bn_bwd_ex accumulates for the same operands, and within tests/test_kernels_gpu.py::close's
default bar of float64."""
import pytest
import torch

from tests.test_kernels_gpu import close

pytestmark = pytest.mark.gpu

dev = "cuda"
DTS = [torch.float32, torch.bfloat16, torch.float16]
SHAPES = [(1, 1, 8), (3, 5, 8), (2, 513, 64), (2, 33, 256), (1, 3, 2048), (3, 7, 2048),
          (2, 300, 256)]
H = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
PAD = 64   # NaN sentinels behind every written buffer


def _padded(n, dt):
    """(a NaN-filled buffer of n + PAD elements, its first n)."""
    full = torch.full((n + PAD,), float("nan"), device=dev, dtype=dt)
    return full, full[:n]


def _operands(dt, G, M, C):
    from mauv import ops
    torch.manual_seed(1000 * G + 10 * M + C)
    y = (torch.randn(G, M, C, device=dev) * 2).to(dt)
    r = torch.randn(G, M, C, device=dev).to(dt)
    s, h = torch.randn(G, C, device=dev), torch.randn(G, C, device=dev)
    s[:, :4] = 0.0          # pre-activations exactly the shift
    h[:, :2] = 0.0          # ... and exactly 0 -> masked
    out = torch.empty_like(y)
    mask = torch.empty(G * M * C // 8, dtype=torch.uint8, device=dev)
    ops.bn_apply_mask(y, s, h, r, out, mask, G, M, C)
    mean, invstd = torch.randn(G, C, device=dev), torch.rand(G, C, device=dev) + 0.5
    dout = torch.randn(G, M, C, device=dev).to(dt)
    return y, out, mask, s, h, mean, invstd, dout


@pytest.mark.parametrize("dt", DTS, ids=["fp32", "bf16", "f16"])
@pytest.mark.parametrize("source", ["none", "lazy", "out", "mask"])
@pytest.mark.parametrize("G,M,C", SHAPES)
def test_bn_bwd_frozen(dt, source, G, M, C):
    from mauv import ops
    y, out, mask, s, h, mean, invstd, dout = _operands(dt, G, M, C)
    o = out if source == "out" else None
    mk = mask if source == "mask" else None
    relu = source != "none"
    # float64 reference on the rounded operands
    if source == "none":
        passed = torch.ones(G, M, C, dtype=torch.bool, device=dev)
    elif source == "lazy":   # the sign of the exact y * scale + shift (the kernels' one fma)
        passed = y.double() * s.double()[:, None] + h.double()[:, None] > 0
    else:
        passed = out.float() > 0
    if relu and M * C > 8:   # the source both passes and blocks
        assert bool(passed.any()) and not bool(passed.all())
    dres_ref = torch.where(passed, dout, torch.zeros_like(dout))
    dz = dres_ref.double()
    dy_ref = s.double()[:, None] * dz
    db_ref = dz.sum((0, 1))
    dg_ref = (dz * (y.double() - mean.double()[:, None]) * invstd.double()[:, None]).sum((0, 1))
    # mauv_bn_bwd_ex's parameter gradients for the same operands, mean and invstd
    ws = torch.empty(ops.bn_workspace_floats(G, M, C), device=dev)
    dg_ex, db_ex = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
    ops.bn_bwd_ex(y, o, mk, dout, relu, mean, invstd, s, h, G, M, C, ws, None, None, dg_ex, db_ex)
    n, wsn = G * M * C, ops.bn_workspace_floats(G, M, C)
    for want_dres in (True, False):
        for grads in (True, False):
            runs = []
            dg, db = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
            for rep in range(2):
                dy_full, dy = _padded(n, dt)
                dres_full, dres = _padded(n, dt)
                ws_full, ws = _padded(wsn, torch.float32)
                ops.bn_bwd_frozen(y, o, mk, dout, relu, mean if grads else None,
                                  invstd if grads else None, s, h, G, M, C,
                                  ws if grads else None, dy.view(G, M, C),
                                  dres.view(G, M, C) if want_dres else None,
                                  dg if grads else None, db if grads else None)
                for full, k in ((dy_full, n), (dres_full, n), (ws_full, wsn)):
                    assert bool(full[k:].isnan().all()), "wrote past its buffer"
                if not want_dres:
                    assert bool(dres_full.isnan().all())
                if not grads:
                    assert bool(ws_full.isnan().all()), "the affine-frozen form takes no workspace"
                runs.append((dy.clone(), dres.clone()))
                if rep == 0 and grads:
                    assert torch.equal(dg, dg_ex) and torch.equal(db, db_ex)
                    close(dg, dg_ref)
                    close(db, db_ref)
            if grads:   # the second run accumulated the same bits into the first's: exactly 2x
                assert torch.equal(dg, 2 * dg_ex) and torch.equal(db, 2 * db_ex)
            (dy0, dres0), (dy1, dres1) = runs
            assert torch.equal(dy0, dy1)
            err = (dy0.view(G, M, C).double() - dy_ref).abs()
            lim = (2.0 ** -23 + H[dt]) * dy_ref.abs() + (2.0 ** -25 if dt == torch.float16 else 0.0)
            assert bool((err <= lim).all()), (err - lim).max().item()
            if want_dres:
                assert torch.equal(dres0, dres1)
                assert torch.equal(dres0.view(G, M, C), dres_ref)


def test_bn_bwd_frozen_gradients_only():
    """dy and dres both None: the parameter gradients alone, mauv_bn_bwd_ex's bits."""
    from mauv import ops
    G, M, C = 2, 33, 256
    y, out, mask, s, h, mean, invstd, dout = _operands(torch.bfloat16, G, M, C)
    res = []
    for fn in (ops.bn_bwd_ex, ops.bn_bwd_frozen):
        ws = torch.empty(ops.bn_workspace_floats(G, M, C), device=dev)
        dg, db = torch.ones(C, device=dev), torch.full((C,), -3.0, device=dev)
        fn(y, None, mask, dout, 1, mean, invstd, s, h, G, M, C, ws, None, None, dg, db)
        res.append((dg, db))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert not torch.equal(res[0][0], torch.ones(C, device=dev))


@pytest.mark.parametrize("C", [12, 2056])
def test_bn_bwd_frozen_refuses_what_bn_bwd_ex_refuses(C):
    from mauv import ops, MauvError
    y = torch.zeros(1, 2, C, device=dev)
    st = torch.ones(1, C, device=dev)
    ws = torch.empty(max(1, ops.bn_workspace_floats(1, 2, C)), device=dev)
    for fn in (ops.bn_bwd_ex, ops.bn_bwd_frozen):
        with pytest.raises(MauvError, match="unsupported C"):
            fn(y, None, None, y, 0, st, st, st, st, 1, 2, C, ws, torch.empty_like(y))


def test_bn_bwd_frozen_operand_checks():
    from mauv import ops
    G, M, C = 1, 4, 8
    y = torch.zeros(G, M, C, device=dev)
    st = torch.ones(G, C, device=dev)
    with pytest.raises(ValueError, match="contiguous"):      # a host tensor
        ops.bn_bwd_frozen(y, None, None, y.cpu(), 0, None, None, st, None, G, M, C, None, y)
    with pytest.raises(ValueError, match="contiguous"):      # another storage type
        ops.bn_bwd_frozen(y, None, None, y.half(), 0, None, None, st, None, G, M, C, None, y)
    with pytest.raises(ValueError, match="sizes"):
        ops.bn_bwd_frozen(y, None, None, y, 0, None, None, st, None, G, M + 1, C, None, y)
    with pytest.raises(ValueError, match="mask size"):
        ops.bn_bwd_frozen(y, None, torch.zeros(3, dtype=torch.uint8, device=dev), y, 1, None,
                          None, st, None, G, M, C, None, y)
    with pytest.raises(ValueError, match="workspace"):
        ops.bn_bwd_frozen(y, None, None, y, 0, st, st, st, None, G, M, C,
                          torch.empty(1, device=dev), y, dgamma=torch.zeros(C, device=dev))


@pytest.mark.parametrize("G,C", [(1, 8), (3, 64), (5, 2048), (2, 1000)])
def test_bn_eval_stats(G, C):
    """scale / shift are mauv_bn_eval_params' bits; mean is the running mean and invstd the fp32
    1 / sqrtf(running_var + eps) (sum, square root and quotient each rounded once), for every
    group."""
    from mauv import ops
    torch.manual_seed(C)
    gamma, beta = torch.randn(C, device=dev), torch.randn(C, device=dev)
    rm = torch.randn(C, device=dev) * 3
    rv = torch.rand(C, device=dev) * 2 + 1e-3
    rv[0] = 4.0e-3
    eps = 1e-5
    ref = torch.full((2, G, C), float("nan"), device=dev)
    ops.bn_eval_params(G, C, gamma, beta, rm, rv, eps, ref[0], ref[1])
    full, flat = _padded(4 * G * C, torch.float32)
    got = flat.view(4, G, C)
    ops.bn_eval_stats(G, C, gamma, beta, rm, rv, eps, got[0], got[1], got[2], got[3])
    assert bool(full[4 * G * C:].isnan().all())
    assert torch.equal(got[2], ref[0]) and torch.equal(got[3], ref[1])
    assert torch.equal(got[0], rm.expand(G, C))
    # each fp32 operation correctly rounded, taken through float64 (53 >= 2 * 24 + 2 bits: the
    # second rounding is innocuous for a square root and for a quotient; torch's vectorised
    # CPU sqrt is not correctly rounded)
    root = torch.sqrt((rv.cpu() + eps).double()).float()
    invstd = (1.0 / root.double()).float()
    assert torch.equal(got[1].cpu(), invstd.expand(G, C))
