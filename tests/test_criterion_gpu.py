"""The criterion-aware MC head (mauv_mc_mean_ce_ex / mauv_mc_mean_bwd_ex) on the GPU: weighted,
label-smoothed, ignore-index cross-entropy with mean or sum reduction at every C in 1..4096.

Kernel level: loss and dlogits (upstream gradient 1.75) of every criterion of the grid, and the
mean and argmax once per shape, against float64 ``F.cross_entropy`` of the float64 mean on
``4 * randn`` logits.  The bar is tests/test_manyclass_gpu.py's ``_within_bar``: error
= max |got - ref| / max |ref| <= 4x the error of torch's fp32 evaluation of the same expression on
the GPU + 2^-23; ``pred`` equals the float64 argmax exactly (the seeds keep every item's top-2 gap
of the float64 mean logit >= 1e-4, asserted before comparing).

Measured on an MI355X (worst over all cases and criteria; kernel error / torch fp32 error, in
units of 2^-24; the two worsts of a pair need not come from the same case):
  loss 0.98/2.80, dlogits 4.02/6.27, mean 0.97/2.08
(a record of one run, not a bar).
"""
import itertools
import math

import pytest
import torch
import torch.nn.functional as F

from tests.test_manyclass_gpu import SEEDS as MANY_SEEDS, GLOSS, _within_bar, _top2_gap

pytestmark = pytest.mark.gpu

CLASSES = [2, 7, 32, 33, 65, 200, 1000, 4096]
SHAPES = [(1, 1), (5, 9), (3, 300)]
# found on the CPU from the float64 mean alone: every item's top-2 gap of the mean logit >= 1e-4
SEEDS = {(2, 1, 1): 2001, (2, 5, 9): 2005, (2, 3, 300): 2003,
         (7, 1, 1): 7001, (7, 5, 9): 7005, (7, 3, 300): 7003,
         (200, 1, 1): 200001, (200, 5, 9): 200005, (200, 3, 300): 200003}
# weights x label_smoothing x reduction, once with ignore_index = -100 and about a quarter of the
# labels ignored, once with ignore_index = 3 (a valid class wherever C > 3)
GRID = [dict(weighted=wt, eps=eps, reduction=red, ignore_index=ii)
        for ii in (-100, 3) for wt, eps, red in itertools.product((False, True), (0.0, 0.1),
                                                                  ("mean", "sum"))]


def _seed(C, G, B):
    return MANY_SEEDS.get((C, G, B)) or SEEDS[(C, G, B)]


def _inputs(C, G, B):
    g = torch.Generator().manual_seed(_seed(C, G, B))
    lg = 4.0 * torch.randn(G, B, C, generator=g)
    y = torch.randint(0, C, (B,), generator=g)
    w = 0.5 + torch.rand(C, generator=g)
    return lg, y, w


def _torch_ce(lg, y, w, eps, ignore_index, reduction):
    """F.cross_entropy of the mean over MC and its gradient under the upstream GLOSS, in the
    dtype and on the device of ``lg`` -> (loss [1], dlogits [G, B, C])."""
    leaf = lg.clone().requires_grad_(True)
    loss = F.cross_entropy(leaf.mean(0), y, weight=w, ignore_index=ignore_index,
                           reduction=reduction, label_smoothing=eps)
    (dl,) = torch.autograd.grad(loss * GLOSS, leaf)
    return loss.detach().reshape(1), dl


def _kernels(lg, y, w, eps, ignore_index, reduction, gloss=GLOSS):
    from mauv import ops
    G, B, C = lg.shape
    dev = lg.device
    mean = torch.empty(B, C, device=dev)
    loss = torch.empty(1, device=dev)
    denom = torch.empty(1, device=dev)
    pred = torch.empty(B, dtype=torch.int64, device=dev)
    ops.mc_mean_ce_ex(lg, y, w, eps, ignore_index, reduction, G, B, C, mean, loss, denom, pred)
    dl = torch.empty(G, B, C, device=dev)
    ops.mc_mean_bwd_ex(torch.full((1,), gloss, device=dev), mean, y, w, eps, ignore_index,
                       reduction, denom, G, B, C, dl)
    return mean, loss, pred, dl


@pytest.mark.parametrize("G,B", SHAPES)
@pytest.mark.parametrize("C", CLASSES)
def test_kernels_against_float64(C, G, B):
    from mauv import ops
    assert hasattr(ops, "mc_mean_ce_ex") and hasattr(ops, "mc_mean_bwd_ex")
    lg, y0, w = _inputs(C, G, B)
    mean64 = lg.double().mean(0)
    if C > 1:
        assert _top2_gap(mean64) >= 1e-4
    lg_d, w_d = lg.cuda(), w.cuda()
    mean32 = lg_d.mean(0)
    worst = {}
    bad = []
    for i, cr in enumerate(GRID):
        y = y0.clone()
        if cr["ignore_index"] == -100:
            y[torch.arange(B) % 4 == 3] = -100
        wt, wt64 = (w_d, w.double()) if cr["weighted"] else (None, None)
        args = (cr["eps"], cr["ignore_index"], cr["reduction"])
        ref_loss, ref_dl = _torch_ce(lg.double(), y, wt64, *args)
        t32_loss, t32_dl = _torch_ce(lg_d, y.cuda(), wt, *args)
        mean, loss, pred, dl = _kernels(lg_d, y.cuda(), wt, *args)
        assert torch.equal(pred.cpu(), mean64.argmax(1)), cr
        outs = [("loss", loss, t32_loss, ref_loss), ("dlogits", dl, t32_dl, ref_dl)]
        if i == 0:
            outs.append(("mean", mean, mean32, mean64))
        else:
            assert torch.equal(mean, mean0), cr   # the criterion does not touch the mean
        mean0 = mean
        assert torch.isfinite(ref_loss).all() and (y != cr["ignore_index"]).any()
        for k, got, t32, ref in outs:
            ok, (e, e32) = _within_bar(got, t32, ref)
            we, we32 = worst.get(k, (0.0, 0.0))
            worst[k] = (max(we, e), max(we32, e32))
            if not ok:
                bad.append((k, cr, e * 2 ** 24, e32 * 2 ** 24))
    print(f"\nC={C} G={G} B={B} worst kernel/torch32 error in 2^-24 over the criterion grid: "
          + ", ".join(f"{k} {e * 2 ** 24:.2f}/{e32 * 2 ** 24:.2f}" for k, (e, e32) in worst.items()))
    assert not bad, bad


@pytest.mark.parametrize("C", [33, 1000])
def test_plain_criterion_equals_the_plain_entries(C):
    """No weights, eps 0, ignore_index -100, mean reduction: mauv_mc_mean_ce's mean, loss and
    pred bit for bit (the same float64 expression), mauv_mc_mean_bwd's dlogits within the bar."""
    from mauv import ops
    assert hasattr(ops, "mc_mean_ce_ex") and hasattr(ops, "mc_mean_bwd_ex")
    G, B = 5, 9
    lg, y, _ = _inputs(C, G, B)
    y[4] = -100
    lg_d, y_d = lg.cuda(), y.cuda()
    mean, loss, pred, dl = _kernels(lg_d, y_d, None, 0.0, -100, "mean")
    mean_p, loss_p = torch.empty_like(mean), torch.empty_like(loss)
    pred_p, dl_p = torch.empty_like(pred), torch.empty_like(dl)
    ops.mc_mean_ce(lg_d, y_d, G, B, C, mean_p, loss_p, pred_p)
    ops.mc_mean_bwd(None, torch.full((1,), GLOSS, device="cuda"), mean_p, y_d, G, B, C, dl_p)
    assert torch.equal(mean.view(torch.int32), mean_p.view(torch.int32))
    assert torch.equal(loss.view(torch.int32), loss_p.view(torch.int32))
    assert torch.equal(pred, pred_p)
    ref_loss, ref_dl = _torch_ce(lg.double(), y, None, 0.0, -100, "mean")
    t32_loss, t32_dl = _torch_ce(lg_d, y_d, None, 0.0, -100, "mean")
    for got in (dl, dl_p):
        ok, es = _within_bar(got, t32_dl, ref_dl)
        assert ok, es
    ok, es = _within_bar(loss, t32_loss, ref_loss)
    assert ok, es


@pytest.mark.parametrize("ii", [-100, 2])
def test_label_rules_at_seven_classes(ii):
    """C = 7 runs the many-class kernels under the criterion: ignored, out-of-range and
    all-ignored labels, no counted weight, and the loss bits of two calls."""
    from mauv import train, mchead
    C, G, B = 7, 3, 6
    g = torch.Generator().manual_seed(7)
    lg = 4.0 * torch.randn(G, B, C, generator=g)
    w = 0.5 + torch.rand(C, generator=g)
    y = torch.tensor([0, 6, ii, 3, ii, 5])
    crit = torch.nn.CrossEntropyLoss(weight=w.cuda(), label_smoothing=0.1, ignore_index=ii)
    lg_d, y_d = lg.cuda(), y.cuda()
    spec = train._ce_spec(crit, lg_d, y_d)
    assert spec is not None      # routed to the fused head: no bad label below reaches torch
    leaf = lg_d.clone().requires_grad_(True)
    loss, mean, pred = mchead.mc_mean_ce_ex(leaf, y_d, **spec)
    (loss * GLOSS).backward()
    ref_loss, ref_dl = _torch_ce(lg.double(), y, w.double(), 0.1, ii, "mean")
    t32_loss, t32_dl = _torch_ce(lg_d, y_d, w.cuda(), 0.1, ii, "mean")
    ok, es = _within_bar(loss, t32_loss, ref_loss)
    assert ok, es
    ok, es = _within_bar(leaf.grad, t32_dl, ref_dl)
    assert ok, es
    assert (leaf.grad[:, [2, 4]] == 0).all().item()
    assert (ref_dl[:, [2, 4]] == 0).all().item()
    loss2 = mchead.mc_mean_ce_ex(lg_d, y_d, **spec)[0]
    assert loss.detach().view(torch.int32).item() == loss2.view(torch.int32).item()
    argmax64 = lg.double().mean(0).argmax(1)
    for badlabel in (7, -1):
        yb = y_d.clone()
        yb[3] = badlabel
        leaf = lg_d.clone().requires_grad_(True)
        loss, mean, pred = mchead.mc_mean_ce_ex(leaf, yb, **spec)
        loss.backward()
        assert math.isnan(loss.item())
        assert torch.isnan(leaf.grad[:, 3]).all().item()
        assert torch.isfinite(leaf.grad[:, [0, 1, 2, 4, 5]]).all().item()
        assert (leaf.grad[:, [2, 4]] == 0).all().item()
        assert torch.isfinite(mean).all().item()
        assert torch.equal(pred.cpu(), argmax64)
    # nothing counted: 0 / 0 for the mean (as torch), an empty sum for the sum
    none = torch.full((B,), ii).cuda()
    assert math.isnan(mchead.mc_mean_ce_ex(lg_d, none, **spec)[0].item())
    assert mchead.mc_mean_ce_ex(lg_d, none, **dict(spec, reduction="sum"))[0].item() == 0.0
    # counted items whose classes all have zero weight: no counted weight either
    w0 = w.clone()
    w0[[0, 6, 3, 5]] = 0.0
    for eps in (0.0, 0.1):
        s0 = dict(spec, weight=w0.cuda(), label_smoothing=eps)
        assert math.isnan(mchead.mc_mean_ce_ex(lg_d, y_d, **s0)[0].item())
        assert math.isnan(F.cross_entropy(lg.double().mean(0), y, weight=w0.double(),
                                          ignore_index=ii, label_smoothing=eps).item())


def _params(m):
    return [p.detach().clone() for p in m.parameters()]


def test_train_step_with_weighted_criterion(tmp_path, monkeypatch):
    """mc_train_step and the unimodal drop-in loop under CrossEntropyLoss(weight, smoothing,
    ignore_index) on a 7-class Bayesian ResNet-50: the device gate steps on a good batch, skips
    a batch with a label outside [0, C) (NaN loss from the fused head) and carries on."""
    from mauv import ops, train
    from mauv.models import ResNet50Custom
    from mauv.layers import dnn_to_bnn
    from mauv.optim import FusedAdam
    from tests.helpers import DEFAULT_PRIOR, ListLoader, NullWriter
    C = 7
    torch.manual_seed(3)
    m = ResNet50Custom(3, C)
    dnn_to_bnn(m, DEFAULT_PRIOR)
    m = m.cuda()
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 3, 64, 64, generator=g).cuda()
    y = torch.tensor([2, 6]).cuda()
    w = (0.5 + torch.rand(C, generator=g)).cuda()
    crit = torch.nn.CrossEntropyLoss(weight=w, label_smoothing=0.1, ignore_index=5)
    assert train._ce_spec(crit, torch.empty(2, 2, C, device="cuda"), y) is not None
    calls = []
    real = ops.mc_mean_ce_ex
    monkeypatch.setattr(ops, "mc_mean_ce_ex", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    opt = FusedAdam(m.parameters(), lr=1e-4)
    r = train.mc_train_step(m, (x,), y, crit, opt, 2, 2, 1e-6)
    assert torch.is_tensor(r["stepped"]) and r["stepped"].is_cuda and r["ok_loss"].is_cuda
    assert bool(r["ok_loss"]) and bool(r["stepped"]) and math.isfinite(float(r["loss"]))
    before = _params(m)
    r = train.mc_train_step(m, (x,), torch.tensor([2, 9]).cuda(), crit, opt, 2, 2, 1e-6)
    assert not bool(r["ok_loss"]) and not bool(r["stepped"]) and math.isnan(float(r["loss"]))
    assert all(torch.equal(a, b) for a, b in zip(before, _params(m)))
    r = train.mc_train_step(m, (x,), y, crit, opt, 2, 2, 1e-6)
    assert bool(r["ok_loss"]) and bool(r["stepped"]) and math.isfinite(float(r["loss"]))
    assert not all(torch.equal(a, b) for a, b in zip(before, _params(m)))
    assert len(calls) == 3

    batches = [dict(main_image=torch.randn(2, 3, 64, 64, generator=g),
                    label=torch.tensor(lab)) for lab in ([1, 5], [6, 0])]
    acc, loss = train.train_unimodal_model(
        m, ListLoader(batches, 2), crit, opt, epoch=1, total_num_epochs=3, num_mc=2,
        sum_writer=NullWriter(), device=torch.device("cuda"),
        model_type="image", csv_path=str(tmp_path / "image.csv"))
    assert len(calls) == 5
    assert math.isfinite(loss) and loss > 0 and 0.0 <= acc <= 1.0


@pytest.mark.parametrize("C", [7, 40])
def test_mc_loss_takes_the_fused_head(C, monkeypatch):
    from mauv import ops, train

    class Fixed(torch.nn.Module):
        def __init__(self, lg):
            super().__init__()
            self.lg = lg

        def mc_forward(self, num_mc):
            return self.lg

    G, B = 3, 5
    g = torch.Generator().manual_seed(6)
    lg = (4.0 * torch.randn(G, B, C, generator=g)).cuda()
    w = (0.5 + torch.rand(C, generator=g)).cuda()
    y = torch.randint(0, C, (B,), generator=g).cuda()
    crit = torch.nn.CrossEntropyLoss(weight=w, label_smoothing=0.1)
    calls = []
    real = ops.mc_mean_ce_ex
    monkeypatch.setattr(ops, "mc_mean_ce_ex", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    leaf = lg.clone().requires_grad_(True)
    loss, output, predicted, ce, _ = train.mc_loss(Fixed(leaf), (), y, crit, G, B, 1.0)
    assert len(calls) == 1
    ce.backward()
    l64 = lg.double().requires_grad_(True)
    ref = F.cross_entropy(l64.mean(0), y, weight=w.double(), label_smoothing=0.1)
    ref.backward()
    l32 = lg.clone().requires_grad_(True)
    t32 = crit(l32.mean(0), y)
    t32.backward()
    ok, es = _within_bar(ce, t32, ref)
    assert ok, es
    ok, es = _within_bar(leaf.grad, l32.grad, l64.grad)
    assert ok, es
    ok, es = _within_bar(output, l32.mean(0), l64.mean(0))
    assert ok, es
    assert torch.equal(predicted.cpu(), l64.mean(0).argmax(1).cpu())
