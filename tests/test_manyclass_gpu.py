"""The many-class Monte-Carlo head (33 <= C <= 4096, csrc/head.hip's *_wide kernels) on the GPU.

Kernel level: every output of mauv_mc_mean_ce / mauv_mc_mean_bwd (both branches) /
mauv_mc_stats / mauv_mc_finalize against float64 torch on ``4 * randn`` logits.  Error of an
output tensor = max |got - ref| / max |ref|; the bar is 4x the error of torch's own fp32 chain on
the GPU against the same float64 reference plus 2^-23, computed in the test on the same inputs
(the margin 4 covers a different summation order and libm differences between ROCm releases).
``pred`` equals the float64 argmax exactly; the seeds below were chosen (on the CPU, from the
float64 reference alone) so that every item's top-2 gap of the mean probability is >= 1e-3.

Measured on an MI355X (worst over the cases of each family; kernel error / torch fp32 error, in
units of 2^-24; the two worsts of a pair need not come from the same case):
  C >= 33   mean 0.82/2.34, loss 0.90/2.09, dlogits 2.40/5.08, dlogits_dmean 0.64/1.06,
            sum_p 5.33/4.60, sum_p2 8.36/8.51, sum_h 1.69/3.18, mean_prob 4.97/5.10,
            aleatoric 2.05/4.52, predictive_entropy 1.64/2.99, var 4.93/7.24;
            largest error / bar of any output of any case: 0.54
  C = 32    mean 1.26/1.60, loss 0.91/0.91, dlogits 5.43/4.40, dlogits_dmean 0.51/1.02,
            sum_p 5.17/2.80, sum_p2 12.39/5.57, sum_h 3.61/3.61, mean_prob 5.30/2.80,
            aleatoric 3.61/3.61, predictive_entropy 2.73/4.59, var 6.13/3.71;
            largest error / bar: 0.80 (sum_p2 at G = 1, B = 1)
The other tests that compare with float64 (ignored labels, the weighted criterion, the tie
test's loss) use the same bar against torch's fp32 evaluation of the same expression.
"""
import copy
import csv
import math

import pytest
import torch
import torch.nn.functional as F

from tests.helpers import build_pair, EpsBridge, oracle64, grad_error_profile, ListLoader

pytestmark = pytest.mark.gpu

EPS_H, EPS_PRED = 1e-7, 1e-8
FLOOR = 2.0 ** -23
CLASSES = [32, 33, 64, 65, 257, 1000, 4096]     # 32: the one-thread-per-item kernels' last C
SHAPES = [(1, 1), (5, 9), (3, 300)]
# per (C, G, B): the first seed (counting from 1000 * C + G) whose float64 reference keeps every
# item's top-2 gap of the mean probability >= 1e-3 and of the mean logit >= 1e-4
SEEDS = {(32, 1, 1): 32001, (32, 5, 9): 32005, (32, 3, 300): 32012,
         (33, 1, 1): 33001, (33, 5, 9): 33005, (33, 3, 300): 33013,
         (64, 1, 1): 64001, (64, 5, 9): 64005, (64, 3, 300): 64026,
         (65, 1, 1): 65001, (65, 5, 9): 65005, (65, 3, 300): 65030,
         (257, 1, 1): 257001, (257, 5, 9): 257005, (257, 3, 300): 257027,
         (1000, 1, 1): 1000001, (1000, 5, 9): 1000005, (1000, 3, 300): 1000042,
         (4096, 1, 1): 4096001, (4096, 5, 9): 4096006, (4096, 3, 300): 4096015,
         (200, 5, 9): 200005, (1537, 5, 9): 1537005}


def _logits(C, G, B):
    g = torch.Generator().manual_seed(SEEDS[(C, G, B)])
    lg = 4.0 * torch.randn(G, B, C, generator=g)
    y = torch.randint(0, C, (B,), generator=g)
    dmean = torch.randn(B, C, generator=g)
    return lg, y, dmean


GLOSS = 1.75    # upstream gradient of the loss in the labels branch of mc_mean_bwd


def _chain(lg, y, dmean, with_var):
    """The reference's maths (train/multimodal.py:121-127, inference/predictors.py:65-84) in the
    dtype and on the device of ``lg`` -> dict of every output the four entry points produce."""
    G = lg.shape[0]
    leaf = lg.clone().requires_grad_(True)
    mean = leaf.mean(0)
    loss = F.cross_entropy(mean, y)
    (dl,) = torch.autograd.grad(loss * GLOSS, leaf)
    P = torch.softmax(lg, dim=2)
    H = -torch.sum(P * torch.log(P + EPS_H), dim=2)          # [G, B]
    mp = P.mean(0)
    out = dict(mean=mean.detach(), loss=loss.detach().reshape(1), dlogits=dl,
               dlogits_dmean=(dmean / G).expand(G, -1, -1),
               sum_p=P.sum(0), sum_p2=(P * P).sum(0), sum_h=H.sum(0),
               mean_prob=mp, aleatoric=H.mean(0),
               predictive_entropy=-torch.sum(mp * torch.log(mp + EPS_PRED), dim=1))
    if with_var:
        out["var"] = torch.var(P, dim=0).mean(dim=1)
    return out


def _kernels(lg, y, dmean):
    from mauv import ops
    G, B, C = lg.shape
    dev = lg.device
    mean = torch.empty(B, C, device=dev)
    loss = torch.empty(1, device=dev)
    pred = torch.empty(B, dtype=torch.int64, device=dev)
    ops.mc_mean_ce(lg, y, G, B, C, mean, loss, pred)
    dl = torch.empty(G, B, C, device=dev)
    ops.mc_mean_bwd(None, torch.full((1,), GLOSS, device=dev), mean, y, G, B, C, dl)
    dl2 = torch.empty(G, B, C, device=dev)
    ops.mc_mean_bwd(dmean, None, None, None, G, B, C, dl2)
    sums = torch.empty(B, 2 * C + 1, dtype=torch.float64, device=dev)
    ops.mc_stats(lg, G, B, C, EPS_H, sums)
    o = dict(mean_prob=torch.empty(B, C, device=dev), var=torch.empty(B, device=dev),
             aleatoric=torch.empty(B, device=dev), predictive_entropy=torch.empty(B, device=dev))
    pred_p = torch.empty(B, dtype=torch.int64, device=dev)
    ops.mc_finalize(sums, G, B, C, EPS_PRED, o["mean_prob"], o["var"], o["aleatoric"],
                    o["predictive_entropy"], pred_p)
    o.update(mean=mean, loss=loss, dlogits=dl, dlogits_dmean=dl2, sum_p=sums[:, :C],
             sum_p2=sums[:, C:2 * C], sum_h=sums[:, 2 * C])
    return o, pred, pred_p


def _err(a, ref):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return ((a - ref).abs().max() / ref.abs().max()).item()


def _within_bar(got, t32, ref):
    """The file's bar: error vs float64 <= 4x torch's fp32 error on the GPU + 2^-23."""
    e, e32 = _err(got, ref), _err(t32, ref)
    return e <= 4 * e32 + FLOOR, (e, e32)


def _top2_gap(t):
    top = torch.topk(t, 2, dim=1).values
    return (top[:, 0] - top[:, 1]).min().item()


@pytest.mark.parametrize("G,B", SHAPES)
@pytest.mark.parametrize("C", CLASSES)
def test_kernels_against_float64(C, G, B):
    _check_kernels(C, G, B)


@pytest.mark.parametrize("C", [200, 1537])
def test_kernels_remaining_class_tiers(C):
    """The kernel instantiations no C of the grid above selects: the 129..256 and 1025..2048
    class tiers of the cross-entropy and statistics kernels."""
    _check_kernels(C, 5, 9)


def _check_kernels(C, G, B):
    lg, y, dmean = _logits(C, G, B)
    ref = _chain(lg.double(), y, dmean.double(), G > 1)
    assert _top2_gap(ref["mean_prob"]) >= 1e-3 and _top2_gap(ref["mean"]) >= 1e-4
    t32 = _chain(lg.cuda(), y.cuda(), dmean.cuda(), G > 1)
    got, pred, pred_p = _kernels(lg.cuda(), y.cuda(), dmean.cuda())
    assert torch.equal(pred.cpu(), ref["mean"].argmax(1))
    assert torch.equal(pred_p.cpu(), ref["mean_prob"].argmax(1))
    report, bad = [], []
    for k in ref:
        e, e32 = _err(got[k], ref[k]), _err(t32[k], ref[k])
        report.append(f"{k} {e * 2 ** 24:.2f}/{e32 * 2 ** 24:.2f}")
        if not e <= 4 * e32 + FLOOR:
            bad.append(k)
    print(f"\nC={C} G={G} B={B} kernel/torch32 error in 2^-24: " + ", ".join(report))
    assert not bad, (bad, report)


@pytest.mark.parametrize("C", [65, 1000])
def test_accumulate_is_chunking_exact(C):
    """Two chunks of G = 2 and G = 3 give the bits of one call with G = 5."""
    from mauv import mchead
    lg = _logits(C, 5, 9)[0].cuda()
    whole = mchead.mc_stats(lg, EPS_H)
    parts = mchead.mc_stats(lg[2:].contiguous(), EPS_H, mchead.mc_stats(lg[:2].contiguous(), EPS_H))
    assert torch.equal(whole, parts)
    assert torch.isfinite(whole).all().item()


def test_ties_nan_and_reproducible_loss():
    from mauv import mchead
    C, B = 257, 4
    g = torch.Generator().manual_seed(11)
    lg = torch.randint(-5, 5, (3, B, C), generator=g).float()
    lg[:, 0, 3] = lg[:, 0, 200] = 9.0          # item 0: classes 3 and 200 tie -> 3
    lg[:, 1, 63] = lg[:, 1, 64] = 9.0          # item 1: a tie across lanes 63 / 0 -> 63
    lg[:, 2] = float("nan")                    # item 2: all NaN -> class 0
    lg[1, 3, 7] = float("nan")                 # item 3: one NaN sample -> NaN mean at class 7
    lg[:, 3, 100] = 9.0
    lg = lg.cuda()
    y = torch.tensor([3, 63, -100, -100]).cuda()
    loss, mean, pred = mchead.mc_mean_ce(lg, y)
    assert pred.tolist() == [3, 63, 0, 100]
    assert math.isfinite(loss.item())          # the NaN items are not labelled
    ref = F.cross_entropy(lg[:, :2].double().mean(0), y[:2])
    ok, es = _within_bar(loss, F.cross_entropy(lg[:, :2].mean(0), y[:2]), ref)
    assert ok, es
    loss2, _, _ = mchead.mc_mean_ce(lg, y)
    assert loss.view(torch.int32).item() == loss2.view(torch.int32).item()
    y[2] = 5
    assert math.isnan(mchead.mc_mean_ce(lg, y)[0].item())
    # the statistics: the same argmax rules on the mean probability; NaN propagates to the sums
    st = mchead.mc_finalize(mchead.mc_stats(lg, EPS_H), 3, C, EPS_PRED)
    assert st["pred"].tolist()[:3] == [3, 63, 0]
    assert torch.isnan(st["aleatoric"][2:]).all().item()
    assert torch.isfinite(st["aleatoric"][:2]).all().item()


def test_labels_ignored_and_out_of_range():
    from mauv import mchead
    C, G, B = 40, 3, 6
    g = torch.Generator().manual_seed(5)
    lg = (4.0 * torch.randn(G, B, C, generator=g)).cuda()
    y = torch.tensor([0, 39, -100, 7, -100, 12]).cuda()
    leaf = lg.clone().requires_grad_(True)
    loss, mean, pred = mchead.mc_mean_ce(leaf, y)
    loss.backward()
    l64 = lg.double().requires_grad_(True)
    ref = F.cross_entropy(l64.mean(0), y, ignore_index=-100)
    ref.backward()
    l32 = lg.clone().requires_grad_(True)
    t32 = F.cross_entropy(l32.mean(0), y, ignore_index=-100)
    t32.backward()
    ok, es = _within_bar(loss, t32, ref)
    assert ok, es
    ok, es = _within_bar(leaf.grad, l32.grad, l64.grad)
    assert ok, es
    assert (leaf.grad[:, [2, 4]] == 0).all().item()
    for badlabel in (40, -1):
        yb = y.clone()
        yb[3] = badlabel
        loss, mean, pred = mchead.mc_mean_ce(lg, yb)
        assert math.isnan(loss.item())
        assert torch.isfinite(mean).all().item()
        assert torch.equal(pred.cpu(), lg.double().mean(0).argmax(1).cpu())
    # nothing but ignored labels: 0 / 0, as torch
    assert math.isnan(mchead.mc_mean_ce(lg, torch.full((B,), -100).cuda())[0].item())


def test_mc_loss_non_plain_criterion():
    """A weighted, label-smoothed criterion takes mc_mean forward and the dmean backward."""
    from mauv import train

    class Fixed(torch.nn.Module):
        def __init__(self, lg):
            super().__init__()
            self.lg = lg

        def mc_forward(self, num_mc):
            return self.lg

    C, G, B = 40, 3, 5
    g = torch.Generator().manual_seed(6)
    lg = (4.0 * torch.randn(G, B, C, generator=g)).cuda()
    w = (0.5 + torch.rand(C, generator=g)).cuda()
    y = torch.randint(0, C, (B,), generator=g).cuda()
    crit = torch.nn.CrossEntropyLoss(weight=w, label_smoothing=0.1)
    assert not train._is_plain_ce(crit)
    leaf = lg.clone().requires_grad_(True)
    loss, output, predicted, ce, _ = train.mc_loss(Fixed(leaf), (), y, crit, G, B, 1.0)
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
    assert torch.equal(predicted.cpu(), l64.mean(0).argmax(1).cpu())


def _cuda(*ts):
    return [t.cuda() for t in ts]


def test_model_train_step_and_statistics_40_classes():
    """build_pair(num_classes=40): one MC train step against the oracle and the float64 oracle
    with tests/test_model_gpu.py's bars, then mc_statistics against predictors.py's maths."""
    from oracle import bayes_ref, loops_ref
    from tests.golden.common import make_batches, SEED_DATA, eps_generator_source
    from tests.helpers import ReplayEps, forward_order
    from mauv.engine import root_state
    from mauv.kl import get_kl_loss
    from mauv.predict import mc_statistics
    from mauv import mchead
    C, B, N = 40, 2, 3
    o, m = build_pair(num_classes=C)
    o_pre = copy.deepcopy(o)
    o_stat = copy.deepcopy(o)
    batch = make_batches(SEED_DATA, 1, B=B, S_opt=64, S_son=64)[0]
    x, b, s = batch["main_image"], batch["bathy_image"], batch["sss_image"]
    y = torch.tensor([33, 39])

    def oracle_loss(model, dt=torch.float32):
        lg = torch.stack([model(x.to(dt), b.to(dt), s.to(dt)) for _ in range(N)])
        loss = F.cross_entropy(lg.mean(0), y) + bayes_ref.get_kl_loss(model) / B * 0.5
        loss.backward()
        return lg, loss

    bridge = EpsBridge(o, m, 99)
    with bridge:
        o_logits, loss_o = oracle_loss(o)
    bridge.collect()
    o64, (l64, loss64) = oracle64(o_pre, bridge.store, lambda mm: oracle_loss(mm, torch.float64))
    root_state(m).eps_provider = bridge.provider
    logits = m.mc_forward(*_cuda(x, b, s), N)
    assert logits.shape == (N, B, C)
    for ref in (o_logits, l64):
        d = (logits.detach().double().cpu() - ref.detach().double()).abs().max().item()
        assert d <= 2e-4 * max(1.0, ref.detach().abs().max().item()), d
    ce, out, pred = mchead.mc_mean_ce(logits, y.cuda())
    loss = ce + get_kl_loss(m) / B * 0.5
    for ref in (loss_o, loss64):
        assert abs(loss.item() - ref.item()) <= 2e-4 * max(1.0, abs(ref.item()))
    loss.backward()
    h, c = grad_error_profile(list(m.parameters()), list(o.parameters()), list(o64.parameters()))
    assert h[0] <= 1.5 * c[0] + 1e-4, (h, c)
    assert h[1] <= 2.0 * c[1] + 1e-4, (h, c)
    assert h[2] <= 2.0 * c[2] + 1e-4, (h, c)

    # statistics: a fresh pair of equal weights, predictors.py's loop on the oracle
    _, m2 = build_pair(num_classes=C)
    order = forward_order(copy.deepcopy(o_stat), x, b, s)
    bayes_ref.set_eps_source(eps_generator_source(5))
    try:
        pred_o, var_o, alea_o, P = loops_ref.predict_batch(o_stat, x, b, s, 5)
    finally:
        bayes_ref.set_eps_source(None)
    root_state(m2).eps_provider = ReplayEps(m2, order, 5)
    with torch.no_grad():
        st = mc_statistics(m2, *_cuda(x, b, s), 5, chunk=3)
    mp = P.mean(0)
    ent_o = -torch.sum(mp * torch.log(mp + 1e-8), dim=1)
    assert torch.equal(st["pred"].cpu(), pred_o)
    assert (st["var"].cpu() - var_o).abs().max().item() <= 1e-6
    assert (st["aleatoric"].cpu() - alea_o).abs().max().item() <= 1e-5
    assert (st["predictive_entropy"].cpu() - ent_o).abs().max().item() <= 1e-5


def test_unimodal_gated_step_and_dropin_predict_40_classes(tmp_path):
    from mauv.models import ResNet50Custom
    from mauv.layers import dnn_to_bnn
    from mauv.optim import FusedAdam
    from mauv.train import mc_train_step
    from mauv.predict import multimodal_predict_and_save
    from tests.helpers import DEFAULT_PRIOR
    C = 40
    torch.manual_seed(3)
    m = ResNet50Custom(3, C)
    dnn_to_bnn(m, DEFAULT_PRIOR)
    m = m.cuda()
    x = torch.randn(2, 3, 64, 64).cuda()
    y = torch.tensor([17, 39]).cuda()
    opt = FusedAdam(m.parameters(), lr=1e-4)
    r = mc_train_step(m, (x,), y, torch.nn.CrossEntropyLoss(), opt, 2, 2, 1e-6)
    assert torch.is_tensor(r["stepped"]) and r["stepped"].is_cuda   # the device gate decided
    assert bool(r["stepped"]) and math.isfinite(float(r["loss"]))
    # the same step with bf16 trunks: the unimodal model's 40-wide fc behind 16-bit features
    from mauv.engine import set_precision
    set_precision(m, torch.bfloat16)
    r = mc_train_step(m, (x,), y, torch.nn.CrossEntropyLoss(), opt, 2, 2, 1e-6)
    assert bool(r["stepped"]) and math.isfinite(float(r["loss"]))

    _, mm = build_pair(num_classes=C)
    g = torch.Generator().manual_seed(8)
    batches = []
    for i in range(2):
        bathy = torch.rand(2, 3, 64, 64, generator=g)
        bathy[:, 2] = 0
        batches.append((torch.randn(2, 3, 64, 64, generator=g), bathy,
                        torch.rand(2, 1, 64, 64, generator=g), [f"t{i}_{j}" for j in range(2)]))
    path = tmp_path / "pred.csv"
    multimodal_predict_and_save(mm, ListLoader(batches, 2), "cuda", str(path), num_mc_samples=4)
    assert mm.__dict__.get("_mauv_graphs"), "the second batch was not captured"
    rows = list(csv.reader(open(path)))
    assert len(rows) == 1 + 4 and [r[0] for r in rows[1:]] == ["t0_0", "t0_1", "t1_0", "t1_1"]
    for r in rows[1:]:
        assert 0 <= int(r[1]) < C
        assert math.isfinite(float(r[2])) and math.isfinite(float(r[3]))
        assert float(r[2]) >= 0 and -1e-6 <= float(r[3]) <= math.log(C) + 1e-5
