"""What loss scaling is for: f16 trunks (5-bit exponent) on the tri-modal model at the sizes of
tests/test_step_gate_gpu.py (B = 2, 64 px, num_mc = 2, 7 classes), ``kl_w = 0`` and
``CrossEntropyLoss(weight = w everywhere, reduction="sum")`` with w = 2^-30.

Precondition, asserted: with no scaling every trunk gradient in the arena is exactly zero — the
feature gradient the fp32 head hands the trunks is at most about w, below 2^-25, and f16 stores
that as 0 (today's behaviour).  With a static ``loss_scale = 2^30`` the arena after the backward
equals, bit for bit, the arena of the same batch with w = 1 and no scaling: w * S = 1 and every
product with a power of two is exact while nothing leaves fp32's normal range.  After the step
the trunk parameters have moved.

Not asserted, printed: the whole-trunk gradient cosine of an f16 backward against the fp32-trunk
backward of the same weights, batch and MC samples, with no scaler and at scale 2^16 (plain
criterion, KL on).  On an MI355X: 0.553983 unscaled (217 exact zeros among 140,876,288 trunk
elements), 0.553866 at 2^16 (none); the bit comparison above: 0 of 146,767,640 elements differ."""
import pytest
import torch

from tests.test_step_gate_gpu import _batch
from tests.test_gradclip_step_gpu import _arm

pytestmark = pytest.mark.gpu

W, S = 2.0 ** -30, 2.0 ** 30
LR = 1e-3


def _f16_arm(dtype=torch.float16):
    from mauv.engine import set_precision
    m = _arm()
    set_precision(m, dtype)
    return m


def _crit(w):
    return torch.nn.CrossEntropyLoss(weight=torch.full((7,), w, device="cuda"), reduction="sum")


def _trunk_mask(model):
    """bool mask over the arena: the elements of the three trunks' parameters."""
    from mauv.engine import root_state
    ar = root_state(model).arena
    names = {id(p): n for n, p in model.named_parameters()}
    mask = torch.zeros(ar.numel, dtype=torch.bool, device=ar.flat.device)
    for p, o in zip(ar.params, ar.offsets):
        if names[id(p)].split(".")[0].endswith("_feat"):
            mask[o:o + p.numel()] = True
    assert mask.any() and not mask.all()
    return mask


def _backward(model, crit, kl_w=0.0, scaler=None):
    """The arena after the backward of the one batch (cloned), and the loss."""
    from mauv.engine import root_state
    from mauv.train import mc_loss
    x, b, s, y = _batch(10, "ok")
    st = root_state(model)
    st.offset = 0
    loss = mc_loss(model, (x, b, s), y, crit, 2, 2, kl_w)[0]
    (loss if scaler is None else scaler.scale(loss)).backward()
    return st.arena.flat.clone(), loss.detach()


def test_unscaled_f16_trunk_gradients_underflow_to_zero():
    m = _f16_arm()
    g, loss = _backward(m, _crit(W))
    trunk = _trunk_mask(m)
    assert torch.isfinite(loss) and loss > 0
    assert torch.isfinite(g).all()
    assert (g[~trunk] != 0).any()                   # the fp32 head still has its gradient
    assert not g[trunk].any()                       # every trunk gradient is exactly zero


def test_static_scale_recovers_the_gradient_bit_for_bit():
    from mauv.amp import LossScaler
    from mauv.engine import root_state
    from mauv.optim import FusedAdam
    from mauv.train import mc_train_step
    one = _f16_arm()
    g_one, _ = _backward(one, _crit(1.0))           # w = 1, no scaling
    trunk = _trunk_mask(one)
    assert torch.isfinite(g_one).all() and (g_one[trunk] != 0).any()
    m = _f16_arm()
    scaler = LossScaler(init_scale=S, dynamic=False)
    g_s, loss = _backward(m, _crit(W), scaler=scaler)
    diff = (g_s != g_one)
    print(f"scaled w=2^-30 S=2^30 vs w=1: {int(diff.sum())} of {g_s.numel()} arena elements "
          f"differ ({int((diff & trunk).sum())} in the trunks)")
    assert torch.equal(g_s, g_one)
    # the step: through the training loop's step, the trunks move
    root_state(m).arena.flat.zero_()
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    opt = FusedAdam(m.parameters(), lr=LR, loss_scale=scaler)
    x, b, s, y = _batch(10, "ok")
    root_state(m).offset = 0
    r = mc_train_step(m, (x, b, s), y, _crit(W), opt, 2, 2, 0.0)
    assert bool(r["ok_loss"]) and bool(r["stepped"]) and float(r["loss_scale"]) == S
    assert torch.equal(r["loss"], loss)             # reported unscaled
    moved = [n for n, p in m.named_parameters()
             if n.split(".")[0].endswith("_feat") and not torch.equal(p.detach(), before[n])]
    trunks = {n.split(".")[0] for n in before if n.split(".")[0].endswith("_feat")}
    assert {n.split(".")[0] for n in moved} == trunks and len(trunks) == 3
    # ... and without the scaler they do not: the same step on the underflowed gradients
    m0 = _f16_arm()
    before0 = {n: p.detach().clone() for n, p in m0.named_parameters()}
    opt0 = FusedAdam(m0.parameters(), lr=LR)
    root_state(m0).offset = 0
    r0 = mc_train_step(m0, (x, b, s), y, _crit(W), opt0, 2, 2, 0.0)
    assert bool(r0["stepped"])
    assert all(torch.equal(p.detach(), before0[n]) for n, p in m0.named_parameters()
               if n.split(".")[0].endswith("_feat"))


def test_f16_trunk_cosine_with_and_without_scaling_is_printed():
    """Measured, not judged: cos(f16 trunk gradient, fp32-trunk gradient) on the same weights,
    batch and MC samples, unscaled and at scale 2^16."""
    from mauv.amp import LossScaler
    crit = torch.nn.CrossEntropyLoss()
    ref_m = _f16_arm(torch.float32)
    ref, _ = _backward(ref_m, crit, kl_w=1e-3)
    trunk = _trunk_mask(ref_m)
    ref = ref[trunk].double()
    for name, scale in (("no scaler", None), ("scale 2^16", 2.0 ** 16)):
        scaler = None if scale is None else LossScaler(init_scale=scale, dynamic=False)
        g, _ = _backward(_f16_arm(), crit, kl_w=1e-3, scaler=scaler)
        g = g[trunk].double() / (scale or 1.0)
        finite = bool(torch.isfinite(g).all())
        cos = float((g * ref).sum() / (g.norm() * ref.norm())) if finite else float("nan")
        zeros = int((g == 0).sum())
        print(f"f16 whole-trunk cosine vs fp32 trunks, {name}: {cos:.6f} "
              f"(finite {finite}, exact zeros {zeros} of {g.numel()})")
    assert torch.isfinite(ref).all()
