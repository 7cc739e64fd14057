"""Global-norm gradient clipping through the training step (mauv.train.mc_train_step with
``FusedAdam(max_grad_norm=c)``) on the tri-modal model at the sizes of
tests/test_step_gate_gpu.py (B = 2, 64 px, num_mc = 2, 7 classes).

The gated arm (the norm rides on the non-finite scan, the gate forms the coefficient, the Adam
kernel multiplies as it loads) is held against the host-decided arm (``step()``: scan, clip in
place, update) on the same weights, batches, seed and MC offsets: same decisions, bit-identical
parameters and norms.  ``c`` is half the first step's unclipped norm, read once from a third
model with the option off, so clipping is active; the first norm is within 1 fp32 ulp of the
float64 norm of that model's cloned arena (the bar of tests/test_gradclip_kernel_gpu.py).  From
the second step on the gated arm makes no synchronising call, also across a reassignment of
``max_grad_norm``.  A NaN gradient skips the step, keeps the arena and reads NaN;
``mauv.optim.clip_grad_norm_`` on the model returns the same norm and scales the arena."""
import copy

import numpy as np
import pytest
import torch

from tests.test_step_gate_gpu import _model, _batch, _nan_into_head_grad

pytestmark = pytest.mark.gpu

SEED = 0x5EED_C11B      # the engine seed of every arm (the MC samples follow seed and offset)
LR, WD = 1e-3, 1e-5


def _arm(seed=0):
    from mauv.engine import root_state
    m = _model(seed)
    root_state(m).seed = SEED
    return m


def _norm64(flat):
    """(float64 L2 norm rounded once to fp32, its ulp) of a device fp32 vector."""
    x = flat.detach().cpu().numpy().astype(np.float64)
    ref = np.float32(np.sqrt(np.sum(x * x)))
    return ref, float(np.spacing(ref))


def _backward(model, i, seed0=10):
    """The loss and backward of step ``i`` outside the loop: the arena holds its gradient."""
    from mauv.engine import root_state
    from mauv.train import mc_loss
    x, b, s, y = _batch(seed0 + i, "ok")
    st = root_state(model)
    st.offset = 1000 * i
    mc_loss(model, (x, b, s), y, torch.nn.CrossEntropyLoss(), 2, 2, 1e-3)[0].backward()
    return st.arena.flat


@pytest.fixture(scope="module")
def first():
    """The third model, option off: (its arena after the first backward, cloned; the float64
    norm of that clone as fp32; its ulp)."""
    m = _arm()
    g = _backward(m, 0).clone()
    ref, ulp = _norm64(g)
    assert np.isfinite(ref) and ref > 0
    return g, ref, ulp


def _run(model, opt, steps, sync_check_from=None, seed0=10):
    from mauv.engine import root_state
    from mauv.train import mc_train_step
    crit = torch.nn.CrossEntropyLoss()
    st = root_state(model)
    out = []
    for i in steps:
        x, b, s, y = _batch(seed0 + i, "ok")
        st.offset = 1000 * i
        if sync_check_from is not None and i >= sync_check_from:
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode("error")
        try:
            r = mc_train_step(model, (x, b, s), y, crit, opt, 2, 2, 1e-3)
        finally:
            torch.cuda.set_sync_debug_mode(0)
        out.append(r)
    torch.cuda.synchronize()
    return out


def _same_params(a, b):
    bad = [n for (n, p), q in zip(a.named_parameters(), b.parameters())
           if not torch.equal(p.detach(), q.detach())]
    assert not bad, bad[:5]


def test_gated_clip_equals_host_decided_clip(first, monkeypatch):
    import mauv.train as T
    from mauv.optim import FusedAdam, G_CLIP_COEF, G_STEP
    _, ref, ulp = first
    c = float(ref) / 2
    gat, host = _arm(), _arm()
    opt_g = FusedAdam(gat.parameters(), lr=LR, weight_decay=WD, max_grad_norm=c)
    opt_h = FusedAdam(host.parameters(), lr=LR, weight_decay=WD, max_grad_norm=c)
    r_g = _run(gat, opt_g, range(4), sync_check_from=1)
    monkeypatch.setattr(T, "_step_gate", lambda *a: None)       # the host-decided path
    r_h = _run(host, opt_h, range(4))
    monkeypatch.undo()
    assert all("ok_loss" in r for r in r_g) and all("ok_loss" not in r for r in r_h)
    assert [bool(r["stepped"]) for r in r_g] == [bool(r["stepped"]) for r in r_h] == [True] * 4
    n_g = [r["grad_norm"].cpu().numpy() for r in r_g]
    n_h = [r["grad_norm"].cpu().numpy() for r in r_h]
    print("grad norms", [float(v) for v in n_g], "c", c, "ref", float(ref))
    for a, b in zip(n_g, n_h):
        assert a.dtype == np.float32 and a.shape == ()
        assert a.view(np.int32) == b.view(np.int32)
        assert a > c                                               # clipping was active
    assert abs(float(n_g[0]) - float(ref)) <= ulp
    _same_params(host, gat)
    last = opt_g.last_grad_norm
    assert last.is_cuda and last.shape == () and last.dtype == torch.float32
    assert last.cpu().numpy().view(np.int32) == n_g[3].view(np.int32)
    gate = opt_g._gate.cpu().numpy()
    assert gate[G_STEP] == 4 and 0 < gate.view(np.float32)[G_CLIP_COEF] < 1
    assert {float(v["step"]) for v in opt_g.state_dict()["state"].values()} == {4.0}


def test_option_reassigned_mid_run_without_a_sync(first):
    """Two clipped steps; then ``max_grad_norm = None``: the next steps follow a twin that
    starts from that state and never clips, bit for bit, with no synchronising call; setting the
    option again clips again, still without one."""
    from mauv.optim import FusedAdam
    from mauv.engine import root_state
    c = float(first[1]) / 2
    a = _arm()
    opt_a = FusedAdam(a.parameters(), lr=LR, weight_decay=WD, max_grad_norm=c)
    _run(a, opt_a, range(2))
    d = _arm(1)
    d.load_state_dict(a.state_dict())
    opt_d = FusedAdam(d.parameters(), lr=LR, weight_decay=WD)
    opt_d.load_state_dict(copy.deepcopy(opt_a.state_dict()))   # (torch's load aliases tensors)
    _same_params(a, d)
    opt_a.max_grad_norm = None
    r_a = _run(a, opt_a, range(2, 4), sync_check_from=2)
    r_d = _run(d, opt_d, range(2, 4))
    assert all("grad_norm" not in r for r in r_a + r_d) and opt_a.last_grad_norm is None
    assert all(bool(r["stepped"]) for r in r_a + r_d)
    _same_params(a, d)
    before = [p.detach().clone() for p in a.parameters()]
    opt_a.max_grad_norm = c / 4
    r = _run(a, opt_a, [4], sync_check_from=4)[0]
    flat = _backward(d, 4)                       # the twin's gradient of the same step
    ref, ulp = _norm64(flat)
    assert abs(float(r["grad_norm"]) - float(ref)) <= ulp and bool(r["stepped"])
    assert any(not torch.equal(p.detach(), q) for p, q in zip(a.parameters(), before))
    assert (root_state(a).arena.flat == 0).all()


def test_nan_gradient_skips_the_clipped_step(first, monkeypatch):
    import mauv.train as T
    from mauv.optim import FusedAdam, G_POISONED, G_SKIP_GRAD, G_STEP
    from mauv.engine import root_state
    c = float(first[1]) / 2
    m = _arm()
    opt = FusedAdam(m.parameters(), lr=LR, weight_decay=WD, max_grad_norm=c)
    state = {"on": False}
    orig = T._scan_grad_norm

    def scan(model, optimizer, gate):            # the NaN arrives before the fused scan
        if state["on"]:
            _nan_into_head_grad(model)
        return orig(model, optimizer, gate)
    monkeypatch.setattr(T, "_scan_grad_norm", scan)
    r0 = _run(m, opt, [0])[0]
    assert bool(r0["stepped"]) and float(r0["grad_norm"]) > c
    before = [p.detach().clone() for p in m.parameters()]
    state["on"] = True
    r1 = _run(m, opt, [1], sync_check_from=1)[0]
    state["on"] = False
    assert bool(r1["ok_loss"]) and not bool(r1["stepped"])
    assert torch.isnan(r1["grad_norm"]) and torch.isnan(opt.last_grad_norm)
    for p, q in zip(m.parameters(), before):
        assert torch.equal(p.detach(), q)
    flat = root_state(m).arena.flat              # kept: the NaN and the batch's gradients
    assert torch.isnan(flat).sum() == 1 and (torch.nan_to_num(flat) != 0).any()
    gate = opt._gate.cpu()
    assert (int(gate[G_STEP]), int(gate[G_POISONED]), int(gate[G_SKIP_GRAD])) == (1, 1, 1)


def test_clip_grad_norm_function_on_the_model(first):
    from mauv.optim import clip_grad_norm_
    from mauv.engine import root_state
    g0, ref, ulp = first
    c = float(ref) / 2
    m = _arm()
    flat = _backward(m, 0)
    assert torch.equal(flat, g0)                 # the third model's gradient, bit for bit
    total = clip_grad_norm_(m, c)                # (builds and caches the span table)
    assert total.shape == () and total.dtype == torch.float32 and total.is_cuda
    assert abs(float(total) - float(ref)) <= ulp
    coef = np.float32(min(1.0, float(np.float32(c)) / (float(total) + 1e-6)))
    want = g0.cpu().numpy() * coef
    assert want.dtype == np.float32 and 0.49 < coef < 0.51
    assert np.array_equal(flat.cpu().numpy().view(np.int32), want.view(np.int32))
    # cached: no synchronising call, for a parameter list as for the model; inf norm likewise
    flat.copy_(g0)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = clip_grad_norm_(m.parameters(), c, norm_type=2.0)
        flat.copy_(g0)
        top = clip_grad_norm_(m, 1e30, norm_type=float("inf"))
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert again.cpu().numpy().view(np.int32) == total.cpu().numpy().view(np.int32)
    assert float(top) == float(g0.abs().max()) and torch.equal(flat, g0)
    root_state(m).arena.flat.zero_()
