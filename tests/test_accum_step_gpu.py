"""Gradient accumulation through the training step (mauv.train.mc_train_step with
``FusedAdam(grad_accumulation=K)``) on the tri-modal model at the sizes of
tests/test_step_gate_gpu.py (B = 2, 64 px, num_mc = 2, 7 classes); engine seed and MC offsets are
fixed per micro-batch, as in tests/test_gradclip_step_gpu.py.

K = 2 and K = 3 over 6 micro-batches, with ``max_grad_norm`` set and unset.  The gated arm (one
decision per window on the device, the 1 / K multiply as the Adam kernel loads the gradient) is
held against a manual arm on the same weights — the backward passes outside the loop, then
``arena.flat.mul_(float32(1 / m))``, then ``FusedAdam.step()`` — and against the host-decided arm
(``_step_gate`` patched to None): the same decisions and bit-identical parameters after every
window.  From the second window on the gated arm makes no synchronising call.  A NaN input inside
a window drops that window only.  With f16 trunks and ``loss_scale="dynamic"`` the scale reported
is constant inside each window and moves between windows.  ``train_multimodal_model`` over a
5-batch loader with K = 2 closes three windows (the last one partial) and leaves a zero arena.

``c`` is a quarter of the first micro-batch's gradient norm, so clipping is active in every
window (asserted).  The three models of the module are built once and put back to the same state
for every case."""
import copy
import os

import numpy as np
import pytest
import torch

from tests.test_step_gate_gpu import _batch
from tests.test_gradclip_step_gpu import _arm, _backward, _norm64, _same_params, SEED, LR, WD

pytestmark = pytest.mark.gpu

N_MICRO = 6


class _Pool:
    """Three models on the same weights, returned to them (parameters, buffers, a zero arena,
    the engine seed) for every case: building one costs more than a whole case."""

    def __init__(self):
        from mauv.engine import root_state
        self.models = [_arm() for _ in range(3)]
        self.precision = root_state(self.models[0]).precision
        self.state = copy.deepcopy(self.models[0].state_dict())

    def fresh(self, n=3):
        from mauv.engine import root_state, set_precision
        for m in self.models[:n]:
            set_precision(m, self.precision)
            m.load_state_dict(self.state)
            st = root_state(m)
            st.seed, st.offset = SEED, 0
            if st.arena is not None:
                st.arena.flat.zero_()
            m.train()
        return self.models[:n]


@pytest.fixture(scope="module")
def pool():
    return _Pool()


@pytest.fixture(scope="module")
def first_norm(pool):
    """The fp32 gradient norm of micro-batch 0 on the pool's weights."""
    from mauv.engine import root_state
    m, = pool.fresh(1)
    ref, _ = _norm64(_backward(m, 0))
    root_state(m).arena.flat.zero_()
    assert np.isfinite(ref) and ref > 0
    return float(ref)


def _micro(model, opt, i, kind="ok", close=None, no_sync=False, crit=None, kl_w=1e-3):
    from mauv.engine import root_state
    from mauv.train import mc_train_step
    x, b, s, y = _batch(10 + i, kind)
    root_state(model).offset = 1000 * i
    if no_sync:
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
    try:
        return mc_train_step(model, (x, b, s), y, crit or torch.nn.CrossEntropyLoss(), opt, 2, 2,
                             kl_w, close_window=close)
    finally:
        torch.cuda.set_sync_debug_mode(0)


def _manual_window(model, opt, idx):
    """The manual arm: the window's backward passes outside the loop, one multiply of the
    arena by float32(1 / m), the ungated step, zero_grad."""
    from mauv.engine import root_state
    for i in idx:
        flat = _backward(model, i)
    flat.mul_(float(np.float32(1.0 / len(idx))))
    opt.step()
    root_state(model).arena.flat.zero_()


@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
@pytest.mark.parametrize("K", [2, 3])
def test_gated_windows_equal_the_manual_and_the_host_decided_arm(pool, first_norm, K, clip,
                                                                 monkeypatch):
    import mauv.train as T
    from mauv.engine import root_state
    from mauv.optim import FusedAdam, G_STEP, A_WINDOWS, A_DROPPED, A_MICRO
    gat, man, host = pool.fresh()
    c = first_norm / 4 if clip else None
    opts = [FusedAdam(m.parameters(), lr=LR, weight_decay=WD, max_grad_norm=c) for m in (gat, man)]
    opt_g, opt_m = opts
    opt_g.grad_accumulation = K
    opt_h = FusedAdam(host.parameters(), lr=LR, weight_decay=WD, max_grad_norm=c,
                      grad_accumulation=K)
    windows = [list(range(w, w + K)) for w in range(0, N_MICRO, K)]
    norms = []
    for w, idx in enumerate(windows):
        r_g = [_micro(gat, opt_g, i, no_sync=w >= 1) for i in idx]
        monkeypatch.setattr(T, "_step_gate", lambda *a: None)       # the host-decided path
        r_h = [_micro(host, opt_h, i) for i in idx]
        monkeypatch.undo()
        _manual_window(man, opt_m, idx)
        torch.cuda.synchronize()
        closes = [False] * (K - 1) + [True]
        assert [r["closed"] for r in r_g] == [r["closed"] for r in r_h] == closes
        assert [bool(r["stepped"]) for r in r_g] == [bool(r["stepped"]) for r in r_h] == closes
        assert all("ok_loss" in r and bool(r["ok_loss"]) for r in r_g)
        assert all("ok_loss" not in r for r in r_h)
        assert all(torch.equal(a["loss"], b["loss"]) for a, b in zip(r_g, r_h))
        assert ["grad_norm" in r for r in r_g] == [clip and cl for cl in closes]
        if clip:
            n_g, n_h = float(r_g[-1]["grad_norm"]), float(r_h[-1]["grad_norm"])
            n_m = float(opt_m.last_grad_norm)
            print(f"K={K} window {w}: grad norm gated {n_g!r} host-decided {n_h!r} "
                  f"manual {n_m!r} c {c!r}")
            assert n_g > c                                           # clipping was active
            norms.append((n_g, n_h, n_m))
        _same_params(man, gat)
        _same_params(host, gat)
        assert (root_state(gat).arena.flat == 0).all()
    acc = opt_g._accum.cpu().numpy()
    assert (acc[A_MICRO], acc[A_WINDOWS], acc[A_DROPPED]) == (0, len(windows), 0)
    assert int(opt_g._gate[G_STEP]) == len(windows)
    assert {float(v["step"]) for v in opt_g.state_dict()["state"].values()} == {float(len(windows))}


def test_a_nan_batch_inside_a_window_drops_that_window_only(pool):
    from mauv.engine import root_state
    from mauv.optim import (FusedAdam, G_STEP, G_SKIP_LOSS, G_SKIP_GRAD, G_POISONED, A_WINDOWS,
                            A_DROPPED, A_MICRO, A_BAD_LOSS)
    gat, man = pool.fresh(2)
    opt_g = FusedAdam(gat.parameters(), lr=LR, weight_decay=WD, grad_accumulation=2)
    opt_m = FusedAdam(man.parameters(), lr=LR, weight_decay=WD)
    before = [p.detach().clone() for p in gat.parameters()]
    r0 = _micro(gat, opt_g, 0)
    r1 = _micro(gat, opt_g, 1, "nan_loss")
    torch.cuda.synchronize()
    assert (r0["closed"], r1["closed"]) == (False, True)
    assert bool(r0["ok_loss"]) and not bool(r1["ok_loss"])
    assert not bool(r0["stepped"]) and not bool(r1["stepped"])
    for p, q in zip(gat.parameters(), before):
        assert torch.equal(p.detach(), q)
    assert (root_state(gat).arena.flat == 0).all()                   # taken back out
    gate, acc = opt_g._gate.cpu().numpy(), opt_g._accum.cpu().numpy()
    assert (gate[G_STEP], gate[G_SKIP_LOSS], gate[G_SKIP_GRAD], gate[G_POISONED]) == (0, 1, 0, 0)
    assert (acc[A_MICRO], acc[A_BAD_LOSS], acc[A_WINDOWS], acc[A_DROPPED]) == (0, 0, 1, 1)
    # the next window steps, as if the dropped one had not been
    r2 = _micro(gat, opt_g, 2, no_sync=True)
    r3 = _micro(gat, opt_g, 3, no_sync=True)
    _manual_window(man, opt_m, [2, 3])
    torch.cuda.synchronize()
    assert (r2["closed"], r3["closed"]) == (False, True)
    assert not bool(r2["stepped"]) and bool(r3["stepped"])
    _same_params(man, gat)
    gate, acc = opt_g._gate.cpu().numpy(), opt_g._accum.cpu().numpy()
    assert (gate[G_STEP], gate[G_SKIP_LOSS]) == (1, 1)
    assert (acc[A_WINDOWS], acc[A_DROPPED]) == (2, 1)
    # a bad loss on the FIRST micro-batch of a window drops it just the same
    before = [p.detach().clone() for p in gat.parameters()]
    r4 = _micro(gat, opt_g, 4, "nan_loss")
    r5 = _micro(gat, opt_g, 5)
    torch.cuda.synchronize()
    assert not bool(r4["ok_loss"]) and bool(r5["ok_loss"]) and not bool(r5["stepped"])
    for p, q in zip(gat.parameters(), before):
        assert torch.equal(p.detach(), q)
    assert (root_state(gat).arena.flat == 0).all()
    assert tuple(opt_g._accum.cpu().numpy()[[A_WINDOWS, A_DROPPED]]) == (3, 2)


def test_zero_grad_abandons_the_open_window(pool):
    from mauv.engine import root_state
    from mauv.optim import FusedAdam, A_WINDOWS, A_MICRO
    gat, man = pool.fresh(2)
    opt_g = FusedAdam(gat.parameters(), lr=LR, weight_decay=WD, grad_accumulation=2)
    opt_m = FusedAdam(man.parameters(), lr=LR, weight_decay=WD)
    _micro(gat, opt_g, 0)
    assert int(opt_g._accum[A_MICRO]) == 1 and opt_g._accum_micro == 1
    opt_g.zero_grad()
    assert int(opt_g._accum[A_MICRO]) == 0 and opt_g._accum_micro == 0
    rs = [_micro(gat, opt_g, i) for i in (1, 2)]
    _manual_window(man, opt_m, [1, 2])
    torch.cuda.synchronize()
    assert [r["closed"] for r in rs] == [False, True] and bool(rs[1]["stepped"])
    _same_params(man, gat)
    assert int(opt_g._accum[A_WINDOWS]) == 1
    assert (root_state(gat).arena.flat == 0).all()


def test_f16_dynamic_loss_scale_is_constant_inside_a_window(pool):
    from mauv.amp import LossScaler
    from mauv.engine import set_precision
    from mauv.optim import FusedAdam, A_WINDOWS
    m, = pool.fresh(1)
    set_precision(m, torch.float16)
    ls = LossScaler(init_scale=2.0 ** 10, growth_interval=1)
    opt = FusedAdam(m.parameters(), lr=LR, weight_decay=WD, loss_scale=ls, grad_accumulation=2)
    rs = [_micro(m, opt, i, no_sync=i >= 2) for i in range(6)]
    torch.cuda.synchronize()
    scales = [float(r["loss_scale"]) for r in rs]
    stepped = [bool(r["stepped"]) for r in rs]
    print("f16 K=2 loss scales", scales, "stepped", stepped)
    for w in range(3):
        assert scales[2 * w] == scales[2 * w + 1]                    # constant inside a window
        assert not stepped[2 * w]
        # between windows: one growth per stepped window, one backoff per overflowed one
        if w < 2:
            assert scales[2 * w + 2] == scales[2 * w] * (2.0 if stepped[2 * w + 1] else 0.5)
    assert scales[0] == 2.0 ** 10 and any(stepped)
    assert int(opt._accum[A_WINDOWS]) == 3
    sd = ls.state_dict()
    assert sd["scale"] == scales[4] * (2.0 if stepped[5] else 0.5)


def test_train_loop_closes_a_partial_window_on_the_last_batch(pool, tmp_path):
    from mauv.engine import root_state
    from mauv.optim import FusedAdam, G_STEP, A_WINDOWS, A_DROPPED, A_MICRO
    from mauv.train import train_multimodal_model
    from tests.helpers import ListLoader, NullWriter
    m, = pool.fresh(1)
    opt = FusedAdam(m.parameters(), lr=1e-4, grad_accumulation=2)
    batches = []
    for i in range(5):
        x, b, s, y = _batch(40 + i, "ok")
        batches.append({"main_image": x.cpu(), "bathy_image": b.cpu(), "sss_image": s.cpu(),
                        "label": y.cpu(), "patch_bathy": {}, "patch_sss": {}})

    class NoLen(ListLoader):
        def __len__(self):
            raise TypeError("this loader has no length")

    loss, acc = train_multimodal_model(m, NoLen(batches, 2), torch.nn.CrossEntropyLoss(), opt, 1,
                                       "cuda", "multimodal", 2, 2, NullWriter(),
                                       csv_path=os.path.join(str(tmp_path), "t.csv"))
    assert loss > 0 and 0.0 <= acc <= 1.0
    assert (root_state(m).arena.flat == 0).all()                     # no window is left open
    a = opt._accum.cpu().numpy()
    assert (a[A_MICRO], a[A_WINDOWS], a[A_DROPPED]) == (0, 3, 0) and opt._accum_micro == 0
    assert int(opt._gate[G_STEP]) == 3
    assert a.view(np.float32)[2] == 1.0                              # the last window held one
