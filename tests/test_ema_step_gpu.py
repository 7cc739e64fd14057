"""The weight EMA through the training step (mauv.train.mc_train_step with
``FusedAdam(ema_decay=d)``) on the tri-modal model at the sizes of tests/test_gradclip_step_gpu.py
(B = 2, 64 px, num_mc = 2, 7 classes), on a pool of three models returned to the same weights for
every case (tests/test_accum_step_gpu.py).

(1) Six gated steps, one of them with a NaN loss, against a twin stepped by the same FusedAdam
    without the option and a ``torch.optim.swa_utils.AveragedModel`` with
    ``get_ema_multi_avg_fn(0.9)`` over its parameters, updated only after the steps that ran: the
    parameters agree bit for bit, the shadows within the bar of tests/test_ema_kernel_gpu.py (3),
    4 units of 2^-24 of |e| + w (|p| + |e|), summed over the updates (the first one copies on
    both sides: no error).
(2) The host-decided arm (``step()`` + ``mauv_ema_update``) gives the gated arm's shadows, bit
    for bit.
(3) ``grad_accumulation=3``: the shadows move once per window.
(4) ``loss_scale="dynamic"``: an induced overflow moves nothing.
(5) ``averaged()``: the logits inside differ, and are back bit for bit after it; a step inside
    raises.
(6) ``state_dict()`` -> a new optimizer -> ``load_state_dict`` continues with identical bits,
    ``ema_updates`` included; the dict loads into torch.optim.Adam.
(7) With the option off no ``"ema"`` key exists and a step equals mauv_adam_step_ex_accum called
    directly on a twin's tensors, bit for bit."""
import copy
import ctypes

import numpy as np
import pytest
import torch
from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn

from tests.test_accum_step_gpu import _Pool, _micro
from tests.test_gradclip_step_gpu import LR, WD, _backward, _same_params
from tests.test_step_gate_gpu import _batch, _nan_into_head_grad

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
DECAY = 0.9


@pytest.fixture(scope="module")
def pool():
    return _Pool()


def _opt(model, **kw):
    from mauv.optim import FusedAdam
    return FusedAdam(model.parameters(), lr=LR, weight_decay=WD, **kw)


def _shadows(opt):
    return [e.clone() for _, e in opt.ema_parameters()]


def _same_tensors(a, b):
    assert len(a) == len(b) and len(a) > 0
    bad = [i for i, (x, y) in enumerate(zip(a, b)) if not torch.equal(x, y)]
    assert not bad, bad[:5]


class _Bag(torch.nn.Module):
    """The very parameter objects of a model, and nothing else, for AveragedModel to copy."""

    def __init__(self, params):
        super().__init__()
        self.ps = torch.nn.ParameterList(params)


# ------------------------------------------------------------------------------------- (1)
def test_gated_ema_equals_the_averaged_model_loop(pool):
    a, b = pool.fresh(2)
    opt_a, opt_b = _opt(a, ema_decay=DECAY), _opt(b)
    bag = _Bag([p for p in b.parameters() if p.requires_grad])
    avg = AveragedModel(bag, multi_avg_fn=get_ema_multi_avg_fn(DECAY))
    # the device's weight (include/mauv.h): (float)(1.0 - (double)(float)decay)
    w = float(np.float32(1.0 - float(np.float32(DECAY))))
    kinds = ["ok", "ok", "nan_loss", "ok", "ok", "ok"]
    tol, restated = None, []
    for i, kind in enumerate(kinds):
        r_a = _micro(a, opt_a, i, kind, no_sync=i >= 2)   # (the caches are built by then)
        r_b = _micro(b, opt_b, i, kind)
        ran = bool(r_b["stepped"])
        assert bool(r_a["stepped"]) is ran is (kind == "ok")
        if not ran:
            continue
        prev = [e.detach().clone() for e in avg.module.parameters()]
        first = int(avg.n_averaged) == 0
        avg.update_parameters(bag)
        if first:
            tol = [torch.zeros_like(e, dtype=torch.float64) for e in prev]
            continue
        # the bar of tests/test_ema_kernel_gpu.py (3) for this update: 4x what the one-fp32-
        # operation restatement fl(fma(w, fl(p - e), e)) errs against float64, floored at 4 units
        scales, units = [], 0.0
        for e32, p in zip(prev, bag.parameters()):
            e, q = e32.double(), p.detach().double()
            scale = e.abs() + w * (q.abs() + e.abs())
            want = e + w * (q - e)
            r32 = (w * (p.detach() - e32).double() + e).float().double()
            ok = scale > 0
            if bool(ok.any()):
                units = max(units, float(((r32 - want).abs()[ok] / (U * scale[ok])).max()))
            scales.append(scale)
        restated.append(units)
        for t, scale in zip(tol, scales):
            t += 4.0 * max(1.0, units) * U * scale
    _same_params(a, b)
    pairs = opt_a.ema_parameters()
    assert opt_a.ema_updates == 5 == int(avg.n_averaged) and len(pairs) == len(tol)
    worst = 0.0
    for (p, e), q, ref, t in zip(pairs, bag.parameters(), avg.module.parameters(), tol):
        assert p.shape == q.shape
        err = (e.double() - ref.detach().double()).abs()
        worst = max(worst, float((err / t.clamp_min(1e-300)).max()))
    print(f"ema vs AveragedModel: fp32 restatement {restated} units per update; worst error "
          f"{worst:.3f} of the accumulated bar")
    for (p, e), ref, t in zip(pairs, avg.module.parameters(), tol):
        err = (e.double() - ref.detach().double()).abs()
        assert bool((err <= t).all())
        assert not torch.equal(e, p)                       # an average, not the weights
    assert "ema" not in opt_b.state[next(iter(opt_b.state))]


# ------------------------------------------------------------------------------------- (2)
def test_host_decided_arm_gives_the_gated_shadows(pool, monkeypatch):
    import mauv.train as T
    gat, host = pool.fresh(2)
    opt_g, opt_h = _opt(gat, ema_decay=DECAY, ema_warmup=True), \
        _opt(host, ema_decay=DECAY, ema_warmup=True)
    for i in range(4):
        assert "ok_loss" in _micro(gat, opt_g, i)
    monkeypatch.setattr(T, "_step_gate", lambda *a: None)           # the host-decided path
    for i in range(4):
        assert "ok_loss" not in _micro(host, opt_h, i)
    monkeypatch.undo()
    _same_params(gat, host)
    _same_tensors(_shadows(opt_g), _shadows(opt_h))
    assert opt_g.ema_updates == opt_h.ema_updates == 4


# ------------------------------------------------------------------------------------- (3)
def test_shadows_move_once_per_accumulation_window(pool):
    m, = pool.fresh(1)
    opt = _opt(m, ema_decay=DECAY, grad_accumulation=3)
    snaps = []
    for i in range(6):
        r = _micro(m, opt, i)
        assert r["closed"] is (i % 3 == 2)
        snaps.append(_shadows(opt))
        if i == 2:                                        # the first update copies
            _same_tensors(snaps[2], [p.detach() for p, _ in opt.ema_parameters()])
    assert snaps[0] == snaps[1] == []                     # created with the first step
    _same_tensors(snaps[2], snaps[3])
    _same_tensors(snaps[3], snaps[4])
    assert not any(torch.equal(x, y) for x, y in zip(snaps[4], snaps[5]))
    assert opt.ema_updates == 2


# ------------------------------------------------------------------------------------- (4)
def test_an_overflow_under_dynamic_loss_scaling_moves_nothing(pool, monkeypatch):
    import mauv.train as T
    m, = pool.fresh(1)
    opt = _opt(m, ema_decay=DECAY, loss_scale="dynamic")
    assert bool(_micro(m, opt, 0)["stepped"]) and bool(_micro(m, opt, 1)["stepped"])
    shadows, params = _shadows(opt), [p.detach().clone() for p in m.parameters()]
    orig = T._count_nonfinite

    def count(model, counter):
        _nan_into_head_grad(model)
        return orig(model, counter)
    monkeypatch.setattr(T, "_count_nonfinite", count)
    r = _micro(m, opt, 2)
    monkeypatch.undo()
    assert not bool(r["stepped"]) and bool(r["ok_loss"])
    _same_tensors(shadows, _shadows(opt))
    _same_tensors(params, [p.detach() for p in m.parameters()])
    assert opt.ema_updates == 2
    assert bool(_micro(m, opt, 3)["stepped"]) and opt.ema_updates == 3


# ------------------------------------------------------------------------------------- (5)
def _logits(model):
    from mauv.engine import root_state
    from mauv.train import mc_logits
    x, b, s, _ = _batch(99, "ok")
    root_state(model).offset = 5000
    with torch.no_grad():
        return mc_logits(model, 2, x, b, s).detach().float().clone()


def test_averaged_swaps_in_and_back_bit_for_bit(pool):
    m, = pool.fresh(1)
    opt = _opt(m, ema_decay=DECAY)
    for i in range(3):
        _micro(m, opt, i)
    m.eval()
    live = [p.detach().clone() for p in m.parameters()]
    shadows = _shadows(opt)
    ptrs = [p.data_ptr() for p in m.parameters()]
    outside = _logits(m)
    with opt.averaged():
        inside = _logits(m)
        _same_tensors(shadows, [p.detach() for p, _ in opt.ema_parameters()])
        for call in (opt.step, opt.state_dict, lambda: opt.step_gated(opt._gate)):
            with pytest.raises(RuntimeError, match="averaged"):
                call()
    assert torch.isfinite(inside).all() and not torch.equal(inside, outside)
    assert torch.equal(_logits(m), outside)
    _same_tensors(live, [p.detach() for p in m.parameters()])
    _same_tensors(shadows, _shadows(opt))
    assert ptrs == [p.data_ptr() for p in m.parameters()]
    m.train()
    assert bool(_micro(m, opt, 3)["stepped"]) and opt.ema_updates == 4


# ------------------------------------------------------------------------------------- (6)
def test_state_dict_round_trip_continues_with_identical_bits(pool):
    a, d = pool.fresh(2)
    opt_a = _opt(a, ema_decay=DECAY, ema_warmup=True)
    for i in range(3):
        _micro(a, opt_a, i)
    sd = copy.deepcopy(opt_a.state_dict())                 # (torch's load aliases tensors)
    assert sd["ema_updates"] == 3 and all("ema" in v for v in sd["state"].values())
    d.load_state_dict(a.state_dict())
    opt_d = _opt(d, ema_decay=DECAY, ema_warmup=True)
    opt_d.load_state_dict(sd)
    assert opt_d.ema_updates == 3
    _same_tensors(_shadows(opt_a), _shadows(opt_d))
    for i in range(3, 5):
        _micro(a, opt_a, i)
        _micro(d, opt_d, i)
    _same_params(a, d)
    _same_tensors(_shadows(opt_a), _shadows(opt_d))
    assert opt_a.ema_updates == opt_d.ema_updates == 5
    ref = torch.optim.Adam(d.parameters(), lr=LR, weight_decay=WD)
    ref.load_state_dict(opt_a.state_dict())
    assert {float(v["step"]) for v in ref.state_dict()["state"].values()} == {5.0}


# ------------------------------------------------------------------------------------- (7)
def test_ema_off_is_the_accum_entry_and_keeps_no_shadow(pool):
    from mauv import ops
    from mauv._lib import lib, check, MauvAdamGroup
    from mauv.engine import root_state
    from mauv.optim import GATE_WORDS, G_OK_LOSS
    a, b = pool.fresh(2)
    opt = _opt(a)
    assert bool(_micro(a, opt, 0)["stepped"])
    assert opt.ema_parameters() == [] and not any("ema" in st for st in opt.state.values())
    assert set(opt.state_dict()) == {"state", "param_groups"}
    # the twin: the same backward outside the loop, then the entry itself on a hand-built table
    _backward(b, 0)
    ps = [p for p in b.parameters() if p.requires_grad]
    ms, vs = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps]
    rows = np.array([(p.data_ptr(), p.grad.data_ptr(), m.data_ptr(), v.data_ptr(), 0, p.numel(), 0)
                     for p, m, v in zip(ps, ms, vs)], dtype=np.int64)
    tab = torch.from_numpy(rows).cuda()
    gate = torch.zeros(GATE_WORDS, dtype=torch.int32, device="cuda")
    gate[G_OK_LOSS] = 1
    grp = (MauvAdamGroup * 1)()
    grp[0].lr, grp[0].beta1, grp[0].beta2, grp[0].eps, grp[0].weight_decay = LR, 0.9, 0.999, 1e-8, WD
    check(lib.mauv_adam_step_ex_accum(tab.data_ptr(), len(ps), ctypes.addressof(grp), 1,
                                      gate.data_ptr(), None, None, ops.stream()),
          "adam_step_ex_accum")
    torch.cuda.synchronize()
    _same_params(a, b)
    for p, m, v in zip([p for p in a.parameters() if p.requires_grad], ms, vs):
        assert torch.equal(opt.state[p]["exp_avg"], m) and torch.equal(opt.state[p]["exp_avg_sq"], v)
    assert not root_state(b).arena.flat.any()
