"""Dynamic loss scaling through the training step (``FusedAdam(loss_scale=...)``,
mauv.amp.LossScaler) on the tri-modal model at the sizes of tests/test_step_gate_gpu.py (B = 2,
64 px, num_mc = 2, 7 classes), fp32 trunks.

* A dynamic scaler (2^8, growing every 2 clean steps) against an arm with no scaler: every scale
  is a power of two and the backward is linear in its upstream scalar, so the parameters after 6
  steps are bit-identical — and with ``max_grad_norm`` set (half the first step's norm: clipping
  is active) so is every reported ``grad_norm``, the norm of the unscaled gradients.
* The gated arm against the host-decided arm (``_step_gate`` patched to None) with an inf written
  into the arena before the scan on two steps: same decisions, the (scale, tracker) sequence of a
  ``torch.amp.GradScaler("cpu")`` driven with the same overflow pattern, bit-identical
  parameters, an all-zero arena after a skipped step, and from the second step on the gated arm
  makes no synchronising call.
* The unimodal loop and the torch idiom (``scaler.scale(loss).backward(); scaler.step(opt);
  scaler.update()``) with a static scale equal the no-scaler run bit for bit.
* Two gloo ranks on one GPU: an inf on rank 0 before the all-reduce makes both ranks skip and
  back off alike."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.test_step_gate_gpu import _model, _batch, _free_port
from tests.test_gradclip_step_gpu import _arm, _same_params
from tests.test_gradclip_step_gpu import first  # noqa: F401  (module fixture: the first step's norm)

pytestmark = pytest.mark.gpu

LR, WD = 1e-3, 1e-5
S0 = 2.0 ** 8


def _inf_into_head_grad(model):
    """An inf in the fusion head's last gradient (a kernel, no host copy)."""
    from mauv.engine import root_state
    from mauv.kl import unwrap
    ar = root_state(unwrap(model)).arena
    ar.flat.narrow(0, ar.offsets[-1], 1).fill_(float("inf"))


class _InjectInf:
    """Write an inf into the arena between the backward and the scan when ``on``: the gated
    path scans in ``_count_nonfinite`` (or, clipping, ``opt.scan_gated``), the host-decided path
    in ``opt.step()``'s own ``scan_gated``."""

    def __init__(self, model, opt):
        import mauv.train as T
        self.T, self.on = T, False
        self.orig_count, scan = T._count_nonfinite, opt.scan_gated

        def count(m, counter):
            if self.on:
                _inf_into_head_grad(m)
            return self.orig_count(m, counter)

        def scan_gated(gate, flat=None):
            if self.on:
                _inf_into_head_grad(model)
            return scan(gate, flat)
        T._count_nonfinite, opt.scan_gated = count, scan_gated

    def close(self):
        self.T._count_nonfinite = self.orig_count


def _run(model, opt, n, bad=(), sync_check_from=None, seed0=10):
    """n steps of mc_train_step -> [(result, scale after, tracker after, arena all zero)]."""
    from mauv.engine import root_state
    from mauv.kl import unwrap
    from mauv.train import mc_train_step
    crit = torch.nn.CrossEntropyLoss()
    st = root_state(unwrap(model))
    inject = _InjectInf(model, opt)
    out = []
    try:
        for i in range(n):
            x, b, s, y = _batch(seed0 + i, "ok")
            st.offset = 1000 * i          # same MC samples in every arm
            inject.on = i in bad
            if sync_check_from is not None and i >= sync_check_from:
                torch.cuda.synchronize()
                torch.cuda.set_sync_debug_mode("error")
            try:
                r = mc_train_step(model, (x, b, s), y, crit, opt, 2, 2, 1e-3)
            finally:
                torch.cuda.set_sync_debug_mode(0)
            ls = opt.loss_scale
            out.append((r, None if ls is None else ls.get_scale(),
                        None if ls is None else ls.get_growth_tracker(),
                        bool((st.arena.flat == 0).all())))
    finally:
        inject.close()
    torch.cuda.synchronize()
    return out


def _grad_scaler_sequence(n, bad, **kw):
    """(scale, tracker) after each step of a torch GradScaler("cpu") fed the overflow pattern."""
    gs = torch.amp.GradScaler("cpu", **kw)
    p = torch.nn.Parameter(torch.zeros(2))
    opt = torch.optim.SGD([p], lr=0.1)
    seq = []
    for i in range(n):
        gs.scale(p.sum()).backward()
        if i in bad:
            p.grad[1] = float("inf")
        gs.step(opt)
        gs.update()
        opt.zero_grad()
        seq.append((gs.get_scale(), gs._get_growth_tracker()))
    return seq


@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
def test_power_of_two_scaling_changes_no_bit(clip, first):  # noqa: F811
    from mauv.amp import LossScaler
    from mauv.optim import FusedAdam
    c = float(first[1]) / 2 if clip else None     # half the first step's norm: clipping is active
    plain, scaled = _arm(), _arm()
    opt_p = FusedAdam(plain.parameters(), lr=LR, weight_decay=WD, max_grad_norm=c)
    opt_s = FusedAdam(scaled.parameters(), lr=LR, weight_decay=WD, max_grad_norm=c,
                      loss_scale=LossScaler(init_scale=S0, growth_interval=2))
    r_p = _run(plain, opt_p, 6)
    r_s = _run(scaled, opt_s, 6, sync_check_from=1)
    assert all("ok_loss" in r for r, *_ in r_p + r_s)            # both arms gated
    assert all(bool(r["stepped"]) for r, *_ in r_p + r_s)
    assert [(s, t) for _, s, t, _ in r_s] == \
        [(S0, 1), (2 * S0, 0), (2 * S0, 1), (4 * S0, 0), (4 * S0, 1), (8 * S0, 0)]
    assert [float(r["loss_scale"]) for r, *_ in r_s] == \
        [S0, S0, 2 * S0, 2 * S0, 4 * S0, 4 * S0]                 # the scale each batch ran with
    assert all("loss_scale" not in r for r, *_ in r_p)
    for (a, *_), (b, *_) in zip(r_p, r_s):                       # reported unscaled
        assert torch.equal(a["loss"], b["loss"]) and torch.equal(a["ce"], b["ce"])
        assert torch.equal(a["scaled_kl"], b["scaled_kl"])
        if clip:
            na, nb = a["grad_norm"].cpu().numpy(), b["grad_norm"].cpu().numpy()
            assert na.view(np.int32) == nb.view(np.int32) and na > c
        else:
            assert "grad_norm" not in a and "grad_norm" not in b
    _same_params(plain, scaled)
    assert opt_s.loss_scale.counters() == (0, 3)
    assert {float(v["step"]) for v in opt_s.state_dict()["state"].values()} == {6.0}
    torch.optim.Adam(scaled.parameters()).load_state_dict(opt_s.state_dict())


def test_gated_arm_equals_host_decided_arm_and_grad_scaler(monkeypatch):
    import mauv.train as T
    from mauv.amp import LossScaler
    from mauv.optim import FusedAdam, G_STEP, G_POISONED, G_SKIP_GRAD
    n, bad = 7, {2, 5}
    kw = dict(init_scale=S0, growth_interval=2)
    gat, host = _arm(), _arm()
    opt_g = FusedAdam(gat.parameters(), lr=LR, weight_decay=WD, loss_scale=LossScaler(**kw))
    opt_h = FusedAdam(host.parameters(), lr=LR, weight_decay=WD, loss_scale=LossScaler(**kw))
    r_g = _run(gat, opt_g, n, bad, sync_check_from=1)
    monkeypatch.setattr(T, "_step_gate", lambda *a: None)       # the host-decided path
    r_h = _run(host, opt_h, n, bad)
    monkeypatch.undo()
    assert all("ok_loss" in r for r, *_ in r_g) and all("ok_loss" not in r for r, *_ in r_h)
    want = [i not in bad for i in range(n)]
    assert [bool(r["stepped"]) for r, *_ in r_g] == want
    assert [bool(r["stepped"]) for r, *_ in r_h] == want
    seq = _grad_scaler_sequence(n, bad, **kw)
    assert seq == [(S0, 1), (2 * S0, 0), (S0, 0), (S0, 1), (2 * S0, 0), (S0, 0), (S0, 1)]
    assert [(s, t) for _, s, t, _ in r_g] == seq
    assert [(s, t) for _, s, t, _ in r_h] == seq
    # the arena is zero after every step, a skipped one included (never "poisoned")
    assert all(z for *_, z in r_g) and all(z for *_, z in r_h)
    _same_params(host, gat)
    for opt in (opt_g, opt_h):
        gate = opt._gate.cpu()
        assert (int(gate[G_STEP]), int(gate[G_POISONED]), int(gate[G_SKIP_GRAD])) == (5, 0, 2)
        assert opt.loss_scale.counters() == (2, 2)
        assert {float(v["step"]) for v in opt.state_dict()["state"].values()} == {5.0}
    moved = _arm()
    assert any(not torch.equal(p.detach(), q.detach())
               for p, q in zip(gat.parameters(), moved.parameters()))


def _image_model(seed=0):
    from mauv.models import define_models, DEFAULT_PRIOR
    from mauv.engine import root_state
    torch.manual_seed(seed)
    m = define_models(None, 7, DEFAULT_PRIOR)["image_model"].cuda()
    root_state(m).seed = 0x5CA1E
    return m


def _image_batches():
    g = torch.Generator().manual_seed(3)
    return [dict(main_image=torch.randn(2, 3, 64, 64, generator=g),
                 label=torch.randint(0, 7, (2,), generator=g)) for _ in range(3)]


def test_unimodal_loop_with_a_static_scale(tmp_path):
    from mauv.optim import FusedAdam
    from mauv.train import train_unimodal_model
    from tests.helpers import ListLoader, NullWriter
    batches, crit = _image_batches(), torch.nn.CrossEntropyLoss()
    res = []
    for name, scale in (("plain", None), ("scaled", 1024.0)):
        m = _image_model()
        opt = FusedAdam(m.parameters(), lr=LR, weight_decay=WD, loss_scale=scale)
        res.append((m, train_unimodal_model(
            m, ListLoader(batches, 2), crit, opt, epoch=1, total_num_epochs=3, num_mc=2,
            sum_writer=NullWriter(), device=torch.device("cuda"), model_type="image",
            csv_path=str(tmp_path / f"{name}.csv"))))
        if scale is not None:
            assert opt.loss_scale.get_scale() == 1024.0 and opt.loss_scale.counters() == (0, 0)
            assert {float(v["step"]) for v in opt.state_dict()["state"].values()} == {3.0}
    (m_p, out_p), (m_s, out_s) = res
    assert out_p == out_s and out_p[1] > 0          # (accuracy, loss): reported unscaled
    _same_params(m_p, m_s)
    fresh = _image_model()
    assert any(not torch.equal(p.detach(), q.detach())
               for p, q in zip(m_s.parameters(), fresh.parameters()))


def test_torch_idiom_with_a_static_scale():
    """``scaler.scale(loss).backward(); scaler.step(opt); scaler.update()`` in a hand-written
    loop against backward / step / zero_grad with no scaler."""
    from mauv.amp import LossScaler
    from mauv.engine import root_state
    from mauv.optim import FusedAdam
    from mauv.train import mc_loss
    batches, crit = _image_batches(), torch.nn.CrossEntropyLoss()
    a, b = _image_model(1), _image_model(1)
    opt_a = FusedAdam(a.parameters(), lr=LR, weight_decay=WD)
    scaler = LossScaler(init_scale=2.0 ** 12, dynamic=False)
    opt_b = FusedAdam(b.parameters(), lr=LR, weight_decay=WD, loss_scale=scaler)
    for i, bt in enumerate(batches):
        x, y = bt["main_image"].cuda(), bt["label"].cuda()
        for m, opt in ((a, opt_a), (b, opt_b)):
            root_state(m).offset = 1000 * i
            loss = mc_loss(m, (x,), y, crit, 2, 2, 1e-3)[0]
            if opt is opt_a:
                loss.backward()
                opt.step()
                opt.zero_grad()
            else:
                scaled = scaler.scale(loss)
                assert float(scaled.detach()) == float(loss.detach()) * 2.0 ** 12
                scaled.backward()
                scaler.step(opt)
                scaler.update()
                assert (root_state(m).arena.flat == 0).all()    # the step consumed them
    _same_params(a, b)
    assert scaler.get_scale() == 2.0 ** 12 and scaler.counters() == (0, 0)
    assert {float(v["step"]) for v in opt_b.state_dict()["state"].values()} == {3.0}


def _worker(rank, world, port, q):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "multimodal-auv_amd")]
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    from mauv.amp import LossScaler
    from mauv.ddp import DistributedMC
    from mauv.optim import FusedAdam
    from mauv.train import mc_train_step
    model = _model()
    ddp = DistributedMC(model)
    opt = FusedAdam(model.parameters(), lr=LR,
                    loss_scale=LossScaler(init_scale=S0, growth_interval=2))
    state = {"on": False}
    orig = ddp.allreduce_grads

    def allreduce():                      # the inf arrives on one rank, before the all-reduce
        if state["on"]:
            _inf_into_head_grad(ddp)
        return orig()
    ddp.allreduce_grads = allreduce
    crit = torch.nn.CrossEntropyLoss()
    out = []
    for i in range(4):
        x, b, s, y = _batch(10 + 100 * rank + i, "ok")
        state["on"] = rank == 0 and i == 1
        r = mc_train_step(ddp, (x, b, s), y, crit, opt, 2, 2, 1e-3)
        out.append((bool(r["ok_loss"]), bool(r["stepped"]), float(r["loss_scale"]),
                    opt.loss_scale.get_scale(), opt.loss_scale.get_growth_tracker()))
    flat = torch.cat([p.detach().flatten() for p in model.parameters()]).cpu()
    torch.save((out, flat, int(opt._gate[4].item())), os.path.join(q, f"r{rank}.pt"))
    dist.destroy_process_group()


def test_two_ranks_skip_and_back_off_alike():
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_worker, args=(2, _free_port(), d), nprocs=2, join=True)
        res = [torch.load(os.path.join(d, f"r{r}.pt")) for r in range(2)]
    want = [(True, True, S0, S0, 1), (True, False, S0, S0 / 2, 0),
            (True, True, S0 / 2, S0 / 2, 1), (True, True, S0 / 2, S0, 0)]
    for out, _, step in res:
        assert out == want, out
        assert step == 3
    assert torch.equal(res[0][1], res[1][1])
