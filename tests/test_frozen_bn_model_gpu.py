"""Frozen BatchNorm on the tri-modal model (fp32, 64 px, B = 3, N = 2, the oracle's epsilons
replayed as in tests/test_model_gpu.py): the forward and the backward on the running statistics
against the oracle frozen the same way (torch's own eval-mode F.batch_norm) and its float64 run,
BatchNorm buffers that no call moves, predictions that do not depend on the rest of the batch,
one frozen trunk beside two live ones, the device-gated training step, and the fp32 data-gradient
epilogue that must not sum partials for a frozen BatchNorm.

The running statistics are calibrated on the test batch first (tests/frozen_helpers.py).  The
gradients are judged by the project's relative rule (test_model_gpu._assert_grads_as_accurate:
HIP against float64 within 1.5x / 2x / 2x (+1e-4) of the fp32 oracle's median / p90 / max
per-tensor error): on the CPU the frozen fp32 oracle itself is 1.4e-2 / 2.9e-2 / 0.17 from its
float64 run at these shapes."""
import types

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import bayes_ref
from tests.golden.common import make_batches, SEED_DATA
from tests.helpers import EpsBridge, oracle64, ListLoader
from tests.frozen_helpers import (batchnorms, calibrated_pair, clone, to_gpu, provider,
                                  bn_buffers, changed)
from tests.test_model_gpu import _assert_close, _assert_grads_as_accurate

pytestmark = pytest.mark.gpu

B, N = 3, 2
TRUNKS = ("image_model_feat", "bathy_model_feat", "sss_model_feat")


def _cuda(*ts):
    return [t.cuda() for t in ts]


def _is_bn_param(model):
    ids = {id(p) for bn in batchnorms(model) for p in bn.parameters()}
    return [id(p) in ids for p in model.parameters()]


def _oracle_step(o, batch, seed, m_names):
    """One fp32 training step of oracle ``o`` (as it is frozen) and the same step in float64 on
    a copy taken before it -> dict(o, o64, logits, l64, loss, store)."""
    x, b, s, y = batch["main_image"], batch["bathy_image"], batch["sss_image"], batch["label"]

    def loss_of(model, dt=torch.float32):
        lg = torch.stack([model(x.to(dt), b.to(dt), s.to(dt)) for _ in range(N)])
        loss = F.cross_entropy(lg.mean(0), y) + bayes_ref.get_kl_loss(model) / B * 0.5
        loss.backward()
        return lg.detach(), loss.detach()

    o_pre = clone(o)
    bridge = EpsBridge(o, m_names, seed)
    with bridge:
        logits, loss = loss_of(o)
    bridge.collect()
    o64, (l64, _) = oracle64(o_pre, bridge.store, lambda mm: loss_of(mm, torch.float64))
    return dict(o=o, o64=o64, logits=logits, l64=l64, loss=loss, store=bridge.store)


@pytest.fixture(scope="module")
def ref():
    """The calibrated pair and the fully frozen oracle's step, computed once and left unchanged."""
    from mauv import freeze_batchnorm
    batch = make_batches(SEED_DATA, 1, B=B, S_opt=64, S_son=64)[0]
    o, m_cpu = calibrated_pair(batch)
    assert min(bn.running_var.min().item() for bn in batchnorms(o)) > 1e-3
    o_live = clone(o)
    assert freeze_batchnorm(o) == 159
    snap = bn_buffers(o)
    r = _oracle_step(o, batch, 99, m_cpu)
    assert not changed(o, snap) and len(snap) == 3 * 159
    r.update(batch=batch, m_cpu=m_cpu, o_live=o_live)
    return r


def _frozen_model(ref, **kw):
    from mauv import freeze_batchnorm
    from mauv.engine import root_state
    m = to_gpu(ref["m_cpu"])
    assert freeze_batchnorm(m, **kw) == 159
    root_state(m).eps_provider = provider(ref["store"], m)
    return m


def _step(m, batch, ref_loss=None):
    """Forward + loss + backward of test_multimodal_train_step_parity on the mauv model."""
    from mauv.kl import get_kl_loss
    from mauv import mchead
    x, b, s, y = _cuda(batch["main_image"], batch["bathy_image"], batch["sss_image"],
                       batch["label"])
    logits = m.mc_forward(x, b, s, N)
    kl = get_kl_loss(m)
    ce, _, _ = mchead.mc_mean_ce(logits, y)
    loss = ce + kl / B * 0.5
    if ref_loss is not None:
        assert abs(loss.item() - ref_loss.item()) <= 1e-4 * abs(ref_loss.item())
    loss.backward()
    return logits.detach(), kl.detach()


@pytest.mark.parametrize("freeze_affine", [False, True], ids=["affine-live", "affine-frozen"])
def test_frozen_step_parity(ref, freeze_affine):
    """Logits against the frozen fp32 oracle and its float64 run, KL and loss as in
    test_multimodal_train_step_parity, every gradient tensor by the relative rule; with
    freeze_affine the BatchNorm parameters get no gradient and the rest the same ones."""
    m = _frozen_model(ref, freeze_affine=freeze_affine)
    m.train()
    snap = bn_buffers(m)
    logits, kl = _step(m, ref["batch"], ref["loss"])
    _assert_close(logits, ref["logits"])
    _assert_close(logits, ref["l64"])
    assert abs(kl.item() - bayes_ref.get_kl_loss(ref["o"]).item()) <= 1e-5 * abs(kl.item())
    assert not changed(m, snap)
    hip, cpu, truth = (list(mm.parameters()) for mm in (m, ref["o"], ref["o64"]))
    assert len(hip) == 696 and all(p.grad is not None for p in truth)
    isbn = _is_bn_param(m)
    assert sum(isbn) == 2 * 159
    if freeze_affine:
        assert all(p.grad is None and not p.requires_grad for p, f in zip(hip, isbn) if f)
        hip, cpu, truth = ([p for p, f in zip(ps, isbn) if not f] for ps in (hip, cpu, truth))
    else:   # every BatchNorm has a gamma gradient to be judged
        assert all(p.grad.abs().max().item() > 0 for p, f in zip(truth, isbn) if f)
    _assert_grads_as_accurate(hip, cpu, truth)


def test_buffers_never_move(ref, tmp_path):
    """Forward, backward, two training steps, mc_statistics and the predictor (its second batch
    replays a captured graph) leave every running_mean / running_var / num_batches_tracked of
    the frozen model bit-unchanged; unfrozen again, one forward moves all of them."""
    from mauv import unfreeze_batchnorm
    from mauv.engine import root_state
    from mauv.optim import FusedAdam
    from mauv.predict import mc_statistics, multimodal_predict_and_save
    from mauv.train import mc_train_step
    m = _frozen_model(ref)
    root_state(m).eps_provider = None      # the free-running sampler, as in production
    snap = bn_buffers(m)
    assert len(snap) == 3 * 159
    batch = ref["batch"]
    x, b, s, y = _cuda(batch["main_image"], batch["bathy_image"], batch["sss_image"],
                       batch["label"])
    m.train()
    _step(m, batch)
    assert not changed(m, snap)
    opt = FusedAdam(m.parameters(), lr=1e-4)
    opt.zero_grad()
    crit = nn.CrossEntropyLoss()
    for _ in range(2):
        r = mc_train_step(m, (x, b, s), y, crit, opt, N, B, 1e-3)
        assert bool(r["stepped"])
    assert not changed(m, snap)
    with torch.no_grad():
        mc_statistics(m, x, b, s, 4)
    assert not changed(m, snap)
    rows = [(bt["main_image"], bt["bathy_image"], bt["sss_image"], [f"i{k}_{j}" for j in range(B)])
            for k, bt in enumerate(make_batches(SEED_DATA + 1, 2, B=B, S_opt=64, S_son=64))]
    multimodal_predict_and_save(m, ListLoader(rows, B), "cuda", str(tmp_path / "p.csv"),
                                num_mc_samples=3)
    assert len(open(tmp_path / "p.csv").read().splitlines()) == 1 + 2 * B
    assert all(not bn.training for bn in batchnorms(m))      # the predictor's model.train()
    assert not changed(m, snap)
    assert unfreeze_batchnorm(m) == 159
    m.train()
    with torch.no_grad():
        m.mc_forward(x, b, s, N)
    assert len(changed(m, snap)) == 3 * 159


def test_prediction_independent_of_batch(ref):
    """Item 0 alone and inside the batch of three, same MC samples: equal within the logits rule
    when frozen; more than 10x that bar apart on the unfrozen control.

    The model is fitted to the batch first (helpers.fit_model, then the calibrating forward):
    at random init the fusion head maps every input to logits within ~3e-4 of each other (|logit|
    <= 0.18), so the control moves by 0.9e-3 to 1.8e-3 over eight batch seeds — a large change
    for those logits, but under 10x the rule's absolute floor of 2e-4 whatever the batch.  Fitted,
    the logits depend on the input (|logit| ~ 50) and the control separates by three orders of
    magnitude more than asked (measured 17.5, 19.7 and 25.4 over three fits with free-running
    MC samples, 14.9 against 10 x 5.4e-3 with the fit's seed fixed as below; frozen: 0.0 each
    time)."""
    from mauv import freeze_batchnorm
    from mauv.engine import root_state
    from tests.helpers import fit_model
    batch = ref["batch"]
    x, b, s, y = _cuda(batch["main_image"], batch["bathy_image"], batch["sss_image"],
                       batch["label"])
    m = to_gpu(ref["m_cpu"])
    root_state(m).seed = 4321           # the fit's MC samples: the same model every run
    fit_model(m, x, b, s, y)
    bns = batchnorms(m)
    for bn in bns:      # the running statistics := this batch's under the fitted weights
        bn.momentum = 1.0
    with torch.no_grad():
        m.mc_forward(x, b, s, 1)
    for bn in bns:
        bn.momentum = 0.1
    state = {k: v.clone() for k, v in m.state_dict().items()}

    def pair():
        st = root_state(m)
        st.seed = 1234
        m.train()
        with torch.no_grad():
            st.offset = 0
            full = m.mc_forward(x, b, s, N)
            st.offset = 0                   # the same MC samples
            alone = m.mc_forward(x[:1], b[:1], s[:1], N)
        return alone, full[:, :1]

    alone, inside = pair()                  # the control: batch statistics
    d = (alone.double() - inside.double()).abs().max().item()
    bar = 2e-4 * max(1.0, inside.abs().max().item())
    print(f"control: item 0 alone vs in the batch {d:.3e} (bar {bar:.3e})")
    assert d > 10 * bar, (d, bar)
    m.load_state_dict(state)                # the control's forwards moved the statistics
    assert freeze_batchnorm(m) == 159
    alone, inside = pair()
    d = (alone.double() - inside.double()).abs().max().item()
    print(f"frozen: item 0 alone vs in the batch {d:.3e}")
    _assert_close(alone, inside)


def test_mixed_frozen_sonar_trunk(ref):
    """The sonar trunk frozen, the optical and bathymetry trunks live, on the oracle and on the
    mauv model alike: one training step passes the gradient rule, the frozen trunk's buffers
    keep their bits and every other BatchNorm's have moved."""
    from mauv import freeze_batchnorm, FrozenBatchNorm2d
    from mauv.engine import root_state
    o = clone(ref["o_live"])
    assert freeze_batchnorm(o.sss_model_feat) == 53
    r = _oracle_step(o, ref["batch"], 99, ref["m_cpu"])
    m = to_gpu(ref["m_cpu"])
    root_state(m)                                   # a state the call below must drop
    assert freeze_batchnorm(m.sss_model_feat, root=m) == 53
    assert "_mauv_state" not in m.__dict__
    assert sum(isinstance(bn, FrozenBatchNorm2d) for bn in batchnorms(m)) == 53
    root_state(m).eps_provider = provider(r["store"], m)
    m.train()
    sonar, rest = bn_buffers(m, "sss_model_feat."), {}
    rest.update(bn_buffers(m, "image_model_feat."), **bn_buffers(m, "bathy_model_feat."))
    assert len(sonar) == 3 * 53 and len(rest) == 6 * 53
    logits, _ = _step(m, ref["batch"], r["loss"])
    _assert_close(logits, r["logits"])
    _assert_close(logits, r["l64"])
    _assert_grads_as_accurate(list(m.parameters()), list(o.parameters()),
                              list(r["o64"].parameters()))
    assert not changed(m, sonar)
    assert len(changed(m, rest)) == len(rest)


def test_gated_training_step(ref, monkeypatch):
    """mc_train_step with FusedAdam over model.parameters() on a model frozen with
    freeze_affine (its BatchNorm parameters sit in the optimizer and are never stepped):
    _step_gate returns the optimizer's gate on every batch, every step is taken, and the gated
    and host-decided arms end bit-identical after three steps (the _both_arms pattern of
    tests/test_step_gate_groups_gpu.py without its injected NaNs)."""
    import mauv.train as T
    from mauv import freeze_batchnorm
    from mauv.engine import root_state
    from mauv.optim import FusedAdam, G_STEP
    from tests.test_step_gate_gpu import _run
    gat, host = to_gpu(ref["m_cpu"]), to_gpu(ref["m_cpu"])
    for m in (gat, host):
        assert freeze_batchnorm(m, freeze_affine=True) == 159
    root_state(host).seed = root_state(gat).seed
    opt_gat = FusedAdam(gat.parameters(), lr=1e-3, weight_decay=1e-5)
    opt_host = FusedAdam(host.parameters(), lr=1e-3, weight_decay=1e-5)
    fresh = [p.detach().clone() for p in gat.parameters()]
    snap = bn_buffers(gat)
    real, gates = T._step_gate, []

    def spy(*a):
        gates.append(real(*a))
        return gates[-1]
    seq, quiet = ["ok"] * 3, types.SimpleNamespace(on=False)
    monkeypatch.setattr(T, "_step_gate", spy)
    f_gat = _run(gat, opt_gat, seq, 10, quiet, sync_check_from=1)
    monkeypatch.setattr(T, "_step_gate", lambda *a: None)   # the host-decided path
    f_host = _run(host, opt_host, seq, 10, quiet)
    monkeypatch.setattr(T, "_step_gate", real)
    assert len(gates) == 3 and all(g is not None and g is opt_gat._gate for g in gates)
    assert f_gat == [(True, True)] * 3 and [st for _, st in f_host] == [True] * 3
    assert int(opt_gat._gate[G_STEP].item()) == 3
    bad = [n for (n, p), q in zip(host.named_parameters(), gat.parameters())
           if not torch.equal(p.detach(), q.detach())]
    assert not bad, bad[:5]
    for (n, p), f, isbn in zip(gat.named_parameters(), fresh, _is_bn_param(gat)):
        if isbn:
            assert torch.equal(p.detach(), f) and p.grad is None and p not in opt_gat.state, n
        else:
            assert not torch.equal(p.detach(), f) or not opt_gat.state[p]["exp_avg_sq"].any(), n
    assert not changed(gat, snap) and not changed(host, snap)


def test_no_dgrad_partials_for_frozen_batchnorm(ref, monkeypatch):
    """The fp32 data-gradient epilogue's BatchNorm partials (engine.BWD_PARTIALS_F32) are never
    requested in front of a frozen BatchNorm — they would be sums over undefined batch
    statistics — so the switch changes no gradient bit of a fully frozen model; the unfrozen
    model does request them."""
    from mauv import engine, ops
    asked = []
    real = ops.conv2d_bwd_data

    def spy(*a, **k):
        asked.append(k.get("bn") is not None)
        return real(*a, **k)
    monkeypatch.setattr(ops, "conv2d_bwd_data", spy)
    grads = []
    for on in (True, False):
        monkeypatch.setattr(engine, "BWD_PARTIALS_F32", on)
        m = _frozen_model(ref)
        _step(m, ref["batch"])
        grads.append([p.grad.detach().clone() for p in m.parameters()])
        del m
    assert asked and not any(asked)
    assert all(torch.equal(a, b) for a, b in zip(*grads))
    monkeypatch.setattr(engine, "BWD_PARTIALS_F32", True)
    live = to_gpu(ref["m_cpu"])
    engine.root_state(live).eps_provider = provider(ref["store"], live)
    del asked[:]
    _step(live, ref["batch"])
    assert any(asked)
