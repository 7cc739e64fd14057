"""The device-gated training step (tests/test_step_gate_gpu.py) beyond one plain parameter group
over a fully trainable model: (a) two groups — the three trunks at lr 1e-4, the fusion head at
lr 1e-3 with amsgrad — stepped by one mauv_adam_step_ex launch, and (b) a frozen sonar trunk
(every parameter of sss_model_feat with requires_grad=False before the first step) under an
optimizer built over model.parameters(), as Example_Retraining_model.py retrains a head.

Each case runs that file's six-batch sequence (a NaN input, a NaN gradient) on the tri-modal
model at 64 px, B = 2, num_mc = 2, once gated and once host-decided (``_step_gate`` patched to
None): ``_step_gate`` returns a gate on every batch, both arms take the decisions that file
expects and end with bit-identical parameters, and from the second batch on the gated step
makes no synchronising call."""
import pytest
import torch

from tests.test_step_gate_gpu import SEQ, _model, _run, _InjectNaNGrad

pytestmark = pytest.mark.gpu

WANT = [(True, True), (True, True), (False, False), (True, True), (True, False), (True, False)]
TRUNKS = ("image_model_feat", "bathy_model_feat", "sss_model_feat")


def _is_trunk(name):
    return name.split(".")[0] in TRUNKS


def _two_groups(model):
    from mauv.optim import FusedAdam
    named = list(model.named_parameters())
    return FusedAdam([dict(params=[p for n, p in named if _is_trunk(n)], lr=1e-4),
                      dict(params=[p for n, p in named if not _is_trunk(n)], lr=1e-3,
                           amsgrad=True)], weight_decay=1e-5)


def _frozen_trunk(model):
    from mauv.optim import FusedAdam
    for p in model.sss_model_feat.parameters():
        p.requires_grad_(False)
    return FusedAdam(model.parameters(), lr=1e-3, weight_decay=1e-5)


def _both_arms(make, monkeypatch):
    """(gated model, its optimizer, host-decided model, its optimizer) after SEQ, and the
    parameters both started from."""
    import mauv.train as T
    from mauv.engine import root_state
    inject = _InjectNaNGrad()
    try:
        gat, host = _model(), _model()
        root_state(host).seed = root_state(gat).seed
        opt_gat, opt_host = make(gat), make(host)
        fresh = [p.detach().clone() for p in gat.parameters()]
        real, gates = T._step_gate, []

        def spy(*a):
            gates.append(real(*a))
            return gates[-1]
        monkeypatch.setattr(T, "_step_gate", spy)
        f_gat = _run(gat, opt_gat, SEQ, 10, inject, sync_check_from=1)
        monkeypatch.setattr(T, "_step_gate", lambda *a: None)   # the host-decided path
        f_host = _run(host, opt_host, SEQ, 10, inject)
        monkeypatch.setattr(T, "_step_gate", real)
    finally:
        inject.close()
    assert len(gates) == len(SEQ) and all(g is not None and g is opt_gat._gate for g in gates)
    assert f_gat == WANT, f_gat
    assert [st for _, st in f_host] == [st for _, st in WANT], f_host
    bad = [n for (n, p), q in zip(host.named_parameters(), gat.parameters())
           if not torch.equal(p.detach(), q.detach())]
    assert not bad, bad[:5]
    return gat, opt_gat, host, opt_host, fresh


def test_two_groups_gated_matches_host_decided(monkeypatch):
    from mauv.optim import G_POISONED, G_STEP, G_SKIP_LOSS, G_SKIP_GRAD
    gat, opt_gat, host, opt_host, fresh = _both_arms(_two_groups, monkeypatch)
    assert "ex" in opt_gat._fast and 0 not in opt_gat._fast
    gate = opt_gat._gate.cpu()
    assert int(gate[G_STEP]) == 3 and int(gate[G_POISONED]) == 1
    assert int(gate[G_SKIP_LOSS]) == 1 and int(gate[G_SKIP_GRAD]) == 2
    for (n, p), f in zip(gat.named_parameters(), fresh):   # every row of both groups stepped
        assert not torch.equal(p.detach(), f) or not opt_gat.state[p]["exp_avg_sq"].any(), n
    for g in opt_gat.param_groups:
        assert any(bool(opt_gat.state[p]["exp_avg_sq"].any()) for p in g["params"][:8])
    for opt in (opt_gat, opt_host):
        sd = opt.state_dict()
        trunk_ids, head_ids = (set(g["params"]) for g in sd["param_groups"])
        assert set(sd["state"]) == trunk_ids | head_ids
        assert {float(v["step"]) for v in sd["state"].values()} == {3.0}
        assert all("max_exp_avg_sq" in sd["state"][i] for i in head_ids)
        assert not any("max_exp_avg_sq" in sd["state"][i] for i in trunk_ids)
    # both groups' state agrees between the arms, max_exp_avg_sq included
    for p, q in zip(gat.parameters(), host.parameters()):
        for k, v in opt_gat.state[p].items():
            if k != "step":
                assert torch.equal(v, opt_host.state[q][k]), k


def test_frozen_trunk_gated_matches_host_decided(monkeypatch):
    from mauv.optim import G_STEP
    gat, opt_gat, host, opt_host, fresh = _both_arms(_frozen_trunk, monkeypatch)
    assert 0 in opt_gat._fast   # one plain group: the mauv_adam_step entry points
    assert int(opt_gat._gate[G_STEP].item()) == 3
    frozen = {id(p) for p in gat.sss_model_feat.parameters()}
    assert frozen and len(frozen) < len(list(gat.parameters()))
    for (n, p), f in zip(gat.named_parameters(), fresh):
        if id(p) in frozen:
            assert not p.requires_grad and p.grad is None, n
            assert torch.equal(p.detach(), f), n
            assert p not in opt_gat.state, n
        else:
            assert not torch.equal(p.detach(), f) or \
                not opt_gat.state[p]["exp_avg_sq"].any(), n
    sd = opt_gat.state_dict()
    assert len(sd["state"]) == len(list(gat.parameters())) - len(frozen)
    assert {float(v["step"]) for v in sd["state"].values()} == {3.0}
    for p in host.sss_model_feat.parameters():
        assert p.grad is None and p not in opt_host.state
