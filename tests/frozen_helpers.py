"""Shared set-up of the frozen-BatchNorm model tests (tests/test_frozen_bn_model_gpu.py,
tests/test_frozen_bn_16_gpu.py): an oracle / mauv pair whose running statistics describe the
test batch, per-test copies of it, and the BatchNorm buffers as a comparable snapshot.

At random init the running statistics are (0, 1) and a frozen BatchNorm is nearly the identity,
so the pair is calibrated first: one train-mode forward of the oracle on the test batch with
every BatchNorm's momentum at 1.0 leaves each running mean / variance at that batch's (the
smallest running variance of the tri-modal model at 64 px, B = 3 is 4e-3), momentum goes back to
0.1, and the mauv model takes that state_dict."""
import copy

import torch
import torch.nn as nn


def batchnorms(model):
    return [m for m in model.modules() if isinstance(m, nn.BatchNorm2d)]


def calibrate(o, *inputs):
    """Running statistics of oracle ``o`` := the batch statistics of ``inputs`` (one MC pass)."""
    bns = batchnorms(o)
    for bn in bns:
        bn.momentum = 1.0
    o.train()
    with torch.no_grad():
        o(*inputs)
    for bn in bns:
        bn.momentum = 0.1


def calibrated_pair(batch, seed=0, num_classes=7):
    """(oracle, mauv model on the CPU) with the same weights and calibrated running statistics,
    nothing frozen yet; copy them with ``clone`` / ``to_gpu`` per test."""
    from mauv.models import define_models
    from oracle.model_ref import define_models as oracle_define, DEFAULT_PRIOR
    torch.manual_seed(seed)
    o = oracle_define(None, num_classes, DEFAULT_PRIOR)["multimodal_model"]
    torch.manual_seed(seed)
    m = define_models(None, num_classes, DEFAULT_PRIOR)["multimodal_model"]
    calibrate(o, batch["main_image"], batch["bathy_image"], batch["sss_image"])
    m.load_state_dict(o.state_dict())
    return o, m


def clone(model):
    c = copy.deepcopy(model)
    for p in c.parameters():
        p.grad = None
    return c


def to_gpu(m_cpu):
    """A fresh GPU copy of the CPU template (no engine state travels: the template never ran)."""
    assert "_mauv_state" not in m_cpu.__dict__
    return clone(m_cpu).cuda()


def provider(store, model):
    """eps_provider serving EpsBridge.collect's ``store`` to ``model`` by qualified module name,
    passes 0..G-1 on every call (EpsBridge.provider for a model built after the recording)."""
    names = {id(mod): n for n, mod in model.named_modules()}

    def prov(module, name, G):
        lst = store[(names[id(module)], name)]
        assert len(lst) >= G
        return torch.stack(lst[:G]).cuda().contiguous()
    return prov


def bn_buffers(model, prefix=""):
    """{name: clone} of every BatchNorm running_mean / running_var / num_batches_tracked."""
    return {n: b.detach().clone() for n, b in model.named_buffers()
            if n.startswith(prefix) and n.rsplit(".", 1)[-1] in
            ("running_mean", "running_var", "num_batches_tracked")}


def changed(model, snap):
    """Names of the snapshot's buffers whose bits differ now."""
    now = dict(model.named_buffers())
    return [n for n, v in snap.items() if not torch.equal(now[n], v)]
