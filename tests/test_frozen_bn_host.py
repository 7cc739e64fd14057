"""mauv.frozen on the host (no GPU): freeze_batchnorm retypes the BatchNorms in place so that
``model.train()`` cannot put them back on batch statistics, keeps the state_dict, survives a deep
copy and pickling, freezes / restores gamma and beta, refuses a BatchNorm without running
statistics, and leaves a torch (CPU) model's forward to torch's own eval-mode F.batch_norm."""
import copy
import pickle

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from mauv import FrozenBatchNorm2d, freeze_batchnorm, unfreeze_batchnorm


def _net(seed=0):
    torch.manual_seed(seed)
    net = nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), nn.BatchNorm2d(8), nn.ReLU(),
                        nn.Sequential(nn.Conv2d(8, 16, 1), nn.BatchNorm2d(16)))
    with torch.no_grad():
        for bn in (net[1], net[3][1]):
            bn.running_mean.normal_()
            bn.running_var.uniform_(0.5, 2.0)
            bn.weight.normal_()
            bn.bias.normal_()
            bn.num_batches_tracked.fill_(7)
    return net


def _bns(net):
    return [m for m in net.modules() if isinstance(m, nn.BatchNorm2d)]


def test_train_leaves_frozen_batchnorm_in_eval():
    net = _net()
    assert freeze_batchnorm(net) == 2
    assert all(type(bn) is FrozenBatchNorm2d and not bn.training for bn in _bns(net))
    net.train()
    assert net.training and net[0].training and net[3].training
    assert all(not bn.training for bn in _bns(net))
    net.eval().train(True)
    assert all(not bn.training for bn in _bns(net))
    assert freeze_batchnorm(net) == 2      # again: nothing to retype, still frozen
    with pytest.raises(ValueError):
        net[1].train("yes")


def test_state_dict_keys_and_bits_unchanged():
    net = _net()
    before = {k: v.clone() for k, v in net.state_dict().items()}
    freeze_batchnorm(net, freeze_affine=True)
    after = net.state_dict()
    assert list(after) == list(before)
    assert all(torch.equal(after[k], before[k]) and after[k].dtype == before[k].dtype
               for k in before)
    plain = _net(seed=1)
    plain.load_state_dict(after)            # strict: an unfrozen model takes it
    assert all(torch.equal(v, before[k]) for k, v in plain.state_dict().items())
    assert all(type(bn) is nn.BatchNorm2d for bn in _bns(plain))


def test_deepcopy_and_pickle_keep_the_class():
    net = _net()
    freeze_batchnorm(net, freeze_affine=True)
    for dup in (copy.deepcopy(net), pickle.loads(pickle.dumps(net))):
        dup.train()
        assert all(type(bn) is FrozenBatchNorm2d and not bn.training for bn in _bns(dup))
        assert all(not bn.weight.requires_grad and not bn.bias.requires_grad for bn in _bns(dup))
        assert unfreeze_batchnorm(dup) == 2     # the copy remembers what it was
        assert all(type(bn) is nn.BatchNorm2d and bn.training and bn.weight.requires_grad
                   for bn in _bns(dup))


def test_freeze_affine_and_unfreeze_restore_flags():
    net = _net()
    net[1].bias.requires_grad_(False)       # a flag the user set: restored as it was
    net.eval()
    freeze_batchnorm(net)
    assert net[1].weight.requires_grad and net[3][1].bias.requires_grad
    freeze_batchnorm(net, freeze_affine=True)
    assert not any(p.requires_grad for bn in _bns(net) for p in bn.parameters())
    assert net[0].weight.requires_grad
    freeze_batchnorm(net, freeze_affine=True)   # twice: the remembered flags are the first ones
    net[3].train()
    assert unfreeze_batchnorm(net) == 2
    assert all(type(bn) is nn.BatchNorm2d for bn in _bns(net))
    assert net[1].weight.requires_grad and not net[1].bias.requires_grad
    assert net[3][1].weight.requires_grad and net[3][1].bias.requires_grad
    assert not net[1].training and net[3][1].training    # each its parent's mode
    assert unfreeze_batchnorm(net) == 0


def test_untracked_batchnorm_raises_and_changes_nothing():
    net = nn.Sequential(nn.BatchNorm2d(8), nn.BatchNorm2d(8, track_running_stats=False))
    with pytest.raises(ValueError, match="running statistics"):
        freeze_batchnorm(net)
    assert all(type(bn) is nn.BatchNorm2d and bn.training for bn in _bns(net))


def test_engine_state_is_invalidated():
    from mauv.engine import root_state
    net = _net()
    st = root_state(net)
    assert root_state(net) is st
    freeze_batchnorm(net[3], root=net)
    assert root_state(net) is not st
    assert type(net[1]) is nn.BatchNorm2d and type(net[3][1]) is FrozenBatchNorm2d
    st = root_state(net)
    unfreeze_batchnorm(net[3], root=net)
    assert root_state(net) is not st


def test_host_forward_uses_running_statistics():
    """A torch model in train mode after freeze_batchnorm: every BatchNorm output is
    F.batch_norm(training=False) of its input, no buffer moves, and an item's output does not
    depend on its batch; the unfrozen copy does all three differently."""
    net, live = _net(), _net()
    freeze_batchnorm(net)
    net.train()
    live.train()
    seen = []
    for bn in _bns(net):
        bn.register_forward_hook(lambda mod, inp, out: seen.append((mod, inp[0], out)))
    torch.manual_seed(3)
    x = torch.randn(4, 3, 9, 7)
    buf = {k: v.clone() for k, v in net.named_buffers()}
    out = net(x)
    assert len(seen) == 2
    for mod, inp, got in seen:
        ref = F.batch_norm(inp, mod.running_mean, mod.running_var, mod.weight, mod.bias, False,
                           0.0, mod.eps)
        assert torch.equal(got, ref)
    assert all(torch.equal(v, buf[k]) for k, v in net.named_buffers())
    torch.testing.assert_close(net(x[:1]), out[:1], rtol=1e-5, atol=1e-6)
    out.sum().backward()
    assert all(bn.weight.grad is not None for bn in _bns(net))
    out_live = live(x)
    assert not torch.allclose(out_live, out, atol=1e-2)
    assert not all(torch.equal(v, buf[k]) for k, v in live.named_buffers())


def test_oracle_trunk_freezes():
    """The oracle's ResNet-50 trunk (plain torch modules): all 53 BatchNorms freeze and a
    train-mode forward leaves its buffers alone."""
    from oracle.model_ref import define_models, DEFAULT_PRIOR
    torch.manual_seed(0)
    o = define_models(None, 7, DEFAULT_PRIOR)["image_model"]
    assert freeze_batchnorm(o) == 53
    o.train()
    buf = {k: v.clone() for k, v in o.named_buffers() if "running" in k or "num_batches" in k}
    assert len(buf) == 3 * 53
    with torch.no_grad():
        o(torch.randn(2, 3, 32, 32))
    now = dict(o.named_buffers())
    assert all(torch.equal(now[k], v) for k, v in buf.items())
