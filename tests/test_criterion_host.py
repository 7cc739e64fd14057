"""The criterion-aware MC head on the host (no GPU): which criteria ``mauv.train._ce_spec`` sends
to the fused head, the library's argument checks of mauv_mc_mean_ce_ex / mauv_mc_mean_bwd_ex with
null buffers (nothing may be dereferenced), and the ``mauv.ops`` wrappers' refusals before
anything reaches the library."""
import pytest
import torch
import torch.nn as nn


class _OnGpu:
    """Stand-in for [G, B, C] logits on a ROCm device: _ce_spec reads the shape and the device."""

    def __init__(self, C, device="cuda:0"):
        self.shape = (3, 4, C)
        self.device = torch.device(device)


def test_ce_spec_routing():
    from mauv.train import _ce_spec, _is_plain_ce
    C = 7
    lg = torch.zeros(3, 4, C)
    y = torch.zeros(4, dtype=torch.int64)
    w = 0.5 + torch.rand(C)
    crit = nn.CrossEntropyLoss(weight=w, label_smoothing=0.1, ignore_index=5, reduction="sum")
    spec = _ce_spec(crit, lg, y)
    assert spec is not None and not _is_plain_ce(crit)
    assert set(spec) == {"weight", "label_smoothing", "ignore_index", "reduction"}
    assert spec["weight"] is crit.weight and spec["label_smoothing"] == 0.1
    assert spec["ignore_index"] == 5 and spec["reduction"] == "sum"
    # the plain criterion is a spec too (mc_loss asks _is_plain_ce first); no weight -> None
    assert _ce_spec(nn.CrossEntropyLoss(), lg, y) == dict(
        weight=None, label_smoothing=0.0, ignore_index=-100, reduction="mean")
    assert _ce_spec(crit, lg, y.int()) is not None

    class Sub(nn.CrossEntropyLoss):
        pass

    assert _ce_spec(Sub(weight=w), lg, y) is None
    assert _ce_spec(nn.NLLLoss(), lg, y) is None
    assert _ce_spec(nn.CrossEntropyLoss(reduction="none"), lg, y) is None
    assert _ce_spec(nn.CrossEntropyLoss(weight=w.double()), lg, y) is None
    assert _ce_spec(nn.CrossEntropyLoss(weight=torch.ones(C + 1)), lg, y) is None
    assert _ce_spec(nn.CrossEntropyLoss(weight=torch.ones(2 * C)[::2]), lg, y) is None
    assert _ce_spec(crit, lg, torch.rand(4, C)) is None          # class probabilities
    assert _ce_spec(crit, lg, torch.zeros(4)) is None            # float class "indices"
    assert _ce_spec(crit, lg, torch.zeros(4, 1, dtype=torch.int64)) is None
    # device logits: a host weight falls back, no weight does not
    assert _ce_spec(crit, _OnGpu(C), y) is None
    assert _ce_spec(nn.CrossEntropyLoss(label_smoothing=0.1), _OnGpu(C), y) is not None


def _entries(lib, C, B, G, eps=0.1, reduction=0):
    return {
        "mc_mean_ce_ex": lambda: lib.mauv_mc_mean_ce_ex(None, None, None, eps, 5, reduction, G, B,
                                                        C, None, None, None, None, None),
        "mc_mean_bwd_ex": lambda: lib.mauv_mc_mean_bwd_ex(None, None, None, None, eps, 5,
                                                          reduction, None, G, B, C, None, None),
    }


NAMES = ["mc_mean_ce_ex", "mc_mean_bwd_ex"]


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("C", [7, 33, 4096])
def test_empty_batch_returns_zero_without_launch(name, C):
    from mauv._lib import lib
    assert _entries(lib, C, 0, 5)[name]() == 0
    assert _entries(lib, C, 4, 0)[name]() == 0
    assert _entries(lib, C, 0, 5, eps=1.0, reduction=1)[name]() == 0


@pytest.mark.parametrize("name", NAMES)
def test_argument_errors_name_the_entry(name):
    from mauv._lib import lib
    assert _entries(lib, 4097, 0, 5)[name]() < 0
    msg = lib.mauv_last_error()
    assert b"4096" in msg and name.encode() in msg, msg
    for kw in (dict(eps=1.5), dict(eps=-0.25), dict(eps=float("nan")), dict(reduction=2),
               dict(reduction=-1)):
        assert _entries(lib, 7, 0, 5, **kw)[name]() < 0, kw
        msg = lib.mauv_last_error()
        assert name.encode() in msg and (b"label_smoothing" in msg and b"reduction" in msg), msg


def test_ops_wrappers_refuse_before_the_library():
    from mauv import ops
    f32 = torch.zeros(1)
    i64 = torch.zeros(1, dtype=torch.int64)
    with pytest.raises(ValueError, match="4096"):
        ops.mc_mean_ce_ex(f32, i64, None, 0.0, -100, "mean", 1, 1, 4097, f32, f32, f32, i64)
    with pytest.raises(ValueError, match="4096"):
        ops.mc_mean_bwd_ex(f32, f32, i64, None, 0.0, -100, "mean", f32, 1, 1, 4097, f32)
    # host tensors never reach a kernel
    with pytest.raises(ValueError, match="ROCm device"):
        ops.mc_mean_ce_ex(f32, i64, None, 0.0, -100, "mean", 1, 1, 1, f32, f32, f32, i64)
    with pytest.raises(ValueError, match="ROCm device"):
        ops.mc_mean_bwd_ex(f32, f32, i64, None, 0.0, -100, "mean", f32, 1, 1, 1, f32)


def test_mchead_refuses_reduction_none():
    from mauv import mchead
    with pytest.raises(ValueError, match="reduction"):
        mchead.mc_mean_ce_ex(torch.zeros(1, 1, 2), torch.zeros(1, dtype=torch.int64),
                             reduction="none")
