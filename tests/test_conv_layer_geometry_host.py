"""The drop-in Bayesian conv layer's geometry, on the host (no GPU): the engine runs square
filters with one stride and one zero padding for both axes, so ``Conv2dReparameterization``
takes an int or an equal pair for ``kernel_size``, ``stride`` and ``padding`` and refuses, by
argument name, what it used to apply as its first element (an unequal pair, a string padding);
``dnn_to_bnn`` passes ``kernel_size`` whole and refuses a non-zero ``padding_mode``."""
import pytest
import torch
import torch.nn as nn

PRIOR = {"prior_mu": 0.0, "prior_sigma": 1.0, "posterior_mu_init": 0.0,
         "posterior_rho_init": -3.0, "type": "Reparameterization", "moped_enable": True,
         "moped_delta": 0.5}


@pytest.mark.parametrize("kw,name", [
    (dict(kernel_size=(1, 3)), "kernel_size"),
    (dict(kernel_size=(3, 1)), "kernel_size"),
    (dict(kernel_size=3, stride=(2, 1)), "stride"),
    (dict(kernel_size=3, padding=(1, 0)), "padding"),
    (dict(kernel_size=3, padding="same"), "padding"),
    (dict(kernel_size=3, padding="valid"), "padding"),
])
def test_layer_refuses_rectangular_geometry_by_name(kw, name):
    from mauv.layers import Conv2dReparameterization
    with pytest.raises(NotImplementedError, match=name):
        Conv2dReparameterization(8, 16, **kw)


def test_layer_accepts_ints_and_equal_pairs():
    from mauv.layers import Conv2dReparameterization
    a = Conv2dReparameterization(4, 8, (3, 3), stride=(1, 1), padding=(1, 1))
    b = Conv2dReparameterization(4, 8, 3, stride=1, padding=1)
    c = Conv2dReparameterization(4, 8, [3, 3], stride=[2, 2], padding=[0, 0], bias=False)
    for m in (a, b):
        assert m.kernel_size == 3 and m.stride == (1, 1) and m.padding == (1, 1)
        assert tuple(m.mu_kernel.shape) == tuple(m.rho_kernel.shape) == (8, 4, 3, 3)
    assert c.kernel_size == 3 and c.stride == (2, 2) and c.padding == (0, 0)
    # (what it already refused)
    with pytest.raises(NotImplementedError):
        Conv2dReparameterization(4, 8, 3, groups=2)
    with pytest.raises(NotImplementedError):
        Conv2dReparameterization(4, 8, 3, dilation=2)


class _Holder(nn.Module):
    def __init__(self, conv):
        super().__init__()
        self.conv = conv
        self.act = nn.ReLU()


def test_dnn_to_bnn_refuses_a_rectangular_filter():
    """It built a 1x1 Bayesian conv from nn.Conv2d(4, 8, (1, 3)) and failed only at the MOPED
    weight copy, or not at all without MOPED: the architecture changed silently."""
    from mauv.layers import dnn_to_bnn
    for moped in (True, False):
        with pytest.raises(NotImplementedError, match="kernel_size"):
            dnn_to_bnn(_Holder(nn.Conv2d(4, 8, (1, 3))), dict(PRIOR, moped_enable=moped))
    with pytest.raises(NotImplementedError, match="stride"):
        dnn_to_bnn(_Holder(nn.Conv2d(4, 8, 3, stride=(2, 1))), dict(PRIOR, moped_enable=False))
    with pytest.raises(NotImplementedError, match="padding"):
        dnn_to_bnn(_Holder(nn.Conv2d(4, 8, 3, padding=(1, 0))), dict(PRIOR, moped_enable=False))
    with pytest.raises(NotImplementedError, match="padding"):
        dnn_to_bnn(_Holder(nn.Conv2d(4, 8, 3, padding="same")), dict(PRIOR, moped_enable=False))


@pytest.mark.parametrize("mode", ["reflect", "replicate", "circular"])
def test_dnn_to_bnn_refuses_nonzero_padding_mode(mode):
    from mauv.layers import dnn_to_bnn
    with pytest.raises(NotImplementedError, match="padding_mode"):
        dnn_to_bnn(_Holder(nn.Conv2d(4, 8, 3, padding=1, padding_mode=mode)), PRIOR)


def test_dnn_to_bnn_square_conv_keeps_geometry_and_weights():
    from mauv.layers import Conv2dReparameterization, dnn_to_bnn, get_rho
    torch.manual_seed(0)
    conv = nn.Conv2d(4, 8, (3, 3), stride=(2, 2), padding=(1, 1), bias=False)
    m = _Holder(conv)
    dnn_to_bnn(m, PRIOR)
    b = m.conv
    assert isinstance(b, Conv2dReparameterization)
    assert b.kernel_size == 3 and b.stride == (2, 2) and b.padding == (1, 1)
    assert torch.equal(b.mu_kernel, conv.weight)
    assert torch.equal(b.rho_kernel, get_rho(conv.weight, PRIOR["moped_delta"]))
