"""The MC head's class range on the host (no GPU): an empty batch launches nothing and returns 0
for a many-class C, and more than 4096 classes are refused by the library (with the bound in
mauv_last_error()) and by the ``mauv.ops`` wrappers before anything reaches the library."""
import pytest
import torch


def _entries(lib, C, B, G):
    """The four MC-head entry points with null buffers (nothing may be dereferenced)."""
    return {
        "mc_mean_ce": lambda: lib.mauv_mc_mean_ce(None, None, G, B, C, None, None, None, None),
        "mc_mean_bwd": lambda: lib.mauv_mc_mean_bwd(None, None, None, None, G, B, C, None, None),
        "mc_stats": lambda: lib.mauv_mc_stats(None, G, B, C, 1e-7, None, 0, None),
        "mc_finalize": lambda: lib.mauv_mc_finalize(None, G, B, C, 1e-10, None, None, None, None,
                                                   None, None),
    }


@pytest.mark.parametrize("name", ["mc_mean_ce", "mc_mean_bwd", "mc_stats", "mc_finalize"])
def test_empty_batch_returns_zero_without_launch(name):
    from mauv._lib import lib
    assert _entries(lib, 33, 0, 5)[name]() == 0
    assert _entries(lib, 4096, 0, 5)[name]() == 0
    if name != "mc_finalize":   # (its third argument is the MC sample count, not a grid extent)
        assert _entries(lib, 33, 4, 0)[name]() == 0


@pytest.mark.parametrize("name", ["mc_mean_ce", "mc_mean_bwd", "mc_stats", "mc_finalize"])
def test_more_than_4096_classes_is_an_argument_error(name):
    from mauv._lib import lib
    assert _entries(lib, 4097, 0, 5)[name]() < 0
    msg = lib.mauv_last_error()
    assert b"4096" in msg and name.encode() in msg, msg


def test_ops_wrappers_raise_value_error_above_4096():
    from mauv import ops
    C = 4097
    f32 = torch.zeros(1)
    i64 = torch.zeros(1, dtype=torch.int64)
    f64 = torch.zeros(1, dtype=torch.float64)
    with pytest.raises(ValueError, match="4096"):
        ops.mc_mean_ce(f32, i64, 1, 1, C, f32, f32, i64)
    with pytest.raises(ValueError, match="4096"):
        ops.mc_mean_bwd(None, f32, f32, i64, 1, 1, C, f32)
    with pytest.raises(ValueError, match="4096"):
        ops.mc_stats(f32, 1, 1, C, 1e-7, f64)
    with pytest.raises(ValueError, match="4096"):
        ops.mc_finalize(f64, 1, 1, C, 1e-10, f32, f32, f32, f32, i64)
    assert ops.MC_MAX_CLASSES == 4096
