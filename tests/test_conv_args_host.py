"""Conv geometry at the C boundary, on the host (no GPU): every conv entry point and sizing
helper refuses a non-positive extent, filter side or stride, a negative padding, a filter larger
than the padded image (Ho or Wo < 1) and, for the weight gradients, splits < 1, before any
arithmetic on them (stride 0 and splits 0 are divisors).  All buffers are null: nothing may be
dereferenced.  The message is what shows that the refusal came from the validation — without
a GPU an unvalidated call also returns an error, from the failed launch — so it must name the
entry point and the offending quantity."""
import pytest

# G, B, H, W, Cin, Cout, R, S, stride, pad: a valid 3x3 conv (16-bit: channels % 8 == 0)
GOOD = dict(G=1, B=2, H=8, W=8, Cin=64, Cout=64, R=3, S=3, stride=1, pad=1)
ORDER = list(GOOD)

BAD = [(q, v) for q in ("G", "B", "H", "W", "Cin", "Cout", "R", "S", "stride")
       for v in (0, -1)] + [("pad", -1)]
# the filter taller / wider than the padded image: the issue's H = 2, R = 5, pad = 0 (Ho = 0; a
# truncating division of the negative numerator would report Ho = 1)
TOO_BIG = [("Ho", dict(H=2, R=5, pad=0)), ("Wo", dict(W=2, S=5, pad=0)),
           ("Ho", dict(H=1, R=4, pad=1, stride=2)), ("Wo", dict(W=3, S=4, pad=0, stride=3))]


def _geo(over):
    g = dict(GOOD)
    g.update(over)
    return [g[k] for k in ORDER]


def _entries(lib, geo, splits=1):
    """name -> call with null buffers; names are the C symbols without the mauv_ prefix."""
    N = None
    return {
        "conv2d_fwd_f32": lambda: lib.mauv_conv2d_fwd_f32(N, N, N, N, 0, N, N, N, *geo,
                                                          N, N, N, N),
        "conv2d_bwd_data_f32": lambda: lib.mauv_conv2d_bwd_data_f32(
            N, N, N, N, N, 0, *geo, N, N, N, N, N, N, N, 0, N, N, N),
        "conv2d_bwd_weight_f32": lambda: lib.mauv_conv2d_bwd_weight_f32(
            N, N, N, N, 0, N, N, splits, *geo, N),
        "conv2d_fwd_h16": lambda: lib.mauv_conv2d_fwd_h16(0, N, N, N, N, 0, N, N, *geo,
                                                          N, N, N, N, N),
        "conv2d_bwd_data_h16": lambda: lib.mauv_conv2d_bwd_data_h16(0, N, N, N, N, 0, *geo, N),
        "conv2d_bwd_data_bn_h16": lambda: lib.mauv_conv2d_bwd_data_bn_h16(
            0, N, N, N, N, 0, *geo, N, N, N, N, N, N, N, N, 0, N, N, N),
        "conv2d_bwd_weight_h16": lambda: lib.mauv_conv2d_bwd_weight_h16(
            0, N, N, N, N, 0, N, N, splits, *geo, N),
        "conv2d_fwd_stat_blocks": lambda: lib.mauv_conv2d_fwd_stat_blocks(*geo),
        "conv2d_bwd_data_stat_blocks": lambda: lib.mauv_conv2d_bwd_data_stat_blocks(*geo),
        "conv2d_wgrad_splits": lambda: lib.mauv_conv2d_wgrad_splits(*geo),
    }


NAMES = list(_entries(None, _geo({})))


def _refused(lib, name, call, quantity):
    assert call() < 0, (name, quantity)
    msg = lib.mauv_last_error()
    assert name.encode() + b":" in msg and b" " + quantity.encode() + b" must" in msg, msg


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("quantity,value", BAD, ids=[f"{q}={v}" for q, v in BAD])
def test_bad_quantity_is_refused_by_name(name, quantity, value):
    from mauv._lib import lib
    _refused(lib, name, _entries(lib, _geo({quantity: value}))[name], quantity)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("quantity,over", TOO_BIG,
                         ids=["H2_R5", "W2_S5", "H1_R4_pad1_stride2", "W3_S4_stride3"])
def test_filter_larger_than_padded_image_is_refused(name, quantity, over):
    from mauv._lib import lib
    _refused(lib, name, _entries(lib, _geo(over))[name], quantity)


@pytest.mark.parametrize("name", ["conv2d_bwd_weight_f32", "conv2d_bwd_weight_h16"])
@pytest.mark.parametrize("splits", [0, -3])
def test_weight_gradient_refuses_splits_below_one(name, splits):
    from mauv._lib import lib
    _refused(lib, name, _entries(lib, _geo({}), splits)[name], "splits")


def test_stride_zero_probe_returns():
    """The issue's probe: stride 0 through the sizing helpers returns an error (it divided by
    zero and killed the process)."""
    from mauv._lib import lib
    assert lib.mauv_conv2d_fwd_stat_blocks(1, 2, 8, 8, 64, 64, 3, 3, 0, 1) < 0
    assert b"stride" in lib.mauv_last_error()
    assert lib.mauv_conv2d_bwd_data_stat_blocks(1, 2, 8, 8, 64, 64, 3, 3, 0, 1) < 0
    assert lib.mauv_conv2d_wgrad_splits(1, 2, 8, 8, 64, 64, 3, 3, 0, 1) < 0


def test_valid_geometry_sizes_are_unchanged():
    """Nothing changes for valid arguments: the helpers' counts, rectangular filters and
    non-square images included (values from the tile rule of include/mauv.h: one partial per
    128 rows, 64 when M <= 64; a data gradient one set per parity class)."""
    from mauv._lib import lib
    assert lib.mauv_conv2d_fwd_stat_blocks(1, 2, 8, 8, 64, 64, 3, 3, 1, 1) == 1
    # 1x3, pad 1 on 7 x 10: Ho x Wo = 9 x 10, M = 2 * 90 = 180 rows -> 2 partials
    assert lib.mauv_conv2d_fwd_stat_blocks(2, 2, 7, 10, 64, 64, 1, 3, 1, 1) == 2
    # stride 2 on 9 x 11, B = 3: classes of 5x6, 5x5, 4x6, 4x5 pixels -> 90, 75, 72, 60 rows
    assert lib.mauv_conv2d_bwd_data_stat_blocks(1, 3, 9, 11, 128, 64, 3, 5, 2, 2) == 4
    assert lib.mauv_conv2d_wgrad_splits(1, 4, 12, 20, 64, 64, 3, 1, 1, 1) >= 2
    assert lib.mauv_conv2d_wgrad_splits(1, 2, 8, 8, 64, 64, 3, 3, 1, 1) == 1


def test_ops_wrappers_take_a_pair_and_raise_on_refusal():
    """mauv.ops sizing helpers: an int is the square filter, a pair is (R, S); a refusal of the
    library raises with its message instead of returning the negative code as a count."""
    from mauv import ops
    from mauv._lib import MauvError
    assert ops.fwd_stat_blocks(2, 2, 7, 10, 64, 64, (1, 3), 1, 1) == 2
    assert ops.fwd_stat_blocks(1, 2, 8, 8, 64, 64, 3, 1, 1) == \
        ops.fwd_stat_blocks(1, 2, 8, 8, 64, 64, (3, 3), 1, 1) == 1
    assert ops.dgrad_stat_blocks(1, 3, 9, 11, 128, 64, (3, 5), 2, 2) == 4
    assert ops.wgrad_splits(1, 4, 12, 20, 64, 64, (3, 1), 1, 1) >= 2
    for fn in (ops.fwd_stat_blocks, ops.dgrad_stat_blocks, ops.wgrad_splits):
        with pytest.raises(MauvError, match="stride"):
            fn(1, 2, 8, 8, 64, 64, 3, 0, 1)
        with pytest.raises(MauvError, match="Ho"):
            fn(1, 2, 2, 8, 64, 64, (5, 1), 1, 0)
    with pytest.raises(ValueError, match="pair"):
        ops.wgrad_splits(1, 2, 8, 8, 64, 64, (3, 3, 3), 1, 1)
