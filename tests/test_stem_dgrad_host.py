"""The stems' data-gradient entries at the C boundary, on the host (no GPU): mauv_stem_bwd_rows_f32,
mauv_stem_bwd_rows_h16 and mauv_stem_col2im refuse every bad quantity before any arithmetic on it,
with null buffers (nothing may be dereferenced), naming the entry and the quantity as
tests/test_conv_args_host.py asks of the convs.  The ABI version stays 4 (the entries are purely
additive); include/mauv.h declares them and mauv._lib binds them."""
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ROWS_GOOD = dict(G=2, M=60, Kp=160, Cout=64)
ROWS_BAD = [(q, v) for q in ROWS_GOOD for v in (0, -1)] + \
    [("Kp", 164), ("Kp", 2056), ("Cout", 12), ("Cout", 36)]
# 2^31 row chunks of 8 columns: M * Kp / 8 = 2^27 * 16
ROWS_CHUNKS = dict(M=1 << 27, Kp=128)

C2I_GOOD = dict(B=2, C=3, H=9, W=12, R=7, S=7, stride=2, pad=3, Kp=160)
C2I_ORDER = list(C2I_GOOD)
C2I_BAD = [(q, dict([(q, v)])) for q in ("B", "C", "H", "W", "R", "S", "stride")
           for v in (0, -1)] + [
    ("pad", dict(pad=-1)),
    ("Ho", dict(H=2, R=5, pad=0)), ("Wo", dict(W=2, S=5, pad=0)),
    ("Ho", dict(H=1, R=4, pad=1, stride=2)),
    ("Kp", dict(Kp=0)), ("Kp", dict(Kp=156)),        # not a multiple of 8
    ("Kp", dict(Kp=144)),                            # below C*R*S = 147
    ("Kp", dict(Kp=2056)),                           # above 2048
    ("Kp", dict(C=42, Kp=2048)),                     # C*R*S = 2058 cannot fit
    ("M * Kp / 8", dict(B=1 << 12, C=1, H=1 << 9, W=1 << 9, R=1, S=1, stride=1, pad=0,
                        Kp=2048)),                   # M = 2^30 rows of 256 chunks
]


def _rows(lib, name, over):
    g = dict(ROWS_GOOD)
    g.update(over)
    a = (g["G"], g["M"], g["Kp"], g["Cout"])
    if name == "stem_bwd_rows_f32":
        return lib.mauv_stem_bwd_rows_f32(None, None, None, *a, None)
    return lib.mauv_stem_bwd_rows_h16(0, None, None, None, *a, None)


def _c2i(lib, over):
    g = dict(C2I_GOOD)
    g.update(over)
    return lib.mauv_stem_col2im(None, *[g[k] for k in C2I_ORDER], None, None)


def _refused(lib, rc, name, quantity):
    assert rc < 0, (name, quantity)
    msg = lib.mauv_last_error()
    assert name.encode() + b":" in msg and b" " + quantity.encode() + b" must" in msg, msg


@pytest.mark.parametrize("name", ["stem_bwd_rows_f32", "stem_bwd_rows_h16"])
@pytest.mark.parametrize("quantity,value", ROWS_BAD, ids=[f"{q}={v}" for q, v in ROWS_BAD])
def test_rows_refuse_bad_quantity_by_name(name, quantity, value):
    from mauv._lib import lib
    _refused(lib, _rows(lib, name, {quantity: value}), name, quantity)


@pytest.mark.parametrize("name", ["stem_bwd_rows_f32", "stem_bwd_rows_h16"])
def test_rows_refuse_two_to_the_31_row_chunks(name):
    from mauv._lib import lib
    _refused(lib, _rows(lib, name, ROWS_CHUNKS), name, "M * Kp / 8")
    # one row fewer is within the count: the refusal that follows is the null buffers'
    _refused(lib, _rows(lib, name, dict(ROWS_CHUNKS, M=(1 << 27) - 1)), name, "drows")


def test_rows_h16_refuses_bad_dtype():
    from mauv._lib import lib
    for dt in (-1, 2):
        assert lib.mauv_stem_bwd_rows_h16(dt, None, None, None, 2, 60, 192, 64, None) < 0
        assert b"stem_bwd_rows_h16: dtype must" in lib.mauv_last_error()


@pytest.mark.parametrize("quantity,over", C2I_BAD,
                         ids=[f"{q}:{'_'.join(f'{k}{v}' for k, v in o.items())}"
                              for q, o in C2I_BAD])
def test_col2im_refuses_bad_quantity_by_name(quantity, over):
    from mauv._lib import lib
    _refused(lib, _c2i(lib, over), "stem_col2im", quantity)


def test_valid_geometry_reaches_the_buffer_check():
    """Valid arguments pass every geometric refusal: with null buffers the next refusal is the
    buffers' own (nothing is launched on a null pointer)."""
    from mauv._lib import lib
    for name in ("stem_bwd_rows_f32", "stem_bwd_rows_h16"):
        _refused(lib, _rows(lib, name, {}), name, "drows")
    _refused(lib, _c2i(lib, {}), "stem_col2im", "dx")
    # a non-stem geometry (3x3 / 1, K = 45 -> 64) and Cout = 16 are within the entries too
    _refused(lib, _c2i(lib, dict(C=5, H=6, W=7, R=3, S=3, stride=1, pad=1, Kp=64)),
             "stem_col2im", "dx")
    _refused(lib, _rows(lib, "stem_bwd_rows_f32", dict(Cout=16)), "stem_bwd_rows_f32", "drows")


def test_abi_version_is_still_4():
    from mauv._lib import lib
    assert lib.mauv_abi_version() == 4


def test_header_declares_and_lib_binds_the_entries():
    from mauv import _lib
    with open(os.path.join(REPO, "include", "mauv.h")) as f:
        header = f.read()
    for name, nargs in (("mauv_stem_bwd_rows_f32", 8), ("mauv_stem_bwd_rows_h16", 9),
                        ("mauv_stem_col2im", 12)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m, name + " is not declared in include/mauv.h"
        assert len(m.group(1).split(",")) == nargs, (name, m.group(1))
        assert len(_lib.SIGNATURES[name]) == nargs
        assert list(getattr(_lib.lib, name).argtypes) == _lib.SIGNATURES[name]


def test_ops_wrappers_exist_and_attribution_is_exported():
    import mauv
    from mauv import ops
    assert callable(ops.stem_bwd_rows) and callable(ops.stem_col2im)
    for name in ("input_gradients", "modality_shares", "fgsm"):
        assert callable(getattr(mauv, name))


def test_modality_shares_rows_sum_to_one_on_the_host():
    """Pure torch: L2-norm shares per item; an item with all-zero gradients gets equal shares."""
    import torch
    from mauv import modality_shares
    torch.manual_seed(0)
    g = (torch.randn(4, 3, 5, 5), 2 * torch.randn(4, 3, 5, 5), torch.randn(4, 1, 5, 5))
    for t in g:
        t[3] = 0
    s = modality_shares(g)
    assert s.shape == (4, 3) and bool((s >= 0).all())
    assert torch.allclose(s.sum(1), torch.ones(4), atol=1e-6)
    assert torch.equal(s[3], torch.full((3,), 1.0 / 3))
    want = g[1][0].norm() / sum(t[0].norm() for t in g)
    assert abs(float(s[0, 1]) - float(want)) < 1e-6
