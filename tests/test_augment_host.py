"""On-device augmentation at the C boundary and in Python, on the host (no GPU):
the four entries are declared, bound and exported; every refusal comes back with null buffers
(nothing may be dereferenced) and names the entry point and the offending quantity — without a
GPU an unvalidated call also returns an error, from the failed launch, so the message is what
shows that the validation refused; valid geometry with null buffers reaches the buffers' own
refusal.  TripletAugment's argument errors and state round trip, the inverse-code table against
torch's flip / transpose on the CPU, and what AugmentedLoader forwards."""
import ctypes
import os
import re

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "mauv.h")
ENTRIES = ("mauv_augment_draw", "mauv_stage_u8_aug", "mauv_resize_u8_aug", "mauv_stage_f32_aug")
N = None


def test_entries_declared_bound_and_exported():
    from mauv._lib import LIB_PATH, SIGNATURES, lib
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    protos = dict(re.findall(r"(mauv_\w+)\(([^)]*)\)\s*;", txt))
    raw = ctypes.CDLL(LIB_PATH)
    for name in ENTRIES:
        assert name in protos, f"{name} is not declared in include/mauv.h"
        assert name in SIGNATURES and hasattr(raw, name)
        assert len(SIGNATURES[name]) == protos[name].count(",") + 1
    assert lib.mauv_abi_version() == 4


def _draw(lib, B=4, mode=2, lo=0.3, hi=1.5, item0=0):
    return lib.mauv_augment_draw(1, 0, item0, B, mode, lo, hi, N, N, N)


def _stage_u8(lib, B=2, H=8, W=8, C=3, tr=0):
    return lib.mauv_stage_u8_aug(N, B, H, W, C, N, N, N, N, N, 1.0, N, N, tr, N, N)


def _resize(lib, B=2, H=9, W=7, C=3, Ho=8, Wo=8, tr=0):
    return lib.mauv_resize_u8_aug(N, B, H, W, C, Ho, Wo, N, N, N, N, N, N, N, 1.0, N, N, tr, N, N)


def _stage_f32(lib, B=2, C=3, H=8, W=8, tr=0, x=N, out=N):
    return lib.mauv_stage_f32_aug(x, B, C, H, W, N, N, N, 1.0, N, N, tr, out, N)


def _refused(lib, rc, entry, *quantities):
    assert rc < 0, entry
    msg = lib.mauv_last_error().decode()
    assert msg.startswith(entry + ":"), msg
    for q in quantities:
        assert re.search(r"\b%s\b" % re.escape(q), msg), (q, msg)


def test_draw_refusals_name_the_quantity():
    from mauv._lib import lib
    _refused(lib, _draw(lib, mode=3), "augment_draw", "mode")
    _refused(lib, _draw(lib, mode=-1), "augment_draw", "mode")
    _refused(lib, _draw(lib, lo=1.5, hi=0.3), "augment_draw", "turb_hi", "turb_lo")
    _refused(lib, _draw(lib, B=-1), "augment_draw", "B")
    _refused(lib, _draw(lib, B=2, item0=2 ** 32 - 1), "augment_draw", "item0")
    _refused(lib, _draw(lib, item0=-1), "augment_draw", "item0")
    assert _draw(lib, B=0) == 0                       # launches nothing
    assert _draw(lib, B=0, item0=2 ** 32) == 0
    _refused(lib, _draw(lib, B=1, item0=2 ** 32 - 1), "augment_draw", "ops_out")   # valid: buffers


@pytest.mark.parametrize("entry,call", [("stage_u8_aug", _stage_u8), ("stage_f32_aug", _stage_f32),
                                        ("resize_u8_aug", _resize)])
def test_staging_refusals_name_the_quantity(entry, call):
    from mauv._lib import lib
    _refused(lib, call(lib, B=-1), entry, "B")
    _refused(lib, call(lib, C=0), entry, "C")
    if entry == "resize_u8_aug":
        _refused(lib, call(lib, Ho=17, Wo=12, tr=1), entry, "allow_transpose", "Ho", "Wo")
        _refused(lib, call(lib, H=17, W=12, Ho=17, Wo=12, tr=1), entry, "allow_transpose", "Ho")
        assert call(lib, H=17, W=12, Ho=16, Wo=16, tr=1) < 0      # square output: on to the buffers
        assert b"allow_transpose" not in lib.mauv_last_error()
        _refused(lib, call(lib, C=5), entry, "C")
        _refused(lib, call(lib, Ho=0), entry, "Ho")
        _refused(lib, call(lib, W=0), entry, "W")
    else:
        _refused(lib, call(lib, H=17, W=12, tr=1), entry, "allow_transpose", "H", "W")
        _refused(lib, call(lib, H=0), entry, "H")
        _refused(lib, call(lib, W=-3), entry, "W")
        # more elements than the kernels' long long indices hold
        _refused(lib, call(lib, B=2 ** 31 - 1, C=2 ** 31 - 1, H=2 ** 16, W=2 ** 16), entry,
                 "elements")
    # valid geometry (flips on 17 x 12 included), null buffers: the buffers' own refusal
    for kw in (dict(), dict(H=17, W=12) if entry != "resize_u8_aug" else dict(Ho=17, Wo=12)):
        assert call(lib, **kw) < 0
        msg = lib.mauv_last_error().decode()
        assert msg.startswith(entry + ":") and ("null" in msg or "exactly one" in msg), msg
    assert call(lib, B=0) == 0 or entry == "resize_u8_aug"


def test_moving_entries_refuse_an_input_that_overlaps_the_output():
    """A move is a gather, so x == out and any partial overlap are refused before anything is
    launched; the pointers are into a host buffer that is never read.  Without codes the u8
    entries are the plain element-wise passes and take what the plain entries take."""
    from mauv._lib import lib
    buf = ctypes.create_string_buffer(256)
    p = ctypes.addressof(buf)
    _refused(lib, _stage_f32(lib, B=1, C=1, H=2, W=2, x=p, out=p), "stage_f32_aug", "x", "out")
    _refused(lib, _stage_f32(lib, B=1, C=1, H=2, W=2, x=p, out=p + 12), "stage_f32_aug", "x",
             "out")
    _refused(lib, _stage_f32(lib, B=1, C=1, H=2, W=2, x=p + 8, out=p), "stage_f32_aug", "x", "out")
    # 2 x 2 x 1 u8 in (4 bytes), fp32 out (16 bytes)
    for x, out in ((p, p), (p + 15, p), (p, p + 3)):
        rc = lib.mauv_stage_u8_aug(x, 1, 2, 2, 1, N, N, N, N, N, 1.0, p + 128, N, 0, out, N)
        _refused(lib, rc, "stage_u8_aug", "x", "out")
    # resize without a pass (2 x 2 -> 2 x 2): the 8-bit output in place, and the fp32 output
    rc = lib.mauv_resize_u8_aug(p, 1, 2, 2, 1, 2, 2, N, p, N, N, N, N, N, 1.0, p + 128, N, 1, N, N)
    _refused(lib, rc, "resize_u8_aug", "x", "out_u8")
    rc = lib.mauv_resize_u8_aug(p + 4, 1, 2, 2, 1, 2, 2, N, N, N, N, N, N, N, 1.0, p + 128, N, 1,
                                p, N)
    _refused(lib, rc, "resize_u8_aug", "x", "out_f32")


def test_turbidity_goes_with_the_fp32_output_and_a_beta():
    from mauv._lib import lib
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    rc = lib.mauv_resize_u8_aug(N, 2, 9, 7, 3, 8, 8, N, p, N, N, p, p, N, 1.0, N, p, 0, N, N)
    _refused(lib, rc, "resize_u8_aug", "turb", "out_f32")
    rc = lib.mauv_stage_u8_aug(N, 2, 8, 8, 3, N, N, N, N, N, 1.0, N, p, 0, N, N)
    _refused(lib, rc, "stage_u8_aug", "turb", "uifm_bt")
    rc = lib.mauv_stage_f32_aug(N, 2, 3, 8, 8, N, N, N, 1.0, N, p, 0, N, N)
    _refused(lib, rc, "stage_f32_aug", "turb", "beta")


# ------------------------------------------------------------------------------ pure Python
def _cpu_move(x, k):
    y = x
    if k & 2:
        y = y.flip(-2)
    if k & 1:
        y = y.flip(-1)
    if k & 4:
        y = y.transpose(-2, -1)
    return y


def test_inverse_code_table_composes_to_identity():
    from mauv.augment import INVERSE_CODES, inverse_ops
    x = torch.arange(25.0).reshape(5, 5)
    seen = set()
    for k in range(8):
        y = _cpu_move(x, k)
        seen.add(tuple(y.reshape(-1).tolist()))
        inv = INVERSE_CODES[k]
        assert inv == (k if not k & 4 else 4 | (k & 1) << 1 | (k >> 1) & 1)
        assert torch.equal(_cpu_move(y, inv), x), k
        assert torch.equal(_cpu_move(_cpu_move(x, inv), k), x), k
    assert len(seen) == 8          # eight distinct moves: the whole group
    codes = torch.arange(16, dtype=torch.uint8)       # only the low 3 bits are read
    assert inverse_ops(codes).tolist() == list(INVERSE_CODES) * 2


def test_triplet_augment_arguments_and_state_round_trip():
    from mauv import TripletAugment
    with pytest.raises(ValueError, match="mode"):
        TripletAugment("rot90")
    with pytest.raises(ValueError, match="hi >= lo"):
        TripletAugment("flips", turbidity=(1.5, 0.3))
    with pytest.raises(ValueError, match="pair"):
        TripletAugment("flips", turbidity=(1.0,))
    with pytest.raises(ValueError, match="item0"):
        TripletAugment(item0=-1)
    a = TripletAugment("flips", turbidity=(0.3, 1.5), depth=2.5, seed=2024, item0=128)
    a.step = 17
    sd = a.state_dict()
    assert sd == {"seed": 2024, "step": 17, "mode": "flips", "turbidity": (0.3, 1.5),
                  "depth": 2.5, "item0": 128}
    b = TripletAugment("none")
    b.load_state_dict(sd)
    assert b.state_dict() == sd and b.last_plan is None
    torch.manual_seed(99)
    assert TripletAugment().seed == 99 and TripletAugment().mode == "dihedral"
    with pytest.raises(ValueError, match="mode"):
        b.load_state_dict(dict(sd, mode="spin"))
    assert b.state_dict() == sd           # a refused state changes nothing


class _Loader:
    batch_size = 6
    dataset = "the dataset"

    def __init__(self, batches):
        self.batches = batches

    def __iter__(self):
        return iter(self.batches)

    def __len__(self):
        return len(self.batches)


def test_augmented_loader_forwards_the_wrapped_loader():
    from mauv import AugmentedLoader, TripletAugment
    inner = _Loader([1, 2, 3])
    ld = AugmentedLoader(inner, TripletAugment("none"), "cuda")
    assert len(ld) == 3 and ld.batch_size == 6 and ld.dataset == "the dataset"
    assert ld.loader is inner
    with pytest.raises(AttributeError):
        ld.sampler
    with pytest.raises(ValueError, match="patch_types"):
        AugmentedLoader(inner, TripletAugment("none"), "cuda", patch_types=("a",))
    with pytest.raises(TypeError, match="batch dicts"):
        next(iter(ld))              # a prediction loader's tuples are not wrapped
