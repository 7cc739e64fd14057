"""mauv_accum_note / mauv_adam_step_ex_accum (csrc/adam.hip) on hand-built tables, with the
Arena, the measure and the bar of tests/test_adam_ex_kernel_gpu.py: rows of 1, 5, 1027 and 4096
elements with every pointer 16-byte aligned (1027 = 256 quads and a tail of 3), a 1027-element row
whose gradient alone is a view one float later (the scalar loop), over a plain group and an
amsgrad one.  The arena's gradients stand for the sum over a window's micro-batches of the
gradients of ``loss * scale``.

(a) A close on a fresh MauvAccum is mauv_adam_step_ex_scaled bit for bit: tensors, all 16 gate
    words, the scaler's words; with and without a scaler.
(b) K=3 and a partial window of 2: p, m, v, vmax equal, bit for bit, the ungated
    mauv_adam_step_ex on a copy of the gradients multiplied in torch by float32(unscale), then
    float32(1/m), then the clip coefficient; and float64 Adam (tests/adam_ref.py) from the
    gradient the kernel is documented to load, the kernel erring at most 4x the fp32 restatement,
    floored at one unit.
(c) The grad_norm word is fl32(fl32(scanned * unscale) * avg) bit for bit, and within 1 ulp(fp32)
    of the float64 norm of the averaged, unscaled gradient (tests/test_gradclip_kernel_gpu.py's
    bar).
(d) A bad loss on micro-batch 2 of 3 drops the window whole; the next window steps normally.
(e) An inf in the arena at the close: poisoned and kept without a scaler, zeroed with exactly one
    backoff with one.
(f) growth_interval 2, K=2, four clean micro-batches: exactly one growth.
(g) mauv_accum_note changes micro, bad_loss, skipped_loss, stepped and mode, and no other word."""
import ctypes

import numpy as np
import pytest
import torch

from tests import adam_ref as A
from tests import kernel_ref as R
from tests.test_adam_ex_kernel_gpu import Arena, KINDS
from tests.test_lossscale_kernel_gpu import _gate, _scaler, _scan, _words, T

pytestmark = pytest.mark.gpu

dev = "cuda"
F32 = np.float32
# (numel, shifted kind, group): group 1 is the amsgrad one
ENTRIES = [(1, None, 0), (5, None, 1), (1027, None, 0), (4096, None, 1), (1027, "g", 0),
           (1027, None, 1)]
GROUPS = [(1e-3, 0.9, 0.999, 1e-8, 1e-5, 0), (3e-4, 0.8, 0.99, 1e-6, 1e-2, A.AMSGRAD)]
STATE = ("p", "m", "v", "x")


def _arena(seed):
    ar = Arena(ENTRIES, seed=seed, groups=GROUPS)
    tab = ar.table().cpu().numpy()
    assert tab[4, 1] % 16 == 4 and not (tab[4, [0, 2, 3]] % 16).any()   # the gradient alone
    return ar


def _accum(micro=0, bad=0):
    from mauv.optim import ACC_WORDS, A_MICRO, A_BAD_LOSS, A_AVG
    w = np.zeros(ACC_WORDS, dtype=np.int32)
    w[A_MICRO], w[A_BAD_LOSS] = micro, bad
    if micro or bad:
        w.view(F32)[A_AVG] = np.nan       # the library writes it before it reads it
    return torch.tensor(w, device=dev)


def _note(gate, acc, ok_loss=1):
    from mauv import ops
    from mauv._lib import lib, check
    from mauv.optim import G_OK_LOSS
    gate[G_OK_LOSS] = ok_loss
    check(lib.mauv_accum_note(gate.data_ptr(), acc.data_ptr(), ops.stream()), "accum_note")
    torch.cuda.synchronize()


def _close(ar, gate, ls, acc, ok_loss=1):
    from mauv import ops
    from mauv._lib import lib, check
    from mauv.optim import G_OK_LOSS
    gate[G_OK_LOSS] = ok_loss
    tab, arr = ar.table(), ar.group_array()
    check(lib.mauv_adam_step_ex_accum(tab.data_ptr(), len(ar.entries), ctypes.addressof(arr),
                                      len(ar.groups), gate.data_ptr(),
                                      None if ls is None else ls.data_ptr(),
                                      None if acc is None else acc.data_ptr(), ops.stream()),
          "adam_step_ex_accum")
    return ar.result()


def _scaled(ar, gate, ls):
    from mauv import ops
    from mauv._lib import lib, check
    tab, arr = ar.table(), ar.group_array()
    check(lib.mauv_adam_step_ex_scaled(tab.data_ptr(), len(ar.entries), ctypes.addressof(arr),
                                       len(ar.groups), gate.data_ptr(),
                                       None if ls is None else ls.data_ptr(), ops.stream()),
          "adam_step_ex_scaled")
    return ar.result()


def _norm64(ar):
    g = np.concatenate([ar.view(ar.host["g"], "g", e) for e in range(len(ar.entries))])
    return float(np.sqrt(np.sum(g.astype(np.float64) ** 2)))


def _same_bits(a, b, kinds=KINDS):
    for k in kinds:
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), k


# ------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("scale", [None, 2.0 ** 16, 3.0], ids=["noscaler", "s65536", "s3"])
@pytest.mark.parametrize("acc_given", [True, False], ids=["fresh", "null"])
def test_window_of_one_is_the_scaled_entry_bitwise(scale, acc_given):
    from mauv.optim import A_MICRO, A_BAD_LOSS, A_AVG, A_WINDOWS, A_DROPPED
    new, old = _arena(11), _arena(11)
    c = _norm64(new) / (scale or 1.0) / 2
    g_new, g_old = _gate(c), _gate(c)
    l_new, l_old = (None, None) if scale is None else (_scaler(scale, interval=1),
                                                       _scaler(scale, interval=1))
    _scan(new, g_new)
    _scan(old, g_old)
    acc = _accum() if acc_given else None
    a = _close(new, g_new, l_new, acc)
    b = _scaled(old, g_old, l_old)
    _same_bits(a, b)
    assert np.array_equal(_words(g_new)[0], _words(g_old)[0])        # all 16 words
    if scale is not None:
        assert np.array_equal(_words(l_new)[0], _words(l_old)[0])
        assert _words(l_new)[1][0] == 2 * scale                       # (it grew: interval 1)
    assert not np.array_equal(a["p"].view(np.int32), new.host["p"].view(np.int32))
    new.grads_zeroed(a)
    if acc_given:
        wi, wf = _words(acc)
        assert (wi[A_MICRO], wi[A_BAD_LOSS], wi[A_WINDOWS], wi[A_DROPPED]) == (0, 0, 1, 0)
        assert wf[A_AVG] == 1.0 and not wi[5:].any()


# -------------------------------------------------------------------------------- (b), (c)
@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
@pytest.mark.parametrize("scale", [None, 2.0 ** 16, 3.0], ids=["noscaler", "s65536", "s3"])
@pytest.mark.parametrize("m", [3, 2])
def test_window_close_against_the_ungated_step_and_float64(m, scale, clip):
    from mauv import amp
    from mauv.optim import (G_MODE, G_STEP, G_STEPPED, G_NONFINITE, G_GRAD_NORM, G_CLIP_COEF,
                            A_MICRO, A_BAD_LOSS, A_AVG, A_WINDOWS, A_DROPPED)
    ar = _arena(20 + m)
    s = scale or 1.0
    unscale = F32(1.0 / float(F32(s)))
    avg = F32(1.0 / m)
    true_norm = _norm64(ar) / s / m            # of the averaged, unscaled gradient (float64)
    c = true_norm / 2 if clip else 0.0
    gate, acc = _gate(c), _accum()
    ls = None if scale is None else _scaler(scale, interval=1000, tracker=5)
    for _ in range(m - 1):
        _note(gate, acc)
    wi, _ = _words(acc)
    assert (wi[A_MICRO], wi[A_BAD_LOSS], wi[A_WINDOWS]) == (m - 1, 0, 0)
    coef = F32(1.0)
    if clip:
        _scan(ar, gate)
        scanned = _words(gate)[1][G_GRAD_NORM]
        norm = (scanned * unscale) * avg
        assert norm.dtype == np.float32
        coef = F32(min(1.0, float(F32(c)) / (float(norm) + 1e-6)))
        assert 0.49 < coef < 0.51               # clipping is active
    got = _close(ar, gate, ls, acc)
    gi_, gf = _words(gate)
    wi, wf = _words(acc)
    assert (gi_[G_MODE], gi_[G_STEP], gi_[G_STEPPED], gi_[G_NONFINITE]) == (3, T, 1, 0)
    assert (wi[A_MICRO], wi[A_BAD_LOSS], wi[A_WINDOWS], wi[A_DROPPED]) == (0, 0, 1, 0)
    assert wf[A_AVG].view(np.int32) == avg.view(np.int32)
    assert gf[G_CLIP_COEF].view(np.int32) == coef.view(np.int32)
    if ls is not None:
        si, sf = _words(ls)
        assert sf[amp.LS_UNSCALE].view(np.int32) == unscale.view(np.int32)
        assert sf[amp.LS_SCALE] == F32(scale) and si[amp.LS_TRACKER] == 6   # once per window
    if clip:                                    # (c)
        assert gf[G_GRAD_NORM].view(np.int32) == norm.view(np.int32)
        ref = F32(true_norm)
        ulp = float(np.spacing(ref))
        print(f"grad_norm m={m} scale={scale}: {gf[G_GRAD_NORM]!r} ref {ref!r} "
              f"diff {abs(float(gf[G_GRAD_NORM]) - float(ref)) / ulp:.2f} ulp")
        assert abs(float(gf[G_GRAD_NORM]) - float(ref)) <= ulp
    ar.outside_unchanged(got)
    ar.grads_zeroed(got)
    # (b) bit for bit: the ungated step on gradients multiplied in torch, one factor at a time
    old = _arena(20 + m)
    old.dev["g"].mul_(float(unscale)).mul_(float(avg)).mul_(float(coef))
    assert old.step(T) == 0
    _same_bits(got, old.result(), STATE)
    # (b) float64 beside it
    fig = np.zeros((2, 4))
    for e, (n, _, gi) in enumerate(ar.entries):
        k = A.consts(*ar.groups[gi][:5], T, ar.groups[gi][5])
        p, g, mm, v, x = (ar.view(ar.host[kk], kk, e) for kk in KINDS)
        gl = ((g * unscale) * avg) * coef       # three fp32 roundings, in the kernel's order
        assert gl.dtype == np.float32
        r64, r32 = A.adam64(p, gl, mm, v, x, k), A.adam32(p, gl, mm, v, x, k)
        for j, kk in enumerate(STATE):
            if r64[j] is None:
                continue
            fig[0, j] = max(fig[0, j], R.units(ar.view(got[kk], kk, e), *r64[j]))
            fig[1, j] = max(fig[1, j], R.units(r32[j], *r64[j]))
    print(f"accum adam m={m} scale={scale} clip={clip}: kernel p/m/v/vmax {fig[0]} units, "
          f"fp32 restatement {fig[1]}")
    for j, name in enumerate(("p", "m", "v", "vmax")):
        assert fig[0, j] <= R.bar(fig[1, j]), (name, fig[:, j])


# ------------------------------------------------------------------------------------- (d)
@pytest.mark.parametrize("scale", [None, 2.0 ** 16], ids=["noscaler", "s65536"])
def test_bad_loss_inside_a_window_drops_it_whole(scale):
    from mauv import amp
    from mauv.optim import (G_MODE, G_STEP, G_STEPPED, G_SKIP_LOSS, G_SKIP_GRAD, G_POISONED,
                            A_MICRO, A_BAD_LOSS, A_WINDOWS, A_DROPPED)
    ar = _arena(31)
    gate, acc = _gate(0.5), _accum()
    ls = None if scale is None else _scaler(scale, interval=2, tracker=1)
    ls_before = None if ls is None else _words(ls)[0].copy()
    _note(gate, acc, ok_loss=1)
    _note(gate, acc, ok_loss=0)
    wi, _ = _words(acc)
    assert (wi[A_MICRO], wi[A_BAD_LOSS]) == (2, 1) and _words(gate)[0][G_SKIP_LOSS] == 1
    _scan(ar, gate)
    got = _close(ar, gate, ls, acc, ok_loss=1)
    gi_, _ = _words(gate)
    wi, _ = _words(acc)
    assert (gi_[G_MODE], gi_[G_STEP], gi_[G_STEPPED], gi_[G_POISONED]) == (2, T - 1, 0, 0)
    assert (gi_[G_SKIP_LOSS], gi_[G_SKIP_GRAD]) == (1, 0)
    assert (wi[A_MICRO], wi[A_BAD_LOSS], wi[A_WINDOWS], wi[A_DROPPED]) == (0, 0, 1, 1)
    ar.unchanged(got, STATE)
    ar.grads_zeroed(got)
    ar.outside_unchanged(got)
    if ls is not None:                           # a NaN input is no overflow
        si = _words(ls)[0]
        assert np.array_equal(np.delete(si, amp.LS_UNSCALE), np.delete(ls_before, amp.LS_UNSCALE))
    # the next window steps normally, on its own gradients
    fresh = _arena(32)
    ar.dev["g"].copy_(fresh.dev["g"])
    _note(gate, acc)
    _note(gate, acc)
    _scan(ar, gate)
    got = _close(ar, gate, ls, acc)
    gi_, _ = _words(gate)
    wi, _ = _words(acc)
    assert (gi_[G_MODE], gi_[G_STEP], gi_[G_STEPPED], gi_[G_SKIP_LOSS]) == (3, T, 1, 1)
    assert (wi[A_MICRO], wi[A_BAD_LOSS], wi[A_WINDOWS], wi[A_DROPPED]) == (0, 0, 2, 1)
    assert not np.array_equal(got["p"].view(np.int32), ar.host["p"].view(np.int32))
    ar.grads_zeroed(got)
    # a bad loss on the closing micro-batch itself counts the same way
    _note(gate, acc)
    got = _close(ar, gate, ls, acc, ok_loss=0)
    gi_, _ = _words(gate)
    wi, _ = _words(acc)
    assert (gi_[G_MODE], gi_[G_STEP], gi_[G_SKIP_LOSS]) == (2, T, 2)
    assert (wi[A_MICRO], wi[A_BAD_LOSS], wi[A_WINDOWS], wi[A_DROPPED]) == (0, 0, 3, 2)


# ------------------------------------------------------------------------------------- (e)
@pytest.mark.parametrize("scaled", [False, True], ids=["noscaler", "scaler"])
def test_inf_in_the_arena_at_the_close(scaled):
    from mauv import amp
    from mauv.optim import (G_MODE, G_STEP, G_STEPPED, G_SKIP_GRAD, G_POISONED, G_NONFINITE,
                            G_GRAD_NORM, A_WINDOWS, A_DROPPED)
    ar = _arena(41)
    ar.dev["g"][ar.start["g"][4] + 2] = float("inf")      # in the row with the shifted gradient
    before = ar.result()
    gate, acc = _gate(1.0), _accum()
    ls = _scaler(2.0 ** 16, interval=5, tracker=3) if scaled else None
    _note(gate, acc)
    _scan(ar, gate)
    assert _words(gate)[0][G_NONFINITE] > 0
    got = _close(ar, gate, ls, acc)
    gi_, gf = _words(gate)
    wi, _ = _words(acc)
    assert (gi_[G_STEP], gi_[G_STEPPED], gi_[G_SKIP_GRAD], gi_[G_NONFINITE]) == (T - 1, 0, 1, 0)
    assert np.isnan(gf[G_GRAD_NORM])
    assert (wi[A_WINDOWS], wi[A_DROPPED]) == (1, 0)       # not a bad-loss drop
    ar.unchanged(got, STATE)
    if scaled:
        assert (gi_[G_MODE], gi_[G_POISONED]) == (2, 0)
        ar.grads_zeroed(got)
        si, sf = _words(ls)
        assert sf[amp.LS_SCALE] == 2.0 ** 15 and sf[amp.LS_UNSCALE] == 2.0 ** -16
        assert (si[amp.LS_TRACKER], si[amp.LS_OVERFLOWS], si[amp.LS_GROWTHS]) == (0, 1, 0)
    else:
        assert (gi_[G_MODE], gi_[G_POISONED]) == (0, 1)
        _same_bits(got, before)                            # kept, the inf too
    ar.outside_unchanged(got)


# ------------------------------------------------------------------------------------- (f)
def test_growth_tracker_moves_once_per_window():
    from mauv import amp
    from mauv.optim import G_STEP, A_WINDOWS
    ar = _arena(51)
    gate, acc, ls = _gate(), _accum(), _scaler(1024.0, interval=2)
    for w in range(2):
        _note(gate, acc)
        si, sf = _words(ls)
        assert si[amp.LS_TRACKER] == w and sf[amp.LS_SCALE] == 1024.0   # note leaves it alone
        _close(ar, gate, ls, acc)
    si, sf = _words(ls)
    assert sf[amp.LS_SCALE] == 2048.0 and sf[amp.LS_UNSCALE] == 2.0 ** -10
    assert (si[amp.LS_TRACKER], si[amp.LS_GROWTHS], si[amp.LS_OVERFLOWS]) == (0, 1, 0)
    assert _words(gate)[0][G_STEP] == T + 1 and _words(acc)[0][A_WINDOWS] == 2


# ------------------------------------------------------------------------------------- (g)
@pytest.mark.parametrize("ok_loss", [1, 0])
def test_note_touches_its_words_only(ok_loss):
    from mauv.optim import (GATE_WORDS, G_OK_LOSS, G_MODE, G_STEPPED, G_SKIP_LOSS, ACC_WORDS,
                            A_MICRO, A_BAD_LOSS)
    ar = _arena(61)
    before = ar.result()
    g0 = np.arange(100, 100 + GATE_WORDS, dtype=np.int32)     # every word a value of its own
    a0 = np.arange(200, 200 + ACC_WORDS, dtype=np.int32)
    gate, acc = torch.tensor(g0, device=dev), torch.tensor(a0, device=dev)
    _note(gate, acc, ok_loss)
    g1, a1 = _words(gate)[0], _words(acc)[0]
    want_g, want_a = g0.copy(), a0.copy()
    want_g[G_OK_LOSS] = ok_loss                                # (the caller's write)
    want_g[G_MODE], want_g[G_STEPPED] = 0, 0
    want_a[A_MICRO] += 1
    if not ok_loss:
        want_g[G_SKIP_LOSS] += 1
        want_a[A_BAD_LOSS] += 1
    assert np.array_equal(g1, want_g) and np.array_equal(a1, want_a)
    _same_bits(ar.result(), before)
