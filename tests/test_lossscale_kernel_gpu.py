"""mauv_adam_step_ex_scaled (csrc/adam.hip) on hand-built tables, in the manner of
tests/test_adam_ex_kernel_gpu.py (its Arena, its measure and its bar): rows of 1, 3, 4, 5 and
1027 elements, each once with every pointer 16-byte aligned and once with all of them one float
later, interleaved over two parameter groups whose option flags run through 0..7; the gradients
stand for those of ``loss * scale`` with scale 1, 2^16 and 3, with and without ``max_norm``.

The reference is tests/adam_ref.py in float64 from the gradient the kernel is documented to load,
fl32(fl32(g * unscale) * clip_coef); the kernel may err 4x what the fp32 restatement errs on the
same inputs, floored at 1 unit — the bar of the unscaled kernel.  The decision's words are held
bit for bit: unscale = fl32(1 / (double)scale), grad_norm = fl32(scanned norm * unscale), the
coefficient from that.  An inf in one row skips the step, zeroes every gradient, backs the scale
off and resets the tracker; the tracker reaching the interval grows the scale unless the product
is not finite; a static scale never changes; a non-finite loss leaves the scaler alone.  A null
scaler equals mauv_adam_step_ex bit for bit, and scale 1 over one plain group equals
mauv_adam_step_gated bit for bit.

Measured on an MI355X, kernel units p / m / v / vmax over all flag pairs (fp32 restatement; bar =
4x it):
  scale 1     no clip 3.48 / 2.17 / 2.25 / 1.69 (3.61 / 2.67 / 3.45 / 1.72)
              clip    3.62 / 2.08 / 2.37 / 1.76 (3.52 / 2.25 / 2.37 / 1.86)
  scale 2^16  no clip 3.42 / 1.12 / 1.64 / 1.64 (3.42 / 1.12 / 2.07 / 2.07)
              clip    3.42 / 1.19 / 1.92 / 1.60 (3.42 / 1.19 / 2.06 / 1.84)
  scale 3     no clip 3.57 / 2.26 / 1.95 / 1.77 (4.23 / 2.27 / 2.80 / 2.80)
              clip    3.30 / 2.06 / 1.82 / 1.82 (3.30 / 2.08 / 1.99 / 1.73)"""
import ctypes

import numpy as np
import pytest
import torch

from tests import adam_ref as A
from tests import kernel_ref as R
from tests.test_adam_ex_kernel_gpu import Arena, KINDS

pytestmark = pytest.mark.gpu

dev = "cuda"
F32 = np.float32
NUMEL = [1, 3, 4, 5, 1027]
T = 7
FLAG_PAIRS = [(0, 7), (1, 6), (2, 5), (3, 4)]          # every combination 0..7, two per launch


def _groups(f0, f1):
    # lr, beta1, beta2, eps, weight_decay, flags
    return [(1e-3, 0.9, 0.999, 1e-8, 1e-5, f0), (3e-4, 0.8, 0.99, 1e-6, 1e-2, f1)]


def _entries(groups=2):
    """Aligned rows, then the same sizes as views at a 4-byte offset; the groups alternate, so
    each holds aligned and shifted rows (and, over the two halves, every size)."""
    ent = [(n, None) for n in NUMEL] + [(n, "all") for n in NUMEL]
    return [(n, sh, e % groups) for e, (n, sh) in enumerate(ent)]


def _gate(max_norm=0.0, ok_loss=1, step=T - 1):
    from mauv.optim import GATE_WORDS, G_OK_LOSS, G_STEP, G_MAX_NORM
    g = np.zeros(GATE_WORDS, dtype=np.int32)
    g[G_OK_LOSS], g[G_STEP] = ok_loss, step
    g.view(F32)[G_MAX_NORM] = max_norm
    return torch.tensor(g, device=dev)


def _scaler(scale, interval=1000, tracker=0, growth=2.0, backoff=0.5):
    from mauv import amp
    w = np.zeros(amp.LS_WORDS, dtype=np.int32)
    f = w.view(F32)
    f[amp.LS_SCALE], f[amp.LS_GROWTH], f[amp.LS_BACKOFF] = scale, growth, backoff
    f[amp.LS_UNSCALE] = np.nan                  # the library writes it before it reads it
    w[amp.LS_INTERVAL], w[amp.LS_TRACKER] = interval, tracker
    return torch.tensor(w, device=dev)


def _words(t):
    w = t.cpu().numpy()
    return w, w.view(F32)


def _step(ar, gate, ls):
    from mauv import ops
    from mauv._lib import lib, check
    tab, arr = ar.table(), ar.group_array()
    check(lib.mauv_adam_step_ex_scaled(tab.data_ptr(), len(ar.entries), ctypes.addressof(arr),
                                       len(ar.groups), gate.data_ptr(),
                                       None if ls is None else ls.data_ptr(), ops.stream()),
          "adam_step_ex_scaled")
    return ar.result()


def _scan(ar, gate):
    """The fused scan over the rows' gradients into the gate's grad_norm / nonfinite words."""
    from mauv import ops
    from mauv.optim import G_GRAD_NORM, G_NONFINITE
    rows = [(ar.dev["g"].data_ptr() + 4 * ar.start["g"][e], n)
            for e, (n, _, _) in enumerate(ar.entries)]
    ws = torch.empty(ops.grad_norm_workspace_bytes(len(rows)), dtype=torch.uint8, device=dev)
    ops.grad_norm(ops.span_table(rows, dev), 0, ws,
                  gate[G_GRAD_NORM:G_GRAD_NORM + 1].view(torch.float32),
                  gate[G_NONFINITE:G_NONFINITE + 1])
    torch.cuda.synchronize()


def _true_norm(ar, scale):
    g = np.concatenate([ar.view(ar.host["g"], "g", e) for e in range(len(ar.entries))])
    return float(np.sqrt(np.sum(g.astype(np.float64) ** 2)) / scale)


@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
@pytest.mark.parametrize("scale", [1.0, 2.0 ** 16, 3.0])
def test_scaled_step_against_float64(scale, clip):
    from mauv import amp
    from mauv.optim import G_MODE, G_STEP, G_STEPPED, G_NONFINITE, G_GRAD_NORM, G_CLIP_COEF
    unscale = F32(1.0 / float(F32(scale)))
    fig = np.zeros((2, 4))
    for f0, f1 in FLAG_PAIRS:
        ar = Arena(_entries(), seed=100 + f0, groups=_groups(f0, f1))
        c = _true_norm(ar, scale) / 2 if clip else 0.0
        gate, ls = _gate(c), _scaler(scale)
        coef = F32(1.0)
        if clip:
            _scan(ar, gate)
            scanned = _words(gate)[1][G_GRAD_NORM]
            norm = scanned * unscale
            assert norm.dtype == np.float32
            coef = F32(min(1.0, float(F32(c)) / (float(norm) + 1e-6)))
            assert 0.49 < coef < 0.51               # clipping is active
        got = _step(ar, gate, ls)
        gi_, gf = _words(gate)
        si, sf = _words(ls)
        assert (gi_[G_MODE], gi_[G_STEP], gi_[G_STEPPED], gi_[G_NONFINITE]) == (3, T, 1, 0)
        assert sf[amp.LS_UNSCALE].view(np.int32) == unscale.view(np.int32)
        assert sf[amp.LS_SCALE] == F32(scale) and si[amp.LS_TRACKER] == 1
        assert (si[amp.LS_OVERFLOWS], si[amp.LS_GROWTHS]) == (0, 0)
        assert gf[G_CLIP_COEF].view(np.int32) == coef.view(np.int32)
        if clip:
            assert gf[G_GRAD_NORM].view(np.int32) == norm.view(np.int32)
            assert abs(float(norm) - 2 * c) <= 2 * c * 2.0 ** -22   # the true norm
        ar.outside_unchanged(got)
        ar.grads_zeroed(got)
        for e, (n, _, gi) in enumerate(ar.entries):
            k = A.consts(*ar.groups[gi][:5], T, ar.groups[gi][5])
            p, g, m, v, x = (ar.view(ar.host[kk], kk, e) for kk in KINDS)
            gl = (g * unscale) * coef               # two fp32 roundings, torch's order
            assert gl.dtype == np.float32
            ref, r32 = A.adam64(p, gl, m, v, x, k), A.adam32(p, gl, m, v, x, k)
            for j, kk in enumerate(("p", "m", "v", "x")):
                if ref[j] is None:
                    continue
                fig[0, j] = max(fig[0, j], R.units(ar.view(got[kk], kk, e), *ref[j]))
                fig[1, j] = max(fig[1, j], R.units(r32[j], *ref[j]))
    print(f"scaled adam scale={scale} clip={clip}: kernel p/m/v/vmax {fig[0]} units, "
          f"fp32 restatement {fig[1]}")
    for j, name in enumerate(("p", "m", "v", "vmax")):
        assert fig[0, j] <= R.bar(fig[1, j]), (name, fig[:, j])


@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
@pytest.mark.parametrize("dynamic", [True, False], ids=["dynamic", "static"])
def test_one_inf_skips_zeroes_and_backs_off(dynamic, clip):
    from mauv import amp
    from mauv.optim import (G_MODE, G_STEP, G_STEPPED, G_NONFINITE, G_POISONED, G_SKIP_GRAD,
                            G_SKIP_LOSS, G_GRAD_NORM)
    ar = Arena(_entries(), seed=7, groups=_groups(0, 5))
    e_bad = 7                                        # a shifted 4-element row
    ar.dev["g"][ar.start["g"][e_bad] + 2] = float("inf")
    gate = _gate(1.0 if clip else 0.0)
    ls = _scaler(2.0 ** 16, interval=5 if dynamic else 0, tracker=3 if dynamic else 0)
    _scan(ar, gate)
    assert _words(gate)[0][G_NONFINITE] > 0
    got = _step(ar, gate, ls)
    gi_, gf = _words(gate)
    si, sf = _words(ls)
    assert (gi_[G_MODE], gi_[G_STEP], gi_[G_STEPPED], gi_[G_POISONED]) == (2, T - 1, 0, 0)
    assert (gi_[G_SKIP_GRAD], gi_[G_SKIP_LOSS], gi_[G_NONFINITE]) == (1, 0, 0)
    assert np.isnan(gf[G_GRAD_NORM])                 # the scanned NaN stays NaN
    assert sf[amp.LS_SCALE] == (2.0 ** 15 if dynamic else 2.0 ** 16)
    assert sf[amp.LS_UNSCALE] == 2.0 ** -16          # of the scale the backward ran with
    assert (si[amp.LS_TRACKER], si[amp.LS_OVERFLOWS], si[amp.LS_GROWTHS]) == (0, 1, 0)
    assert si[amp.LS_INTERVAL] == (5 if dynamic else 0)
    ar.unchanged(got, ("p", "m", "v", "x"))
    ar.grads_zeroed(got)                             # the inf went with the rest
    ar.outside_unchanged(got)


def test_growth_static_scale_and_nonfinite_loss():
    from mauv import amp
    from mauv.optim import G_MODE, G_STEP, G_SKIP_LOSS
    # the tracker reaches the interval: the scale grows
    ar = Arena(_entries(), seed=8, groups=_groups(0, 0))
    gate, ls = _gate(), _scaler(3.0, interval=4, tracker=3, growth=1.5)
    got = _step(ar, gate, ls)
    si, sf = _words(ls)
    assert sf[amp.LS_SCALE] == 4.5 and sf[amp.LS_UNSCALE] == F32(1.0 / 3.0)
    assert (si[amp.LS_TRACKER], si[amp.LS_OVERFLOWS], si[amp.LS_GROWTHS]) == (0, 0, 1)
    assert _words(gate)[0][G_STEP] == T
    ar.grads_zeroed(got)
    # ... one step earlier it only counts
    gate, ls = _gate(), _scaler(3.0, interval=4, tracker=2, growth=1.5)
    _step(Arena(_entries(), seed=8, groups=_groups(0, 0)), gate, ls)
    si, sf = _words(ls)
    assert sf[amp.LS_SCALE] == 3.0 and (si[amp.LS_TRACKER], si[amp.LS_GROWTHS]) == (3, 0)
    # ... and a product that is not finite is not taken (torch's _amp_update_scale_)
    gate, ls = _gate(), _scaler(2.0 ** 127, interval=1, tracker=0)
    _step(Arena(_entries(), seed=8, groups=_groups(0, 0)), gate, ls)
    si, sf = _words(ls)
    assert sf[amp.LS_SCALE] == 2.0 ** 127 and si[amp.LS_TRACKER] == 0
    # a static scale never changes and counts nothing
    gate, ls = _gate(), _scaler(1024.0, interval=0)
    for t in range(3):
        _step(Arena(_entries(), seed=9 + t, groups=_groups(0, 0)), gate, ls)
    si, sf = _words(ls)
    assert sf[amp.LS_SCALE] == 1024.0 and sf[amp.LS_UNSCALE] == 2.0 ** -10
    assert (si[amp.LS_INTERVAL], si[amp.LS_TRACKER], si[amp.LS_GROWTHS]) == (0, 0, 0)
    assert _words(gate)[0][G_STEP] == T + 2
    # a non-finite loss: today's branch (mode 2 on a clean arena), the scaler is not touched
    ar = Arena(_entries(), seed=12, groups=_groups(0, 0))
    gate, ls = _gate(ok_loss=0), _scaler(2.0 ** 16, interval=2, tracker=1)
    got = _step(ar, gate, ls)
    gi_, _ = _words(gate)
    si, sf = _words(ls)
    assert (gi_[G_MODE], gi_[G_STEP], gi_[G_SKIP_LOSS]) == (2, T - 1, 1)
    assert sf[amp.LS_SCALE] == 2.0 ** 16
    assert (si[amp.LS_TRACKER], si[amp.LS_OVERFLOWS], si[amp.LS_GROWTHS]) == (1, 0, 0)
    ar.unchanged(got, ("p", "m", "v", "x"))
    ar.grads_zeroed(got)


def _same_bits(a, b):
    for k in KINDS:
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), k


def test_null_scaler_and_unit_scale_equal_the_existing_entries_bitwise():
    from mauv import ops
    from mauv._lib import lib, check
    # a null scaler: mauv_adam_step_ex's gated form, clipping on, every flag
    for f0, f1 in FLAG_PAIRS:
        new = Arena(_entries(), seed=30 + f0, groups=_groups(f0, f1))
        old = Arena(_entries(), seed=30 + f0, groups=_groups(f0, f1))
        c = _true_norm(new, 1.0) / 2
        g_new, g_old = _gate(c), _gate(c)
        _scan(new, g_new)
        _scan(old, g_old)
        a = _step(new, g_new, None)
        assert old.step(0, g_old) == 0
        b = old.result()
        _same_bits(a, b)
        assert np.array_equal(_words(g_new)[0], _words(g_old)[0])
        assert not np.array_equal(a["p"].view(np.int32), new.host["p"].view(np.int32))
    # scale 1 over one plain group: mauv_adam_step_gated (x * 1 is x; flags 0 is adam_elem)
    ent = _entries(groups=1)
    new = Arena(ent, seed=40, groups=_groups(0, 0)[:1])
    old = Arena(ent, seed=40, groups=_groups(0, 0)[:1])
    c = _true_norm(new, 1.0) / 2
    g_new, g_old = _gate(c), _gate(c)
    _scan(new, g_new)
    _scan(old, g_old)
    a = _step(new, g_new, _scaler(1.0))
    lr, b1, b2, eps, wd, _ = _groups(0, 0)[0]
    tab = old.table4()
    check(lib.mauv_adam_step_gated(tab.data_ptr(), len(ent), lr, b1, b2, eps, wd,
                                   g_old.data_ptr(), ops.stream()), "adam_step_gated")
    _same_bits(a, old.result())
    assert np.array_equal(_words(g_new)[0], _words(g_old)[0])
