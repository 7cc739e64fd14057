"""mauv_adam_step_ex_ema / mauv_ema_update / mauv_ema_swap (csrc/adam.hip) on hand-built tables,
with the Arena of tests/test_adam_ex_kernel_gpu.py and a sixth flat buffer for the shadows.

Rows of 1, 3, 4, 5, 1023 and 65536 + 5 elements with every pointer 16-byte aligned (one grid is
64 x 256 threads x 4 floats = 65536 elements per stride, so the last row takes a second stride
and a scalar tail), a 1023-element row whose shadow alone is a view one float later (read and
written float by float: the row keeps the vector loop it takes without a shadow, whose bits the
scalar loop does not give) and a 1023-element row with a NULL shadow, over two parameter groups.
The option flags 0 and 7 meet every row size (the groups swap between two launches); the single
flags 1, 2, 4 ride on two more.

(1) fused == unfused, bit for bit: p, m, v, vmax, the zeroed gradients and the shadows equal
    mauv_adam_step_ex_accum on a copy of the inputs followed by mauv_ema_update at the weight the
    MauvEma reports.
(2) w == 1 (the first update): the shadow is the new p, bit for bit.
(3) Against float64 from the device's own inputs: e64 = e + w (p - e), in units of 2^-24 of
    |e| + w (|p| + |e|) (tests/kernel_ref.py), the kernel erring at most 4x what the one-fp32-
    operation restatement fl(fma(w, fl(p - e), e)) errs, floored at one unit.
(4) Every decision but "Adam step" leaves the MauvEma and every shadow as they are, bit for bit;
    a clean window of 3 moves ``updates`` by exactly 1.
(5) The warm-up: the weight of updates 1..12.
(6) The NULL-shadow row steps, and every float outside the shadow views is intact.
(7) ema == NULL (or ema_rows == NULL) is mauv_adam_step_ex_accum, bit for bit.
(8) Argument errors answer negative and launch nothing.
(9) mauv_ema_swap exchanges exactly; twice is the identity.

Measured on an MI355X, (3): kernel 1.56 / 1.55 / 1.62 / 1.41 units for the flag pairs (0, 7),
(7, 0), (1, 2), (4, 0), the fp32 restatement the same figures (bar: 4x, floored at 4)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import kernel_ref as R
from tests.test_adam_ex_kernel_gpu import Arena, KINDS, PAD
from tests.test_lossscale_kernel_gpu import _gate, _scaler, _words, T

pytestmark = pytest.mark.gpu

dev = "cuda"
F32 = np.float32
SIZES = [1, 3, 4, 5, 1023, 65536 + 5]
# (numel, "e" = the shadow is a view one float later / "null" = no shadow / None)
SHAPES = [(n, None) for n in SIZES] + [(1023, "e"), (1023, "null")]
FLAG_PAIRS = [(0, 7), (7, 0), (1, 2), (4, 0)]
DECAY = 0.9


def _groups(f0, f1):
    # lr, beta1, beta2, eps, weight_decay, flags
    return [(1e-3, 0.9, 0.999, 1e-8, 1e-5, f0), (3e-4, 0.8, 0.99, 1e-6, 1e-2, f1)]


class EmaArena(Arena):
    """The Arena with a shadow view per row in a flat buffer of its own (guards on both sides,
    as for the other kinds): aligned, one float later, or absent."""

    def __init__(self, seed, flags=(0, 7), shapes=SHAPES):
        entries = [(n, None, i % 2) for i, (n, _) in enumerate(shapes)]
        super().__init__(entries, seed=seed, groups=_groups(*flags))
        self.shapes = shapes
        rng = np.random.default_rng(seed + 1000)
        self.e_start = [s + (1 if sh == "e" else 0) for s, (_, sh) in zip(self.start["p"], shapes)]
        self.e_host = rng.standard_normal(self.total).astype(np.float32)
        self.e_dev = torch.tensor(self.e_host, device=dev)
        assert self.e_dev.data_ptr() % 16 == 0

    def e_view(self, arr, i):
        return arr[self.e_start[i]:self.e_start[i] + self.entries[i][0]]

    def has_shadow(self, i):
        return self.shapes[i][1] != "null"

    def shadow_table(self):
        ptrs = np.array([self.e_dev.data_ptr() + 4 * self.e_start[i] if self.has_shadow(i) else 0
                         for i in range(len(self.entries))], dtype=np.int64)
        for i, (_, sh) in enumerate(self.shapes):
            assert (ptrs[i] % 16 != 0) == (sh == "e")
        return torch.tensor(ptrs, device=dev)

    def row_table(self):
        """MauvEmaRow rows (shadow, parameter, numel) of the rows that have a shadow."""
        rows = [(self.e_dev.data_ptr() + 4 * self.e_start[i],
                 self.dev["p"].data_ptr() + 4 * self.start["p"][i], self.entries[i][0])
                for i in range(len(self.entries)) if self.has_shadow(i)]
        return torch.tensor(np.array(rows, dtype=np.int64), device=dev), len(rows)

    def step_ema(self, gate, ema, ls=None, acc=None, shadows=True):
        from mauv import ops
        from mauv._lib import lib, check
        tab, arr = self.table(), self.group_array()
        sh = self.shadow_table() if shadows else None
        check(lib.mauv_adam_step_ex_ema(
            tab.data_ptr(), len(self.entries), ctypes.addressof(arr), len(self.groups),
            gate.data_ptr(), None if ls is None else ls.data_ptr(),
            None if acc is None else acc.data_ptr(), None if sh is None else sh.data_ptr(),
            None if ema is None else ema.data_ptr(), ops.stream()), "adam_step_ex_ema")
        return self.all()

    def step_accum(self, gate, ls=None, acc=None):
        from mauv import ops
        from mauv._lib import lib, check
        tab, arr = self.table(), self.group_array()
        check(lib.mauv_adam_step_ex_accum(
            tab.data_ptr(), len(self.entries), ctypes.addressof(arr), len(self.groups),
            gate.data_ptr(), None if ls is None else ls.data_ptr(),
            None if acc is None else acc.data_ptr(), ops.stream()), "adam_step_ex_accum")
        return self.all()

    def update(self, w):
        from mauv import ops
        from mauv._lib import lib, check
        rows, n = self.row_table()
        check(lib.mauv_ema_update(rows.data_ptr(), n, w, ops.stream()), "ema_update")
        return self.all()

    def swap(self):
        from mauv import ops
        from mauv._lib import lib, check
        rows, n = self.row_table()
        check(lib.mauv_ema_swap(rows.data_ptr(), n, ops.stream()), "ema_swap")
        return self.all()

    def all(self):
        got = self.result()
        got["e"] = self.e_dev.cpu().numpy()
        return got

    def shadows_outside_unchanged(self, got):
        """Every float of the shadow buffer outside the views, and the whole span of a row with
        a NULL shadow."""
        out = np.ones(self.total, dtype=bool)
        for i, (n, _, _) in enumerate(self.entries):
            if self.has_shadow(i):
                out[self.e_start[i]:self.e_start[i] + n] = False
        assert np.array_equal(got["e"][out].view(np.int32), self.e_host[out].view(np.int32)), \
            "a float outside the shadow views changed"

    def shadows_unchanged(self, got):
        assert np.array_equal(got["e"].view(np.int32), self.e_host.view(np.int32))


def _ema(decay=DECAY, warmup=0, updates=0):
    from mauv.optim import EMA_WORDS, E_DECAY, E_WARMUP, E_UPDATES, E_WEIGHT
    w = np.zeros(EMA_WORDS, dtype=np.int32)
    w.view(F32)[E_DECAY] = decay
    w[E_WARMUP], w[E_UPDATES] = warmup, updates
    if updates:
        w.view(F32)[E_WEIGHT] = np.nan          # the library writes it before it is read
    return torch.tensor(w, device=dev)


def _accum():
    from mauv.optim import ACC_WORDS
    return torch.zeros(ACC_WORDS, dtype=torch.int32, device=dev)


def _same_bits(a, b, kinds=KINDS + ("e",)):
    for k in kinds:
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), k


def _weight(decay, warmup, n):
    if n == 0:
        return F32(1.0)
    d = float(F32(decay))
    if warmup:
        d = min(d, (1.0 + n) / (10.0 + n))
    return F32(1.0 - d)


# --------------------------------------------------------------------- (1) (2) (3) (6)
@pytest.mark.parametrize("updates", [0, 3], ids=["first", "fourth"])
@pytest.mark.parametrize("flags", FLAG_PAIRS, ids=lambda f: f"flags{f[0]}{f[1]}")
def test_fused_equals_unfused_and_float64(flags, updates):
    from mauv.optim import G_MODE, G_STEP, G_STEPPED, E_UPDATES, E_WEIGHT, E_DECAY, E_WARMUP
    new, old = EmaArena(5 + flags[0], flags), EmaArena(5 + flags[0], flags)
    g_new, g_old, ema = _gate(), _gate(), _ema(updates=updates)
    got = new.step_ema(g_new, ema)
    ei, ef = _words(ema)
    w = ef[E_WEIGHT]
    assert ei[E_UPDATES] == updates + 1 and ei[E_WARMUP] == 0 and not ei[4:].any()
    assert ef[E_DECAY] == F32(DECAY)
    assert w.view(np.int32) == _weight(DECAY, 0, updates).view(np.int32)
    gi_ = _words(g_new)[0]
    assert (gi_[G_MODE], gi_[G_STEP], gi_[G_STEPPED]) == (3, T, 1)
    # (1) the unfused pair on a copy of the inputs
    mid = old.step_accum(g_old)
    assert np.array_equal(_words(g_new)[0], _words(g_old)[0])         # all 16 gate words
    _same_bits(got, mid, KINDS)
    old.shadows_unchanged(mid)
    ref = old.update(float(w))
    _same_bits(got, ref)
    # (6) the guards of all six buffers, the NULL row's shadow span, the gradients
    new.outside_unchanged(got)
    new.shadows_outside_unchanged(got)
    new.grads_zeroed(got)
    fig = np.zeros(2)
    for i, (n, _, _) in enumerate(new.entries):
        p1 = new.view(got["p"], "p", i)
        assert not np.array_equal(p1.view(np.int32), new.view(new.host["p"], "p", i).view(np.int32))
        if not new.has_shadow(i):
            continue
        e0, e1 = new.e_view(new.e_host, i), new.e_view(got["e"], i)
        if updates == 0:                                               # (2)
            assert w == 1.0 and np.array_equal(e1.view(np.int32), p1.view(np.int32))
            continue
        # (3) float64 from the device's own inputs, and the one-fp32-operation restatement
        p64, e64, w64 = p1.astype(np.float64), e0.astype(np.float64), float(w)
        want = e64 + w64 * (p64 - e64)
        scale = np.abs(e64) + w64 * (np.abs(p64) + np.abs(e64))
        d32 = p1 - e0
        assert d32.dtype == np.float32
        r32 = (w64 * d32.astype(np.float64) + e64).astype(np.float32)  # the product is exact
        fig[0] = max(fig[0], R.units(e1, want, scale))
        fig[1] = max(fig[1], R.units(r32, want, scale))
    if updates:
        print(f"ema flags={flags}: kernel {fig[0]:.2f} units, fp32 restatement {fig[1]:.2f}")
        assert fig[0] <= R.bar(fig[1]), fig


def test_fused_equals_unfused_under_a_scaler_and_a_window():
    """The same with a loss scaler and a window of one beside the gate: the EMA entry takes
    mauv_adam_step_ex_accum's decision whatever else stands beside the gate."""
    from mauv.optim import E_UPDATES, E_WEIGHT
    new, old = EmaArena(21), EmaArena(21)
    g_new, g_old, ema = _gate(), _gate(), _ema(updates=9)
    l_new, l_old = _scaler(3.0, interval=1), _scaler(3.0, interval=1)
    a_new, a_old = _accum(), _accum()
    got = new.step_ema(g_new, ema, l_new, a_new)
    old.step_accum(g_old, l_old, a_old)
    ei, ef = _words(ema)
    assert ei[E_UPDATES] == 10 and ef[E_WEIGHT] == F32(1.0 - float(F32(DECAY)))
    _same_bits(got, old.update(float(ef[E_WEIGHT])))
    for a, b in ((g_new, g_old), (l_new, l_old), (a_new, a_old)):
        assert np.array_equal(_words(a)[0], _words(b)[0])
    assert _words(l_new)[1][0] == 6.0                                   # (it grew: interval 1)


# ------------------------------------------------------------------------------------- (4)
def _note(gate, acc, ok_loss):
    from mauv import ops
    from mauv._lib import lib, check
    from mauv.optim import G_OK_LOSS
    gate[G_OK_LOSS] = ok_loss
    check(lib.mauv_accum_note(gate.data_ptr(), acc.data_ptr(), ops.stream()), "accum_note")
    torch.cuda.synchronize()


@pytest.mark.parametrize("case", ["bad_loss", "nonfinite", "overflow", "poisoned", "bad_window"])
def test_every_other_decision_leaves_the_average_alone(case):
    from mauv.optim import G_MODE, G_STEP, G_STEPPED, G_NONFINITE, G_POISONED
    ar = EmaArena(31)
    ema = _ema(warmup=1, updates=4)
    before = _words(ema)[0].copy()
    gate = _gate(ok_loss=0 if case in ("bad_loss", "poisoned") else 1)
    ls = _scaler(2.0 ** 16, interval=5, tracker=3) if case == "overflow" else None
    acc = _accum() if case == "bad_window" else None
    if case in ("nonfinite", "overflow"):
        gate[G_NONFINITE] = 2
    if case == "poisoned":
        gate[G_POISONED] = 1
    if case == "bad_window":
        _note(gate, acc, 1)
        _note(gate, acc, 0)
        assert np.array_equal(_words(ema)[0], before)                  # (mauv_accum_note)
        gate[0] = 1
    got = ar.step_ema(gate, ema, ls, acc)
    gi_ = _words(gate)[0]
    mode = {"bad_loss": 2, "nonfinite": 0, "overflow": 2, "poisoned": 0, "bad_window": 2}[case]
    assert (gi_[G_MODE], gi_[G_STEP], gi_[G_STEPPED]) == (mode, T - 1, 0)
    assert np.array_equal(_words(ema)[0], before)                       # all 8 words
    ar.shadows_unchanged(got)
    ar.unchanged(got, ("p", "m", "v", "x"))
    if mode == 2:
        ar.grads_zeroed(got)
    else:
        ar.unchanged(got, ("g",))


def test_a_clean_window_of_three_moves_the_average_once():
    from mauv.optim import G_STEP, E_UPDATES, E_WEIGHT, A_WINDOWS
    ar = EmaArena(41)
    gate, acc, ema = _gate(), _accum(), _ema(updates=2)
    before = _words(ema)[0].copy()
    for _ in range(2):
        _note(gate, acc, 1)
        assert np.array_equal(_words(ema)[0], before)
        ar.shadows_unchanged(ar.all())
    got = ar.step_ema(gate, ema, None, acc)
    ei, ef = _words(ema)
    assert ei[E_UPDATES] == 3 and ef[E_WEIGHT] == F32(1.0 - float(F32(DECAY)))
    assert _words(gate)[0][G_STEP] == T and _words(acc)[0][A_WINDOWS] == 1
    assert not np.array_equal(got["e"].view(np.int32), ar.e_host.view(np.int32))
    ar.shadows_outside_unchanged(got)


# ------------------------------------------------------------------------------------- (5)
@pytest.mark.parametrize("warmup", [1, 0])
def test_warmup_weights_of_twelve_updates(warmup):
    from mauv.optim import E_UPDATES, E_WEIGHT
    decay = 0.999
    ar = EmaArena(51, shapes=[(5, None), (3, "e")])
    gate, ema = _gate(), _ema(decay=decay, warmup=warmup)
    for k in range(1, 13):
        ar.step_ema(gate, ema)
        ei, ef = _words(ema)
        n = k - 1                                     # updates taken before this one
        want = F32(1.0) if n == 0 else \
            F32(1.0 - min(float(F32(decay)), (1.0 + n) / (10.0 + n)) if warmup
                else 1.0 - float(F32(decay)))
        assert ei[E_UPDATES] == k
        assert ef[E_WEIGHT].view(np.int32) == want.view(np.int32), (k, ef[E_WEIGHT], want)
    assert _words(gate)[0][4] == T - 1 + 12


# ------------------------------------------------------------------------------------- (7)
@pytest.mark.parametrize("null", ["ema", "rows", "both"])
def test_null_ema_is_the_accum_entry_bitwise(null):
    new, old = EmaArena(61, (7, 0)), EmaArena(61, (7, 0))
    g_new, g_old, ema = _gate(), _gate(), _ema()
    before = _words(ema)[0].copy()
    l_new, l_old = _scaler(3.0), _scaler(3.0)
    a_new, a_old = _accum(), _accum()
    got = new.step_ema(g_new, None if null in ("ema", "both") else ema, l_new, a_new,
                       shadows=null == "ema")
    ref = old.step_accum(g_old, l_old, a_old)
    _same_bits(got, ref)
    new.shadows_unchanged(got)
    for a, b in ((g_new, g_old), (l_new, l_old), (a_new, a_old)):
        assert np.array_equal(_words(a)[0], _words(b)[0])
    assert np.array_equal(_words(ema)[0], before)
    assert not np.array_equal(got["p"].view(np.int32), new.host["p"].view(np.int32))


# ------------------------------------------------------------------------------------- (8)
def test_argument_errors_launch_nothing():
    from mauv import ops
    from mauv._lib import lib
    ar = EmaArena(71)
    gate, ema = _gate(), _ema()
    g0, e0 = _words(gate)[0].copy(), _words(ema)[0].copy()
    tab, arr, sh = ar.table(), ar.group_array(), ar.shadow_table()
    n, grp = len(ar.entries), ctypes.addressof(arr)
    t, gp, sp, ep = tab.data_ptr(), gate.data_ptr(), sh.data_ptr(), ema.data_ptr()
    for a in [(None, n, grp, 2, gp), (t, 0, grp, 2, gp), (t, -1, grp, 2, gp),
              (t, 65536, grp, 2, gp), (t, n, None, 2, gp), (t, n, grp, 0, gp),
              (t, n, grp, 9, gp), (t, n, grp, 2, None)]:
        assert lib.mauv_adam_step_ex_ema(*a, None, None, sp, ep, ops.stream()) < 0, a[1:4:2]
        assert b"adam_step_ex_ema" in lib.mauv_last_error()
    rows, nr = ar.row_table()
    for r, k, w in ((None, nr, 0.5), (rows.data_ptr(), 0, 0.5), (rows.data_ptr(), 65536, 0.5),
                    (rows.data_ptr(), nr, 0.0), (rows.data_ptr(), nr, 1.5),
                    (rows.data_ptr(), nr, float("nan"))):
        assert lib.mauv_ema_update(r, k, w, ops.stream()) < 0
        assert b"ema_update" in lib.mauv_last_error()
    for r, k in ((None, nr), (rows.data_ptr(), 0), (rows.data_ptr(), 65536)):
        assert lib.mauv_ema_swap(r, k, ops.stream()) < 0
        assert b"ema_swap" in lib.mauv_last_error()
    got = ar.all()
    ar.unchanged(got, KINDS)
    ar.shadows_unchanged(got)
    assert np.array_equal(_words(gate)[0], g0) and np.array_equal(_words(ema)[0], e0)


# ------------------------------------------------------------------------------------- (9)
def test_swap_exchanges_exactly_and_twice_is_the_identity():
    ar = EmaArena(81)
    once = ar.swap()
    for i, (n, _, _) in enumerate(ar.entries):
        p0, e0 = ar.view(ar.host["p"], "p", i), ar.e_view(ar.e_host, i)
        p1, e1 = ar.view(once["p"], "p", i), ar.e_view(once["e"], i)
        if ar.has_shadow(i):
            assert np.array_equal(p1.view(np.int32), e0.view(np.int32)), i
            assert np.array_equal(e1.view(np.int32), p0.view(np.int32)), i
        else:
            assert np.array_equal(p1.view(np.int32), p0.view(np.int32)), i
    ar.outside_unchanged(once)
    ar.shadows_outside_unchanged(once)
    ar.unchanged(once, ("g", "m", "v", "x"))
    twice = ar.swap()
    ar.unchanged(twice, KINDS)
    ar.shadows_unchanged(twice)
