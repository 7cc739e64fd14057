"""mauv_adam_step_ex (csrc/adam.hip) on a hand-built table, in the manner of
tests/test_adam_kernel_gpu.py: three parameter groups with different lr, betas, eps, weight decay
and options (none; amsgrad + decoupled decay; maximize) interleaved over the rows of ONE launch,
against the float64 update from the same fp32 inputs and constants (tests/adam_ref.py).  Rows of
1, 3, 4, 5 and 65543 elements, each once with every pointer 16-byte aligned and once with one of
the (up to five) pointers one float later, plus a 32773-element row with all of them shifted;
the floats around every view are checked bit-unchanged.  max_exp_avg_sq starts at half or twice
the new second moment, so the maximum is taken both ways.  One group with no option equals
mauv_adam_step bit for bit; the gated form (modes 3, 2, 0) and the argument errors follow.

Measure and bars: tests/kernel_ref.py / tests/adam_ref.py — the kernel may err 4x what the fp32
restatement of the update errs on the same inputs (floored at 1 unit).

Measured on an MI355X, kernel units p / m / v / vmax (fp32 restatement; bar = 4x it), per
group: 0 plain, 1 amsgrad + decoupled, 2 maximize (no vmax in groups 0 and 2):
  t=1      0: 4.10 / 2.93 / 3.09          (4.49 / 2.93 / 4.45)
           1: 4.59 / 2.47 / 2.37 / 2.17   (4.83 / 2.47 / 2.37 / 2.17)
           2: 3.88 / 2.99 / 3.48          (3.50 / 2.99 / 4.93)
  t=7      0: 4.10 / 3.19 / 2.95          (4.79 / 3.19 / 3.50)
           1: 3.60 / 2.44 / 2.24 / 2.24   (4.49 / 2.44 / 2.55 / 2.55)
           2: 4.35 / 3.05 / 3.38          (4.35 / 3.05 / 5.26)
  t=100000 0: 3.54 / 2.96 / 3.27          (4.33 / 2.96 / 4.29)
           1: 3.30 / 2.57 / 2.39 / 2.23   (4.09 / 2.57 / 2.39 / 2.36)
           2: 3.02 / 2.85 / 3.22          (3.05 / 2.85 / 4.38)
  gated, count 6 -> 7:
           0: 4.51 / 2.80 / 3.37          (4.68 / 2.80 / 3.37)
           1: 3.49 / 2.43 / 2.42 / 2.42   (4.01 / 2.47 / 2.42 / 2.42)
           2: 3.20 / 3.02 / 3.88          (3.25 / 3.02 / 4.90)
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import adam_ref as A
from tests import kernel_ref as R

pytestmark = pytest.mark.gpu

dev = "cuda"
SMALL = [1, 3, 4, 5, 65536 + 7]      # 65543: two vector sweeps of 64 x 256 quads plus a tail
STRIDED = 2 * 16384 + 5              # scalar loop: two grid-strides of 64 x 256 threads + 5
PAD = 8                              # guard floats on both sides of every view
KINDS = ("p", "g", "m", "v", "x")    # x = max_exp_avg_sq
STEPS = [1, 7, 100000]
# lr, beta1, beta2, eps, weight_decay, flags
GROUPS = [(1e-3, 0.9, 0.999, 1e-8, 1e-5, 0),
          (3e-4, 0.8, 0.99, 1e-6, 1e-2, A.AMSGRAD | A.DECOUPLED),
          (5e-3, 0.95, 0.9999, 1e-3, 1e-3, A.MAXIMIZE)]
ERR_ARG = -1


def _entries(groups=3):
    """[(numel, shifted kind or None, group)]: the groups interleaved over the rows; a row that
    shifts max_exp_avg_sq belongs to the amsgrad group (the others pass no such pointer)."""
    ent = [(n, None) for n in SMALL] + [(n, k) for k in KINDS for n in SMALL] + [(STRIDED, "all")]
    if groups == 1:
        return [(n, sh, 0) for n, sh in ent]
    return [(n, sh, 1 if sh in ("x", "all") else e % groups) for e, (n, sh) in enumerate(ent)]


class Arena:
    """Every entry's p, g, m, v, x as views into one flat buffer per kind.  Entry e's view of
    kind k starts 16-byte aligned, or one float later when the entry shifts k (or "all")."""

    def __init__(self, entries, seed, groups=GROUPS):
        rng = np.random.default_rng(seed)
        self.entries, self.groups = entries, groups
        self.start = {k: [] for k in KINDS}
        off = 0
        for n, sh, _ in entries:
            for k in KINDS:
                self.start[k].append(off + PAD + (1 if sh in (k, "all") else 0))
            off += PAD + 4 + (n + 3) // 4 * 4 + PAD   # a multiple of 4: aligned starts
        self.total = off
        self.host = {k: rng.standard_normal(off).astype(np.float32) for k in KINDS}   # guards too
        for e, (n, _, gi) in enumerate(entries):
            sl = {k: slice(self.start[k][e], self.start[k][e] + n) for k in KINDS}
            g = (rng.standard_normal(n) * np.logspace(-6, 2, n)).astype(np.float32)
            v = (rng.random(n) * np.logspace(-12, 2, n)).astype(np.float32)
            self.host["g"][sl["g"]], self.host["v"][sl["v"]] = g, v
            self.host["m"][sl["m"]] = (0.1 * rng.standard_normal(n)).astype(np.float32)
            if self.ams(e):
                # half / twice the float64 second moment after this step, alternating: the
                # maximum keeps the old value on odd elements and takes the new one on even ones
                k = A.consts(*groups[gi][:5], 1, groups[gi][5])
                p = self.host["p"][sl["p"]]
                v1 = A.adam64(p, g, self.host["m"][sl["m"]], v, v, k)[2][0]
                self.host["x"][sl["x"]] = (v1 * np.where(np.arange(n) % 2, 2.0, 0.5)).astype(np.float32)
        self.dev = {k: torch.tensor(self.host[k], device=dev) for k in KINDS}
        for k in KINDS:
            assert self.dev[k].data_ptr() % 16 == 0

    def ams(self, e):
        return bool(self.groups[self.entries[e][2]][5] & A.AMSGRAD)

    def view(self, arr, k, e):
        return arr[self.start[k][e]:self.start[k][e] + self.entries[e][0]]

    def table(self):
        rows = np.zeros((len(self.entries), 7), dtype=np.int64)
        for e, (n, sh, gi) in enumerate(self.entries):
            for j, k in enumerate(KINDS):
                rows[e, j] = self.dev[k].data_ptr() + 4 * self.start[k][e]
                assert (rows[e, j] % 16 != 0) == (sh in (k, "all"))
            if not self.ams(e):
                rows[e, 4] = 0
            rows[e, 5], rows[e, 6] = n, gi
        return torch.tensor(rows, device=dev)

    def table4(self):
        """The same rows for mauv_adam_step (MauvAdamEntry: p, g, m, v, numel)."""
        rows = self.table().cpu().numpy()
        return torch.tensor(np.ascontiguousarray(rows[:, [0, 1, 2, 3, 5]]), device=dev)

    def group_array(self):
        from mauv._lib import MauvAdamGroup
        arr = (MauvAdamGroup * len(self.groups))()
        for a, (lr, b1, b2, eps, wd, flags) in zip(arr, self.groups):
            a.lr, a.beta1, a.beta2, a.eps, a.weight_decay, a.flags = lr, b1, b2, eps, wd, flags
        return arr

    def step(self, t, gate=None, n_groups=None):
        from mauv import ops
        from mauv._lib import lib
        tab, arr = self.table(), self.group_array()
        return lib.mauv_adam_step_ex(tab.data_ptr(), len(self.entries), ctypes.addressof(arr),
                                     len(self.groups) if n_groups is None else n_groups, t,
                                     None if gate is None else gate.data_ptr(), ops.stream())

    def result(self):
        torch.cuda.synchronize()
        return {k: self.dev[k].cpu().numpy() for k in KINDS}

    def outside_unchanged(self, got):
        """Every float outside the views, and every max_exp_avg_sq float of a row without amsgrad."""
        for k in KINDS:
            out = np.ones(self.total, dtype=bool)
            for e, (n, _, _) in enumerate(self.entries):
                if k != "x" or self.ams(e):
                    out[self.start[k][e]:self.start[k][e] + n] = False
            assert np.array_equal(got[k][out].view(np.int32), self.host[k][out].view(np.int32)), \
                f"a float outside the views of {k} changed"

    def unchanged(self, got, kinds):
        for k in kinds:
            assert np.array_equal(got[k].view(np.int32), self.host[k].view(np.int32)), k

    def grads_zeroed(self, got):
        for e in range(len(self.entries)):
            assert not self.view(got["g"], "g", e).view(np.int32).any(), "gradient not zeroed"


def _check_update(ar, got, t):
    """p, m, v, x of every entry against float64 with its group's constants at step t: returns
    fig[group] = [[kernel units], [restated units]] for p, m, v, x."""
    fig = np.zeros((len(ar.groups), 2, 4))
    for e, (n, _, gi) in enumerate(ar.entries):
        k = A.consts(*ar.groups[gi][:5], t, ar.groups[gi][5])
        p, g, m, v, x = (ar.view(ar.host[kk], kk, e) for kk in KINDS)
        ref, r32 = A.adam64(p, g, m, v, x, k), A.adam32(p, g, m, v, x, k)
        if ar.ams(e) and n >= 8:   # the maximum is exercised both ways
            kept = x.astype(np.float64) > ref[2][0]
            assert kept.any() and not kept.all(), (e, n)
        for j, kk in enumerate(KINDS[:1] + KINDS[2:]):
            if ref[j] is None:
                continue
            fig[gi, 0, j] = max(fig[gi, 0, j], R.units(ar.view(got[kk], kk, e), *ref[j]))
            fig[gi, 1, j] = max(fig[gi, 1, j], R.units(r32[j], *ref[j]))
    return fig


def _assert_bars(fig, what):
    for gi in range(fig.shape[0]):
        print(f"adam_ex {what} group {gi}: kernel p {fig[gi, 0, 0]:.2f} m {fig[gi, 0, 1]:.2f} "
              f"v {fig[gi, 0, 2]:.2f} vmax {fig[gi, 0, 3]:.2f} units; fp32 restatement "
              f"p {fig[gi, 1, 0]:.2f} m {fig[gi, 1, 1]:.2f} v {fig[gi, 1, 2]:.2f} "
              f"vmax {fig[gi, 1, 3]:.2f}")
    for gi in range(fig.shape[0]):
        for j, name in enumerate(("p", "m", "v", "vmax")):
            assert fig[gi, 0, j] <= R.bar(fig[gi, 1, j]), (gi, name, fig[gi, :, j])


@pytest.mark.parametrize("t", STEPS)
def test_adam_step_ex_three_groups_one_launch(t):
    ar = Arena(_entries(), seed=t)
    assert {gi for _, _, gi in ar.entries} == {0, 1, 2}
    assert ar.step(t) == 0
    got = ar.result()
    ar.outside_unchanged(got)
    ar.unchanged(got, ("g",))   # the ungated step keeps the gradients
    _assert_bars(_check_update(ar, got, t), f"t={t}")


@pytest.mark.parametrize("t", STEPS)
def test_one_plain_group_equals_adam_step_bitwise(t):
    """One group, no option, no max_exp_avg_sq pointer: p, m, v equal mauv_adam_step's on a copy
    of the same table, bit for bit."""
    from mauv import ops
    from mauv._lib import lib, check
    ent = _entries(groups=1)
    new, old = Arena(ent, seed=20 + t, groups=GROUPS[:1]), Arena(ent, seed=20 + t, groups=GROUPS[:1])
    for k in KINDS:
        assert np.array_equal(new.host[k].view(np.int32), old.host[k].view(np.int32))
    assert new.step(t) == 0
    lr, b1, b2, eps, wd, _ = GROUPS[0]
    tab = old.table4()
    check(lib.mauv_adam_step(tab.data_ptr(), len(ent), lr, b1, b2, eps, wd, t, ops.stream()),
          "adam_step")
    a, b = new.result(), old.result()
    for k in KINDS:
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), k
    new.unchanged(a, ("g", "x"))
    assert not np.array_equal(a["p"].view(np.int32), new.host["p"].view(np.int32))


def _gate(ok_loss, nonfinite, step):
    from mauv.optim import GATE_WORDS, G_OK_LOSS, G_NONFINITE, G_STEP
    g = torch.zeros(GATE_WORDS, dtype=torch.int32)
    g[G_OK_LOSS], g[G_NONFINITE], g[G_STEP] = ok_loss, nonfinite, step
    return g.to(dev)


def test_adam_step_ex_gated_modes():
    """ok_loss = 1 on a clean gate: mode 3, the count t + 1 once for all groups, every group's
    rows updated with its own constants, every gradient zeroed.  ok_loss = 0: mode 2, only the
    gradients go.  Non-finite gradients: mode 0, nothing changes, the gate is poisoned."""
    from mauv.optim import G_MODE, G_STEP, G_STEPPED, G_SKIP_LOSS, G_SKIP_GRAD, G_POISONED, \
        G_NONFINITE
    t = 7
    ar = Arena(_entries(), seed=11)
    gate = _gate(1, 0, t - 1)
    assert ar.step(0, gate) == 0
    got, gw = ar.result(), gate.cpu().tolist()
    assert (gw[G_MODE], gw[G_STEP], gw[G_STEPPED], gw[G_POISONED]) == (3, t, 1, 0)
    ar.outside_unchanged(got)
    _assert_bars(_check_update(ar, got, t), f"gated t={t}")
    ar.grads_zeroed(got)

    ar = Arena(_entries(), seed=12)
    gate = _gate(0, 0, t - 1)
    assert ar.step(0, gate) == 0
    got, gw = ar.result(), gate.cpu().tolist()
    assert (gw[G_MODE], gw[G_STEP], gw[G_STEPPED], gw[G_SKIP_LOSS]) == (2, t - 1, 0, 1)
    ar.outside_unchanged(got)
    ar.unchanged(got, ("p", "m", "v", "x"))
    ar.grads_zeroed(got)

    ar = Arena(_entries(), seed=13)
    gate = _gate(1, 1, t - 1)
    assert ar.step(0, gate) == 0
    got, gw = ar.result(), gate.cpu().tolist()
    assert (gw[G_MODE], gw[G_STEP], gw[G_STEPPED], gw[G_SKIP_GRAD]) == (0, t - 1, 0, 1)
    assert gw[G_POISONED] == 1 and gw[G_NONFINITE] == 0
    ar.unchanged(got, KINDS)


def test_adam_step_ex_argument_errors_launch_nothing():
    from mauv import ops
    from mauv._lib import lib
    ar = Arena(_entries()[:6], seed=14)
    assert ar.step(1, n_groups=0) == ERR_ARG
    assert b"adam_step_ex" in lib.mauv_last_error()
    assert ar.step(1, n_groups=9) == ERR_ARG
    assert ar.step(0) == ERR_ARG            # an ungated step count below 1
    tab, arr = ar.table(), ar.group_array()
    for n in (0, 65536):
        assert lib.mauv_adam_step_ex(tab.data_ptr(), n, ctypes.addressof(arr), 3, 1, None,
                                     ops.stream()) == ERR_ARG
    ar.unchanged(ar.result(), KINDS)
