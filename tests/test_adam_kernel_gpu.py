"""mauv_adam_step / mauv_adam_step_gated (csrc/adam.hip) on a hand-built table against the
float64 update from the same fp32 p, g, m, v and the same fp32 constants: the 16-byte vector
path (every pointer aligned) and the scalar loop an entry takes when any one of its four
pointers is not — views one float into a buffer, as a parameter that is a view may be — in one
launch, with the floats around every view checked bit-unchanged.

Measure and bars: tests/kernel_ref.py — units of 2^-24 of |m| + (1 - b1)(|g'| + |m|) for m, of
|v'| for v and of |p| + |update| for p; the kernel may err 4x what the fp32 restatement of the
update errs on the same inputs (floored at 1 unit).

Measured on an MI355X, (t, wd, eps): kernel units p / m / v (fp32 restatement; bar = 4x it):
  (1, 0, 1e-8)         4.45 / 2.48 / 2.51   (4.41 / 2.49 / 2.51; 17.6 / 10.0 / 10.0)
  (7, 1e-5, 1e-8)      4.30 / 3.10 / 3.54   (5.48 / 3.21 / 3.52; 21.9 / 12.8 / 14.1)
  (100000, 1e-2, 1e-3) 3.31 / 3.05 / 4.53   (4.64 / 5.48 / 5.85; 18.6 / 21.9 / 23.4)
"""
import numpy as np
import pytest
import torch

from tests import kernel_ref as R

pytestmark = pytest.mark.gpu

dev = "cuda"
LR, B1, B2 = 1e-3, 0.9, 0.999
CASES = [(1, 0.0, 1e-8), (7, 1e-5, 1e-8), (100000, 1e-2, 1e-3)]
SMALL = [1, 3, 4, 5, 65536 + 7]      # 65543: two vector sweeps of 64 x 256 quads plus a tail
STRIDED = 2 * 16384 + 5              # scalar loop: two grid-strides of 64 x 256 threads + 5
PAD = 8                              # guard floats on both sides of every view
KINDS = ("p", "g", "m", "v")


class Arena:
    """Every entry's p, g, m, v as views into one flat buffer per kind.  Entry e's view of
    kind k starts 16-byte aligned, or one float later when the entry shifts k (or "all")."""

    def __init__(self, entries, seed):
        rng = np.random.default_rng(seed)
        self.entries = entries                      # [(numel, shifted kind or None)]
        self.start = {k: [] for k in KINDS}
        off = 0
        for n, sh in entries:
            for k in KINDS:
                self.start[k].append(off + PAD + (1 if sh in (k, "all") else 0))
            off += PAD + 4 + (n + 3) // 4 * 4 + PAD   # a multiple of 4: aligned starts
        self.total = off
        self.host = {k: rng.standard_normal(off).astype(np.float32) for k in KINDS}   # guards too
        for e, (n, _) in enumerate(entries):
            sl = {k: slice(self.start[k][e], self.start[k][e] + n) for k in KINDS}
            self.host["g"][sl["g"]] = (rng.standard_normal(n) * np.logspace(-6, 2, n)).astype(np.float32)
            self.host["v"][sl["v"]] = (rng.random(n) * np.logspace(-12, 2, n)).astype(np.float32)
            self.host["m"][sl["m"]] = (0.1 * rng.standard_normal(n)).astype(np.float32)
        self.dev = {k: torch.tensor(self.host[k], device=dev) for k in KINDS}
        for k in KINDS:
            assert self.dev[k].data_ptr() % 16 == 0

    def view(self, arr, k, e):
        return arr[self.start[k][e]:self.start[k][e] + self.entries[e][0]]

    def table(self):
        rows = np.zeros((len(self.entries), 5), dtype=np.int64)
        for e, (n, sh) in enumerate(self.entries):
            for j, k in enumerate(KINDS):
                rows[e, j] = self.dev[k].data_ptr() + 4 * self.start[k][e]
                assert (rows[e, j] % 16 != 0) == (sh in (k, "all"))
            rows[e, 4] = n
        return torch.tensor(rows, device=dev)

    def result(self):
        return {k: self.dev[k].cpu().numpy() for k in KINDS}

    def outside_unchanged(self, got, kinds=KINDS):
        for k in kinds:
            out = np.ones(self.total, dtype=bool)
            for e, (n, _) in enumerate(self.entries):
                out[self.start[k][e]:self.start[k][e] + n] = False
            assert np.array_equal(got[k][out].view(np.int32), self.host[k][out].view(np.int32)), \
                f"a float outside the views of {k} changed"


def _check_update(ar, got, k, entries=None):
    """p, m, v of the listed entries against float64; returns [[kernel units], [restated]] for
    p, m, v."""
    fig = np.zeros((2, 3))
    for e in (range(len(ar.entries)) if entries is None else entries):
        p, g, m, v = (ar.view(ar.host[kk], kk, e) for kk in KINDS)
        ref, r32 = R.adam64(p, g, m, v, k), R.adam32(p, g, m, v, k)
        for j, kk in enumerate(("p", "m", "v")):
            u = R.units(ar.view(got[kk], kk, e), *ref[j])
            r = R.units(r32[j], *ref[j])
            fig[0, j], fig[1, j] = max(fig[0, j], u), max(fig[1, j], r)
    return fig


ENTRIES = ([(n, None) for n in SMALL] + [(n, k) for k in KINDS for n in SMALL] +
           [(STRIDED, "all")])


@pytest.mark.parametrize("t,wd,eps", CASES)
def test_adam_step_table(t, wd, eps):
    from mauv import ops
    from mauv._lib import lib, check
    ar = Arena(ENTRIES, seed=t)
    tab = ar.table()
    check(lib.mauv_adam_step(tab.data_ptr(), len(ENTRIES), LR, B1, B2, eps, wd, t,
                             ops.stream()), "adam_step")
    got = ar.result()
    ar.outside_unchanged(got)
    assert np.array_equal(got["g"].view(np.int32), ar.host["g"].view(np.int32)), "mode 1 keeps g"
    k = R.adam_consts(LR, B1, B2, eps, wd, t)
    fig = _check_update(ar, got, k)
    print(f"adam (t={t}, wd={wd}, eps={eps}): kernel p {fig[0, 0]:.2f} m {fig[0, 1]:.2f} "
          f"v {fig[0, 2]:.2f} units; fp32 restatement p {fig[1, 0]:.2f} m {fig[1, 1]:.2f} "
          f"v {fig[1, 2]:.2f}")
    for j, name in enumerate(("p", "m", "v")):
        assert fig[0, j] <= R.bar(fig[1, j]), (name, fig[:, j])


def _gate(**words):
    from mauv.optim import GATE_WORDS, G_OK_LOSS, G_NONFINITE, G_STEP
    g = torch.zeros(GATE_WORDS, dtype=torch.int32)
    g[G_OK_LOSS], g[G_NONFINITE], g[G_STEP] = words["ok_loss"], words["nonfinite"], words["step"]
    return g.to(dev)


def test_adam_step_gated_unaligned():
    """The gated form on unaligned entries (the scalar loop's `zero` modes): ok_loss = 1 on a
    clean gate steps at count step + 1 and zeroes the gradient after it (mode 3); ok_loss = 0
    zeroes the gradient only (mode 2)."""
    from mauv import ops
    from mauv._lib import lib, check
    from mauv.optim import G_MODE, G_STEP, G_STEPPED, G_SKIP_LOSS
    entries = [(5, "g"), (65536 + 7, "p"), (STRIDED, "all")]
    t, wd, eps = 7, 1e-5, 1e-8
    ar = Arena(entries, seed=11)
    gate, tab = _gate(ok_loss=1, nonfinite=0, step=t - 1), ar.table()
    check(lib.mauv_adam_step_gated(tab.data_ptr(), len(entries), LR, B1, B2, eps, wd,
                                   gate.data_ptr(), ops.stream()), "adam_step_gated")
    got, gw = ar.result(), gate.cpu().tolist()
    assert (gw[G_MODE], gw[G_STEP], gw[G_STEPPED]) == (3, t, 1)
    ar.outside_unchanged(got)
    fig = _check_update(ar, got, R.adam_consts(LR, B1, B2, eps, wd, t))
    for j, name in enumerate(("p", "m", "v")):
        assert fig[0, j] <= R.bar(fig[1, j]), (name, fig[:, j])
    for e in range(len(entries)):
        assert not ar.view(got["g"], "g", e).view(np.int32).any(), "gradient not zeroed"
    # a non-finite loss on a clean gate: only the gradient goes
    ar = Arena(entries, seed=12)
    gate, tab = _gate(ok_loss=0, nonfinite=0, step=t - 1), ar.table()
    check(lib.mauv_adam_step_gated(tab.data_ptr(), len(entries), LR, B1, B2, eps, wd,
                                   gate.data_ptr(), ops.stream()), "adam_step_gated")
    got, gw = ar.result(), gate.cpu().tolist()
    assert (gw[G_MODE], gw[G_STEP], gw[G_STEPPED], gw[G_SKIP_LOSS]) == (2, t - 1, 0, 1)
    ar.outside_unchanged(got)
    for kk in ("p", "m", "v"):
        assert np.array_equal(got[kk].view(np.int32), ar.host[kk].view(np.int32)), kk
    for e in range(len(entries)):
        assert not ar.view(got["g"], "g", e).view(np.int32).any(), "gradient not zeroed"
