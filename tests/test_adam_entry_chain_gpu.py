"""The gated all-groups Adam entries as one chain, and the bound on cached device tables.

(a) mauv_adam_step_ex_ema, _accum, _scaled and the gated mauv_adam_step_ex each take one optional
state pointer more than the one before; with that pointer NULL an entry IS the one before
(include/mauv.h).  One table — 5 elements at a view one float past 16-byte alignment, 8, 1027 and
70001 elements (the grid-stride loops take a second trip) — option flags 0 and 7, one and two
groups, and the three decisions (step, bad loss, non-finite gradient): every entry that can
express a call leaves identical bits in p, m, v, max_exp_avg_sq, g, all 16 gate words and the
scaler's and the window's words.

(b) Parameters that do not share a step count step in one launch per distinct count.  The device
tables cached for those launches are bounded by the number of distinct counts: 25 steps cache
what 5 steps cached, and each parameter ends bit-equal to the same parameter stepped alone, by a
FusedAdam of its own, on the same gradients.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

dev = "cuda"
NUMELS = [5, 8, 1027, 70001]
KINDS = ("p", "g", "m", "v", "x")    # x = max_exp_avg_sq
# lr, beta1, beta2, eps, weight_decay
GROUPS = [(1e-3, 0.9, 0.999, 1e-8, 1e-2), (3e-4, 0.8, 0.99, 1e-6, 1e-5)]
GATES = {"step": (1, 0), "bad_loss": (0, 0), "nonfinite_grad": (1, 3)}   # ok_loss, nonfinite


class Problem:
    """The host image of one call's inputs; ``run`` uploads a fresh copy, makes the call and
    returns every byte it may have written."""

    def __init__(self, flags, n_groups, gate_state):
        rng = np.random.default_rng(20260)
        self.flags, self.n_groups = flags, n_groups
        self.start, off = [], 0
        for i, n in enumerate(NUMELS):
            self.start.append(off + (1 if i == 0 else 0))   # row 0: one float past alignment
            off += 4 + (n + 3) // 4 * 4
        self.host = {k: rng.standard_normal(off).astype(np.float32) for k in KINDS}
        self.host["g"] *= 1e-2
        self.host["v"] = np.abs(self.host["v"]) * 1e-4
        self.host["x"] = self.host["v"] * np.where(np.arange(off) % 2, 2.0, 0.5).astype(np.float32)
        ok_loss, nonfinite = GATES[gate_state]
        if nonfinite:
            self.host["g"][self.start[2] + np.array([0, 7, 1026])] = (np.inf, -np.inf, np.nan)
        from mauv.optim import (GATE_WORDS, G_OK_LOSS, G_NONFINITE, G_STEP, G_MAX_NORM,
                                G_GRAD_NORM)
        self.gate = np.zeros(GATE_WORDS, dtype=np.int32)
        self.gate[[G_OK_LOSS, G_NONFINITE, G_STEP]] = ok_loss, nonfinite, 6
        # clipping on: the scanned norm is 2.5 times max_norm (NaN beside non-finite gradients)
        self.gate.view(np.float32)[[G_MAX_NORM, G_GRAD_NORM]] = 1.0, np.nan if nonfinite else 2.5

    def run(self, entry, scaler=False, window=False):
        from mauv import ops
        from mauv._lib import lib, MauvAdamGroup
        buf = {k: torch.tensor(self.host[k], device=dev) for k in KINDS}
        rows = np.zeros((len(NUMELS), 7), dtype=np.int64)
        for i, n in enumerate(NUMELS):
            rows[i, :5] = [buf[k].data_ptr() + 4 * self.start[i] for k in KINDS]
            assert (rows[i, 0] % 16 != 0) == (i == 0)
            if not self.flags & 1:
                rows[i, 4] = 0
            rows[i, 5], rows[i, 6] = n, i % self.n_groups
        tab = torch.tensor(rows, device=dev)
        arr = (MauvAdamGroup * self.n_groups)()
        for a, (lr, b1, b2, eps, wd) in zip(arr, GROUPS):
            a.lr, a.beta1, a.beta2, a.eps, a.weight_decay, a.flags = lr, b1, b2, eps, wd, self.flags
        gate = torch.tensor(self.gate, device=dev)
        # a dynamic scaler one good step short of growing; a window of two earlier micro-batches
        ls = np.zeros(8, dtype=np.int32)
        ls.view(np.float32)[:4] = 1024.0, 0.0, 2.0, 0.5
        ls[4:6] = 3, 2
        ls, acc = torch.tensor(ls, device=dev), torch.tensor([2] + [0] * 7, dtype=torch.int32,
                                                             device=dev)
        head = (tab.data_ptr(), len(NUMELS), ctypes.addressof(arr), self.n_groups)
        g, s = gate.data_ptr(), ls.data_ptr() if scaler else None
        a, st = acc.data_ptr() if window else None, ops.stream()
        if entry == "ex":
            assert not scaler and not window
            rc = lib.mauv_adam_step_ex(*head, 0, g, st)
        elif entry == "scaled":
            assert not window
            rc = lib.mauv_adam_step_ex_scaled(*head, g, s, st)
        elif entry == "accum":
            rc = lib.mauv_adam_step_ex_accum(*head, g, s, a, st)
        else:
            rc = lib.mauv_adam_step_ex_ema(*head, g, s, a, None, None, st)
        assert rc == 0, lib.mauv_last_error()
        torch.cuda.synchronize()
        out = {k: buf[k].cpu().numpy().tobytes() for k in KINDS}
        out.update(gate=gate.cpu().numpy().tobytes(), scaler=ls.cpu().numpy().tobytes(),
                   window=acc.cpu().numpy().tobytes())
        return out


@pytest.mark.parametrize("gate_state", list(GATES))
@pytest.mark.parametrize("n_groups", [1, 2])
@pytest.mark.parametrize("flags", [0, 7])
def test_null_chain_is_bit_exact(flags, n_groups, gate_state):
    from mauv.optim import G_MODE
    pb = Problem(flags, n_groups, gate_state)
    chains = {(False, False): ("ema", "accum", "scaled", "ex"),
              (True, False): ("ema", "accum", "scaled"),
              (False, True): ("ema", "accum"),
              (True, True): ("ema", "accum")}
    for (scaler, window), entries in chains.items():
        outs = [pb.run(e, scaler, window) for e in entries]
        for e, out in zip(entries[1:], outs[1:]):
            for k in out:
                assert out[k] == outs[0][k], (scaler, window, e, k)
        # the call did what its gate state says (mode 3 step, 2 zero the gradients, 0 nothing)
        mode = np.frombuffer(outs[0]["gate"], dtype=np.int32)[G_MODE]
        want = {"step": 3, "bad_loss": 2, "nonfinite_grad": 2 if scaler else 0}[gate_state]
        assert mode == want, (scaler, window, mode)
        assert (outs[0]["p"] != pb.host["p"].tobytes()) == (mode == 3)


def _cached_tables(opt):
    plans = list(opt._fast.values()) + [p for ps in opt._split.values() for p in ps]
    return len({p.table.data_ptr() for p in plans})


@pytest.mark.parametrize("kw", [dict(), dict(amsgrad=True)], ids=["plain", "amsgrad"])
def test_split_step_counts_cache_a_bounded_number_of_tables(kw):
    from mauv.optim import FusedAdam
    rng = np.random.default_rng(7)
    init = [rng.standard_normal(n).astype(np.float32) for n in (5, 8)]
    grads = [[torch.tensor(rng.standard_normal(n).astype(np.float32), device=dev)
              for n in (5, 8)] for _ in range(25)]

    def drive(which, check=None):
        ps = [torch.tensor(init[i], device=dev, requires_grad=True) for i in which]
        opt = FusedAdam(ps, lr=1e-2, weight_decay=1e-3, **kw)
        for t in range(25):
            for p, i in zip(ps, which):
                p.grad = None if (i == 1 and t == 0) else grads[t][i].clone()
            opt.step()
            if check:
                check(opt, t)
        return [p.detach().cpu().numpy().tobytes() for p in ps], opt

    seen = {}
    got, opt = drive([0, 1], lambda o, t: seen.__setitem__(t, _cached_tables(o)))
    assert seen[4] == seen[24] == 2, seen     # one table per distinct step count, from step 2 on
    assert [int(opt.state[p]["step"]) for p in opt.param_groups[0]["params"]] == [25, 24]
    for i in (0, 1):
        assert got[i] == drive([i])[0][0], i
