"""csrc/gradnorm.hip (mauv_grad_norm, mauv_grad_clip) and the clip coefficient of the gated Adam
kernels (csrc/adam.hip), on hand-built tables against float64 NumPy.

Norm.  Reference: the float64 sum of squares of the fp32 inputs, sqrt, rounded once to fp32.
Bar: |norm - ref| <= 1 ulp(fp32).  Derived, not measured: the kernel squares and sums in double;
a double sum of n non-negative terms errs by at most n 2^-53 relative, below 1e-9 at these sizes
(n <= 5 2^20 + 3), and NumPy's pairwise float64 sum by less; the square root and the final
rounding to fp32 give half an fp32 ulp each.  The max-abs norm is exact.  1e20 and 1e-30 inputs
(fp32 squares overflow / underflow) show the double accumulation.  Two launches give the same bits
(fixed-order sum, no floating-point atomics).  A NaN / Inf anywhere makes the norm NaN and the
counter positive; the counter accumulates; nothing is written outside workspace and outputs.

Clip.  Every element equals fp32(g) * fp32(coef) bit for bit, coef restated in float64 from the
fp32 norm word by the library's formula min(1, max_norm / (norm + 1e-6)).

Gated Adam.  With max_norm in the gate the update equals tests/adam_ref.py's float64 step fed
fp32(g * coef), by adam_ref's bars (the kernel may err 4x the fp32 restatement, floored at one
unit), and is bit-identical to clipping in place first and stepping with clipping off."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import adam_ref as A
from tests import kernel_ref as R

pytestmark = pytest.mark.gpu

dev = "cuda"
F32 = np.float32
# one block; the block edges; several blocks; 2048 blocks (the cap) with 2.5 grid-strides
SIZES = [1, 3, 255, 256, 257, 1023, 2 ** 20 + 5, 5 * 2 ** 20 + 3]
TABLE = [1, 7, 0, 4096, 100003]
NANF = float("nan")


def _table(rows):
    return torch.tensor(rows, dtype=torch.int64, device=dev).reshape(-1, 2)


def _rows(t):
    return [(t.data_ptr(), t.numel())]


class Scan:
    """One mauv_grad_norm launch with NaN sentinels behind the workspace and around the norm
    and counter words."""

    def __init__(self, n_spans):
        from mauv import ops
        self.bytes = ops.grad_norm_workspace_bytes(n_spans)
        self.ws = torch.zeros(self.bytes + 64, dtype=torch.uint8, device=dev)
        self.ws[self.bytes:].view(torch.float32).fill_(NANF)
        self.out = torch.tensor([NANF, 0.0, NANF], device=dev)
        self.cnt = torch.tensor([-7, 0, -7], dtype=torch.int32, device=dev)

    def run(self, spans, kind):
        from mauv import ops
        ops.grad_norm(spans, kind, self.ws[:self.bytes], self.out[1:2], self.cnt[1:2])
        torch.cuda.synchronize()
        out, cnt = self.out.cpu().numpy(), self.cnt.cpu().numpy()
        assert np.isnan(out[0]) and np.isnan(out[2]), "a float beside the norm word changed"
        assert cnt[0] == -7 and cnt[2] == -7, "a word beside the counter changed"
        assert torch.isnan(self.ws[self.bytes:].view(torch.float32)).all(), \
            "a float behind the workspace changed"
        return out[1], int(cnt[1])


def _l2(x):
    """(ref rounded once to fp32, its ulp) of fp32 x."""
    x = x.astype(np.float64)
    ref = F32(np.sqrt(np.sum(x * x)))
    return ref, float(np.spacing(ref))


def _within_ulp(got, x):
    ref, ulp = _l2(x)
    print(f"norm {got!r} ref {ref!r} diff {abs(float(got) - float(ref)) / ulp:.2f} ulp")
    assert np.isfinite(got) and abs(float(got) - float(ref)) <= ulp, (got, ref)


@functools.lru_cache(maxsize=None)
def _data(n):
    """fp32 host values of n + 1 floats with magnitudes over eight decades, and their device
    copy (16-byte aligned); [0:n] is the aligned span, [1:n + 1] the one a float later."""
    rng = np.random.default_rng(n)
    h = (rng.standard_normal(n + 1) * 10.0 ** rng.uniform(-6, 2, n + 1)).astype(F32)
    d = torch.tensor(h, device=dev)
    assert d.data_ptr() % 16 == 0
    return h, d


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_l2_and_max_single_span(n, off):
    h, d = _data(n)
    x, t = h[off:off + n], d[off:off + n]
    assert (t.data_ptr() % 16 != 0) == bool(off)
    s = Scan(1)
    got, cnt = s.run(_table(_rows(t)), 0)
    assert cnt == 0
    _within_ulp(got, x)
    got, cnt = s.run(_table(_rows(t)), 1)
    assert cnt == 0 and got.view(np.int32) == np.abs(x).max().view(np.int32)


@pytest.mark.parametrize("value", [1e20, 1e-30])
def test_l2_range_needs_the_double_accumulation(value):
    x = np.full(4096, value, dtype=F32)
    assert not np.isfinite(x * x).all() or not (x * x).any()   # fp32 squares overflow / vanish
    t = torch.tensor(x, device=dev)          # (kept alive: the table only holds its address)
    got, cnt = Scan(1).run(_table(_rows(t)), 0)
    assert cnt == 0 and got > 0
    _within_ulp(got, x)


def _cut(sizes, seed):
    """Spans of ``sizes`` cut from one buffer, every start at an odd float offset:
    (host buffer, device buffer, [(start, n)])."""
    rng = np.random.default_rng(seed)
    cuts, off = [], 1
    for n in sizes:
        cuts.append((off, n))
        off += n + 2 + (n % 2)       # stays odd
    h = (rng.standard_normal(off + 8) * 10.0 ** rng.uniform(-4, 2, off + 8)).astype(F32)
    d = torch.tensor(h, device=dev)
    assert d.data_ptr() % 16 == 0 and all(o % 2 for o, _ in cuts)
    return h, d, cuts


def _cut_rows(d, cuts):
    return [(d.data_ptr() + 4 * o, n) for o, n in cuts]


def test_table_equals_the_concatenation():
    h, d, cuts = _cut(TABLE, 1)
    cat = np.concatenate([h[o:o + n] for o, n in cuts])
    ref, ulp = _l2(cat)
    tab = _table(_cut_rows(d, cuts))
    s = Scan(len(cuts))
    got, cnt = s.run(tab, 0)
    assert cnt == 0
    _within_ulp(got, cat)
    cat_dev = torch.tensor(cat, device=dev)
    one, _ = Scan(1).run(_table(_rows(cat_dev)), 0)
    assert abs(float(got) - float(one)) <= ulp
    again, _ = s.run(tab, 0)
    assert again.view(np.int32) == got.view(np.int32)
    mx, _ = s.run(tab, 1)
    assert mx.view(np.int32) == np.abs(cat).max().view(np.int32)


def test_two_runs_give_identical_bits():
    n = 2 ** 20 + 5
    _, d = _data(n)
    a, _ = Scan(1).run(_table(_rows(d[:n])), 0)
    b, _ = Scan(1).run(_table(_rows(d[:n])), 0)    # a fresh workspace too
    assert a.view(np.int32) == b.view(np.int32)


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("value", [NANF, float("inf")])
def test_nonfinite_makes_the_norm_nan_and_the_counter_positive(value, where, off):
    n = 2 ** 16 + 7                         # 65 blocks of quads, a head and a tail
    h, _ = _data(n)
    x = h[off:off + n].copy()
    clean = torch.tensor(h, device=dev)[off:off + n]
    bad = torch.tensor(h, device=dev)
    pos = {"first": 0, "middle": n // 2 + 1, "last": n - 1}[where]
    bad[off + pos] = value
    bad = bad[off:off + n]
    for kind in (0, 1):
        s = Scan(1)
        got, cnt = s.run(_table(_rows(bad)), kind)
        assert np.isnan(got) and cnt > 0
        # a clean launch on the same counter: it adds, it does not reset; the norm is this
        # launch's own
        got, cnt2 = s.run(_table(_rows(clean)), kind)
        assert cnt2 == cnt > 0
        if kind == 0:
            _within_ulp(got, x)
        else:
            assert got == np.abs(x).max()
        got, cnt3 = s.run(_table(_rows(bad)), kind)
        assert np.isnan(got) and cnt3 > cnt


def test_nonfinite_in_a_table_row():
    h, d, cuts = _cut(TABLE, 2)
    d[cuts[1][0] + 3] = float("-inf")
    got, cnt = Scan(len(cuts)).run(_table(_cut_rows(d, cuts)), 0)
    assert np.isnan(got) and cnt > 0


# ------------------------------------------------------------------------------------ clip
def _coef(max_norm, norm):
    """The library's coefficient, restated in float64 from the fp32 words."""
    return F32(min(1.0, float(F32(max_norm)) / (float(F32(norm)) + 1e-6)))


def _clip(rows, max_norm, kind=0):
    """Scan, then clip in place: the fp32 norm word."""
    from mauv import ops
    s = Scan(len(rows))
    tab = _table(rows)
    norm, _ = s.run(tab, kind)
    ops.grad_clip(tab, s.out[1:2], float(max_norm))
    torch.cuda.synchronize()
    return norm


@pytest.mark.parametrize("kind", [0, 1])
def test_clip_scales_every_element_bitwise(kind):
    h, d, cuts = _cut(TABLE, 3)
    pre = _clip(_cut_rows(d, cuts), 1e30, kind)       # no clip: reads the norm
    assert np.array_equal(d.cpu().numpy().view(np.int32), h.view(np.int32))
    c = float(pre) / 2
    norm = _clip(_cut_rows(d, cuts), c, kind)
    coef = _coef(c, norm)
    assert norm == pre and 0.49 < coef < 0.51
    want = h.copy()
    for o, n in cuts:
        want[o:o + n] = h[o:o + n] * coef
    assert want.dtype == np.float32
    assert np.array_equal(d.cpu().numpy().view(np.int32), want.view(np.int32))   # guards too
    # the single aligned span, 2048 blocks and more than one sweep
    n = 5 * 2 ** 20 + 3
    h1, _ = _data(n)
    d1 = torch.tensor(h1, device=dev)
    norm = _clip(_rows(d1[:n]), 0.125, kind)
    want = h1.copy()
    want[:n] = h1[:n] * _coef(0.125, norm)
    assert np.array_equal(d1.cpu().numpy().view(np.int32), want.view(np.int32))


def test_clip_leaves_small_gradients_alone_and_follows_the_formula_near_the_edge():
    h, d, cuts = _cut(TABLE, 4)
    norm = _clip(_cut_rows(d, cuts), 1e30)
    _clip(_cut_rows(d, cuts), float(norm) * 2)
    _clip(_cut_rows(d, cuts), float(norm) * 1.001)
    assert np.array_equal(d.cpu().numpy().view(np.int32), h.view(np.int32))
    # norm < max_norm, but within the 1e-6 of it: the formula gives a coefficient below 1
    x = np.zeros(1027, dtype=F32)
    x[5], x[700] = 0.6, 0.8
    t = torch.tensor(np.concatenate([[F32(9)], x]), device=dev)[1:]
    c = np.nextafter(F32(1.0), F32(2.0))
    norm = _clip(_rows(t), float(c))
    coef = _coef(c, norm)
    assert norm < c and coef < 1
    assert np.array_equal(t.cpu().numpy().view(np.int32), (x * coef).view(np.int32))


# ------------------------------------------------------------------- gated Adam with clipping
NUMEL = [5, 1024, 4099]
SHIFTED = 1                     # this row's five views start one float after a 16-byte boundary
PAD = 8
KINDS = ("p", "g", "m", "v", "x")
PLAIN = [(1e-3, 0.9, 0.999, 1e-8, 1e-5, 0)]
TWO = [(1e-3, 0.9, 0.999, 1e-8, 1e-5, 0), (3e-4, 0.8, 0.99, 1e-6, 1e-2, A.AMSGRAD | A.DECOUPLED)]
T = 7


class Rows:
    """p, g, m, v, x of three rows as views into one flat buffer per kind, with guard floats."""

    def __init__(self, groups, row_group, seed=5):
        rng = np.random.default_rng(seed)
        self.groups, self.row_group = groups, row_group
        self.start, off = [], 0
        for e, n in enumerate(NUMEL):
            self.start.append(off + PAD + (1 if e == SHIFTED else 0))
            off += PAD + 4 + (n + 3) // 4 * 4 + PAD
        self.total = off
        self.host = {k: rng.standard_normal(off).astype(F32) for k in KINDS}
        self.host["v"] = np.abs(self.host["v"]) * F32(1e-2)
        self.host["x"] = np.abs(self.host["x"]) * F32(1e-2)
        self.host["m"] *= F32(0.1)
        self.dev = {k: torch.tensor(self.host[k], device=dev) for k in KINDS}

    def sl(self, e):
        return slice(self.start[e], self.start[e] + NUMEL[e])

    def ams(self, e):
        return bool(self.groups[self.row_group[e]][5] & A.AMSGRAD)

    def ptr(self, k, e):
        p = self.dev[k].data_ptr() + 4 * self.start[e]
        assert (p % 16 != 0) == (e == SHIFTED)
        return p

    def spans(self):
        return [(self.ptr("g", e), NUMEL[e]) for e in range(len(NUMEL))]

    def step(self, gate, simple):
        """mauv_adam_step_gated (one plain group) or mauv_adam_step_ex, gated."""
        from mauv import ops
        from mauv._lib import lib, check, MauvAdamGroup
        if simple:
            rows = [[self.ptr(k, e) for k in KINDS[:4]] + [NUMEL[e]] for e in range(len(NUMEL))]
            tab = torch.tensor(rows, dtype=torch.int64, device=dev)
            lr, b1, b2, eps, wd, _ = self.groups[0]
            check(lib.mauv_adam_step_gated(tab.data_ptr(), len(rows), lr, b1, b2, eps, wd,
                                           gate.data_ptr(), ops.stream()), "adam_step_gated")
        else:
            rows = [[self.ptr(k, e) for k in KINDS[:4]] +
                    [self.ptr("x", e) if self.ams(e) else 0, NUMEL[e], self.row_group[e]]
                    for e in range(len(NUMEL))]
            tab = torch.tensor(rows, dtype=torch.int64, device=dev)
            arr = (MauvAdamGroup * len(self.groups))()
            for a, (lr, b1, b2, eps, wd, flags) in zip(arr, self.groups):
                a.lr, a.beta1, a.beta2, a.eps, a.weight_decay, a.flags = lr, b1, b2, eps, wd, flags
            check(lib.mauv_adam_step_ex(tab.data_ptr(), len(rows), ctypes.addressof(arr),
                                        len(self.groups), 0, gate.data_ptr(), ops.stream()),
                  "adam_step_ex")
        torch.cuda.synchronize()
        return {k: self.dev[k].cpu().numpy() for k in KINDS}

    def scan(self, gate):
        """The fused scan into the gate's grad_norm and nonfinite words."""
        from mauv import ops
        from mauv.optim import G_GRAD_NORM, G_NONFINITE
        ws = torch.empty(ops.grad_norm_workspace_bytes(len(NUMEL)), dtype=torch.uint8, device=dev)
        ops.grad_norm(_table(self.spans()), 0, ws,
                      gate[G_GRAD_NORM:G_GRAD_NORM + 1].view(torch.float32),
                      gate[G_NONFINITE:G_NONFINITE + 1])

    def grad_norm64(self):
        return _l2(np.concatenate([self.host["g"][self.sl(e)] for e in range(len(NUMEL))]))


def _gate(max_norm, ok_loss=1, step=T - 1):
    from mauv.optim import GATE_WORDS, G_OK_LOSS, G_STEP, G_MAX_NORM
    g = np.zeros(GATE_WORDS, dtype=np.int32)
    g[G_OK_LOSS], g[G_STEP] = ok_loss, step
    g.view(F32)[G_MAX_NORM] = max_norm
    return torch.tensor(g, device=dev)


def _words(gate):
    w = gate.cpu().numpy()
    return w, w.view(F32)


CONFIGS = [("gated", PLAIN, [0, 0, 0], True), ("ex-plain", PLAIN, [0, 0, 0], False),
           ("ex-two", TWO, [0, 1, 1], False)]


@pytest.mark.parametrize("name,groups,row_group,simple", CONFIGS)
def test_gated_adam_clips_as_it_loads(name, groups, row_group, simple):
    from mauv import ops
    from mauv.optim import G_MODE, G_STEP, G_STEPPED, G_NONFINITE, G_GRAD_NORM, G_CLIP_COEF
    ar = Rows(groups, row_group)
    ref, ulp = ar.grad_norm64()
    c = float(ref) / 2
    gate = _gate(c)
    ar.scan(gate)
    got = ar.step(gate, simple)
    wi, wf = _words(gate)
    assert (wi[G_MODE], wi[G_STEP], wi[G_STEPPED], wi[G_NONFINITE]) == (3, T, 1, 0)
    assert abs(float(wf[G_GRAD_NORM]) - float(ref)) <= ulp
    coef = _coef(c, wf[G_GRAD_NORM])
    assert wf[G_CLIP_COEF].view(np.int32) == coef.view(np.int32) and 0.49 < coef < 0.51
    fig = np.zeros((2, 4))
    for e in range(len(NUMEL)):
        gi = row_group[e]
        k = A.consts(*groups[gi][:5], T, groups[gi][5])
        p, g, m, v, x = (ar.host[kk][ar.sl(e)] for kk in KINDS)
        gc = g * coef
        assert gc.dtype == np.float32
        r64, r32 = A.adam64(p, gc, m, v, x, k), A.adam32(p, gc, m, v, x, k)
        for j, kk in enumerate(("p", "m", "v", "x")):
            if r64[j] is None:
                assert np.array_equal(got["x"][ar.sl(e)].view(np.int32), x.view(np.int32))
                continue
            fig[0, j] = max(fig[0, j], R.units(got[kk][ar.sl(e)], *r64[j]))
            fig[1, j] = max(fig[1, j], R.units(r32[j], *r64[j]))
        assert not got["g"][ar.sl(e)].view(np.int32).any(), "gradient not zeroed (mode 3)"
    print(f"{name}: kernel p/m/v/vmax {fig[0]} units, fp32 restatement {fig[1]}")
    for j in range(4):
        assert fig[0, j] <= R.bar(fig[1, j]), (name, j, fig[:, j])
    for k in KINDS:                                    # the guard floats
        out = np.ones(ar.total, dtype=bool)
        for e in range(len(NUMEL)):
            out[ar.sl(e)] = False
        assert np.array_equal(got[k][out].view(np.int32), ar.host[k][out].view(np.int32)), k
    # the same bits as clipping in place and then stepping with clipping off
    two = Rows(groups, row_group)
    norm = torch.tensor([wf[G_GRAD_NORM]], device=dev)
    ops.grad_clip(_table(two.spans()), norm, c)
    g2 = _gate(0.0)
    alt = two.step(g2, simple)
    assert _words(g2)[1][G_CLIP_COEF] == 1.0
    for k in KINDS:
        assert np.array_equal(alt[k].view(np.int32), got[k].view(np.int32)), k


@pytest.mark.parametrize("name,groups,row_group,simple", CONFIGS)
def test_inactive_clip_is_bit_identical_to_off(name, groups, row_group, simple):
    from mauv.optim import G_CLIP_COEF
    on, off = Rows(groups, row_group), Rows(groups, row_group)
    ref, _ = on.grad_norm64()
    gate_on, gate_off = _gate(float(ref) * 2), _gate(0.0)
    on.scan(gate_on)
    off.scan(gate_off)
    a, b = on.step(gate_on, simple), off.step(gate_off, simple)
    assert _words(gate_on)[1][G_CLIP_COEF] == 1.0 and _words(gate_off)[1][G_CLIP_COEF] == 1.0
    for k in KINDS:
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), k
    assert not np.array_equal(a["p"].view(np.int32), on.host["p"].view(np.int32))


@pytest.mark.parametrize("name,groups,row_group,simple", CONFIGS)
def test_skip_rules_are_untouched(name, groups, row_group, simple):
    from mauv.optim import G_MODE, G_STEP, G_STEPPED, G_SKIP_LOSS, G_SKIP_GRAD, G_POISONED, \
        G_NONFINITE, G_GRAD_NORM
    ar = Rows(groups, row_group)
    ar.dev["g"][ar.start[2] + 17] = NANF
    before = {k: ar.dev[k].cpu().numpy() for k in KINDS}
    gate = _gate(0.5)
    ar.scan(gate)
    assert int(gate[G_NONFINITE]) > 0
    got = ar.step(gate, simple)
    wi, wf = _words(gate)
    assert (wi[G_MODE], wi[G_STEP], wi[G_STEPPED], wi[G_SKIP_GRAD]) == (0, T - 1, 0, 1)
    assert wi[G_POISONED] == 1 and wi[G_NONFINITE] == 0 and np.isnan(wf[G_GRAD_NORM])
    for k in KINDS:                                    # no tensor changes, the arena is kept
        assert np.array_equal(got[k].view(np.int32), before[k].view(np.int32)), k
    ar = Rows(groups, row_group)
    gate = _gate(0.5, ok_loss=0)
    ar.scan(gate)
    got = ar.step(gate, simple)
    wi, _ = _words(gate)
    assert (wi[G_MODE], wi[G_STEP], wi[G_STEPPED], wi[G_SKIP_LOSS]) == (2, T - 1, 0, 1)
    for k in ("p", "m", "v", "x"):
        assert np.array_equal(got[k].view(np.int32), ar.host[k].view(np.int32)), k
    for e in range(len(NUMEL)):
        assert not got["g"][ar.sl(e)].view(np.int32).any()
