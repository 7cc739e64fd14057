"""The free-running Philox stream — the path training, prediction and bench.py run — against an
independent float64 reference: the identity of every epsilon the production path uses, forward
and backward, at kernel and model level.

Every other parity test replaces the generator with explicit epsilons; here ``eps=None`` /
``eps_provider=None`` and the epsilons are restated on the CPU (oracle.philox_ref, Philox4x32-10
integer words bit-exact, Box-Muller in float64 on the kernel's fp32-rounded uniforms).  A wrong
quad, sample, layer or seed word in any kernel moves a sampled weight by ~sigma (0.05 at
rho = -3): about 1,000 times the comparison bars below.

Bars:
  normals      |gpu - ref| <= NORMAL_BAR * 2^-24 * max(|ref|, 2^-10): 4x the error measured once on
               an MI355X (NORMAL_MEASURED, the fp32 libm calls of normal4), see
               test_philox_raw_counter_edges
  kernels      ``close``: 1e-4 of the reference's max + 1e-5 (tests/test_kernels_gpu.py); 16-bit
               outputs 2 ulp of the format
  model level  the header of tests/test_model_gpu.py against the oracle; bit-equality between the
               free-running engine and the same engine fed ops.philox_raw's normals through the
               explicit-epsilon path (that path is pinned to the oracle by the parity suite)
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import bayes_ref, loops_ref
from oracle.philox_ref import philox4x32_10, eps_for_layer
from tests.golden.common import make_batches, SEED_DATA
from tests.helpers import (build_pair, oracle64, oracle_replay, philox_store, PhiloxRawProvider,
                           normal_err_units, NORMAL_BAR)
from tests.test_model_gpu import _assert_close, _assert_grads_as_accurate

pytestmark = pytest.mark.gpu

dev = "cuda"
SEED = 0x1234_5678_9ABC
ULP = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}   # as tests/test_centre16_gpu.py


def close(a, b, rtol=1e-4, atol=1e-5):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    err = (a - b).abs().max().item()
    lim = atol + rtol * b.abs().max().item()
    assert err <= lim, f"max err {err:.3e} > {lim:.3e}"


def _eps(numel, sample, layer, seed=SEED):
    return torch.from_numpy(eps_for_layer(numel, seed, sample, layer, u32=True))


# ------------------------------------------------------------------ 2. mauv_philox_raw
RAW_EDGES = [(SEED, 77, 6, 1 << 18)] + \
    [(SEED, s, 6, 4096) for s in (2 ** 32 - 1, 2 ** 32, 2 ** 40 + 3)] + \
    [(s, 77, 6, 4096) for s in (1, 2 ** 32, 2 ** 62 - 1)] + \
    [(SEED, 77, l, 4096) for l in (0, 1, 347)]


def test_philox_raw_counter_edges():
    """mauv_philox_raw at the counter edges: the sample's high word (counter word 3) set, both
    seed words, layer ids 0, 1 and 347 = 2*173 + 1 (the largest the model uses).  Integer words
    bit-exact; normals against the fp32-uniform restatement.

    Measured on an MI355X: max |gpu - ref| / max(|ref|, 2^-10) = 3.93 x 2^-24 (NORMAL_MEASURED:
    the fp32 logf / sqrtf / sincospif of normal4; 3.09 - 3.75 on the nine 4,096-quad edges, 3.93
    on the 2^18 quads); asserted: NORMAL_BAR = 4x that = 15.72 x 2^-24 (libm differences between
    ROCm releases).  At |eps| = 6 the bar is 5.6e-6 absolute, below the 1e-5 that separates the
    fp32-uniform from the float64-uniform restatement (the GPU normals are 1.4e-5 from the
    latter on the same quads): the test tells the two apart."""
    from mauv import ops
    worst = 0.0
    for seed, sample, layer, nq in RAW_EDGES:
        raw, nrm = ops.philox_raw(seed, sample, layer, nq)
        ref_raw = philox4x32_10(np.arange(nq, dtype=np.uint64), sample, layer, seed)
        assert np.array_equal(raw.cpu().numpy().view(np.uint32).reshape(-1, 4), ref_raw), \
            (seed, sample, layer)
        e = normal_err_units(nrm.cpu().numpy(), ref_raw)
        print(f"philox_raw seed={seed:#x} sample={sample:#x} layer={layer} nq={nq}: "
              f"normal err {e:.3f} x 2^-24")
        worst = max(worst, e)
    print(f"philox_raw normals: worst {worst:.3f} x 2^-24 (bar {NORMAL_BAR})")
    assert NORMAL_BAR * 2.0 ** -24 * 6 < 1e-5
    assert worst <= NORMAL_BAR, worst


# ------------------------------------------------------------------ 3. forward sampling
def _sample_ref(mu, rho, G, sample0, layer):
    """[G, *mu.shape] float64: mu + log1p(exp(rho)) * restated eps."""
    mu, rho = mu.double().cpu(), rho.double().cpu()
    eps = torch.stack([_eps(mu.numel(), sample0 + g, layer) for g in range(G)])
    return mu + torch.log1p(torch.exp(rho)) * eps.view(G, *mu.shape)


SAMPLE_CASES = [
    # Cout, Cin, R, cin_pad, dtype
    (16, 8, 3, None, torch.float32),        # block form
    (5, 1028, 1, None, torch.float32),      # ragged 1024 + 4 channel range
    (8, 3, 7, 4, torch.float32),            # padded fp32 stem, element kernel
    (8, 1, 7, 8, torch.bfloat16),           # 16-bit sonar stem
    (8, 147, 1, "kp", torch.float32),       # the stem as one GEMM
    (8, 147, 1, "kp", torch.float16),
    (7, 1, 1, None, torch.float32),         # a bias: the last quad is partial
]


@pytest.mark.parametrize("blk", [False, True], ids=["elem", "blk"])
@pytest.mark.parametrize("Cout,Cin,R,cin_pad,dt", SAMPLE_CASES)
def test_sample_matches_restated_eps(Cout, Cin, R, cin_pad, dt, blk):
    """reparam_sample / reparam_sample_ex with eps=None against float64 on restated epsilons:
    G = 3 samples from 2^32 - 2 (the batch crosses the sample's word boundary), both kernel
    forms, pad channels untouched; the device sample counter's values (not only that they
    differ)."""
    from mauv import ops
    torch.manual_seed(31)
    G, layer, s0 = 3, 6, 2 ** 32 - 2
    if cin_pad == "kp":
        cin_pad = ops.stem_kp(dt, Cin)
    cp = cin_pad or Cin
    mu = (0.1 * torch.randn(Cout, Cin, R, R)).to(dev)
    rho = (torch.randn(Cout, Cin, R, R) - 3).to(dev)
    rtol = 1e-4 if dt == torch.float32 else 2 * ULP[dt]
    base = torch.tensor([2 ** 32 - 7], dtype=torch.int64, device=dev)
    prev = ops.set_reparam_kernels(sample_blk=blk)
    try:
        out = torch.full((G, Cout, R, R, cp), 7.0, device=dev).to(dt)
        ops.reparam_sample(mu, rho, out, G, SEED, s0, layer, Cout, Cin, R * R, cin_pad=cin_pad)
        out_ex = torch.full((G, Cout, R, R, cp), 7.0, device=dev).to(dt)
        ops.reparam_sample_ex(mu, rho, out_ex, G, SEED, 5, base, layer, Cout, Cin, R * R,
                              cin_pad=cin_pad)
        f32 = torch.full((G, Cout, R, R, cp), 7.0, device=dev)
        ops.reparam_sample(mu, rho, f32, G, SEED, s0, layer, Cout, Cin, R * R, cin_pad=cin_pad)
        torch.cuda.synchronize()
    finally:
        ops.set_reparam_kernels(sample_blk=prev[0])
    ref = _sample_ref(mu, rho, G, s0, layer).permute(0, 1, 3, 4, 2)
    close(out[..., :Cin].float(), ref, rtol=rtol)
    ref_ex = _sample_ref(mu, rho, G, 5 + 2 ** 32 - 7, layer).permute(0, 1, 3, 4, 2)
    close(out_ex[..., :Cin].float(), ref_ex, rtol=rtol)
    if cp > Cin:
        assert (out[..., Cin:].float() == 7.0).all() and (out_ex[..., Cin:].float() == 7.0).all()
    if dt == torch.bfloat16 or (dt == torch.float16 and blk and Cin % 4 == 0):
        assert torch.equal(out, f32.to(dt))   # the fp32 sample rounded once more


@pytest.mark.parametrize("blk", [False, True], ids=["elem", "blk"])
def test_sample_qkv_slabs(blk):
    """Three (32, 64, 1) layers (ids 10, 12, 14) and their biases (11, 13, 15) written into one
    [G, 96, 64] / [G, 96] buffer through out_gstride — the attention q|k|v projection: every
    slab holds its own layer's epsilons and nothing is written outside it."""
    from mauv import ops
    torch.manual_seed(32)
    G, Hd, D, s0 = 3, 32, 64, 2 ** 32 - 2
    w = torch.full((G, 3 * Hd, D), 7.0, device=dev)
    b = torch.full((G, 3 * Hd + 1), 7.0, device=dev)   # one guard column
    ps = [((0.1 * torch.randn(Hd, D)).to(dev), (torch.randn(Hd, D) - 3).to(dev),
           (0.1 * torch.randn(Hd)).to(dev), (torch.randn(Hd) - 3).to(dev)) for _ in range(3)]
    prev = ops.set_reparam_kernels(sample_blk=blk)
    try:
        for j in (0, 2, 1):   # the middle slab is written last: its neighbours must survive it
            mu, rho, mub, rhob = ps[j]
            ops.reparam_sample(mu, rho, w.view(G, -1)[:, j * Hd * D:], G, SEED, s0, 10 + 2 * j,
                               Hd, D, 1, out_gstride=3 * Hd * D)
            ops.reparam_sample(mub, rhob, b[:, j * Hd:], G, SEED, s0, 11 + 2 * j, Hd, 1, 1,
                               out_gstride=3 * Hd + 1)
        torch.cuda.synchronize()
    finally:
        ops.set_reparam_kernels(sample_blk=prev[0])
    ref_w = torch.cat([_sample_ref(p[0], p[1], G, s0, 10 + 2 * j) for j, p in enumerate(ps)], 1)
    ref_b = torch.cat([_sample_ref(p[2], p[3], G, s0, 11 + 2 * j) for j, p in enumerate(ps)], 1)
    close(w, ref_w)
    close(b[:, :3 * Hd], ref_b)
    assert (b[:, 3 * Hd] == 7.0).all()


# ------------------------------------------------------------------ 4. backward regeneration
BWD_SHAPES = [
    # G, Cout, Cin, R, splits, dw_cin   (the first eight: test_reparam_bwd_sample_batches)
    (11, 24, 20, 3, 3, None), (11, 8, 70, 1, 3, None), (5, 24, 20, 3, 3, None),
    (12, 16, 64, 3, 3, None), (5, 16, 300, 1, 20, None), (3, 8, 64, 1, 7, None),
    (5, 32, 128, 3, 9, None), (2, 4, 12, 1, 1, None),
    (3, 16, 3, 7, 2, 8),            # padded 16-bit stem
    (3, 8, 147, 1, 2, "kp32"),      # the stem as one GEMM, fp32 / 16-bit row width
    (3, 8, 147, 1, 2, "kp16"),
    (3, 8, 12, 1, 2, "slab"),       # a column slice of a wider [splits][G][3*Cout*Cin] slab
    (3, 8, 1, 1, 1, "slab"),        # ... of a [G][3*Cout] bias slab (db[:, j*Hd:])
]
BWD_S0, BWD_LAYER = 2 ** 32 - 3, 9


@pytest.mark.parametrize("fixed_off", [None, -1, 4], ids=["exact", "fixed_last", "fixed_later"])
@pytest.mark.parametrize("bwd4", [False, True], ids=["bwd", "bwd4"])
@pytest.mark.parametrize("G,Cout,Cin,R,splits,dw_cin", BWD_SHAPES)
def test_bwd_regenerates_restated_eps(G, Cout, Cin, R, splits, dw_cin, bwd4, fixed_off):
    """reparam_bwd with eps=None against float64 on restated epsilons: the epsilon the backward
    regenerates is the one the forward drew (sample0 + g, layer, OIHW quad) in exact mode, and
    the one of MC sample ``fixed_sample`` in reference mode — the forward's last sample, or one
    of a LATER forward (sample0 + G + 4: engine._reparam_bwd passes st.offset - 1 when another
    forward ran before the backward).  Both kernels, ragged channel blocks, 1 to 20 split-K
    slabs, padded KRSC rows (pad channels hold 1e9 and are ignored), strided slabs; sample0 =
    2^32 - 3 crosses the sample's word boundary; gradients accumulate onto nonzero values."""
    from mauv import ops
    torch.manual_seed(9)
    s0, RS = BWD_S0, R * R
    fixed = -1 if fixed_off is None else s0 + G + fixed_off
    mu = torch.randn(Cout, Cin, R, R) * 0.1
    rho = torch.randn(Cout, Cin, R, R) - 3
    dmu0, drho0 = torch.randn(Cout, Cin, R, R), torch.randn(Cout, Cin, R, R)
    kw = {}
    if dw_cin == "slab":
        j, wide = 1, 3 * Cout * Cin
        slab = torch.randn(splits, G, wide)
        dws = slab[:, :, j * Cout * Cin:(j + 1) * Cout * Cin].reshape(splits, G, Cout, R, R, Cin)
        slab_d = slab.to(dev)
        dw_d = slab_d[:, :, j * Cout * Cin:]
        kw = dict(dw_gstride=wide, dw_sstride=G * wide)
        cp = Cin
    else:
        if dw_cin in ("kp32", "kp16"):
            dw_cin = ops.stem_kp(torch.float32 if dw_cin == "kp32" else torch.bfloat16, Cin)
        cp = dw_cin or Cin
        dws = torch.randn(splits, G, Cout, R, R, cp)
        dws[..., Cin:] = 1e9
        dw_d = dws.to(dev)
        if dw_cin:
            kw = dict(dw_cin=dw_cin)
    dmu, drho = dmu0.clone().to(dev), drho0.clone().to(dev)
    prev = ops.set_reparam_kernels(bwd4=bwd4)
    try:
        ops.reparam_bwd(dw_d, splits, mu.to(dev), rho.to(dev), dmu, drho, G, SEED, s0, BWD_LAYER,
                        Cout, Cin, RS, fixed_sample=fixed, **kw)
        torch.cuda.synchronize()
    finally:
        ops.set_reparam_kernels(bwd4=prev[1])
    dW = dws[..., :Cin].double().sum(0).permute(0, 1, 4, 2, 3)   # [G][Cout][Cin][R][R]
    e = torch.stack([_eps(mu.numel(), fixed if fixed >= 0 else s0 + g, BWD_LAYER)
                     for g in range(G)]).view(G, Cout, Cin, R, R)
    close(dmu, dmu0.double() + dW.sum(0))
    close(drho, drho0.double() + (dW * e).sum(0) * torch.sigmoid(rho.double()))


def test_bwd_rejects_fixed_sample_before_window():
    """0 <= fixed_sample < sample0 is an argument error (the kernels would take exact mode from
    fixed_sample - sample0 < 0 with a term count sized for fixed mode); it returns before any
    launch and leaves the gradients alone."""
    from mauv import ops
    mu = torch.zeros(4, 4, 1, 1, device=dev)
    dw = torch.ones(1, 2, 4, 1, 1, 4, device=dev)
    dmu, drho = torch.zeros_like(mu), torch.zeros_like(mu)
    for bwd4 in (False, True):
        prev = ops.set_reparam_kernels(bwd4=bwd4)
        try:
            with pytest.raises(RuntimeError, match="fixed_sample"):
                ops.reparam_bwd(dw, 1, mu, mu, dmu, drho, 2, SEED, 10, 9, 4, 4, 1, fixed_sample=9)
            with pytest.raises(RuntimeError, match="fixed_sample"):
                ops.reparam_bwd(dw, 1, mu, mu, dmu, drho, 2, SEED, 2 ** 32 + 1, 9, 4, 4, 1,
                                fixed_sample=0)
        finally:
            ops.set_reparam_kernels(bwd4=prev[1])
    torch.cuda.synchronize()
    assert not dmu.any() and not drho.any()


# ------------------------------------------------------------------ 5. model level
S0, NPASS = 5, 5


@pytest.fixture(scope="module")
def store():
    """The restated epsilons of MC samples 5 .. 9 for all 174 layers (~4 s of numpy per pass),
    built once and shared: the train steps replay passes 0-2, the inference test all five."""
    _, m = build_pair()
    return philox_store(m, SEED, S0, NPASS)


def _first(store, n):
    return {k: v[:n] for k, v in store.items()}


def _batch(seed=SEED_DATA, B=2):
    batch = make_batches(seed, 1, B=B, S_opt=64, S_son=64)[0]
    return batch["main_image"], batch["bathy_image"], batch["sss_image"], batch["label"]


def _cuda(*ts):
    return [t.cuda() for t in ts]


class _Stepper:
    """One HIP train step from the same start (parameters, running statistics, zeroed gradients,
    sample counter S0, seed SEED), free-running or with an epsilon provider."""

    def __init__(self, m):
        from mauv.engine import root_state
        self.m, self.st = m, root_state(m)
        self.sd = {k: v.clone() for k, v in m.state_dict().items()}

    def reset(self, provider):
        self.m.load_state_dict(self.sd)
        for p in self.m.parameters():
            p.grad = None
        self.st.seed, self.st.offset = SEED, S0
        self.st.__dict__.pop("eps_last", None)
        self.st.refresh_centres()
        self.st.eps_provider = provider(self.m, SEED, S0) if provider else None

    def grads(self):
        return [None if p.grad is None else p.grad.detach().clone() for p in self.m.parameters()]


def _assert_bit_equal(free, prov):
    (lg_f, loss_f, g_f), (lg_p, loss_p, g_p) = free, prov
    assert torch.equal(lg_f, lg_p)
    assert loss_f == loss_p
    for i, (a, b) in enumerate(zip(g_f, g_p)):
        assert (a is None) == (b is None), i
        if a is not None:
            assert torch.equal(a, b), (i, (a - b).abs().max().item())


def _mc_step(stp, x, b, s, y, N, kl):
    from mauv.kl import get_kl_loss
    from mauv import mchead
    logits = stp.m.mc_forward(*_cuda(x, b, s), N)
    ce, _, _ = mchead.mc_mean_ce(logits, y.cuda())
    loss = ce + get_kl_loss(stp.m) / x.shape[0] * 0.5 if kl else ce
    loss.backward()
    torch.cuda.synchronize()
    return logits.detach().clone(), loss.item()


def test_train_step_free_running_reference_mode(store):
    """One MC train step (N = 3 from sample 5, CE + KL, bayesian-torch's aliased rho gradient)
    with NO epsilon provider against the oracle replaying the restated Philox stream: logits,
    loss and all gradients at the bars of tests/test_model_gpu.py; then the same step with
    ops.philox_raw's normals fed through the explicit-epsilon path is bit-identical in the
    logits and every gradient — any epsilon mismatch in any of the 174 layers' forward or
    backward breaks that."""
    o, m = build_pair()
    x, b, s, y = _batch()
    N, B = 3, x.shape[0]
    st3 = _first(store, N)

    def oracle_loss(model, dt=torch.float32):
        lg = torch.stack([model(x.to(dt), b.to(dt), s.to(dt)) for _ in range(N)])
        loss = F.cross_entropy(lg.mean(0), y) + bayes_ref.get_kl_loss(model) / B * 0.5
        loss.backward()
        return lg, loss

    o32, (o_logits, loss_o) = oracle_replay(o, st3, oracle_loss)
    o64, (l64, _) = oracle64(o, st3, lambda mm: oracle_loss(mm, torch.float64))
    stp = _Stepper(m)
    stp.reset(None)
    logits, loss = _mc_step(stp, x, b, s, y, N, kl=True)
    assert stp.st.offset == S0 + N
    _assert_close(logits, o_logits)
    _assert_close(logits, l64)
    assert abs(loss - loss_o.item()) <= 1e-4 * abs(loss_o.item())
    _assert_grads_as_accurate(list(m.parameters()), list(o32.parameters()), list(o64.parameters()))
    free = (logits, loss, stp.grads())
    stp.reset(PhiloxRawProvider)
    logits_p, loss_p = _mc_step(stp, x, b, s, y, N, kl=True)
    _assert_bit_equal(free, (logits_p, loss_p, stp.grads()))


def test_train_step_free_running_exact_mode(store):
    """The same with rho_grad = "exact" (per-sample epsilons in the backward), cross-entropy
    only: gradients against the float64 oracle with non-aliased epsilons, and bit-equality with
    the provider run."""
    from mauv.engine import set_rho_grad_mode
    o, m = build_pair()
    x, b, s, y = _batch()
    N = 3
    st3 = _first(store, N)

    def oracle_loss(model, dt=torch.float32):
        lg = torch.stack([model(x.to(dt), b.to(dt), s.to(dt)) for _ in range(N)])
        F.cross_entropy(lg.mean(0), y).backward()
        return lg

    bayes_ref.ALIAS_EPS = False
    try:
        o32, o_logits = oracle_replay(o, st3, oracle_loss)
        o64, _ = oracle64(o, st3, lambda mm: oracle_loss(mm, torch.float64))
    finally:
        bayes_ref.ALIAS_EPS = True
    set_rho_grad_mode(m, "exact")
    stp = _Stepper(m)
    stp.reset(None)
    logits, loss = _mc_step(stp, x, b, s, y, N, kl=False)
    _assert_close(logits, o_logits)
    _assert_grads_as_accurate(list(m.parameters()), list(o32.parameters()), list(o64.parameters()))
    free = (logits, loss, stp.grads())
    stp.reset(PhiloxRawProvider)
    logits_p, loss_p = _mc_step(stp, x, b, s, y, N, kl=False)
    _assert_bit_equal(free, (logits_p, loss_p, stp.grads()))


def test_sequential_forwards_one_backward_free_running():
    """The noise Examples' pattern (test_noise_examples_sequential_grad_pattern, 64 px, B = 2,
    N = 3): N grad-enabled single-sample forwards, then ONE backward — every forward but the
    last regenerates the epsilon of a sample beyond its own window (fixed_sample = st.offset - 1).
    Free-running equals the provider run bit for bit."""
    from mauv.kl import get_kl_loss
    _, m = build_pair()
    x, b, s, y = _batch(SEED_DATA + 2)
    N, B = 3, x.shape[0]
    stp = _Stepper(m)

    def run(provider):
        stp.reset(provider)
        outs, kls = [], []
        for _ in range(N):
            outs.append(m(*_cuda(x, b, s)))
            kls.append(get_kl_loss(m))
        output = torch.mean(torch.stack(outs), dim=0)
        loss = F.cross_entropy(output, y.cuda()) + torch.mean(torch.stack(kls), dim=0) / B * 0.5
        loss.backward()
        torch.cuda.synchronize()
        assert stp.st.offset == S0 + N
        return torch.stack(outs).detach().clone(), loss.item(), stp.grads()

    free = run(None)
    assert not torch.equal(free[0][0], free[0][1])
    _assert_bit_equal(free, run(PhiloxRawProvider))


def test_bf16_train_step_free_running():
    """bf16 trunks (the padded 16-bit stems, the 16-bit sampling and the fold): one free-running
    step equals the provider run bit for bit."""
    _, m = build_pair()
    x, b, s, y = _batch()
    stp = _Stepper(m)
    stp.st.precision = torch.bfloat16
    runs = []
    for provider in (None, PhiloxRawProvider):
        stp.reset(provider)
        logits, loss = _mc_step(stp, x, b, s, y, 2, kl=True)
        runs.append((logits, loss, stp.grads()))
    assert torch.isfinite(runs[0][0]).all()
    _assert_bit_equal(*runs)


def test_inference_chunks_free_running(store):
    """mc_statistics(N = 5, chunk = 2) in fp32 under no_grad, free-running and eager, against the
    oracle's sequential 5-pass statistics on the restated stream (entropies 1e-5, variances 1e-6
    absolute, the class): the chunks consume sample indices 5 .. 9 without gaps or reuse.  Also
    bit-equal to the provider run."""
    from mauv import predict
    from mauv.engine import root_state
    from mauv.predict import mc_statistics
    o, m = build_pair()
    x, b, s, _ = _batch()
    N = NPASS
    _, (pred_o, var_o, alea_o, P) = oracle_replay(
        o, store, lambda mm: loops_ref.predict_batch(mm, x, b, s, N))
    pm = P.double().mean(0)
    pent_o = -(pm * torch.log(pm + 1e-8)).sum(-1)
    st = root_state(m)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    prev = predict.GRAPH_INFER
    predict.GRAPH_INFER = False
    runs = []
    try:
        for provider in (None, PhiloxRawProvider):
            m.load_state_dict(sd)
            st.seed, st.offset = SEED, S0
            st.eps_provider = provider(m, SEED, S0) if provider else None
            with torch.no_grad():
                runs.append({k: v.clone() for k, v in
                             mc_statistics(m, *_cuda(x, b, s), N, chunk=2).items()})
            assert st.offset == S0 + N
    finally:
        predict.GRAPH_INFER = prev
    free, prov = runs
    assert torch.equal(free["pred"].cpu(), pred_o)
    np.testing.assert_allclose(free["var"].cpu().numpy(), var_o.numpy(), atol=1e-6, rtol=1e-3)
    np.testing.assert_allclose(free["aleatoric"].cpu().numpy(), alea_o.numpy(), atol=1e-5)
    np.testing.assert_allclose(free["predictive_entropy"].double().cpu().numpy(), pent_o.numpy(),
                               atol=1e-5)
    for k in free:
        assert torch.equal(free[k], prov[k]), k


def test_standalone_layer_free_running():
    """A standalone Conv2dReparameterization(64, 64, 3) root (run_layer): its kernel draws layer
    id 0 and its bias layer id 1 at the root's own sample counter, against float64 F.conv2d on
    restated epsilons."""
    from mauv.layers import Conv2dReparameterization
    from mauv.engine import root_state, run_layer
    torch.manual_seed(41)
    layer = Conv2dReparameterization(64, 64, 3, padding=1, bias=True)
    with torch.no_grad():
        layer.mu_kernel.normal_(0, 0.1)
        layer.rho_kernel.normal_(-3, 1)
        layer.mu_bias.normal_(0, 0.1)
        layer.rho_bias.normal_(-3, 1)
    layer = layer.to(dev)
    st = root_state(layer)
    assert (st.layer_id(layer), st.layer_id(layer, True)) == (0, 1)
    s0 = 2 ** 32 - 1
    st.seed, st.offset = SEED, s0
    x = torch.randn(2, 64, 8, 8)
    for k in range(2):   # the second call draws the next sample index (across the word boundary)
        with torch.no_grad():
            y = run_layer(layer, x.to(dev))
        w = _sample_ref(layer.mu_kernel.detach(), layer.rho_kernel.detach(), 1, s0 + k, 0)[0]
        bias = _sample_ref(layer.mu_bias.detach(), layer.rho_bias.detach(), 1, s0 + k, 1)[0]
        close(y, F.conv2d(x.double(), w, bias, padding=1))
    assert st.offset == s0 + 2


# ------------------------------------------------------------------ 6. stream separation
def test_streams_are_uncorrelated_and_ids_distinct():
    """2^20 normals (mu = 0, softplus(rho) = 1: w = eps) of the base stream (SEED, sample 77,
    layer 6) against the neighbouring layers, the next sample, the sample 2^32 further (the
    counter's high word), the DistributedMC rank seeds and the (sample, layer) pair swapped:
    |correlation| < 4 / sqrt(n) = 3.9e-3 (the restatement itself stays within 2.0e-3 for these
    inputs).  And the engine's ids give every weight and bias of the model its own layer id."""
    from mauv import ops
    from mauv.engine import root_state
    from mauv.models import define_models, DEFAULT_PRIOR
    Cout, Cin = 256, 4096
    n = Cout * Cin
    mu = torch.zeros(Cout, Cin, 1, 1, device=dev)
    rho = torch.full((Cout, Cin, 1, 1), math.log(math.e - 1), device=dev)

    def draw(seed, sample, layer):
        out = torch.empty(1, Cout, 1, 1, Cin, device=dev)
        ops.reparam_sample(mu, rho, out, 1, seed, sample, layer, Cout, Cin, 1)
        return out.double().flatten()

    base = draw(SEED, 77, 6)
    assert abs(base.mean().item()) < 4 / math.sqrt(n) and abs(base.std().item() - 1) < 4e-3
    ranks = [(SEED + 0x9E3779B97F4A7C15 * (r + 1)) % (1 << 62) for r in (0, 1, 7)]
    others = [(SEED, 77, 7), (SEED, 77, 8), (SEED, 78, 6), (SEED, 77 + 2 ** 32, 6)] + \
        [(sd, 77, 6) for sd in ranks] + [(SEED, 6, 77)]
    for key in others:
        o = draw(*key)
        rho_c = torch.corrcoef(torch.stack([base, o]))[0, 1].item()
        assert abs(rho_c) < 4 / math.sqrt(n), (key, rho_c)
    m = define_models(None, 7, DEFAULT_PRIOR)["multimodal_model"]
    ids = root_state(m).ids
    lids = {2 * i + bias for i in ids.values() for bias in (0, 1)}
    assert len(lids) == 348 and max(lids) == 347
