"""Shared helpers for the parity tests: build matching oracle / mauv models and feed both the
same epsilons (the oracle's draws are recorded and replayed into the HIP sampler)."""
import torch

from oracle import bayes_ref
from oracle.model_ref import define_models as oracle_define, DEFAULT_PRIOR
from tests.golden.common import RecordingEpsSource


def build_pair(seed=0, num_classes=7, key="multimodal_model"):
    from mauv.models import define_models
    torch.manual_seed(seed)
    o = oracle_define(None, num_classes, DEFAULT_PRIOR)[key]
    torch.manual_seed(seed)
    m = define_models(None, num_classes, DEFAULT_PRIOR)[key]
    m.load_state_dict(o.state_dict())
    return o, m.cuda()


class EpsBridge:
    """Record the oracle's per-layer epsilons over N sequential passes and serve them to the
    mauv engine as [G, numel] tensors keyed by the same qualified module name."""

    def __init__(self, oracle_model, mauv_model, seed):
        self.src = RecordingEpsSource(seed)
        self.o_names = {id(mod): n for n, mod in oracle_model.named_modules()}
        self.m_names = {id(mod): n for n, mod in mauv_model.named_modules()}
        self.store = {}

    def __enter__(self):
        bayes_ref.set_eps_source(self.src)
        return self

    def __exit__(self, *a):
        bayes_ref.set_eps_source(None)

    def collect(self):
        self.store = {}
        for layer, name, e in self.src.log:
            self.store.setdefault((self.o_names[id(layer)], name), []).append(e.reshape(-1))
        self.src.log.clear()

    def provider(self, module, name, G):
        lst = self.store[(self.m_names[id(module)], name)]
        assert len(lst) >= G, (self.m_names[id(module)], name, len(lst), G)
        return torch.stack(lst[:G]).cuda().contiguous()

    def sequential(self):
        """A provider that hands out each layer's recorded draws in order across calls: MC
        chunks (mc_statistics with chunk < N) get passes 0..c-1, c..2c-1, ... as the oracle's
        sequential loop consumed them (``provider`` restarts at pass 0 on every call)."""
        used = {}

        def prov(module, name, G):
            k = (self.m_names[id(module)], name)
            i = used.get(k, 0)
            lst = self.store[k]
            assert len(lst) >= i + G, (k, len(lst), i, G)
            used[k] = i + G
            return torch.stack(lst[i:i + G]).cuda().contiguous()
        return prov


# mauv_common.h::normal4 against oracle.philox_ref.normal4(u32=True): max |gpu - ref| /
# max(|ref|, 2^-10) in units of 2^-24, measured once on an MI355X over the quads of
# tests/test_philox_stream_gpu.py::test_philox_raw_counter_edges (the error of the kernel's fp32
# logf / sqrtf / sincospif), and the asserted bar: 4x that, for libm differences between ROCm
# releases
NORMAL_MEASURED = 3.93    # worst of 2^18 quads at (seed 0x123456789ABC, sample 77, layer 6)
NORMAL_BAR = 4 * NORMAL_MEASURED   # 15.72: 5.6e-6 absolute at |eps| = 6


def normal_err_units(got, ref_raw):
    """max |got - ref| / max(|ref|, 2^-10) in units of 2^-24 of GPU normals [nq * 4] against the
    fp32-uniform restatement of the same Philox words (the figure NORMAL_BAR bounds)."""
    import numpy as np
    from oracle.philox_ref import normal4
    ref = normal4(ref_raw, u32=True)
    got = np.asarray(got, dtype=np.float64).reshape(-1, 4)
    assert np.isfinite(got).all()
    return float((np.abs(got - ref) / np.maximum(np.abs(ref), 2.0 ** -10)).max() * 2.0 ** 24)


def _bayes_tensors(mauv_model):
    """[(module name, module, eps name, numel, bias?)] of every Bayesian tensor of a mauv model,
    in module order: the (layer, tensor) pairs the engine draws an epsilon for."""
    from mauv.layers import is_bayesian
    out = []
    for n, mod in mauv_model.named_modules():
        if not is_bayesian(mod):
            continue
        w = "kernel" if hasattr(mod, "mu_kernel") else "weight"
        out.append((n, mod, w, getattr(mod, "mu_" + w).numel(), False))
        if mod.mu_bias is not None:
            out.append((n, mod, "bias", mod.mu_bias.numel(), True))
    return out


def philox_store(mauv_model, seed, s0, passes, u32=True):
    """The epsilons the free-running engine draws for MC samples s0 .. s0+passes-1, restated on
    the CPU (oracle.philox_ref.eps_for_layer keyed by the engine's own layer ids) in the format
    EpsBridge.collect produces — {(module name, "kernel"|"weight"|"bias"): [eps of pass 0, 1,
    ...]}, fp32 like the recorded draws — so oracle_replay / oracle64 replay the production
    stream."""
    from mauv.engine import root_state
    from oracle.philox_ref import eps_for_layer
    st = root_state(mauv_model)
    store = {}
    for n, mod, name, numel, bias in _bayes_tensors(mauv_model):
        lid = st.layer_id(mod, bias)
        store[(n, name)] = [torch.from_numpy(eps_for_layer(numel, seed, s0 + g, lid, u32=u32)).float()
                            for g in range(passes)]
    return store


class PhiloxRawProvider:
    """eps_provider that serves each layer's [G, numel] from ops.philox_raw(seed, s0 + g,
    layer id, quads): the normals the sampling and backward kernels themselves draw, fed through
    the explicit-epsilon path.  A layer asked in more than one engine call (MC chunks, sequential
    forwards) gets the next G sample indices each time, as EpsBridge.sequential hands out the
    recorded passes."""

    def __init__(self, model, seed, s0):
        from mauv.engine import root_state
        self.st, self.seed, self.s0 = root_state(model), seed, s0
        self.numel = {(id(mod), name): (numel, bias)
                      for _, mod, name, numel, bias in _bayes_tensors(model)}
        self.used = {}

    def __call__(self, module, name, G):
        from mauv import ops
        key = (id(module), name)
        numel, bias = self.numel[key]
        i = self.used.get(key, 0)
        self.used[key] = i + G
        lid = self.st.layer_id(module, bias)
        rows = [ops.philox_raw(self.seed, self.s0 + i + g, lid, (numel + 3) // 4)[1][:numel]
                for g in range(G)]
        return torch.stack(rows).contiguous()


def oracle64(o, store, fn):
    """Run ``fn(o64)`` on a float64 copy of the oracle, replaying the recorded epsilons
    (``store`` from EpsBridge.collect) in the same per-layer order -> the 'truth' used to
    judge the fp32 HIP path against the fp32 CPU path (both are fp32 chains through an
    ill-conditioned BN backward at small spatial sizes)."""
    import copy
    o64 = copy.deepcopy(o).double()
    for p in o64.parameters():
        p.grad = None
    names = {id(mod): n for n, mod in o64.named_modules()}
    cnt = {}

    def src(layer, name, shape):
        k = (names[id(layer)], name)
        i = cnt.get(k, 0)
        cnt[k] = i + 1
        return store[k][i].double().reshape(shape)
    bayes_ref.set_eps_source(src)
    try:
        out = fn(o64)
    finally:
        bayes_ref.set_eps_source(None)
    return o64, out


def oracle_replay(o, store, fn, dtype=torch.float32, device="cpu"):
    """``fn(copy)`` on a copy of the oracle moved to ``device`` / ``dtype``, replaying the
    recorded epsilons (EpsBridge.collect) in the same per-layer order.  With device="cuda"
    and ``fn`` running under torch.autocast this is the reference's own mixed-precision
    scheme (inference/predictors.py:55) on the same weights and epsilons: the bar for the
    16-bit HIP paths."""
    import copy
    oc = copy.deepcopy(o).to(device=device, dtype=dtype)
    for p in oc.parameters():
        p.grad = None
    names = {id(mod): n for n, mod in oc.named_modules()}
    cnt = {}

    def src(layer, name, shape):
        k = (names[id(layer)], name)
        i = cnt.get(k, 0)
        cnt[k] = i + 1
        return store[k][i].to(dtype).reshape(shape)
    bayes_ref.set_eps_source(src)
    try:
        out = fn(oc)
    finally:
        bayes_ref.set_eps_source(None)
    return oc, out


def cosines(params, truth_params):
    """name -> cosine similarity of each parameter's gradient with the truth's gradient
    (tensors whose true gradient is zero are skipped)."""
    out = {}
    for (n, p), pt in zip(params, truth_params):
        if pt.grad is None or p.grad is None:
            continue
        t = pt.grad.detach().double().cpu().flatten()
        if t.norm() == 0:
            continue
        a = p.grad.detach().double().cpu().flatten()
        out[n] = float(a @ t / (a.norm() * t.norm() + 1e-300))
    return out


def fit_model(m, x, b, s, labels, steps=20, lr=1e-3, num_mc=2):
    """A few FusedAdam MC training steps (fp32) of a mauv model on one batch so that its
    predicted class depends on the input (tests of class agreement): at random init the
    per-item logits differ by ~3e-4 — less than the MC noise — and every item gets one class
    (every golden row is class 4).  Returns the cross-entropy of the last step."""
    from mauv.optim import FusedAdam
    from mauv.train import mc_train_step
    opt = FusedAdam(m.parameters(), lr=lr)
    crit = torch.nn.CrossEntropyLoss()
    ce = None
    for _ in range(steps):
        r = mc_train_step(m, (x, b, s), labels, crit, opt, num_mc, labels.numel(), 1e-6)
        ce = float(r["ce"])
    opt.zero_grad(set_to_none=True)
    return ce


def grad_error_profile(hip_params, cpu_params, truth_params):
    """Per-tensor max-relative errors of HIP and CPU-fp32 grads vs the fp64 truth."""
    hip, cpu = [], []
    for ph, pc, pt in zip(hip_params, cpu_params, truth_params):
        if pt.grad is None:
            continue
        hip.append(max_rel(ph.grad, pt.grad))
        cpu.append(max_rel(pc.grad, pt.grad))
    import numpy as np
    q = lambda v: np.quantile(np.array(v), [0.5, 0.9, 1.0])
    return q(hip), q(cpu)


def max_rel(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


def forward_order(oracle_model, *inputs):
    """[(module name, eps name, shape)] in the order one oracle forward draws its epsilons —
    the order the reference's bayesian-torch layers consume torch's generator."""
    names = {id(mod): n for n, mod in oracle_model.named_modules()}
    order = []

    def src(layer, name, shape):
        order.append((names[id(layer)], name, shape))
        return torch.zeros(shape)
    bayes_ref.set_eps_source(src)
    try:
        with torch.no_grad():
            oracle_model(*inputs)
    finally:
        bayes_ref.set_eps_source(None)
    return order


class ReplayEps:
    """eps_provider for the mauv engine that replays ``eps_generator_source(seed)`` — the
    stream the golden run fed the reference — in the reference's consumption order: pass k of
    the sequential MC loop draws every layer's epsilon in forward order before pass k+1.  The
    engine asks per layer for the next G passes; each request that runs past the passes
    generated so far draws whole passes from the generator, so chunked MC consumption matches
    the sequential stream."""

    def __init__(self, model, order, seed):
        self.g = torch.Generator().manual_seed(seed)
        self.order = order
        self.names = {id(mod): n for n, mod in model.named_modules()}
        self.queues = {(n, e): [] for n, e, _ in order}

    def _draw_pass(self):
        for n, e, shape in self.order:
            self.queues[(n, e)].append(torch.randn(shape, generator=self.g).reshape(-1))

    def __call__(self, module, name, G):
        q = self.queues[(self.names[id(module)], name)]
        while len(q) < G:
            self._draw_pass()
        out, q[:G] = q[:G], []
        return torch.stack(out).cuda().contiguous()


class ListLoader:
    """Minimal DataLoader stand-in (iterable of batches with ``batch_size``), as the golden
    run fed the reference loops (tests/golden/make_golden.py)."""

    def __init__(self, batches, batch_size):
        self.batches, self.batch_size = batches, batch_size

    def __iter__(self):
        return iter(self.batches)

    def __len__(self):
        return len(self.batches)


class NullWriter:
    """SummaryWriter stand-in (tensorboard is not installed)."""

    def add_scalar(self, *a, **k):
        pass


# ---- pooling kernels against torch in float64 (tests/test_kernels_gpu.py fp32, test_kernels16_gpu.py)
# (N, H, W, C): one pixel, W != H throughout, odd and even extents, 1 to 8 channel chunks
POOL_SHAPES = [(1, 1, 1, 8), (2, 2, 3, 8), (1, 4, 6, 16), (3, 7, 5, 24), (2, 9, 12, 64)]


def check_maxpool(dt, N, H, W, C, close):
    """maxpool_fwd + maxpool_bwd on N non-square NHWC images of storage type ``dt`` against
    F.max_pool2d(return_indices=True) in float64 on the same rounded inputs: equal pooled values,
    argmax bytes equal to torch's index as the tap r*3 + s of its window, dx against autograd
    (``close``; bit-equal in fp32 wherever at most one window feeds the pixel).  A block of zeros
    gives ties (first maximum in scan order) and one NaN input wins its windows, as in torch."""
    import torch.nn.functional as F
    from mauv import ops
    torch.manual_seed(N * 1000 + H * 100 + W)
    x = torch.randn(N, H, W, C).to(dt)
    x[0, :3, :3, :] = 0.0
    x[N - 1, H - 1, W // 2, 3] = float("nan")
    Ho, Wo = ops.out_hw(H, 3, 2, 1), ops.out_hw(W, 3, 2, 1)
    y = torch.empty(N, Ho, Wo, C, device="cuda", dtype=dt)
    idx = torch.empty(N, Ho, Wo, C, dtype=torch.uint8, device="cuda")
    ops.maxpool_fwd(x.cuda(), N, H, W, C, y, idx)
    xr = x.double().permute(0, 3, 1, 2).requires_grad_(True)
    yr, flat = F.max_pool2d(xr, 3, 2, 1, return_indices=True)
    yk, yt = y.double().cpu(), yr.detach().permute(0, 2, 3, 1)
    assert yt.isnan().any() and bool(((yk == yt) | (yk.isnan() & yt.isnan())).all())
    oh = torch.arange(Ho).view(1, 1, Ho, 1)
    ow = torch.arange(Wo).view(1, 1, 1, Wo)
    tap = (flat // W - (2 * oh - 1)) * 3 + (flat % W - (2 * ow - 1))
    assert bool(((tap >= 0) & (tap < 9)).all())
    assert torch.equal(idx.cpu(), tap.permute(0, 2, 3, 1).to(torch.uint8))
    dy = torch.randn(N, Ho, Wo, C).to(dt)
    yr.backward(dy.double().permute(0, 3, 1, 2))
    dx = torch.empty(N, H, W, C, device="cuda", dtype=dt)
    ops.maxpool_bwd(dy.cuda(), idx, N, H, W, C, dx)
    ref = xr.grad.permute(0, 2, 3, 1)
    assert ref[N - 1, H - 1, W // 2, 3] != 0, "the NaN input takes its windows' gradient"
    close(dx, ref)
    if dt == torch.float32:
        fed = torch.zeros(N, C, H * W).scatter_add_(2, flat.reshape(N, C, -1),
                                                    torch.ones(N, C, Ho * Wo))
        one = (fed <= 1).view(N, C, H, W).permute(0, 2, 3, 1)
        assert torch.equal(dx.cpu().double()[one], ref[one])


def check_avgpool(dt, N, HW, C):
    """avgpool_fwd (fp32 means of ``dt`` storage) and avgpool_bwd against float64.  Bounds: a
    sequential fp32 sum of HW terms errs at most HW 2^-24 sum|x|, so the mean at most
    HW 2^-24 max|x|; dx = dy * fl(1/HW) takes two fp32 roundings (2^-23 |dx| to first order,
    2^-22 asserted) and, for 16-bit storage, the rounding to it (half an ulp: 2^-8 |dx| bf16;
    2^-11 |dx| f16, or 2^-25, half its subnormal spacing)."""
    from mauv import ops
    torch.manual_seed(HW * 10 + C)
    x = torch.randn(N, HW, C).to(dt)
    a = torch.empty(N, C, device="cuda")
    ops.avgpool_fwd(x.cuda(), N, HW, C, a)
    err = (a.double().cpu() - x.double().mean(1)).abs().max().item()
    assert err <= (HW + 1) * 2.0 ** -24 * x.double().abs().max().item(), err
    da = torch.randn(N, C)
    dxa = torch.empty(N, HW, C, device="cuda", dtype=dt)
    ops.avgpool_bwd(da.cuda(), N, HW, C, dxa)
    ref = (da.double() / HW)[:, None, :].expand(N, HW, C)
    rel = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}[dt] + 2.0 ** -22
    sub = 2.0 ** -25 if dt == torch.float16 else 0.0
    assert bool(((dxa.double().cpu() - ref).abs() <= rel * ref.abs() + sub).all())
