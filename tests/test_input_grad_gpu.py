"""Input gradients through the trunks (the stems' data gradient, stem_dgrad.hip) at model level:
64 px, B = 4, N = 2, fp32, the oracle's epsilons replayed as in tests/test_model_gpu.py; one
ragged case with a 72 x 88 optical tile.  The loss is the cross-entropy of the MC-mean logits
(mc_loss without its KL term, which does not depend on the inputs).

The bar for dx is the one tests/test_model_gpu.py applies to parameter gradients: against a
float64 run of the oracle, max_rel(HIP, fp64) <= 2 max_rel(oracle fp32, fp64) + 1e-4 for every
input (both sides are printed: pytest -rP).  Before the feature every ``x.grad`` here is None.

Also: logits and every parameter gradient are bit-identical with and without inputs requiring
grad; a fully frozen model (live and frozen BatchNorm) gives dx and no parameter gradient; under
mauv.freeze_batchnorm item 0's dx does not depend on the other items; one modality alone; the
16-bit trunks (finite, non-zero; bf16 against the oracle under torch.autocast by the random-init
cosine bar of tests/test_parity16_gpu.py); and the mauv.attribution helpers."""
import pytest
import torch
import torch.nn.functional as F

from tests.golden.common import make_batches, SEED_DATA
from tests.helpers import build_pair, EpsBridge, max_rel, oracle64, oracle_replay, fit_model
from tests.frozen_helpers import calibrated_pair, clone, to_gpu, provider

pytestmark = pytest.mark.gpu

B, N = 4, 2
KEYS = ("main_image", "bathy_image", "sss_image")


def _record_eps(o, names_model, inputs, seed=99):
    """The epsilons depend on the layers only: recorded on one-item forwards of the oracle."""
    bridge = EpsBridge(o, names_model, seed)
    with bridge, torch.no_grad():
        for _ in range(N):
            o(*[t[:1] for t in inputs])
    bridge.collect()
    return bridge.store


def _oracle_dx(o, store, inputs, y, dtype=torch.float32, device="cpu", amp=None):
    """d CE(mean_n logits) / d inputs of a replayed copy of the oracle (its BatchNorm state
    untouched), by plain autograd."""
    def fn(model):
        xs = [t.detach().clone().to(device, dtype).requires_grad_(True) for t in inputs]
        if amp is not None:
            with torch.autocast("cuda", dtype=amp):
                lg = torch.stack([model(*xs) for _ in range(N)])
        else:
            lg = torch.stack([model(*xs) for _ in range(N)])
        loss = F.cross_entropy(lg.to(dtype).mean(0), y.to(device))
        return [g.detach().cpu() for g in torch.autograd.grad(loss, xs)]
    if dtype == torch.float64:
        return oracle64(o, store, fn)[1]
    return oracle_replay(o, store, fn, dtype=dtype, device=device)[1]


def _hip_step(m, inputs, y, want=None):
    """Forward, CE of the MC-mean logits, backward on the mauv model -> (leaves, logits)."""
    want = range(len(inputs)) if want is None else want
    xs = [t.detach().cuda().requires_grad_(i in want) for i, t in enumerate(inputs)]
    logits = m.mc_forward(*xs, N)
    F.cross_entropy(logits.mean(0), y.cuda()).backward()
    torch.cuda.synchronize()
    return xs, logits.detach()


def _assert_bar(tag, got, o32, o64):
    for i, (g, a, t) in enumerate(zip(got, o32, o64)):
        assert g is not None, f"{tag}: input {i} has no gradient"
        assert g.shape == t.shape and g.dtype == torch.float32
        hip, cpu = max_rel(g, t), max_rel(a, t)
        print(f"{tag} input {i}: max_rel vs fp64: HIP {hip:.3e}, oracle fp32 {cpu:.3e}")
        assert torch.isfinite(g).all().item() and g.abs().max().item() > 0
        # Both sides are fp32 chains through the same ill-conditioned backward, so the ratio is
        # a draw: measured 0.4-1.97 over these cases (the frozen-BatchNorm
        # bathymetry and side-scan inputs 3.8e-2 vs 1.9e-2 and 1.6e-2 vs 8.5e-3).  The right-hand
        # side is the CPU oracle's own fp32 error, which moves with the host's BLAS summation
        # order and thread count: a miss by a few per cent on another host is that, not the
        # kernels (the kernel tests bound those at ~1e-7 relative).
        assert hip <= 2.0 * cpu + 1e-4, (tag, i, hip, cpu)


def _tri_reference(inputs, y):
    o, m = build_pair()
    store = _record_eps(o, m, inputs)
    # (m is a template that never runs: every test copies it, _model)
    return dict(o=o, m=m, store=store, inputs=inputs, y=y,
                o32=_oracle_dx(o, store, inputs, y),
                o64=_oracle_dx(o, store, inputs, y, torch.float64))


def _model(ref):
    from mauv.engine import root_state
    m = clone(ref["m"])
    root_state(m).eps_provider = provider(ref["store"], m)
    return m


@pytest.fixture(scope="module")
def tri():
    """The tri-modal pair at 64 px with the oracle's fp32 and float64 dx, computed once."""
    batch = make_batches(SEED_DATA, 1, B=B, S_opt=64, S_son=64)[0]
    return _tri_reference([batch[k] for k in KEYS], batch["label"])


def test_trimodal_input_gradients(tri):
    m = _model(tri)
    xs, _ = _hip_step(m, tri["inputs"], tri["y"])
    _assert_bar("tri-modal", [x.grad for x in xs], tri["o32"], tri["o64"])


@pytest.fixture(scope="module")
def uni():
    """The unimodal ResNet50Custom(3, 7) pair and its recorded epsilons (a template, as tri)."""
    o, m = build_pair(key="image_model")
    store = _record_eps(o, m, [make_batches(SEED_DATA, 1, B=1, S_opt=64, S_son=64)[0]["main_image"]],
                        seed=7)
    return dict(o=o, m=m, store=store)


@pytest.mark.parametrize("H,W", [(64, 64), (72, 88)], ids=["64", "ragged72x88"])
def test_unimodal_input_gradient(uni, H, W):
    """ResNet50Custom(3, 7) at 64 px and on a ragged optical tile: 72 x 88 gives the stem a
    36 x 44 grid (M = 6336: ragged against the 128-row tiles, H != W)."""
    g = torch.Generator().manual_seed(3)
    inputs, y = [torch.randn(B, 3, H, W, generator=g)], torch.randint(0, 7, (B,), generator=g)
    o32 = _oracle_dx(uni["o"], uni["store"], inputs, y)
    o64 = _oracle_dx(uni["o"], uni["store"], inputs, y, torch.float64)
    m = _model(uni)
    xs, _ = _hip_step(m, inputs, y)
    _assert_bar(f"ResNet50Custom(3, 7) {H}x{W}", [xs[0].grad], o32, o64)
    # forward (one sample) reaches the same backward
    x1 = inputs[0].cuda().requires_grad_(True)
    m(x1).sum().backward()
    assert x1.grad is not None and x1.grad.abs().max().item() > 0


def test_nothing_existing_moves(tri):
    """Same weights and epsilons: the logits and every parameter gradient have the same bits
    whether or not the inputs require grad."""
    runs = []
    for want in ((), (0, 1, 2)):
        m = _model(tri)
        xs, logits = _hip_step(m, tri["inputs"], tri["y"], want=want)
        assert all((x.grad is not None) == (i in want) for i, x in enumerate(xs))
        runs.append((logits, [p.grad.clone() for p in m.parameters()]))
    assert torch.equal(runs[0][0], runs[1][0])
    assert len(runs[0][1]) == 696
    assert all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))


def test_one_modality_only(tri):
    m = _model(tri)
    xs, _ = _hip_step(m, tri["inputs"], tri["y"], want=(1,))
    assert xs[0].grad is None and xs[2].grad is None
    _assert_bar("bathymetry only", [xs[1].grad], tri["o32"][1:2], tri["o64"][1:2])


def test_fully_frozen_model_live_batchnorm(tri):
    """Every parameter frozen: the logits still carry a graph, dx meets the bar, no parameter
    gets a gradient and no gradient arena is made."""
    from mauv.engine import root_state
    m = _model(tri)
    for p in m.parameters():
        p.requires_grad_(False)
    xs, _ = _hip_step(m, tri["inputs"], tri["y"])
    _assert_bar("frozen parameters", [x.grad for x in xs], tri["o32"], tri["o64"])
    assert all(p.grad is None for p in m.parameters())
    assert root_state(m).arena is None


def test_fully_frozen_model_frozen_batchnorm():
    """mauv.freeze_batchnorm on both sides (the oracle's BatchNorms then run in eval mode, on
    calibrated running statistics): dx meets the bar, and item 0's dx does not change when items
    1..3 are replaced — the per-item property mauv.attribution documents."""
    from mauv import freeze_batchnorm
    from mauv.engine import root_state
    batch = make_batches(SEED_DATA, 1, B=B, S_opt=64, S_son=64)[0]
    other = make_batches(SEED_DATA + 5, 1, B=B, S_opt=64, S_son=64)[0]
    inputs, y = [batch[k] for k in KEYS], batch["label"]
    o, m_cpu = calibrated_pair(batch)
    assert freeze_batchnorm(o) == 159
    store = _record_eps(o, m_cpu, inputs)
    o32 = _oracle_dx(o, store, inputs, y)
    o64 = _oracle_dx(o, store, inputs, y, torch.float64)
    m = to_gpu(m_cpu)
    assert freeze_batchnorm(m) == 159
    m.train()
    for p in m.parameters():
        p.requires_grad_(False)
    root_state(m).eps_provider = provider(store, m)
    xs, _ = _hip_step(m, inputs, y)
    _assert_bar("frozen BatchNorm", [x.grad for x in xs], o32, o64)
    assert all(p.grad is None for p in m.parameters())
    mixed = [torch.cat([a[:1], b[1:]]) for a, b in zip(inputs, (other[k] for k in KEYS))]
    ys = torch.cat([y[:1], other["label"][1:]])
    xm, _ = _hip_step(m, mixed, ys)
    for i, (a, b) in enumerate(zip(xs, xm)):
        d = (a.grad[0] - b.grad[0]).abs().max().item()
        print(f"item 0, input {i}: max |dx - dx(other items replaced)| = {d:.3e}")
        assert torch.equal(a.grad[0], b.grad[0])
        assert not torch.equal(a.grad[1], b.grad[1])


def _cos(a, b):
    a, b = a.double().flatten().cpu(), b.double().flatten().cpu()
    return float(a @ b / (a.norm() * b.norm() + 1e-300))


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_16bit_trunks(tri, dt):
    """bf16 / f16 trunks (set_precision): dx is finite and non-zero, fp32 NCHW like the input.
    bf16: its cosine with the float64 dx is at least that of the oracle under torch.autocast on
    the GPU, less 0.1 (tests/test_parity16_gpu.py's random-init margin: trunk gradients at random
    init are conditioning-dominated)."""
    from mauv.engine import set_precision
    m = _model(tri)
    set_precision(m, dt)
    xs, _ = _hip_step(m, tri["inputs"], tri["y"])
    for x in xs:
        assert x.grad is not None and x.grad.dtype == torch.float32 and x.grad.shape == x.shape
        assert torch.isfinite(x.grad).all().item() and x.grad.abs().max().item() > 0
    if dt == torch.bfloat16:
        oac = _oracle_dx(tri["o"], tri["store"], tri["inputs"], tri["y"], device="cuda", amp=dt)
        for i, (x, a, t) in enumerate(zip(xs, oac, tri["o64"])):
            hip, ac = _cos(x.grad, t), _cos(a, t)
            print(f"bf16 input {i}: cosine with fp64 dx: HIP {hip:.4f}, torch.autocast {ac:.4f}")
            assert hip >= ac - 0.1, (i, hip, ac)


def test_input_gradients_helper_and_shares(tri):
    """input_gradients(..., "predicted") equals the hand-written autograd expression on the same
    MC samples; it writes no parameter gradient; modality_shares rows sum to 1."""
    from mauv import input_gradients, modality_shares
    m = _model(tri)
    xs = [t.cuda().requires_grad_(True) for t in tri["inputs"]]
    mean = m.mc_forward(*xs, N).mean(0)
    want = torch.autograd.grad(mean.gather(1, mean.argmax(1, keepdim=True)).sum(), xs)
    for p in m.parameters():
        p.grad = None
    grads, logits = input_gradients(m, tuple(tri["inputs"]), N, "predicted")
    assert logits.shape == (N, B, 7) and not logits.requires_grad
    assert all(p.grad is None and p.requires_grad for p in m.parameters())
    for i, (g, w) in enumerate(zip(grads, want)):
        print(f"input {i}: max |helper - autograd| = {(g - w).abs().max().item():.3e}")
        assert torch.equal(g, w)
    s = modality_shares(grads)
    assert s.shape == (B, 3) and bool((s > 0).all())
    assert torch.allclose(s.sum(1), torch.ones(B, device=s.device), atol=1e-6)
    ge, _ = input_gradients(m, tuple(tri["inputs"]), N, "entropy")
    gc, _ = input_gradients(m, tri["inputs"], N, lambda lg: lg.mean(0)[:, 0].sum())
    assert all(torch.isfinite(g).all().item() and g.abs().max().item() > 0 for g in ge + gc)
    with pytest.raises(ValueError, match="score"):
        input_gradients(m, tuple(tri["inputs"]), N, "nope")


def test_fgsm_moves_by_eps_and_does_not_lower_the_loss():
    """On a fitted model, with the same MC samples before and after: every element moves by
    exactly +eps, -eps or 0 (inputs on a 1/256 grid, eps = 1/64: the sums are exact in fp32) and
    the loss does not go down."""
    from mauv import fgsm
    from mauv.engine import root_state
    _, m = build_pair()
    g = torch.Generator().manual_seed(21)
    xs = [(torch.randint(0, 256, (B, c, 64, 64), generator=g) / 256.0).cuda() for c in (3, 3, 1)]
    y = torch.randint(0, 7, (B,), generator=g).cuda()
    fit_model(m, *xs, y, steps=20)
    crit, eps, st = torch.nn.CrossEntropyLoss(), 1.0 / 64, root_state(m)

    def loss_at(inp):
        st.offset = 1000   # the same MC samples every time
        with torch.no_grad():
            return crit(m.mc_forward(*inp, N).mean(0), y).item()

    before = loss_at(xs)
    st.offset = 1000
    adv = fgsm(m, tuple(xs), y, crit, eps, N)
    moved = 0
    for a, x in zip(adv, xs):
        d = a - x
        assert a.shape == x.shape and not a.requires_grad
        assert bool(((d == eps) | (d == -eps) | (d == 0)).all())
        moved += int((d != 0).sum())
    assert moved > 0
    after = loss_at(adv)
    print(f"fgsm eps = 1/64: CE {before:.5f} -> {after:.5f}")
    assert after >= before
