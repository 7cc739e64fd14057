"""Frozen BatchNorm on the 16-bit trunks (bf16 and f16 storage, 64 px).

* One training step (B = 3, N = 2, running statistics calibrated on the batch,
  tests/frozen_helpers.py) against the frozen fp32 oracle at SURVEY §8c's bf16 row as
  tests/test_model16_gpu.py asserts it — logits |d| <= 5e-2 max(1, |ref|), loss within 5e-2
  relative — once with every block boundary that fits folded into the next conv1
  (engine.FOLD_MIN_TILES = 0: the folded block output meets a frozen bn3, whose backward reads
  the fold's mask bits) and once with engine.FOLD off: bit-identical logits and gradients, as
  tests/test_fold_gpu.py requires of the live path.
* The f16 predictor (B = 4, N = 8) on a model fitted by helpers.fit_model and then frozen:
  every item's class is the frozen fp32 oracle's, and aleatoric / predictive entropy deviate from
  it by at most max(1e-2, 1.25 x torch-autocast's own worst item), torch-autocast being the
  oracle frozen the same way under torch.autocast on the GPU with the same weights and epsilons —
  the yardstick and ratio of tests/test_parity16_gpu.py.  Both schemes' deviations are printed
  (-rP)."""
import pytest
import torch
import torch.nn.functional as F

from oracle import bayes_ref, loops_ref
from tests.golden.common import make_batches, SEED_DATA
from tests.helpers import build_pair, EpsBridge, oracle_replay, fit_model
from tests.frozen_helpers import batchnorms, calibrated_pair, to_gpu, provider, bn_buffers, changed
from tests.test_fold_gpu import _train_step
from tests.test_parity16_gpu import ENTROPY_BAR, WORST_RATIO

pytestmark = pytest.mark.gpu
DTS = [torch.bfloat16, torch.float16]
B, N = 3, 2


def _cuda(*ts):
    return [t.cuda() for t in ts]


@pytest.fixture(scope="module")
def ref():
    """The calibrated pair and one step of the frozen fp32 oracle, computed once."""
    from mauv import freeze_batchnorm
    batch = make_batches(SEED_DATA, 1, B=B, S_opt=64, S_son=64)[0]
    x, b, s, y = batch["main_image"], batch["bathy_image"], batch["sss_image"], batch["label"]
    o, m_cpu = calibrated_pair(batch)
    assert freeze_batchnorm(o) == 159
    bridge = EpsBridge(o, m_cpu, 99)
    with bridge, torch.no_grad():
        logits = torch.stack([o(x, b, s) for _ in range(N)])
        loss = F.cross_entropy(logits.mean(0), y) + bayes_ref.get_kl_loss(o) / B * 0.5
    bridge.collect()
    return dict(batch=batch, m_cpu=m_cpu, logits=logits, loss=loss, store=bridge.store)


@pytest.mark.parametrize("dt", DTS, ids=["bf16", "f16"])
def test_frozen_train_step16(ref, dt, monkeypatch):
    from mauv import engine, ops, mchead, freeze_batchnorm
    from mauv.kl import get_kl_loss
    m = to_gpu(ref["m_cpu"])
    assert freeze_batchnorm(m) == 159
    engine.set_precision(m, dt)
    engine.root_state(m).eps_provider = provider(ref["store"], m)
    m.train()
    snap = bn_buffers(m)
    x, b, s, y = _cuda(*(ref["batch"][k] for k in ("main_image", "bathy_image", "sss_image",
                                                    "label")))
    ran = []
    real = ops.conv2d_fwd_fold
    monkeypatch.setattr(ops, "conv2d_fwd_fold", lambda *a, **k: ran.append(real(*a, **k)) or ran[-1])
    monkeypatch.setattr(engine, "FOLD_MIN_TILES", 0)
    monkeypatch.setattr(engine, "FOLD", True)
    lg1, g1 = _train_step(m, x, b, s, y, N)
    assert any(ran), "no block boundary folded: the folded output never met a frozen bn3"
    monkeypatch.setattr(engine, "FOLD", False)
    lg0, g0 = _train_step(m, x, b, s, y, N)
    assert torch.equal(lg0, lg1)
    bad = [n for n in g0 if not torch.equal(g0[n], g1[n])]
    assert not bad, bad[:5]
    assert all(bool(torch.isfinite(g).all()) for g in g0.values())
    assert sum(bool(g.any()) for g in g0.values()) > 600
    assert not changed(m, snap)
    o_logits = ref["logits"]
    d = (lg0.double().cpu() - o_logits.double()).abs().max().item()
    ce, _, _ = mchead.mc_mean_ce(lg0, y)
    loss = (ce + get_kl_loss(m) / B * 0.5).item()
    print(f"{dt}: max |dlogit| {d:.3e} (|ref| <= {o_logits.abs().max().item():.3f}), loss {loss:.6f} "
          f"vs {ref['loss'].item():.6f}")
    assert d <= 5e-2 * max(1.0, o_logits.abs().max().item()), d
    assert abs(loss - ref["loss"].item()) <= 5e-2 * abs(ref["loss"].item())


def test_frozen_predictor_f16_vs_torch_autocast():
    from mauv import freeze_batchnorm
    from mauv.engine import root_state
    from mauv.predict import mc_statistics
    Bp, Np = 4, 8
    o, m = build_pair()
    batch = make_batches(SEED_DATA + 1, 1, B=Bp, S_opt=64, S_son=64)[0]
    x, b, s = batch["main_image"], batch["bathy_image"], batch["sss_image"]
    labels = torch.randint(0, 7, (Bp,), generator=torch.Generator().manual_seed(3))
    fit_model(m, *_cuda(x, b, s), labels.cuda())
    o.load_state_dict({k: v.cpu() for k, v in m.state_dict().items()})
    assert min(bn.running_var.min().item() for bn in batchnorms(o)) > 0
    assert freeze_batchnorm(o) == 159 and freeze_batchnorm(m) == 159
    snap = bn_buffers(m)
    bridge = EpsBridge(o, m, 7)
    with bridge:
        pred32, var32, alea32, P32 = loops_ref.predict_batch(o, x, b, s, Np)   # frozen fp32 oracle
    bridge.collect()

    def ac(mm):
        assert all(not bn.training for bn in batchnorms(mm))
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            lg = torch.stack([mm(*_cuda(x, b, s)) for _ in range(Np)])
        P = torch.softmax(lg.float(), -1)
        return tuple(t.cpu() for t in loops_ref.mc_uncertainty_from_probs(P)) + (P.cpu(),)
    _, (pred_ac, var_ac, alea_ac, P_ac) = oracle_replay(o, bridge.store, ac, device="cuda")
    root_state(m).eps_provider = bridge.provider
    m.train()
    with torch.no_grad(), torch.autocast("cuda"):
        st = mc_statistics(m, *_cuda(x, b, s), Np, chunk=Np)
    assert not changed(m, snap)

    def pent(P):
        pm = P.double().mean(0)
        return -(pm * torch.log(pm + 1e-8)).sum(-1)
    pe32 = pent(P32)
    dev = dict(da_h=(st["aleatoric"].double().cpu() - alea32.double()).abs(),
               da_a=(alea_ac.double() - alea32.double()).abs(),
               dp_h=(st["predictive_entropy"].double().cpu() - pe32).abs(),
               dp_a=(pent(P_ac) - pe32).abs())
    print(f"\nfrozen f16 predictor 64 px B={Bp} N={Np}: classes fp32 {pred32.tolist()} HIP "
          f"{st['pred'].cpu().tolist()} torch-autocast {pred_ac.tolist()}")
    for k, name in (("da", "aleatoric"), ("dp", "pred. entropy")):
        h, a = dev[k + "_h"], dev[k + "_a"]
        print(f"  {name:13s} |d| vs frozen fp32 oracle max/mean: HIP {h.max():.3e}/{h.mean():.3e}  "
              f"torch-autocast {a.max():.3e}/{a.mean():.3e}")
    assert torch.equal(st["pred"].cpu(), pred32)
    for k in ("da", "dp"):
        lim = max(ENTROPY_BAR, WORST_RATIO * dev[k + "_a"].max().item())
        assert dev[k + "_h"].max().item() <= lim, (k, dev[k + "_h"].max().item(), lim)
