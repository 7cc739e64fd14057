"""mauv_kl_fwd / mauv_kl_bwd (csrc/reparam.hip) on hand-built tables against float64, and
get_kl_loss on a tiny two-layer model against oracle.bayes_ref in float64 — with some of the
parameters frozen too (a frozen tensor's gradient pointer is null and the backward skips it).

Measure and bars: tests/kernel_ref.py — units of 2^-24 of the sum of the absolute terms; the
kernel may err 4x what the fp32 restatement of the same formula errs on the same inputs (floored
at 1 unit).  The forward is judged as a whole (the restated reduction errs 0.6 to 2.2 units, so
its bar is 4 to 8.6 units; one element missed in an entry of 20000 among 70 entries moves the
result by more), the backward elementwise.

Measured on an MI355X, worst over all cases (fp32 restatement on the same inputs; bar):
  forward out     2.24 units at unit prior / MOPED rho (restatement 0.69; bar 4.0); where the
                  restatement is worst, 2.16 (narrow prior / wide rho), the kernel errs 2.16
  backward dmu    3.59 units (restatement 4.35; bar 17.4)
  backward drho   5.33 units (restatement 5.45; bar 21.8)
  get_kl_loss, two layers   1.49 units (restatement 1.49; bar 6.0); its gradients 4.20 units
                  at worst (rho_weight of the MOPED layer; restatement 6.12; bar 24.5)
"""
import numpy as np
import pytest
import torch

from tests import kernel_ref as R

pytestmark = pytest.mark.gpu

dev = "cuda"
SIZES = [1, 3, 255, 256, 257, 8191, 8192, 8193, 20000]   # 8192 = one sweep of 32 blocks x 256
PRIORS = {"unit": [(0.0, 1.0)], "narrow": [(0.3, 0.1)], "tight": [(-0.05, 0.02)],
          "mixed": [(0.0, 1.0), (0.3, 0.1), (-0.05, 0.02), (0.7, 2.5)]}
RHOS = {"init": (-6.0, 0.0), "moped": (-46.0, -3.0), "wide": (-46.0, 20.0)}
GAP = 3   # untouched floats between two entries of a flat buffer (odd: entries at any offset)


class Table:
    """n entries laid out in flat device buffers (mu, rho, dmu, drho) with GAP floats between
    them, and the [n, 6] int64 rows KLTable._build makes."""

    def __init__(self, sizes, priors, rho_range, seed):
        rng = np.random.default_rng(seed)
        self.sizes = sizes
        self.priors = [priors[i % len(priors)] for i in range(len(sizes))]
        self.offs = np.cumsum([GAP] + [s + GAP for s in sizes])[:-1]
        total = int(self.offs[-1] + sizes[-1] + GAP)
        self.mu = rng.standard_normal(total).astype(np.float32)
        self.rho = rng.uniform(rho_range[0], rho_range[1], total).astype(np.float32)
        for o, s, (pm, _) in zip(self.offs, sizes, self.priors):
            self.mu[o:o + s] = np.float32(pm) + np.float32(0.1) * self.mu[o:o + s]
        self.g_mu = rng.standard_normal(total).astype(np.float32)    # the kernel adds into these
        self.g_rho = rng.standard_normal(total).astype(np.float32)
        self.d_mu, self.d_rho = torch.tensor(self.mu, device=dev), torch.tensor(self.rho, device=dev)

    def entries(self):
        return [(self.mu[o:o + s], self.rho[o:o + s], pm, ps)
                for o, s, (pm, ps) in zip(self.offs, self.sizes, self.priors)]

    def rows(self, dmu=None, drho=None, null=()):
        """null: {(entry, column)} whose gradient pointer is 0 (column 2 = dmu, 3 = drho)."""
        rows = np.zeros((len(self.sizes), 6), dtype=np.int64)
        for i, (o, s, (pm, ps)) in enumerate(zip(self.offs, self.sizes, self.priors)):
            rows[i, 0] = self.d_mu.data_ptr() + 4 * int(o)
            rows[i, 1] = self.d_rho.data_ptr() + 4 * int(o)
            if dmu is not None:
                rows[i, 2] = 0 if (i, 2) in null else dmu.data_ptr() + 4 * int(o)
                rows[i, 3] = 0 if (i, 3) in null else drho.data_ptr() + 4 * int(o)
            rows[i, 4] = s
            rows[i, 5] = R.pack_prior(pm, ps)
        return torch.tensor(rows, device=dev)


def _tables(priors, rho_range, seed):
    """n = 1 (every size), n = 3 (three tables covering every size), n = 70 (the sizes cycled:
    the finalize's lanes take a second entry each)."""
    out = [[s] for s in SIZES] + [SIZES[i:i + 3] for i in (0, 3, 6)]
    out.append([SIZES[i % len(SIZES)] for i in range(70)])
    return [Table(sz, priors, rho_range, seed + k) for k, sz in enumerate(out)]


def _fwd(tab, scale):
    from mauv import ops
    n = len(tab.sizes)
    ws = torch.full((n * 32,), float("nan"), dtype=torch.float64, device=dev)  # fully rewritten
    out = torch.full((1,), float("nan"), device=dev)
    ops.kl_fwd(tab.rows(), n, ws, out, scale=scale)
    return out.cpu().numpy()[0]


@pytest.mark.parametrize("rho", list(RHOS))
@pytest.mark.parametrize("prior", list(PRIORS))
def test_kl_fwd_tables(prior, rho):
    from mauv._lib import lib
    worst = rest = 0.0
    for tab in _tables(PRIORS[prior], RHOS[rho], 100):
        n = len(tab.sizes)
        assert lib.mauv_kl_workspace_bytes(n) == n * 32 * 8
        for scale in (1.0, 0.37):
            got = _fwd(tab, scale)
            assert got.tobytes() == _fwd(tab, scale).tobytes(), "two calls differ"
            ref, mag = R.kl_fwd64(tab.entries(), scale)
            r = R.units(R.kl_fwd32(tab.entries(), scale), ref, mag)
            u = R.units(got, ref, mag)
            worst, rest = max(worst, u), max(rest, r)
            assert u <= R.bar(r), (n, tab.sizes[:3], scale, u, r)
    print(f"kl_fwd {prior}/{rho}: kernel {worst:.2f} units, fp32 restatement {rest:.2f}")


def _bwd_check(tab, coef, scale, null=()):
    """One mauv_kl_bwd over tab: live entries against float64, null halves and the floats
    between entries bit-unchanged.  Returns (dmu units, drho units, restated dmu, restated drho)."""
    from mauv import ops
    dmu, drho = torch.tensor(tab.g_mu, device=dev), torch.tensor(tab.g_rho, device=dev)
    cdev = None if coef is None else torch.tensor([coef], device=dev)
    ops.kl_bwd(tab.rows(dmu, drho, null), len(tab.sizes), cdev, scale=scale)
    dmu, drho = dmu.cpu().numpy(), drho.cpu().numpy()
    c = 1.0 if coef is None else coef
    live = np.zeros((2, dmu.size), dtype=bool)
    fig = np.zeros(4)
    for i, ((mu, rho, pm, ps), o, s) in enumerate(zip(tab.entries(), tab.offs, tab.sizes)):
        sl = slice(o, o + s)
        ref = R.kl_bwd64(mu, rho, pm, ps, tab.g_mu[sl], tab.g_rho[sl], c, scale)
        r32 = R.kl_bwd32(mu, rho, pm, ps, tab.g_mu[sl], tab.g_rho[sl], c, scale)
        for j, got in enumerate((dmu, drho)):
            if (i, 2 + j) in null:
                continue
            live[j, sl] = True
            fig[j] = max(fig[j], R.units(got[sl], *ref[j]))
            fig[2 + j] = max(fig[2 + j], R.units(r32[j], *ref[j]))
    for j, (got, g0) in enumerate(((dmu, tab.g_mu), (drho, tab.g_rho))):
        assert np.array_equal(got[~live[j]].view(np.int32), g0[~live[j]].view(np.int32)), \
            "a float outside the live entries changed"
    assert fig[0] <= R.bar(fig[2]) and fig[1] <= R.bar(fig[3]), (tab.sizes[:3], coef, scale, fig)
    return fig


@pytest.mark.parametrize("rho", list(RHOS))
@pytest.mark.parametrize("prior", list(PRIORS))
def test_kl_bwd_tables(prior, rho):
    worst = np.zeros(4)
    for tab in _tables(PRIORS[prior], RHOS[rho], 200):
        for coef, scale in ((0.73, 0.37), (None, 1.0), (-1.9, 1.0)):
            worst = np.maximum(worst, _bwd_check(tab, coef, scale))
    print(f"kl_bwd {prior}/{rho}: dmu {worst[0]:.2f} units (fp32 restatement {worst[2]:.2f}), "
          f"drho {worst[1]:.2f} (restatement {worst[3]:.2f})")


def test_kl_bwd_frozen_entries():
    """Null gradient pointers: entry 1 of 3 frozen as a whole, then only its mu, then only its
    rho — the live halves come out as in test_kl_bwd_tables, nothing else is written."""
    tab = Table([257, 8193, 3], PRIORS["mixed"], RHOS["wide"], 300)
    for null in ({(1, 2), (1, 3)}, {(1, 2)}, {(1, 3)}):
        fig = _bwd_check(tab, 0.73, 0.37, null=null)
        print(f"kl_bwd null {sorted(null)}: dmu {fig[0]:.2f} units, drho {fig[1]:.2f}")


# ---------------------------------------------------------------------------- model level
def _tiny_pair(seed=7):
    """Two LinearReparameterization layers with different priors (no trunk): the mauv model on
    the GPU and oracle.bayes_ref's in float64 on the same fp32 parameters; layer 0 MOPED-like."""
    from mauv.layers import LinearReparameterization as Lin
    from oracle.bayes_ref import LinearReparameterization as RefLin
    torch.manual_seed(seed)
    priors = [(0.3, 0.1), (-0.05, 0.02)]
    shapes = [(37, 300), (300, 5)]
    m = torch.nn.Sequential(*[Lin(i, o, prior_mean=pm, prior_variance=ps)
                              for (i, o), (pm, ps) in zip(shapes, priors)])
    with torch.no_grad():
        for lin, (pm, _) in zip(m, priors):
            lin.mu_weight.add_(pm)
            lin.mu_bias.add_(pm)
        m[0].rho_weight.uniform_(-46.0, -3.0)
        m[1].rho_bias.uniform_(-46.0, 20.0)
    o = torch.nn.Sequential(*[RefLin(i, o_, prior_mean=pm, prior_variance=ps)
                              for (i, o_), (pm, ps) in zip(shapes, priors)])
    o.load_state_dict(m.state_dict())
    # .double() after construction: the prior buffers hold fp32(prior), as the kernel's table does
    return m.to(dev), o.double(), priors


def _model_entries(m, priors):
    out = []
    for lin, (pm, ps) in zip(m, priors):
        for mu, rho in ((lin.mu_weight, lin.rho_weight), (lin.mu_bias, lin.rho_bias)):
            out.append((mu, rho, mu.detach().cpu().numpy().ravel(),
                        rho.detach().cpu().numpy().ravel(), pm, ps))
    return out


def _check_model_grads(m, o, priors, coef, layers):
    """.grad of the listed layers of m against the oracle's float64 gradients."""
    ref_params = dict(o.named_parameters())
    names = {id(p): n for n, p in m.named_parameters()}
    for mu_p, rho_p, mu, rho, pm, ps in _model_entries(m, priors):
        if int(names[id(mu_p)].split(".")[0]) not in layers:
            continue
        z = np.zeros_like(mu)
        r64 = R.kl_bwd64(mu, rho, pm, ps, z, z, coef, 1.0)
        r32 = R.kl_bwd32(mu, rho, pm, ps, z, z, coef, 1.0)
        for j, p in enumerate((mu_p, rho_p)):
            orc = ref_params[names[id(p)]].grad.numpy().ravel()
            # the restated float64 formula is the oracle's autograd (to float64 rounding)
            assert R.units(r64[j][0], orc, r64[j][1]) < 1e-3
            u = R.units(p.grad.cpu().numpy().ravel(), orc, r64[j][1])
            r = R.units(r32[j], orc, r64[j][1])
            print(f"  {names[id(p)]}: {u:.2f} units (fp32 restatement {r:.2f})")
            assert u <= R.bar(r), (names[id(p)], u, r)


def test_kl_model_two_priors():
    from mauv.kl import get_kl_loss
    from oracle import bayes_ref
    m, o, priors = _tiny_pair()
    ent = [e[2:] for e in _model_entries(m, priors)]
    kl, ref = get_kl_loss(m), bayes_ref.get_kl_loss(o)
    ref64, mag = R.kl_fwd64(ent, 1.0)
    assert R.units(ref64, ref.item(), mag) < 1e-3
    u = R.units(kl.item(), ref.item(), mag)
    r = R.units(R.kl_fwd32(ent, 1.0), ref.item(), mag)
    print(f"get_kl_loss: {u:.2f} units (fp32 restatement {r:.2f})")
    assert u <= R.bar(r), (u, r)
    (kl * 0.5).backward()
    (ref * 0.5).backward()
    _check_model_grads(m, o, priors, 0.5, layers=(0, 1))


def test_kl_model_frozen_layer():
    """Layer 0 frozen: its .grad stays None (its table row carries null pointers), layer 1's
    gradients equal the oracle's."""
    from mauv.kl import get_kl_loss
    from oracle import bayes_ref
    m, o, priors = _tiny_pair(seed=8)
    m[0].requires_grad_(False)
    kl, ref = get_kl_loss(m), bayes_ref.get_kl_loss(o)
    kl.backward()
    ref.backward()
    torch.cuda.synchronize()
    assert all(p.grad is None for p in m[0].parameters())
    _check_model_grads(m, o, priors, 1.0, layers=(1,))
    # only mu frozen in a layer: drho still arrives
    m2, o2, priors = _tiny_pair(seed=9)
    m2[1].mu_weight.requires_grad_(False)
    get_kl_loss(m2).backward()
    bayes_ref.get_kl_loss(o2).backward()
    assert m2[1].mu_weight.grad is None
    g = m2[1].rho_weight.grad.cpu().numpy().ravel()
    e = [x for x in _model_entries(m2, priors) if x[1] is m2[1].rho_weight][0]
    z = np.zeros_like(e[2])
    r64 = R.kl_bwd64(e[2], e[3], e[4], e[5], z, z, 1.0, 1.0)[1]
    r32 = R.kl_bwd32(e[2], e[3], e[4], e[5], z, z, 1.0, 1.0)[1]
    orc = o2[1].rho_weight.grad.numpy().ravel()
    assert R.units(g, orc, r64[1]) <= R.bar(R.units(r32, orc, r64[1]))
