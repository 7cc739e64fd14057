"""Float64 statement and fp32 restatement of the KL kernels (csrc/reparam.hip mauv_kl_fwd /
mauv_kl_bwd) and of the fused Adam update (csrc/adam.hip), with the error measure the kernel
tests share: |got - ref64| in units of 2^-24 of a condition-aware scale (the sum of the absolute
values of the terms, so a cancelling result such as -1/s + s/sp^2 near s = sp is not judged
against itself).

The bar of a kernel is not a constant: each test runs the fp32 restatement below — the same
formula on the CPU, one fp32 operation per kernel operation — measures its error against
float64 in the same units, and allows the kernel 4x that figure (floored at 1 unit).  The factor
covers the device's expf / log1pf / logf against the host's and FMA contraction; it is the
margin tests.helpers.NORMAL_BAR gives the normals.

Valid for rho in [-80, 60]: below about -87 expf(rho) is denormal and the formula itself (kernel
and restatement alike) loses its relative accuracy.
"""
import numpy as np

F32 = np.float32
U = 2.0 ** -24
MARGIN = 4.0


def bar(restated_units):
    return MARGIN * max(1.0, float(restated_units))


def units(got, ref, scale):
    """max |got - ref| / (2^-24 scale) elementwise (float64 arrays or scalars)."""
    got, ref, scale = (np.asarray(a, dtype=np.float64) for a in (got, ref, scale))
    assert np.isfinite(got).all() and np.isfinite(ref).all() and (scale > 0).all()
    return float((np.abs(got - ref) / (U * scale)).max())


# ------------------------------------------------------------------------------------- KL
def kl_terms64(mu, rho, pm, ps):
    """(term, sum |terms|) of one entry, elementwise, float64 from the fp32 inputs."""
    mu, rho = mu.astype(np.float64), rho.astype(np.float64)
    pm, ps = float(F32(pm)), float(F32(ps))
    s = np.log1p(np.exp(rho))
    d = mu - pm
    q = (s * s + d * d) / (2.0 * ps * ps)
    return np.log(ps) - np.log(s) + q - 0.5, abs(np.log(ps)) + np.abs(np.log(s)) + q + 0.5


def kl_terms32(mu, rho, pm, ps):
    """kl_partial_kernel's element, one fp32 rounding per operation."""
    pm, ps = F32(pm), F32(ps)
    lsp = np.log(ps)
    inv2 = F32(1.0) / (F32(2.0) * ps * ps)
    s = np.log1p(np.exp(rho))
    d = mu - pm
    t = lsp - np.log(s) + (s * s + d * d) * inv2 - F32(0.5)
    assert t.dtype == np.float32
    return t


def kl_fwd64(entries, scale):
    """(out, unit scale) of a table: entries = [(mu, rho, prior_mu, prior_sigma)] fp32 arrays."""
    out = mag = 0.0
    for mu, rho, pm, ps in entries:
        t, a = kl_terms64(mu, rho, pm, ps)
        out += t.mean()
        mag += a.mean()
    sc = float(F32(scale))
    return out * sc, abs(sc) * mag


def kl_fwd32(entries, scale):
    """The kernels' reduction: fp32 elements summed in double, one mean per entry, the sum
    times the fp32 scale rounded to fp32."""
    acc = 0.0
    for mu, rho, pm, ps in entries:
        acc += kl_terms32(mu, rho, pm, ps).astype(np.float64).sum() / mu.size
    return float(F32(acc * float(F32(scale))))


def kl_bwd64(mu, rho, pm, ps, g_mu, g_rho, coef, scale):
    """((dmu, its unit scale), (drho, its unit scale)) after the kernel added into g_mu / g_rho."""
    mu, rho = mu.astype(np.float64), rho.astype(np.float64)
    g_mu, g_rho = g_mu.astype(np.float64), g_rho.astype(np.float64)
    pm, ps = float(F32(pm)), float(F32(ps))
    c = float(F32(coef)) * float(F32(scale)) / mu.size
    s = np.log1p(np.exp(rho))
    sg = 1.0 / (1.0 + np.exp(-rho))
    d = mu - pm
    dmu = g_mu + c * d / (ps * ps)
    drho = g_rho + c * (-1.0 / s + s / (ps * ps)) * sg
    return ((dmu, np.abs(g_mu) + abs(c) * np.abs(d) / (ps * ps)),
            (drho, np.abs(g_rho) + abs(c) * (1.0 / s + s / (ps * ps)) * sg))


def kl_bwd32(mu, rho, pm, ps, g_mu, g_rho, coef, scale):
    """kl_bwd_kernel's element, one fp32 rounding per operation."""
    pm, ps = F32(pm), F32(ps)
    c = F32(coef) * F32(scale) / F32(mu.size)
    inv_sp2 = F32(1.0) / (ps * ps)
    s = np.log1p(np.exp(rho))
    sg = F32(1.0) / (F32(1.0) + np.exp(-rho))
    dmu = g_mu + c * (mu - pm) * inv_sp2
    drho = g_rho + c * (F32(-1.0) / s + s * inv_sp2) * sg
    assert dmu.dtype == np.float32 and drho.dtype == np.float32
    return dmu, drho


def pack_prior(pm, ps):
    """The (prior_mu, prior_sigma) floats of a MauvKlEntry as the int64 KLTable._build stores."""
    return int(np.array([pm, ps], dtype=np.float32).view(np.int64)[0])


# ----------------------------------------------------------------------------------- Adam
def adam_consts(lr, beta1, beta2, eps, wd, t):
    """The constants as the library forms them from its fp32 arguments (adam.hip)."""
    lr, b1, b2, eps, wd = (float(F32(v)) for v in (lr, beta1, beta2, eps, wd))
    bc1 = 1.0 - b1 ** t
    bc2 = 1.0 - b2 ** t
    return dict(b1=b1, b2=b2, eps=eps, wd=wd, step_size=lr / bc1, bc2_sqrt=np.sqrt(bc2))


def adam64(p, g, m, v, k):
    """One torch.optim.Adam step in float64 from fp32 p, g, m, v: ((new, unit scale) of p, m, v)."""
    p, g, m, v = (a.astype(np.float64) for a in (p, g, m, v))
    omb1, omb2 = 1.0 - k["b1"], 1.0 - k["b2"]
    ge = g + k["wd"] * p
    m1 = m + omb1 * (ge - m)
    v1 = v * k["b2"] + omb2 * ge * ge
    upd = k["step_size"] * (m1 / (np.sqrt(v1) / k["bc2_sqrt"] + k["eps"]))
    return ((p - upd, np.abs(p) + np.abs(upd)),
            (m1, np.abs(m) + omb1 * (np.abs(ge) + np.abs(m))),
            (v1, np.abs(v1)))


def adam32(p, g, m, v, k):
    """adam_elem, one fp32 rounding per operation (step_size, bc2_sqrt rounded as the host does)."""
    b2, eps, wd = F32(k["b2"]), F32(k["eps"]), F32(k["wd"])
    omb1, omb2 = F32(1.0) - F32(k["b1"]), F32(1.0) - b2
    ss, bs = F32(k["step_size"]), F32(k["bc2_sqrt"])
    ge = g + wd * p if wd != 0 else g
    m1 = m + omb1 * (ge - m)
    v1 = v * b2 + omb2 * ge * ge
    p1 = p - ss * (m1 / (np.sqrt(v1) / bs + eps))
    assert p1.dtype == np.float32 and m1.dtype == np.float32 and v1.dtype == np.float32
    return p1, m1, v1
