"""Float64 statement and fp32 restatement of mauv_adam_step_ex's element (csrc/adam.hip
adam_elem_ex): torch's single-tensor Adam with amsgrad / maximize / decoupled weight decay.  The
error measure and the bar are tests/kernel_ref.py's (units of 2^-24 of a scale; the kernel may
err MARGIN x what the one-fp32-operation-per-kernel-operation restatement errs, floored at 1).

Scales: m and v as kernel_ref.adam64; p by |p| + |lr wd p| + |update| (the decoupled decay is a
term of its own); max_exp_avg_sq by its own float64 value.
"""
import numpy as np

from tests import kernel_ref as R

F32 = np.float32
AMSGRAD, MAXIMIZE, DECOUPLED = 1, 2, 4


def consts(lr, beta1, beta2, eps, wd, t, flags):
    """kernel_ref.adam_consts plus what the options need, from the fp32 arguments."""
    k = R.adam_consts(lr, beta1, beta2, eps, wd, t)
    k.update(lr=float(F32(lr)), flags=int(flags))
    return k


def adam64(p, g, m, v, x, k):
    """One step in float64 from fp32 p, g, m, v, x (x = max_exp_avg_sq, ignored without
    amsgrad): ((new, unit scale) of p, m, v, x); x's pair is None without amsgrad."""
    p, g, m, v = (a.astype(np.float64) for a in (p, g, m, v))
    omb1, omb2 = 1.0 - k["b1"], 1.0 - k["b2"]
    f, wd = k["flags"], k["wd"]
    if f & MAXIMIZE:
        g = -g
    ge, pd, decay_term = g, p, np.zeros_like(p)
    if wd != 0:
        if f & DECOUPLED:
            pd = p * (1.0 - k["lr"] * wd)
            decay_term = np.abs(k["lr"] * wd * p)
        else:
            ge = g + wd * p
    m1 = m + omb1 * (ge - m)
    v1 = v * k["b2"] + omb2 * ge * ge
    x1 = np.maximum(x.astype(np.float64), v1) if f & AMSGRAD else None
    d = x1 if f & AMSGRAD else v1
    upd = k["step_size"] * (m1 / (np.sqrt(d) / k["bc2_sqrt"] + k["eps"]))
    return ((pd - upd, np.abs(p) + decay_term + np.abs(upd)),
            (m1, np.abs(m) + omb1 * (np.abs(ge) + np.abs(m))),
            (v1, np.abs(v1)),
            (x1, np.abs(x1)) if f & AMSGRAD else None)


def adam32(p, g, m, v, x, k):
    """adam_elem_ex, one fp32 rounding per operation (step_size, bc2_sqrt and the decay factor
    rounded from double as the library rounds them): (p, m, v, x or None)."""
    b2, eps, wd = F32(k["b2"]), F32(k["eps"]), F32(k["wd"])
    omb1, omb2 = F32(1.0) - F32(k["b1"]), F32(1.0) - b2
    ss, bs = F32(k["step_size"]), F32(k["bc2_sqrt"])
    decay = F32(1.0 - k["lr"] * k["wd"])
    f = k["flags"]
    if f & MAXIMIZE:
        g = -g
    ge = g
    if wd != 0:
        if f & DECOUPLED:
            p = p * decay
        else:
            ge = g + wd * p
    m1 = m + omb1 * (ge - m)
    v1 = v * b2 + omb2 * ge * ge
    x1 = np.maximum(x, v1) if f & AMSGRAD else None
    d = x1 if f & AMSGRAD else v1
    p1 = p - ss * (m1 / (np.sqrt(d) / bs + eps))
    assert p1.dtype == np.float32 and m1.dtype == np.float32 and v1.dtype == np.float32
    assert x1 is None or x1.dtype == np.float32
    return p1, m1, v1, x1
