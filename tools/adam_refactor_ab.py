"""FusedAdam end to end, bit for bit, for comparing two commits.

Seeded scenarios drive ``FusedAdam.step()`` and ``step_gated`` through the public API only: one
plain group, two groups and amsgrad; clipping off, L2 and inf; a static and a dynamic loss scaler
with an overflow and with growth at the interval; ``grad_accumulation=3`` with a clean and a
dropped window; ``ema_decay`` with and without warm-up; bad losses and non-finite gradients on the
gated form.  Each scenario runs 6 steps on tensors of 5, 8, 1027 and 70001 elements and prints one
SHA-256 over p after every step and, at the end, p, the gradients, exp_avg, exp_avg_sq,
max_exp_avg_sq, the shadows, the gate, scaler, window and EMA words, the last gradient norm and
``state_dict()["state"][*]["step"]``.

Run it once per commit on one box and compare the outputs line by line:

    python tools/adam_refactor_ab.py                     # this tree and its library
    python tools/adam_refactor_ab.py --tree /path/to/parent/checkout
"""
import argparse
import hashlib
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                help="the checkout whose mauv package (and built library) is driven")
ARGS = ap.parse_args()
sys.path[:0] = [ARGS.tree, os.path.join(ARGS.tree, "multimodal-auv_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import mauv.optim as O  # noqa: E402
from mauv._lib import LIB_PATH  # noqa: E402
from mauv.amp import LossScaler  # noqa: E402

NUMELS = (5, 8, 1027, 70001)
STEPS = 6
dev = torch.device("cuda", 0)


def make_opt(route, **kw):
    rng = np.random.default_rng(11)
    ps = [torch.tensor(rng.standard_normal(n).astype(np.float32), device=dev, requires_grad=True)
          for n in NUMELS]
    if route == "two":
        groups = [dict(params=ps[:2], lr=1e-3, weight_decay=1e-2),
                  dict(params=ps[2:], lr=3e-4, betas=(0.8, 0.99), eps=1e-6)]
        return ps, O.FusedAdam(groups, **kw)
    return ps, O.FusedAdam(ps, lr=1e-3, weight_decay=1e-2, amsgrad=route == "ams", **kw)


def grads_of(step, scale=1.0, poison=False):
    rng = np.random.default_rng(1000 + step)
    gs = [(rng.standard_normal(n) * 1e-2 * scale).astype(np.float32) for n in NUMELS]
    if poison:
        gs[2][[0, 1026]] = np.inf, np.nan
    return [torch.tensor(g, device=dev) for g in gs]


def raw(t):
    return t.detach().contiguous().cpu().numpy().tobytes()


def run(name, route, gated, kw, bad_loss=(), poison=(), scale=1.0):
    """``bad_loss`` / ``poison``: the steps whose loss is non-finite (gated form) / whose
    gradients hold inf and NaN; ``scale``: what the gradients are multiplied by, as a backward on
    loss * scale would (an initial scale; a dynamic scaler then moves away from it)."""
    ps, opt = make_opt(route, **kw)
    h = hashlib.sha256()
    for p in ps:
        p.grad = torch.zeros_like(p)
    gate = None
    if gated:
        gate = opt.gate(ps, dev)
        assert gate is not None, name
    for t in range(STEPS):
        for p, g in zip(ps, grads_of(t, scale, t in poison)):
            p.grad.copy_(g)
        if gated:
            gate[O.G_OK_LOSS] = 0 if t in bad_loss else 1
            if opt.closes_window():
                if opt.max_grad_norm is not None:
                    opt.scan_gated(gate)
                else:
                    gate[O.G_NONFINITE] = sum(int((~torch.isfinite(p.grad)).sum()) for p in ps)
            opt.step_gated(gate)
        else:
            opt.step()
        for p in ps:
            h.update(raw(p))
    sd = opt.state_dict()
    for i, p in enumerate(ps):
        st = opt.state.get(p, {})
        for t in [p, p.grad] + [st[k] for k in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq", "ema")
                                if k in st]:
            h.update(raw(t))
        h.update(np.float64(float(sd["state"][i]["step"]) if i in sd["state"] else -1).tobytes())
    ls = opt.loss_scale
    for words in (getattr(opt, "_gate", None), None if ls is None else ls.device_state(dev),
                  getattr(opt, "_accum", None), getattr(opt, "_ema", None), opt.last_grad_norm):
        h.update(b"-" if words is None else raw(words))
    h.update(repr(sd.get("ema_updates")).encode())
    print(f"{name:44s} {h.hexdigest()}", flush=True)
    return h.digest()


def main():
    print(f"# library {os.path.relpath(LIB_PATH, ARGS.tree)}, {STEPS} steps, numel {NUMELS}",
          flush=True)
    total = hashlib.sha256()
    clips = {"noclip": {}, "l2": dict(max_grad_norm=0.05),
             "inf": dict(max_grad_norm=0.01, grad_norm_type=float("inf"))}
    for route in ("plain", "two", "ams"):
        for gated in (False, True):
            form = "gated" if gated else "step"
            events = dict(bad_loss=(1,), poison=(3,)) if gated else {}
            for cn, ckw in clips.items():
                total.update(run(f"{route}/{form}/{cn}", route, gated, ckw, **events))
            static = LossScaler(init_scale=1024.0, dynamic=False)
            total.update(run(f"{route}/{form}/l2/static-scale", route, gated,
                             dict(loss_scale=static, **clips["l2"]), scale=1024.0, poison=(2,)))
            dynamic = LossScaler(init_scale=1024.0, growth_interval=2)
            total.update(run(f"{route}/{form}/noclip/dynamic-scale", route, gated,
                             dict(loss_scale=dynamic), scale=1024.0, poison=(2,),
                             **({"bad_loss": (4,)} if gated else {})))
            for warm in (False, True):
                total.update(run(f"{route}/{form}/noclip/ema{'-warmup' if warm else ''}", route,
                                 gated, dict(ema_decay=0.9, ema_warmup=warm), **events))
        # windows of 3 micro-batches: a clean one, then one dropped for a bad loss
        total.update(run(f"{route}/gated/noclip/accum3", route, True, dict(grad_accumulation=3),
                         bad_loss=(4,)))
        total.update(run(f"{route}/gated/l2/accum3+dynamic-scale+ema", route, True,
                         dict(grad_accumulation=3, ema_decay=0.9, **clips["l2"],
                              loss_scale=LossScaler(init_scale=1024.0, growth_interval=1)),
                         scale=1024.0, bad_loss=(4,)))
    print(f"{'all':44s} {total.hexdigest()}", flush=True)


if __name__ == "__main__":
    main()
