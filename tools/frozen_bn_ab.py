"""A/B of frozen BatchNorm, in one process on one GPU.

Step time: the bench's training step (B = 64, num_mc = 5, 224 / 256 px; fp32 and bf16 trunks),
three arms interleaved, each run `--repeats` times with `--warmup` warm-up and `--steps` timed
steps (wall clock over a device synchronise):

  live    every BatchNorm on batch statistics: the baseline
  stats   freeze_batchnorm(model): running statistics, gamma / beta trainable
  affine  freeze_batchnorm(model, freeze_affine=True): gamma / beta frozen too

Each arm is a model of its own with the same weights, its running statistics set to the bench
batch's by one momentum-1.0 forward before it is frozen (at (0, 1) a frozen BatchNorm is nearly
the identity), stepped by its own FusedAdam.

Kernel rate (HIP events over `--launches` launches, mask-bit ReLU) on the layer-1 block-output
shape (G = 5, M = 64 * 56 * 56, C = 256) and the layer-4 one (M = 64 * 49, C = 2048):

  apply_rows   bn_bwd_apply_rows: bn_bwd_ex handed one ready partial per channel (its finalize
               over that one partial rides along), the existing kernel the new one is held to
  frozen_rows  bn_bwd_frozen with gamma / beta frozen: the one-pass kernel
  fused        bn_bwd_frozen with dgamma / dbeta: sums and stores in one kernel + finalize
  two_launch   the same result as bn_bwd_ex(dy = dres = None) (the existing partial pass +
               finalize) followed by frozen_rows
  train        the live backward, bn_bwd_ex: partial pass + finalize + apply_rows

with the bytes each moves per element and the resulting TB/s.

    python tools/frozen_bn_ab.py [--dtypes fp32 bf16] [--repeats 3] [--warmup 5] [--steps 20]
                                 [--launches 20] [--no-steps] [--no-kernels]
"""
import argparse
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "multimodal-auv_amd")]
import torch  # noqa: E402

import bench  # noqa: E402
from mauv import ops, freeze_batchnorm  # noqa: E402
from mauv.engine import set_precision  # noqa: E402
from mauv.models import define_models, DEFAULT_PRIOR  # noqa: E402
from mauv.optim import FusedAdam  # noqa: E402
from mauv.train import mc_train_step  # noqa: E402

ARMS = ("live", "stats", "affine")
DT = {"fp32": torch.float32, "bf16": torch.bfloat16}


def _model(dev, x, b, s):
    torch.manual_seed(0)
    m = define_models(None, 7, DEFAULT_PRIOR)["multimodal_model"].to(dev)
    bns = [mod for mod in m.modules() if isinstance(mod, torch.nn.BatchNorm2d)]
    for bn in bns:
        bn.momentum = 1.0
    with torch.no_grad():
        m.mc_forward(x, b, s, 1)
    for bn in bns:
        bn.momentum = 0.1
    return m


def step_times(dtype, a):
    dev = torch.device("cuda", 0)
    B = 64
    x, b, s, y = bench.synthetic_batch(B, 224, 256, dev, 1234)
    crit = torch.nn.CrossEntropyLoss()
    kl_w = 2.0 ** 1 / 2.0 ** 30
    fns = {}
    for name in ARMS:
        m = _model(dev, x, b, s)
        if name != "live":
            freeze_batchnorm(m, freeze_affine=name == "affine")
        set_precision(m, torch.bfloat16 if dtype == "bf16" else None)
        opt = FusedAdam(m.parameters(), lr=5e-5)
        fns[name] = lambda m=m, opt=opt: mc_train_step(m, (x, b, s), y, crit, opt, 5, B, kl_w)
    res = {k: [] for k in ARMS}
    for r in range(a.repeats):
        for name in ARMS[r % 3:] + ARMS[:r % 3]:      # rotate the order between repeats
            fn = fns[name]
            for _ in range(a.warmup):
                out = fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                out = fn()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) / a.steps * 1e3
            res[name].append(ms)
            print(f"[{dtype}] repeat {r} {name:6s}: {ms:.2f} ms/step  (loss {float(out['loss']):.4f}, "
                  f"stepped {bool(out['stepped'])})", flush=True)
    mean = {k: sum(v) / len(v) for k, v in res.items()}
    for k in ARMS:
        print(f"[{dtype}] {k:6s}: " + " ".join(f"{v:.2f}" for v in res[k]) +
              f"  mean {mean[k]:.2f} ms/step, spread [{min(res[k]):.2f}, {max(res[k]):.2f}]")
    print(f"[{dtype}] stats - live = {mean['stats'] - mean['live']:+.2f} ms "
          f"({mean['stats'] / mean['live'] - 1:+.1%}), affine - live = "
          f"{mean['affine'] - mean['live']:+.2f} ms ({mean['affine'] / mean['live'] - 1:+.1%})",
          flush=True)


def _time(fn, launches):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches


def kernel_rates(dtype, G, M, C, launches):
    dev, dt = "cuda", DT[dtype]
    n, e = G * M * C, torch.tensor([], dtype=DT[dtype]).element_size()
    torch.manual_seed(1)
    y = torch.randn(G, M, C, device=dev).to(dt)
    dout = torch.randn(G, M, C, device=dev).to(dt)
    dy = torch.empty_like(y)
    mask = torch.randint(0, 256, (n // 8,), dtype=torch.uint8, device=dev)
    mean, invstd = torch.randn(G, C, device=dev), torch.rand(G, C, device=dev) + 0.5
    scale, shift = torch.randn(G, C, device=dev), torch.randn(G, C, device=dev)
    ws = torch.empty(ops.bn_workspace_floats(G, M, C), device=dev)
    dg, db = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
    one = torch.zeros(2, G, 1, C, device=dev)       # one ready partial per (group, channel)

    def frozen_rows():
        ops.bn_bwd_frozen(None, None, mask, dout, 1, None, None, scale, None, G, M, C, None, dy)

    def partial_only():
        ops.bn_bwd_ex(y, None, mask, dout, 1, mean, invstd, scale, shift, G, M, C, ws, None, None,
                      dg, db)

    arms = {
        "apply_rows": (lambda: ops.bn_bwd_ex(y, None, mask, dout, 1, mean, invstd, scale, shift,
                                             G, M, C, ws, dy, pre=(one[0], one[1], 1)),
                       3 * e + 0.125),
        "frozen_rows": (frozen_rows, 2 * e + 0.125),
        "fused": (lambda: ops.bn_bwd_frozen(y, None, mask, dout, 1, mean, invstd, scale, shift, G,
                                            M, C, ws, dy, None, dg, db), 3 * e + 0.125),
        "two_launch": (lambda: (partial_only(), frozen_rows()), 4 * e + 0.25),
        "train": (lambda: ops.bn_bwd_ex(y, None, mask, dout, 1, mean, invstd, scale, shift, G, M,
                                        C, ws, dy, None, dg, db), 5 * e + 0.25),
    }
    t = {}
    for name, (fn, bpe) in arms.items():
        t[name] = _time(fn, launches)
        print(f"[{dtype} G={G} M={M} C={C}] {name:11s}: {t[name]:.3f} ms, {bpe:.3f} B/element, "
              f"{bpe * n / t[name] / 1e9:.2f} TB/s", flush=True)
    r = (arms["frozen_rows"][1] / t["frozen_rows"]) / (arms["apply_rows"][1] / t["apply_rows"])
    print(f"[{dtype} G={G} M={M} C={C}] frozen_rows / apply_rows: {r:.2f}x the TB/s, "
          f"{t['apply_rows'] / t['frozen_rows']:.2f}x faster; fused vs two_launch: "
          f"{t['fused']:.3f} vs {t['two_launch']:.3f} ms", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtypes", nargs="+", default=["fp32", "bf16"], choices=["fp32", "bf16"])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--no-steps", action="store_true")
    ap.add_argument("--no-kernels", action="store_true")
    a = ap.parse_args()
    for dtype in a.dtypes:
        if not a.no_kernels:
            for M, C in ((64 * 56 * 56, 256), (64 * 49, 2048)):
                kernel_rates(dtype, 5, M, C, a.launches)
                torch.cuda.empty_cache()
        if not a.no_steps:
            step_times(dtype, a)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
