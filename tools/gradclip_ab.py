"""A/B of global-norm gradient clipping on the bench's training step (B = 64, num_mc = 5,
224 / 256 px; fp32 and bf16 trunks), three arms interleaved in one process, each run `--repeats`
times with `--warmup` warm-up and `--steps` timed steps (wall clock over a device synchronise):

  off     mc_train_step + FusedAdam, no clipping: the baseline
  fused   FusedAdam(max_grad_norm=c) through the gated mc_train_step: the norm rides on the
          non-finite scan, the Adam kernel multiplies as it loads
  torch   option off; a hand-written loop with torch.nn.utils.clip_grad_norm_ between the
          backward and an ungated FusedAdam.step(): what clipping cost before the option

c is half the norm of a first probing step, so every clipped step really clips.  Also prints the
HIP-event time of the fused scan (mauv_grad_norm) beside mauv_nonfinite_count over the arena.

    python tools/gradclip_ab.py [--dtypes fp32 bf16] [--repeats 3] [--warmup 5] [--steps 20]
"""
import argparse
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "multimodal-auv_amd")]
import torch  # noqa: E402

import bench  # noqa: E402
from mauv import ops  # noqa: E402
from mauv.engine import root_state, set_precision  # noqa: E402
from mauv.models import define_models, DEFAULT_PRIOR  # noqa: E402
from mauv.optim import FusedAdam  # noqa: E402
from mauv.train import mc_loss, mc_train_step  # noqa: E402

ARMS = ("off", "fused", "torch")


def scan_times(flat, reps=20):
    """ms per launch (HIP events over `reps` launches) of the two scans over the arena."""
    dev = flat.device
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    norm = torch.zeros(1, device=dev)
    spans = ops.span_table([(flat.data_ptr(), flat.numel())], dev)
    ws = torch.empty(ops.grad_norm_workspace_bytes(1), dtype=torch.uint8, device=dev)
    out = {}
    for name, fn in (("nonfinite_count", lambda: ops.nonfinite_count(flat, cnt)),
                     ("grad_norm", lambda: ops.grad_norm(spans, 0, ws, norm, cnt))):
        for _ in range(3):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out[name] = e0.elapsed_time(e1) / reps
    return out


def run(dtype, a):
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = define_models(None, 7, DEFAULT_PRIOR)["multimodal_model"].to(dev)
    opt = FusedAdam(model.parameters(), lr=5e-5)
    crit = torch.nn.CrossEntropyLoss()
    B = 64
    x, b, s, y = bench.synthetic_batch(B, 224, 256, dev, 1234)
    set_precision(model, torch.bfloat16 if dtype == "bf16" else None)
    kl_w = 2.0 ** 1 / 2.0 ** 30
    params = list(model.parameters())

    def gated():
        return mc_train_step(model, (x, b, s), y, crit, opt, 5, B, kl_w)

    opt.max_grad_norm = 1e30          # probe: reads the norm, clips nothing
    first = float(gated()["grad_norm"])
    c = first / 2
    print(f"[{dtype}] first step's gradient norm {first:.6g}: max_grad_norm = {c:.6g}", flush=True)

    def hand_written():
        loss = mc_loss(model, (x, b, s), y, crit, 5, B, kl_w)[0]
        if not torch.isfinite(loss):
            return
        loss.backward()
        torch.nn.utils.clip_grad_norm_(params, c)
        opt.step()
        opt.zero_grad()

    def arm(name):
        opt.max_grad_norm = c if name == "fused" else None
        return hand_written if name == "torch" else gated

    res = {k: [] for k in ARMS}
    for r in range(a.repeats):
        for name in ARMS[r % 3:] + ARMS[:r % 3]:      # rotate the order between repeats
            fn = arm(name)
            for _ in range(a.warmup):
                fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                fn()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) / a.steps * 1e3
            res[name].append(ms)
            print(f"[{dtype}] repeat {r} {name:5s}: {ms:.2f} ms/step", flush=True)
    opt.max_grad_norm = None
    mean = {k: sum(v) / len(v) for k, v in res.items()}
    for k in ARMS:
        print(f"[{dtype}] {k:5s}: " + " ".join(f"{v:.2f}" for v in res[k]) +
              f"  mean {mean[k]:.2f} ms/step")
    lo, hi = min(res["off"]), max(res["off"])
    print(f"[{dtype}] fused mean {mean['fused']:.2f} vs off's spread [{lo:.2f}, {hi:.2f}]: "
          f"{'inside' if lo <= mean['fused'] <= hi else 'OUTSIDE'}; "
          f"torch - off = {mean['torch'] - mean['off']:+.2f} ms, "
          f"fused - off = {mean['fused'] - mean['off']:+.2f} ms")
    flat = root_state(model).arena.flat
    st = scan_times(flat)
    print(f"[{dtype}] arena {flat.numel()} floats: nonfinite_count {st['nonfinite_count']:.3f} ms, "
          f"grad_norm (scan + finalize) {st['grad_norm']:.3f} ms per launch", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtypes", nargs="+", default=["fp32", "bf16"], choices=["fp32", "bf16"])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    for dtype in a.dtypes:
        run(dtype, a)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
