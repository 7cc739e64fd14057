"""HIP-event time of the gated all-groups Adam launch over the tri-modal parameter set (696 tensors,
146.8 M floats, one plain group), by DESIGN.md §2.35's procedure: 5 warm-up and 20 timed
repetitions, HIP events around each launch, median and minimum.

  gated_ex     mauv_adam_step_ex with a gate: the launch every gated step with options, groups
               or a loss scaler takes (decision kernel + Adam kernel, mode 3 every time)
  accum_close  mauv_adam_step_ex_accum closing a window of three micro-batches: the same two
               launches, the gradient multiplied by 1 / 3 as it is loaded

Run it once per library and alternate the runs on one box; a library from before the
accumulation entry (MAUV_LIB=...) runs `gated_ex` alone.

    python tools/accum_close_ab.py [--warmup 5] [--reps 20]
    MAUV_LIB=/path/to/older/libmauv_hip.so python tools/accum_close_ab.py
"""
import argparse
import ctypes
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "multimodal-auv_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from mauv import ops  # noqa: E402
from mauv._lib import lib, check, MauvAdamGroup, LIB_PATH  # noqa: E402
from mauv.models import define_models, DEFAULT_PRIOR  # noqa: E402
from mauv.optim import GATE_WORDS, G_OK_LOSS  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = define_models(None, 7, DEFAULT_PRIOR)["multimodal_model"]
    numels = [p.numel() for p in model.parameters()]
    del model
    offs, off = [], 0
    for n in numels:
        offs.append(off)
        off += (n + 3) // 4 * 4
    bufs = {k: torch.randn(off, device=dev) * s for k, s in
            (("p", 0.1), ("g", 1e-3), ("m", 1e-4), ("v", 1e-3))}
    bufs["v"].abs_()
    rows = np.zeros((len(numels), 7), dtype=np.int64)
    for i, (n, o) in enumerate(zip(numels, offs)):
        rows[i] = [bufs[k].data_ptr() + 4 * o for k in ("p", "g", "m", "v")] + [0, n, 0]
    tab = torch.from_numpy(rows).to(dev)
    arr = (MauvAdamGroup * 1)()
    arr[0].lr, arr[0].beta1, arr[0].beta2, arr[0].eps = 5e-5, 0.9, 0.999, 1e-8
    gate = torch.zeros(GATE_WORDS, dtype=torch.int32, device=dev)
    gate[G_OK_LOSS] = 1
    acc = torch.zeros(8, dtype=torch.int32, device=dev)
    has_accum = hasattr(ctypes.CDLL(LIB_PATH), "mauv_adam_step_ex_accum")

    def gated_ex():
        check(lib.mauv_adam_step_ex(tab.data_ptr(), len(numels), ctypes.addressof(arr), 1, 0,
                                    gate.data_ptr(), ops.stream()), "adam_step_ex")

    def accum_close():
        check(lib.mauv_adam_step_ex_accum(tab.data_ptr(), len(numels), ctypes.addressof(arr), 1,
                                          gate.data_ptr(), None, acc.data_ptr(), ops.stream()),
              "adam_step_ex_accum")

    print(f"library {LIB_PATH}: {len(numels)} tensors, {sum(numels)} floats", flush=True)
    for name, fn in (("gated_ex", gated_ex),) + ((("accum_close", accum_close),) if has_accum
                                                  else ()):
        ms = []
        for r in range(a.warmup + a.reps):
            bufs["g"].normal_(0, 1e-3)      # the launch zeroes the gradients: refill them
            acc[0] = 2                      # two micro-batches noted: a close is the third
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if r >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        print(f"{name:12s} median {statistics.median(ms):.3f} ms  min {min(ms):.3f} ms  "
              f"max {max(ms):.3f} ms  ({a.reps} launches)", flush=True)


if __name__ == "__main__":
    main()
