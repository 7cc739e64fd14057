"""The weight EMA in the gated Adam step, timed two ways on one MI355X.

  step    the fp32 training step of bench.py's configs[1] shape (B = 64, num_mc = 5, 224 / 256 px)
          through mauv.train.mc_train_step with FusedAdam(lr=5e-5), EMA off or `--ema DECAY`:
          `--warmup` steps, then `--rounds` rounds of `--steps` steps each between two HIP events
          (one synchronisation per round), ms per step of every round, median and spread.
  launch  HIP events around the Adam launch alone over the tri-modal parameter set (696 tensors,
          146.8 M floats, one plain group), by DESIGN.md §2.35's procedure: the gated
          `mauv_adam_step_ex` and, where the library has it, `mauv_adam_step_ex_ema` with a shadow
          per row.

One process measures one arm; alternate the processes on one box.  The parent commit's library
takes the place of this one through MAUV_LIB (EMA off only):

    python tools/ema_step_ab.py step                          # this library, EMA off
    python tools/ema_step_ab.py step --ema 0.999              # this library, EMA on
    MAUV_LIB=/path/to/parent/libmauv_hip.so python tools/ema_step_ab.py step
    python tools/ema_step_ab.py launch
    rocprofv3 --kernel-trace --stats -- python tools/ema_step_ab.py step --ema 0.999 --rounds 1
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

from bench import synthetic_batch  # noqa: E402
from mauv import ops  # noqa: E402
from mauv._lib import lib, check, MauvAdamGroup, LIB_PATH  # noqa: E402
from mauv.models import define_models, DEFAULT_PRIOR  # noqa: E402
from mauv.optim import FusedAdam, GATE_WORDS, G_OK_LOSS  # noqa: E402


def step_arm(a):
    from mauv.train import mc_train_step
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = define_models(None, 7, DEFAULT_PRIOR)["multimodal_model"].to(dev)
    opt = FusedAdam(model.parameters(), lr=5e-5, **({} if a.ema is None else {"ema_decay": a.ema}))
    crit = torch.nn.CrossEntropyLoss()
    x, b, s, y = synthetic_batch(64, 224, 256, dev, 1234)
    kl_w = 2.0 ** 1 / 2.0 ** 30

    def step():
        return mc_train_step(model, (x, b, s), y, crit, opt, 5, 64, kl_w)

    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            r = step()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / a.steps)
    assert bool(r["stepped"])
    arm = "ema off" if a.ema is None else f"ema {a.ema}"
    print(f"step [{arm}] library {LIB_PATH}: ms/step per round of {a.steps}: "
          + " ".join(f"{v:.2f}" for v in ms)
          + f"  median {statistics.median(ms):.2f}  min {min(ms):.2f}  max {max(ms):.2f}",
          flush=True)
    if a.ema is not None:
        print(f"  ema updates {opt.ema_updates} over {a.warmup + a.rounds * a.steps} steps",
              flush=True)


def launch_arm(a):
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
            (("p", 0.1), ("g", 1e-3), ("m", 1e-4), ("v", 1e-3), ("e", 0.1))}
    bufs["v"].abs_()
    rows = np.zeros((len(numels), 7), dtype=np.int64)
    for i, (n, o) in enumerate(zip(numels, offs)):
        rows[i] = [bufs[k].data_ptr() + 4 * o for k in ("p", "g", "m", "v")] + [0, n, 0]
    tab = torch.from_numpy(rows).to(dev)
    shadows = torch.from_numpy(np.array([bufs["e"].data_ptr() + 4 * o for o in offs],
                                        dtype=np.int64)).to(dev)
    arr = (MauvAdamGroup * 1)()
    arr[0].lr, arr[0].beta1, arr[0].beta2, arr[0].eps = 5e-5, 0.9, 0.999, 1e-8
    gate = torch.zeros(GATE_WORDS, dtype=torch.int32, device=dev)
    gate[G_OK_LOSS] = 1
    ema = torch.zeros(8, dtype=torch.int32, device=dev)
    ema[:1].view(torch.float32).fill_(0.999)
    has_ema = hasattr(ctypes.CDLL(LIB_PATH), "mauv_adam_step_ex_ema")

    def gated_ex():
        check(lib.mauv_adam_step_ex(tab.data_ptr(), len(numels), ctypes.addressof(arr), 1, 0,
                                    gate.data_ptr(), ops.stream()), "adam_step_ex")

    def gated_ema():
        check(lib.mauv_adam_step_ex_ema(tab.data_ptr(), len(numels), ctypes.addressof(arr), 1,
                                        gate.data_ptr(), None, None, shadows.data_ptr(),
                                        ema.data_ptr(), ops.stream()), "adam_step_ex_ema")

    print(f"launch: library {LIB_PATH}: {len(numels)} tensors, {sum(numels)} floats", flush=True)
    for name, fn in (("gated_ex", gated_ex),) + ((("gated_ema", gated_ema),) if has_ema else ()):
        ms = []
        for r in range(a.warmup + a.reps):
            bufs["g"].normal_(0, 1e-3)      # the launch zeroes the gradients: refill them
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if r >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        print(f"  {name:10s} median {statistics.median(ms):.3f} ms  min {min(ms):.3f} ms  "
              f"max {max(ms):.3f} ms  ({a.reps} launches)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["step", "launch"])
    ap.add_argument("--ema", type=float, default=None, help="ema_decay of the step arm")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    (step_arm if a.what == "step" else launch_arm)(a)


if __name__ == "__main__":
    main()
