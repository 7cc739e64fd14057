"""Measurements of the stems' data gradient, in one process on one GPU.

Kernels (HIP events over `--launches` launches, `--repeats` repeats of each arm, interleaved):
B = 64, G = 5, 224 and 256 px, C = 3 and 1, fp32 and bf16 operands.

  new      ops.stem_bwd_rows + ops.stem_col2im: one GEMM over (g, co) into fp32 rows, then the
           gather into the fp32 NCHW gradient
  generic  what the library's earlier entry points assemble: ops.conv2d_bwd_data of the 7x7 / 2
           conv for the G samples (one launch per output-parity class, G on the grid; the input
           channels padded to 4 fp32 / 8 16-bit as every conv of the trunks), then the sum over
           the samples and the NHWC -> fp32 NCHW conversion in torch

Step (wall clock over a device synchronise, `--steps` timed steps after `--warmup`): the bench's
fp32 training step (B = 64, num_mc = 5, 224 / 256 px) with and without the three inputs requiring
grad, interleaved, `--repeats` times.

    python tools/stem_dgrad_bench.py [--repeats 3] [--launches 10] [--steps 5] [--warmup 2]
                                     [--no-kernels] [--no-step]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "multimodal-auv_amd")]
import torch  # noqa: E402

import bench  # noqa: E402
from mauv import ops  # noqa: E402
from mauv.models import define_models, DEFAULT_PRIOR  # noqa: E402
from mauv.optim import FusedAdam  # noqa: E402
from mauv.train import mc_train_step  # noqa: E402

DT = {"fp32": torch.float32, "bf16": torch.bfloat16}
B, G, COUT, R, ST, PD = 64, 5, 64, 7, 2, 3


def _time(fn, launches):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches


def kernel_arms(dt, S, C):
    """(new, generic) closures on the same dy and weights, and a check that they agree."""
    K = C * R * R
    Kp = ops.stem_kp(dt, K)
    Ho = ops.out_hw(S, R, ST, PD)
    M = B * Ho * Ho
    cp = (C + 3) // 4 * 4 if dt == torch.float32 else (C + 7) // 8 * 8
    g = torch.Generator(device="cuda").manual_seed(S + C)
    dy = torch.randn(G, M, COUT, device="cuda", generator=g).to(dt)
    w4 = 0.05 * torch.randn(G, COUT, C, R, R, device="cuda", generator=g)
    w = torch.zeros(G, COUT, Kp, device="cuda")
    w[:, :, :K] = w4.reshape(G, COUT, K)
    w = w.to(dt)
    wk = torch.zeros(G, COUT, R, R, cp, device="cuda")        # KRSC, padded input channels
    wk[..., :C] = w4.permute(0, 1, 3, 4, 2)
    wk = wk.to(dt).contiguous()
    drows = torch.empty(M, Kp, device="cuda")
    dx = torch.empty(B, C, S, S, device="cuda")
    dxg = torch.empty(G, B, S, S, cp, device="cuda", dtype=dt)
    out = {}

    def new():
        ops.stem_bwd_rows(dy, w, drows, G, M, Kp, COUT, K)
        ops.stem_col2im(drows, B, C, S, S, R, ST, PD, Kp, dx)

    def generic():
        ops.conv2d_bwd_data(dy, wk, dxg, G, B, S, S, cp, COUT, R, ST, PD)
        out["dx"] = dxg[..., :C].float().sum(0).permute(0, 3, 1, 2).contiguous()

    new()
    try:
        generic()
    except Exception as e:   # a shape the earlier entry points refuse: reported, not timed
        print(f"generic route refused ({dt}, {S} px, C = {C}): {e}", flush=True)
        return new, None, float("nan"), 4.0 * M * Kp * 2
    torch.cuda.synchronize()
    d = (dx - out["dx"]).abs().max().item() / out["dx"].abs().max().item()
    nbytes = 4.0 * M * Kp * 2    # the staged rows: one write and one read
    return new, generic, d, nbytes


def run_kernels(args):
    rows = []
    for name, dt in DT.items():
        for S in (224, 256):
            for C in (3, 1):
                new, generic, d, nbytes = kernel_arms(dt, S, C)
                tn, tg = [], []
                for _ in range(args.repeats):
                    tn.append(_time(new, args.launches))
                    if generic is not None:
                        tg.append(_time(generic, args.launches))
                row = dict(dtype=name, px=S, C=C, new_ms=[round(t, 4) for t in tn],
                           generic_ms=[round(t, 4) for t in tg],
                           ratio_generic_over_new=round(min(tg) / min(tn), 3) if tg else None,
                           max_rel_diff=float(f"{d:.3e}"),
                           staged_rows_gbytes=round(nbytes / 1e9, 3))
                rows.append(row)
                print(json.dumps(row), flush=True)
                del new, generic
                torch.cuda.empty_cache()
    return rows


def run_step(args):
    dev = torch.device("cuda")
    x, b, s, y = bench.synthetic_batch(B, 224, 256, dev, 1234)
    crit = torch.nn.CrossEntropyLoss()
    kl_w = 2.0 ** 1 / 2.0 ** 30
    torch.manual_seed(0)
    model = define_models(None, 7, DEFAULT_PRIOR)["multimodal_model"].to(dev)
    opt = FusedAdam(model.parameters(), lr=5e-5)

    def steps(n, want):
        xs = tuple(t.detach().requires_grad_(want) for t in (x, b, s))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            mc_train_step(model, xs, y, crit, opt, G, B, kl_w)
            if want:
                assert all(t.grad is not None for t in xs)
                for t in xs:
                    t.grad = None
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    steps(args.warmup, False)
    steps(args.warmup, True)
    res = {"plain_ms": [], "input_grad_ms": []}
    for _ in range(args.repeats):
        res["plain_ms"].append(round(steps(args.steps, False), 2))
        res["input_grad_ms"].append(round(steps(args.steps, True), 2))
    res["ratio"] = round(min(res["input_grad_ms"]) / min(res["plain_ms"]), 4)
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    if not args.no_kernels:
        run_kernels(args)
    if not args.no_step:
        run_step(args)


if __name__ == "__main__":
    main()
