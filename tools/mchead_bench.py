"""Many-class MC head timing: the fused kernels (mauv_mc_stats + mauv_mc_finalize; mauv_mc_mean_ce
+ mauv_mc_mean_bwd through mauv.mchead's autograd op) against the reference's own torch maths on
the same GPU tensors.

  statistics leg  softmax -> var(0).mean(1), per-sample entropy (eps 1e-7), mean probability,
                  argmax (inference/predictors.py:65-84) at G = 100, B = 256
  training leg    mean(0) -> F.cross_entropy -> autograd backward (train/multimodal.py:121-138)
                  at G = 5, B = 64

Both arms run in one process, alternated in rounds (ROUNDS x ITERS >= 200 iterations per arm),
each round between two device events after a warm-up of every shape.  The rate printed is
ALGORITHMIC bytes (4 G B C of logits read once plus every output written once) over the median
per-iteration time, and its share of the HBM bandwidth a float4 copy reaches (6.29 TB/s).

    python tools/mchead_bench.py [--out profiles/mchead_bench.txt]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "multimodal-auv_amd")]
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from mauv import mchead  # noqa: E402

HBM_COPY_BW = 6.29e12   # bytes/s, measured float4 copy on an MI355X
ROUNDS, ITERS, WARMUP = 10, 20, 5
CLASSES = (64, 1000, 4096)


def stats_arms(G, B, C):
    lg = 4.0 * torch.randn(G, B, C, device="cuda")

    def fused():
        return mchead.mc_finalize(mchead.mc_stats(lg, 1e-7), G, C, 1e-8)

    def chain():
        P = torch.softmax(lg, dim=2)
        var = torch.var(P, dim=0).mean(dim=1)
        alea = torch.mean(-torch.sum(P * torch.log(P + 1e-7), dim=-1), dim=0)
        mp = P.mean(0)
        return mp, var, alea, torch.argmax(mp, dim=1)

    nbytes = 4 * G * B * C + 8 * B * (2 * C + 1) + 4 * B * C + 3 * 4 * B + 8 * B
    return fused, chain, nbytes


def train_arms(G, B, C):
    lg = (4.0 * torch.randn(G, B, C, device="cuda")).requires_grad_(True)
    y = torch.randint(0, C, (B,), device="cuda")

    def fused():
        lg.grad = None
        loss, _, _ = mchead.mc_mean_ce(lg, y)
        loss.backward()
        return lg.grad

    def chain():
        lg.grad = None
        loss = F.cross_entropy(lg.mean(0), y)
        loss.backward()
        return lg.grad

    nbytes = 4 * G * B * C + 4 * B * C + 4 + 8 * B + 4 * G * B * C
    return fused, chain, nbytes


def train_kernel_arm(G, B, C):
    """The training leg's three launches alone (mauv.ops, outputs allocated once): what the
    kernels take without the Python autograd.Function around them."""
    from mauv import ops
    lg = 4.0 * torch.randn(G, B, C, device="cuda")
    y = torch.randint(0, C, (B,), device="cuda")
    mean, loss = torch.empty(B, C, device="cuda"), torch.empty(1, device="cuda")
    pred = torch.empty(B, dtype=torch.int64, device="cuda")
    one, dl = torch.ones(1, device="cuda"), torch.empty(G, B, C, device="cuda")

    def kernels():
        ops.mc_mean_ce(lg, y, G, B, C, mean, loss, pred)
        ops.mc_mean_bwd(None, one, mean, y, G, B, C, dl)
        return dl

    return kernels


def time_arms(arms):
    """Median per-iteration milliseconds of each arm, the arms alternated round by round."""
    for fn in arms:
        for _ in range(WARMUP):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in arms]
    for _ in range(ROUNDS):
        for i, fn in enumerate(arms):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(ITERS):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[i].append(e0.elapsed_time(e1) / ITERS)
    return [(statistics.median(t), min(t), max(t)) for t in times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "mchead_bench needs a ROCm GPU"
    lines = [f"# {torch.cuda.get_device_name(0)}; {ROUNDS} rounds x {ITERS} iterations per arm, "
             f"median (min .. max) ms per iteration"]
    for leg, G, B, make in (("stats", 100, 256, stats_arms), ("train", 5, 64, train_arms)):
        for C in CLASSES:
            fused, chain, nbytes = make(G, B, C)
            arms = [fused, chain] + ([train_kernel_arm(G, B, C)] if leg == "train" else [])
            (tf, fmin, fmax), (tc, cmin, cmax), *rest = time_arms(arms)
            rate = nbytes / (tf * 1e-3)
            rec = dict(leg=leg, G=G, B=B, C=C, fused_ms=round(tf, 5), torch_ms=round(tc, 5),
                       fused_over_torch=round(tf / tc, 4), algorithmic_bytes=nbytes,
                       fused_GBps=round(rate / 1e9, 1), hbm_share=round(rate / HBM_COPY_BW, 4),
                       fused_ms_range=[round(fmin, 5), round(fmax, 5)],
                       torch_ms_range=[round(cmin, 5), round(cmax, 5)])
            if rest:   # the launches alone, next to the autograd op the loops call
                rec.update(kernels_ms=round(rest[0][0], 5),
                           kernels_over_torch=round(rest[0][0] / tc, 4),
                           kernels_GBps=round(nbytes / (rest[0][0] * 1e-3) / 1e9, 1))
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
            del fused, chain
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
