"""Gradient accumulation over two gloo ranks on CPU (the style of tests/test_ddp_cpu.py): with
K=2 over 4 micro-batches ``DistributedMC`` exchanges the gradient arena once per window, not once
per micro-batch, the trunk-ready hook issues nothing while a window is open, and the arena at each
close is the mean over ranks of the summed micro-batch gradients."""
import os

import torch
import torch.distributed as dist

from tests.test_ddp_cpu import _init, _run

K, MICRO = 2, 4


class Tri(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.f = torch.nn.Linear(12, 3)

    def forward(self, x, b, s):
        return self.f(torch.cat([x, b, s], 1))


class KeepGrads(torch.optim.SGD):
    """zero_grad() zeroes in place: the gradients stay the views of the arena."""

    def zero_grad(self, set_to_none=False):
        super().zero_grad(False)


def _accum_worker(rank, world, port, q):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "multimodal-auv_amd")]
    _init(rank, world, port)
    from mauv.ddp import DistributedMC
    from mauv.engine import root_state
    from mauv.train import mc_train_step
    torch.manual_seed(0)
    net = Tri()
    ddp = DistributedMC(net, bucket_bytes=64)     # 16 floats a bucket: several per exchange
    st = root_state(net)
    arena = st.grads(torch.device("cpu"))
    views = [p.grad for p in net.parameters()]
    opt = KeepGrads(net.parameters(), lr=0.1)
    opt.grad_accumulation = K
    crit = torch.nn.CrossEntropyLoss()
    snaps, reduce = [], ddp.allreduce_grads

    def exchange():
        reduce()
        snaps.append(arena.flat.clone())
    ddp.allreduce_grads = exchange
    g = torch.Generator().manual_seed(100 + rank)      # every rank its own micro-batches
    y = torch.tensor([0, 1, 2, 0])
    sums, counts, quiet = [], [], []
    for i in range(MICRO):
        xs = tuple(torch.randn(4, 4, generator=g) for _ in range(3))
        w = [p.detach().clone().requires_grad_() for p in net.parameters()]
        out = torch.nn.functional.linear(torch.cat(xs, 1), w[0], w[1])
        grads = torch.autograd.grad(torch.nn.functional.cross_entropy(out, y), w)
        if i % K == 0:
            sums.append([gr.clone() for gr in grads])
        else:
            sums[-1] = [a + gr for a, gr in zip(sums[-1], grads)]
        r = mc_train_step(ddp, xs, y, crit, opt, 1, 4, 0.5)
        assert r["closed"] is (i % K == K - 1) and r["stepped"] is r["closed"]
        counts.append((ddp.n_buckets, ddp.elems_reduced))
        if not r["closed"]:
            # the engine's hook on an open window: nothing is issued
            st.kl_bwd_count += 1
            st.grad_ready_hook(net.f)
            quiet.append(ddp.window_open and not ddp._done and not ddp._pending
                         and ddp.n_buckets == counts[-1][0])
    same_views = all(p.grad is v for p, v in zip(net.parameters(), views))
    torch.save((snaps, sums, counts, quiet, arena.flat.numel(), same_views,
                [p.detach().clone() for p in net.parameters()]),
               os.path.join(q, f"r{rank}.pt"))
    dist.destroy_process_group()


def test_one_arena_exchange_per_window_of_summed_gradients(tmp_path):
    res = _run(_accum_worker, tmp_path)
    numel = res[0][4]
    assert numel == 36 + 4                       # 3 x 12 weights, 3 biases padded to 4
    per = -(-numel // 16)                        # buckets of one arena exchange
    for snaps, _, counts, quiet, n, same_views, _ in res:
        assert n == numel and same_views and quiet == [True, True]
        assert len(snaps) == MICRO // K          # allreduce_grads ran at the closes only
        assert counts == [(0, 0), (per, numel), (per, numel), (2 * per, 2 * numel)]
    for w in range(MICRO // K):
        a, b = res[0][0][w], res[1][0][w]
        assert torch.equal(a, b)                 # every rank holds the same arena
        s0, s1 = res[0][1][w], res[1][1][w]
        # weights [0:36], bias [36:39], one float of padding that stays zero
        want = torch.cat([((x + y) * 0.5).reshape(-1) for x, y in zip(s0, s1)] +
                         [torch.zeros(1)])
        assert torch.equal(a, want), w
    for p, q in zip(res[0][6], res[1][6]):
        assert torch.equal(p, q)                 # and takes the same steps
