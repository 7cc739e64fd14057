"""mauv.optim.FusedAdam / FusedAdamW with every option torch.optim.Adam takes: amsgrad, maximize,
decoupled weight decay, several parameter groups under a StepLR, a parameter that misses steps,
state_dict interchange, and the drop-in factory handing the caller's options through.

Reference and bar: torch.optim.Adam with the same options in float64 on the CPU, from the same
start and the same gradients.  The error of a run is max |got - ref64| in units of 2^-24
(tests/kernel_ref.py) of a condition-aware scale, taken over all five tensors; FusedAdam may err
MARGIN (4) x what torch's own fp32 CPU Adam errs against the same float64 run (floored at 1
unit).  The scale of a parameter is |p64| plus, for every step of the float64 run, the update
with the first moment replaced by the sum of the absolute values of its terms (A_t = b1 A_t-1 +
(1 - b1)(|g| + wd |p|), so a first moment that cancels is not judged against itself) and the
decoupled decay |lr wd p|; the scale of exp_avg_sq / max_exp_avg_sq is the float64 value itself.

The library's C ABI carries the betas as fp32.  Runs that give all three optimizers betas fp32
holds exactly (BETAS: the defaults rounded) do the same Adam to the last bit of its constants, and
their moments are held to the bar like the parameters.  With betas fp32 does not hold (the
group tests keep torch's defaults) FusedAdam's moments are those of the rounded betas —
exp_avg_sq moves by (fp32(0.999) - 0.999) / (1 - 0.999) = 1.3e-5 of itself — while the
parameters, whose bias correction uses the same rounded betas, stay within the bar: those
runs hold the parameters only.

Measured on an MI355X, FusedAdam units p / v / vmax (torch fp32 CPU Adam; bar = 4x it):
  amsgrad               3.99 / 5.04 / 5.04   (3.99 / 5.39 / 4.57)
  maximize              3.90 / 3.95          (3.90 / 4.77)
  decoupled             7.86 / 4.54          (7.86 / 4.54)
  all three             7.73 / 3.23 / 3.23   (7.73 / 4.54 / 4.54)
  AdamW + amsgrad       7.86 / 4.54 / 4.54   (7.86 / 4.54 / 4.54)
  three groups, StepLR  4.05                 (4.05)
  missed steps          3.60                 (3.60)
"""
import copy

import numpy as np
import pytest
import torch

from tests import kernel_ref as R

pytestmark = pytest.mark.gpu

dev = "cuda"
SHAPES = [(64, 3, 7, 7), (7,), (300, 20), (5, 3), (1,)]   # the last: a view one float into a buffer
STEPS = 5
BETAS = (float(np.float32(0.9)), float(np.float32(0.999)))


def _start(seed):
    g = torch.Generator().manual_seed(seed)
    host = [torch.randn(s, generator=g) for s in SHAPES]
    grads = [[torch.randn(s, generator=g) for s in SHAPES] for _ in range(STEPS)]
    return host, grads


def _gpu_params(host):
    ps = [h.to(dev).requires_grad_(True) for h in host[:-1]]
    buf = torch.zeros(8, device=dev)
    buf[1:2] = host[-1].to(dev)
    view = buf[1:2].detach().requires_grad_(True)
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4
    return ps + [view], buf


def _cpu_params(host, dtype):
    return [h.to(dtype).clone().requires_grad_(True) for h in host]


def _drive(ps, opt, grads, sched=None, skip=(), persistent=False, scale=False):
    """len(grads) steps.  scale: return every parameter's unit scale less |p| (module docstring),
    read from the optimizer's state after each step (the float64 run)."""
    group_of = {id(p): g for g in opt.param_groups for p in g["params"]}
    terms = [torch.zeros_like(p, dtype=torch.float64, device="cpu") for p in ps]
    moved = [torch.zeros_like(a) for a in terms]
    for k, gs in enumerate(grads):
        for i, (p, g) in enumerate(zip(ps, gs)):
            g = g.to(device=p.device, dtype=p.dtype)
            if (k, i) in skip:
                p.grad = None
            elif persistent and p.grad is not None:
                p.grad.copy_(g)
            else:
                p.grad = g.clone()
        before = [p.detach().double().cpu().abs() for p in ps] if scale else None
        opt.step()
        for i, (p, g) in enumerate(zip(ps, gs)):
            if not scale or (k, i) in skip:
                continue
            gr, st = group_of[id(p)], opt.state[p]
            (b1, b2), lr, wd, t = gr["betas"], gr["lr"], gr["weight_decay"], float(st["step"])
            dec = gr.get("decoupled_weight_decay", False)
            terms[i] = b1 * terms[i] + (1 - b1) * (g.double().abs() + (0 if dec else wd) * before[i])
            v = st["max_exp_avg_sq"] if gr["amsgrad"] else st["exp_avg_sq"]
            den = v.detach().double().sqrt() / (1 - b2 ** t) ** 0.5 + gr["eps"]
            moved[i] += lr / (1 - b1 ** t) * terms[i] / den + (lr * wd * before[i] if dec else 0)
        if sched is not None:
            sched.step()
    return moved if scale else None


def _figures(ps, opt, p64, o64, moved, moments):
    """[p, v, vmax] units of a run against the float64 one, over all tensors."""
    fig = [0.0, 0.0, 0.0]
    for p, q, mv in zip(ps, p64, moved):
        ref = q.detach()
        fig[0] = max(fig[0], R.units(p.detach().double().cpu().numpy(), ref.numpy(),
                                     (ref.abs() + mv).numpy()))
        for j, key in ((1, "exp_avg_sq"), (2, "max_exp_avg_sq")):
            if key in o64.state[q] and not moments:
                assert key in opt.state[p]
            elif key in o64.state[q]:
                want = o64.state[q][key].numpy()
                got = opt.state[p][key].detach().double().cpu().numpy().reshape(want.shape)
                fig[j] = max(fig[j], R.units(got, want, np.abs(want)))
            else:
                assert key not in opt.state.get(p, {}), key
    return fig


def _against_torch(what, make_fused, make_torch, groups=None, sched=None, skip=(), seed=31,
                   persistent=False, moments=False):
    """Run FusedAdam on the GPU, torch's optimizer in float64 and in fp32 on the CPU; assert the
    bar; return (gpu params, fused optimizer, float64 optimizer, float64 params)."""
    host, grads = _start(seed)
    groups = groups or (lambda ps: ps)
    runs = []
    for ps, make in ((_cpu_params(host, torch.float64), make_torch),
                     (_cpu_params(host, torch.float32), make_torch),
                     (_gpu_params(host), make_fused)):
        buf = None
        if isinstance(ps, tuple):
            ps, buf = ps
        opt = make(groups(ps))
        moved = _drive(ps, opt, grads, sched(opt) if sched else None, skip, persistent,
                       scale=make is make_torch and ps[0].dtype == torch.float64)
        runs.append((ps, opt, moved, buf))
    (p64, o64, moved, _), (p32, o32, _, _), (pg, og, _, buf) = runs
    assert not buf[0].item() and not buf[2:].any().item(), "a float beside the view changed"
    f_gpu = _figures(pg, og, p64, o64, moved, moments)
    f_cpu = _figures(p32, o32, p64, o64, moved, moments)
    print(f"FusedAdam {what}: p {f_gpu[0]:.2f} v {f_gpu[1]:.2f} vmax {f_gpu[2]:.2f} units; "
          f"torch fp32 CPU p {f_cpu[0]:.2f} v {f_cpu[1]:.2f} vmax {f_cpu[2]:.2f}")
    for name, a, b in zip(("p", "exp_avg_sq", "max_exp_avg_sq"), f_gpu, f_cpu):
        assert a <= R.bar(b), (what, name, a, b)
    for p, q in zip(pg, p64):   # the step counts are torch's
        if q in o64.state and len(o64.state[q]):
            assert float(og.state[p]["step"]) == float(o64.state[q]["step"])
    return pg, og, o64, p64


OPTIONS = {"amsgrad": dict(amsgrad=True), "maximize": dict(maximize=True),
           "decoupled": dict(decoupled_weight_decay=True),
           "all": dict(amsgrad=True, maximize=True, decoupled_weight_decay=True)}


@pytest.mark.parametrize("name", list(OPTIONS))
def test_options_match_torch_adam_float64(name):
    from mauv.optim import FusedAdam
    kw = dict(lr=1e-3, betas=BETAS, weight_decay=1e-2, **OPTIONS[name])
    pg, og, _, _ = _against_torch(name, lambda ps: FusedAdam(ps, **kw),
                                  lambda ps: torch.optim.Adam(ps, **kw), moments=True)
    assert ("max_exp_avg_sq" in og.state[pg[0]]) == bool(kw.get("amsgrad"))
    assert 0 not in og._fast   # not the plain-group entry points


def _three_groups(ps):
    return [dict(params=ps[:2], lr=1e-3),
            dict(params=ps[2:3], lr=3e-3, weight_decay=1e-2, amsgrad=True),
            dict(params=ps[3:], lr=1e-4, weight_decay=1e-3)]


def test_three_groups_steplr_one_launch(monkeypatch):
    """Three groups with different lr, weight decay and amsgrad, a StepLR halving every lr after
    every second step: one mauv_adam_step_ex call per step (the first included: every parameter
    is at the same count) and no other Adam launch; the lr each step uses is the scheduler's."""
    from mauv.optim import FusedAdam
    from mauv._lib import lib
    calls = {"ex": 0, "plain": 0}
    real_ex, real_plain = lib.mauv_adam_step_ex, lib.mauv_adam_step

    def ex(tab, n, groups, n_groups, *a):
        calls["ex"] += 1
        assert (n, n_groups) == (len(SHAPES), 3)
        return real_ex(tab, n, groups, n_groups, *a)

    def plain(*a):
        calls["plain"] += 1
        return real_plain(*a)
    monkeypatch.setattr(lib, "mauv_adam_step_ex", ex)
    monkeypatch.setattr(lib, "mauv_adam_step", plain)
    per_step = []

    def sched(opt):
        s = torch.optim.lr_scheduler.StepLR(opt, step_size=2, gamma=0.5)
        if isinstance(opt, FusedAdam):
            opt.register_step_post_hook(lambda *a: per_step.append(calls["ex"]))
        return s
    pg, og, o64, _ = _against_torch("three groups + StepLR", FusedAdam, torch.optim.Adam,
                                    groups=_three_groups, sched=sched, persistent=True)
    assert per_step == [1, 2, 3, 4, 5] and calls["plain"] == 0
    assert [g["lr"] for g in og.param_groups] == [g["lr"] for g in o64.param_groups]
    assert og.param_groups[0]["lr"] == pytest.approx(1e-3 / 4)
    assert "ex" in og._fast   # the cached path took the later steps
    assert ["max_exp_avg_sq" in og.state[p] for p in pg] == [False, False, True, False, False]


def test_ten_groups_take_two_launches(monkeypatch):
    """More than 8 groups: the first eight in one launch, the rest in a second (a row's group
    column counts within its launch); ten one-tensor groups with their own lr, every other one
    with amsgrad, against torch.optim.Adam on the GPU tensors' float64 copies."""
    from mauv.optim import FusedAdam
    from mauv._lib import lib
    seen, real = [], lib.mauv_adam_step_ex
    monkeypatch.setattr(lib, "mauv_adam_step_ex",
                        lambda tab, n, g, ng, *a: seen.append((n, ng)) or real(tab, n, g, ng, *a))
    gen = torch.Generator().manual_seed(51)
    host = [torch.randn(3 + i, generator=gen) for i in range(10)]
    pg = [h.clone().to(dev).requires_grad_(True) for h in host]
    p64 = [h.double().requires_grad_(True) for h in host]
    groups = lambda ps: [dict(params=[p], lr=1e-3 * (i + 1), amsgrad=bool(i % 2))
                         for i, p in enumerate(ps)]
    og, o64 = FusedAdam(groups(pg), betas=BETAS), torch.optim.Adam(groups(p64), betas=BETAS)
    for _ in range(3):
        for p, q in zip(pg, p64):
            g = torch.randn(p.shape, generator=gen)
            p.grad, q.grad = g.to(dev), g.double()
        og.step()
        o64.step()
    assert seen == [(8, 8), (2, 2)] * 3
    for i, (p, q) in enumerate(zip(pg, p64)):
        assert ("max_exp_avg_sq" in og.state[p]) == bool(i % 2)
        # |p| < 4: three fp32 roundings of p are within 3 * 2^-23 = 3.6e-7; the three updates,
        # each about lr in size, within 1e-4 of themselves.  Another group's lr (a wrong group
        # column) would move p by 1e-3 or more.
        assert float(q.detach().abs().max()) < 4
        torch.testing.assert_close(p.detach().double().cpu(), q.detach(), rtol=0,
                                   atol=1e-6 + 1e-4 * 3 * 1e-3 * (i + 1))


def test_parameter_without_gradient_keeps_its_own_count():
    """Tensor 2 (the amsgrad group's) has no gradient on steps 2 and 3: its count stays behind
    like torch's, and its later steps use its own bias correction."""
    from mauv.optim import FusedAdam
    pg, og, o64, p64 = _against_torch("missed steps", FusedAdam, torch.optim.Adam,
                                      groups=_three_groups, skip={(1, 2), (2, 2)})
    assert [float(og.state[p]["step"]) for p in pg] == [5.0, 5.0, 3.0, 5.0, 5.0]


def test_amsgrad_state_dict_round_trip_through_torch_adam():
    """A FusedAdam state_dict with amsgrad loads into torch.optim.Adam and from there into a
    second FusedAdam (copies: torch's load keeps the very step tensors it is given); all three
    continue: the two FusedAdam bit-identically, torch's within rounding."""
    from mauv.optim import FusedAdam
    host, grads = _start(41)
    kw = dict(lr=2e-3, betas=BETAS, weight_decay=1e-2, amsgrad=True)
    pa, _ = _gpu_params(host)
    oa = FusedAdam(pa, **kw)
    _drive(pa, oa, grads[:3])
    sd = oa.state_dict()
    assert set(sd["param_groups"][0]) == set(torch.optim.Adam(
        [torch.zeros(1, requires_grad=True)]).state_dict()["param_groups"][0])
    assert all(set(s) == {"step", "exp_avg", "exp_avg_sq", "max_exp_avg_sq"}
               for s in sd["state"].values())
    pt = [p.detach().clone().requires_grad_(True) for p in pa]
    ot = torch.optim.Adam(pt, lr=1.0)
    ot.load_state_dict(copy.deepcopy(sd))
    assert ot.param_groups[0]["amsgrad"] and ot.param_groups[0]["lr"] == 2e-3
    pb = [p.detach().clone().requires_grad_(True) for p in pa]
    ob = FusedAdam(pb, lr=1.0)
    ob.load_state_dict(copy.deepcopy(ot.state_dict()))
    for ps, opt in ((pa, oa), (pt, ot), (pb, ob)):
        _drive(ps, opt, grads[3:])
    for a, t, b in zip(pa, pt, pb):
        assert torch.equal(a.detach(), b.detach())
        assert torch.equal(oa.state[a]["max_exp_avg_sq"], ob.state[b]["max_exp_avg_sq"])
        assert float(oa.state[a]["step"]) == float(ot.state[t]["step"]) == 5.0
        torch.testing.assert_close(t.detach(), a.detach(), rtol=1e-6, atol=1e-7)
        torch.testing.assert_close(ot.state[t]["max_exp_avg_sq"], oa.state[a]["max_exp_avg_sq"],
                                   rtol=1e-6, atol=1e-12)


def test_fused_adamw_is_torch_adamw():
    from mauv.optim import FusedAdamW
    kw = dict(lr=1e-3, betas=BETAS, amsgrad=True)
    pg, og, o64, _ = _against_torch("AdamW", lambda ps: FusedAdamW(ps, **kw),
                                    lambda ps: torch.optim.AdamW(ps, **kw), moments=True)
    g, t = og.param_groups[0], o64.param_groups[0]
    assert set(g) == set(t)
    assert g["weight_decay"] == t["weight_decay"] == 1e-2 and g["decoupled_weight_decay"] is True
    pt = [p.detach().clone().requires_grad_(True) for p in pg]
    ot = torch.optim.AdamW(pt)
    ot.load_state_dict(copy.deepcopy(og.state_dict()))
    og2 = FusedAdamW(pg)
    og2.load_state_dict(copy.deepcopy(ot.state_dict()))
    assert float(og2.state[pg[0]]["step"]) == STEPS


def test_factory_passes_the_callers_options_for_a_gpu_model():
    """define_optimizers_and_schedulers forwards optimizer_params[...] as keyword arguments, as
    the reference does into torch.optim.Adam: amsgrad and fused=True build a FusedAdam."""
    from mauv.loop_utils import define_optimizers_and_schedulers
    from mauv.optim import FusedAdam
    keys = ("image_model", "bathy_model", "sss_model", "multimodal_model")
    models = {k: torch.nn.Linear(5, 3).to(dev) for k in keys}
    opts = {k: {"lr": 1e-4, "weight_decay": 1e-5, "amsgrad": True, "fused": True} for k in keys}
    _, optimizers, schedulers = define_optimizers_and_schedulers(
        models, opts, {k: {"step_size": 1, "gamma": 0.5} for k in keys})
    for k in keys:
        opt = optimizers[k]
        assert isinstance(opt, FusedAdam)
        g = opt.param_groups[0]
        assert g["amsgrad"] is True and g["fused"] is True and g["lr"] == 1e-4
        models[k](torch.randn(4, 5, device=dev)).sum().backward()
        before = [p.detach().clone() for p in models[k].parameters()]
        opt.step()
        schedulers[k].step()
        assert g["lr"] == 5e-5
        for p, b in zip(models[k].parameters(), before):
            assert "max_exp_avg_sq" in opt.state[p] and not torch.equal(p.detach(), b)
