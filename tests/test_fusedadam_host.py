"""FusedAdam's host side, no GPU: the constructor options it takes and refuses, param_groups
keys equal to torch.optim.Adam's (so a state_dict loads either way), and the new entry point
exported by the library, declared in include/mauv.h and bound with the same arity."""
import ctypes
import os
import re

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "mauv.h")


def _params():
    return [torch.zeros(3, requires_grad=True), torch.zeros(2, 2, requires_grad=True)]


@pytest.mark.parametrize("kw", [
    dict(amsgrad=True), dict(maximize=True), dict(decoupled_weight_decay=True),
    dict(amsgrad=True, maximize=True, decoupled_weight_decay=True, weight_decay=1e-2),
    dict(fused=True), dict(foreach=True), dict(fused=False, foreach=False),
    dict(capturable=False, differentiable=False),
], ids=lambda kw: "+".join(kw))
def test_accepted_options_are_kept_in_param_groups(kw):
    from mauv.optim import FusedAdam
    opt = FusedAdam(_params(), lr=1e-4, **kw)
    ref = torch.optim.Adam(_params(), lr=1e-4)
    assert list(opt.param_groups[0]) == list(ref.param_groups[0])
    for k, v in kw.items():
        assert opt.param_groups[0][k] == v
    for k in set(ref.param_groups[0]) - set(kw) - {"params"}:
        assert opt.param_groups[0][k] == ref.param_groups[0][k], k


@pytest.mark.parametrize("kw", [
    dict(capturable=True), dict(differentiable=True), dict(lr=torch.tensor(1e-3)),
    dict(betas=(torch.tensor(0.9), 0.999)), dict(betas=(0.9, torch.tensor(0.999))),
    dict(lr=-1.0), dict(eps=-1e-8), dict(betas=(1.0, 0.999)), dict(weight_decay=-1.0),
    dict(nesterov=True),
], ids=lambda kw: "+".join(kw))
def test_rejected_options_raise_value_error(kw):
    from mauv.optim import FusedAdam
    with pytest.raises(ValueError):
        FusedAdam(_params(), **kw)


def test_rejected_options_in_a_group_raise_too():
    from mauv.optim import FusedAdam
    with pytest.raises(ValueError):
        FusedAdam([dict(params=_params(), capturable=True)])
    opt = FusedAdam(_params())
    with pytest.raises(ValueError):
        opt.add_param_group(dict(params=[torch.zeros(1, requires_grad=True)],
                                 lr=torch.tensor(1e-3)))


def test_adamw_defaults_and_keys():
    from mauv.optim import FusedAdamW
    opt, ref = FusedAdamW(_params()), torch.optim.AdamW(_params())
    assert list(opt.param_groups[0]) == list(ref.param_groups[0])
    for k in set(ref.param_groups[0]) - {"params"}:
        assert opt.param_groups[0][k] == ref.param_groups[0][k], k
    assert opt.param_groups[0]["weight_decay"] == 1e-2
    with pytest.raises(ValueError):
        FusedAdamW(_params(), decoupled_weight_decay=False)


def test_state_dict_groups_load_into_torch_adam_and_back():
    """Before any step (no GPU here): the param_groups of one optimizer are the other's."""
    from mauv.optim import FusedAdam
    groups = [dict(params=_params()[:1], lr=1e-4),
              dict(params=_params()[1:], lr=1e-3, amsgrad=True, weight_decay=1e-2)]
    opt = FusedAdam(groups, fused=True)
    sd = opt.state_dict()
    ref = torch.optim.Adam([dict(params=_params()[:1]), dict(params=_params()[1:])])
    ref.load_state_dict(sd)
    assert [g["amsgrad"] for g in ref.param_groups] == [False, True]
    assert ref.param_groups[1]["weight_decay"] == 1e-2 and ref.param_groups[0]["fused"] is True
    back = FusedAdam([dict(params=_params()[:1]), dict(params=_params()[1:])])
    back.load_state_dict(ref.state_dict())
    assert [g["lr"] for g in back.param_groups] == [1e-4, 1e-3]
    # a state_dict from before these keys existed
    old = opt.state_dict()
    for g in old["param_groups"]:
        for k in ("foreach", "capturable", "differentiable", "fused", "decoupled_weight_decay"):
            del g[k]
    back.load_state_dict(old)
    assert all(g["decoupled_weight_decay"] is False and g["fused"] is None
               for g in back.param_groups)


def test_gate_needs_a_device_and_one_to_eight_groups():
    """gate() answers None without touching a device when the group count is out of range or
    the parameters are not the optimizer's trainable ones."""
    from mauv.optim import FusedAdam
    ps = [torch.zeros(1, requires_grad=True) for _ in range(9)]
    assert FusedAdam([dict(params=[p]) for p in ps]).gate(ps, "cpu") is None
    opt = FusedAdam(ps[:3])
    assert opt.gate(ps[:2], "cpu") is None
    ps[2].requires_grad_(False)
    ps[2].grad = torch.zeros(1)     # a frozen parameter still holding a gradient
    assert opt.gate(ps[:2], "cpu") is None


def test_adam_step_ex_exported_declared_and_bound():
    from mauv._lib import LIB_PATH, SIGNATURES, MauvAdamGroup
    assert hasattr(ctypes.CDLL(LIB_PATH), "mauv_adam_step_ex")
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    protos = dict(re.findall(r"(mauv_\w+)\(([^)]*)\)\s*;", txt))
    assert "mauv_adam_step_ex" in protos
    assert len(SIGNATURES["mauv_adam_step_ex"]) == protos["mauv_adam_step_ex"].count(",") + 1 == 7
    assert ctypes.sizeof(MauvAdamGroup) == 32
    assert re.search(r"#define\s+MAUV_ADAM_MAX_GROUPS\s+8\b", txt)
    # the entries this one joins are as they were
    assert len(SIGNATURES["mauv_adam_step"]) == 9 and len(SIGNATURES["mauv_adam_step_gated"]) == 9


def test_adam_step_ex_argument_errors_need_no_device():
    """The argument checks come before any launch: they answer on a machine without a GPU."""
    from mauv._lib import lib, MauvAdamGroup
    arr = (MauvAdamGroup * 8)()
    table = (ctypes.c_longlong * 7)()
    tab, grp = ctypes.addressof(table), ctypes.addressof(arr)
    for n, ng, step in ((0, 1, 1), (65536, 1, 1), (1, 0, 1), (1, 9, 1), (1, 1, 0)):
        assert lib.mauv_adam_step_ex(tab, n, grp, ng, step, None, None) == -1, (n, ng, step)
        assert b"adam_step_ex" in lib.mauv_last_error()


def test_gated_entries_argument_errors_start_with_their_own_name():
    """Every gated all-groups entry refuses n = 0, n = 65536, 0 or 9 groups, a null table, null
    groups and a null gate before any launch, with ERR_ARG and a message that starts with the
    entry's own name — also with every optional pointer NULL, where the entry computes exactly
    what the one before it does."""
    from mauv._lib import lib, MauvAdamGroup, MauvLossScale, MauvAccum, MauvEma
    arr = (MauvAdamGroup * 8)()
    table = (ctypes.c_longlong * 7)()
    gate = (ctypes.c_int * 16)()
    shadows = (ctypes.c_void_p * 1)()
    ls, acc, ema = MauvLossScale(scale=2.0), MauvAccum(), MauvEma(decay=0.9)
    tab, grp, gp, lp, ap, sp, ep = (ctypes.addressof(x)
                                    for x in (table, arr, gate, ls, acc, shadows, ema))
    entries = {
        "adam_step_ex": lambda t, n, g, ng, gt, on: lib.mauv_adam_step_ex(t, n, g, ng, 0, gt, None),
        "adam_step_ex_scaled": lambda t, n, g, ng, gt, on: lib.mauv_adam_step_ex_scaled(
            t, n, g, ng, gt, lp if on else None, None),
        "adam_step_ex_accum": lambda t, n, g, ng, gt, on: lib.mauv_adam_step_ex_accum(
            t, n, g, ng, gt, lp if on else None, ap if on else None, None),
        "adam_step_ex_ema": lambda t, n, g, ng, gt, on: lib.mauv_adam_step_ex_ema(
            t, n, g, ng, gt, lp if on else None, ap if on else None, sp if on else None,
            ep if on else None, None),
    }
    cases = [(tab, 0, grp, 1, gp), (tab, 65536, grp, 1, gp), (tab, 1, grp, 0, gp),
             (tab, 1, grp, 9, gp), (None, 1, grp, 1, gp), (tab, 1, None, 1, gp),
             (tab, 1, grp, 1, None)]
    for name, call in entries.items():
        for case in cases:
            if name == "adam_step_ex" and case[4] is None:
                continue   # a null gate is this entry's ungated form (refused above at step 0)
            for on in (True, False):
                assert call(*case, on) == -1, (name, case[1], case[3], on)
                msg = lib.mauv_last_error()
                assert msg.startswith(name.encode() + b": "), (name, msg)
    assert list(gate) == [0] * 16 and ls.scale == 2.0 and acc.windows == 0 and ema.updates == 0
