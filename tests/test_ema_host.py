"""The weight EMA of the gated Adam step, the parts that need no GPU: the C-ABI of
``mauv_adam_step_ex_ema`` / ``mauv_ema_update`` / ``mauv_ema_swap`` (exported, declared, defined,
bound; ``MauvEma`` is 32 bytes beside an unchanged 64-byte gate; every documented argument error
answers before any launch), FusedAdam's ``ema_decay`` / ``ema_warmup`` / ``ema_eval`` options
(validated plain attributes, no ``param_groups`` keys) and their way through
``define_optimizers_and_schedulers`` to both optimizer kinds, a host model under
``torch.optim.Adam`` + ``HostEma`` through ``mc_train_step`` with one NaN batch, which must equal
``torch.optim.swa_utils.AveragedModel`` with ``get_ema_multi_avg_fn`` updated after the steps that
ran, bit for bit, and ``train_and_evaluate_unimodal_model`` evaluating inside ``averaged()``."""
import ctypes
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn

from tests.test_abi_host import HEADER, header_functions
from tests.test_accum_host import _struct_fields, _DeviceModel, KEYS, CSRC
from tests.test_gradclip_host import Tiny, _batches, _params

NEW = {"mauv_adam_step_ex_ema": 10, "mauv_ema_update": 4, "mauv_ema_swap": 3}


# ------------------------------------------------------------------------------------- ABI
def test_ema_struct_is_32_bytes_and_the_gate_is_unchanged():
    from mauv import optim
    from mauv._lib import MauvEma, MauvEmaRow, lib
    fields = _struct_fields("MauvEma")

    class Ema(ctypes.Structure):
        _fields_ = fields

    assert ctypes.sizeof(Ema) == ctypes.sizeof(MauvEma) == 32 == 4 * optim.EMA_WORDS
    assert [(n, t._type_ if hasattr(t, "_length_") else t) for n, t in fields] == \
        [(n, t._type_ if hasattr(t, "_length_") else t) for n, t in MauvEma._fields_]
    assert MauvEma.decay.offset == 4 * optim.E_DECAY == 0 and dict(fields)["decay"] is ctypes.c_float
    assert MauvEma.warmup.offset == 4 * optim.E_WARMUP == 4
    assert MauvEma.updates.offset == 4 * optim.E_UPDATES == 8
    assert MauvEma.weight.offset == 4 * optim.E_WEIGHT == 12
    assert dict(fields)["weight"] is ctypes.c_float
    assert MauvEma.reserved.offset == 16
    assert ctypes.sizeof(MauvEmaRow) == 24 and MauvEmaRow.numel.offset == 16

    class Gate(ctypes.Structure):
        _fields_ = _struct_fields("MauvStepGate")

    assert ctypes.sizeof(Gate) == 64 == 4 * optim.GATE_WORDS and Gate.reserved.offset == 56
    assert lib.mauv_abi_version() == 4


def test_entry_points_exported_declared_defined_and_bound():
    from mauv._lib import LIB_PATH, SIGNATURES
    raw = ctypes.CDLL(LIB_PATH)
    names = header_functions()
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    protos = dict(re.findall(r"(mauv_\w+)\(([^)]*)\)\s*;", txt))
    src = re.sub(r"//[^\n]*", "", open(CSRC).read())
    defs = dict(re.findall(r"MAUV_API\s+int\s+(mauv_\w+)\(([^)]*)\)\s*\{", src))

    def types(params):
        out = []
        for p in params.split(","):
            p = re.sub(r"\bconst\b", "", p).strip()
            out.append(re.sub(r"\s*\w+$", "", p).replace(" ", ""))
        return out

    for n, arity in NEW.items():
        assert hasattr(raw, n) and n in names and n in SIGNATURES and n in defs, n
        assert len(SIGNATURES[n]) == arity == len(types(protos[n])) == len(types(defs[n])), n
        assert types(protos[n]) == types(defs[n]), n
        for ct, ty in zip(SIGNATURES[n], types(protos[n])):
            assert (ct is ctypes.c_int) == (ty == "int"), (n, ty)
            assert (ct is ctypes.c_float) == (ty == "float"), (n, ty)
            assert (ct is ctypes.c_void_p) == (ty.endswith("*") or ty == "hipStream_t"), (n, ty)
    # the entries these join are as they were
    assert len(SIGNATURES["mauv_adam_step_ex_accum"]) == 8
    assert len(SIGNATURES["mauv_adam_step_ex_scaled"]) == 7


def test_argument_errors_answer_without_a_device():
    """The checks come before any launch (this process has no GPU: a launch would fail
    differently) and name their entry point."""
    from mauv._lib import lib, MauvAdamGroup, MauvLossScale, MauvAccum, MauvEma, MauvEmaRow
    arr = (MauvAdamGroup * 8)()
    table = (ctypes.c_longlong * 7)()
    gate = (ctypes.c_int * 16)()
    shadows = (ctypes.c_void_p * 1)()
    ls, acc, ema = MauvLossScale(scale=2.0), MauvAccum(), MauvEma(decay=0.9)
    tab, grp, gp, lp, ap, sp, ep = (ctypes.addressof(x)
                                    for x in (table, arr, gate, ls, acc, shadows, ema))
    cases = [(None, 1, grp, 1, gp), (tab, 0, grp, 1, gp), (tab, -1, grp, 1, gp),
             (tab, 65536, grp, 1, gp), (tab, 1, None, 1, gp), (tab, 1, grp, 0, gp),
             (tab, 1, grp, 9, gp), (tab, 1, grp, 1, None)]
    for t, n, g, ng, gt in cases:
        for scaler in (lp, None):
            for a in (ap, None):
                for rows, e in ((sp, ep), (None, ep), (sp, None)):
                    assert lib.mauv_adam_step_ex_ema(t, n, g, ng, gt, scaler, a, rows, e,
                                                     None) < 0, (n, ng)
                    assert b"adam_step_ex_ema" in lib.mauv_last_error()
    rows = (MauvEmaRow * 1)()
    rp = ctypes.addressof(rows)
    for r, n, w in ((None, 1, 0.5), (rp, 0, 0.5), (rp, -1, 0.5), (rp, 65536, 0.5), (rp, 1, 0.0),
                    (rp, 1, -0.5), (rp, 1, 1.5), (rp, 1, float("nan")), (rp, 1, float("inf"))):
        assert lib.mauv_ema_update(r, n, w, None) < 0, (n, w)
        assert b"ema_update" in lib.mauv_last_error()
    for r, n in ((None, 1), (rp, 0), (rp, -1), (rp, 65536)):
        assert lib.mauv_ema_swap(r, n, None) < 0
        assert b"ema_swap" in lib.mauv_last_error()
    assert list(gate) == [0] * 16 and ls.scale == 2.0 and acc.windows == 0
    assert (ema.updates, ema.weight, ema.warmup) == (0, 0.0, 0)


# ----------------------------------------------------------------------------------- options
@pytest.mark.parametrize("bad", [0, 1, -0.1, True, "x", float("inf"), float("nan"), 1.5,
                                 torch.tensor(0.5)])
def test_bad_ema_decay_raises(bad):
    from mauv.optim import FusedAdam, FusedAdamW, HostEma
    for cls in (FusedAdam, FusedAdamW):
        with pytest.raises(ValueError, match="ema_decay"):
            cls(_params(), ema_decay=bad)
    opt = FusedAdam(_params(), ema_decay=0.99)
    with pytest.raises(ValueError, match="ema_decay"):
        opt.ema_decay = bad
    assert opt.ema_decay == 0.99
    with pytest.raises(ValueError, match="ema_decay"):
        HostEma(_params(), bad)


@pytest.mark.parametrize("name", ["ema_warmup", "ema_eval"])
def test_bad_ema_flags_raise(name):
    from mauv.optim import FusedAdam
    for bad in (1, 0, None, "yes"):
        with pytest.raises(ValueError, match=name):
            FusedAdam(_params(), ema_decay=0.9, **{name: bad})


def test_the_option_was_unsupported_before_and_others_still_are():
    from mauv.optim import FusedAdam
    opt = FusedAdam(_params(), ema_decay=0.999)      # (ValueError: unsupported option, before)
    assert opt.ema_decay == 0.999 and opt.ema_warmup is False and opt.ema_eval is True
    with pytest.raises(ValueError, match="unsupported option"):
        FusedAdam(_params(), ema_decay=0.999, ema_buffers=True)


def test_options_are_attributes_out_of_the_groups():
    from mauv.optim import FusedAdam, FusedAdamW
    d = FusedAdam(_params())
    assert d.ema_decay is None and d.ema_warmup is False and d.ema_eval is True
    assert set(d.state_dict()) == {"state", "param_groups"} and d.ema_parameters() == []
    with pytest.raises(RuntimeError, match="no weight EMA"):
        d.swap_ema()
    for o, ref in ((FusedAdam(_params(), lr=1e-3, ema_decay=0.9, ema_warmup=True, ema_eval=False),
                    torch.optim.Adam(_params(), lr=1e-3)),
                   (FusedAdamW(_params(), ema_decay=0.5), torch.optim.AdamW(_params()))):
        assert list(o.param_groups[0]) == list(ref.param_groups[0])
        sd = o.state_dict()
        assert set(sd) == {"state", "param_groups", "ema_updates"} and sd["ema_updates"] == 0
        assert not any("ema" in k for g in sd["param_groups"] for k in g)
        ref.load_state_dict(sd)
        o.load_state_dict(ref.state_dict())
        assert o.ema_decay in (0.9, 0.5)           # loading a state leaves the options alone
        o.load_state_dict(dict(sd, ema_updates=7))
        assert o.ema_updates == 7 and o.state_dict()["ema_updates"] == 7
    o.ema_decay = 0.75                             # reassigned between steps
    o.ema_warmup, o.ema_eval = True, False
    assert (o.ema_decay, o.ema_warmup, o.ema_eval) == (0.75, True, False)
    # no shadows yet (nothing stepped): the swap is a flag, and guards the step and the state
    with o.averaged():
        for call in (o.step, o.state_dict, lambda: o.step_gated(None)):
            with pytest.raises((RuntimeError, AssertionError), match="averaged|gate"):
                call()
    o.state_dict()
    o.ema_decay = None
    assert set(o.state_dict()) == {"state", "param_groups"}


def test_host_weight_rule_is_the_documented_one():
    from mauv.optim import ema_weight
    for decay in (0.9, 0.999, 0.9999):
        d32 = float(np.float32(decay))
        assert ema_weight(0, decay, False) == 1.0 == ema_weight(0, decay, True)
        for n in range(1, 40):
            assert ema_weight(n, decay, False) == float(np.float32(1.0 - d32))
            assert ema_weight(n, decay, True) == \
                float(np.float32(1.0 - min(d32, (1.0 + n) / (10.0 + n))))


def test_factory_carries_the_options_to_both_optimizer_kinds():
    from mauv.loop_utils import define_optimizers_and_schedulers
    from mauv.optim import FusedAdam, HostEma, ema_of
    models = {k: (_DeviceModel() if k == "image_model" else Tiny()) for k in KEYS}
    sched = {k: dict(step_size=5, gamma=0.5) for k in KEYS}
    _, opts, _ = define_optimizers_and_schedulers(
        models, {k: dict(lr=1e-2, ema_decay=0.99, ema_warmup=True, ema_eval=False)
                 for k in KEYS}, sched)
    fused, host = opts["image_model"], opts["multimodal_model"]
    assert type(fused) is FusedAdam and type(host) is torch.optim.Adam
    assert (fused.ema_decay, fused.ema_warmup, fused.ema_eval) == (0.99, True, False)
    assert ema_of(fused) is fused and type(host.ema) is HostEma and ema_of(host) is host.ema
    assert (host.ema.ema_decay, host.ema.ema_warmup, host.ema.ema_eval) == (0.99, True, False)
    for o in (fused, host):
        assert not any(k.startswith("ema") for k in o.param_groups[0])
    ps = list(models["multimodal_model"].parameters())
    assert [p is q for p, (q, _) in zip(ps, host.ema.ema_parameters())] == [True] * len(ps)
    assert all(torch.equal(p, e) and e is not p for p, e in host.ema.ema_parameters())
    plain = define_optimizers_and_schedulers(models, {k: dict(lr=1e-2) for k in KEYS}, sched)[1]
    assert plain["image_model"].ema_decay is None and ema_of(plain["image_model"]) is None
    assert plain["multimodal_model"].ema is None and ema_of(plain["multimodal_model"]) is None
    for v in (0, 1, True, "x"):
        with pytest.raises(ValueError, match="ema_decay"):
            define_optimizers_and_schedulers(
                models, {k: dict(lr=1e-2, ema_decay=v) for k in KEYS}, sched)


# --------------------------------------------------------------------------------- host loop
def _host_pair(**ema):
    from mauv.loop_utils import define_optimizers_and_schedulers
    torch.manual_seed(0)
    model, ref = Tiny(), Tiny()
    ref.load_state_dict(model.state_dict())
    models = {k: (model if k == "multimodal_model" else Tiny()) for k in KEYS}
    crit, opts, _ = define_optimizers_and_schedulers(
        models, {k: dict(lr=1e-2, weight_decay=1e-5, **ema) for k in KEYS},
        {k: dict(step_size=50, gamma=0.5) for k in KEYS})
    ropt = torch.optim.Adam(ref.parameters(), lr=1e-2, weight_decay=1e-5)
    return model, ref, crit, opts["multimodal_model"], ropt


def _nan_batch(batches, i):
    nan = batches[i][0].clone()
    nan[0, 0, 0, 0] = float("nan")
    batches[i] = (nan,) + batches[i][1:]


def test_host_model_equals_the_averaged_model_loop_bit_for_bit(caplog):
    from mauv.train import mc_train_step
    model, ref, crit, opt, ropt = _host_pair(ema_decay=0.9)
    avg = AveragedModel(ref, multi_avg_fn=get_ema_multi_avg_fn(0.9))
    batches = _batches(6)
    _nan_batch(batches, 2)
    ran = []
    for i, (x, b, s, y) in enumerate(batches):
        with caplog.at_level("WARNING"):
            r = mc_train_step(model, (x, b, s), y, crit, opt, 2, 4, 0.5)
        ran.append(r is not None)
        if i == 2:
            continue
        out = torch.stack([ref(x, b, s) for _ in range(2)]).mean(0)
        F.cross_entropy(out, y).backward()
        ropt.step()
        ropt.zero_grad()
        avg.update_parameters(ref)                  # only after a step that ran
        for (p, e), q, a in zip(opt.ema.ema_parameters(), ref.parameters(), avg.parameters()):
            assert torch.equal(p, q) and torch.equal(e, a), i
    assert ran == [True, True, False, True, True, True] and "NaN/Inf loss" in caplog.text
    assert opt.ema.ema_updates == 5 == int(avg.n_averaged)
    assert not any(torch.equal(p, e) for p, e in opt.ema.ema_parameters())   # it is an average


def test_host_warmup_follows_the_capped_decay():
    from mauv.optim import HostEma
    torch.manual_seed(1)
    p = torch.nn.Parameter(torch.randn(5))
    ema, e = HostEma([p], 0.999, ema_warmup=True), None
    for n in range(12):
        with torch.no_grad():
            p.add_(torch.randn(5))
        ema.update()
        if n == 0:
            e = p.detach().clone()
        else:
            e.lerp_(p.detach(), 1 - min(0.999, (1.0 + n) / (10.0 + n)))
        assert torch.equal(ema.shadows[0], e), n


def test_host_swap_is_exact_and_guards_the_update():
    from mauv.optim import HostEma
    torch.manual_seed(2)
    ps = [torch.nn.Parameter(torch.randn(4)), torch.nn.Parameter(torch.randn(2, 3))]
    frozen = torch.nn.Parameter(torch.randn(3), requires_grad=False)
    ema = HostEma(ps + [frozen], 0.5)
    assert len(ema.ema_parameters()) == 2            # a frozen parameter gets no shadow
    ema.update()
    with torch.no_grad():
        for p in ps:
            p.mul_(3.0)
    ema.update()
    live = [p.detach().clone() for p in ps]
    shadow = [e.clone() for e in ema.shadows]
    with ema.averaged():
        assert all(torch.equal(p, s) for p, s in zip(ps, shadow))
        assert all(torch.equal(e, l) for e, l in zip(ema.shadows, live))
        with pytest.raises(RuntimeError, match="averaged"):
            ema.update()
    assert all(torch.equal(p, l) for p, l in zip(ps, live))
    assert all(torch.equal(e, s) for e, s in zip(ema.shadows, shadow))


@pytest.mark.parametrize("ema_eval", [True, False])
def test_unimodal_loop_evaluates_inside_averaged(tmp_path, monkeypatch, ema_eval):
    """train_and_evaluate_unimodal_model with a HostEma: the (stubbed) evaluation sees the
    shadows' checksum when ``ema_eval`` is true, the live weights' otherwise, and the live weights
    are back afterwards."""
    import mauv.loop_utils as LU
    import mauv.train as T
    from mauv.optim import HostEma
    from tests.helpers import ListLoader, NullWriter
    monkeypatch.setattr(T, "get_kl_loss", lambda model: torch.tensor(0.05))

    class Uni(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.f = torch.nn.Linear(3 * 8 * 8, 3)

        def forward(self, x):
            return self.f(x.flatten(1))

    def checksum(ts):
        return [t.detach().double().sum().item() for t in ts]

    torch.manual_seed(0)
    model = Uni()
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    opt.ema = HostEma(model.parameters(), 0.9, ema_eval=ema_eval)
    seen = []

    def evaluate(model, **kw):
        seen.append((checksum(model.parameters()), checksum(opt.ema.shadows)))
        return 0.5

    monkeypatch.setattr(LU, "evaluate_unimodal_model", evaluate)
    batches = [{"main_image": x, "label": y} for x, _, _, y in _batches(3)]
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=5)
    LU.train_and_evaluate_unimodal_model(
        model, ListLoader(batches, 4), ListLoader(batches, 4), torch.nn.CrossEntropyLoss(), opt,
        sched, num_epochs=3, device=torch.device("cpu"), model_name="image",
        save_dir=str(tmp_path), num_mc=2, sum_writer=NullWriter())
    assert len(seen) == 2 and opt.ema.ema_updates == 6
    live, shadow = checksum(model.parameters()), checksum(opt.ema.shadows)
    assert live != shadow
    # the last evaluation: inside averaged() the model held the shadows and the shadows the live
    assert seen[-1] == ((shadow, live) if ema_eval else (live, shadow))
    assert opt.ema._swapped is False
