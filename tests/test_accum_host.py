"""Gradient accumulation in the gated Adam step, the parts that need no GPU: the C-ABI of
``mauv_accum_note`` / ``mauv_adam_step_ex_accum`` (exported, declared, bound; ``MauvAccum`` is 32
bytes beside an unchanged 64-byte gate; every documented argument error answers before any
launch), FusedAdam's ``grad_accumulation`` option (a validated plain attribute: no
``param_groups`` key, not in the optimizer state) and its way through
``define_optimizers_and_schedulers`` to both optimizer kinds, and a host model under
``torch.optim.Adam`` through ``mc_train_step`` with K=3 over 7 micro-batches, which must equal a
hand-written torch loop bit for bit: three backward passes summed, ``_foreach_mul_(1/3)``, step;
at the end one backward, ``1/1``, step.  A NaN loss inside a window drops that window whole.
``train_unimodal_model`` accumulates a host model the same way."""
import ctypes
import re

import pytest
import torch
import torch.nn.functional as F

from tests.test_abi_host import HEADER, header_functions
from tests.test_gradclip_host import Tiny, _batches, _params

NEW = {"mauv_accum_note": 3, "mauv_adam_step_ex_accum": 8}
KEYS = ("image_model", "bathy_model", "sss_model", "multimodal_model")
CSRC = HEADER.replace("include/mauv.h", "multimodal-auv_amd/csrc/adam.hip")


# ------------------------------------------------------------------------------------- ABI
def _struct_fields(name):
    txt = open(HEADER).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = decl.split(None, 1)
        ct = {"int": ctypes.c_int, "float": ctypes.c_float}[ctype]
        for n in names.split(","):
            m = re.fullmatch(r"(\w+)\[(\d+)\]", n.strip())
            fields.append((m.group(1), ct * int(m.group(2))) if m else (n.strip(), ct))
    return fields


def test_accum_struct_is_32_bytes_and_the_gate_is_unchanged():
    from mauv import optim
    from mauv._lib import MauvAccum, lib
    fields = _struct_fields("MauvAccum")

    class Acc(ctypes.Structure):
        _fields_ = fields

    assert ctypes.sizeof(Acc) == ctypes.sizeof(MauvAccum) == 32 == 4 * optim.ACC_WORDS
    assert [(n, t._type_ if hasattr(t, "_length_") else t) for n, t in fields] == \
        [(n, t._type_ if hasattr(t, "_length_") else t) for n, t in MauvAccum._fields_]
    assert MauvAccum.micro.offset == 4 * optim.A_MICRO == 0
    assert MauvAccum.bad_loss.offset == 4 * optim.A_BAD_LOSS == 4
    assert MauvAccum.avg.offset == 4 * optim.A_AVG == 8 and dict(fields)["avg"] is ctypes.c_float
    assert MauvAccum.windows.offset == 4 * optim.A_WINDOWS == 12
    assert MauvAccum.dropped.offset == 4 * optim.A_DROPPED == 16
    assert MauvAccum.reserved.offset == 20

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
        """Parameter types in order: pointers by their pointee name, scalars by their type."""
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
            assert (ct is ctypes.c_void_p) == (ty.endswith("*") or ty == "hipStream_t"), (n, ty)
    # the entries these join are as they were
    assert len(SIGNATURES["mauv_adam_step_ex_scaled"]) == 7
    assert len(SIGNATURES["mauv_adam_step_ex"]) == 7


def test_argument_errors_answer_without_a_device():
    """The checks come before any launch (this process has no GPU: a launch would fail
    differently) and name their entry point."""
    from mauv._lib import lib, MauvAdamGroup, MauvLossScale, MauvAccum
    arr = (MauvAdamGroup * 8)()
    table = (ctypes.c_longlong * 7)()
    gate = (ctypes.c_int * 16)()
    ls = MauvLossScale(scale=2.0)
    acc = MauvAccum()
    tab, grp, gp, lp, ap = (ctypes.addressof(x) for x in (table, arr, gate, ls, acc))
    cases = [(None, 1, grp, 1, gp), (tab, 0, grp, 1, gp), (tab, -1, grp, 1, gp),
             (tab, 65536, grp, 1, gp), (tab, 1, None, 1, gp), (tab, 1, grp, 0, gp),
             (tab, 1, grp, 9, gp), (tab, 1, grp, 1, None)]
    for t, n, g, ng, gt in cases:
        for scaler in (lp, None):
            for a in (ap, None):
                assert lib.mauv_adam_step_ex_accum(t, n, g, ng, gt, scaler, a, None) < 0, (n, ng)
                assert b"adam_step_ex_accum" in lib.mauv_last_error()
    for gt, a in ((None, ap), (gp, None), (None, None)):
        assert lib.mauv_accum_note(gt, a, None) < 0
        assert b"accum_note" in lib.mauv_last_error()
    assert list(gate) == [0] * 16 and ls.scale == 2.0 and ls.overflows == 0
    assert (acc.micro, acc.bad_loss, acc.avg, acc.windows, acc.dropped) == (0, 0, 0.0, 0, 0)


# ----------------------------------------------------------------------------------- option
@pytest.mark.parametrize("bad", [0, -1, 2.0, 1.5, True, False, "2", float("nan"),
                                 torch.tensor(2), [2]])
def test_bad_grad_accumulation_raises(bad):
    from mauv.optim import FusedAdam, FusedAdamW
    for cls in (FusedAdam, FusedAdamW):
        with pytest.raises(ValueError, match="grad_accumulation"):
            cls(_params(), grad_accumulation=bad)
    opt = FusedAdam(_params(), grad_accumulation=2)
    with pytest.raises(ValueError, match="grad_accumulation"):
        opt.grad_accumulation = bad
    assert opt.grad_accumulation == 2


def test_option_is_an_attribute_out_of_groups_and_state():
    from mauv.optim import FusedAdam, FusedAdamW
    assert FusedAdam(_params()).grad_accumulation is None
    assert not FusedAdam(_params()).accumulating()
    assert not FusedAdam(_params(), grad_accumulation=1).accumulating()
    for o, ref in ((FusedAdam(_params(), lr=1e-3, grad_accumulation=4),
                    torch.optim.Adam(_params(), lr=1e-3)),
                   (FusedAdamW(_params(), grad_accumulation=2), torch.optim.AdamW(_params()))):
        assert o.accumulating() and not o.closes_window() and o.closes_window(True)
        assert list(o.param_groups[0]) == list(ref.param_groups[0])
        sd = o.state_dict()
        assert set(sd) == {"state", "param_groups"}
        assert not any("accum" in k for g in sd["param_groups"] for k in g)
        ref.load_state_dict(sd)
        o.load_state_dict(ref.state_dict())
        assert o.grad_accumulation in (2, 4)      # loading a state leaves the option alone
    o.grad_accumulation = 3                        # reassigned between windows
    assert o.grad_accumulation == 3
    o.grad_accumulation = None
    assert not o.accumulating() and o.closes_window() and o.closes_window(False)
    o.zero_grad()                                  # no window, no device: nothing to reset


class _OnDevice(torch.Tensor):
    """A host tensor that says it is on a ROCm device: the factory's choice of FusedAdam can
    be seen without one (nothing is stepped)."""

    @property
    def is_cuda(self):
        return True


class _DeviceModel:
    def __init__(self):
        self.ps = [torch.zeros(3).as_subclass(_OnDevice).requires_grad_()]

    def parameters(self):
        return iter(self.ps)


def test_factory_carries_the_option_to_both_optimizer_kinds():
    from mauv.loop_utils import define_optimizers_and_schedulers
    from mauv.optim import FusedAdam
    models = {k: (_DeviceModel() if k == "image_model" else Tiny()) for k in KEYS}
    _, opts, _ = define_optimizers_and_schedulers(
        models, {k: dict(lr=1e-2, grad_accumulation=3) for k in KEYS},
        {k: dict(step_size=5, gamma=0.5) for k in KEYS})
    fused, host = opts["image_model"], opts["multimodal_model"]
    assert type(fused) is FusedAdam and type(host) is torch.optim.Adam
    assert fused.grad_accumulation == 3 and host.grad_accumulation == 3
    assert "grad_accumulation" not in fused.param_groups[0]
    assert "grad_accumulation" not in host.param_groups[0]
    plain = define_optimizers_and_schedulers(
        models, {k: dict(lr=1e-2) for k in KEYS},
        {k: dict(step_size=5, gamma=0.5) for k in KEYS})[1]
    assert plain["image_model"].grad_accumulation is None
    assert plain["multimodal_model"].grad_accumulation is None
    for v in (0, 2.0, True):
        with pytest.raises(ValueError, match="grad_accumulation"):
            define_optimizers_and_schedulers(
                models, {k: dict(lr=1e-2, grad_accumulation=v) for k in KEYS},
                {k: dict(step_size=5, gamma=0.5) for k in KEYS})


# ------------------------------------------------------------------------------- host windows
def _host_pair(K):
    from mauv.loop_utils import define_optimizers_and_schedulers
    torch.manual_seed(0)
    model, ref = Tiny(), Tiny()
    ref.load_state_dict(model.state_dict())
    models = {k: (model if k == "multimodal_model" else Tiny()) for k in KEYS}
    crit, opts, _ = define_optimizers_and_schedulers(
        models, {k: dict(lr=1e-2, weight_decay=1e-5, grad_accumulation=K) for k in KEYS},
        {k: dict(step_size=50, gamma=0.5) for k in KEYS})
    ropt = torch.optim.Adam(ref.parameters(), lr=1e-2, weight_decay=1e-5)
    return model, ref, crit, opts["multimodal_model"], ropt


def _ref_backward(ref, x, b, s, y):
    out = torch.stack([ref(x, b, s) for _ in range(2)]).mean(0)
    loss = F.cross_entropy(out, y)
    loss.backward()
    return loss.detach()


def test_host_model_equals_a_hand_written_accumulation_loop():
    from mauv.train import mc_train_step
    model, ref, crit, opt, ropt = _host_pair(3)
    batches = _batches(7)
    closed = []
    for i, (x, b, s, y) in enumerate(batches):
        last = i == len(batches) - 1
        r = mc_train_step(model, (x, b, s), y, crit, opt, 2, 4, 0.5,
                          close_window=True if last else None)
        loss = _ref_backward(ref, x, b, s, y)
        assert torch.equal(r["loss"], loss)
        closes = i % 3 == 2 or last
        assert r["closed"] is closes and r["stepped"] is closes
        closed.append(r["closed"])
        if closes:
            m = 1 if last else 3
            torch._foreach_mul_([p.grad for p in ref.parameters()], 1.0 / m)
            ropt.step()
            ropt.zero_grad()
            for p, q in zip(model.parameters(), ref.parameters()):
                assert torch.equal(p, q), i
            assert all(p.grad is None or not p.grad.any() for p in model.parameters())
        else:
            for p, q in zip(model.parameters(), ref.parameters()):   # the gradients sum
                assert torch.equal(p.grad, q.grad), i
    assert closed == [False, False, True, False, False, True, True]
    assert ropt.state[next(ref.parameters())]["step"] == 3
    # K=3 does not equal stepping on every batch
    assert not torch.equal(next(model.parameters()), _every_batch(batches))


def _every_batch(batches):
    torch.manual_seed(0)
    ref = Tiny()
    ropt = torch.optim.Adam(ref.parameters(), lr=1e-2, weight_decay=1e-5)
    for x, b, s, y in batches:
        _ref_backward(ref, x, b, s, y)
        ropt.step()
        ropt.zero_grad()
    return next(ref.parameters())


def test_nan_loss_inside_a_window_drops_it_whole(caplog):
    from mauv.train import mc_train_step
    model, ref, crit, opt, ropt = _host_pair(3)
    batches = _batches(6)
    nan = batches[1][0].clone()
    nan[0, 0, 0, 0] = float("nan")
    batches[1] = (nan,) + batches[1][1:]
    before = [p.detach().clone() for p in model.parameters()]
    with caplog.at_level("WARNING"):
        rs = [mc_train_step(model, (x, b, s), y, crit, opt, 2, 4, 0.5)
              for x, b, s, y in batches[:3]]
    assert rs[1] is None and "NaN/Inf loss" in caplog.text
    assert rs[0]["closed"] is False and rs[2]["closed"] is True and rs[2]["stepped"] is False
    for p, q in zip(model.parameters(), before):
        assert torch.equal(p, q)                       # no step
    assert all(p.grad is None or not p.grad.any() for p in model.parameters())
    assert not opt.state                               # Adam never ran
    # the next window steps as if the dropped one had not been
    for x, b, s, y in batches[3:]:
        r = mc_train_step(model, (x, b, s), y, crit, opt, 2, 4, 0.5)
        _ref_backward(ref, x, b, s, y)
    torch._foreach_mul_([p.grad for p in ref.parameters()], 1.0 / 3)
    ropt.step()
    assert r["closed"] is True and r["stepped"] is True
    for p, q in zip(model.parameters(), ref.parameters()):
        assert torch.equal(p, q)


def test_train_epoch_warns_about_a_skipped_step_on_closing_calls_only(caplog):
    from mauv.train import _TrainEpoch

    class Writer:
        def add_scalar(self, *a):
            pass

    labels = torch.tensor([0, 1])
    t, f = torch.tensor(True), torch.tensor(False)

    def result(**extra):
        return dict(loss=torch.tensor(1.0), ce=torch.tensor(0.), scaled_kl=torch.tensor(0.),
                    predicted=torch.tensor([0, 0]), ok_loss=t, stepped=f, **extra)

    ep = _TrainEpoch(0, Writer())
    with caplog.at_level("WARNING"):
        ep.add(0, result(closed=False), labels)
        ep.add(1, result(closed=False), labels)
        ep.flush()
    assert "Skipping optimizer step" not in caplog.text and ep.total == 4
    with caplog.at_level("WARNING"):
        ep.add(2, result(closed=True), labels)
        ep.flush()
    assert caplog.text.count("Skipping optimizer step") == 1 and ep.total == 6


def test_unimodal_loop_accumulates_on_the_host(tmp_path, monkeypatch):
    """train_unimodal_model with K=2 over 3 batches: zero_grad at a window's start only, one
    multiply by 1 / m at the close (the loader's last batch closes a window of one)."""
    import Multimodal_AUV.train.unimodal as um
    from tests.helpers import ListLoader, NullWriter
    monkeypatch.setattr(um, "get_kl_loss", lambda model: torch.tensor(0.05))

    class Uni(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.f = torch.nn.Linear(3 * 8 * 8, 3)

        def forward(self, x):
            return self.f(x.flatten(1))
    torch.manual_seed(0)
    model, ref = Uni(), Uni()
    ref.load_state_dict(model.state_dict())
    batches = [{"main_image": x, "label": y} for x, _, _, y in _batches(3)]
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    opt.grad_accumulation = 2
    um.train_unimodal_model(
        model, ListLoader(batches, 4), torch.nn.CrossEntropyLoss(), opt, epoch=0,
        total_num_epochs=2, num_mc=2, sum_writer=NullWriter(), device=torch.device("cpu"),
        model_type="image", csv_path=str(tmp_path / "uni.csv"))
    ropt = torch.optim.Adam(ref.parameters(), lr=1e-2)
    for window in ([0, 1], [2]):
        ropt.zero_grad()
        for i in window:
            b = batches[i]
            out = torch.stack([ref(b["main_image"]) for _ in range(2)]).mean(0)
            (F.cross_entropy(out, b["label"]) + 0.5 * (torch.tensor(0.05) / 4)).backward()
        torch._foreach_mul_([p.grad for p in ref.parameters()], 1.0 / len(window))
        ropt.step()
    assert ropt.state[ref.f.weight]["step"] == 2
    for p, q in zip(model.parameters(), ref.parameters()):
        assert torch.equal(p, q)
