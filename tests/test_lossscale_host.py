"""Dynamic loss scaling, the parts that need no GPU: ``mauv.amp.LossScaler``'s argument checks and
its state dict against ``torch.amp.GradScaler("cpu")``'s, FusedAdam's ``loss_scale`` option (a
plain attribute: no ``param_groups`` key, not in the optimizer state), the C-ABI of
``mauv_adam_step_ex_scaled`` (exported, declared, bound; every documented argument error answers
before any launch), and a host model trained through ``define_optimizers_and_schedulers(
loss_scale=...)`` + ``mc_train_step`` with an inf forced into one gradient on two batches, which
must equal a hand-written ``torch.amp.GradScaler("cpu")`` loop bit for bit, parameters and the
(scale, growth tracker) sequence alike."""
import ctypes
import math
import re

import pytest
import torch
import torch.nn.functional as F

from tests.test_abi_host import HEADER, header_functions
from tests.test_gradclip_host import Tiny, _batches, _params

NEW = "mauv_adam_step_ex_scaled"
KEYS = ("image_model", "bathy_model", "sss_model", "multimodal_model")


# ------------------------------------------------------------------------- options and state
@pytest.mark.parametrize("kw", [
    dict(init_scale=0), dict(init_scale=-1.0), dict(init_scale=float("inf")),
    dict(init_scale=float("nan")), dict(init_scale="1"), dict(init_scale=True),
    dict(init_scale=1e39), dict(growth_factor=1.0), dict(growth_factor=0.5),
    dict(backoff_factor=1.0), dict(backoff_factor=0.0), dict(backoff_factor=-0.5),
    dict(growth_interval=0), dict(growth_interval=-1), dict(growth_interval=2.5),
    dict(growth_interval=2 ** 31),
], ids=lambda kw: "+".join(f"{k}={v}" for k, v in kw.items()))
def test_bad_scaler_values_raise(kw):
    from mauv.amp import LossScaler
    with pytest.raises(ValueError):
        LossScaler(**kw)


@pytest.mark.parametrize("bad", [0, -2.0, float("nan"), float("inf"), "static", True,
                                 torch.tensor(2.0), [1024]])
def test_bad_loss_scale_option_raises(bad):
    from mauv.optim import FusedAdam, FusedAdamW
    for cls in (FusedAdam, FusedAdamW):
        with pytest.raises(ValueError):
            cls(_params(), loss_scale=bad)
    opt = FusedAdam(_params())
    with pytest.raises(ValueError):
        opt.loss_scale = bad
    assert opt.loss_scale is None


def test_option_is_an_attribute_out_of_groups_and_state():
    from mauv.amp import LossScaler
    from mauv.optim import FusedAdam, FusedAdamW
    assert FusedAdam(_params()).loss_scale is None
    dyn = FusedAdam(_params(), lr=1e-3, loss_scale="dynamic")
    assert isinstance(dyn.loss_scale, LossScaler) and dyn.loss_scale.dynamic
    assert dyn.loss_scale.state_dict() == torch.amp.GradScaler("cpu").state_dict()
    static = FusedAdamW(_params(), loss_scale=1024)
    assert not static.loss_scale.dynamic and static.loss_scale.get_scale() == 1024.0
    mine = LossScaler(init_scale=4.0, growth_interval=3)
    opt = FusedAdam(_params(), loss_scale=mine)
    assert opt.loss_scale is mine
    for o, ref in ((dyn, torch.optim.Adam(_params(), lr=1e-3)),
                   (static, torch.optim.AdamW(_params()))):
        assert list(o.param_groups[0]) == list(ref.param_groups[0])
        sd = o.state_dict()
        assert set(sd) == {"state", "param_groups"}
        assert not any("scale" in k for g in sd["param_groups"] for k in g)
        ref.load_state_dict(sd)
        o.load_state_dict(ref.state_dict())
        assert o.loss_scale is not None            # loading a state leaves the option alone
    opt.loss_scale = None                          # reassigned between steps
    assert opt.loss_scale is None and opt._scaler() is None
    off = LossScaler(enabled=False)
    opt.loss_scale = off
    assert opt.loss_scale is off and opt._scaler() is None
    assert off.get_scale() == 1.0 and off.state_dict() == {}
    t = torch.ones(())
    assert off.scale(t) is t


def test_scaler_round_trips_a_torch_grad_scaler_state():
    from mauv.amp import LossScaler
    gs = torch.amp.GradScaler("cpu", init_scale=2.0 ** 10, growth_factor=4.0, backoff_factor=0.25,
                              growth_interval=7)
    sd = gs.state_dict()
    sd["_growth_tracker"] = 3
    ls = LossScaler()
    ls.load_state_dict(sd)
    assert ls.state_dict() == sd
    assert list(ls.state_dict()) == list(sd)       # torch's keys, torch's order
    assert ls.get_scale() == 1024.0 and ls.get_growth_tracker() == 3
    assert (ls.get_growth_factor(), ls.get_backoff_factor(), ls.get_growth_interval()) == \
        (4.0, 0.25, 7)
    back = torch.amp.GradScaler("cpu")
    back.load_state_dict(ls.state_dict())
    assert back.state_dict() == sd
    with pytest.raises(RuntimeError):
        ls.load_state_dict({})
    with pytest.raises(ValueError):
        ls.load_state_dict(dict(sd, growth_factor=1.0))
    assert ls.state_dict() == sd                   # a refused load changes nothing
    ls.update()                                    # nothing to do
    assert ls.state_dict() == sd
    ls.update(64.0)
    assert ls.get_scale() == 64.0 and ls.get_growth_tracker() == 3


def test_scaler_step_takes_a_fused_adam_only():
    from mauv.amp import LossScaler
    from mauv.optim import FusedAdam
    ls = LossScaler()
    with pytest.raises(TypeError, match="GradScaler"):
        ls.step(torch.optim.Adam(_params()))
    with pytest.raises(ValueError, match="another"):
        ls.step(FusedAdam(_params(), loss_scale="dynamic"))
    with pytest.raises(TypeError, match="ROCm"):
        ls.scale(torch.ones(()))


def test_scaled_step_refuses_what_the_gated_form_cannot_take():
    """More than 8 groups, or parameters with different step counts: a ValueError that says so,
    raised before anything touches a device — never a step on scaled gradients."""
    from mauv.optim import FusedAdam
    ps = [torch.zeros(1, requires_grad=True) for _ in range(9)]
    for p in ps:
        p.grad = torch.ones(1)
    opt = FusedAdam([dict(params=[p]) for p in ps], loss_scale=2.0)
    with pytest.raises(ValueError, match="at most 8 parameter groups"):
        opt.step()
    opt = FusedAdam(ps[:2], loss_scale=2.0)
    opt.state[ps[0]]["step"] = torch.tensor(3.0)
    opt.state[ps[1]]["step"] = torch.tensor(5.0)
    with pytest.raises((ValueError, TypeError)) as e:
        opt.step()
    # (host gradients are refused first; on a device the step counts are)
    assert "ROCm gradients" in str(e.value) or "one step count" in str(e.value)
    assert all(torch.equal(p, torch.zeros(1)) for p in ps)


# ------------------------------------------------------------------------------------- ABI
def test_entry_exported_declared_bound_and_struct_is_32_bytes():
    from mauv import amp
    from mauv._lib import LIB_PATH, SIGNATURES, MauvLossScale, lib
    assert hasattr(ctypes.CDLL(LIB_PATH), NEW) and NEW in header_functions() and NEW in SIGNATURES
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    protos = dict(re.findall(r"(mauv_\w+)\(([^)]*)\)\s*;", txt))
    assert len(SIGNATURES[NEW]) == protos[NEW].count(",") + 1 == 7
    assert lib.mauv_abi_version() == 4
    body = re.search(r"typedef struct MauvLossScale \{(.*?)\} MauvLossScale;", txt, re.S).group(1)
    names = [n.strip() for decl in body.split(";") if decl.strip()
             for n in decl.strip().split(None, 1)[1].split(",")]
    assert names == [f for f, _ in MauvLossScale._fields_]
    assert ctypes.sizeof(MauvLossScale) == 32 == 4 * amp.LS_WORDS
    assert MauvLossScale.scale.offset == 4 * amp.LS_SCALE == 0
    assert MauvLossScale.unscale.offset == 4 * amp.LS_UNSCALE
    assert MauvLossScale.growth_factor.offset == 4 * amp.LS_GROWTH
    assert MauvLossScale.backoff_factor.offset == 4 * amp.LS_BACKOFF
    assert MauvLossScale.growth_interval.offset == 4 * amp.LS_INTERVAL == 16
    assert MauvLossScale.growth_tracker.offset == 4 * amp.LS_TRACKER
    assert MauvLossScale.overflows.offset == 4 * amp.LS_OVERFLOWS
    assert MauvLossScale.growths.offset == 4 * amp.LS_GROWTHS == 28
    # the entries this one joins are as they were
    assert len(SIGNATURES["mauv_adam_step_ex"]) == 7 and len(SIGNATURES["mauv_adam_step_gated"]) == 9


def test_argument_errors_answer_without_a_device():
    """The checks come before any launch (this process has no GPU: a launch would fail
    differently): null table / groups / gate, n outside 1..65535, group count outside 1..8."""
    from mauv._lib import lib, MauvAdamGroup, MauvLossScale
    arr = (MauvAdamGroup * 8)()
    table = (ctypes.c_longlong * 7)()
    gate = (ctypes.c_int * 16)()
    ls = MauvLossScale(scale=2.0)
    tab, grp, gp, lp = (ctypes.addressof(x) for x in (table, arr, gate, ls))
    cases = [(None, 1, grp, 1, gp), (tab, 0, grp, 1, gp), (tab, -1, grp, 1, gp),
             (tab, 65536, grp, 1, gp), (tab, 1, None, 1, gp), (tab, 1, grp, 0, gp),
             (tab, 1, grp, 9, gp), (tab, 1, grp, 1, None)]
    for t, n, g, ng, gt in cases:
        for scaler in (lp, None):
            assert lib.mauv_adam_step_ex_scaled(t, n, g, ng, gt, scaler, None) == -1, (n, ng)
            assert b"adam_step_ex_scaled" in lib.mauv_last_error()
    assert list(gate) == [0] * 16 and ls.scale == 2.0 and ls.overflows == 0


# ---------------------------------------------------------------------------------- factory
def _inf_on(param, batches_with_inf, counter):
    """A gradient hook that forces an inf into ``param``'s gradient on the chosen batches (the
    hook runs inside backward: before GradScaler.unscale_ in either loop)."""
    def hook(g):
        i = counter["i"]
        if i in batches_with_inf:
            g = g.clone()
            g.view(-1)[1] = float("inf")
        return g
    param.register_hook(hook)


def test_factory_host_model_equals_a_grad_scaler_loop():
    from mauv.amp import LossScaler
    from mauv.loop_utils import define_optimizers_and_schedulers
    from mauv.train import mc_train_step
    torch.manual_seed(0)
    model, ref = Tiny(), Tiny()
    ref.load_state_dict(model.state_dict())
    models = {k: (model if k == "multimodal_model" else Tiny()) for k in KEYS}
    kw = dict(lr=1e-2, weight_decay=1e-5, max_grad_norm=0.05,
              loss_scale=LossScaler(init_scale=2.0 ** 16, growth_interval=2))
    crit, opts, _ = define_optimizers_and_schedulers(
        models, {k: dict(kw) for k in KEYS}, {k: dict(step_size=50, gamma=0.5) for k in KEYS})
    opt = opts["multimodal_model"]
    assert type(opt) is torch.optim.Adam and isinstance(opt.grad_scaler, torch.amp.GradScaler)
    assert "loss_scale" not in opt.param_groups[0]
    assert len({id(o.grad_scaler) for o in opts.values()}) == 4   # one scaler per optimizer
    ropt = torch.optim.Adam(ref.parameters(), lr=1e-2, weight_decay=1e-5)
    rs = torch.amp.GradScaler("cpu", init_scale=2.0 ** 16, growth_interval=2)
    bad = {2, 5}
    at = {"i": 0}
    _inf_on(model.out.weight, bad, at)
    _inf_on(ref.out.weight, bad, at)
    seq, want, used = [], [], []
    for i, (x, b, s, y) in enumerate(_batches(8)):
        at["i"] = i
        r = mc_train_step(model, (x, b, s), y, crit, opt, 2, 4, 0.5)
        seq.append((opt.grad_scaler.get_scale(), opt.grad_scaler._get_growth_tracker()))
        used.append(float(r["loss_scale"]))
        out = torch.stack([ref(x, b, s) for _ in range(2)]).mean(0)
        loss = F.cross_entropy(out, y)
        rs.scale(loss).backward()
        rs.unscale_(ropt)
        finite = all(torch.isfinite(p.grad).all() for p in ref.parameters())
        if finite:
            total = torch.nn.utils.clip_grad_norm_(ref.parameters(), 0.05)
        rs.step(ropt)
        rs.update()
        ropt.zero_grad()
        want.append((rs.get_scale(), rs._get_growth_tracker()))
        assert r["stepped"] == finite == (i not in bad)
        assert torch.equal(r["loss"], loss.detach())            # reported unscaled
        if finite:
            assert torch.equal(r["grad_norm"], total) and total > 0.05
        else:
            assert "grad_norm" not in r
    S = 65536.0
    assert want == [(S, 1), (2 * S, 0), (S, 0), (S, 1), (2 * S, 0), (S, 0), (S, 1), (2 * S, 0)]
    assert seq == want
    assert used == [S, S, 2 * S, S, S, 2 * S, S, S]
    for p, q in zip(model.parameters(), ref.parameters()):
        assert torch.equal(p, q)
    assert all(p.grad is None or not p.grad.any() for p in model.parameters())
    # "dynamic" and a disabled scaler; a static scale needs the device scaler
    opts = define_optimizers_and_schedulers(
        models, {k: dict(lr=1e-2, loss_scale="dynamic") for k in KEYS},
        {k: dict(step_size=5, gamma=0.5) for k in KEYS})[1]
    assert opts["image_model"].grad_scaler.state_dict() == torch.amp.GradScaler("cpu").state_dict()
    opts = define_optimizers_and_schedulers(
        models, {k: dict(lr=1e-2, loss_scale=LossScaler(enabled=False)) for k in KEYS},
        {k: dict(step_size=5, gamma=0.5) for k in KEYS})[1]
    assert opts["image_model"].grad_scaler is None
    x, b, s, y = _batches(1, seed=1)[0]
    assert "loss_scale" not in mc_train_step(model, (x, b, s), y, crit, opts["multimodal_model"],
                                             2, 4, 0.5)
    for v in (1024.0, -1.0, "on"):
        with pytest.raises(ValueError, match="loss_scale"):
            define_optimizers_and_schedulers(
                models, {k: dict(lr=1e-2, loss_scale=v) for k in KEYS},
                {k: dict(step_size=5, gamma=0.5) for k in KEYS})


def test_train_epoch_logs_the_loss_scale_and_the_overflow(caplog):
    from mauv.train import _TrainEpoch

    class Writer:
        def __init__(self):
            self.rows = []

        def add_scalar(self, tag, value, step):
            self.rows.append((tag, value, step))

    labels = torch.tensor([0, 1])

    def result(loss, **extra):
        return dict(loss=torch.tensor(loss), ce=torch.tensor(0.), scaled_kl=torch.tensor(0.),
                    predicted=torch.tensor([0, 0]), **extra)

    w = Writer()
    ep = _TrainEpoch(0, w)
    t, f = torch.tensor(True), torch.tensor(False)
    ep.add(0, result(1.0, ok_loss=t, stepped=t, loss_scale=torch.tensor(256.0)), labels)
    assert w.rows == []                        # settled when the next batch has been issued
    ep.add(1, result(2.0, ok_loss=t, stepped=f, loss_scale=torch.tensor(512.0)), labels)
    assert w.rows == [("Loss/train", 1.0, 0), ("LossScale/train", 256.0, 0)]
    with caplog.at_level("WARNING"):
        ep.flush()
    assert w.rows[2:] == [("Loss/train", 2.0, 1), ("LossScale/train", 512.0, 1)]
    assert "overflow at loss scale 512" in caplog.text
    assert math.isclose(ep.total_loss, 3.0)    # the skipped step's batch still counts


def test_unimodal_loop_drives_a_host_grad_scaler(tmp_path, monkeypatch):
    """train_unimodal_model steps the optimizer itself: a host optimizer carrying a GradScaler
    is driven there too, equal to a hand-written GradScaler loop bit for bit."""
    import Multimodal_AUV.train.unimodal as um
    from mauv.amp import LossScaler, host_grad_scaler
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
    batches = [{"main_image": x, "label": y} for x, _, _, y in _batches(4)]
    kw = dict(init_scale=2.0 ** 10, growth_interval=2)
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    opt.grad_scaler = host_grad_scaler(LossScaler(**kw))
    at = {"i": 0}
    _inf_on(model.f.weight, {1}, at)
    _inf_on(ref.f.weight, {1}, at)

    class Loader(ListLoader):
        def __iter__(self):
            for i, b in enumerate(self.batches):
                at["i"] = i
                yield b
    acc, loss = um.train_unimodal_model(
        model, Loader(batches, 4), torch.nn.CrossEntropyLoss(), opt, epoch=0, total_num_epochs=2,
        num_mc=2, sum_writer=NullWriter(), device=torch.device("cpu"), model_type="image",
        csv_path=str(tmp_path / "uni.csv"))
    assert math.isfinite(loss) and loss > 0          # reported unscaled
    ropt = torch.optim.Adam(ref.parameters(), lr=1e-2)
    rs = torch.amp.GradScaler("cpu", **kw)
    for i, b in enumerate(batches):
        at["i"] = i
        ropt.zero_grad()
        out = torch.stack([ref(b["main_image"]) for _ in range(2)]).mean(0)
        rs.scale(F.cross_entropy(out, b["label"]) + 0.5 * (torch.tensor(0.05) / 4)).backward()
        rs.step(ropt)
        rs.update()
    assert (rs.get_scale(), rs._get_growth_tracker()) == (1024.0, 0)   # 1024, 512, 512, 1024
    assert opt.grad_scaler.state_dict() == rs.state_dict()
    for p, q in zip(model.parameters(), ref.parameters()):
        assert torch.equal(p, q)


def test_factory_copies_a_scaler_instance_per_optimizer():
    """One LossScaler instance in the settings of several optimizers: each gets a copy (settings
    and state), so no two models share a scale; strings, numbers and None pass through."""
    from mauv.amp import LossScaler, own_loss_scaler
    src = LossScaler(init_scale=4.0, growth_factor=3.0, backoff_factor=0.25, growth_interval=3)
    src.load_state_dict(dict(src.state_dict(), _growth_tracker=2))
    a, b = own_loss_scaler(src), own_loss_scaler(src)
    assert a is not src and a is not b and a.dynamic and a.is_enabled()
    assert a.state_dict() == b.state_dict() == src.state_dict()
    static = own_loss_scaler(LossScaler(init_scale=8.0, dynamic=False, enabled=False))
    assert not static.dynamic and not static.is_enabled()
    assert own_loss_scaler(None) is None
    assert own_loss_scaler("dynamic").state_dict() == LossScaler().state_dict()
    assert not own_loss_scaler(1024).dynamic
    with pytest.raises(ValueError, match="loss_scale"):
        own_loss_scaler("on")
