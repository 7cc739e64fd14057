"""Global-norm gradient clipping, the parts that need no GPU: FusedAdam's ``max_grad_norm`` /
``grad_norm_type`` options, the C-ABI of csrc/gradnorm.hip (exported, declared, bound; every
documented argument error answers before any launch), and a host model trained through
``define_optimizers_and_schedulers`` + ``mc_train_step`` with the option set, which must equal a
manual loop of ``torch.nn.utils.clip_grad_norm_`` before ``torch.optim.Adam.step()`` bit for bit."""
import ctypes
import math
import re

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests.test_abi_host import HEADER, header_functions

NEW = ("mauv_grad_norm_workspace_bytes", "mauv_grad_norm", "mauv_grad_clip")


def _params():
    return [nn.Parameter(torch.zeros(3)), nn.Parameter(torch.zeros(2, 2))]


def test_options_accepted_and_kept_out_of_groups_and_state():
    from mauv.optim import FusedAdam, FusedAdamW
    opt = FusedAdam(_params(), lr=1e-3, max_grad_norm=1.0, grad_norm_type=float("inf"))
    assert opt.max_grad_norm == 1.0 and opt.grad_norm_type == math.inf
    assert opt.last_grad_norm is None
    ref = torch.optim.Adam(_params(), lr=1e-3)
    assert list(opt.param_groups[0]) == list(ref.param_groups[0])
    sd = opt.state_dict()
    assert "max_grad_norm" not in sd and all("max_grad_norm" not in g for g in sd["param_groups"])
    ref.load_state_dict(sd)
    opt.load_state_dict(ref.state_dict())
    assert opt.max_grad_norm == 1.0            # loading a state leaves the option alone
    w = FusedAdamW(_params(), max_grad_norm=2, grad_norm_type=2)
    assert w.max_grad_norm == 2.0 and w.grad_norm_type == 2.0
    assert list(w.param_groups[0]) == list(torch.optim.AdamW(_params()).param_groups[0])
    d = FusedAdam(_params())
    assert d.max_grad_norm is None and d.grad_norm_type == 2.0
    d.max_grad_norm = 0.5                      # reassigned between steps
    d.max_grad_norm = None
    d.grad_norm_type = float("inf")
    with pytest.raises(ValueError):
        d.max_grad_norm = 0
    with pytest.raises(ValueError):
        d.grad_norm_type = 3
    assert d.max_grad_norm is None and d.grad_norm_type == math.inf


@pytest.mark.parametrize("bad", [0, -1, float("nan"), float("inf"), torch.tensor(1.0), "1", True])
def test_bad_max_grad_norm_raises(bad):
    from mauv.optim import FusedAdam, FusedAdamW
    for cls in (FusedAdam, FusedAdamW):
        with pytest.raises(ValueError, match="max_grad_norm"):
            cls(_params(), max_grad_norm=bad)


@pytest.mark.parametrize("bad", [1, 1.0, 0, 3, float("nan"), -float("inf"), torch.tensor(2.0), None])
def test_bad_grad_norm_type_raises(bad):
    from mauv.optim import FusedAdam
    with pytest.raises(ValueError, match="grad_norm_type"):
        FusedAdam(_params(), max_grad_norm=1.0, grad_norm_type=bad)


def test_unknown_option_still_raises():
    from mauv.optim import FusedAdam
    with pytest.raises(ValueError, match="nesterov"):
        FusedAdam(_params(), max_grad_norm=1.0, nesterov=True)


def test_new_entry_points_exported_declared_bound():
    from mauv._lib import LIB_PATH, SIGNATURES, lib
    raw = ctypes.CDLL(LIB_PATH)
    names = header_functions()
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    protos = dict(re.findall(r"(mauv_\w+)\(([^)]*)\)\s*;", txt))
    for n in NEW:
        assert hasattr(raw, n) and n in names and n in SIGNATURES, n
        assert len(SIGNATURES[n]) == protos[n].count(",") + 1, n
    assert "MauvSpan" in txt and lib.mauv_abi_version() == 4
    assert lib.mauv_grad_norm_workspace_bytes.restype is ctypes.c_longlong


def test_gate_is_still_64_bytes_with_the_named_words():
    """MauvStepGate as include/mauv.h declares it, restated as a ctypes Structure: the four new
    words sit at 10..13 (mauv.optim's indices), 14 and 15 stay reserved."""
    from mauv import optim
    txt = open(HEADER).read()
    body = re.search(r"typedef struct MauvStepGate \{(.*?)\} MauvStepGate;", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = decl.split(None, 1)
        ct = {"int": ctypes.c_int, "float": ctypes.c_float}[ctype]
        for name in names.split(","):
            name = name.strip()
            m = re.fullmatch(r"(\w+)\[(\d+)\]", name)
            fields.append((m.group(1), ct * int(m.group(2))) if m else (name, ct))

    class Gate(ctypes.Structure):
        _fields_ = fields

    assert ctypes.sizeof(Gate) == 64 == 4 * optim.GATE_WORDS
    assert Gate.max_norm.offset == 4 * optim.G_MAX_NORM == 40
    assert Gate.grad_norm.offset == 4 * optim.G_GRAD_NORM == 44
    assert Gate.clip_coef.offset == 4 * optim.G_CLIP_COEF == 48
    assert Gate.norm_kind.offset == 4 * optim.G_NORM_KIND == 52
    assert Gate.reserved.offset == 56 and optim.G_SCRATCH == 15
    assert dict(fields)["max_norm"] is ctypes.c_float and dict(fields)["norm_kind"] is ctypes.c_int


def test_argument_errors_answer_without_a_device():
    """Every documented argument error returns < 0 before any launch (this process has no GPU:
    a launch would fail differently) and names its entry point in mauv_last_error()."""
    from mauv._lib import lib
    spans = (ctypes.c_longlong * 2)(0, 0)      # never dereferenced: the checks come first
    ws = (ctypes.c_double * 8192)()
    out = ctypes.c_float(0)
    cnt = ctypes.c_int(0)
    sp, wp, op, cp = (ctypes.addressof(x) for x in (spans, ws, out, cnt))

    def err(rc, who):
        assert rc < 0
        assert who in lib.mauv_last_error(), lib.mauv_last_error()

    for n in (0, -1, 65536):
        err(lib.mauv_grad_norm_workspace_bytes(n), b"grad_norm_workspace_bytes")
        err(lib.mauv_grad_norm(sp, n, 0, wp, op, cp, None), b"grad_norm")
        err(lib.mauv_grad_clip(sp, n, op, 1.0, None), b"grad_clip")
    err(lib.mauv_grad_norm(None, 1, 0, wp, op, cp, None), b"grad_norm")
    err(lib.mauv_grad_norm(sp, 1, 0, None, op, cp, None), b"grad_norm")
    err(lib.mauv_grad_norm(sp, 1, 0, wp, None, cp, None), b"grad_norm")
    for kind in (-1, 2):
        err(lib.mauv_grad_norm(sp, 1, kind, wp, op, cp, None), b"grad_norm")
    err(lib.mauv_grad_clip(None, 1, op, 1.0, None), b"grad_clip")
    err(lib.mauv_grad_clip(sp, 1, None, 1.0, None), b"grad_clip")
    for c in (0.0, -1.0, float("nan"), float("inf")):
        err(lib.mauv_grad_clip(sp, 1, op, c, None), b"grad_clip")
    assert out.value == 0 and cnt.value == 0
    # the sizing helper: a double and a flag per block, blocks for one span >= 256 CUs' worth
    one = lib.mauv_grad_norm_workspace_bytes(1)
    assert one >= 256 * 12 and one % 8 == 0
    for n in (2, 696, 65535):
        assert lib.mauv_grad_norm_workspace_bytes(n) >= 12 * n


class Tiny(nn.Module):
    """A host model: no mc_forward (tests/test_dropin_cpu.py)."""

    def __init__(self):
        super().__init__()
        self.a = nn.Linear(3 * 8 * 8, 4)
        self.b = nn.Linear(3 * 8 * 8, 4)
        self.c = nn.Linear(1 * 8 * 8, 4)
        self.out = nn.Linear(12, 3)

    def forward(self, x, bathy, sss):
        f = torch.cat([self.a(x.flatten(1)), self.b(bathy.flatten(1)), self.c(sss.flatten(1))], 1)
        return self.out(f)


def _batches(n, B=4, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(B, 3, 8, 8, generator=g) * 30, torch.rand(B, 3, 8, 8, generator=g),
             torch.rand(B, 1, 8, 8, generator=g), torch.randint(0, 3, (B,), generator=g))
            for _ in range(n)]


@pytest.mark.parametrize("norm_type", [2.0, float("inf")])
def test_host_model_clips_through_mc_train_step(norm_type):
    from mauv.loop_utils import define_optimizers_and_schedulers
    from mauv.train import mc_train_step
    torch.manual_seed(0)
    model, ref = Tiny(), Tiny()
    ref.load_state_dict(model.state_dict())
    c = 0.05
    keys = ("image_model", "bathy_model", "sss_model", "multimodal_model")
    models = {k: (model if k == "multimodal_model" else Tiny()) for k in keys}
    kw = dict(lr=1e-2, weight_decay=1e-5, max_grad_norm=c, grad_norm_type=norm_type)
    crit, opts, _ = define_optimizers_and_schedulers(
        models, {k: dict(kw) for k in keys}, {k: dict(step_size=5, gamma=0.5) for k in keys})
    opt = opts["multimodal_model"]
    assert type(opt) is torch.optim.Adam
    assert opt.max_grad_norm == c and opt.grad_norm_type == norm_type
    assert not {"max_grad_norm", "grad_norm_type"} & set(opt.param_groups[0])
    ropt = torch.optim.Adam(ref.parameters(), lr=1e-2, weight_decay=1e-5)
    for x, b, s, y in _batches(2):
        r = mc_train_step(model, (x, b, s), y, crit, opt, 2, 4, 0.5)
        out = torch.stack([ref(x, b, s) for _ in range(2)]).mean(0)
        F.cross_entropy(out, y).backward()
        total = torch.nn.utils.clip_grad_norm_(ref.parameters(), c, norm_type)
        assert total > c                       # clipping is active
        ropt.step()
        ropt.zero_grad()
        assert r["stepped"] and torch.equal(r["grad_norm"], total)
    for p, q in zip(model.parameters(), ref.parameters()):
        assert torch.equal(p, q)
    # without the option nothing new is reported
    plain = define_optimizers_and_schedulers(
        models, {k: dict(lr=1e-2) for k in keys},
        {k: dict(step_size=5, gamma=0.5) for k in keys})[1]["multimodal_model"]
    x, b, s, y = _batches(1, seed=1)[0]
    assert "grad_norm" not in mc_train_step(model, (x, b, s), y, crit, plain, 2, 4, 0.5)
    with pytest.raises(ValueError, match="max_grad_norm"):
        define_optimizers_and_schedulers(
            models, {k: dict(lr=1e-2, max_grad_norm=-1.0) for k in keys},
            {k: dict(step_size=5, gamma=0.5) for k in keys})


def test_train_epoch_logs_grad_norm_one_batch_late():
    """_TrainEpoch writes GradNorm/train right after the batch's Loss/train when the result
    carries grad_norm, and nothing new otherwise (the log order is unchanged)."""
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
    ep.add(0, result(1.0, grad_norm=torch.tensor(3.5)), labels)
    assert w.rows == []                        # settled when the next batch has been issued
    ep.add(1, result(2.0, grad_norm=torch.tensor(float("nan"))), labels)
    assert w.rows == [("Loss/train", 1.0, 0), ("GradNorm/train", 3.5, 0)]
    ep.flush()
    assert [r[0] for r in w.rows[2:]] == ["Loss/train", "GradNorm/train"] and math.isnan(w.rows[3][1])
    w = Writer()
    ep = _TrainEpoch(0, w)
    ep.add(0, result(1.0), labels)
    ep.flush()
    assert w.rows == [("Loss/train", 1.0, 0)]


def test_unimodal_loop_clips_a_host_model(tmp_path, monkeypatch):
    """train_unimodal_model steps the optimizer itself: a host optimizer carrying the option is
    clipped there too, equal to a manual clip_grad_norm_ + Adam loop bit for bit."""
    import Multimodal_AUV.train.unimodal as um
    from tests.helpers import ListLoader, NullWriter
    monkeypatch.setattr(um, "get_kl_loss", lambda model: torch.tensor(0.05))

    class Uni(nn.Module):
        def __init__(self):
            super().__init__()
            self.f = nn.Linear(3 * 8 * 8, 3)

        def forward(self, x):
            return self.f(x.flatten(1))
    torch.manual_seed(0)
    model, ref = Uni(), Uni()
    ref.load_state_dict(model.state_dict())
    batches = [{"main_image": x, "label": y} for x, _, _, y in _batches(2)]
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    opt.max_grad_norm, opt.grad_norm_type = 0.05, 2.0
    csv_path = tmp_path / "uni.csv"
    um.train_unimodal_model(model, ListLoader(batches, 4), nn.CrossEntropyLoss(), opt, epoch=0,
                            total_num_epochs=2, num_mc=2, sum_writer=NullWriter(),
                            device=torch.device("cpu"), model_type="image",
                            csv_path=str(csv_path))
    ropt = torch.optim.Adam(ref.parameters(), lr=1e-2)
    for b in batches:
        ropt.zero_grad()
        out = torch.stack([ref(b["main_image"]) for _ in range(2)]).mean(0)
        (F.cross_entropy(out, b["label"]) + 0.5 * (torch.tensor(0.05) / 4)).backward()
        assert torch.nn.utils.clip_grad_norm_(ref.parameters(), 0.05) > 0.05
        ropt.step()
    for p, q in zip(model.parameters(), ref.parameters()):
        assert torch.equal(p, q)
