"""FusedAdam — torch.optim.Adam's update for every parameter tensor in one HIP launch.

The reference optimises each model with ``torch.optim.Adam(model.parameters(), lr=...,
weight_decay=...)`` (train/loop_utils.py:45-61), forwarding the caller's optimizer options as
keyword arguments, and steps it after every accepted batch (train/multimodal.py:141-143).
``FusedAdam`` is a drop-in ``torch.optim.Optimizer``: torch.optim.Adam's constructor arguments
(``amsgrad``, ``maximize`` and ``decoupled_weight_decay`` change the update; ``foreach`` and
``fused`` pick torch's implementation, not the maths, and are only kept; ``capturable``,
``differentiable`` and a tensor ``lr`` / betas are rejected), the same ``param_groups`` keys (so
``StepLR`` drives ``lr``), and the same per-parameter state keys ``step`` / ``exp_avg`` /
``exp_avg_sq`` (/ ``max_exp_avg_sq`` with amsgrad) — its ``state_dict()`` loads into
torch.optim.Adam and back.  ``FusedAdamW`` is the same for torch.optim.AdamW.

One parameter group with the three options off steps through ``mauv_adam_step`` over a device
table of (param, grad, exp_avg, exp_avg_sq, numel) rows.  Anything else — options, several
groups — steps through ``mauv_adam_step_ex``: all groups in ONE launch (eight groups per launch),
rows of (param, grad, exp_avg, exp_avg_sq, max_exp_avg_sq, numel, group) and the groups' lr /
betas / eps / weight_decay / flags by value.  Either way the step's tensors, device table and step
count are cached in a ``_Plan``, rebuilt only when a pointer changes.  Parameters whose ``.grad``
is None are skipped, like torch.

``step_gated(gate)`` is the training loop's form (mauv.train.mc_train_step): the decision of
multimodal.py:133-145 — skip on a non-finite loss, skip the step and the zero_grad on
non-finite gradients — is read from a device ``MauvStepGate`` by the kernel, and the Adam
step count lives in that gate, so a training step never waits on the host.  It covers 1 to 8
groups over the model's trainable parameters; frozen ones get no state and no step.

``max_grad_norm`` (None, or a number > 0) with ``grad_norm_type`` (2 or inf) adds global-norm
gradient clipping, ``torch.nn.utils.clip_grad_norm_(all parameters, max_grad_norm)`` ahead of the
update, on the kernels of gradnorm.hip.  Both are plain attributes that may be reassigned between
steps; they are no ``param_groups`` keys and stay out of ``state_dict()``.  ``step()`` scans the
norm, clips in place and updates, without a host synchronisation.  The gated form scans with
``scan_gated(gate)`` in place of the non-finite count, the gate forms the coefficient and the
Adam kernel multiplies the gradient as it loads it: no extra pass.  ``last_grad_norm`` is the
last step's pre-clip norm (torch's return value) as a 0-dim device tensor, NaN when a gradient
was non-finite.  ``clip_grad_norm_`` below is the same clip as a function with torch's signature.

``loss_scale`` (None, ``"dynamic"``, a number for a static scale, or a ``mauv.amp.LossScaler``)
adds dynamic loss scaling, ``torch.amp.GradScaler``'s algorithm, for f16 training (DESIGN.md
§2.37).  It is a plain attribute like ``max_grad_norm``: no ``param_groups`` key, not in
``state_dict()`` (the scaler has its own).  The caller runs the backward on
``opt.loss_scale.scale(loss)`` (mauv.train does).  The gated form then hands the scaler's device
state to the kernel: the decision skips the step and zeroes the gradients on an overflow, backs
the scale off or grows it, and the kernel multiplies each gradient by 1 / scale ahead of the
clip coefficient; ``last_grad_norm`` is the norm of the unscaled gradients.
``step()`` with a scaler set goes through the same device decision on a gate of its own over the
live parameters (``ok_loss`` = 1): it scans, unscales, clips, steps AND zeroes the gradients
(stepped or skipped, as GradScaler's ``step`` followed by ``zero_grad``), a skipped step does not
advance Adam's step count, and nothing waits on the host.  Where the gated form cannot apply —
parameters with different step counts, more than 8 groups — it raises a ValueError rather than
step on scaled gradients.

``grad_accumulation`` (None, or an integer >= 1) adds gradient accumulation to the gated form
(DESIGN.md §2.39): a plain attribute like ``max_grad_norm``, reassignable between windows, no
``param_groups`` key and not in ``state_dict()``.  With K > 1 ``step_gated(gate)`` closes a window
every K-th call (or when told to, ``close=True``); the other calls queue ``mauv_accum_note`` only:
no scan, no Adam launch.  The closing call is the step: one decision for the window (a window
holding any non-finite loss is dropped whole), the loss scaler moves once per window, and the
kernel multiplies each gradient by 1 / micro-batches between 1 / scale and the clip coefficient,
so the step is Adam on the mean of the micro-batch gradients.  ``zero_grad()`` also abandons the
open window.  The ungated ``step()`` and ``mauv.amp.LossScaler.step(opt)`` in a user's own loop
do not look at the option: such a loop divides its gradients itself.

``ema_decay`` (None, or a number with 0 < d < 1) keeps an exponential moving average (EMA) of the
weights beside Adam, what ``torch.optim.swa_utils.AveragedModel`` with
``get_ema_multi_avg_fn(d)`` or timm's ``ModelEma`` keep: after every step that HAPPENED, and only
then, each parameter's shadow moves towards it, ``e += (1 - d)(p - e)``; the first update copies.
``ema_warmup=True`` caps the decay at ``(1 + n) / (10 + n)`` on update n (timm's warm-up).
``ema_eval`` (default True) tells the training loops to evaluate on the averaged weights.  All
three are plain attributes like ``max_grad_norm``, no ``param_groups`` keys.  The shadow of a
parameter is ``state[p]["ema"]``, created beside ``exp_avg`` as a clone of the parameter (frozen
parameters get none; with the option off the key never appears), so ``state_dict()`` carries the
shadows, and beside them a top-level ``"ema_updates"``; it still loads into torch.optim.Adam and
back.  In the gated form the device decision also forms the weight, in a ``MauvEma`` beside the
gate, and the Adam kernel stores the shadow beside the new parameter it holds in a register — no
extra pass and no host wait; a skipped step (bad loss, non-finite gradients, overflow, dropped
window) moves nothing.  The ungated ``step()``
is decided on the host: its Adam launches are followed by ``mauv_ema_update`` over the same live
parameters at the weight of a host count kept equal to the device rule — ONE EXTRA PASS over
parameters and shadows.  ``step()`` with a loss scaler takes the gated entry, EMA included.
``swap_ema()`` exchanges parameters and shadows in place (``mauv_ema_swap``; no pointer changes,
so no cached table or engine state is invalidated), ``averaged()`` is the context manager that
swaps in and, on exit, back, ``ema_parameters()`` lists ``(p, shadow)``.  While swapped, ``step``,
``step_gated`` and ``state_dict`` raise RuntimeError.  BatchNorm buffers (running statistics) are
not averaged — AveragedModel's default: under the swap the live buffers serve.
"""
import contextlib
import ctypes
import functools
import math
import numbers

import numpy as np
import torch

from . import ops  # noqa: F401  (loads the library)
from ._lib import lib, check, MauvAdamGroup
from .amp import as_loss_scaler

GATE_WORDS = 16          # sizeof(MauvStepGate) / 4 (include/mauv.h)
G_OK_LOSS, G_NONFINITE, G_POISONED, G_MODE, G_STEP, G_STEPPED, G_SKIP_LOSS, G_SKIP_GRAD = range(8)
G_MAX_NORM, G_GRAD_NORM, G_CLIP_COEF, G_NORM_KIND = 10, 11, 12, 13   # fp32, fp32, fp32, int
G_SCRATCH = 15           # a reserved word the training step counts non-finite inputs in
ACC_WORDS = 8            # sizeof(MauvAccum) / 4
A_MICRO, A_BAD_LOSS, A_AVG, A_WINDOWS, A_DROPPED = range(5)   # int, int, fp32, int, int
EMA_WORDS = 8            # sizeof(MauvEma) / 4
E_DECAY, E_WARMUP, E_UPDATES, E_WEIGHT = range(4)             # fp32, int, int, fp32
MAX_GROUPS = 8           # MAUV_ADAM_MAX_GROUPS
F_AMSGRAD, F_MAXIMIZE, F_DECOUPLED = 1, 2, 4
EX = "ex"                # key of the all-groups table / fast entry (group 0 alone keeps key 0)


def _flags(group):
    return (F_AMSGRAD if group["amsgrad"] else 0) | (F_MAXIMIZE if group["maximize"] else 0) | \
        (F_DECOUPLED if group["decoupled_weight_decay"] else 0)


def check_max_grad_norm(v):
    """``max_grad_norm``: None (no clipping) or a finite Python number > 0."""
    if v is None:
        return None
    if isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(v) or v <= 0:
        raise ValueError(f"max_grad_norm must be None or a finite number > 0, got {v!r}")
    return float(v)


def check_grad_norm_type(v):
    """``grad_norm_type``: 2 (the L2 norm) or float("inf") (the largest magnitude)."""
    if isinstance(v, bool) or not isinstance(v, numbers.Real) or v not in (2.0, math.inf):
        raise ValueError(f"grad_norm_type must be 2 or float('inf'), got {v!r}")
    return float(v)


def check_grad_accumulation(v):
    """``grad_accumulation``: None (off) or an integer >= 1 (1 is off too)."""
    if v is None:
        return None
    if isinstance(v, bool) or not isinstance(v, numbers.Integral) or v < 1:
        raise ValueError(f"grad_accumulation must be None or an integer >= 1, got {v!r}")
    return int(v)


def check_ema_decay(v):
    """``ema_decay``: None (no weight EMA) or a Python number with 0 < d < 1."""
    if v is None:
        return None
    if isinstance(v, bool) or not isinstance(v, numbers.Real) or not 0 < v < 1:
        raise ValueError(f"ema_decay must be None or a number with 0 < d < 1, got {v!r}")
    return float(v)


def check_ema_flag(name, v):
    """``ema_warmup`` / ``ema_eval``: a bool."""
    if not isinstance(v, bool):
        raise ValueError(f"{name} must be True or False, got {v!r}")
    return v


def ema_weight(n, decay, warmup):
    """The weight of EMA update number ``n`` (0-based) as the device forms it (adam.hip
    step_gate_kernel): 1 for the first update, else (float)(1 - d) with d the fp32 decay,
    capped at (1 + n) / (10 + n) under the warm-up."""
    if n == 0:
        return 1.0
    d = float(np.float32(decay))
    if warmup:
        d = min(d, (1.0 + n) / (10.0 + n))
    return float(np.float32(1.0 - d))


def _span_rows(grads):
    """[(data_ptr, numel)] of a MauvSpan table over ``grads``: ONE row when they are exactly the
    views of a gradient arena (mauv.engine.GradArena: views at 16-byte steps of one flat buffer
    whose gaps stay zero, so they add nothing to either norm), else one row per tensor."""
    base = grads[0]._base
    if base is not None and getattr(base, "_mauv_gaps_zero", False):
        end = base.data_ptr()
        for g in sorted(grads, key=lambda g: g.data_ptr()):
            if g._base is not base or g.data_ptr() != end:
                break
            end += (g.numel() + 3) // 4 * 16
        else:
            if end == base.data_ptr() + 4 * base.numel():
                return [(base.data_ptr(), base.numel())]
    return [(g.data_ptr(), g.numel()) for g in grads]


class _NormPlan:
    """The device span table and workspace of the norm scan / clip over one set of gradients,
    rebuilt only when a pointer changes (like the Adam tables)."""

    def __init__(self):
        self.rows = self.spans = self.ws = None

    def get(self, rows, device):
        if self.rows != rows or self.spans.device != torch.device(device):
            if len(rows) > 65535:
                raise ValueError("gradient clipping: more than 65535 gradient tensors")
            self.spans = ops.span_table(rows, device)
            self.ws = torch.empty(ops.grad_norm_workspace_bytes(len(rows)), dtype=torch.uint8,
                                  device=device)
            self.rows = rows
        return self.spans, self.ws


def _kind(norm_type):
    return 1 if norm_type == math.inf else 0


def word(struct, i, fp32=False):
    """Word ``i`` of a device struct kept as an int32 tensor (a gate, MauvAccum, MauvEma): a
    one-element view, as int32 or as the fp32 it holds."""
    w = struct[i:i + 1]
    return w.view(torch.float32) if fp32 else w


class _Checked:
    """A plain attribute validated on assignment.  The value lives in the instance ``__dict__``
    and reads as ``default`` before ``__init__`` has set it: ``Optimizer.__init__`` calls
    ``add_param_group``, and unpickling bypasses ``__init__``."""

    def __init__(self, check_fn, default=None):
        self.check_fn, self.default = check_fn, default

    def __set_name__(self, owner, name):
        self.key = "_" + name

    def __get__(self, obj, owner=None):
        return self if obj is None else obj.__dict__.get(self.key, self.default)

    def __set__(self, obj, v):
        obj.__dict__[self.key] = self.check_fn(v)


class _Plan:
    """What one Adam launch set was built over, cached so that the next step over the same
    tensors skips the per-parameter Python work (checks, one .item() per step counter, table
    rows).  It holds strong references to the moment (and shadow) tensors the device table points
    at, and serves only while the state still holds exactly those tensors: a cleared / replaced
    state drops to the slow path instead of writing through stale pointers.  ``layout`` is None
    for the 5-column rows of one plain group (mauv_adam_step / _gated); otherwise the rows have 7
    columns, ``chunks`` lists the launches as (first row, rows, group indices) — at most
    MAX_GROUPS groups each, a row's group column counting within its launch — and, with the
    weight EMA on, ``shadows`` / ``shadow_table`` are the rows' shadow tensors and the device
    table of their pointers.  ``steps`` is the CPU tensor every ``state[p]["step"]`` is a 0-dim
    view of (still float tensors, torch.optim.Adam-compatible), at count ``t``."""
    __slots__ = ("ptrs", "gptrs", "moments", "shadows", "state_id", "t", "table", "steps",
                 "layout", "chunks", "shadow_table", "ident")

    def valid_for(self, opt, live, layout):
        if self.state_id != id(opt.state) or len(self.ptrs) != len(live) or self.layout != layout:
            return False
        if [p.data_ptr() for p in live] != self.ptrs or \
                [p.grad.data_ptr() for p in live] != self.gptrs:
            return False
        if layout is not None and (self.shadows is None) != (opt.ema_decay is None):
            return False
        try:
            for p, mom in zip(live, self.moments):
                st = opt.state[p]
                if st["exp_avg"] is not mom[0] or st["exp_avg_sq"] is not mom[1]:
                    return False
                if len(mom) == 3 and st["max_exp_avg_sq"] is not mom[2]:
                    return False
            for p, sh in zip(live, self.shadows or ()):
                if opt.state[p]["ema"] is not sh:
                    return False
        except KeyError:
            return False
        return True

    def advance(self):
        """The next step count, in the plan and in every parameter's state["step"]."""
        self.t += 1
        self.steps.add_(1.0)
        return self.t


class FusedAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                 amsgrad=False, *, foreach=None, maximize=False, capturable=False,
                 differentiable=False, fused=None, decoupled_weight_decay=False,
                 max_grad_norm=None, grad_norm_type=2.0, loss_scale=None,
                 grad_accumulation=None, ema_decay=None, ema_warmup=False, ema_eval=True,
                 **unsupported):
        for k, v in unsupported.items():
            if v not in (None, False):
                raise ValueError(f"FusedAdam: unsupported option {k}={v}")
        # global-norm gradient clipping (torch.nn.utils.clip_grad_norm_ over every group's
        # gradients before the update): plain attributes, not group keys and not in state_dict()
        self.max_grad_norm = max_grad_norm
        self.grad_norm_type = grad_norm_type
        self.last_grad_norm = None   # 0-dim fp32 device tensor: the last step's pre-clip norm
        self._norm_plan = _NormPlan()
        self._norm_word = None
        self._gate_clip = (0.0, 0)   # (max_norm, norm_kind) the device gate holds
        # dynamic loss scaling (mauv.amp.LossScaler): a plain attribute too
        self.loss_scale = loss_scale
        # gradient accumulation in the gated form: a plain attribute too
        self.grad_accumulation = grad_accumulation
        self._accum = None         # device MauvAccum (int32[8]) beside the gate
        self._accum_micro = 0      # micro-batches of the open window (host count)
        # weight EMA: plain attributes too; the shadows live in the per-parameter state
        self.ema_decay = ema_decay
        self.ema_warmup = ema_warmup
        self.ema_eval = ema_eval
        self._ema = None           # device MauvEma (int32[8]) beside the gate
        self._ema_opts = None      # (decay, warmup) the device struct holds
        self._ema_updates = 0      # EMA updates taken (host count; see _ema_dirty)
        self._ema_dirty = False    # the device count is ahead of the host count (gated steps)
        self._ema_pushed = False   # the device count holds the host count (or is ahead of it)
        self._ema_rows = None      # (key, device MauvEmaRow table) of mauv_ema_update / _swap
        self._ema_swapped = False  # swap_ema(): the parameters hold the averages right now
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                                      amsgrad=amsgrad, maximize=maximize, foreach=foreach,
                                      capturable=capturable, differentiable=differentiable,
                                      fused=fused, decoupled_weight_decay=decoupled_weight_decay))
        # key 0 (one plain group) or EX (all groups) -> the _Plan of the last step, when every
        # live parameter shared one step count; else _split[key] holds one plan per distinct
        # count, by position, and every step takes the slow path
        self._fast = {}
        self._split = {}
        self._gate = None          # device MauvStepGate (int32[16]) of the gated form
        self._gate_dirty = False   # the gate's step count is ahead of state["step"]
        self._gate_params = None
        self._gate_live = None     # [(parameter, group index)] the gate was built over

    max_grad_norm = _Checked(check_max_grad_norm)
    grad_norm_type = _Checked(check_grad_norm_type, 2.0)
    loss_scale = _Checked(as_loss_scaler)   # the optimizer's mauv.amp.LossScaler, or None
    grad_accumulation = _Checked(check_grad_accumulation)
    ema_decay = _Checked(check_ema_decay)
    ema_warmup = _Checked(functools.partial(check_ema_flag, "ema_warmup"), False)
    ema_eval = _Checked(functools.partial(check_ema_flag, "ema_eval"), True)

    def accumulating(self):
        """Gradient accumulation is on (K > 1), or a window opened under it is still open."""
        return (self.grad_accumulation or 1) > 1 or self.__dict__.get("_accum_micro", 0) > 0

    def closes_window(self, close=None):
        """Whether the next ``step_gated`` call closes its window: ``close`` when given, else
        every ``grad_accumulation``-th call (always, when accumulation is off)."""
        if not self.accumulating():
            return True
        if close is not None:
            return bool(close)
        return self._accum_micro + 1 >= (self.grad_accumulation or 1)

    def zero_grad(self, set_to_none=True):
        """torch's ``zero_grad``; it also abandons an open accumulation window: the host count
        and, by a device fill, the window's micro / bad_loss words."""
        super().zero_grad(set_to_none)
        self._accum_micro = 0
        if self._accum is not None:
            self._accum[A_MICRO:A_BAD_LOSS + 1].zero_()

    def _scaler(self):
        """The loss scaler when it is set and enabled, else None."""
        ls = self.loss_scale
        return ls if ls is not None and ls.is_enabled() else None

    def _clip_live(self):
        """The ungated step's clip: norm scan over every group's live gradients, then the
        in-place multiply — two launches of gradnorm.hip, no host synchronisation."""
        grads = [p.grad for g in self.param_groups for p in g["params"] if p.grad is not None]
        if not grads:
            return
        for g in grads:
            if g.dtype != torch.float32 or not g.is_cuda or g.is_sparse or not g.is_contiguous():
                raise TypeError("FusedAdam: dense contiguous fp32 ROCm gradients only")
        dev = grads[0].device
        spans, ws = self._norm_plan.get(_span_rows(grads), dev)
        if self._norm_word is None or self._norm_word.device != dev:
            self._norm_word = torch.zeros(1, device=dev)
        ops.grad_norm(spans, _kind(self.grad_norm_type), ws, self._norm_word)
        ops.grad_clip(spans, self._norm_word, self.max_grad_norm)
        self.last_grad_norm = self._norm_word.clone()[0]

    def _write_gate_clip(self, gate):
        """The gate's max_norm / norm_kind words follow the attributes: a device fill when one
        changed, no host synchronisation."""
        want = (self.max_grad_norm or 0.0, _kind(self.grad_norm_type))
        if self._gate_clip != want:
            word(gate, G_MAX_NORM, fp32=True).fill_(want[0])
            word(gate, G_NORM_KIND).fill_(want[1])
            self._gate_clip = want

    def scan_gated(self, gate, flat=None):
        """With ``max_grad_norm`` set, the gated step's scan: the global norm of the gradients
        into the gate's grad_norm word and their non-finite count into its nonfinite word, in
        one pass (``flat``: the gradient arena every gradient is a view of — one span)."""
        assert gate is self._gate, "scan_gated: use the gate returned by FusedAdam.gate()"
        self._write_gate_clip(gate)
        if flat is not None:
            rows = [(flat.data_ptr(), flat.numel())]
        else:
            rows = _span_rows([p.grad for p, _ in self._gate_live])
        spans, ws = self._norm_plan.get(rows, gate.device)
        ops.grad_norm(spans, _kind(self.grad_norm_type), ws,
                      word(gate, G_GRAD_NORM, fp32=True), word(gate, G_NONFINITE))

    @staticmethod
    def _check_group(group):
        """torch.optim.Adam's own range checks, and the options this optimizer does not take."""
        lr, betas = group["lr"], group["betas"]
        if isinstance(lr, torch.Tensor) or any(isinstance(b, torch.Tensor) for b in betas):
            raise ValueError("FusedAdam: a tensor lr / betas is not supported")
        if group["capturable"] or group["differentiable"]:
            raise ValueError("FusedAdam: capturable / differentiable are not supported")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= group["eps"]:
            raise ValueError(f"Invalid epsilon value: {group['eps']}")
        for i, b in enumerate(betas):
            if not 0.0 <= b < 1.0:
                raise ValueError(f"Invalid beta parameter at index {i}: {b}")
        if not 0.0 <= group["weight_decay"]:
            raise ValueError(f"Invalid weight_decay value: {group['weight_decay']}")

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        self._check_group(self.param_groups[-1])
        if getattr(self, "_gate", None) is not None:   # the gate was built over the old groups
            self._sync_gate()
            self._gate = None
        if hasattr(self, "_fast"):
            self._fast.pop(EX, None)

    def _simple(self):
        """One group, amsgrad / maximize / decoupled off: the mauv_adam_step entry points."""
        return len(self.param_groups) == 1 and _flags(self.param_groups[0]) == 0

    def _layout(self, pairs):
        """What an all-groups table depends on besides the pointers: each row's group and every
        group's option flags (amsgrad adds a column)."""
        return tuple(gi for _, gi in pairs), tuple(_flags(g) for g in self.param_groups)

    def _count(self, p):
        """The parameter's step count on the host (0 before its first step)."""
        return int(self.state[p]["step"].item()) if "step" in self.state.get(p, ()) else 0

    def _shared_step_count(self, params):
        """The sorted distinct step counts of ``params``: one entry when they share a count."""
        return sorted({self._count(p) for p in params})

    def _prepare(self, pairs):
        """Check the parameters and create the per-parameter state they lack."""
        for p, gi in pairs:
            if p.dtype != torch.float32 or not p.is_cuda or not p.is_contiguous() \
                    or p.grad.is_sparse:
                raise TypeError("FusedAdam: dense contiguous fp32 ROCm parameters only")
            st = self.state[p]
            if len(st) == 0:
                st["step"] = torch.tensor(0.0)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            if self.param_groups[gi]["amsgrad"] and "max_exp_avg_sq" not in st:
                st["max_exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            if self.ema_decay is not None and "ema" not in st:
                # the shadow starts from the parameter's current value (also one that joins later)
                st["ema"] = p.detach().clone(memory_format=torch.preserve_format)

    def _build(self, pairs, t, layout, old):
        """The _Plan over ``pairs`` = [(parameter, group index)] in group order at step count
        ``t``: the device table (``old``'s when nothing it holds changed), and the step counters
        re-homed as views of one CPU tensor, which ``advance`` bumps in one op."""
        plan, ex = _Plan(), layout is not None
        live = [p for p, _ in pairs]
        ams = [bool(g["amsgrad"]) for g in self.param_groups]
        rows = np.zeros((len(pairs), 7 if ex else 5), dtype=np.int64)
        chunks, plan.moments = [], []
        for i, (p, gi) in enumerate(pairs):
            if not chunks or (gi != chunks[-1][2][-1] and len(chunks[-1][2]) == MAX_GROUPS):
                chunks.append([i, 0, [gi]])
            elif gi != chunks[-1][2][-1]:
                chunks[-1][2].append(gi)
            chunks[-1][1] += 1
            st = self.state[p]
            mom = (st["exp_avg"], st["exp_avg_sq"]) + \
                ((st["max_exp_avg_sq"],) if ams[gi] else ())
            plan.moments.append(mom)
            ptrs = (p.data_ptr(), p.grad.data_ptr(), mom[0].data_ptr(), mom[1].data_ptr())
            rows[i] = ptrs + ((mom[2].data_ptr() if ams[gi] else 0, p.numel(),
                               len(chunks[-1][2]) - 1) if ex else (p.numel(),))
        plan.ptrs, plan.gptrs = rows[:, 0].tolist(), rows[:, 1].tolist()
        plan.chunks = tuple((a, b, tuple(c)) for a, b, c in chunks) if ex else None
        # with the weight EMA on, the rows' shadow pointers travel in a table of their own
        plan.shadows = sh = None
        if ex and self.ema_decay is not None:
            plan.shadows = [self.state[p]["ema"] for p in live]
            sh = np.array([e.data_ptr() for e in plan.shadows], dtype=np.int64)
        plan.ident = (rows.tobytes(), plan.chunks, None if sh is None else sh.tobytes())
        if old is not None and old.ident == plan.ident:
            plan.table, plan.shadow_table = old.table, old.shadow_table
        else:
            dev = live[0].device
            plan.table = torch.from_numpy(rows).to(dev)
            plan.shadow_table = None if sh is None else torch.from_numpy(sh).to(dev)
        plan.steps = torch.full((len(live),), float(t))
        for i, p in enumerate(live):
            self.state[p]["step"] = plan.steps[i]
        plan.state_id, plan.t, plan.layout = id(self.state), t, layout
        return plan

    def _replan(self, key, by_count):
        """The slow path of every route: the plans of ``by_count`` = {step count: pairs} under
        ``key`` (0: one plain group, 5-column rows; EX: all groups).  One shared count is cached in
        ``_fast[key]`` for the next step; several are kept by position in ``_split[key]``, which
        only saves rebuilding their device tables.  Every other cached plan is dropped: its step
        buffer may no longer be what the parameters' counters are views of."""
        old = [self._fast[key]] if key in self._fast else self._split.get(key, [])
        self._fast.clear()
        self._split.clear()
        for pairs in by_count.values():
            self._prepare(pairs)
        plans = [self._build(pairs, t, None if key == 0 else self._layout(pairs),
                             old[i] if i < len(old) else None)
                 for i, (t, pairs) in enumerate(by_count.items())]
        if len(plans) == 1:
            self._fast[key] = plans[0]
        else:
            self._split[key] = plans
        return plans

    def _launch(self, plan, gate=None, scaler=None, accum=None, ema=None):
        """The Adam launch of ``plan`` at its step count, or (``gate``: the device MauvStepGate
        pointer) gated, with the device MauvLossScale / MauvAccum / MauvEma pointers of whatever
        is on.  The groups' current lr, betas, eps, weight_decay and flags travel by value."""
        if plan.layout is None:
            g = self.param_groups[0]
            args = (plan.table.data_ptr(), len(plan.ptrs), g["lr"], *g["betas"], g["eps"],
                    g["weight_decay"])
            if gate is None:
                check(lib.mauv_adam_step(*args, plan.t, ops.stream()), "adam_step")
            else:
                check(lib.mauv_adam_step_gated(*args, gate, ops.stream()), "adam_step_gated")
            return
        assert gate is None or len(plan.chunks) == 1   # gate() takes at most MAX_GROUPS groups
        assert ema is None or plan.shadow_table is not None
        for r0, n, gis in plan.chunks:
            arr = (MauvAdamGroup * len(gis))()
            for a, gi in zip(arr, gis):
                g = self.param_groups[gi]
                a.lr, a.eps, a.weight_decay = g["lr"], g["eps"], g["weight_decay"]
                (a.beta1, a.beta2), a.flags = g["betas"], _flags(g)
            args = (plan.table.data_ptr() + 56 * r0, n, ctypes.addressof(arr), len(gis))
            if gate is None:
                check(lib.mauv_adam_step_ex(*args, plan.t, None, ops.stream()), "adam_step_ex")
            else:
                check(lib.mauv_adam_step_ex_ema(
                    *args, gate, scaler, accum,
                    None if ema is None else plan.shadow_table.data_ptr() + 8 * r0, ema,
                    ops.stream()), "adam_step_ex_ema")

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._not_swapped("step")
        if self._scaler() is not None:
            self._step_scaled()
            return loss
        self._sync_gate()
        self._gate = None   # an ungated step moves the count on the host: re-read it next time
        if self.max_grad_norm is not None:
            self._clip_live()
        else:
            self.last_grad_norm = None
        if self.ema_decay is not None:
            self._step_then_ema()
            return loss
        self._step_adam()
        return loss

    def _step_then_ema(self):
        """The ungated step with the weight EMA on: the Adam launches as without it, then
        ``mauv_ema_update`` over the same live parameters, at the weight the device rule gives
        the host's update count — one extra pass over parameters and shadows."""
        live = [p for g in self.param_groups for p in g["params"] if p.grad is not None]
        for p in live:   # a parameter stepped before the option was set: its shadow starts here
            st = self.state.get(p)
            if st and "ema" not in st:
                st["ema"] = p.detach().clone(memory_format=torch.preserve_format)
        self._step_adam()
        if not live:
            return
        rows = self._ema_row_table([(p, self.state[p]["ema"]) for p in live])
        w = ema_weight(self._ema_updates, self.ema_decay, self.ema_warmup)
        check(lib.mauv_ema_update(rows.data_ptr(), len(live), w, ops.stream()), "ema_update")
        self._ema_updates += 1
        self._ema_pushed = False

    def _step_adam(self):
        """The Adam launches of the ungated step: one plain group through mauv_adam_step, anything
        else through mauv_adam_step_ex, every group with live parameters in one launch (per
        shared step count, MAX_GROUPS groups per launch)."""
        pairs = [(p, gi) for gi, g in enumerate(self.param_groups) for p in g["params"]
                 if p.grad is not None]
        if not pairs:
            return
        key = 0 if self._simple() else EX
        plan = self._fast.get(key)
        if plan is not None and plan.valid_for(self, [p for p, _ in pairs],
                                               None if key == 0 else self._layout(pairs)):
            plan.advance()
            self._launch(plan)
            return
        # one bias-correction step per launch (a param that missed steps because its grad was
        # None keeps its own count like torch — split it)
        by_count = {}
        for p, gi in pairs:
            by_count.setdefault(self._count(p) + 1, []).append((p, gi))
        for plan in self._replan(key, by_count):
            self._launch(plan)

    def _step_scaled(self):
        """``step()`` with a loss scaler: the gated step on a gate of this optimizer's own over
        the live parameters, the loss taken as finite.  The scan (norm + non-finite count), the
        decision and the Adam launch are queued; nothing is read back."""
        if len(self.param_groups) > MAX_GROUPS:
            raise ValueError(f"FusedAdam: loss scaling steps through the device-gated form, "
                             f"which takes at most {MAX_GROUPS} parameter groups "
                             f"({len(self.param_groups)} given)")
        pairs = [(p, gi) for gi, g in enumerate(self.param_groups) for p in g["params"]
                 if p.grad is not None]
        if not pairs:
            return
        for p, _ in pairs:
            g = p.grad
            if g.dtype != torch.float32 or not g.is_cuda or g.is_sparse or not g.is_contiguous():
                raise TypeError("FusedAdam: dense contiguous fp32 ROCm gradients only")
        dev = pairs[0][0].device
        same = self._gate is not None and self._gate.device == dev and \
            self._gate_live is not None and len(self._gate_live) == len(pairs) and \
            all(a is b and i == j for (a, i), (b, j) in zip(self._gate_live, pairs))
        if not same:
            self._sync_gate()
            counts = self._shared_step_count(p for p, _ in pairs)
            if len(counts) != 1:
                raise ValueError("FusedAdam: loss scaling steps through the device-gated form, "
                                 "which needs one step count for all parameters "
                                 f"(found {counts})")
            self._new_gate(dev, counts[0], 0)
            self._gate_params = None
            self._gate_live = pairs
        gate = self._gate
        word(gate, G_OK_LOSS).fill_(1)
        self.scan_gated(gate)
        self._step_gated(gate)

    # ---- the device-gated form ---------------------------------------------------------------
    def _new_gate(self, device, step, poisoned):
        """A fresh device MauvStepGate at Adam step count ``step``."""
        g = torch.zeros(GATE_WORDS, dtype=torch.int32)
        g[G_STEP], g[G_POISONED] = step, poisoned
        self._gate = g.to(device)
        self._gate_dirty = False
        self._gate_clip = (0.0, 0)

    def gate(self, params, device):
        """The device MauvStepGate for a training loop over ``params`` (the model's trainable
        parameters), or None when the gated form does not apply: 1 to 8 parameter groups whose
        parameters with requires_grad are exactly those tensors, all sharing one step count,
        and whose other parameters are frozen and hold no gradient."""
        if self._gate is not None and self._gate_params is params and \
                self._gate.device == torch.device(device):
            return self._gate
        if not 1 <= len(self.param_groups) <= MAX_GROUPS:
            return None
        pairs = [(p, gi) for gi, g in enumerate(self.param_groups) for p in g["params"]]
        if any(p.grad is not None for p, _ in pairs if not p.requires_grad):
            return None
        pairs = [(p, gi) for p, gi in pairs if p.requires_grad]
        gp = [p for p, _ in pairs]
        if len(gp) != len(params) or {id(p) for p in gp} != {id(p) for p in params}:
            return None
        if self._gate is None or self._gate.device != torch.device(device):
            counts = self._shared_step_count(gp)
            if len(counts) != 1:
                return None
            # the gate takes a skipped batch's gradients back out by zeroing a clean arena, so it
            # starts from what the arena holds: non-finite values (an ungated step skipped on
            # them: "poisoned", kept as the reference keeps them) or nothing.  Finite leftovers
            # (a backward outside the loop) would be lost by that zeroing: such a step takes the
            # host-decided path, whose skip runs no backward (multimodal.py:133-135)
            grads = [p.grad for p in gp if p.grad is not None]
            poisoned = 0
            if grads:
                top = torch.stack(torch._foreach_norm(grads, float("inf")))
                if not bool(torch.isfinite(top).all()):
                    poisoned = 1
                elif bool((top != 0).any()):
                    return None
            self._new_gate(device, counts[0], poisoned)
        self._gate_params = params
        self._gate_live = pairs
        return self._gate

    @torch.no_grad()
    def step_gated(self, gate, close=None):
        """One step whose execution (step + zero_grad, restore, or nothing) the kernel reads
        from ``gate`` — no host synchronisation.  Every trainable parameter of every group must
        hold a gradient (the model's arena views); frozen ones get no state and no step.

        With ``grad_accumulation`` K > 1 each call is one micro-batch.  ``close=None`` closes the
        window on every K-th call (a host count), ``close=True`` / ``False`` says so outright (a
        loader's last batch closes a partial window, averaged by its true count).  A call that
        does not close queues ``mauv_accum_note`` alone; the closing call is the step, through
        the all-groups entry.  The ungated ``step()`` and ``mauv.amp.LossScaler.step(opt)`` in
        a user's own loop ignore the option."""
        assert gate is self._gate, "step_gated: use the gate returned by FusedAdam.gate()"
        self._not_swapped("step_gated")
        accum = None
        if self.accumulating():
            closing = self.closes_window(close)
            if self._accum is None or self._accum.device != gate.device:
                self._accum = torch.zeros(ACC_WORDS, dtype=torch.int32, device=gate.device)
            accum = self._accum
            if not closing:
                self._accum_micro += 1
                check(lib.mauv_accum_note(gate.data_ptr(), accum.data_ptr(), ops.stream()),
                      "accum_note")
                return
            self._accum_micro = 0
        from torch.optim import optimizer as _topt
        for hook in list(_topt._global_optimizer_pre_hooks.values()) + \
                list(self._optimizer_step_pre_hooks.values()):
            hook(self, (self,), {})
        self._step_gated(gate, accum)
        # what torch.optim.Optimizer.step's wrapper records: an LR scheduler stepped after this
        # does not warn "lr_scheduler.step() before optimizer.step()"; step hooks still run
        self._opt_called = True
        for hook in list(self._optimizer_step_post_hooks.values()) + \
                list(_topt._global_optimizer_post_hooks.values()):
            hook(self, (self,), {})

    def _step_gated(self, gate, accum=None):
        """step_gated without the step hooks (``step()`` runs them itself).  ``accum``: the
        device MauvAccum of the accumulation window this step closes."""
        pairs = self._gate_live
        live = [p for p, _ in pairs]
        if any(p.grad is None for p in live):
            raise RuntimeError("step_gated: every parameter needs a gradient tensor")
        ls = self._scaler()
        ema_on = self.ema_decay is not None
        # with a loss scaler, an accumulation window or the weight EMA every layout takes the
        # all-groups entry: one plain group there is adam_elem, the simple kernel's element
        key = 0 if self._simple() and ls is None and accum is None and not ema_on else EX
        layout = None if key == 0 else self._layout(pairs)
        plan = self._fast.get(key)
        if plan is None or not plan.valid_for(self, live, layout):
            plan, = self._replan(key, {self._gate_step_host(): pairs})
        self._write_gate_clip(gate)   # (the caller's scan_gated wrote them already when on)
        self._launch(plan, gate.data_ptr(),
                     None if ls is None else ls.device_state(gate.device).data_ptr(),
                     None if accum is None else accum.data_ptr(),
                     self._ema_state(gate.device).data_ptr() if ema_on else None)
        self._ema_dirty = self._ema_dirty or ema_on
        self.last_grad_norm = None if self.max_grad_norm is None else \
            word(gate, G_GRAD_NORM, fp32=True).clone()[0]
        self._gate_dirty = True

    def _gate_step_host(self):
        """Step count held by the gate (one device read; only on a cache rebuild)."""
        return int(self._gate[G_STEP].item()) if self._gate is not None else 0

    # ---- the weight EMA ----------------------------------------------------------------------
    def _ema_state(self, device):
        """The device MauvEma of the gated form, holding the current options and an update
        count that is the host's or ahead of it; device fills only, no host synchronisation."""
        opts = (self.ema_decay, self.ema_warmup)
        e = self._ema
        if e is None or e.device != torch.device(device):
            self._sync_ema()
            w = np.zeros(EMA_WORDS, dtype=np.int32)
            w.view(np.float32)[E_DECAY] = opts[0]
            w[E_WARMUP], w[E_UPDATES] = opts[1], self._ema_updates
            e = self._ema = torch.from_numpy(w).to(device)
            self._ema_opts, self._ema_pushed = opts, True
        if self._ema_opts != opts:
            word(e, E_DECAY, fp32=True).fill_(opts[0])
            word(e, E_WARMUP).fill_(int(opts[1]))
            self._ema_opts = opts
        if not self._ema_pushed:
            word(e, E_UPDATES).fill_(self._ema_updates)
            self._ema_pushed = True
        return e

    def _sync_ema(self):
        """After gated steps, bring the host's EMA update count up to the device's (one device
        read, where _sync_gate reads the step count)."""
        if self._ema is not None and self._ema_dirty:
            self._ema_updates = int(self._ema[E_UPDATES].item())
        self._ema_dirty = False

    @property
    def ema_updates(self):
        """EMA updates taken so far (after gated steps: one device read)."""
        self._sync_ema()
        return self._ema_updates

    def ema_parameters(self):
        """[(parameter, its shadow)] of every parameter that holds one."""
        return [(p, self.state[p]["ema"]) for g in self.param_groups for p in g["params"]
                if "ema" in self.state.get(p, ())]

    def _ema_row_table(self, pairs):
        """The device MauvEmaRow table over ``pairs``, rebuilt only when a pointer changes."""
        rows = np.array([(e.data_ptr(), p.data_ptr(), p.numel()) for p, e in pairs],
                        dtype=np.int64)
        if len(rows) > 65535:
            raise ValueError("FusedAdam: more than 65535 tensors with a weight EMA")
        key = (rows.tobytes(), pairs[0][0].device)
        if self._ema_rows is None or self._ema_rows[0] != key:
            self._ema_rows = (key, torch.from_numpy(rows).to(pairs[0][0].device))
        return self._ema_rows[1]

    def _not_swapped(self, what):
        if self.__dict__.get("_ema_swapped"):
            raise RuntimeError(f"FusedAdam.{what}: the parameters hold the averaged weights "
                               "(swap_ema() / averaged()); swap back first")

    @torch.no_grad()
    def swap_ema(self):
        """Exchange every parameter with its shadow, element-wise and in place
        (``mauv_ema_swap``): the model then computes on the averaged weights, and a second call
        brings the live ones back bit for bit.  No pointer changes, so cached tables and engine
        state stay valid.  BatchNorm buffers are not averaged: the live ones serve."""
        if self.ema_decay is None and not self.ema_parameters():
            raise RuntimeError("FusedAdam.swap_ema: no weight EMA (ema_decay is None)")
        pairs = self.ema_parameters()
        if pairs:
            for p, e in pairs:
                if not (p.is_cuda and e.is_cuda and p.is_contiguous() and e.is_contiguous()
                        and p.dtype == e.dtype == torch.float32):
                    raise TypeError("FusedAdam: dense contiguous fp32 ROCm parameters only")
            with torch.cuda.device(pairs[0][0].device):
                rows = self._ema_row_table(pairs)
                check(lib.mauv_ema_swap(rows.data_ptr(), len(pairs), ops.stream()), "ema_swap")
        self._ema_swapped = not self._ema_swapped

    @contextlib.contextmanager
    def averaged(self):
        """``with opt.averaged():`` the model runs on the averaged weights (evaluate, save);
        the live weights are back, bit for bit, on exit."""
        self.swap_ema()
        try:
            yield self
        finally:
            self.swap_ema()

    def _sync_gate(self):
        """After gated steps, bring state["step"] up to the device count (before an ungated
        step or a state_dict)."""
        self._sync_ema()
        if self._gate is None or not self._gate_dirty:
            return
        t = self._gate_step_host()
        for group in self.param_groups:
            for p in group["params"]:
                st = self.state.get(p)   # (a frozen parameter has none, and gets none here)
                if st is not None and "step" in st:
                    st["step"].fill_(float(t))
        for plan in self._fast.values():   # (_split plans are rebuilt from the state's counts
            plan.t = t                     # on every step: their t is never read again)
        self._gate_dirty = False

    def state_dict(self):
        """torch's state_dict; with the weight EMA it carries the shadows (``state[p]["ema"]``)
        and a top-level ``"ema_updates"``, and still loads into torch.optim.Adam."""
        self._not_swapped("state_dict")
        self._sync_gate()
        sd = super().state_dict()
        if self.ema_decay is not None:
            sd["ema_updates"] = self._ema_updates
        return sd

    def load_state_dict(self, state_dict):
        """torch's load (new state tensors, step counts): the cached tables are dropped.  A
        top-level ``"ema_updates"`` restores the EMA update count."""
        self._not_swapped("load_state_dict")
        self._sync_ema()
        super().load_state_dict(state_dict)
        for group in self.param_groups:   # a state_dict saved before these keys existed
            for k, v in self.defaults.items():
                group.setdefault(k, v)
            self._check_group(group)
        self._fast.clear()
        self._split.clear()
        self._gate = None
        self._gate_dirty = False
        self._ema_rows = None
        if "ema_updates" in state_dict:
            self._ema_updates = int(state_dict["ema_updates"])
            self._ema_dirty = self._ema_pushed = False


class FusedAdamW(FusedAdam):
    """torch.optim.AdamW: FusedAdam with decoupled weight decay (default 1e-2); its
    ``state_dict()`` loads into torch.optim.AdamW and back."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2,
                 amsgrad=False, **options):
        if not options.pop("decoupled_weight_decay", True):
            raise ValueError("FusedAdamW: decoupled_weight_decay is always on")
        super().__init__(params, lr, betas, eps, weight_decay, amsgrad,
                         decoupled_weight_decay=True, **options)


class HostEma:
    """The weight EMA of a host model under a torch optimizer, FusedAdam's interface on torch's
    own kernels: define_optimizers_and_schedulers hangs one on the optimizer (``optimizer.ema``)
    and the training loops call ``update()`` after exactly those ``optimizer.step()`` calls that
    ran.  The shadows are clones of the trainable parameters taken at construction; the first
    update copies (``_foreach_copy_``), later ones are ``_foreach_lerp_(shadows, params, 1 - d)``
    — ``torch.optim.swa_utils.AveragedModel`` with ``get_ema_multi_avg_fn(d)``, bit for bit —
    with d capped at ``(1 + n) / (10 + n)`` on update n under the warm-up.  Buffers are not
    averaged."""

    def __init__(self, params, ema_decay, ema_warmup=False, ema_eval=True):
        self.ema_decay = check_ema_decay(ema_decay)
        if self.ema_decay is None:
            raise ValueError("HostEma: ema_decay must be a number with 0 < d < 1, got None")
        self.ema_warmup = check_ema_flag("ema_warmup", ema_warmup)
        self.ema_eval = check_ema_flag("ema_eval", ema_eval)
        self.params = [p for p in params if p.requires_grad]
        self.shadows = [p.detach().clone() for p in self.params]
        self.ema_updates = 0
        self._swapped = False

    @torch.no_grad()
    def update(self):
        if self._swapped:
            raise RuntimeError("HostEma.update: the parameters hold the averaged weights")
        n = self.ema_updates
        if n == 0:
            torch._foreach_copy_(self.shadows, self.params)
        else:
            d = self.ema_decay
            if self.ema_warmup:
                d = min(d, (1.0 + n) / (10.0 + n))
            torch._foreach_lerp_(self.shadows, self.params, 1 - d)
        self.ema_updates = n + 1

    def ema_parameters(self):
        return list(zip(self.params, self.shadows))

    @torch.no_grad()
    def swap_ema(self):
        for p, e in zip(self.params, self.shadows):
            live = p.detach().clone()
            p.copy_(e)
            e.copy_(live)
        self._swapped = not self._swapped

    @contextlib.contextmanager
    def averaged(self):
        self.swap_ema()
        try:
            yield self
        finally:
            self.swap_ema()


def ema_of(optimizer):
    """What carries an optimizer's weight EMA — the FusedAdam itself with ``ema_decay`` set, or
    the HostEma hung on a torch optimizer — or None."""
    if isinstance(optimizer, FusedAdam):
        return optimizer if optimizer.ema_decay is not None else None
    return getattr(optimizer, "ema", None)


_clip_plans = {}   # (device, span rows) -> _NormPlan of clip_grad_norm_ (a few, oldest dropped)


def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None):
    """``torch.nn.utils.clip_grad_norm_`` (same arguments; a model stands for its parameters)
    on gradnorm.hip: one scan and one in-place multiply over all gradients, returning the total
    pre-clip norm as a 0-dim device tensor.  Nothing synchronises with the host — once the span
    table of these gradient tensors is cached — unless ``error_if_nonfinite`` asks for the
    check.  Non-finite gradients give a NaN norm and are left as they are.  Anything but dense
    contiguous fp32 ROCm gradients on one device with norm_type 2 / inf and a finite
    max_norm > 0 is handed to torch's function."""
    if isinstance(parameters, torch.nn.Module):
        parameters = list(parameters.parameters())
    elif isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    else:
        parameters = list(parameters)
    grads = [p.grad for p in parameters if p.grad is not None]
    try:
        max_norm_f, kind = check_max_grad_norm(max_norm), _kind(check_grad_norm_type(norm_type))
    except ValueError:
        max_norm_f = None
    if max_norm_f is None or not grads or len(grads) > 65535 or any(
            g.dtype != torch.float32 or not g.is_cuda or g.is_sparse or not g.is_contiguous()
            or g.device != grads[0].device for g in grads):
        return torch.nn.utils.clip_grad_norm_(parameters, max_norm, norm_type,
                                              error_if_nonfinite, foreach)
    dev = grads[0].device
    rows = _span_rows(grads)
    key = (dev, tuple(rows))
    plan = _clip_plans.get(key)
    if plan is None:
        while len(_clip_plans) >= 4:
            _clip_plans.pop(next(iter(_clip_plans)))
        plan = _clip_plans[key] = _NormPlan()
    with torch.cuda.device(dev):
        spans, ws = plan.get(rows, dev)
        norm = torch.empty(1, device=dev)
        ops.grad_norm(spans, kind, ws, norm)
        if error_if_nonfinite and not bool(torch.isfinite(norm).item()):
            raise RuntimeError(f"The total norm of order {norm_type} for gradients from "
                               "`parameters` is non-finite, so it cannot be clipped.")
        ops.grad_clip(spans, norm, max_norm_f)
    return norm[0]
