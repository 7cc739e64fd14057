"""LossScaler — ``torch.amp.GradScaler``'s dynamic loss scaling, decided and applied on the device.

f16 has a 5-bit exponent: an activation gradient below 2^-25 is stored as 0 and one above 65504
as inf.  The cure is GradScaler's: run the backward on ``loss * scale``, divide the gradients by
``scale`` before the update, skip the update and back the scale off when a gradient overflowed,
grow it after ``growth_interval`` clean steps.  Here the scale lives in a 32-byte device struct
(``MauvLossScale``, include/mauv.h) beside FusedAdam's ``MauvStepGate``: the gated Adam step's
one-thread decision (adam.hip) reads the non-finite count of the gradient scan,
skips / backs off / grows, and the Adam kernel multiplies each gradient by ``1 / scale`` as it
loads it.  No pass over the gradients is added and nothing waits on the host.

Use it through the optimizer, ``FusedAdam(..., loss_scale="dynamic" | number | LossScaler)``: the
training loops (mauv.train) then scale the loss themselves.  In a hand-written loop the torch
idiom works::

    scaler = LossScaler()
    opt = FusedAdam(model.parameters(), loss_scale=scaler)
    scaler.scale(loss).backward()
    scaler.step(opt)        # decision, unscale, clip, Adam, zero_grad: one device step
    scaler.update()         # nothing left to do: the decision updated the scale

``step`` takes a FusedAdam only (the unscale is part of its kernel); with torch's optimizers use
``torch.amp.GradScaler``, whose ``state_dict()`` loads here and the reverse.  A stepped FusedAdam
has consumed the gradients: they are zero afterwards, stepped or skipped, as after GradScaler's
``step`` followed by ``zero_grad``.

Under DistributedMC the scan runs after ``allreduce_grads()``: every rank sees the same arena,
takes the same decision and holds the same scale, so no collective is added.
"""
import math
import numbers

import numpy as np
import torch

LS_WORDS = 8             # sizeof(MauvLossScale) / 4 (include/mauv.h)
(LS_SCALE, LS_UNSCALE, LS_GROWTH, LS_BACKOFF,                     # fp32
 LS_INTERVAL, LS_TRACKER, LS_OVERFLOWS, LS_GROWTHS) = range(8)    # int32


def _number(v, what):
    if isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(v):
        raise ValueError(f"LossScaler: {what} must be a finite number, got {v!r}")
    return float(v)


class LossScaler:
    def __init__(self, init_scale=2.0 ** 16, growth_factor=2.0, backoff_factor=0.5,
                 growth_interval=2000, dynamic=True, enabled=True):
        init_scale = _number(init_scale, "init_scale")
        growth_factor = _number(growth_factor, "growth_factor")
        backoff_factor = _number(backoff_factor, "backoff_factor")
        if not 0.0 < init_scale <= float(np.finfo(np.float32).max):
            raise ValueError(f"LossScaler: init_scale must be a positive fp32, got {init_scale}")
        if growth_factor <= 1.0:      # torch.amp.GradScaler's own conditions
            raise ValueError("LossScaler: the growth factor must be > 1.0")
        if not 0.0 < backoff_factor < 1.0:
            raise ValueError("LossScaler: the backoff factor must be in (0, 1)")
        if isinstance(growth_interval, bool) or not isinstance(growth_interval, numbers.Integral) \
                or not 1 <= growth_interval < 2 ** 31:
            raise ValueError(f"LossScaler: growth_interval must be an int >= 1, got "
                             f"{growth_interval!r}")
        self._enabled, self.dynamic = bool(enabled), bool(dynamic)
        self._growth_factor, self._backoff_factor = growth_factor, backoff_factor
        self._growth_interval = int(growth_interval)
        # the host copy holds the truth until a device asks for the state, and after a load
        self._host = dict(scale=float(np.float32(init_scale)), tracker=0, overflows=0, growths=0)
        self._dev = None             # int32[8] device tensor laid out as MauvLossScale

    # ---- the device state ------------------------------------------------------------------
    def device_state(self, device):
        """The MauvLossScale words on ``device`` (int32[8]; the fp32 fields are bit views),
        written once from the host copy — the way FusedAdam writes its gate."""
        device = torch.device(device)
        if self._dev is not None and self._dev.device != device:
            self._pull()
            self._dev = None
        if self._dev is None:
            w = np.zeros(LS_WORDS, dtype=np.int32)
            f = w.view(np.float32)
            f[LS_SCALE], f[LS_UNSCALE] = self._host["scale"], 1.0 / self._host["scale"]
            f[LS_GROWTH], f[LS_BACKOFF] = self._growth_factor, self._backoff_factor
            w[LS_INTERVAL] = self._growth_interval if self.dynamic else 0
            w[LS_TRACKER], w[LS_OVERFLOWS] = self._host["tracker"], self._host["overflows"]
            w[LS_GROWTHS] = self._host["growths"]
            self._dev = torch.from_numpy(w).to(device)
        return self._dev

    def scale_tensor(self, device):
        """The scale as a 1-element fp32 view of the device state (no copy, no sync)."""
        return self.device_state(device)[LS_SCALE:LS_SCALE + 1].view(torch.float32)

    def _pull(self):
        """Device state -> host copy (synchronises)."""
        if self._dev is not None:
            w = self._dev.cpu().numpy()
            self._host = dict(scale=float(w.view(np.float32)[LS_SCALE]),
                              tracker=int(w[LS_TRACKER]), overflows=int(w[LS_OVERFLOWS]),
                              growths=int(w[LS_GROWTHS]))
        return self._host

    # ---- torch.amp.GradScaler's surface ----------------------------------------------------
    def is_enabled(self):
        return self._enabled

    def get_scale(self):
        """The current scale as a Python float: the one call here that synchronises."""
        return self._pull()["scale"] if self._enabled else 1.0

    def get_growth_tracker(self):
        return self._pull()["tracker"] if self._enabled else 0

    def counters(self):
        """(overflows, growths) so far (synchronises)."""
        h = self._pull()
        return h["overflows"], h["growths"]

    def get_growth_factor(self):
        return self._growth_factor

    def get_backoff_factor(self):
        return self._backoff_factor

    def get_growth_interval(self):
        return self._growth_interval

    def scale(self, loss):
        """``loss * scale``, the scale read on the device (no synchronisation)."""
        if not self._enabled:
            return loss
        if not loss.is_cuda:
            raise TypeError("LossScaler.scale: a ROCm tensor (host models: torch.amp.GradScaler)")
        return loss * self.scale_tensor(loss.device)[0]

    def step(self, optimizer, *args, **kwargs):
        """``optimizer.step()`` through the device decision; the optimizer must be a FusedAdam
        carrying this scaler (a FusedAdam with no scaler yet takes this one)."""
        from .optim import FusedAdam
        if not isinstance(optimizer, FusedAdam):
            raise TypeError("LossScaler.step drives mauv.optim.FusedAdam; with a torch optimizer "
                            "use torch.amp.GradScaler")
        if optimizer.loss_scale is None:
            optimizer.loss_scale = self
        if optimizer.loss_scale is not self:
            raise ValueError("LossScaler.step: the optimizer carries another loss scaler")
        return optimizer.step(*args, **kwargs)

    def update(self, new_scale=None):
        """The scale was updated by the step's decision; only an explicit ``new_scale`` (a
        number) does anything: it restarts the scaler from that scale."""
        if new_scale is None or not self._enabled:
            return
        if isinstance(new_scale, torch.Tensor):
            new_scale = float(new_scale)
        s = _number(new_scale, "new_scale")
        if s <= 0:
            raise ValueError("LossScaler.update: new_scale must be > 0")
        h = self._pull()
        h["scale"] = float(np.float32(s))
        self._dev = None

    def state_dict(self):
        """torch.amp.GradScaler's keys: either loads the other's (synchronises)."""
        if not self._enabled:
            return {}
        h = self._pull()
        return {"scale": h["scale"], "growth_factor": self._growth_factor,
                "backoff_factor": self._backoff_factor,
                "growth_interval": self._growth_interval, "_growth_tracker": h["tracker"]}

    def load_state_dict(self, state_dict):
        if not self._enabled:
            return
        if len(state_dict) == 0:
            raise RuntimeError("The source state dict is empty, possibly because it was saved "
                               "from a disabled instance of GradScaler.")
        fresh = LossScaler(state_dict["scale"], state_dict["growth_factor"],
                           state_dict["backoff_factor"], state_dict["growth_interval"],
                           self.dynamic)
        tracker = int(state_dict["_growth_tracker"])
        if tracker < 0:
            raise ValueError("LossScaler: _growth_tracker must be >= 0")
        self._pull()
        self._growth_factor, self._backoff_factor = fresh._growth_factor, fresh._backoff_factor
        self._growth_interval = fresh._growth_interval
        self._host.update(scale=fresh._host["scale"], tracker=tracker)
        self._dev = None


def as_loss_scaler(v):
    """``FusedAdam(loss_scale=...)``: None, "dynamic" (the defaults), a number (a static scale) or
    a LossScaler -> a LossScaler or None."""
    if v is None or isinstance(v, LossScaler):
        return v
    if isinstance(v, str):
        if v != "dynamic":
            raise ValueError(f"loss_scale must be None, 'dynamic', a number > 0 or a LossScaler, "
                             f"got {v!r}")
        return LossScaler()
    if isinstance(v, bool) or not isinstance(v, numbers.Real) or \
            not 0.0 < v <= float(np.finfo(np.float32).max):
        raise ValueError(f"loss_scale must be None, 'dynamic', a number > 0 or a LossScaler, got "
                         f"{v!r}")
    return LossScaler(init_scale=v, dynamic=False)


def own_loss_scaler(v):
    """The option for one optimizer of several built from the same settings
    (define_optimizers_and_schedulers): a LossScaler instance is copied — settings and state — so
    that no two optimizers share a scale; reach it as ``optimizer.loss_scale``."""
    ls = as_loss_scaler(v)
    if ls is None or ls is not v:
        return ls
    own = LossScaler(dynamic=ls.dynamic, enabled=ls.is_enabled())
    own._growth_factor, own._backoff_factor = ls._growth_factor, ls._backoff_factor
    own._growth_interval = ls._growth_interval
    own._host = dict(ls._pull())
    return own


def host_grad_scaler(v):
    """The same option for a host model stepped by a torch optimizer: a
    ``torch.amp.GradScaler("cpu", ...)`` with the LossScaler's settings and state, or None.
    GradScaler has no static mode, so a static scale is refused here."""
    ls = as_loss_scaler(v)
    if ls is None or not ls.is_enabled():
        return None
    if not ls.dynamic:
        raise ValueError("loss_scale: a static scale needs a model on a ROCm device "
                         "(torch.amp.GradScaler, which drives a host model, is always dynamic)")
    gs = torch.amp.GradScaler("cpu")
    gs.load_state_dict(ls.state_dict())
    return gs
