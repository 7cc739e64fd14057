"""On-device augmentation of seabed triplets through libmauv_hip (staging.hip).

The optical tile, the bathymetry patch and the side-scan patch of one item are co-registered,
so one move per item goes to all three.  A move is a code of the dihedral group of the square
(bit0 = flip W, bit1 = flip H, bit2 = transpose applied last; include/mauv.h); the codes and a
per-item turbidity are drawn on the device from Philox, keyed by (seed, step, item index), and
the move is applied inside the staging passes that exist anyway: the Resize / ToTensor /
Normalize (/ UIFM) pass of decoded uint8 tiles, or one gather pass over fp32 tensors the
host datasets already transformed.  The turbidity degrades the optical tile only, as in the
reference (Examples/"Example training with image noise.py":254,419, one draw per batch there).

* ``TripletAugment``: ``draw`` a plan for a batch, ``apply`` it to the three tensors.
* ``dihedral`` / ``undo_dihedral``: the move and its inverse on fp32 NCHW tensors, with
  autograd: a ``mauv.input_gradients`` map of an augmented batch comes back to the original
  frame with ``undo_dihedral(grad, plan.ops)``.
* ``AugmentedLoader``: wraps a train loader of the reference's batch dicts; the training loops
  take it unchanged.  Evaluation and prediction loaders stay bare.

Nothing here reads a device value on the host: no ``.item()``, no wait.
"""
import torch
from torch.autograd.function import once_differentiable

from . import ops as _ops
from . import staging

MODES = {"none": 0, "flips": 1, "dihedral": 2}
# inverse of code k: k when bit2 is clear, else k with bit0 and bit1 swapped
INVERSE_CODES = (0, 1, 2, 3, 4, 6, 5, 7)

_inverse_lut = {}


def inverse_ops(ops, allow_transpose=True):
    """The codes that undo ``ops`` (uint8 [B]), formed on the tensor's device.  Without the
    transpose only bits 0 and 1 of a code are applied, and a flip undoes itself."""
    if not allow_transpose:
        return ops & 3
    lut = _inverse_lut.get(ops.device)
    if lut is None:
        lut = _inverse_lut[ops.device] = torch.tensor(INVERSE_CODES, dtype=torch.uint8,
                                                      device=ops.device)
    return lut[(ops & 7).long()]


def _transposing(x, allow_transpose):
    """Whether bit2 of a code is applied to ``x``: by default on square tiles only."""
    if x.dim() != 4:
        raise ValueError("dihedral moves take fp32 [B, C, H, W] tensors on a ROCm device")
    square = x.shape[-2] == x.shape[-1]
    if allow_transpose and not square:
        raise ValueError(f"a transposing move needs a square tile, got {tuple(x.shape[-2:])}")
    return square if allow_transpose is None else bool(allow_transpose)


def _move(x, ops, allow_transpose):
    if x.dim() != 4 or x.dtype != torch.float32 or not x.is_cuda:
        raise ValueError("dihedral moves take fp32 [B, C, H, W] tensors on a ROCm device")
    if ops.dtype != torch.uint8 or ops.numel() != x.shape[0]:
        raise ValueError("ops must be uint8 [B], one move code per item")
    x = x.contiguous()
    out = torch.empty_like(x)
    _ops.stage_f32_aug(x, None, None, None, 1.0, ops.contiguous(), None, allow_transpose, out)
    return out


class _Dihedral(torch.autograd.Function):
    """The move by ``ops``; ``allow_transpose`` is resolved by the caller, so that the forward
    and the backward read the same bits of a code."""

    @staticmethod
    def forward(ctx, x, ops, allow_transpose):
        ctx.allow_transpose = allow_transpose
        ctx.save_for_backward(ops)
        return _move(x, ops, allow_transpose)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        (ops,) = ctx.saved_tensors
        inv = inverse_ops(ops, ctx.allow_transpose)
        return _move(grad, inv, ctx.allow_transpose), None, None


def dihedral(x, ops, allow_transpose=None):
    """Item b of fp32 NCHW ``x`` moved by code ``ops[b]``:
    ``y = x; bit1: y.flip(-2); bit0: y.flip(-1); bit2: y.transpose(-2, -1)``.
    Differentiable in ``x`` once (the backward is :func:`undo_dihedral`).  Bit2 is read only on
    square tiles (``allow_transpose`` defaults to ``H == W``); where it is not read, code k
    acts as ``k & 3`` in the move, its gradient and its inverse alike."""
    return _Dihedral.apply(x, ops, _transposing(x, allow_transpose))


def undo_dihedral(x, ops, allow_transpose=None):
    """The inverse move: ``undo_dihedral(dihedral(x, ops), ops)`` is ``x`` bit for bit."""
    tr = _transposing(x, allow_transpose)
    return _Dihedral.apply(x, inverse_ops(ops, tr), tr)


class AugmentPlan:
    """One batch's draws: ``ops`` uint8 [B] and ``turb`` fp32 [B] (or None) on the device, the
    ``step`` they were drawn at and the mode they were drawn in."""

    def __init__(self, ops, turb, step, mode):
        self.ops, self.turb, self.step, self.mode = ops, turb, step, mode


class TripletAugment:
    """Per-item dihedral moves and turbidity for a triplet batch.

    mode: "dihedral" (8 codes), "flips" (4) or "none".  turbidity: None or (lo, hi), the range
    of the per-item turbidity factor of the UIFM degradation (optical tile only), at distance
    ``depth``.  Item ``i = item0 + b`` of the batch drawn at step ``s`` gets the Philox words of
    counter (i, s) under ``seed``; every ``draw`` advances the step.  Under ``DistributedMC``
    give rank r ``item0 = r * B`` so the ranks draw different moves from one seed.
    """

    def __init__(self, mode="dihedral", turbidity=None, depth=1.0, seed=None, item0=0):
        if mode not in MODES:
            raise ValueError(f"mode must be one of {sorted(MODES)}, got {mode!r}")
        if turbidity is not None:
            if len(turbidity) != 2:
                raise ValueError("turbidity is None or a pair (lo, hi)")
            turbidity = (float(turbidity[0]), float(turbidity[1]))
            if not turbidity[1] >= turbidity[0]:
                raise ValueError(f"turbidity (lo, hi) needs hi >= lo, got {turbidity}")
        if int(item0) < 0:
            raise ValueError("item0 must be >= 0")
        self.mode, self.turbidity, self.depth = mode, turbidity, float(depth)
        self.seed = (torch.initial_seed() if seed is None else int(seed)) & (2 ** 64 - 1)
        self.item0 = int(item0)
        self.step = 0
        self.last_plan = None

    # ------------------------------------------------------------------ state
    def state_dict(self):
        return {"seed": self.seed, "step": self.step, "mode": self.mode,
                "turbidity": self.turbidity, "depth": self.depth, "item0": self.item0}

    def load_state_dict(self, sd):
        fresh = TripletAugment(sd["mode"], sd["turbidity"], sd["depth"], sd["seed"], sd["item0"])
        self.__dict__.update(fresh.__dict__)
        self.step = int(sd["step"])

    # ------------------------------------------------------------------ draw / apply
    def draw(self, B, device):
        """The plan of the next batch of ``B`` items (one launch, no host sync)."""
        device = torch.device(device)
        ops = torch.empty(B, dtype=torch.uint8, device=device)
        turb = None
        lo = hi = 0.0
        if self.turbidity is not None:
            lo, hi = self.turbidity
            turb = torch.empty(B, dtype=torch.float32, device=device)
        plan = AugmentPlan(ops, turb, self.step, self.mode)
        with torch.cuda.device(device):
            _ops.augment_draw(self.seed, self.step, self.item0, MODES[self.mode], lo, hi, ops,
                              turb)
        self.step += 1
        self.last_plan = plan
        return plan

    def apply_one(self, plan, t, optical=False):
        """One batch tensor under ``plan``: decoded uint8 HWC tiles [B, H, W, C] (C = 1 or 3) are
        staged as ``staging.stage_tile_batch`` does with the move in the same pass; transformed
        fp32 NCHW tensors take one gather pass.  ``optical``: Normalize (uint8 tiles) and the
        plan's turbidity."""
        if t.dim() != 4 or not t.is_cuda or t.shape[0] != plan.ops.numel():
            raise ValueError("an image batch is a 4-D tensor on the plan's ROCm device with one "
                             f"item per move code, got {tuple(t.shape)} on {t.device}")
        turb = plan.turb if optical else None
        transpose = plan.mode == "dihedral"
        if t.dtype == torch.uint8:
            if t.shape[-1] not in (1, 3):
                raise ValueError("decoded tiles are uint8 [B, H, W, C] with C = 1 or 3")
            if transpose and staging.TILE_SIZE[0] != staging.TILE_SIZE[1]:
                raise ValueError("\"dihedral\" needs a square staged tile")
            mean, std = (staging.OPTICAL_MEAN, staging.OPTICAL_STD) if optical else (None, None)
            # mode "none": no codes, so the plain kernel runs (with turbidity, the per-item one)
            codes = None if plan.mode == "none" else plan.ops
            return staging.resize_to_tensor_aug(t, codes, turb, transpose, staging.TILE_SIZE,
                                                mean, std, self.depth)
        if t.dtype != torch.float32:
            raise ValueError(f"an image batch is uint8 HWC or fp32 NCHW, got {t.dtype}")
        if transpose and t.shape[-2] != t.shape[-1]:
            raise ValueError(f"\"dihedral\" needs square tiles, got {tuple(t.shape[-2:])}; "
                             "use mode=\"flips\"")
        if plan.mode == "none" and turb is None:
            return t
        return staging.stage_f32_aug(t, plan.ops, turb, transpose, self.depth)

    def apply(self, plan, inputs, bathy, sss):
        """(inputs, bathy, sss) under one plan: the same moves to all three, the turbidity to
        ``inputs`` (the optical tile) only."""
        return (self.apply_one(plan, inputs, optical=True), self.apply_one(plan, bathy),
                self.apply_one(plan, sss))

    def __call__(self, inputs, bathy, sss):
        return self.apply(self.draw(inputs.shape[0], inputs.device), inputs, bathy, sss)


class AugmentedLoader:
    """A train loader of the reference's batch dicts (``main_image``, ``bathy_image``,
    ``sss_image``, ``patch_bathy[...]``, ``patch_sss[...]``, ``label``, ...) whose image entries
    arrive on ``device`` already augmented, one plan per batch for all of them.  With
    ``patch_types = (bathy_patch_type, sss_patch_type)`` only those two patch entries are moved
    and transformed, the others are left as they are; every non-image entry is left alone.
    ``len()``, ``batch_size``, ``dataset`` and every other attribute come from the wrapped
    loader, so ``train_multimodal_model`` / ``train_unimodal_model`` and the loop_utils drivers
    take it in the loader's place (``mauv.train._tile_to`` passes fp32 device tensors through).
    Wrap the train loader only: evaluation and prediction see the tiles as they are."""

    IMAGE_KEYS = ("main_image", "bathy_image", "sss_image")

    def __init__(self, loader, augment, device, patch_types=None):
        if patch_types is not None and len(patch_types) != 2:
            raise ValueError("patch_types is None or (bathy_patch_type, sss_patch_type)")
        self.loader, self.augment, self.device = loader, augment, torch.device(device)
        self.patch_types = patch_types

    def __len__(self):
        return len(self.loader)

    def __getattr__(self, name):     # only what this object lacks: batch_size, dataset, sampler...
        if name == "loader":
            raise AttributeError(name)
        return getattr(self.loader, name)

    def _image(self, plan, t, optical=False):
        return self.augment.apply_one(plan, t.to(self.device, non_blocking=True), optical)

    def __iter__(self):
        for batch in self.loader:
            if not isinstance(batch, dict) or "main_image" not in batch:
                raise TypeError("AugmentedLoader wraps a train loader of batch dicts with a "
                                "'main_image' entry")
            out = dict(batch)
            plan = self.augment.draw(batch["main_image"].shape[0], self.device)
            for key in self.IMAGE_KEYS:
                if key in batch:
                    out[key] = self._image(plan, batch[key], optical=key == "main_image")
            for slot, key in enumerate(("patch_bathy", "patch_sss")):
                if key not in batch:
                    continue
                chosen = None if self.patch_types is None else self.patch_types[slot]
                out[key] = {k: self._image(plan, v)
                            if self.patch_types is None or k == chosen else v
                            for k, v in batch[key].items()}
            yield out
