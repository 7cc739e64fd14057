"""Frozen BatchNorm: fine-tune and predict on the stored running statistics.

The reference keeps every model in ``.train()`` for training, evaluation and prediction, so each
BatchNorm normalises with the batch in front of it and every call moves its running statistics.
``freeze_batchnorm`` pins the BatchNorms of a module to their running statistics instead — the
standard recipe for retraining a checkpoint on a small new survey, and what makes a prediction
independent of the other items of its batch — in a way the drop-in loops cannot undo: they call
``model.train()`` at the top of every epoch, and a ``FrozenBatchNorm2d`` stays in eval through it.

The engine decides per BatchNorm (``bn.training``): a frozen one takes its scale / shift from the
running statistics (ops.bn_eval_stats), updates nothing, and its backward is dy = scale * dz
(ops.bn_bwd_frozen).  Host (CPU) models and plain torch modules work too: torch's own eval-mode
``F.batch_norm`` does the rest there.
"""
import torch.nn as nn

from . import engine

# instance attributes a frozen BatchNorm carries (they travel with deepcopy / pickle)
_FROM = "_mauv_frozen_from"       # the class it had
_AFFINE = "_mauv_frozen_affine"   # (weight.requires_grad, bias.requires_grad) before freeze_affine


class FrozenBatchNorm2d(nn.BatchNorm2d):
    """An ``nn.BatchNorm2d`` (same parameters, buffers and state_dict keys) that normalises with
    its running statistics whatever mode its parent is put in: ``train(mode)`` leaves
    ``training`` False."""

    def train(self, mode=True):
        if not isinstance(mode, bool):
            raise ValueError("training mode is expected to be boolean")
        return super().train(False)


def _batchnorms(module):
    return [m for m in module.modules() if isinstance(m, nn.BatchNorm2d)]


def freeze_batchnorm(module, freeze_affine=False, root=None):
    """Pin every ``nn.BatchNorm2d`` under ``module`` to its running statistics, in place: each
    becomes a ``FrozenBatchNorm2d`` in eval.  ``freeze_affine`` also stops gamma / beta from
    training (``requires_grad=False``; unfreeze_batchnorm restores the flags they had).
    ``root``: the model whose engine state holds ``module`` (a trunk of a MultiModalModel: pass
    the model); that state — gradient arena, trainable list, sample counter, eps_provider — is
    rebuilt at the next call.  Returns the number of BatchNorms now frozen under ``module``.
    Raises ValueError, changing nothing, if one of them keeps no running statistics."""
    bns = _batchnorms(module)
    for bn in bns:
        if not bn.track_running_stats or bn.running_mean is None or bn.running_var is None:
            raise ValueError("freeze_batchnorm: a BatchNorm2d without running statistics "
                             "(track_running_stats=False) has nothing to freeze to")
    for bn in bns:
        if not isinstance(bn, FrozenBatchNorm2d):
            bn.__dict__[_FROM] = bn.__class__
            bn.__class__ = FrozenBatchNorm2d
        bn.train(False)
        if freeze_affine and bn.affine and _AFFINE not in bn.__dict__:
            bn.__dict__[_AFFINE] = (bn.weight.requires_grad, bn.bias.requires_grad)
            bn.weight.requires_grad_(False)
            bn.bias.requires_grad_(False)
    engine.invalidate(root if root is not None else module)
    return len(bns)


def unfreeze_batchnorm(module, root=None):
    """Undo freeze_batchnorm under ``module``: every frozen BatchNorm gets its class and its
    gamma / beta ``requires_grad`` flags back and the mode of its parent (``module`` itself, if
    it is one: train).  Returns the number of BatchNorms unfrozen."""
    n = 0
    for parent, bn in [(None, module)] + [(p, c) for p in module.modules()
                                          for c in p.children()]:
        if not isinstance(bn, FrozenBatchNorm2d) or _FROM not in bn.__dict__:
            continue
        bn.__class__ = bn.__dict__.pop(_FROM)
        flags = bn.__dict__.pop(_AFFINE, None)
        if flags is not None:
            bn.weight.requires_grad_(flags[0])
            bn.bias.requires_grad_(flags[1])
        bn.train(True if parent is None else parent.training)
        n += 1
    engine.invalidate(root if root is not None else module)
    return n
