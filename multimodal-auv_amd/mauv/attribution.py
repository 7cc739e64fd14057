"""Input gradients of the MC models: pixel attributions, modality shares, gradient-sign noise.

Plain autograd reaches the images through every mauv entry (``ResNet.forward`` / ``mc_forward``,
``ResNet50Custom``, ``MultiModalModel``): the trunks' backward ends in the stems' data gradient
(stem_dgrad.hip), summed over the MC samples.  The helpers here are pure torch on top of that.

Batch coupling.  With live BatchNorm (``model.train()``, the reference's MC mode) every item's
activations depend on the whole batch, so a score is differentiated as the batch SUM: row ``i``
of a gradient then also holds what item ``i`` contributed to the other items' scores through the
batch statistics.  Under ``mauv.freeze_batchnorm`` predictions do not depend on the rest of the
batch and row ``i`` is exactly item ``i``'s own attribution.

The helpers freeze the parameters while they run (and restore them): no parameter gradient is
written or accumulated, and no weight-gradient kernel is launched.

Side effects.  Each call is an ordinary forward of the model in the mode it is in: it draws the
next ``num_mc`` MC samples (the model's sample counter advances, so two calls see different
weights unless the counter or an epsilon provider is set), and with live BatchNorm in
``train()`` mode it moves the running statistics like any other training-mode forward.  After
``mauv.freeze_batchnorm(model)`` no buffer moves.
"""
import contextlib

import torch


def _tuple(inputs):
    return (inputs,) if torch.is_tensor(inputs) else tuple(inputs)


def _mc_logits(model, num_mc, xs):
    if hasattr(model, "mc_forward"):
        return model.mc_forward(*xs, num_mc)
    return torch.stack([model(*xs) for _ in range(num_mc)])


@contextlib.contextmanager
def _params_frozen(model):
    live = [p for p in model.parameters() if p.requires_grad]
    for p in live:
        p.requires_grad_(False)
    try:
        yield
    finally:
        for p in live:
            p.requires_grad_(True)


def _leaves(model, inputs):
    """Fresh leaf copies of the inputs on the model's device that require grad."""
    dev = next(model.parameters()).device
    return tuple(x.detach().to(dev, torch.float32).requires_grad_(True) for x in _tuple(inputs))


def predicted_score(logits):
    """Sum over the batch of each item's MC-mean logit of its predicted class."""
    mean = logits.float().mean(0)
    return mean.gather(1, mean.argmax(1, keepdim=True)).sum()


def entropy_score(logits, eps=1e-7):
    """Sum over the batch of the predictive entropy of the MC-mean softmax (mc_eval_stats')."""
    p = torch.softmax(logits.float(), dim=2).mean(0)
    return -(p * torch.log(p + eps)).sum()


_SCORES = {"predicted": predicted_score, "entropy": entropy_score}


def input_gradients(model, inputs, num_mc=1, score="predicted"):
    """``(grads, logits)``: the gradient of a scalar score of the ``[num_mc, B, C]`` logits with
    respect to every input (a tensor for a tensor, a tuple for a tuple of modalities), and the
    detached logits.  ``score``: "predicted" (each item's MC-mean logit of its predicted class),
    "entropy" (the predictive entropy of the MC-mean softmax), both summed over the batch, or a
    callable mapping the logits to a scalar.  See the module docstring for batch coupling."""
    fn = _SCORES.get(score, score) if isinstance(score, str) else score
    if not callable(fn):
        raise ValueError(f'score must be "predicted", "entropy" or a callable, got {score!r}')
    xs = _leaves(model, inputs)
    with _params_frozen(model), torch.enable_grad():
        logits = _mc_logits(model, num_mc, xs)
        grads = torch.autograd.grad(fn(logits), xs)
    return (grads[0] if torch.is_tensor(inputs) else grads), logits.detach()


def modality_shares(grads):
    """``[B, n_modalities]``: each modality's share of the per-item L2 norm of the gradients
    (``grads``: one ``[B, ...]`` tensor per modality); rows sum to 1 (an item whose gradients
    are all zero gets equal shares)."""
    norms = torch.stack([g.detach().float().flatten(1).norm(dim=1) for g in _tuple(grads)], 1)
    total = norms.sum(1, keepdim=True)
    return torch.where(total > 0, norms / total.clamp_min(1e-38),
                       torch.full_like(norms, 1.0 / norms.shape[1]))


def fgsm(model, inputs, labels, criterion, eps, num_mc=1):
    """The inputs moved by ``eps * sign(d loss / d input)``, loss = ``criterion`` of the MC-mean
    logits (the training loss without its KL term): the worst-case first-order perturbation of
    size ``eps`` per element, the adversarial companion of the reference's noise Examples.
    Returns detached tensors on the model's device, shaped like ``inputs``."""
    xs = _leaves(model, inputs)
    with _params_frozen(model), torch.enable_grad():
        logits = _mc_logits(model, num_mc, xs)
        loss = criterion(logits.float().mean(0), labels.to(logits.device))
        grads = torch.autograd.grad(loss, xs)
    out = tuple((x + eps * g.sign()).detach() for x, g in zip(xs, grads))
    return out[0] if torch.is_tensor(inputs) else out
