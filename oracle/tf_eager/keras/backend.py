"""keras.backend: the learning phase and the sparse cross-entropy."""
import torch

from .. import _core
from .._core import wrap


def learning_phase():
    return _core.STATE.training


def set_learning_phase(value):
    _core.STATE.training = bool(value)


def floatx():
    return _core.working_dtype()


def sparse_categorical_crossentropy(target, output, from_logits=False, axis=-1):
    """per element: logsumexp(logits) - logits[target] (from probabilities: -log p[target])"""
    if axis != -1:
        raise NotImplementedError
    logp = output - torch.logsumexp(output, dim=-1, keepdim=True) if from_logits else torch.log(output)
    idx = target.to(torch.int64)
    if idx.dim() == logp.dim():
        idx = idx.squeeze(-1)
    return wrap(-logp.gather(-1, idx[..., None])[..., 0])
