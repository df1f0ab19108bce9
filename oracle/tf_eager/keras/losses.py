"""keras.losses of the two schemes in scope, reduced with SUM_OVER_BATCH_SIZE."""
import torch

from .._core import wrap
from . import backend


class Loss:
    def __init__(self, name=None, **kwargs):
        self.name = name


class MeanAbsoluteError(Loss):
    def __call__(self, y_true, y_pred):
        return wrap(torch.abs(y_pred - y_true.to(y_pred.dtype)).mean(dim=-1).mean())


class SparseCategoricalCrossentropy(Loss):
    def __init__(self, from_logits=False, **kwargs):
        super().__init__(**kwargs)
        self.from_logits = from_logits

    def __call__(self, y_true, y_pred):
        return wrap(backend.sparse_categorical_crossentropy(y_true, y_pred, self.from_logits).mean())
