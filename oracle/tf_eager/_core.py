"""State and the tensor type of the eager stand-in: working dtype, learning phase, fed inputs, injected samples."""
from __future__ import annotations

import contextlib

import torch


class TensorShape(tuple):
    """what `tensor.shape` answers: a tuple of ints with TensorFlow's `.rank` / `.as_list()`"""

    @property
    def rank(self):
        return len(self)

    def as_list(self):
        return list(self)

    def numel(self):
        n = 1
        for s in self:
            n *= s
        return n

    def __getitem__(self, i):
        r = tuple.__getitem__(self, i)
        return TensorShape(r) if isinstance(i, slice) else r

    def __add__(self, other):
        return TensorShape(tuple(self) + tuple(other))


class Tensor(torch.Tensor):
    """a torch tensor that also answers the few TensorFlow tensor attributes the reference touches: `.shape.rank`,
    `.set_shape()` (checks the static shape instead of setting it) and a per-object `_keras_mask`.  Results of torch
    operations are fresh objects of this class and therefore carry no mask, as in TensorFlow."""

    @property
    def shape(self):
        return TensorShape(self.size())

    def set_shape(self, shape):
        shape = list(shape)
        if len(shape) != self.dim():
            raise ValueError(f"set_shape{shape}: tensor has rank {self.dim()}")
        for want, have in zip(shape, self.size()):
            if want is not None and int(want) != have:
                raise ValueError(f"set_shape{shape}: tensor has shape {tuple(self.size())}")

    def numpy(self):
        return self.detach().as_subclass(torch.Tensor).numpy()


def wrap(t) -> Tensor:
    if isinstance(t, Tensor):
        return t
    if not isinstance(t, torch.Tensor):
        t = torch.as_tensor(t)
    return t.as_subclass(Tensor)


class _State:
    dtype = torch.float64          # the working dtype: every float the reference asks for (tf.float32 included) is this one
    training = False               # keras.backend.learning_phase()
    feed = {}                      # Input(name=...) -> the concrete batch tensor
    uniform = []                   # samples handed out, in order, by tf.random.uniform
    keep = []                      # keep masks handed out, in order, by tf.nn.dropout and unnamed Dropout layers
    keep_by_name = {}              # Dropout layer name -> keep mask
    weights = None                 # `layer/weight` -> initial value, taken by add_weight (None: weights start as NaN)


STATE = _State()


def working_dtype():
    return STATE.dtype


def float_dtype(dtype):
    """the torch dtype a requested TensorFlow dtype means here"""
    if dtype is None:
        return STATE.dtype
    if isinstance(dtype, str):
        dtype = getattr(torch, dtype)
    return STATE.dtype if dtype.is_floating_point else dtype


@contextlib.contextmanager
def session(*, dtype=torch.float64, training=False, feed=None, uniform=(), keep=(), keep_by_name=None, weights=None):
    """one run of reference code: the working dtype, the learning phase, the batch behind every `Input`, and the random
    samples in the order (or under the Dropout layer names) the code will ask for them.  A sample that is asked for and was
    not injected is an error, and so is one that is left over.  `weights` ({`layer/weight`: array}) initialises the weights
    the layers create during the run; with it, a weight that is created and not listed, or listed and never created, is an
    error."""
    saved = {k: getattr(STATE, k) for k in ("dtype", "training", "feed", "uniform", "keep", "keep_by_name", "weights")}
    STATE.dtype, STATE.training = dtype, bool(training)
    STATE.feed = dict(feed or {})
    STATE.uniform, STATE.keep, STATE.keep_by_name = list(uniform), list(keep), dict(keep_by_name or {})
    STATE.weights = None if weights is None else dict(weights)
    try:
        yield STATE
        if STATE.weights:
            raise KeyError(f"weights the run never created: {sorted(STATE.weights)}")
        left = len(STATE.uniform) + len(STATE.keep) + len(STATE.keep_by_name)
        if left:
            raise RuntimeError(f"{left} injected random sample(s) were never asked for")
    finally:
        for k, v in saved.items():
            setattr(STATE, k, v)


def take_uniform(shape):
    if not STATE.uniform:
        raise RuntimeError("tf.random.uniform: no injected sample left (the stand-in never draws one itself)")
    u = wrap(torch.as_tensor(STATE.uniform.pop(0)).to(STATE.dtype))
    if tuple(u.size()) != tuple(int(s) for s in shape):
        raise ValueError(f"tf.random.uniform{tuple(shape)}: the injected sample has shape {tuple(u.size())}")
    return u


def take_keep(shape, name=None):
    if name is not None and name in STATE.keep_by_name:
        k = STATE.keep_by_name.pop(name)
    elif STATE.keep:
        k = STATE.keep.pop(0)
    else:
        raise RuntimeError(f"dropout {name or ''}: no injected keep mask left (the stand-in never draws one itself)")
    k = wrap(torch.as_tensor(k).to(STATE.dtype))
    if tuple(k.size()) != tuple(int(s) for s in shape):
        raise ValueError(f"dropout {name or ''}: the injected keep mask has shape {tuple(k.size())}, the input {tuple(shape)}")
    return k
