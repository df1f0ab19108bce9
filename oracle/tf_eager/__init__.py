"""An eager stand-in, on torch, for the part of the TensorFlow 2 / Keras API that the reference's model code calls.

TEST INFRASTRUCTURE ONLY.  oracle/ref_exec.py registers this package under the name `tensorflow`, imports the reference's
model modules from where they lie and runs them unmodified on concrete tensors: in fp64 (the default working dtype) to pin
oracle/egt_oracle.py and oracle/egt_model_oracle.py by execution, in fp32 to reproduce the rounding of the additive masks.
torch autograd differentiates through it.  Nothing of the reference's text lives here; what lives here is our reading of the
PUBLIC API semantics, and that reading is what stays "by construction".  Every default that is hard-coded is in this table:

    what                              value here                                                     TensorFlow 2.1 source of the rule
    --------------------------------  -------------------------------------------------------------  ---------------------------------
    float dtypes                      every float dtype asked for (tf.float32 included, Python       floatx is float32; here the
                                      float constants too) is the session's working dtype            working dtype replaces it
    Dense                             tensordot(x, kernel [in,out]) + bias, then the activation;     keras/layers/core.py Dense
                                      weights 'kernel', 'bias'; supports_masking (mask passes)
    LayerNormalization                axis -1, epsilon 1e-3, biased variance; inv = rsqrt(var+eps)   keras/layers/normalization.py,
                                      * gamma; x * inv + (beta - mean * inv); weights 'gamma',       nn.batch_normalization
                                      'beta'; mask passes
    Embedding                         lookup of int(inputs) in 'embeddings' [input_dim, output_dim]; keras/layers/embeddings.py
                                      mask_zero: mask = inputs != 0, row 0 stays an ordinary row
    Masking                           keep = any(x != mask_value, axis -1); outputs x * keep;        keras/layers/core.py Masking
                                      mask = keep
    Dropout / tf.nn.dropout           inverted: x * (1 / (1 - rate)) * keep, only when training;     nn_ops.dropout_v2
                                      the keep mask is INJECTED, never drawn; mask passes
    Add                               inputs summed left to right; mask = AND of the non-None masks  keras/layers/merge.py _Merge
    Concatenate                       axis -1; all-None masks -> None, else AND over the             keras/layers/merge.py
                                      concatenated masks (None = all True)
    Flatten                           reshape [B, -1]; no mask support: the mask is dropped          keras/layers/core.py Flatten
    Activation / LeakyReLU            'elu' (alpha 1), 'relu', 'linear'/None; LeakyReLU max(ax, x),  keras/activations.py,
                                      alpha 0.3 unless given; mask passes                            advanced_activations.py
    Input                             the fed batch tensor; dtype float32 unless given, i.e. the     keras/engine/input_layer.py
                                      working dtype (integer features arrive as floats, as in Keras)
    Embedding bounds                  an index outside [0, input_dim) raises, as TensorFlow's CPU    embedding_ops / gather
                                      kernel does (its GPU kernel would return zeros instead)
    Lambda                            function(inputs[, mask=][, training=]); without `mask=` the    keras/layers/core.py Lambda
                                      output has no mask; with a callable `mask=` it computes it
    GlobalAveragePooling1D            with a mask: sum(x * m, 1) / sum(m, 1); without: mean(x, 1);   keras/layers/pooling.py
                                      output mask None
    Layer.__call__                    input masks = each input's `_keras_mask`; `mask=` is passed    keras/engine/base_layer.py
                                      only when `call` names it and some mask is not None (a list,   __call__, _collect_input_masks,
                                      one per input, for list inputs); `training=` is passed when    _set_mask_metadata, compute_mask
                                      `call` names it (the learning phase); the output mask is
                                      computed only when the layer sets supports_masking or
                                      overrides compute_mask; the default compute_mask passes the
                                      mask on; outputs that are the input objects keep their masks
    add_weight                        a NaN-filled leaf unless the initializer is Constant: a        --
                                      weight nobody loads poisons the outputs instead of hiding
    softmax                           max-subtracted (torch.softmax)                                 nn_ops.softmax
    clip_by_value gradient            passes where lo <= x <= hi                                     clip_ops._clip_by_value_grad
    math.round                        half to even                                                   math_ops.round
    sparse_categorical_crossentropy   logsumexp(logits) - logits[target]                             keras/backend.py
    losses.MeanAbsoluteError,         mean over the last axis, then over the batch                   keras/losses.py,
    SparseCategoricalCrossentropy     (SUM_OVER_BATCH_SIZE)                                          losses_utils
    add_loss                          appended to the layer's `losses`; the total loss of a model    keras/engine/training.py
                                      is the compiled loss plus the sum of them
"""
from __future__ import annotations

import builtins as _b
import types

import torch

from . import _core
from ._core import Tensor, TensorShape, wrap, session  # noqa: F401

float32, float64, float16 = torch.float32, torch.float64, torch.float16
int32, int64, bool = torch.int32, torch.int64, torch.bool          # noqa: A001  (the reference says tf.bool)

# (this module defines `bool` and `abs`, as TensorFlow does: built-ins are spelled through `builtins` below)
_isinstance, _tuple, _list, _int, _float = _b.isinstance, _b.tuple, _b.list, _b.int, _b.float


def _t(x):
    """a tensor of the working dtype (floats) from a tensor or a Python constant"""
    if _isinstance(x, torch.Tensor):
        return wrap(x)
    t = torch.as_tensor(x)
    if t.is_floating_point():
        t = t.to(_core.working_dtype())
    return wrap(t)


def _ints(shape):
    return [_int(s) for s in shape]


def shape(x):
    return TensorShape(_t(x).size())


def reshape(x, shape):
    return wrap(torch.reshape(_t(x), _ints(shape)))


def unstack(x, num=None, axis=0):
    if not _isinstance(x, torch.Tensor):
        return _list(x)
    parts = _list(torch.unbind(x, dim=axis))
    if num is not None and len(parts) != num:
        raise ValueError(f"unstack: num={num}, axis {axis} has {len(parts)}")
    return [wrap(p) for p in parts]


def stack(values, axis=0):
    return wrap(torch.stack([_t(v) for v in values], dim=axis))


def einsum(equation, *operands):
    return wrap(torch.einsum(equation, *[_t(o) for o in operands]))


def matmul(a, b, transpose_a=False, transpose_b=False):
    a, b = _t(a), _t(b)
    if transpose_a:
        a = a.transpose(-1, -2)
    if transpose_b:
        b = b.transpose(-1, -2)
    return wrap(torch.matmul(a, b))


def clip_by_value(x, clip_value_min, clip_value_max):
    return wrap(torch.clamp(_t(x), _float(clip_value_min), _float(clip_value_max)))


def cast(x, dtype):
    return wrap(_t(x).to(_core.float_dtype(dtype)))


def where(condition, x=None, y=None):
    c = _t(condition)
    x, y = _t(x), _t(y)
    return wrap(torch.where(c, x, y))


def sigmoid(x):
    return wrap(torch.sigmoid(_t(x)))


def _axis(axis):
    return _tuple(axis) if _isinstance(axis, (_list, _tuple)) else axis


def reduce_sum(x, axis=None, keepdims=False):
    x = _t(x)
    return wrap(x.sum() if axis is None else x.sum(dim=_axis(axis), keepdim=keepdims))


def reduce_mean(x, axis=None, keepdims=False):
    x = _t(x)
    return wrap(x.mean() if axis is None else x.mean(dim=_axis(axis), keepdim=keepdims))


def pad(x, paddings, mode="CONSTANT", constant_values=0):
    if mode != "CONSTANT":
        raise NotImplementedError(mode)
    flat = []
    for lo, hi in reversed(_list(paddings)):
        flat += [_int(lo), _int(hi)]
    return wrap(torch.nn.functional.pad(_t(x), flat, value=constant_values))


def concat(values, axis):
    return wrap(torch.cat([_t(v) for v in values], dim=axis))


def split(x, num_or_size_splits, axis=0):
    n = num_or_size_splits
    x = _t(x)
    sizes = x.size(axis) // n if _isinstance(n, _int) else _ints(n)
    return [wrap(p) for p in torch.split(x, sizes, dim=axis)]


def tile(x, multiples):
    return wrap(_t(x).repeat(*_ints(multiples)))


def transpose(x, perm=None):
    x = _t(x)
    return wrap(x.permute(*(perm if perm is not None else reversed(range(x.dim())))))


def one_hot(indices, depth, dtype=None):
    return wrap(torch.nn.functional.one_hot(_t(indices).long(), _int(depth)).to(_core.float_dtype(dtype)))


def ones(shape, dtype=None):
    return wrap(torch.ones(_ints(shape), dtype=_core.float_dtype(dtype)))


def zeros(shape, dtype=None):
    return wrap(torch.zeros(_ints(shape), dtype=_core.float_dtype(dtype)))


def constant(value, dtype=None):
    t = _t(value)
    return t if dtype is None else cast(t, dtype)


def expand_dims(x, axis):
    return wrap(torch.unsqueeze(_t(x), axis))


def squeeze(x, axis=None):
    x = _t(x)
    if axis is None:
        return wrap(x.squeeze())
    for a in sorted(_axis(axis) if _isinstance(axis, (_list, _tuple)) else (axis,), reverse=True):
        x = x.squeeze(a)
    return wrap(x)


def abs(x):  # noqa: A001
    return wrap(torch.abs(_t(x)))


def square(x):
    x = _t(x)
    return wrap(x * x)


def minimum(x, y):
    return wrap(torch.minimum(_t(x), _t(y).to(_t(x).dtype)))


def maximum(x, y):
    return wrap(torch.maximum(_t(x), _t(y).to(_t(x).dtype)))


class VariableAggregation:
    NONE, SUM, MEAN, ONLY_FIRST_REPLICA = range(4)


def _module(name, **members):
    m = types.ModuleType(f"{__name__}.{name}")
    m.__dict__.update(members)
    return m


# ---------------------------------------------------------------------------------------------------- tf.nn -----
def _softmax(logits, axis=-1):
    return wrap(torch.softmax(_t(logits), dim=axis))


def _dropout(x, rate, noise_shape=None, seed=None, name=None):
    """nn_ops.dropout_v2: x * (1 / (1 - rate)) * keep, with the keep mask injected (session(keep=[...]))"""
    x = _t(x)
    if noise_shape is not None:
        raise NotImplementedError("noise_shape")
    keep = _core.take_keep(x.size())
    return wrap(x * (1.0 / (1.0 - _float(rate))) * keep)


nn = _module("nn", softmax=_softmax, dropout=_dropout,
             elu=lambda x: wrap(torch.nn.functional.elu(_t(x))), relu=lambda x: wrap(torch.relu(_t(x))))


# ------------------------------------------------------------------------------------------------ tf.random -----
def _uniform(shape, minval=0, maxval=None, dtype=None, seed=None, name=None):
    """the next injected sample (session(uniform=[...])), which is taken to lie in [0, 1)"""
    if _float(minval) != 0.0 or (maxval is not None and _float(maxval) != 1.0):
        raise NotImplementedError("tf.random.uniform: only [0, 1)")
    return _core.take_uniform(_ints(shape))


random = _module("random", uniform=_uniform)


# -------------------------------------------------------------------------------------------------- tf.math -----
def _add_n(inputs):
    out = _t(inputs[0])
    for v in inputs[1:]:
        out = out + _t(v)
    return wrap(out)


def _divide_no_nan(x, y):
    x, y = _t(x), _t(y)
    safe = torch.where(y == 0, torch.ones_like(y), y)
    return wrap(torch.where(y == 0, torch.zeros_like(x / safe), x / safe))


math = _module("math", log=lambda x: wrap(torch.log(_t(x))), round=lambda x: wrap(torch.round(_t(x))), add_n=_add_n,
               divide_no_nan=_divide_no_nan, reduce_sum=reduce_sum, reduce_mean=reduce_mean, sigmoid=sigmoid)

from . import keras  # noqa: E402,F401
