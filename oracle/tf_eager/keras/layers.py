"""The Keras layers the reference's models use, eager, on torch.  The rules are the table in oracle/tf_eager/__init__.py."""
from __future__ import annotations

import inspect

import torch

from .. import _core
from .._core import TensorShape, wrap
from . import initializers as _init

_uid = {}


def _default_name(cls):
    n = _uid[cls] = _uid.get(cls, 0) + 1
    return f"{cls.__name__.lower()}_{n}"


def _is_list(x):
    return isinstance(x, (list, tuple))


def activation_fn(name):
    if name is None or name == "linear":
        return lambda x: x
    if callable(name):
        return name
    if name == "elu":
        return lambda x: wrap(torch.nn.functional.elu(x))
    if name == "relu":
        return lambda x: wrap(torch.relu(x))
    raise NotImplementedError(f"activation {name!r}")


class Layer:
    def __init__(self, name=None, dtype=None, trainable=True, **kwargs):
        if kwargs:
            raise TypeError(f"{type(self).__name__}: unknown arguments {sorted(kwargs)}")
        self.name = name or _default_name(type(self))
        self.trainable = trainable
        self.built = False
        self.supports_masking = False
        self._weights = {}
        self._trainable = {}
        self.losses = []
        self.metrics = {}

    # ---- weights ----
    def add_weight(self, name=None, shape=None, dtype=None, initializer=None, regularizer=None, trainable=True, constraint=None,
                   aggregation=None, **kwargs):
        dt = _core.float_dtype(dtype)
        shape = [int(s) for s in (shape or [])]
        key = f"{self.name}/{name}"
        given = _core.STATE.weights
        if isinstance(initializer, _init.Constant):
            w = torch.full(shape, initializer.value, dtype=dt)
        elif given is not None and trainable:
            if key not in given:
                raise KeyError(f"{key}: the run creates this weight and no value was given for it")
            w = torch.as_tensor(given.pop(key)).to(dt).clone()
            if list(w.shape) != shape:
                raise ValueError(f"{key}: created as {shape}, given {list(w.shape)}")
        else:   # never a silent default: a weight that nobody loads poisons whatever reads it
            w = torch.full(shape, float("nan"), dtype=dt) if dt.is_floating_point else torch.zeros(shape, dtype=dt)
        w = wrap(w)
        if trainable and dt.is_floating_point:
            w.requires_grad_()
        self._weights[name] = w
        self._trainable[name] = bool(trainable)
        return w

    @property
    def weights(self):
        return list(self._weights.values())

    def get_weights(self):
        return [w.numpy() for w in self._weights.values()]

    def add_loss(self, loss):
        self.losses.append(loss)

    def add_metric(self, value, name=None, aggregation=None):
        self.metrics[name] = value

    def get_config(self):
        return dict(name=self.name)

    # ---- the call protocol ----
    def build(self, input_shape):
        self.built = True

    def call(self, inputs, **kwargs):
        return inputs

    def compute_mask(self, inputs, mask=None):
        if not self.supports_masking:
            ms = mask if _is_list(mask) else [mask]
            if any(m is not None for m in ms):
                raise TypeError(f"Layer {self.name} does not support masking, but was passed an input_mask")
            return None
        return mask

    compute_mask._is_default = True

    def __call__(self, inputs, **kwargs):
        if _is_list(inputs):
            inputs = [wrap(x) for x in inputs]
            masks = [getattr(x, "_keras_mask", None) for x in inputs]
            shapes = [TensorShape(x.size()) for x in inputs]
            in_mask = masks if any(m is not None for m in masks) else None
        else:
            inputs = wrap(inputs)
            in_mask = getattr(inputs, "_keras_mask", None)
            shapes = TensorShape(inputs.size())
        if not self.built:
            self.build(shapes)
            self.built = True
        names = inspect.signature(self.call).parameters
        if "mask" in names and "mask" not in kwargs and in_mask is not None:
            kwargs["mask"] = in_mask
        if "training" in names and kwargs.get("training") is None:
            kwargs["training"] = _core.STATE.training
        outputs = self.call(inputs, **kwargs)
        self.input, self.output = inputs, outputs      # Keras' layer.input / layer.output (of the latest call)
        # _set_mask_metadata
        flat = list(outputs) if _is_list(outputs) else [outputs]
        if all(getattr(o, "_keras_mask", None) is not None for o in flat):
            return outputs
        should = self.supports_masking or not getattr(self.compute_mask, "_is_default", False)
        out_masks = self.compute_mask(inputs, in_mask) if should else None
        if out_masks is None:
            flat_masks = [None] * len(flat)
        else:
            flat_masks = list(out_masks) if _is_list(out_masks) else [out_masks]
        for o, m in zip(flat, flat_masks):
            if isinstance(o, torch.Tensor):
                o._keras_mask = m
        return outputs


def Input(shape=None, name=None, dtype=None, **kwargs):
    """the concrete batch tensor fed under `name` (session(feed={name: tensor})), floats in the working dtype"""
    if name not in _core.STATE.feed:
        raise KeyError(f"Input {name!r}: nothing fed under this name")
    t = torch.as_tensor(_core.STATE.feed[name])
    t = wrap(t.to(_core.float_dtype(dtype or torch.float32)).clone())
    for want, have in zip(list(shape or []), list(t.size())[1:]):
        if want is not None and int(want) != have:
            raise ValueError(f"Input {name!r}: declared {list(shape)}, fed {list(t.size())}")
    if shape is not None and len(shape) != t.dim() - 1:
        raise ValueError(f"Input {name!r}: declared {list(shape)}, fed {list(t.size())}")
    return t


class Dense(Layer):
    def __init__(self, units, activation=None, use_bias=True, kernel_initializer="glorot_uniform", bias_initializer="zeros",
                 kernel_regularizer=None, bias_regularizer=None, activity_regularizer=None, kernel_constraint=None,
                 bias_constraint=None, **kwargs):
        super().__init__(**kwargs)
        self.units, self.activation, self.use_bias = int(units), activation_fn(activation), use_bias
        self.kernel_regularizer = kernel_regularizer
        self.supports_masking = True

    def build(self, input_shape):
        self.kernel = self.add_weight("kernel", [input_shape[-1], self.units])
        self.bias = self.add_weight("bias", [self.units]) if self.use_bias else None

    def call(self, inputs):
        y = torch.matmul(inputs, self.kernel)
        if self.bias is not None:
            y = y + self.bias
        return self.activation(wrap(y))


class LayerNormalization(Layer):
    def __init__(self, axis=-1, epsilon=1e-3, center=True, scale=True, **kwargs):
        super().__init__(**kwargs)
        if axis != -1 or not (center and scale):
            raise NotImplementedError
        self.epsilon = epsilon
        self.supports_masking = True

    def build(self, input_shape):
        self.gamma = self.add_weight("gamma", [input_shape[-1]])
        self.beta = self.add_weight("beta", [input_shape[-1]])

    def call(self, inputs):
        mean = inputs.mean(dim=-1, keepdim=True)
        variance = ((inputs - mean) ** 2).mean(dim=-1, keepdim=True)
        inv = torch.rsqrt(variance + self.epsilon) * self.gamma
        return wrap(inputs * inv + (self.beta - mean * inv))


class BatchNormalization(Layer):
    def __init__(self, **kwargs):
        raise NotImplementedError("BatchNormalization: no shipped config asks for it")


class Embedding(Layer):
    def __init__(self, input_dim, output_dim, embeddings_initializer="uniform", embeddings_regularizer=None,
                 activity_regularizer=None, embeddings_constraint=None, mask_zero=False, input_length=None, **kwargs):
        super().__init__(**kwargs)
        self.input_dim, self.output_dim, self.mask_zero = int(input_dim), int(output_dim), mask_zero
        self.supports_masking = mask_zero

    def build(self, input_shape):
        self.embeddings = self.add_weight("embeddings", [self.input_dim, self.output_dim])

    def call(self, inputs):
        idx = inputs.to(torch.int64).as_subclass(torch.Tensor)
        if int(idx.min()) < 0 or int(idx.max()) >= self.input_dim:
            raise IndexError(f"{self.name}: index outside [0, {self.input_dim})")
        return wrap(self.embeddings[idx])

    def compute_mask(self, inputs, mask=None):
        if not self.mask_zero:
            return None
        return wrap(inputs != 0)


class Masking(Layer):
    def __init__(self, mask_value=0., **kwargs):
        super().__init__(**kwargs)
        self.mask_value = mask_value
        self.supports_masking = True

    def compute_mask(self, inputs, mask=None):
        return wrap((inputs != self.mask_value).any(dim=-1))

    def call(self, inputs):
        keep = (inputs != self.mask_value).any(dim=-1, keepdim=True)
        out = wrap(inputs * keep.to(inputs.dtype))
        out._keras_mask = wrap(keep.squeeze(-1))
        return out


class Dropout(Layer):
    def __init__(self, rate, noise_shape=None, seed=None, **kwargs):
        super().__init__(**kwargs)
        if noise_shape is not None:
            raise NotImplementedError("noise_shape")
        self.rate = float(rate)
        self.supports_masking = True

    def call(self, inputs, training=None):
        if not training or self.rate <= 0.0:
            return inputs
        keep = _core.take_keep(inputs.size(), self.name)
        return wrap(inputs * (1.0 / (1.0 - self.rate)) * keep)


class _Merge(Layer):
    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        self.supports_masking = True

    def compute_mask(self, inputs, mask=None):
        if mask is None:
            return None
        ms = [m for m in mask if m is not None]
        if not ms:
            return None
        out = ms[0]
        for m in ms[1:]:
            out = out & m
        return wrap(out)


class Add(_Merge):
    def call(self, inputs):
        out = inputs[0]
        for x in inputs[1:]:
            out = out + x
        return wrap(out)


class Concatenate(_Merge):
    def __init__(self, axis=-1, **kwargs):
        super().__init__(**kwargs)
        if axis != -1:
            raise NotImplementedError("Concatenate: only the last axis")

    def call(self, inputs):
        return wrap(torch.cat(list(inputs), dim=-1))

    def compute_mask(self, inputs, mask=None):
        if mask is None or all(m is None for m in mask):
            return None
        ms = []
        for x, m in zip(inputs, mask):     # a missing mask counts as all True; masks of rank n-1 get the feature axis
            m = torch.ones_like(x, dtype=torch.bool) if m is None else (m[..., None].expand_as(x) if m.dim() < x.dim() else m)
            ms.append(m)
        return wrap(torch.cat(ms, dim=-1).all(dim=-1))


class Flatten(Layer):
    def call(self, inputs):
        return wrap(inputs.reshape(inputs.size(0), -1))


class Activation(Layer):
    def __init__(self, activation, **kwargs):
        super().__init__(**kwargs)
        self.activation = activation_fn(activation)
        self.supports_masking = True

    def call(self, inputs):
        return self.activation(inputs)


class LeakyReLU(Layer):
    def __init__(self, alpha=0.3, **kwargs):
        super().__init__(**kwargs)
        self.alpha = float(alpha)
        self.supports_masking = True

    def call(self, inputs):
        return wrap(torch.maximum(self.alpha * inputs, inputs))


class Lambda(Layer):
    def __init__(self, function, output_shape=None, mask=None, arguments=None, **kwargs):
        super().__init__(**kwargs)
        self.function, self.arguments = function, dict(arguments or {})
        if mask is not None:
            self.supports_masking = True
        self.mask = mask

    def call(self, inputs, mask=None, training=None):
        kw = dict(self.arguments)
        names = inspect.signature(self.function).parameters
        if "mask" in names:
            kw["mask"] = mask
        if "training" in names:
            kw["training"] = training
        out = self.function(inputs, **kw)
        return [wrap(o) for o in out] if _is_list(out) else wrap(out)

    def compute_mask(self, inputs, mask=None):
        if callable(self.mask):
            return self.mask(inputs, mask)
        return self.mask


class GlobalAveragePooling1D(Layer):
    def __init__(self, data_format="channels_last", **kwargs):
        super().__init__(**kwargs)
        if data_format != "channels_last":
            raise NotImplementedError
        self.supports_masking = True

    def call(self, inputs, mask=None):
        if mask is not None:
            m = mask.to(inputs.dtype).unsqueeze(2)
            return wrap((inputs * m).sum(dim=1) / m.sum(dim=1))
        return wrap(inputs.mean(dim=1))

    def compute_mask(self, inputs, mask=None):
        return None
