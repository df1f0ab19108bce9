"""Run the reference's model code, unmodified, on the eager stand-in of oracle/tf_eager.

TEST INFRASTRUCTURE ONLY.  `reference()` registers the stand-in under the names `tensorflow`, `tensorflow.keras`, ... in
`sys.modules`, puts the reference root (EGT_REFERENCE_DIR, default /root/reference) on `sys.path`, imports the reference's
model modules from where they lie and yields them; on exit every `tensorflow*` and `lib*` entry is removed again and
`sys.path` is restored, so `import tensorflow` fails afterwards as it did before.  Nothing of the reference is copied: the
modules exist only while the context is open, on a machine that has the reference tree.

`load_weights` / `read_weights` / `weight_grads` address the weights of the reference's `tracked_layers` by their Keras names
(`<layer name>/<weight name>`, e.g. `dense_qkv_00/kernel`).
"""
from __future__ import annotations

import contextlib
import importlib
import os
import sys
import types

import torch

from . import tf_eager
from .tf_eager import _core

DEFAULT_DIR = "/root/reference"
MODEL_MODULES = {                     # name in the yielded namespace -> module of the reference
    "egt_layers": "lib.models.egt_layers",
    "xformer_base": "lib.models.graph_xformer_model_base",
    "graph_base": "lib.models.graph_model_base",
    "zinc": "lib.models.zinc.dc",
    "cifar10": "lib.models.cifar10.dc",
    "virtual_nodes": "lib.base.graph_layers.virtual_nodes",
    "masking": "lib.base.xformer_layers.masking",
    "loss_layers": "lib.base.genutil.loss_layers",
}


def reference_dir():
    return os.environ.get("EGT_REFERENCE_DIR", DEFAULT_DIR)


def available():
    return os.path.isfile(os.path.join(reference_dir(), "lib", "models", "egt_layers.py"))


def _stand_in_modules():
    k = tf_eager.keras
    mods = {"tensorflow": tf_eager, "tensorflow.keras": k, "tensorflow.nn": tf_eager.nn, "tensorflow.random": tf_eager.random,
            "tensorflow.math": tf_eager.math}
    for n in ("backend", "callbacks", "initializers", "layers", "losses", "metrics", "models", "regularizers"):
        mods[f"tensorflow.keras.{n}"] = getattr(k, n)
    # two private imports at the top of lib/base/graph_layers/virtual_nodes.py, unused by its code
    chain = {"tensorflow.python": {}, "tensorflow.python.ops": {}, "tensorflow.python.ops.gen_array_ops": {"shape": tf_eager.shape},
             "tensorflow.python.training": {}, "tensorflow.python.training.tracking": {},
             "tensorflow.python.training.tracking.base": {"no_automatic_dependency_tracking_scope": contextlib.nullcontext}}
    for name, members in chain.items():
        m = types.ModuleType(name)
        m.__path__ = []
        m.__dict__.update(members)
        mods[name] = m
    return mods


def _ours(name):
    return name == "tensorflow" or name.startswith("tensorflow.") or name == "lib" or name.startswith("lib.")


@contextlib.contextmanager
def reference():
    root = reference_dir()
    if not available():
        raise FileNotFoundError(f"no reference tree at {root} (EGT_REFERENCE_DIR)")
    clash = [n for n in sys.modules if _ours(n)]
    if clash:
        raise RuntimeError(f"modules already imported under the names the reference needs: {clash[:4]}")
    saved_path = list(sys.path)
    saved_bytecode = sys.dont_write_bytecode
    sys.dont_write_bytecode = True                 # the reference tree is read, never written
    try:
        sys.modules.update(_stand_in_modules())
        sys.path.insert(0, root)
        importlib.invalidate_caches()
        yield types.SimpleNamespace(tf=tf_eager, **{k: importlib.import_module(v) for k, v in MODEL_MODULES.items()})
    finally:
        for n in [n for n in sys.modules if _ours(n)]:
            del sys.modules[n]
        sys.path[:] = saved_path
        sys.dont_write_bytecode = saved_bytecode
        importlib.invalidate_caches()


session = _core.session
wrap = _core.wrap


def masked(t, mask):
    """the tensor as the stand-in's type, carrying `mask` as its Keras mask"""
    t = wrap(t)
    t._keras_mask = None if mask is None else wrap(mask)
    return t


# ---------------------------------------------------------------------------------------------- weights -----
def _layers(tracked):
    return tracked.get_layers_dict() if hasattr(tracked, "get_layers_dict") else dict(tracked)


def named_weights(tracked, trainable_only=True):
    """{`layer/weight`: tensor} of every built layer, in creation order"""
    out = {}
    for lname, layer in _layers(tracked).items():
        for wname, w in getattr(layer, "_weights", {}).items():
            if layer._trainable[wname] or not trainable_only:
                out[f"{lname}/{wname}"] = w
    return out


def load_weights(tracked, values):
    """copy `values` ({`layer/weight`: array}) into the weights; the two key sets must be equal"""
    ws = named_weights(tracked)
    if set(ws) != set(values):
        raise KeyError(f"weights not given: {sorted(set(ws) - set(values))}; not in the model: {sorted(set(values) - set(ws))}")
    with torch.no_grad():
        for k, w in ws.items():
            v = torch.as_tensor(values[k]).to(w.dtype)
            if tuple(v.shape) != tuple(w.size()):
                raise ValueError(f"{k}: model {tuple(w.size())}, given {tuple(v.shape)}")
            w.copy_(v)


def read_weights(tracked):
    return {k: w.detach().as_subclass(torch.Tensor).clone() for k, w in named_weights(tracked).items()}


def weight_grads(tracked, loss):
    """{`layer/weight`: d loss / d weight}; a weight the loss does not depend on (a layer Keras would leave out of the
    functional model) gets zeros"""
    ws = named_weights(tracked)
    gs = torch.autograd.grad(loss, list(ws.values()), allow_unused=True)
    return {k: (torch.zeros_like(w) if g is None else g).detach().as_subclass(torch.Tensor) for (k, w), g in zip(ws.items(), gs)}


def added_losses(tracked):
    """sum of what the layers passed to add_loss (None when there is none)"""
    terms = [v for layer in _layers(tracked).values() for v in getattr(layer, "losses", [])]
    return sum(terms[1:], terms[0]) if terms else None
