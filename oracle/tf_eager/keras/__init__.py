"""`tensorflow.keras` of the eager stand-in (see oracle/tf_eager/__init__.py)."""
from . import backend, callbacks, initializers, layers, losses, metrics, models, regularizers  # noqa: F401
