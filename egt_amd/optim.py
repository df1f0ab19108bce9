"""The parameter update of a training step as two launches: ``FlatOptimizer`` (Adam / RMSprop / SGD with torch.optim's
arithmetic) on the library's ``egt_optim_prepare`` / ``egt_optim_step`` (include/egt_amd.h, csrc/egt_optim.hip).

The gradients are the flat buffer of a ``FlatGradAllReduce`` (egt_amd.dp: running sum of numel(), no padding); the moments
are flat buffers of the same layout owned by the optimizer; the parameters stay where they are and reach the kernel through
a device-resident table of work items that ``plan_items`` cuts so that no item straddles a parameter.

Checkpoints: ``state_dict()`` / ``load_state_dict()`` speak the layout of the corresponding torch.optim class
(``flat_to_state`` / ``state_to_flat`` below are the two conversions, on plain tensors), so a run saved with
torch.optim.Adam resumes with FlatOptimizer and the other way round.
"""
from __future__ import annotations

import ctypes as C
import struct
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

ALGOS = ("adam", "rmsprop", "sgd")
ITEM = 2048          # elements per work item: 256 threads x two dwordx4; a 500 k-float model is ~250 full items + the short ones
_MOMENT_KEYS = {"adam": ("exp_avg", "exp_avg_sq"), "rmsprop": (None, "square_avg"), "sgd": (None, None)}


def plan_items(numels: Sequence[int], item: int = ITEM) -> List[Tuple[int, int, int, int]]:
    """Work items [(parameter index, first element in the parameter, flat offset, count)] over parameters of `numels`
    elements laid out back to back: every element exactly once, in flat order, no item across two parameters, count in
    [1, item].  A parameter without elements gets no item."""
    if item < 1:
        raise ValueError("item must be >= 1")
    out, off = [], 0
    for i, n in enumerate(numels):
        n = int(n)
        if n < 0:
            raise ValueError(f"parameter {i} has a negative element count")
        for s in range(0, n, item):
            out.append((i, s, off + s, min(item, n - s)))
        off += n
    return out


def _numel(shape) -> int:
    n = 1
    for s in shape:
        n *= int(s)
    return n


def flat_to_state(algo: str, shapes: Sequence[Sequence[int]], step: int, m: torch.Tensor = None, v: torch.Tensor = None) -> Dict[int, dict]:
    """The ``state`` entry of the torch.optim class's ``state_dict()`` from the flat moments: per parameter index
    ``step`` (a float32 scalar, as torch keeps it) and ``exp_avg`` / ``exp_avg_sq`` (Adam) or ``square_avg`` (RMSprop) as
    copies in the parameter's shape.  Empty before the first step and for SGD without momentum, as torch's is."""
    mk, vk = _MOMENT_KEYS[algo]
    if vk is None or int(step) == 0:
        return {}
    out, off = {}, 0
    for i, shp in enumerate(shapes):
        n = _numel(shp)
        d = {"step": torch.tensor(float(step), dtype=torch.float32)}
        if mk is not None:
            d[mk] = m[off:off + n].clone().view(*shp)
        d[vk] = v[off:off + n].clone().view(*shp)
        out[i] = d
        off += n
    return out


def state_to_flat(algo: str, state: Dict[int, dict], shapes: Sequence[Sequence[int]], m: torch.Tensor = None, v: torch.Tensor = None) -> int:
    """The inverse: fills the flat moments `m` / `v` (where the algorithm has them) from a torch.optim ``state`` and returns
    the step count.  An empty state is a fresh run (zeros, step 0).  Refused with ValueError: per-parameter steps that
    differ (the flat optimizer has ONE counter), a state that covers only some parameters, shapes that do not match, and
    entries this optimizer does not keep (amsgrad's max_exp_avg_sq, a momentum buffer, a centered average)."""
    mk, vk = _MOMENT_KEYS[algo]
    keys = {k for k in (mk, vk) if k is not None}
    if vk is None:
        for i, d in state.items():
            if d:
                raise ValueError(f"sgd: parameter {i} carries optimizer state {sorted(d)} (momentum is not supported)")
        return 0
    if not state:
        for flat in (m, v):
            if flat is not None:
                flat.zero_()
        return 0
    state = {int(i): d for i, d in state.items()}
    if sorted(state) != list(range(len(shapes))):
        raise ValueError(f"{algo}: the state covers parameters {sorted(state)[:8]}... of {len(shapes)}: all or none")
    steps = {float(d["step"]) for d in state.values()}
    if len(steps) != 1:
        raise ValueError(f"{algo}: per-parameter step counts differ ({sorted(steps)[:4]}...): the flat optimizer has one counter")
    step = steps.pop()
    if step != int(step) or step < 0:
        raise ValueError(f"{algo}: step {step} is not a step count")
    off = 0
    for i, shp in enumerate(shapes):
        d, n = state[i], _numel(shp)
        extra = set(d) - keys - {"step"}
        if extra or not keys <= set(d):
            raise ValueError(f"{algo}: parameter {i} has state {sorted(d)}; expected {sorted(keys | {'step'})}")
        for k, flat in ((mk, m), (vk, v)):
            if k is None:
                continue
            if tuple(d[k].shape) != tuple(int(s) for s in shp):
                raise ValueError(f"{algo}: {k} of parameter {i} has shape {tuple(d[k].shape)}, the parameter {tuple(shp)}")
            flat[off:off + n].copy_(d[k].detach().reshape(-1).to(device=flat.device, dtype=flat.dtype))
        off += n
    return int(step)


def _torch_defaults(algo: str, lr: float, betas, alpha: float, eps: float) -> dict:
    """param_groups keys of the corresponding torch.optim class, from the class itself"""
    dummy = [torch.zeros(1)]
    if algo == "adam":
        return dict(torch.optim.Adam(dummy, lr=lr, betas=tuple(betas), eps=eps).defaults)
    if algo == "rmsprop":
        return dict(torch.optim.RMSprop(dummy, lr=lr, alpha=alpha, eps=eps).defaults)
    return dict(torch.optim.SGD(dummy, lr=lr).defaults)


_UNSUPPORTED = dict(weight_decay=0, amsgrad=False, maximize=False, momentum=0, centered=False, nesterov=False, dampening=0,
                    decoupled_weight_decay=False)


class FlatOptimizer(torch.optim.Optimizer):
    """``step()`` = egt_optim_prepare + egt_optim_step on the current stream: two launches, no synchronisation, capturable.

    params      fp32, contiguous, on a GPU; the list `flat_grads` was built over, in its order
    flat_grads  a FlatGradAllReduce: its buffer is the gradient input
    clip_value  elementwise clamp of the gradient before use (Keras clipvalue; what clip_grad_value_ does)
    zero_grad   every gradient element is set to 0 once the step has read it
    ``param_groups[0]["lr"]`` is the learning rate, as with torch.optim: a changed value reaches the device with the next
    ``step()`` (or ``push_lr()``, in front of the replay of a captured step) as a 16-byte asynchronous copy."""

    def __init__(self, params, flat_grads, algo: str = "adam", lr: float = 1e-3, clip_value=None, zero_grad: bool = False,
                 betas=(0.9, 0.999), alpha: float = 0.9, eps: float = 1e-7):
        if algo not in ALGOS:
            raise ValueError(f"FlatOptimizer: algo must be one of {ALGOS} (got {algo!r})")
        params = list(params)
        if not params:
            raise ValueError("FlatOptimizer: no parameters")
        if len(params) != len(flat_grads.params) or any(a is not b for a, b in zip(params, flat_grads.params)):
            raise ValueError("FlatOptimizer: params must be the parameter list of flat_grads, in its order")
        for i, p in enumerate(params):
            self._check_param(i, p, None)
        if clip_value is not None and not float(clip_value) > 0:
            raise ValueError(f"FlatOptimizer: clip_value must be > 0 (got {clip_value})")
        self.algo, self.flat_grads = algo, flat_grads
        self.clip_value, self.zero_grad_in_step = (None if clip_value is None else float(clip_value)), bool(zero_grad)
        self.grad_scale = 1.0
        super().__init__(params, _torch_defaults(algo, float(lr), betas, alpha, eps))
        from . import _lib
        self._L, self._lib = _lib, _lib.load()
        flat = flat_grads.flat
        if flat.dtype != torch.float32 or not flat.is_cuda or flat.numel() != sum(p.numel() for p in params):
            raise ValueError("FlatOptimizer: flat_grads.flat must be an fp32 GPU buffer of sum(numel) elements")
        self._params = params
        self._shapes = [tuple(p.shape) for p in params]
        self._numels = [p.numel() for p in params]
        self._m = torch.zeros_like(flat) if algo == "adam" else None
        self._v = torch.zeros_like(flat) if algo != "sgd" else None
        self._state = torch.zeros(_lib.OPTIM_STATE_BYTES, dtype=torch.uint8, device=flat.device)
        self._slots, self._pushed = [], None
        self._ptrs, self._table, self._items = None, None, 0
        self._bind()
        self.push_lr()

    # ---- construction / binding ----
    @staticmethod
    def _check_param(i, p, numel):
        why = None
        if not p.is_cuda:
            why = f"is on {p.device}: FlatOptimizer needs the parameters on a GPU (device='cuda')"
        elif p.dtype != torch.float32:
            why = f"is {p.dtype}: fp32 only"
        elif not p.is_contiguous():
            why = "is not contiguous"
        elif numel is not None and p.numel() != numel:
            why = f"changed its element count ({numel} -> {p.numel()})"
        if why:
            raise ValueError(f"FlatOptimizer: parameter {i} {why}")

    def _bind(self):
        """(re)build the device table from where the parameters live now"""
        for i, (p, n) in enumerate(zip(self._params, self._numels)):
            self._check_param(i, p, n)
        ptrs = [p.data_ptr() for p in self._params]
        items = plan_items(self._numels)
        host = np.empty((len(items), 3), dtype=np.int64)
        for k, (i, s, off, cnt) in enumerate(items):
            host[k] = (ptrs[i] + 4 * s, off, cnt)
        assert host.dtype.itemsize * 3 == C.sizeof(self._L.OptimSegment)
        self._table = torch.from_numpy(host).to(self.flat_grads.flat.device)
        self._ptrs, self._items = ptrs, len(items)

    def pointers_current(self) -> bool:
        """every parameter still lives where the table says (the check `step()` runs before it launches)"""
        ptrs = self._ptrs
        for i, p in enumerate(self._params):
            if p.data_ptr() != ptrs[i]:
                return False
        return True

    # ---- the few bytes the host owns in the state block ----
    def push_lr(self):
        """copy (lr, grad_scale) to the device state if they changed since the last copy: asynchronous, from a pinned slot
        that is not reused before its copy has run"""
        cur = (float(self.param_groups[0]["lr"]), float(self.grad_scale))
        if cur == self._pushed:
            return
        capturing = torch.cuda.is_current_stream_capturing()
        slot = None
        if not capturing:
            for s in self._slots:
                if s[1] is not None and s[1].query():
                    slot = s
                    break
        if slot is None:
            slot = [torch.empty(16, dtype=torch.uint8).pin_memory(), None if capturing else torch.cuda.Event()]
            self._slots.append(slot)
        slot[0].copy_(torch.frombuffer(bytearray(struct.pack("<dfi", cur[0], cur[1], 0)), dtype=torch.uint8))
        self._state[8:24].copy_(slot[0], non_blocking=True)
        if slot[1] is not None:
            slot[1].record()
        self._pushed = cur

    def set_lr(self, lr: float):
        """param_groups' lr and the device copy at once: what a captured step needs in front of its replay"""
        for g in self.param_groups:
            g["lr"] = float(lr)
        self.push_lr()

    def _desc(self):
        g = self.param_groups[0]
        L = self._L
        b1, b2 = g["betas"] if self.algo == "adam" else (0.0, g.get("alpha", 0.0))
        flags = (L.OPT_CLIP if self.clip_value is not None else 0) | (L.OPT_ZERO_GRAD if self.zero_grad_in_step else 0)
        return L.OptimDesc(algo=ALGOS.index(self.algo), flags=flags, num_segments=self._items, reserved=0,
                           total=self.flat_grads.flat.numel(), beta1=float(b1), beta2=float(b2), eps=float(g.get("eps", 0.0)),
                           clip_value=self.clip_value or 0.0)

    @torch.no_grad()
    def step(self, closure=None):
        if closure is not None:
            raise ValueError("FlatOptimizer.step takes no closure")
        if not self.pointers_current():        # a parameter was moved (p.data = ...): never write through the old address
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("FlatOptimizer: a parameter moved; the table cannot be rebuilt while a graph is captured")
            self._bind()
        self.push_lr()
        L, lib = self._L, self._lib
        d, st = C.byref(self._desc()), L.current_stream()
        L.check(lib.egt_optim_prepare(d, L.ptr(self._state), st))
        L.check(lib.egt_optim_step(d, L.ptr(self._table), L.ptr(self.flat_grads.flat), L.ptr(self._m), L.ptr(self._v),
                                   L.ptr(self._state), st))
        return None

    def zero_grad(self, set_to_none: bool = False):
        """the gradients are views of the flat buffer: zero it in place (set_to_none would cut the aliasing)"""
        self.flat_grads.zero()
        self.flat_grads.rebind()

    # ---- checkpoints in torch.optim's layout ----
    def step_count(self) -> int:
        return int(self._state[:8].view(torch.int64).item())

    def state_dict(self):
        groups = [dict({k: v for k, v in g.items() if k != "params"}, params=list(range(len(self._params))))
                  for g in self.param_groups]
        return {"state": flat_to_state(self.algo, self._shapes, self.step_count(), self._m, self._v), "param_groups": groups}

    def load_state_dict(self, state_dict):
        groups = state_dict["param_groups"]
        if len(groups) != 1 or len(groups[0]["params"]) != len(self._params):
            raise ValueError("FlatOptimizer: the checkpoint must hold one parameter group over the same parameters")
        g = groups[0]
        for k, off in _UNSUPPORTED.items():
            if k in g and g[k] != off:
                raise ValueError(f"FlatOptimizer: the checkpoint was written with {k}={g[k]!r}, which the fused update does not do")
        step = state_to_flat(self.algo, state_dict["state"], self._shapes, self._m, self._v)
        self.param_groups[0].update({k: v for k, v in g.items() if k != "params" and k in self.param_groups[0]})
        self._state[:8].copy_(torch.tensor([step], dtype=torch.int64).view(torch.uint8))
        self.push_lr()
