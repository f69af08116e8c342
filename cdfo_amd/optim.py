"""Adam on the device (csrc/adam.hip; DESIGN.md "Adam on the device"): `DeviceAdam` keeps the moments of all parameters in one fp32
buffer each, the step count and the step's scalars on the device, and makes a step in three launches without a host read: the
gradient's norm (fp64 partials per chunk), the scalars (norm, clip coefficient, skip flag, bias corrections), the update.  A
non-finite gradient skips the step: parameters and moments keep their bits, ``skipped`` counts it.  The statement of the update is
``torch.optim.Adam``'s single-tensor one (L2 weight decay, no amsgrad); its state loads here and this state loads there."""
from __future__ import annotations

import math
from typing import Iterable, List, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import _vp, check

CHUNK = 4096                          # CDFO_ADAM_CHUNK: elements of one workgroup
STAGES = 4                            # pinned copies of the table in flight before one is reused


def chunk_table(sizes: Sequence[int], chunk: int = CHUNK) -> Tuple[np.ndarray, np.ndarray, int]:
    """(offsets int64 [T], chunks int32 [C, 2], total) of tensors of ``sizes`` elements: tensor t owns ``[offsets[t], offsets[t] +
    sizes[t])`` of the moment buffers, every offset a multiple of 4 and ``total`` the buffers' length; ``chunks`` lists (tensor,
    first element) of every run of at most ``chunk`` elements, each element of each tensor in exactly one.  A function of the sizes."""
    if isinstance(chunk, bool) or not isinstance(chunk, (int, np.integer)) or chunk <= 0 or chunk % 4:
        raise ValueError(f"chunk_table: chunk must be a positive multiple of 4, got {chunk!r}")
    offsets, rows, total = [], [], 0
    for t, n in enumerate(sizes):
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n <= 0 or n >= 2 ** 31:
            raise ValueError(f"chunk_table: size {t} must be an integer from 1 to 2^31 - 1, got {n!r}")
        offsets.append(total)
        rows.extend((t, first) for first in range(0, int(n), chunk))
        total += (int(n) + 3) // 4 * 4
    if not offsets:
        raise ValueError("chunk_table: no tensors")
    return np.asarray(offsets, np.int64), np.asarray(rows, np.int32).reshape(-1, 2), total


def _check_max_norm(max_grad_norm, who: str):
    if max_grad_norm is None:
        return None
    if isinstance(max_grad_norm, bool) or not isinstance(max_grad_norm, (int, float)) or not math.isfinite(max_grad_norm) or max_grad_norm <= 0:
        raise ValueError(f"{who}: max_grad_norm must be a finite positive number or None, got {max_grad_norm!r}")
    return float(max_grad_norm)


def adam_moments(state: dict, count: int, indices=None):
    """(step, skipped, exp_avg list, exp_avg_sq list, hyper-parameters or None) of a `DeviceAdam.state_dict()` or a
    ``torch.optim.Adam.state_dict()`` over ``count`` parameters; a torch state without moments yet is step 0 with ``None`` lists.
    ``indices``: the ``count`` parameters of a torch state that the moments are wanted of (torch keeps none for a parameter that
    never had a gradient); default all of its parameters."""
    if "param_groups" in state and "state" in state:                      # torch.optim.Adam
        groups = state["param_groups"]
        if len(groups) != 1:
            raise ValueError(f"load_state_dict: one parameter group expected, got {len(groups)}")
        g = groups[0]
        if g.get("amsgrad") or g.get("maximize") or g.get("decoupled_weight_decay"):
            raise ValueError("load_state_dict: amsgrad, maximize and decoupled weight decay are not supported")
        if indices is None:
            indices = list(range(len(g["params"])))
        if len(indices) != count:
            raise ValueError(f"load_state_dict: the state has {len(indices)} parameters, the optimizer {count}")
        hyper = dict(lr=float(g["lr"]), betas=tuple(float(b) for b in g["betas"]), eps=float(g["eps"]), weight_decay=float(g["weight_decay"]))
        per = state["state"]
        if not per:
            return 0, 0, None, None, hyper
        if not set(indices) <= set(per):
            raise ValueError("load_state_dict: the state holds moments for some parameters only")
        steps = {int(float(per[i]["step"])) for i in indices}
        if len(steps) != 1:
            raise ValueError(f"load_state_dict: the parameters' step counts differ: {sorted(steps)}")
        return steps.pop(), 0, [per[i]["exp_avg"] for i in indices], [per[i]["exp_avg_sq"] for i in indices], hyper
    for key in ("step", "skipped", "exp_avg", "exp_avg_sq"):
        if key not in state:
            raise ValueError(f"load_state_dict: not an Adam state: no {key!r}")
    if len(state["exp_avg"]) != count or len(state["exp_avg_sq"]) != count:
        raise ValueError(f"load_state_dict: the state has {len(state['exp_avg'])} parameters, the optimizer {count}")
    hyper = None
    if "lr" in state:
        hyper = dict(lr=float(state["lr"]), betas=tuple(float(b) for b in state["betas"]), eps=float(state["eps"]),
                     weight_decay=float(state["weight_decay"]))
    return int(state["step"]), int(state["skipped"]), list(state["exp_avg"]), list(state["exp_avg_sq"]), hyper


def load_into_torch_adam(optimizer: torch.optim.Adam, state: dict, params=None) -> None:
    """Continue a ``torch.optim.Adam`` (one group, moments not yet made or made) from a `DeviceAdam.state_dict()`; a torch state dict
    goes to ``optimizer.load_state_dict``.  ``params``: the optimizer's parameters that the state's moments belong to, in the state's
    order (default all of them).  ``skipped`` has no place there and is dropped."""
    if "param_groups" in state:
        optimizer.load_state_dict(state)
        return
    if params is None:
        params = [p for g in optimizer.param_groups for p in g["params"]]
    step, _, m, v, _ = adam_moments(state, len(params))
    for i, p in enumerate(params):
        if tuple(m[i].shape) != tuple(p.shape) or tuple(v[i].shape) != tuple(p.shape):
            raise ValueError(f"load_state_dict: parameter {i} has shape {tuple(p.shape)}, its moments {tuple(m[i].shape)}")
        optimizer.state[p] = {"step": torch.tensor(float(step), dtype=torch.float32),
                              "exp_avg": m[i].detach().to(device=p.device, dtype=p.dtype, copy=True).contiguous(),
                              "exp_avg_sq": v[i].detach().to(device=p.device, dtype=p.dtype, copy=True).contiguous()}


class DeviceAdam:
    """Adam over ``params`` (contiguous fp32 tensors of one device, or ``(name, tensor)`` pairs as ``named_parameters()`` gives: the
    errors then name the parameter) with the update, the gradient norm, the optional clip to
    ``max_grad_norm`` (``clip_grad_norm_``'s coefficient) and the step count on the device.  ``step()`` reads nothing back;
    ``grad_norm`` is the last step's norm before clipping (a device fp64 scalar, a view: clone it to keep it), ``steps`` and
    ``skipped`` read the device.  ``lr`` may be set between steps."""

    def __init__(self, params: Iterable[torch.Tensor], lr: float = 1e-4, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, max_grad_norm=None):
        given = list(params)
        named = bool(given) and all(isinstance(e, tuple) and len(e) == 2 and isinstance(e[0], str) for e in given)
        self.named = named
        self.params: List[torch.Tensor] = [e[1] for e in given] if named else given
        self.names: List[str] = [e[0] for e in given] if named else ["parameter %d" % i for i in range(len(given))]
        if not self.params:
            raise ValueError("DeviceAdam: no parameters")
        for i, p in enumerate(self.params):
            if not isinstance(p, torch.Tensor) or not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous() or p.numel() == 0:
                raise ValueError(f"DeviceAdam: {self.names[i]} is not a non-empty contiguous fp32 device tensor")
            if p.device != self.params[0].device:
                raise ValueError(f"DeviceAdam: {self.names[i]} is on {p.device}, {self.names[0]} on {self.params[0].device}")
        if not (isinstance(lr, (int, float)) and math.isfinite(lr) and lr >= 0):
            raise ValueError(f"DeviceAdam: lr must be a finite number >= 0, got {lr!r}")
        if len(betas) != 2 or not all(isinstance(b, (int, float)) and 0.0 <= b < 1.0 for b in betas):
            raise ValueError(f"DeviceAdam: betas must be two numbers in [0, 1), got {betas!r}")
        if not (isinstance(eps, (int, float)) and math.isfinite(eps) and eps >= 0):
            raise ValueError(f"DeviceAdam: eps must be a finite number >= 0, got {eps!r}")
        if not (isinstance(weight_decay, (int, float)) and math.isfinite(weight_decay) and weight_decay >= 0):
            raise ValueError(f"DeviceAdam: weight_decay must be a finite number >= 0, got {weight_decay!r}")
        self.lr, self.betas, self.eps, self.weight_decay = float(lr), (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)
        self.max_grad_norm = _check_max_norm(max_grad_norm, "DeviceAdam")
        self.device = dev = self.params[0].device
        self.sizes = [p.numel() for p in self.params]
        self.offsets, chunks, self.total = chunk_table(self.sizes)
        with torch.cuda.device(dev):
            self._m = torch.zeros(self.total, dtype=torch.float32, device=dev)
            self._v = torch.zeros(self.total, dtype=torch.float32, device=dev)
            self._counters = torch.zeros(2, dtype=torch.int64, device=dev)            # step, skipped
            self._scalars = torch.zeros(6, dtype=torch.float64, device=dev)           # cdfo_adam_scalars
            self._chunks = torch.from_numpy(chunks).to(dev)                           # depends on the sizes alone: uploaded once
            self._partials = torch.zeros(len(chunks), dtype=torch.float64, device=dev)
            self._table = torch.zeros((len(self.params), 4), dtype=torch.int64, device=dev)
        # The gradients are reallocated every step, so the table is refreshed every step: written to a pinned copy, uploaded on the
        # stream.  A pinned copy is rewritten only after the event behind its last upload has passed (STAGES steps later).
        self._stage = [torch.zeros((len(self.params), 4), dtype=torch.int64).pin_memory() for _ in range(STAGES)]
        self._stage_np = [s.numpy() for s in self._stage]
        self._events = [None] * STAGES
        self._turn, self._last, self._uploaded = 0, None, None
        fixed = np.stack([np.asarray([p.data_ptr() for p in self.params], np.int64), np.zeros(len(self.params), np.int64), self.offsets,
                          np.asarray(self.sizes, np.int64)], axis=1)
        for s in self._stage_np:
            s[:] = fixed

    # -- the step ------------------------------------------------------------------------------------------------------------
    def _gradients(self) -> List[int]:
        ptrs = []
        for i, p in enumerate(self.params):
            g = p.grad
            if g is None:
                raise ValueError(f"DeviceAdam.step: {self.names[i]} {tuple(p.shape)} has no gradient")
            if g.dtype != torch.float32 or not g.is_contiguous() or g.device != self.device or g.shape != p.shape:
                raise ValueError(f"DeviceAdam.step: the gradient of {self.names[i]} {tuple(p.shape)} is not a contiguous fp32 tensor of "
                                 f"its shape on {self.device} ({g.dtype}, {tuple(g.shape)}, {g.device})")
            ptrs.append(g.data_ptr())
        return ptrs

    def _refresh(self, ptrs: List[int]) -> int:
        """Bring the device table to the step's pointers; returns the pinned copy that equals it."""
        mine = [p.data_ptr() for p in self.params]
        if self._uploaded == (mine, ptrs):
            return self._last
        k = self._turn
        self._turn = (k + 1) % STAGES
        if self._events[k] is not None and not self._events[k].query():
            self._events[k].synchronize()                                            # STAGES uploads behind: passed long ago
        self._stage_np[k][:, 0] = mine
        self._stage_np[k][:, 1] = ptrs
        self._table.copy_(self._stage[k], non_blocking=True)
        if self._events[k] is None:
            self._events[k] = torch.cuda.Event()
        self._events[k].record()
        self._last, self._uploaded = k, (mine, ptrs)
        return k

    @torch.no_grad()
    def step(self) -> None:
        ptrs = self._gradients()                                                     # every ValueError comes before any launch
        lib = _lib.lib()
        T, C = len(self.params), self._chunks.shape[0]
        with torch.cuda.device(self.device):
            host = self._stage[self._refresh(ptrs)].data_ptr()
            stream = torch.cuda.current_stream().cuda_stream
            check(lib.cdfo_grad_norm_partials(host, _vp(self._table), T, _vp(self._chunks), C, _vp(self._partials), stream),
                  "cdfo_grad_norm_partials")
            check(lib.cdfo_adam_scalars(_vp(self._partials), C, self.lr, self.betas[0], self.betas[1], self.max_grad_norm or 0.0,
                                        _vp(self._counters), _vp(self._scalars), stream), "cdfo_adam_scalars")
            check(lib.cdfo_adam_step(host, _vp(self._table), T, _vp(self._chunks), C, _vp(self._m), _vp(self._v), self.total,
                                     _vp(self._scalars), self.betas[0], self.betas[1], self.eps, self.weight_decay, stream), "cdfo_adam_step")
        # the update went through raw pointers: whatever keys a cache on (data_ptr, _version) must see the write
        torch.autograd.graph.increment_version(self.params)

    def zero_grad(self, set_to_none: bool = True) -> None:
        for p in self.params:
            if p.grad is None:
                continue
            if set_to_none:
                p.grad = None
            else:
                p.grad.detach_()
                p.grad.zero_()

    # -- what the device holds -----------------------------------------------------------------------------------------------
    @property
    def grad_norm(self) -> torch.Tensor:
        return self._scalars[0]

    @property
    def norm_sum(self) -> torch.Tensor:
        """The sum of ``grad_norm`` over the unskipped steps of this object (a device fp64 scalar; not part of the state)."""
        return self._scalars[5]

    @property
    def counters(self) -> torch.Tensor:
        """(step, skipped) on the device, int64."""
        return self._counters

    @property
    def steps(self) -> int:
        return int(self._counters[0])

    @property
    def skipped(self) -> int:
        return int(self._counters[1])

    def _moments(self, buf: torch.Tensor) -> List[torch.Tensor]:
        return [buf[o:o + n].view(p.shape) for o, n, p in zip(self.offsets.tolist(), self.sizes, self.params)]

    def state_dict(self) -> dict:
        step, skipped = self._counters.tolist()
        return {"step": step, "skipped": skipped, "names": list(self.names) if self.named else None, "lr": self.lr,
                "betas": self.betas, "eps": self.eps, "weight_decay": self.weight_decay, "max_grad_norm": self.max_grad_norm, "exp_avg": [t.clone() for t in self._moments(self._m)],
                "exp_avg_sq": [t.clone() for t in self._moments(self._v)]}

    @torch.no_grad()
    def load_state_dict(self, state: dict) -> None:
        """Take the step count, the moments and the hyper-parameters of a `state_dict()` of this class or of ``torch.optim.Adam``
        (one group, no amsgrad).  ``max_grad_norm`` comes with a state of this class and stays as it is with torch's."""
        step, skipped, m, v, hyper = adam_moments(state, len(self.params))
        if self.named and state.get("names") is not None and list(state["names"]) != self.names:
            other = next((a for a, b in zip(state["names"], self.names) if a != b), None)
            raise ValueError(f"load_state_dict: the state's parameters are not this optimizer's (the state has {other!r})")
        if step < 0 or skipped < 0:
            raise ValueError(f"load_state_dict: negative step count ({step}, {skipped})")
        for i, p in enumerate(self.params):
            for t in (() if m is None else (m[i], v[i])):
                if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(p.shape):
                    raise ValueError(f"load_state_dict: the moments of parameter {i} do not have its shape {tuple(p.shape)}")
        if "max_grad_norm" in state:
            self.max_grad_norm = _check_max_norm(state["max_grad_norm"], "load_state_dict")
        if hyper is not None:
            self.lr, self.betas, self.eps, self.weight_decay = hyper["lr"], hyper["betas"], hyper["eps"], hyper["weight_decay"]
        with torch.cuda.device(self.device):
            if m is None:
                self._m.zero_()
                self._v.zero_()
            else:
                for dst, src in zip(self._moments(self._m) + self._moments(self._v), list(m) + list(v)):
                    dst.copy_(src.to(torch.float32))
            self._counters.copy_(torch.tensor([step, skipped], dtype=torch.int64))
