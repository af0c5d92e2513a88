"""What `DeviceNormalizer`, `DeviceRolloutBuffer` and `DeviceReplayBuffer` share: one handle of the C ABI behind a family of entries
`fleet_<prefix>_*` (create, destroy, last_error, set_stream), its errors as exceptions, its stream, its end -- the Python side of
fleetrl_amd/csrc/fleet_handle.h -- and what `DevicePPOGrad`, `DeviceTD3Grad` and `DeviceAdam` share on top of it: a handle made ON
another handle's weight image (`_ImageBorrower`; fleetrl_amd/csrc/fleet_mlp.h `FleetMlpUser`)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi
from ._capi import FleetHipError


class _DeviceArray:
    """A view of device memory somebody else owns, for torch.as_tensor (the CUDA array interface)."""

    def __init__(self, ptr: int, shape: tuple, typestr: str, owner):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 2,
                                         "strides": None}
        self._owner = owner  # the tensor made from this object keeps it, and with it the buffer, alive


class _DeviceHandle:
    _prefix = ""  # "rollout": the entries are fleet_rollout_*
    _tensors = None  # the buffers' zero-copy views, made on first use

    def _entry(self, name: str):
        return getattr(self.lib, f"fleet_{self._prefix}_{name}")

    def _open(self, device: int, params, *more):
        """fleet_<prefix>_create on `device` with the family's parameter struct, and what the entry takes behind it (`more`)."""
        self.lib = _capi.load_library()
        self.device = int(device)
        h = C.c_void_p()
        rc = self._entry("create")(self.device, C.byref(params), *more, C.byref(h))
        if rc != _capi.OK:
            raise FleetHipError(rc, self._entry("last_error")(None).decode())
        self.h = h
        self._stream = None

    def _check(self, rc: int):
        if rc != _capi.OK:
            raise FleetHipError(rc, self._entry("last_error")(self.h).decode())

    def set_stream(self, hip_stream: int | None):
        self._check(self._entry("set_stream")(self.h, hip_stream))
        self._stream = hip_stream

    def use_torch_stream(self, device=None):
        """Launch on torch's current stream of `device` (default: the handle's own) from now on (no-op if already there)."""
        import torch

        cur = torch.cuda.current_stream(device if device is not None else self.device).cuda_stream
        if cur != self._stream:
            self.set_stream(cur)

    def _make_views(self, spec: dict) -> dict:
        """name -> zero-copy tensor over the address `arrays_dev()` gives for it; spec: name -> (shape, typestr)."""
        import torch

        dev = torch.device("cuda", self.device)
        ptrs = self.arrays_dev()
        return {n: torch.as_tensor(_DeviceArray(ptrs[n], shape, typestr, self), device=dev) for n, (shape, typestr) in spec.items()}

    def _tensor(self, t, shape, dtypes):
        import torch

        if isinstance(t, np.ndarray) or not isinstance(t, torch.Tensor):  # convenience, not the fast path
            t = torch.as_tensor(np.ascontiguousarray(t)).to(torch.device("cuda", self.device))
            if t.dtype not in dtypes:
                t = t.to(dtypes[0])
        if t.dtype == torch.bool and torch.uint8 in dtypes:
            t = t.view(torch.uint8)
        if t.device.type != "cuda" or t.device.index != self.device or t.dtype not in dtypes or t.numel() != int(np.prod(shape)) or \
                not t.is_contiguous():
            raise ValueError(f"expected a contiguous tensor of {int(np.prod(shape))} elements {shape}, dtype in {dtypes}, on "
                             f"cuda:{self.device}; got {tuple(t.shape)} {t.dtype} on {t.device}")
        return t

    def _per_action(self, key: str, v):
        """`v` as a device f32 [act_dim] tensor (handles with an `act_dim` and a `_constants` dict): a tensor is taken as it is, a
        float or an array is broadcast into a cached one.  A float that CHANGES between calls replaces the cached tensor through a
        host-to-device copy, which synchronises the host with the stream: a value that varies inside a loop (a decaying sigma, a
        learned log_std) belongs in a device tensor."""
        import torch

        if isinstance(v, torch.Tensor):
            return self._tensor(v.detach(), (self.act_dim,), (torch.float32,))
        host = np.broadcast_to(np.asarray(v, dtype=np.float32), (self.act_dim,))
        hit = self._constants.get(key)
        if hit is None or not np.array_equal(hit[0], host):
            hit = self._constants[key] = (host.copy(), torch.from_numpy(host.copy()).to(torch.device("cuda", self.device)))
        return hit[1]

    def close(self):
        if getattr(self, "h", None):
            self._tensors = None
            self._entry("destroy")(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown
            pass


class _ImageBorrower(_DeviceHandle):
    """A handle that works on the weight image of `owner` (a `DevicePolicy` or a `DeviceTD3Target`) and owns none: it lives on the
    owner's device, launches on the owner's stream, and the owner must outlive it (the object is kept)."""

    def _open_on(self, owner, create_entry: str, params):
        """`create_entry` (the C ABI's full name) on `owner`'s handle with the family's parameter struct."""
        self.lib = _capi.load_library()
        self._owner, self.device = owner, owner.device
        h = C.c_void_p()
        rc = getattr(self.lib, create_entry)(owner.h, C.byref(params), C.byref(h))
        if rc != _capi.OK:
            raise FleetHipError(rc, self._entry("last_error")(None).decode())
        self.h = h
        self._grad_cache = {}  # slot -> (the parameters, the pointer array of their .grad, the addresses) of the last call

    def set_stream(self, hip_stream):
        """The handle has no stream of its own: the owner's is set."""
        self._owner.set_stream(hip_stream)

    def use_torch_stream(self, device=None):
        self._owner.use_torch_stream(device)

    def _grad_pointers(self, slot, into, shapes, what: str):
        """The (c_void_p * n) array of the `.grad` addresses of the parameters `into`, which must have `shapes` (`what` names their
        order in the message); a `.grad` that is missing is allocated.  The array of the last call in `slot` is kept and returned
        again while the parameters are the same objects and their `.grad` lie where they lay."""
        import torch

        into = list(into)
        hit = self._grad_cache.get(slot)
        if hit is not None and len(hit[0]) == len(into) and all(a is b for a, b in zip(hit[0], into)) and \
                all(p.grad is not None and p.grad.data_ptr() == q for p, q in zip(into, hit[2])):
            return hit[1]
        if len(into) != len(shapes):
            raise ValueError(f"into: expected {len(shapes)} parameters (W, b per layer, {what}), got {len(into)}")
        ptrs = []
        for p, s in zip(into, shapes):
            if tuple(p.shape) != s:
                raise ValueError(f"into: expected a parameter of shape {s}, got {tuple(p.shape)}")
            if p.grad is None:  # allocated once; the launches overwrite it
                p.grad = torch.empty_like(p, memory_format=torch.contiguous_format)
            ptrs.append(self._tensor(p.grad, s, (torch.float32,)).data_ptr())
        arr = (C.c_void_p * len(ptrs))(*ptrs)
        self._grad_cache[slot] = (into, arr, ptrs)
        return arr
