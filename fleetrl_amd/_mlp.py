"""What `DevicePolicy` and `DeviceTD3Target` share: a handle whose device block is the weight image of a few MLPs (the Python side of
fleetrl_amd/csrc/fleet_mlp.h) -- filling the C ABI's `FleetPolicyHead`s from [(W, b), ...] lists, the packed host weights, creation with
them, and torch's parameter tensors as the pointer array of the `*_load_dev` / `*_polyak_dev` / `*_export_dev` entries."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi
from ._handle import _DeviceHandle

_ACTIVATIONS = {"tanh": _capi.POLICY_ACT_TANH, "relu": _capi.POLICY_ACT_RELU}
_OUTPUTS = {"none": _capi.POLICY_OUT_NONE, "clip": _capi.POLICY_OUT_CLIP, "tanh": _capi.POLICY_OUT_TANH}


def _array(t) -> np.ndarray:
    if hasattr(t, "detach"):
        t = t.detach().cpu().numpy()
    return np.ascontiguousarray(t, dtype=np.float32)


def _arrays(layers) -> list:
    return [(_array(w), _array(b)) for w, b in layers]


class _MlpHandle(_DeviceHandle):
    def _set_transforms(self, activation: str, output: str):
        if activation not in _ACTIVATIONS:
            raise ValueError(f"activation must be one of {sorted(_ACTIVATIONS)}, got {activation!r}")
        if output not in _OUTPUTS:
            raise ValueError(f"output must be one of {sorted(_OUTPUTS)}, got {output!r}")
        self.activation, self.output = activation, output

    def _fill_head(self, P, who: str, net, inp: int, output: str = "none", low: float = 0.0, high: float = 0.0):
        """`net` [(W [out, in], b [out]), ...] over `inp` columns into the FleetPolicyHead P; only an actor has an output transform."""
        for l, (w, b) in enumerate(net):
            if w.ndim != 2 or b.shape != (w.shape[0],) or w.shape[1] != inp:
                raise ValueError(f"{who}, layer {l}: expected W [out, {inp}] and b [out], got {w.shape} and {b.shape}")
            inp = w.shape[0]
        P.n_layers = len(net)  # (more than the ABI's 4: refused by the library, with its reason)
        for l, (w, _) in enumerate(net[:_capi.POLICY_MAX_LAYERS]):
            P.width[l] = w.shape[0]
        P.activation, P.output = _ACTIVATIONS[self.activation], _OUTPUTS[output]
        P.lo, P.hi = float(low), float(high)

    @staticmethod
    def _pack(nets) -> np.ndarray:
        return np.ascontiguousarray(np.concatenate([a.ravel() for net in nets for w, b in net for a in (w, b)]), dtype=np.float32)

    def _create(self, device: int, params, nets):
        self._shapes = [(w.shape, b.shape) for net in nets for w, b in net]
        packed = self._pack(nets)  # (alive across the call: the entry reads it through its address)
        self._open(device, params, packed.ctypes.data)
        self._constants = {}  # _per_action's device tensors of float arguments
        self.tile_rows = self.describe()["tile_rows"]

    def _pointers(self, what: str, parameters):
        """torch's tensors (W, b per layer, net after net), checked against the handle's shapes, as the entries' pointer array."""
        import torch

        self.use_torch_stream()
        params = [p.detach() for p in parameters]
        flat = [s for pair in self._shapes for s in pair]
        if len(params) != len(flat):
            raise ValueError(f"{what}: expected {len(flat)} tensors (W, b per layer, net after net), got {len(params)}")
        tensors = [self._tensor(t, s, (torch.float32,)) for t, s in zip(params, flat)]
        for t, s in zip(tensors, flat):
            if tuple(t.shape) != tuple(s):
                raise ValueError(f"{what}: expected a tensor of shape {tuple(s)}, got {tuple(t.shape)}")
        return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors]), tensors

    @staticmethod
    def _head_dict(H) -> dict:
        names = {v: k for k, v in _ACTIVATIONS.items()}, {v: k for k, v in _OUTPUTS.items()}
        return {"widths": list(H.width[:H.n_layers]), "activation": names[0][H.activation], "output": names[1][H.output],
                "low": H.lo, "high": H.hi}
