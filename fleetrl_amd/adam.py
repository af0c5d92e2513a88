"""`DeviceAdam`: `clip_grad_norm_`, `torch.optim.Adam.step()` and the `load_torch` behind them in two launches (include/fleet_hip.h
`fleet_adam_*`, fleetrl_amd/csrc/fleet_adam.hip).

The optimiser is made ON the weight image of a `DevicePolicy` or a `DeviceTD3Target` and owns a span of its networks plus up to two
flat tensors that are in no image (PPO's `log_std`).  A step reads the `.grad` of torch's own parameters -- where `DevicePPOGrad` and
`DeviceTD3Grad` wrote them --, forms the global norm in a stated order, applies SB3's clip and torch's Adam update, and writes every
new weight both to the torch parameter and, transposed, to the image: nothing is left to `load_torch`.  Deterministic from the
gradients to the weights; the arithmetic is the header's and tests/adam_model.py's, bit for bit.
"""
from __future__ import annotations

import ctypes as C

from . import _capi
from ._handle import _ImageBorrower

__all__ = ["DeviceAdam"]


def _net_layers(image) -> list:
    """Layers per net of the image, in the image's order."""
    d = image.describe()
    if image._prefix == "policy":
        return [len(h["widths"]) for h in d["heads"]]
    if image._prefix == "qtarget":
        return [len(d["actor"]["widths"])] + [len(c["widths"]) for c in d["critics"]]
    raise TypeError("image must be a DevicePolicy or a DeviceTD3Target")


class DeviceAdam(_ImageBorrower):
    """One `fleet_adam_*` handle on `image` (a `DevicePolicy` or a `DeviceTD3Target`, which must outlive it).

    nets: None (every net of the image), "actor" (net 0), "critic" (the nets behind it), "none" (no net: a flat Adam over the extras).
    params: the torch parameters of the span in `load_torch`'s order (W, b per layer, net after net), then at most two extras of
    any shape.  Their `.grad` is what a step reads.  lr, betas, eps: torch.optim.Adam's; max_grad_norm: `clip_grad_norm_`'s over ALL
    of `params`, None or <= 0 for no clipping.  It launches on the image's stream."""
    _prefix = "adam"

    def __init__(self, image, params, *, nets=None, lr: float = 3e-4, betas=(0.9, 0.999), eps: float = 1e-8, max_grad_norm=None):
        self.image = image
        per_net = _net_layers(image)
        spans = {None: (0, len(per_net)), "actor": (0, 1), "critic": (1, len(per_net) - 1), "none": (0, 0)}
        if nets not in spans:
            raise ValueError(f"nets must be None, 'actor', 'critic' or 'none', got {nets!r}")
        first, n = spans[nets]
        flat = [tuple(s) for pair in image._shapes for s in pair]
        lo = 2 * sum(per_net[:first])
        self._shapes = flat[lo:lo + 2 * sum(per_net[first:first + n])]
        params = list(params)
        n_extra = len(params) - len(self._shapes)
        if n_extra < 0 or n_extra > _capi.ADAM_MAX_EXTRA:
            raise ValueError(f"params: expected {len(self._shapes)} tensors of the span (W, b per layer, net after net) and at most "
                             f"{_capi.ADAM_MAX_EXTRA} extras, got {len(params)}")
        for p, s in zip(params, self._shapes):
            if tuple(p.shape) != s:
                raise ValueError(f"params: expected a parameter of shape {s}, got {tuple(p.shape)}")
        self._shapes = self._shapes + [tuple(p.shape) for p in params[len(self._shapes):]]
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.max_grad_norm = 0.0 if max_grad_norm is None else float(max_grad_norm)
        p = _capi.FleetAdamParams()
        p.struct_bytes, p.first_net, p.n_nets, p.n_extra = C.sizeof(p), first, n, n_extra
        for i, t in enumerate(params[len(params) - n_extra:] if n_extra else []):
            p.extra_len[i] = t.numel()
        self._open_on(image, f"fleet_adam_create_{image._prefix}", p)
        self.params = params
        self._ptrs = None  # (the pointer arrays of the parameters and of their .grad, the addresses) of the last step

    def describe(self) -> dict:
        """What fleet_adam_describe reports."""
        p, info = _capi.FleetAdamParams(), _capi.FleetAdamInfo()
        self._check(self.lib.fleet_adam_describe(self.h, C.byref(p), C.byref(info)))
        return {"first_net": p.first_net, "n_nets": p.n_nets, "n_extra": p.n_extra, "extra_len": list(p.extra_len[:p.n_extra]),
                "state_bytes": int(info.state_bytes), "n_elements": int(info.n_elements), "step": int(info.step),
                "n_tensors": info.n_tensors, "norm_chunk": info.norm_chunk, "step_tile": info.step_tile}

    def step_dev(self, args: "_capi.FleetAdamStepArgs", param_ptrs, grad_ptrs, count: int):
        """Raw device addresses in two (c_void_p * count) arrays, on the image handle's stream."""
        args.struct_bytes = C.sizeof(_capi.FleetAdamStepArgs)
        self._check(self.lib.fleet_adam_step_dev(self.h, C.byref(args), param_ptrs, grad_ptrs, int(count)))

    def _pointers(self):
        import torch

        hit = self._ptrs
        if hit is not None and all(p.data_ptr() == a and p.grad is not None and p.grad.data_ptr() == b
                                   for p, a, b in zip(self.params, hit[2], hit[3])):
            return hit[0], hit[1]
        f32 = (torch.float32,)
        pa, ga = [], []
        for i, (p, s) in enumerate(zip(self.params, self._shapes)):
            if p.grad is None:
                raise ValueError(f"parameter {i} has no .grad")
            pa.append(self._tensor(p.detach(), s, f32).data_ptr())
            ga.append(self._tensor(p.grad, s, f32).data_ptr())
        n = len(pa)
        self._ptrs = ((C.c_void_p * n)(*pa), (C.c_void_p * n)(*ga), pa, ga)
        return self._ptrs[0], self._ptrs[1]

    def step_gated_dev(self, args: "_capi.FleetAdamStepArgs", param_ptrs, grad_ptrs, count: int, skip_ptr: int):
        """The same through fleet_adam_step_gated_dev: `skip_ptr` is the address of a device u32."""
        args.struct_bytes = C.sizeof(_capi.FleetAdamStepArgs)
        self._check(self.lib.fleet_adam_step_gated_dev(self.h, C.byref(args), param_ptrs, grad_ptrs, int(count), skip_ptr))

    def settle(self, base_step: int, steps_taken):
        """The step count becomes `base_step` + the one-element int32 / uint32 device tensor `steps_taken`, read behind everything
        enqueued so far (fleet_adam_settle_dev): enqueue-only; whoever asks for the count next waits for it."""
        import torch

        self.use_torch_stream()
        words = (torch.int32, torch.uint32) if hasattr(torch, "uint32") else (torch.int32,)
        self._check(self.lib.fleet_adam_settle_dev(self.h, int(base_step), self._tensor(steps_taken, (1,), words).data_ptr()))

    def step(self, lr=None, norm_out=None, skip=None):
        """One optimiser step on torch's current stream, no host synchronisation: the parameters and the image move together.
        lr: this step's learning rate (default: the constructor's; SB3 sets it every iteration).  norm_out f32 [1] on the device:
        the gradients' norm before clipping, what `clip_grad_norm_` returns.  skip: None, or a one-element int32 / uint32 device
        tensor written by something enqueued earlier (fleet_adam_step_gated_dev): nonzero when the launches run means that they
        return at once and write nothing; the step count on the host advances all the same (`settle` says afterwards how many ran)."""
        import torch

        self.use_torch_stream()
        a = _capi.FleetAdamStepArgs()
        a.lr = self.lr if lr is None else float(lr)
        a.beta1, a.beta2, a.eps, a.max_grad_norm = self.betas[0], self.betas[1], self.eps, self.max_grad_norm
        if norm_out is not None:
            a.norm_out = self._tensor(norm_out, (1,), (torch.float32,)).data_ptr()
        pa, ga = self._pointers()
        if skip is None:
            self.step_dev(a, pa, ga, len(self.params))
        else:
            words = (torch.int32, torch.uint32) if hasattr(torch, "uint32") else (torch.int32,)
            self.step_gated_dev(a, pa, ga, len(self.params), self._tensor(skip, (1,), words).data_ptr())

    def export_image(self, out_tensors=None) -> list:
        """The WHOLE weight image (every net of it) in torch's layout, into `out_tensors` (ordered and shaped as for the image's
        `load_torch`; made when None): one launch on torch's current stream.  After a step the span's tensors equal the parameters."""
        import torch

        if out_tensors is None:
            dev = torch.device("cuda", self.device)
            out_tensors = [torch.empty(tuple(s), device=dev, dtype=torch.float32) for pair in self.image._shapes for s in pair]
        ptrs, keep = self.image._pointers("export_image", out_tensors)
        self._check(self.lib.fleet_adam_export_image_dev(self.h, ptrs, len(keep)))
        return keep

    # ---- the state, in torch.optim.Adam's format -------------------------------------------------------------------------------
    def _state_dev(self, mode, exp_avg, exp_avg_sq, step: int) -> int:
        import torch

        self.use_torch_stream()
        f32 = (torch.float32,)
        if len(exp_avg) != len(self._shapes) or len(exp_avg_sq) != len(self._shapes):
            raise ValueError(f"expected the state of {len(self._shapes)} tensors, got {len(exp_avg)} and {len(exp_avg_sq)}")
        ma = [self._tensor(t, s, f32) for t, s in zip(exp_avg, self._shapes)]
        va = [self._tensor(t, s, f32) for t, s in zip(exp_avg_sq, self._shapes)]
        n = len(ma)
        st = C.c_int64(int(step))
        self._check(self.lib.fleet_adam_state_dev(self.h, mode, (C.c_void_p * n)(*[t.data_ptr() for t in ma]),
                                                  (C.c_void_p * n)(*[t.data_ptr() for t in va]), n, C.byref(st)))
        return int(st.value)

    def state_dict(self) -> dict:
        """`torch.optim.Adam.state_dict()`'s format: state[i] = {step, exp_avg, exp_avg_sq} (copies on the device, in the
        parameters' shapes) and one param group with the hyperparameters."""
        import torch

        dev = torch.device("cuda", self.device)
        m = [torch.empty(s, device=dev, dtype=torch.float32) for s in self._shapes]
        v = [torch.empty(s, device=dev, dtype=torch.float32) for s in self._shapes]
        step = self._state_dev(_capi.ADAM_STATE_EXPORT, m, v, 0)
        state = {i: {"step": torch.tensor(float(step)), "exp_avg": m[i], "exp_avg_sq": v[i]} for i in range(len(m))} if step else {}
        # the param group of the installed torch's own Adam, so that its load_state_dict finds every key it knows
        group = torch.optim.Adam([torch.zeros(1)], lr=self.lr, betas=self.betas, eps=self.eps).state_dict()["param_groups"][0]
        group["params"] = list(range(len(m)))
        return {"state": state, "param_groups": [group]}

    def load_state_dict(self, sd: dict):
        """From `state_dict()`'s or `torch.optim.Adam.state_dict()`'s: the moments of every parameter and ONE step count (torch keeps
        one per parameter; they must agree).  An empty state resets the optimiser.  lr, betas and eps are taken from the param group."""
        import torch

        dev = torch.device("cuda", self.device)
        state, n = sd["state"], len(self._shapes)
        if len(sd["param_groups"]) != 1 or len(sd["param_groups"][0]["params"]) != n:
            raise ValueError(f"expected one param group of {n} parameters")
        g = sd["param_groups"][0]
        if g.get("weight_decay", 0) or g.get("amsgrad", False) or g.get("maximize", False):
            raise ValueError("weight_decay, amsgrad and maximize are not supported")
        if not state:
            m = [torch.zeros(s, device=dev, dtype=torch.float32) for s in self._shapes]
            v, step = [torch.zeros_like(t) for t in m], 0
        else:
            if sorted(state) != list(range(n)):
                raise ValueError(f"expected the state of parameters 0..{n - 1}")
            steps = {int(float(state[i]["step"])) for i in range(n)}
            if len(steps) != 1:
                raise ValueError(f"the parameters' step counts differ: {sorted(steps)}")
            step = steps.pop()
            conv = lambda t, s: t.detach().to(device=dev, dtype=torch.float32).reshape(s).contiguous()  # noqa: E731
            m = [conv(state[i]["exp_avg"], s) for i, s in enumerate(self._shapes)]
            v = [conv(state[i]["exp_avg_sq"], s) for i, s in enumerate(self._shapes)]
        self._state_dev(_capi.ADAM_STATE_LOAD, m, v, step)
        self.lr, self.betas, self.eps = float(g["lr"]), (float(g["betas"][0]), float(g["betas"][1])), float(g["eps"])
        # the copies were enqueued on torch's current stream, where `m` and `v` were made: they may go when this returns
