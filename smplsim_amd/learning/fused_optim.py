"""The optimiser step on the library's own kernels (include/smplsim_mlp.h: ss_adam_step).

What it replaces: torch.nn.utils.clip_grad_norm_ (a chain of foreach-norm / stack / norm / clamp / foreach-mul launches) followed by torch.optim.Adam's step in
AgentPPO.update_params (the reference's agents/agent_ppo.py:85-88, agent_humanoid.py:110-111), and — for the weights whose bf16 images are attached — the two
multi-tensor bf16 copies of every network pass in learning/fused_train.py: the step writes the new fp32 weight, its bf16 image and its transposed bf16 image
from one launch.  Three launches per optimiser step, reproducible by construction (the header states the arithmetic and the order of every sum).

    opt = LibAdam(net.parameters(), lr=5e-5, max_grad_norm=25.0)       # max_grad_norm: an attribute of the object, not a param-group key
    opt.attach_images(layer.weight, w_bf16=..., wt_bf16=...)           # optional: images the step keeps current
    loss.backward(); opt.step(); opt.last_grad_norm                    # [] fp32 on the device: the norm before clipping

The state is torch's own (`step` a CPU fp32 tensor, `exp_avg`, `exp_avg_sq`) and the param groups carry exactly torch.optim.Adam's keys, so state_dict() loads into
a plain torch.optim.Adam on any device and the reverse.  No CPU path: the package has none.  One stream per object (its workspace is shared between its calls).
"""
import ctypes

import torch

from .. import _cabi
from .._lib import _check, _launch_stream, lib
from ._scratch import Scratch

_REFUSED = ("amsgrad", "maximize", "capturable", "differentiable", "decoupled_weight_decay")


def _refuse(group):
    for k in _REFUSED:
        if group.get(k):
            raise ValueError(f"LibAdam: {k}=True is not implemented by ss_adam_step")


class LibAdam(torch.optim.Adam):
    """torch.optim.Adam (amsgrad=False, maximize=False) whose step() is one ss_adam_step call per set of hyper-parameters.  max_grad_norm (None: off) clips the
    global gradient norm over the tensors of the call as clip_grad_norm_ does, inside the step; it needs all parameters with a gradient in ONE call (same
    hyper-parameters and step count, at most 32 tensors) and raises otherwise."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=None, **kw):
        _refuse(kw)
        for k in ("foreach", "fused"):
            if kw.get(k):
                raise ValueError(f"LibAdam: {k}=True selects one of torch's own implementations; the step here is ss_adam_step")
        if isinstance(lr, torch.Tensor):
            raise ValueError("LibAdam: lr must be a float (the step takes it as a host scalar)")
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        self.max_grad_norm = max_grad_norm
        self.last_grad_norm = None
        self._images = {}                                           # id(param) -> (w_bf16, wt_bf16)
        self._ws = Scratch()
        self._norm = None

    # ------------------------------------------------------------------ images
    def attach_images(self, param, w_bf16=None, wt_bf16=None):
        """Register bf16 images of a 2-D parameter [rows, cols] that every step() rewrites: w_bf16 [>= rows, >= cols] (W as torch.nn.Linear holds it) and wt_bf16
        [>= cols, >= rows] (W^T), row-major with unit column stride; the step writes [rows, cols] / [cols, rows] and leaves the padding alone.  The step changes
        such a parameter through raw pointers and does NOT advance its torch version counter: the images' owner relies on that (learning/fused_train.py)."""
        if param.dim() != 2:
            raise ValueError("attach_images: a 2-D parameter")
        rows, cols = param.shape
        for name, t, need in (("w_bf16", w_bf16, (rows, cols)), ("wt_bf16", wt_bf16, (cols, rows))):
            if t is None:
                continue
            if t.dtype != torch.bfloat16 or t.dim() != 2 or t.device != param.device or t.stride(1) != 1 or t.shape[0] < need[0] or t.shape[1] < need[1]:
                raise ValueError(f"attach_images: {name} must be a bf16 matrix of at least {need} on the parameter's device, unit column stride")
            if t.stride(0) % 8 or t.data_ptr() % 16:
                raise ValueError(f"attach_images: {name} needs a row stride that is a multiple of 8 and a 16-byte aligned base")
        self._images[id(param)] = (w_bf16, wt_bf16)

    # ------------------------------------------------------------------ state
    def load_state_dict(self, state_dict):
        """torch's load, with what another Adam variant left behind normalised once: the implementation switches of the saved groups (fused, foreach) are dropped,
        and a `step` saved as a device tensor (fused=True, capturable=True) becomes the CPU fp32 tensor torch's default Adam keeps."""
        sd = dict(state_dict)
        sd["param_groups"] = [dict(g, fused=None, foreach=None) if ("fused" in g or "foreach" in g) else dict(g) for g in state_dict["param_groups"]]
        for g in sd["param_groups"]:
            _refuse(g)
        super().load_state_dict(sd)
        for st in self.state.values():
            s = st.get("step")
            if s is not None:
                st["step"] = torch.as_tensor(s).detach().to(device="cpu", dtype=torch.float32).reshape(()).clone()   # (its own counter: torch's load keeps the tensor it is given)

    def _init_state(self, p):
        st = self.state[p]
        if len(st) == 0:
            st["step"] = torch.tensor(0.0, dtype=torch.float32)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return st

    # ------------------------------------------------------------------ the step
    @staticmethod
    def _describe(p, st, g, images):
        """One ss_adam_tensor: a 2-D tensor as it lies; a 1-D tensor as one row, or as one column when its gradient is strided.  A gradient in another layout is copied."""
        if p.dim() == 2:
            rows, cols = p.shape
            if g.stride(1) != 1 or g.stride(0) < cols:
                g = g.contiguous()
            ldg = g.stride(0)
        else:
            n = p.numel()
            g = g.reshape(-1) if p.dim() != 1 else g
            if n == 1 or g.stride(0) == 1:
                rows, cols, ldg = 1, n, n
            elif g.stride(0) > 1:
                rows, cols, ldg = n, 1, g.stride(0)
            else:
                g = g.contiguous()
                rows, cols, ldg = 1, n, n
        w, wt = images.get(id(p), (None, None))
        d = _cabi.AdamTensor(p=p.data_ptr(), m=st["exp_avg"].data_ptr(), v=st["exp_avg_sq"].data_ptr(), g=g.data_ptr(),
                             w_bf16=None if w is None else w.data_ptr(), wt_bf16=None if wt is None else wt.data_ptr(), rows=rows, cols=cols, ldg=ldg,
                             ld_w=0 if w is None else w.stride(0), ld_wt=0 if wt is None else wt.stride(0))
        return d, g

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        calls = {}                                                  # (hyper-parameters, step) -> [(param, state)]
        for group in self.param_groups:
            _refuse(group)
            if isinstance(group["lr"], torch.Tensor):
                raise ValueError("LibAdam: lr must be a float (the step takes it as a host scalar)")
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.device.type != "cuda":
                    raise RuntimeError("LibAdam needs its parameters on a GPU (there is no CPU path)")
                if p.grad.is_sparse:
                    raise RuntimeError("LibAdam does not support sparse gradients")
                if p.dtype != torch.float32 or p.grad.dtype != torch.float32 or not p.is_contiguous():
                    raise RuntimeError("LibAdam: parameters and gradients must be fp32, parameters contiguous")
                st = self._init_state(p)
                if st["exp_avg"].dtype != torch.float32 or not st["exp_avg"].is_contiguous() or not st["exp_avg_sq"].is_contiguous() or st["exp_avg"].device != p.device:
                    raise RuntimeError("LibAdam: exp_avg / exp_avg_sq must be contiguous fp32 tensors on the parameter's device")
                st["step"] += 1
                key = (float(group["lr"]), float(group["betas"][0]), float(group["betas"][1]), float(group["eps"]), float(group["weight_decay"]), int(st["step"].item()),
                       p.device)
                calls.setdefault(key, []).append((p, st))
        clip = self.max_grad_norm
        if clip is not None and len(calls) > 1:
            raise RuntimeError("LibAdam: max_grad_norm is the norm over ONE ss_adam_step call; the parameters with a gradient differ in hyper-parameters or step count")
        L = lib()
        for (lr, b1, b2, eps, wd, step, dev), items in calls.items():
            if len(items) > _cabi.ADAM_MAX_TENSORS and clip is not None:
                raise RuntimeError(f"LibAdam: max_grad_norm over more than {_cabi.ADAM_MAX_TENSORS} tensors")
            if self._norm is None or self._norm.device != dev:
                self._norm = torch.empty(1, dtype=torch.float32, device=dev)
            for i in range(0, len(items), _cabi.ADAM_MAX_TENSORS):
                chunk = items[i:i + _cabi.ADAM_MAX_TENSORS]
                table = (_cabi.AdamTensor * len(chunk))()
                keep = []                                           # gradients that had to be copied stay alive until the launches are enqueued
                for j, (p, st) in enumerate(chunk):
                    table[j], g = self._describe(p, st, p.grad, self._images)
                    keep.append(g)
                    if id(p) not in self._images:
                        torch.autograd.graph.increment_version(p)   # written in place behind torch's back: say so (parameters with images: see attach_images)
                ws = self._ws.get(dev, L.ss_adam_step_workspace(table, len(chunk)))
                _check(L.ss_adam_step(table, len(chunk), step, lr, b1, b2, eps, wd, float(clip) if clip is not None else 0.0, ctypes.c_void_p(self._norm.data_ptr()),
                                      ctypes.c_void_p(ws.data_ptr()), ws.numel() * 8, _launch_stream(dev)))
            self.last_grad_norm = self._norm[0]
        return loss
