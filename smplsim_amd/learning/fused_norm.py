"""RunningNorm in train mode on the library's own kernels (include/smplsim_mlp.h: ss_running_norm_update, ss_obs_to_bf16).

What it replaces: RunningNorm.forward in train mode (learning/networks.py; the reference's running_norm.py:22-42) in front of the policy's pass of every optimisation
iteration of AgentPPO.update_params — var_mean and about eight small launches for the merge, then sub, div, clamp and where, each writing a fresh fp32 tensor of the
batch's size, then the pass's own cast of the result into its padded bf16 operand.  Here: two launches for the statistics (fp64, rounded once, fixed order, no atomics:
the header states the arithmetic) and one that writes the normalised bf16 operand the first layer's product reads.

    norm = LibRunningNorm(policy.norm)
    mean = fused_policy(norm(states))          # a Bf16Operand (learning/fused_train.py): the pass takes it as it is

The module's own buffers (n, mean, var, std) remain the state: checkpoints, the torch path and FusedPolicyInference see nothing new.  No CPU path: the package has none.
One stream per object (its workspace and its operand are shared between its calls).
"""
import torch

from .._lib import _check, _launch_stream, _ptr, lib
from ._scratch import Scratch
from .fused_train import Bf16Operand, _pad

_FLT_MAX = 3.4028234663852886e38


class LibRunningNorm:
    """Callable over an existing RunningNorm module: update(x) merges the batch into the module's buffers, operand(x) is the normalised batch as the padded bf16
    operand of FusedMLPTrain, calling the object is the first (while the module is in train mode) followed by the second."""

    def __init__(self, norm_module):
        if not (norm_module.demean and norm_module.destd):
            raise ValueError("LibRunningNorm: demean=False / destd=False are not implemented by ss_obs_to_bf16")
        self.module = norm_module
        self.dim = int(norm_module.dim)
        self._check_buffers()
        self._ws = Scratch()
        self._out = None                                            # the operand of the most recent M: a Bf16Operand

    def _check_buffers(self):
        m = self.module
        for name in ("n", "mean", "var", "std"):
            if getattr(m, name).device.type != "cuda":
                raise RuntimeError("LibRunningNorm needs the module's buffers on a GPU (there is no CPU path)")
        if m.n.dtype != torch.int64 or any(t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != self.dim for t in (m.mean, m.var, m.std)):
            raise RuntimeError("LibRunningNorm: n must be int64; mean, var, std contiguous fp32 [dim]")

    def _input(self, x):
        m = self.module
        if x.dim() != 2 or x.shape[1] != self.dim or x.shape[0] < 1 or x.dtype != torch.float32 or x.device != m.mean.device:
            raise ValueError(f"LibRunningNorm: the input must be an fp32 [M >= 1, {self.dim}] tensor on the buffers' device")
        return x.detach() if x.stride(1) == 1 and x.stride(0) >= self.dim else x.detach().contiguous()

    @torch.no_grad()
    def update(self, x):
        """RunningNorm.update(x) by ss_running_norm_update: the module's buffers change in place, in stream order."""
        self._check_buffers()
        x = self._input(x)
        m, M, L = self.module, x.shape[0], lib()
        ws = self._ws.get(x.device, L.ss_running_norm_workspace(M, self.dim))
        _check(L.ss_running_norm_update(_ptr(x), M, self.dim, x.stride(0), _ptr(m.mean), _ptr(m.var), _ptr(m.std), _ptr(m.n), _ptr(ws), ws.numel() * 8,
                                        _launch_stream(x.device)))
        for t in (m.mean, m.var, m.std, m.n):
            torch.autograd.graph.increment_version(t)               # written in place behind torch's back: say so

    @torch.no_grad()
    def operand(self, x):
        """clamp((x - mean) / (std + 1e-8), -clip, clip) (x itself while n == 0), rounded to bf16 into a persistent [pad(M, 128), pad(dim, 128)] tensor whose pad rows
        and columns are zero.  Consecutive calls with one M return the same tensor (only the latest M's is kept): it must not be needed any more when the next call is enqueued."""
        self._check_buffers()
        x = self._input(x)
        m, M, kpad = self.module, x.shape[0], _pad(self.dim, 128)
        if self._out is None or self._out.M != M:
            self._out = Bf16Operand(torch.zeros(_pad(M, 128), kpad, dtype=torch.bfloat16, device=x.device), M, self.dim)
        _check(lib().ss_obs_to_bf16(_ptr(x), M, self.dim, x.stride(0), _ptr(m.mean), _ptr(m.std), _ptr(m.n), -_FLT_MAX, _FLT_MAX,
                                    float(m.clip) if m.clip else _FLT_MAX, _ptr(self._out.t), kpad, _launch_stream(x.device)))
        return self._out

    def __call__(self, x):
        if self.module.training:
            self.update(x)
        return self.operand(x)
