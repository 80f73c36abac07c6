"""The scratch the library's entries ask for by their `_workspace` queries (learning/fused_loss.py, fused_optim.py, fused_norm.py, fused_train.py)."""
import torch

from .._lib import lib


class Scratch:
    """One grow-only fp64 workspace per device.  Every entry overwrites its workspace before it reads it and an owner's calls go on one stream: one buffer serves them all."""

    def __init__(self):
        self.t = {}

    def get(self, device, nbytes):
        """nbytes: the answer of an `ss_*_workspace` query; negative (the query refused its arguments): the library's own message as a RuntimeError."""
        if nbytes < 0:
            raise RuntimeError(lib().ss_last_error().decode())
        t = self.t.get(device)
        if t is None or t.numel() * 8 < nbytes:
            t = self.t[device] = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=device)
        return t
