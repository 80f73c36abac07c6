"""The PPO update's loss heads on the library's own kernels (include/smplsim_mlp.h: ss_ppo_policy_head, ss_value_head).

What it replaces: the torch expressions between a network's output and `loss.backward()` in AgentPPO.ppo_loss / update_value (the reference's
agents/agent_ppo.py:20-83) — log-density of the Gaussian head, ratio, clamp, minimum, mean, the MSE — about 15 elementwise and reduction launches
forward and as many through autograd.  Here the forward call runs the head kernel, which already leaves the loss's gradient with respect to the
network's output (and to log_std); backward only scales it by the incoming gradient.  The results are reproducible by construction (fixed-order
fp64 sums, no atomics: the header states the order) and do not depend on how torch orders its reductions.

    loss = ppo_surrogate(mean, log_std, actions, adv, old_logp, clip_eps)      # 0-dim; ppo_surrogate.last_stats = [loss, clip_frac, approx_kl, mean_ratio]
    loss = value_mse(pred, target)

No CPU path: the package has none.  One stream per caller: a PPOSurrogate / ValueMSE object (the module-level `ppo_surrogate` and `value_mse` are such objects)
keeps one workspace (learning/_scratch.py), so two calls of one object must not be in flight on different streams; use an object per stream.
"""
import torch

from .._lib import _check, _launch_stream, _ptr, lib
from ._scratch import Scratch


def _rows(t, M, what):
    t = t.detach().reshape(-1)
    if t.numel() != M:
        raise ValueError(f"{what}: {t.numel()} values for {M} rows")
    return t.float().contiguous()


def _matrix(t):
    """[M, dim] fp32 with unit column stride as the kernel reads it: (tensor, row stride)."""
    t = t.detach()
    if t.dtype != torch.float32 or t.stride(1) != 1 or t.stride(0) < t.shape[1]:
        t = t.float().contiguous()
    return t, t.stride(0)


class _Surrogate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mean, log_std, actions, adv, old_logp, clip_eps, owner):
        M, dim = mean.shape
        m, ldm = _matrix(mean)
        a, lda = _matrix(actions)
        if a.shape != m.shape:
            raise ValueError(f"actions {tuple(a.shape)} against mean {tuple(m.shape)}")
        ls = log_std.detach().reshape(-1)
        if ls.numel() != dim:
            raise ValueError(f"log_std: {ls.numel()} values for {dim} action dimensions")
        ls = ls.float().contiguous()
        dev = m.device
        L = lib()
        dmean = torch.empty(M, dim, dtype=torch.float32, device=dev)
        dls = torch.empty(dim, dtype=torch.float32, device=dev)
        stats = torch.empty(4, dtype=torch.float32, device=dev)
        ws = owner.ws.get(dev, L.ss_ppo_policy_head_workspace(M, dim))
        _check(L.ss_ppo_policy_head(_ptr(m), ldm, _ptr(a), lda, _ptr(ls), _ptr(_rows(adv, M, "adv")), _ptr(_rows(old_logp, M, "old_logp")), M, dim, float(clip_eps),
                                    None, _ptr(dmean), dim, 0, _ptr(dls), _ptr(stats), _ptr(ws), ws.numel() * 8, _launch_stream(dev)))
        owner.last_stats = stats
        ctx.save_for_backward(dmean, dls)
        ctx.ls_shape = log_std.shape
        return stats[0].clone()

    @staticmethod
    def backward(ctx, grad_out):
        dmean, dls = ctx.saved_tensors
        g_ls = (grad_out * dls).reshape(ctx.ls_shape) if ctx.needs_input_grad[1] else None
        return grad_out * dmean, g_ls, None, None, None, None, None


class _ValueMSE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, owner):
        p = pred.detach().reshape(-1).float().contiguous()
        M = p.numel()
        t = _rows(target, M, "target")
        dev = p.device
        L = lib()
        dpred = torch.empty(M, dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        ws = owner.ws.get(dev, L.ss_value_head_workspace(M))
        _check(L.ss_value_head(_ptr(p), _ptr(t), M, _ptr(dpred), 1, 0, _ptr(loss), _ptr(ws), ws.numel() * 8, _launch_stream(dev)))
        ctx.save_for_backward(dpred)
        ctx.shape = pred.shape
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        (dpred,) = ctx.saved_tensors
        return (grad_out * dpred).reshape(ctx.shape), None, None


def _need_gpu(name, *tensors):
    for t in tensors:
        if t.device.type != "cuda":
            raise RuntimeError(f"{name} needs its tensors on a GPU (there is no CPU path)")


class PPOSurrogate:
    """loss = -mean(min(r A, clamp(r, 1 - eps, 1 + eps) A)), r = exp(logp(actions; mean, log_std) - old_logp): differentiable with respect to `mean`
    [M, dim] and `log_std` ([dim] or [1, dim]).  Calls of one object go on one stream (its workspace is shared between them).  `last_stats`: the [loss, clip_frac, approx_kl, mean_ratio] tensor of the latest call (on the device)."""

    def __init__(self):
        self.ws = Scratch()
        self.last_stats = None

    def __call__(self, mean, log_std, actions, adv, old_logp, clip_eps):
        _need_gpu("ppo_surrogate", mean, log_std, actions, adv, old_logp)
        return _Surrogate.apply(mean, log_std, actions, adv, old_logp, clip_eps, self)


class ValueMSE:
    """loss = mean((pred - target)^2) over all elements, differentiable with respect to `pred`.  Calls of one object go on one stream (its workspace is shared
    between them)."""

    def __init__(self):
        self.ws = Scratch()

    def __call__(self, pred, target):
        _need_gpu("value_mse", pred, target)
        return _ValueMSE.apply(pred, target, self)


ppo_surrogate = PPOSurrogate()
value_mse = ValueMSE()
