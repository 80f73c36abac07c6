"""CPU restatement (float64 torch, no kernels) of the fused MLP passes: test infrastructure, like the rest of oracle/.

What it restates is smplsim_amd/learning/fused_train.py (_FusedMLP.forward / .backward) and the forward chain of
smplsim_amd/learning/fast_policy.py (FusedPolicyInference.mean), with a rounding to bf16 at every place where those passes store a
bf16 tensor and nowhere else.  What is then left between the GPU and this file is the order of the fp32 accumulations and the fast
exp / rcp of the activation epilogues (csrc/ss_gemm128.h:41-42, 441-442).  It imports nothing of smplsim_amd.learning.

Rounding points (R*) and the lines they restate:
  R1  h_0 = rb(x)            fused_train.py `h[:M, :x.shape[1]] = x` (fp32 -> bf16 copy; FusedMLPTrain.operand: `t[:M, :D] = x`);
                             fast_policy.py: ss_obs_to_bf16 writes the bf16 operand (forward_only takes it as it is)
  R2  Wb_i = rb(W_i)         fused_train.py `torch._foreach_copy_([wbs[i][:, :n_in] ...], ws)` (and _WeightImages.refresh_moved);
                             fast_policy.py refresh(): `l.weight.detach().to(torch.bfloat16)`
  R3  h_{i+1} = rb(act(z_i)) ss_gemm128.h `Cs[...] = (__bf16)fn(acc[tn][r])` (ss_gemm256_kernels.h `Cs[at] = (__bf16)h`): the bias is added to the
                             fp32 accumulator first, nothing is rounded between the product and the activation
  R4  g_i = rb(act'(z_i))    ss_gemm128.h:441-444 `Cs[...] = (__bf16)d` (ss_gemm256_kernels.h `Cs[HALF_IMG + at] = (__bf16)d`)
  --  y = h_L Wb_L^T + b_L   NOT rounded: fused_train.py's head is ss_linear_bf16 with an fp32 output (`out = torch.empty(..., float32)`),
                             and so is fast_policy.py's last layer (`int(last)`)
  R5  dz_L = rb(grad_out)    fused_train.py `dz[:M, :nh] = grad_out`
  --  db_L = colsum(dz_L)    fused_train.py: ss_wgrad_bf16 of dz_head against a column of ones, fp32 sums of the bf16 values
  --  dW_i = dz_i^T h_i      fused_train.py `wgrad(dz, ctx.hs[i], dw, ...)`: bf16 operands, fp32 result, not rounded
  R6  dz_{i-1} = rb(r), r = (dz_i Wb_i) * g_{i-1}
                             the multiply happens on the fp32 accumulator (ss_gemm128.h `v *= (float)a.mul[...]`, ss_gemm256_kernels.h
                             `v *= (float)Cs[...]`), the product is stored as bf16
  --  db_{i-1} = colsum(r)        where dx256[i]: ss_gemm256_kernels.h sums `acc[tm][tn][r]` (fp32, after the multiply, before the store)
      db_{i-1} = colsum(rb(r))    otherwise: fused_train.py `dz[:, :n_out].sum(0, dtype=torch.float32)` sums the stored bf16 tensor
The biases are fp32 and enter as they are (`bs[i].detach().float()`).
"""
import torch

ACTS = ("silu", "tanh", "relu")


def rb(v):
    """fp64 -> fp32 (round to nearest even) -> bf16 (round to nearest even) -> fp64."""
    return v.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def _ident(v):
    return v


def act64(z, act):
    if act == "silu":
        return z * torch.sigmoid(z)
    if act == "tanh":
        return torch.tanh(z)
    if act == "relu":
        return torch.where(z > 0, z, torch.zeros_like(z))
    raise ValueError(act)


def dact64(z, act):
    """The kernel's own expressions (ss_gemm128.h:441-443)."""
    if act == "silu":
        s = torch.sigmoid(z)
        return s * (1 + z * (1 - s))
    if act == "tanh":
        return 1 - torch.tanh(z) ** 2
    if act == "relu":
        return (z > 0).to(z.dtype)
    raise ValueError(act)


def _ops(accumulate):
    """(matmul, column sum) of fp64 tensors, evaluated in fp64 or in fp32 (the oracle's own noise estimator: the GPU's accumulators are fp32)."""
    if accumulate == "fp64":
        return (lambda a, b: a @ b), (lambda a: a.sum(0))
    if accumulate == "fp32":
        f = torch.float32
        return (lambda a, b: (a.to(f) @ b.to(f)).double()), (lambda a: a.to(f).sum(0).double())
    raise ValueError(accumulate)


def _f64(t):
    return torch.as_tensor(t).detach().cpu().to(torch.float64)


def forward_only(operand_bf16, Ws, bs, act, accumulate="fp64"):
    """The inference chain (fast_policy.py mean()): operand_bf16 [M, >= D] is the bf16 first-layer operand as ss_obs_to_bf16 left it (columns
    past D ignored); R2, R3 per hidden layer, the head unrounded.  Returns y [M, n_head] fp64."""
    mm, _ = _ops(accumulate)
    Ws, bs = [_f64(w) for w in Ws], [_f64(b) for b in bs]
    h = _f64(operand_bf16)[:, :Ws[0].shape[1]]
    for i, (W, b) in enumerate(zip(Ws, bs)):
        z = mm(h, rb(W).T) + b
        h = rb(act64(z, act)) if i < len(Ws) - 1 else z
    return h


def train_pass(x, Ws, bs, grad_out, act, dx256, accumulate="fp64", round=True):
    """One tracked pass of FusedMLPTrain and its backward (module docstring).  x [M, D], Ws[i] [n_out, n_in], bs[i] [n_out], grad_out [M, n_head];
    dx256[i]: layer i's dX product takes the 256 x 256 kernel (the bias gradient of layer i - 1 from its fp32 column sums).
    Returns dict(y, dW, db, db_scale): db_scale[i] = the column sums of the MAGNITUDES of the terms db[i] adds up."""
    r_ = rb if round else _ident
    mm, colsum = _ops(accumulate)
    Ws, bs = [_f64(w) for w in Ws], [_f64(b) for b in bs]
    nl = len(Ws)
    assert len(bs) == nl and len(dx256) == nl and not dx256[0]
    Wb = [r_(W) for W in Ws]                                           # R2
    hs, gs = [r_(_f64(x))], []                                         # R1
    for i in range(nl - 1):
        z = mm(hs[-1], Wb[i].T) + bs[i]
        hs.append(r_(act64(z, act)))                                   # R3
        gs.append(r_(dact64(z, act)))                                  # R4
    y = mm(hs[-1], Wb[-1].T) + bs[-1]
    dz = r_(_f64(grad_out))                                            # R5
    dW, db, scale = [None] * nl, [None] * nl, [None] * nl
    db[-1], scale[-1] = colsum(dz), dz.abs().sum(0)
    for i in range(nl - 1, -1, -1):
        dW[i] = mm(dz.T, hs[i])
        if i > 0:
            r = mm(dz, Wb[i]) * gs[i - 1]
            dzb = r_(r)                                                # R6
            terms = r if dx256[i] else dzb
            db[i - 1], scale[i - 1] = colsum(terms), terms.abs().sum(0)
            dz = dzb
    return dict(y=y, dW=dW, db=db, db_scale=scale)
