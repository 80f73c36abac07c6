"""The cases of the fused-MLP oracle tests (test_mlp_oracle_cpu.py, test_fused_mlp_gpu.py): shapes, seeded operands, the oracle's pass over
them (computed once per case and shared), and the distance measures of both files.  No test lives here."""
import functools

import torch

from oracle import mlp_oracle as MO

D = 45                                                                  # kpad[0] = 128

# name -> (hidden, head, M, the dx256 list _Plan.per_rows must give at pad(M, 128) rows)
CASES = {
    "A": ((256, 256, 128), 69, 2100, [False, True, True, False]),       # both column-sum layers; Mp = 2176 = 8.5 x 256; the head through the small kernel
    "B": ((256, 128), 1, 2000, [False, True, False]),                   # Mp = 2048: exactly at the row threshold; 1-wide head
    "C": ((256, 192), 69, 2100, [False, False, False]),                 # n_outp = 192: not a multiple of 128
    "D": ((128, 64), 69, 130, [False, False, False]),                   # K = 64 products; Mp = 256
    "E": ((128, 64), 1, 1, [False, False, False]),                      # one real row
}
# (case, activation) of every comparison with the oracle; A and B also run with deterministic=True
RUNS = [("A", "silu"), ("A", "tanh"), ("A", "relu"), ("B", "silu"), ("C", "silu"), ("D", "silu"), ("E", "silu")]
Z_STD = 2.0                                                             # pre-activations of rms 2: +-6 is three of them


@functools.lru_cache(maxsize=None)
def operands(case, act):
    """x [M, D], Ws, bs (fp32, NOT bf16-exact), grad_out [M, head] on the CPU.  Laid out as test_gemm_kernels_gpu._operands does (a ramp over the
    columns of x and the rows of W: a row or column swap cannot pass; an all-zero row of x and of every W), each hidden layer's weights then
    scaled so that its pre-activations over THIS batch have root mean square Z_STD: they span +-6 whatever the activation below feeds it."""
    hidden, head, M, _ = CASES[case]
    g = torch.Generator().manual_seed(1000 * (ord(case) - 64) + MO.ACTS.index(act))
    x = torch.randn(M, D, generator=g) + torch.linspace(-0.5, 1.0, D)[None, :]
    if M > 3:
        x[3] = 0.0
    dims = [D, *hidden, head]
    Ws, bs, h = [], [], x.double()
    for i in range(len(dims) - 1):
        K, N = dims[i], dims[i + 1]
        w = (torch.randn(N, K, generator=g) + torch.linspace(-0.3, 0.6, N)[:, None]).double()
        if N > 5:
            w[5] = 0.0
        last = i == len(dims) - 2
        w = w * ((1.0 if last else Z_STD) / (h @ w.T).square().mean().sqrt().clamp_min(1e-6))
        b = torch.randn(N, generator=g) * 0.5
        Ws.append(w.float())
        bs.append(b)
        h = MO.act64(h @ Ws[-1].double().T + b.double(), act)
    grad_out = torch.randn(M, head, generator=g)
    return x, tuple(Ws), tuple(bs), grad_out


@functools.lru_cache(maxsize=None)
def reference(case, act, accumulate="fp64"):
    """The oracle's pass over operands(case, act).  Shared: read it, do not write it."""
    x, Ws, bs, go = operands(case, act)
    return MO.train_pass(x, Ws, bs, go, act, CASES[case][3], accumulate=accumulate)


INFER = [(hidden, act) for hidden in ((128, 64), (256, 256, 128)) for act in ("silu", "tanh")]
INFER_M = (1, 37, 300)
OBS_STRIDE, OBS_OFF = 50, 2                                             # the observations: columns OBS_OFF .. OBS_OFF + D of a [M, OBS_STRIDE] tensor


@functools.lru_cache(maxsize=None)
def policy_case(hidden, act, normed):
    """(PolicyGaussian(D, 69, hidden, act) on the CPU with its own initialisation, {M: [M, OBS_STRIDE] fp32}); normed: RunningNorm statistics as after 7 rows
    (n = 0 otherwise: the policy sees the clamped observation).  Shared: deep-copy the policy before moving it."""
    from smplsim_amd.learning.networks import PolicyGaussian
    g = torch.Generator().manual_seed(100 * len(hidden) + len(act) + 10 * normed)
    torch.manual_seed(len(hidden) * 10 + len(act))
    policy = PolicyGaussian(D, 69, hidden, act)
    if normed:
        with torch.no_grad():
            policy.norm.mean.copy_(torch.randn(D, generator=g) * 0.5)
            policy.norm.var.copy_((torch.rand(D, generator=g) + 0.5) ** 2)
            policy.norm.std.copy_(policy.norm.var.sqrt())
            policy.norm.n.fill_(7)
    return policy.eval(), {M: torch.randn(M, OBS_STRIDE, generator=g) * 3 for M in INFER_M}


def distances(got, ref):
    """got, ref: dict(y, dW, db[, db_scale]) -> {class: [per tensor]}.  y and the weight gradients by relative norm, the weight gradients also by
    max |difference| over max |reference|; a bias gradient against ref's db_scale, the sum of the magnitudes of its terms (the scaling of
    test_fused_update_at_production_width_against_fp64_autograd), by norm and element-wise."""
    f = lambda t: t.detach().cpu().double()
    out = dict(y=[((f(got["y"]) - ref["y"]).norm() / ref["y"].norm()).item()], w_norm=[], w_elem=[], b_norm=[], b_elem=[])
    for a, b in zip(got["dW"], ref["dW"]):
        d = f(a) - b
        out["w_norm"].append((d.norm() / b.norm()).item())
        out["w_elem"].append((d.abs().max() / b.abs().max()).item())
    for a, b, s in zip(got["db"], ref["db"], ref["db_scale"]):
        d = f(a) - b
        out["b_norm"].append((d.norm() / s.norm()).item())
        out["b_elem"].append((d.abs() / s.clamp_min(1e-300)).max().item())    # (a column without terms: both sides exactly 0)
    return out
