"""FusedMLPTrain's forward and backward (learning/fused_train.py: a Python chain rule over ss_linear_bf16_train, ss_linear_bf16, ss_wgrad_bf16[_det],
ss_linear_bf16_dx[_det]) and FusedPolicyInference.mean (learning/fast_policy.py) against oracle/mlp_oracle.py: a float64 pass that rounds to bf16 where
the kernels store bf16, so that what is left between the two is fp32 accumulation order and the epilogues' fast exp / rcp.  The single kernels have
their tests in test_gemm_kernels_gpu.py; this file is about which buffer feeds which product.

The cases (fused_mlp_cases.CASES) are chosen by the paths of _Plan.per_rows: the 256 x 256 dX kernel with the bias gradient from its column sums
(A, B: at the row threshold), its veto by a width (C), the small kernels with K = 64 and mostly padding rows (D, E); each asserts the dx256 list it
is meant to reach.  The gates are 3x the worst distance measured on the MI355X, per class; the measured table, the oracle's own noise E_ref
(test_mlp_oracle_cpu.py) and the reasons for what exceeds it are in profiles/fused_mlp_oracle.txt."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import fused_mlp_cases as FC  # noqa: E402
from oracle import mlp_oracle as MO  # noqa: E402

# 3x the worst value measured on the MI355X, per class (profiles/fused_mlp_oracle.txt): y 1.61e-4 (inference, 256-256-128 tanh, 300 rows; the training passes
# 3.5e-5), weight gradients 3.16e-4 by norm and 5.28e-4 by element (A tanh, dW_0), bias gradients 1.00e-5 by norm and 7.50e-5 by element (D, db_0).
# The older tests' gate on the same quantities is 3e-2.
GATE = dict(y=4.8e-4, w_norm=9.5e-4, w_elem=1.6e-3, b_norm=3.0e-5, b_elem=2.25e-4)


def _record(name, **vals):
    from test_gpu_parity import _record as rec
    rec(name, **vals)


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _net(case, act, **kw):
    from smplsim_amd.learning.fused_train import FusedMLPTrain
    _, Ws, bs, _ = FC.operands(case, act)
    layers = [torch.nn.Linear(w.shape[1], w.shape[0]).cuda() for w in Ws]
    with torch.no_grad():
        for l, w, b in zip(layers, Ws, bs):
            l.weight.copy_(w)
            l.bias.copy_(b)
    return FusedMLPTrain(layers[:-1], layers[-1], act, **kw), [p for l in layers for p in (l.weight, l.bias)]


def _pass(fused, params, inp, go):
    y = fused(inp)
    g = torch.autograd.grad(y, params, grad_outputs=go)
    torch.cuda.synchronize()
    return dict(y=y.detach(), dW=list(g[0::2]), db=list(g[1::2]))


DET_TOO = [r for r in FC.RUNS if r[0] in "AB"]


@pytest.mark.parametrize("case,act,det", [(*r, False) for r in FC.RUNS] + [(*r, True) for r in DET_TOO])
def test_tracked_pass_matches_the_rounding_faithful_oracle(case, act, det):
    hidden, head, M, dx256 = FC.CASES[case]
    x, Ws, bs, go = FC.operands(case, act)
    ref = FC.reference(case, act)
    fused, params = _net(case, act, deterministic=det)
    xg, gog = x.cuda(), go.cuda()
    got = _pass(fused, params, xg, gog)
    assert fused.work.sets[M].dx256 == dx256 and fused.work.sets[M].Mp == -(-M // 128) * 128
    assert got["y"].shape == (M, head) and got["y"].dtype == torch.float32
    for a, p in zip(got["dW"] + got["db"], params[0::2] + params[1::2]):
        assert a.shape == p.shape and a.dtype == torch.float32           # (no padded column or row of the kernels' layouts)
    d = FC.distances(got, ref)
    _record(f"fused_mlp_gpu_{case}_{act}_{'det' if det else 'default'}", **d)
    for k, v in d.items():
        assert max(v) <= GATE[k], (k, v, GATE[k])
    with torch.no_grad():                                               # GAE's value pass: no derivative written, the same result
        y0 = fused(xg)
    assert y0.shape == (M, head) and torch.equal(_bits(y0), _bits(got["y"]))


@pytest.mark.parametrize("case", ["A", "B"])
def test_weight_images_and_operand_passes_are_the_plain_pass_bit_for_bit(case):
    """deterministic=True at the shapes that take the 256 x 256 dX kernel (test_norm_gpu has the operand at 200 rows, test_optim_gpu the images through an
    agent): the values are the plain pass's, so its comparison with the oracle above covers them."""
    x, _, _, go = FC.operands(case, "silu")
    xg, gog = x.cuda(), go.cuda()
    plain, p0 = _net(case, "silu", deterministic=True)
    want = _pass(plain, p0, xg, gog)
    imaged, p1 = _net(case, "silu", deterministic=True, weight_images=True)
    for name, fused, params, inp in (("images", imaged, p1, xg), ("operand", plain, p0, plain.operand(xg)), ("both", imaged, p1, imaged.operand(xg))):
        got = _pass(fused, params, inp, gog)
        for a, b in zip([got["y"]] + got["dW"] + got["db"], [want["y"]] + want["dW"] + want["db"]):
            assert a.abs().sum() > 0 and torch.equal(_bits(a), _bits(b)), (name, tuple(a.shape))


@pytest.mark.parametrize("hidden,act", FC.INFER)
def test_policy_inference_mean_matches_the_oracles_forward(hidden, act):
    """FusedPolicyInference.mean on observations in a strided view, without statistics (n = 0) and with them, against forward_only on the operand
    ss_obs_to_bf16 itself writes into a buffer of this test (that kernel's bits: test_obs_to_bf16_rounding_normalisation_and_padding), so the
    normaliser's one-ulp latitude stays out of the chain's comparison.  rows_off (recorded): the rows further than 1e-6 from the oracle, those in
    which an activation was rounded to the other bf16 neighbour (profiles/fused_mlp_oracle.txt)."""
    import copy

    from smplsim_amd._lib import lib
    from smplsim_amd.learning.fast_policy import FusedPolicyInference
    p = lambda t: C.c_void_p(t.data_ptr())
    dist, rows_off = [], []
    for normed in (False, True):
        cpu_policy, obs_by_m = FC.policy_case(hidden, act, normed)
        policy = copy.deepcopy(cpu_policy).cuda()
        layers = list(policy.net.affine_layers) + [policy.action_mean]
        Ws, bs = [l.weight.detach() for l in layers], [l.bias.detach() for l in layers]
        inf = FusedPolicyInference(policy)
        nm, kp = policy.norm, inf.kpad[0]
        for M in FC.INFER_M:
            obs = obs_by_m[M].cuda()[:, FC.OBS_OFF:FC.OBS_OFF + FC.D]
            assert obs.stride() == (FC.OBS_STRIDE, 1)
            y = inf.mean(obs)
            assert y.shape == (M, 69) and y.dtype == torch.float32
            op = torch.full((M, kp), -768.0, dtype=torch.bfloat16, device="cuda")
            assert lib().ss_obs_to_bf16(p(obs), M, FC.D, FC.OBS_STRIDE, p(nm.mean), p(nm.std), p(nm.n), -5.0, 5.0, 5.0, p(op), kp,
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
            torch.cuda.synchronize()
            opc, clamped = op.cpu(), obs.cpu().clamp(-5.0, 5.0).to(torch.bfloat16)
            assert (opc[:, FC.D:] == 0).all() and torch.equal(opc[:, :FC.D], clamped) == (not normed)   # (the statistics are in use when they should be)
            ref = MO.forward_only(opc, Ws, bs, act)
            d = y.cpu().double() - ref
            dist.append((d.norm() / ref.norm()).item())
            rows_off.append(int((d.norm(dim=1) > 1e-6 * ref.norm(dim=1)).sum()))
    _record(f"fused_mlp_gpu_inference_{'x'.join(map(str, hidden))}_{act}", y=dist, rows_off=rows_off)
    assert max(dist) <= GATE["y"], dist

