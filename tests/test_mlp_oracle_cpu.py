"""oracle/mlp_oracle.py on its own (no GPU, nothing of smplsim_amd.learning): its chain rule against torch's fp64 autograd with the rounding off;
its own accumulation noise E_ref (fp32 against fp64 products over the same roundings) on the cases of test_fused_mlp_gpu.py, recorded for
profiles/fused_mlp_oracle.txt; and what the gates of test_fused_mlp_gpu.py can tell apart: a dropped and a doubled batch row."""
import pytest

torch = pytest.importorskip("torch")

import fused_mlp_cases as FC  # noqa: E402
from oracle import mlp_oracle as MO  # noqa: E402

OLD_GATE = 3e-2                                                         # test_gpu_parity / test_gemm_kernels_gpu: FUSED_REL


def _record(name, **vals):
    from test_gpu_parity import _record as rec
    rec(name, **vals)


def test_rb_is_two_nearest_even_roundings():
    one = 1.0 + 2.0 ** -8                                               # halfway between 1 and 1 + 2^-7
    v = torch.tensor([one, 1.0 + 3 * 2.0 ** -8, one + 2.0 ** -40, -(one + 2.0 ** -20), 0.1, -0.0], dtype=torch.float64)
    # one + 2^-40 is above the bf16 tie in fp64, ON it after the fp32 rounding: the kernels see fp32, so it goes to even
    want = torch.tensor([1.0, 1.0 + 2.0 ** -6, 1.0, -(1.0 + 2.0 ** -7), 0.10009765625, -0.0], dtype=torch.float64)
    assert torch.equal(MO.rb(v), want)


def _autograd64(x, Ws, bs, go, act):
    p = [t.double().requires_grad_(True) for pair in zip(Ws, bs) for t in pair]
    h = x.double()
    for i in range(len(Ws)):
        z = h @ p[2 * i].T + p[2 * i + 1]
        h = {"silu": torch.nn.functional.silu, "tanh": torch.tanh, "relu": torch.relu}[act](z) if i < len(Ws) - 1 else z
    g = torch.autograd.grad(h, p, grad_outputs=go.double())
    return h.detach(), g[0::2], g[1::2]


@pytest.mark.parametrize("act", MO.ACTS)
@pytest.mark.parametrize("case", ["A", "B", "E"])
def test_unrounded_oracle_is_fp64_autograd(case, act):
    """round=False: y and every gradient equal torch's fp64 autograd over the same layers to 1e-12, with every dx256 entry off and on (the two bias
    paths are the same sums once nothing is rounded) — heads of 69 (A) and 1 (B; E: one row), all three activations."""
    x, Ws, bs, go = FC.operands(case, act)
    y, gw, gb = _autograd64(x, Ws, bs, go, act)
    nl = len(Ws)
    for bits in range(2 ** (nl - 1)):
        dx256 = [False] + [bool(bits >> k & 1) for k in range(nl - 1)]
        o = MO.train_pass(x, Ws, bs, go, act, dx256, round=False)
        assert o["y"].shape == y.shape and (o["y"] - y).norm() <= 1e-12 * y.norm()
        for a, b in zip(o["dW"] + o["db"], list(gw) + list(gb)):
            assert a.shape == b.shape and (a - b).norm() <= 1e-12 * b.norm(), (case, act, dx256, tuple(b.shape))
    fo = MO.forward_only(MO.rb(x.double()), Ws, bs, act)               # the inference chain is the training forward
    assert torch.equal(fo, MO.train_pass(x, Ws, bs, go, act, [False] * nl)["y"])


@pytest.mark.parametrize("case,act", FC.RUNS)
def test_record_the_oracles_own_accumulation_noise(case, act):
    """E_ref: the rounding-faithful pass with fp32 products and sums against the same with fp64 ones, per tensor.  Recorded, and bounded only by what
    the old gate allows (were the oracle's own noise near 3e-2, it would be no sharper than the tests it supplements)."""
    e = FC.distances(FC.reference(case, act, "fp32"), FC.reference(case, act))
    _record(f"fused_mlp_eref_{case}_{act}", **e)
    assert max(max(v) for v in e.values()) < OLD_GATE / 5, e


@pytest.mark.parametrize("hidden,act", FC.INFER)
def test_record_the_inference_chains_own_accumulation_noise(hidden, act):
    """E_ref of forward_only on the inference cases (the operand by torch's expression of the normaliser: a noise estimate needs the distribution, not
    the bits).  rows_off: the rows further than 1e-6 apart — those in which the two accumulations rounded an activation to different bf16 neighbours."""
    dist, rows_off = [], []
    for normed in (False, True):
        policy, obs_by_m = FC.policy_case(hidden, act, normed)
        layers = list(policy.net.affine_layers) + [policy.action_mean]
        Ws, bs = [l.weight.detach() for l in layers], [l.bias.detach() for l in layers]
        for M in FC.INFER_M:
            with torch.no_grad():
                op = policy.norm(obs_by_m[M][:, FC.OBS_OFF:FC.OBS_OFF + FC.D].clamp(-5.0, 5.0)).to(torch.bfloat16)
            a, b = MO.forward_only(op, Ws, bs, act, "fp32"), MO.forward_only(op, Ws, bs, act)
            dist.append(((a - b).norm() / b.norm()).item())
            rows_off.append(int(((a - b).norm(dim=1) > 1e-6 * b.norm(dim=1)).sum()))
    _record(f"fused_mlp_eref_inference_{'x'.join(map(str, hidden))}_{act}", y=dist, rows_off=rows_off)
    assert max(dist) < OLD_GATE / 5, dist


def _mutants(act):
    x, Ws, bs, go = FC.operands("A", act)
    dx256 = FC.CASES["A"][3]
    rows = torch.cat([torch.arange(len(x)), torch.tensor([len(x) - 1])])
    return dict(m1=MO.train_pass(x[:-1], Ws, bs, go[:-1], act, dx256),   # batch row M - 1 is in no dW and no db (rows are independent: the pass without it)
                m2=MO.train_pass(x[rows], Ws, bs, go[rows], act, dx256))  # row M - 1 of dz_L counted twice, as a stale pad row would be: the pass with it twice


@pytest.mark.parametrize("act", MO.ACTS)
def test_the_gate_sees_a_dropped_and_a_doubled_batch_row(act):
    """Case A, mutated two ways (_mutants): each must differ from the oracle by MORE than test_fused_mlp_gpu's weight-gradient gate in at least one weight
    gradient (measured: every one of them, by 8x to 33x), whatever the activation.  Under silu, the only activation the 3e-2 tests run, every weight
    gradient of both also stays UNDER 3e-2 (0.7e-2 .. 1.2e-2): what that gate lets through.  (One row's share depends on the row: under tanh
    the same row moves dW_1 by 3.1e-2, the other three by 1.7e-2 .. 2.7e-2; under relu 1.1e-2 .. 1.4e-2.  Removing a row and adding it a
    second time move a sum by the same amount, so the two mutants measure the same.)"""
    from test_fused_mlp_gpu import GATE
    ref = FC.reference("A", act)
    for name, m in _mutants(act).items():
        d = FC.distances(dict(m, y=ref["y"]), ref)                     # (y has another row count; the mutation is in the gradients)
        _record(f"fused_mlp_mutant_{name}_{act}", w_norm=d["w_norm"], w_elem=d["w_elem"])
        assert max(d["w_norm"]) > GATE["w_norm"] and max(d["w_elem"]) > GATE["w_elem"], (name, d, GATE)
        if act == "silu":
            assert max(d["w_norm"]) < OLD_GATE, (name, d["w_norm"])
