"""The deterministic form of the PPO update's reductions (include/smplsim_mlp.h: ss_wgrad_bf16_det, ss_linear_bf16_dx_det; FusedMLPTrain(deterministic=True);
PPOConfig.deterministic_update): the reduce pass is exactly the sum the header states (bit for bit, from the partials the product leaves in the workspace),
every partial is the right number (float64 reference, the element-wise bounds of test_gemm_kernels_gpu.py), the results do not change from call to call while
a second stream keeps the device busy, and two agents with the same seed end an update with the same bits."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from test_gemm_kernels_gpu import (C_ACC, DISPATCH_MAP, U, Ref, _g256, _launch_zero, _lib, _operands, _p, _record, _st, check_out, check_untouched,  # noqa: E402
                                   last_gemm, out_buf)

NAN_MARGIN = 4096            # floats of workspace beyond the documented size: they must keep their NaN


def _bits(t):
    return t.contiguous().view(torch.int32)


def _nan_ws(nbytes):
    assert nbytes > 0 and nbytes % 4 == 0
    return torch.full((nbytes // 4 + NAN_MARGIN,), float("nan"), dtype=torch.float32, device="cuda")


def _fold(parts):
    """((p0 + p1) + p2) + ... with fp32 torch additions, in that order."""
    s = parts[0].clone()
    for k in range(1, parts.shape[0]):
        s = s + parts[k]
    return s


def _shares(desc):
    return int(desc.split("ksplit=")[1].split()[0]), int(desc.split("kper=")[1].split()[0])


def _wgrad_desc(S, kper, out="f32det"):
    return f"wgrad mode=- bn=256 bk=64 waves=8 out={out} ksplit={S} kper={kper}"


def _wgrad_operands(Mb, n_out, n_in, ldz, ldh, seed):
    """dz [Mb, ldz], h [Mb, ldh] bf16 as in the default entry's test: the columns beyond n_out / n_in hold NaN and Inf."""
    g = torch.Generator().manual_seed(seed)
    dz = torch.randn(Mb, ldz, generator=g) + torch.linspace(-1, 1, ldz)[None, :] * 0.3
    h = torch.randn(Mb, ldh, generator=g) + torch.linspace(1, -1, Mb)[:, None] * 0.3
    dz[:, n_out:] = float("nan"); dz[::2, n_out:] = float("inf")
    h[:, n_in:] = float("-inf"); h[1::3, n_in:] = float("nan")
    prior = torch.randn(n_out, n_in, generator=g)
    return dz.to(torch.bfloat16).cuda(), h.to(torch.bfloat16).cuda(), prior.cuda()


# ---------------------------------------------------------------------------------------------------------------- 1, 2: the weight gradient
@pytest.mark.parametrize("Mb,n_out,n_in,ldz,ldh,ldw,want", [
    (128, 72, 136, 80, 144, 139, (1, 2)),                # one share
    (3200, 72, 136, 80, 144, 139, (5, 10)),              # five shares of ten K tiles
    (1024, 264, 520, 272, 528, 523, (2, 8))])            # 2 x 3 output tiles, ragged in both directions, ldw > n_in
def test_wgrad_det_is_the_stated_sum_of_the_right_partials(Mb, n_out, n_in, ldz, ldh, ldw, want):
    """dw == dw_in + (((p0 + p1) + p2) + ...) bit for bit, with p_s read back from the workspace; p_s is the product over the rows of share s (float64
    reference, C_ACC bound with K = the share's rows); dw against the product of all rows with the default entry's bound; the padding of dw keeps its
    sentinel; the workspace started as NaN and none reaches dw; nothing is written beyond S * n_out * n_in floats of it."""
    dz, h, prior = _wgrad_operands(Mb, n_out, n_in, ldz, ldh, Mb + n_out)
    L, st = _lib(), _st()
    need = L.ss_wgrad_bf16_det_workspace(Mb, n_out, n_in)
    assert need == want[0] * n_out * n_in * 4
    ws = _nan_ws(need)
    flat, full = out_buf(n_out, n_in, ldw, torch.float32, 0)
    full[:, :n_in] = prior
    assert L.ss_wgrad_bf16_det(_p(dz), _p(h), _p(full), Mb, n_out, n_in, ldz, ldh, ldw, _p(ws), need, st) == 0, L.ss_last_error()
    desc = last_gemm()
    assert desc == _wgrad_desc(*want)
    S, kper = _shares(desc)
    torch.cuda.synchronize()
    check_untouched(flat, full, n_in, 0)
    assert torch.isnan(ws[S * n_out * n_in:]).all(), "a write beyond the documented workspace"
    parts = ws[:S * n_out * n_in].view(S, n_out, n_in)
    assert not torch.isnan(parts).any() and not torch.isnan(full[:, :n_in]).any()
    expect = prior + _fold(parts)
    assert torch.equal(_bits(full[:, :n_in]), _bits(expect)), int((_bits(full[:, :n_in]) != _bits(expect)).sum())
    a, hh = dz[:, :n_out].double(), h[:, :n_in].double()
    for s in range(S):
        r0, r1 = s * kper * 64, min((s + 1) * kper * 64, Mb)
        assert r1 > r0
        z = a[r0:r1].T @ hh[r0:r1]
        e = C_ACC * U * (r1 - r0) * (a[r0:r1].abs().T @ hh[r0:r1].abs())
        check_out(parts[s], z, e, "none", False, "wgrad_det_part", f" share {s}")
    z = prior.double() + a.T @ hh
    e = C_ACC * U * (Mb * (a.abs().T @ hh.abs()) + prior.double().abs())
    check_out(full[:, :n_in], z, e, "none", False, "wgrad_det")


# ---------------------------------------------------------------------------------------------------------------- 1, 2: the column sums
def _dx_operands(M, N, K, ldy, seed):
    x, w, _ = _operands(M, N, K, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    mulbuf = torch.full((M, ldy), float("nan"), dtype=torch.bfloat16)
    mulbuf[:, :N] = torch.rand(M, N, generator=g) + 0.5
    prior = torch.randn(N, generator=g) * 10
    return x, w, mulbuf.cuda(), prior.cuda()


@pytest.mark.parametrize("M,N,K,ldy", [(2049, 300, 384, 304), (4100, 1024, 640, 1024)])
def test_dx_det_column_sums_are_the_stated_sum_and_y_is_unchanged(M, N, K, ldy):
    """colsum == colsum_in + (((P0 + P1) + P2) + ...) bit for bit with the 2 * ceil(M / 256) partial rows read back from the workspace; each partial row is
    the column sum of its 128 rows (float64), rows beyond M count zero; y is bit-identical to ss_linear_bf16_dx's; NaN in the workspace and in the padding
    of mul reaches nothing."""
    x, w, mulbuf, prior = _dx_operands(M, N, K, ldy, 5)
    ref = Ref(x, w)
    z, e = ref.pre(None, mulbuf[:, :N])
    L, st = _lib(), _st()
    flat0, y0 = out_buf(M, N, ldy, torch.bfloat16, 0)
    cs0 = prior.clone()
    assert L.ss_linear_bf16_dx(_p(x), _p(w), _p(mulbuf), _p(y0), _p(cs0), M, N, K, ldy, st) == 0
    assert last_gemm() == _g256("DXN")
    P = 2 * ((M + 255) // 256)
    need = L.ss_linear_bf16_dx_det_workspace(M, N, K)
    assert need == P * N * 4
    ws = _nan_ws(need)
    flat1, y1 = out_buf(M, N, ldy, torch.bfloat16, 0)
    cs = torch.full((N + 64,), -12345.0, dtype=torch.float32, device="cuda")
    cs[:N] = prior
    assert L.ss_linear_bf16_dx_det(_p(x), _p(w), _p(mulbuf), _p(y1), _p(cs), M, N, K, ldy, _p(ws), need, st) == 0, L.ss_last_error()
    assert last_gemm() == _g256("DXN") + " colsum=det"
    torch.cuda.synchronize()
    check_untouched(flat1, y1, N, 0)
    assert torch.equal(flat0.view(torch.int16), flat1.view(torch.int16)), "y differs from the default entry's"
    assert (cs[N:] == -12345.0).all()
    assert torch.isnan(ws[P * N:]).all(), "a write beyond the documented workspace"
    parts = ws[:P * N].view(P, N)
    assert not torch.isnan(parts).any() and not torch.isnan(cs[:N]).any()
    expect = prior + _fold(parts)
    assert torch.equal(_bits(cs[:N]), _bits(expect)), int((_bits(cs[:N]) != _bits(expect)).sum())
    # each partial row: the rows' own error E, plus fp32 additions of depth 64 (a lane's rows) + 1 (its partner)
    worst = 0.0
    for p in range(P):
        r0, r1 = 128 * p, min(128 * p + 128, M)
        if r1 <= r0:
            assert (parts[p] == 0).all(), p
            continue
        ref_p = z[r0:r1].sum(0)
        bound = e[r0:r1].sum(0) + 65 * U * z[r0:r1].abs().sum(0)
        err = (parts[p].double() - ref_p).abs()
        assert (err <= bound).all(), (p, (err / bound).max().item())
        worst = max(worst, (err / bound.clamp_min(1e-300)).max().item())
    _record(f"det_colsum_part_{M}", ratio=worst)
    depth = 64 + 1 + P
    csr = prior.double() + z.sum(0)
    bound = e.sum(0) + depth * U * (z.abs().sum(0) + prior.double().abs())
    err = (cs[:N].double() - csr).abs()
    assert (err <= bound).all(), (err / bound).max().item()


# ---------------------------------------------------------------------------------------------------------------- 3: disturbed scheduling
SIDE_SHAPES = [(512, 512, 512), (4096, 1024, 512), (1000, 256, 1024), (8192, 2048, 512), (300, 64, 320), (2048, 1536, 576)]


class _Disturbance:
    """Unrelated ss_linear_bf16 launches of varying size on a second stream, a few before every call under test: the two queues stay full, so the
    workgroups of the call under test share the CUs with a different neighbour every time."""

    def __init__(self):
        self.stream = torch.cuda.Stream()
        self.ops = []
        for i, (M, N, K) in enumerate(SIDE_SHAPES):
            x, w, b = _operands(M, N, K, seed=100 + i)
            self.ops.append((x, w, b, torch.empty(M, N, dtype=torch.bfloat16, device="cuda"), M, N, K))
        self.i = 0
        torch.cuda.synchronize()

    def kick(self, n=3):
        L, st = _lib(), C.c_void_p(self.stream.cuda_stream)
        for _ in range(n):
            x, w, b, y, M, N, K = self.ops[self.i % len(self.ops)]
            self.i += 1 + (self.i % 3 == 0)                                     # an irregular walk over the shapes
            assert L.ss_linear_bf16(_p(x), _p(w), _p(b), _p(y), M, N, K, N, 1, 0, st) == 0


def _count_differing(outs):
    return sum(int(not torch.equal(_bits(o), _bits(outs[0]))) for o in outs[1:])


def test_wgrad_det_is_invariant_under_disturbed_scheduling():
    """Mb = 8192, 256 x 256: one output tile, 16 shares.  20 calls of ss_wgrad_bf16_det on the same inputs, a second stream busy meanwhile: 20 identical
    results.  The default entry under the same disturbance is recorded (how many of its 20 results differ from the first), not asserted."""
    Mb, n = 8192, 256
    dz, h, prior = _wgrad_operands(Mb, n, n, n, n, 11)
    L, st = _lib(), _st()
    need = L.ss_wgrad_bf16_det_workspace(Mb, n, n)
    ws = _nan_ws(need)
    side = _Disturbance()
    outs = [prior.clone() for _ in range(20)]
    for o in outs:
        side.kick()
        assert L.ss_wgrad_bf16_det(_p(dz), _p(h), _p(o), Mb, n, n, n, n, n, _p(ws), need, st) == 0
        assert last_gemm() == _wgrad_desc(16, 8)                                # (per host thread: the side launches overwrite it)
    torch.cuda.synchronize()
    assert _count_differing(outs) == 0
    ctrl = [prior.clone() for _ in range(20)]
    for o in ctrl:
        side.kick()
        assert L.ss_wgrad_bf16(_p(dz), _p(h), _p(o), Mb, n, n, n, n, n, st) == 0
        assert last_gemm() == _wgrad_desc(16, 8, "f32acc")
    torch.cuda.synchronize()
    _record("det_control_wgrad", differing=_count_differing(ctrl), calls=20)


def test_dx_det_is_invariant_under_disturbed_scheduling():
    """M = 4100 (17 row tiles, 34 partial rows), N = 1024, K = 640: 20 calls of ss_linear_bf16_dx_det, a second stream busy meanwhile: colsum and y
    identical in all 20.  The default entry's column sums under the same disturbance are recorded, not asserted."""
    M, N, K = 4100, 1024, 640
    x, w, mulbuf, prior = _dx_operands(M, N, K, N, 21)
    L, st = _lib(), _st()
    need = L.ss_linear_bf16_dx_det_workspace(M, N, K)
    ws = _nan_ws(need)
    side = _Disturbance()
    cols = [prior.clone() for _ in range(20)]
    ys = [torch.empty(M, N, dtype=torch.bfloat16, device="cuda") for _ in range(20)]
    for c, y in zip(cols, ys):
        side.kick()
        assert L.ss_linear_bf16_dx_det(_p(x), _p(w), _p(mulbuf), _p(y), _p(c), M, N, K, N, _p(ws), need, st) == 0
        assert last_gemm() == _g256("DXN") + " colsum=det"
    torch.cuda.synchronize()
    assert _count_differing(cols) == 0
    assert all(torch.equal(y.view(torch.int16), ys[0].view(torch.int16)) for y in ys[1:])
    ctrl = [prior.clone() for _ in range(20)]
    for c, y in zip(ctrl, ys):
        side.kick()
        assert L.ss_linear_bf16_dx(_p(x), _p(w), _p(mulbuf), _p(y), _p(c), M, N, K, N, st) == 0
        assert last_gemm() == _g256("DXN")
    torch.cuda.synchronize()
    _record("det_control_colsum", differing=_count_differing(ctrl), calls=20)


# ---------------------------------------------------------------------------------------------------------------- 4: FusedMLPTrain(deterministic=True)
FUSED_REL = 3e-2             # the bound of the existing autograd comparison; both modes add the same fp32 partial sums in a different order


@pytest.mark.parametrize("hidden,M", [((512, 256, 256), 1000), (None, 4100)])
@pytest.mark.parametrize("out_dim", [69, 1])
def test_fused_mlp_train_deterministic_is_reproducible_and_close_to_the_default(hidden, M, out_dim):
    """FusedMLPTrain(deterministic=True) at (512, 256, 256) with 1000 rows (Mp = 1024: weight gradients of two shares, bias gradients by torch) and at the
    production widths with 4100 rows (every _det entry): forward + backward twice, and once more through a second object with its own workspace, every
    gradient bit-identical; against deterministic=False every gradient within FUSED_REL by relative norm.  Measured on the MI355X: 0 at the small
    widths (two shares added to zero commute), 6.2e-8 .. 4.3e-7 at the production widths."""
    from smplsim_amd.agents.ppo import PPOConfig
    from smplsim_amd.learning.fused_train import FusedMLPTrain
    from smplsim_amd.learning.networks import MLP
    hidden = hidden or PPOConfig().hidden
    torch.manual_seed(out_dim + M)
    net = MLP(289, hidden, "silu").cuda()
    head = torch.nn.Linear(hidden[-1], out_dim).cuda()
    params = [p for l in list(net.affine_layers) + [head] for p in (l.weight, l.bias)]
    x = torch.randn(M, 289, device="cuda") * 2
    target = torch.randn(M, out_dim, device="cuda")

    def grads(fused):
        y = fused(x)
        return [g.clone() for g in torch.autograd.grad((y * target).sum(), params)]

    det = FusedMLPTrain(net.affine_layers, head, "silu", deterministic=True)
    g1, g2 = grads(det), grads(det)
    again = grads(FusedMLPTrain(net.affine_layers, head, "silu", deterministic=True))       # a second object: its own (zero-filled) workspace
    for i, (a, b, c) in enumerate(zip(g1, g2, again)):
        assert torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(a), _bits(c)), (i, tuple(a.shape))
    g0 = grads(FusedMLPTrain(net.affine_layers, head, "silu"))
    rels = [((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300)).item() for a, b in zip(g1, g0)]
    _record(f"det_fused_vs_default_{len(hidden)}x{M}_{out_dim}", rel_grads=rels)
    for i, r in enumerate(rels):
        assert r < FUSED_REL, (i, tuple(params[i].shape), r)


def test_fused_mlp_train_gradients_of_a_shorter_batch_do_not_take_in_the_longer_ones_rows():
    """One FusedMLPTrain(deterministic=True) object at (512, 256, 256), heads of 69 and of 1: gradients at 1000 rows, then on x[:900] — the same 1024 padded rows, and
    every weight gradient contracts over all of them.  The second pass's gradients are bit-identical to those of a fresh object that only ever saw x[:900]: the
    work tensors of a pass belong to its exact row count, so rows 900..999 of the first pass's operand and dZ reach nothing."""
    from smplsim_amd.learning.fused_train import FusedMLPTrain
    from smplsim_amd.learning.networks import MLP
    for out_dim in (69, 1):
        torch.manual_seed(out_dim)
        net = MLP(289, (512, 256, 256), "silu").cuda()
        head = torch.nn.Linear(256, out_dim).cuda()
        params = [p for l in list(net.affine_layers) + [head] for p in (l.weight, l.bias)]
        x = torch.randn(1000, 289, device="cuda") * 2
        target = torch.randn(1000, out_dim, device="cuda")

        def grads(fused, M):
            return [g.clone() for g in torch.autograd.grad((fused(x[:M]) * target[:M]).sum(), params)]

        used = FusedMLPTrain(net.affine_layers, head, "silu", deterministic=True)
        grads(used, 1000)
        got, want = grads(used, 900), grads(FusedMLPTrain(net.affine_layers, head, "silu", deterministic=True), 900)
        for i, (a, b) in enumerate(zip(got, want)):
            assert torch.equal(_bits(a), _bits(b)), (out_dim, i, tuple(a.shape), float((a - b).abs().max()))


# ---------------------------------------------------------------------------------------------------------------- 5: end to end
def _agent_state(agent):
    out = {}
    for name, net in (("policy", agent.policy_net), ("value", agent.value_net)):
        for k, v in net.state_dict().items():
            out[f"{name}.{k}"] = v
    for name, opt in (("opt_policy", agent.optimizer_policy), ("opt_value", agent.optimizer_value)):
        for i, (p, st) in enumerate(opt.state.items()):
            for k, v in st.items():
                if torch.is_tensor(v):
                    out[f"{name}.{i}.{k}"] = v
    return out


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


def test_two_agents_with_one_seed_end_an_update_with_the_same_bits():
    """PPOConfig(mfma_update=True, deterministic_update=True): two agents built with the same seed get clones of one rollout; after update_params every
    parameter and buffer of both networks (the RunningNorm statistics among them) and every moment tensor of both optimisers is bit-identical.  A second
    update on a second shared rollout repeats the comparison with a non-zero Adam state."""
    from smplsim_amd.agents.ppo import AgentPPO, PPOConfig
    from smplsim_amd.batch import SMPLSimVecEnv
    env = SMPLSimVecEnv(256, task="HumanoidSpeed", autoreset=True, seed=3)
    cfg = dict(mfma_update=True, deterministic_update=True, hidden=(256, 128, 128), min_batch_size=2048, opt_num_epochs=2)
    a, b = AgentPPO(env, PPOConfig(**cfg), seed=1), AgentPPO(env, PPOConfig(**cfg), seed=1)
    assert a.fused_policy.deterministic and a.fused_value.deterministic and b.fused_policy.deterministic
    sa, sb = _agent_state(a), _agent_state(b)
    assert all(_same_bits(sa[k], sb[k]) for k in sa)
    for round_ in range(2):
        batch = a.sample()
        a.update_params({k: v.clone() for k, v in batch.items()})
        b.update_params({k: v.clone() for k, v in batch.items()})
        torch.cuda.synchronize()
        sa, sb = _agent_state(a), _agent_state(b)
        assert sa.keys() == sb.keys()
        assert {"policy.norm.mean", "policy.norm.var", "policy.norm.std", "policy.norm.n"} <= set(sa)
        assert any(k.startswith("opt_policy.") and k.endswith("exp_avg_sq") for k in sa) and any(k.startswith("opt_value.") for k in sa)
        differing = [k for k in sa if not _same_bits(sa[k], sb[k])]
        assert not differing, (round_, differing)


# ---------------------------------------------------------------------------------------------------------------- 6: dispatch
def test_det_entries_report_their_gemm_and_the_default_entries_what_they_did():
    L, st = _lib(), _st()
    z = lambda *s, dt=torch.bfloat16: torch.zeros(*s, dtype=dt, device="cuda")
    for entry, args, expect in DISPATCH_MAP:
        if entry == "wgrad":
            Mb, no, ni = args
            need = L.ss_wgrad_bf16_det_workspace(Mb, no, ni)
            ws = _nan_ws(need)
            assert L.ss_wgrad_bf16_det(_p(z(Mb, no)), _p(z(Mb, ni)), _p(z(no, ni, dt=torch.float32)), Mb, no, ni, no, ni, ni, _p(ws), need, st) == 0
            assert last_gemm() == expect.replace("out=f32acc", "out=f32det")
        elif entry == "dx":
            M, N, K = args
            need = L.ss_linear_bf16_dx_det_workspace(M, N, K)
            ws = _nan_ws(need)
            assert L.ss_linear_bf16_dx_det(_p(z(M, K)), _p(z(N, K)), _p(z(M, N)), _p(z(M, N)), _p(z(N, dt=torch.float32)), M, N, K, N, _p(ws), need, st) == 0
            assert last_gemm() == expect + " colsum=det"
        else:
            continue
        assert _launch_zero(entry, args) == 0 and last_gemm() == expect, (entry, args)
    torch.cuda.synchronize()
