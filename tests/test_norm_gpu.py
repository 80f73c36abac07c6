"""Train-mode RunningNorm on the GPU (include/smplsim_mlp.h: ss_running_norm_update; learning/fused_norm.py: LibRunningNorm; learning/fused_train.py: Bf16Operand;
PPOConfig.fused_norm).

The bounds against float64 follow from the header's rule "formed in fp64, rounded to fp32 once": one fp32 ulp of the reference (half an ulp of rounding, the rest for
the few 1e-16 by which two float64 evaluations differ), not from measurements.  torch's own fp32 RunningNorm.update runs on the same inputs and its error is recorded
for information (`running_norm_e32_*`)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from test_det_update_gpu import _Disturbance, _agent_state, _nan_ws, _same_bits  # noqa: E402
from test_gemm_kernels_gpu import _lib, _p, _record, _st  # noqa: E402

FACTOR = 4.0                 # test_optim_gpu.py's: a different order of operations than torch's fp32 path, not a different precision class
SENT = -12345.0              # what lies behind the dim-th element of mean / var / std: it must stay
NAN = float("nan")


def _R():
    from smplsim_amd._cabi import NORM_BLOCK_ROWS
    return NORM_BLOCK_ROWS


def _shapes():
    R = _R()
    # (M, dim, ldx, column offset inside the [M, ldx] buffer)
    return [(1, 1, 1, 0), (R - 1, 63, 63, 0), (R, 64, 64, 0), (R + 1, 65, 72, 0), (3 * R + 37, 289, 300, 5), (2 * R, 289, 289, 0)]


SHAPE_IDS = ["1x1", "R-1x63", "Rx64", "R+1x65_ld72", "3R+37x289_ld300_off5", "2Rx289"]
CONST = np.float32(0.1)


def _batch(M, dim, ldx, off, seed, lone_row):
    """x [M, dim] fp32 as a view into a NaN-filled [M, ldx] buffer: every column its own mean (up to +-5) and scale (1e-3 .. 3); with dim >= 3 column 1 is the
    constant 0.1f and column 2 is zero but for `lone_row`."""
    g = torch.Generator().manual_seed(seed)
    mean = (torch.rand(dim, generator=g) * 2 - 1) * 5
    scale = 10.0 ** (torch.rand(dim, generator=g) * (np.log10(3.0) + 3.0) - 3.0)
    x = torch.randn(M, dim, generator=g) * scale + mean
    if dim >= 3:
        x[:, 1] = float(CONST)
        x[:, 2] = 0.0
        x[lone_row % M, 2] = 2.5
    big = torch.full((M, ldx), NAN)
    big[:, off:off + dim] = x
    big = big.cuda()
    return big[:, off:off + dim]


class _State:
    """mean, var, std [dim] as the head of sentinel-filled buffers, n [1] int64: what ss_running_norm_update works on."""

    def __init__(self, dim, n=0, mean=None, var=None):
        self.buf = torch.full((3, dim + 8), SENT, device="cuda")
        self.mean, self.var, self.std = (self.buf[i, :dim] for i in range(3))
        self.mean.copy_(torch.zeros(dim) if mean is None else mean)
        self.var.copy_(torch.zeros(dim) if var is None else var)
        self.std.copy_(self.var.sqrt())
        self.n = torch.tensor([n], dtype=torch.int64, device="cuda")
        self.dim = dim

    def clone(self):
        s = _State(self.dim)
        s.buf.copy_(self.buf); s.n.copy_(self.n)
        return s

    def host(self):
        return int(self.n.item()), self.mean.double().cpu().numpy(), self.var.double().cpu().numpy(), self.std.double().cpu().numpy()

    def outputs(self):
        return [self.mean, self.var, self.std, self.n]


def _update(x, st, fill=NAN, kick=None):
    """One ss_running_norm_update call on st (in place).  Returns the partials [P, dim, 2] float64 read back from the workspace; checks the query, that nothing beyond
    the documented workspace was written and that the sentinels behind the statistics stayed."""
    L, R = _lib(), _R()
    M, dim = x.shape
    P = -(-M // R)
    need = L.ss_running_norm_workspace(M, dim)
    assert need == P * dim * 16, (need, L.ss_last_error())
    ws = _nan_ws(need)
    if fill == fill:
        ws[:need // 4] = fill
    torch.cuda.synchronize()
    if kick is not None:
        kick()
    rc = L.ss_running_norm_update(_p(x), M, dim, x.stride(0), _p(st.mean), _p(st.var), _p(st.std), _p(st.n), _p(ws), need, _st())
    assert rc == 0, L.ss_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(ws[need // 4:]).all(), "a write beyond the documented workspace"
    assert (st.buf[:, dim:] == SENT).all(), "a write beyond mean / var / std [dim]"
    return ws[:need // 4].view(torch.float64).view(P, dim, 2)


def _ulp32(ref):
    """The spacing of fp32 at |ref| (float64 array in, float64 out)."""
    return np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)


def _bits(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


# ---------------------------------------------------------------------------------------------------------------- 1: partials and merge against float64
@pytest.mark.parametrize("n0", [0, 10 ** 7])
@pytest.mark.parametrize("shape", _shapes(), ids=SHAPE_IDS)
def test_three_chained_updates_against_float64(shape, n0):
    """Three calls with different batches, each checked against oracle.ppo_oracle.running_norm_update (float64) started from the kernel's own previous output.
    Partials: the kernel adds d = x - K and d * d over at most 256 rows in fp64 (u = 1.1e-16), so its mean is off by at most (256 u * 2 + u) max|x| < 1e-13 max|x| and
    its M2 = S2 - S1^2 / rows by at most ~3 * 256 u * S2 with S2 <= 4 rows max|x|^2, i.e. < 3.4e-13 rows max|x|^2: the bound is 1e-12 (|value| + scale) with scale =
    max|x| for the mean and rows * max|x|^2 for M2, over the block's rows of that column."""
    from oracle.ppo_oracle import running_norm_update
    from smplsim_amd.learning.networks import RunningNorm
    M, dim, ldx, off = shape
    R = _R()
    g = torch.Generator().manual_seed(7 + M)
    if n0:
        mean0 = (torch.rand(dim, generator=g) * 2 - 1) * 5
        var0 = torch.rand(dim, generator=g) * 4 + 1e-4
        if dim >= 3:
            mean0[1], var0[1] = float(CONST), 0.0                     # the running statistics of a column that has always been 0.1f
        st = _State(dim, n0, mean0, var0)
    else:
        st = _State(dim)
    worst = dict(mean=[0.0, 0.0], var=[0.0, 0.0], std=[0.0, 0.0])      # [kernel, torch fp32] in fp32 ulps of the reference
    for call in range(3):
        x = _batch(M, dim, ldx, off, 100 * call + M, lone_row=0 if call == 0 else M - 1 - call)
        assert x.stride(0) == ldx and x.data_ptr() % 16 == (4 * off) % 16
        n_prev, mean_prev, var_prev, _ = st.host()
        ref_mod = RunningNorm(dim).cuda()
        ref_mod.n.fill_(n_prev); ref_mod.mean.copy_(st.mean); ref_mod.var.copy_(st.var); ref_mod.std.copy_(st.std)
        part = _update(x, st).cpu().numpy()
        x64 = x.double().cpu().numpy()
        # every partial
        for b in range(part.shape[0]):
            rows = x64[b * R:min((b + 1) * R, M)]
            bmean = rows.mean(axis=0)
            m2 = ((rows - bmean) ** 2).sum(axis=0)
            amax = np.abs(rows).max(axis=0)
            assert (np.abs(part[b, :, 0] - bmean) <= 1e-12 * (np.abs(bmean) + amax)).all(), (call, b, "mean")
            assert (np.abs(part[b, :, 1] - m2) <= 1e-12 * (np.abs(m2) + len(rows) * amax ** 2)).all(), (call, b, "M2")
            assert (part[b, :, 1] >= 0).all()
        # the merge
        n_ref, mean_ref, var_ref = running_norm_update(n_prev, mean_prev, var_prev, x64)
        n, mean, var, std = st.host()
        assert n == n_ref == n_prev + M
        bm = x64.mean(axis=0)
        e_mean = np.abs(mean - mean_ref)
        assert (e_mean <= _ulp32(mean_ref) + 1e-12 * (np.abs(mean_prev) + np.abs(bm))).all(), (call, (e_mean / _ulp32(mean_ref)).max())
        e_var = np.abs(var - var_ref)
        assert (e_var <= _ulp32(var_ref)).all(), (call, (e_var / _ulp32(var_ref)).max())
        assert (var >= 0).all()
        e_std = np.abs(std - np.sqrt(var))
        assert (e_std <= _ulp32(np.sqrt(var))).all(), (call, (e_std / _ulp32(np.sqrt(var))).max())
        if dim >= 3:
            assert var[1] == 0.0 and std[1] == 0.0 and mean[1] == float(CONST), (call, mean[1], var[1])
        # torch's fp32 update from the same state on the same batch: recorded, not asserted
        ref_mod.update(x)
        torch.cuda.synchronize()
        t32 = dict(mean=ref_mod.mean, var=ref_mod.var, std=ref_mod.std)
        refs = dict(mean=mean_ref, var=var_ref, std=np.sqrt(var_ref))
        for k, got in (("mean", mean), ("var", var), ("std", std)):
            u = _ulp32(refs[k])
            worst[k][0] = max(worst[k][0], float((np.abs(got - refs[k]) / u).max()))
            worst[k][1] = max(worst[k][1], float((np.abs(t32[k].double().cpu().numpy() - refs[k]) / u).max()))
    tag = f"running_norm_e32_{M}x{dim}_n{n0}"
    _record(tag, **worst)
    print(tag, worst)


# ---------------------------------------------------------------------------------------------------------------- 2: NaN is not hidden and stays in its column
def test_a_nan_makes_its_column_nan_and_leaves_the_others_their_bits():
    M, dim, ldx, off = _shapes()[3]
    x = _batch(M, dim, ldx, off, 5, lone_row=3)
    g = torch.Generator().manual_seed(6)
    start = _State(dim, 1000, torch.randn(dim, generator=g), torch.rand(dim, generator=g) + 0.1)
    clean = start.clone()
    _update(x, clean)
    assert all(torch.isfinite(t).all() for t in clean.outputs()[:3])
    for r, c in ((100, 7), (M - 1, 64), (0, 0)):                        # inside a block, the last row (a block of one row) in the last column, the block's K itself
        xn = x.clone()
        xn[r, c] = NAN
        st = start.clone()
        _update(xn, st)
        assert int(st.n.item()) == 1000 + M
        others = torch.ones(dim, dtype=torch.bool, device="cuda"); others[c] = False
        for name, got, want in zip(("mean", "var", "std"), st.outputs(), clean.outputs()):
            assert torch.isnan(got[c]), (r, c, name)
            assert torch.equal(_bits(got[others]), _bits(want[others])), (r, c, name)


# ---------------------------------------------------------------------------------------------------------------- 3: reproducible
def test_five_calls_give_the_same_bits_while_a_second_stream_keeps_the_device_busy():
    M, dim, ldx, off = _shapes()[4]
    x = _batch(M, dim, ldx, off, 8, lone_row=17)
    g = torch.Generator().manual_seed(9)
    start = _State(dim, 53248, torch.randn(dim, generator=g), torch.rand(dim, generator=g) + 0.1)
    side = _Disturbance()
    first = None
    for i in range(5):
        st = start.clone()
        part = _update(x, st, fill=[NAN, 1.0, 0.0][i % 3], kick=side.kick)
        out = st.outputs() + [part]
        if first is None:
            first = [t.clone() for t in out]
            assert all(torch.isfinite(t).all() for t in out[:3])
            continue
        differing = [j for j, (a, b) in enumerate(zip(out, first)) if not torch.equal(_bits(a), _bits(b))]
        assert not differing, (i, differing)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- 4: LibRunningNorm
def test_lib_running_norm_updates_the_modules_buffers_and_fills_a_persistent_padded_operand():
    from smplsim_amd.learning.fused_norm import LibRunningNorm
    from smplsim_amd.learning.fused_train import Bf16Operand
    from smplsim_amd.learning.networks import RunningNorm
    M, dim, clip = 300, 45, 3.0
    mod = RunningNorm(dim, clip=clip).cuda()
    norm = LibRunningNorm(mod)
    xs = [_batch(M, dim, 50, 3, 20 + i, lone_row=i) for i in range(2)]

    def state():
        return [t.clone() for t in (mod.mean, mod.var, mod.std, mod.n)]

    def check_operand(op, x):
        assert isinstance(op, Bf16Operand) and (op.M, op.D) == (M, dim)
        t = op.t
        assert t.dtype == torch.bfloat16 and tuple(t.shape) == (384, 128) and t.is_contiguous()
        assert (t[:, dim:].view(torch.int16) == 0).all() and (t[M:].view(torch.int16) == 0).all()           # the padding: +0.0
        if int(mod.n.item()) == 0:
            want = x
        else:
            want = torch.clamp((x - mod.mean) / (mod.std + 1e-8), -clip, clip)                                 # in fp32 torch, with the kernel's statistics
        ulp = 2.0 ** (torch.floor(torch.log2(want.abs().clamp_min(2.0 ** -126))) - 7)
        assert ((t[:M, :dim].float() - want).abs() <= ulp).all()

    # eval mode before any update: the statistics stay, the operand is x itself (n == 0)
    mod.eval()
    before = state()
    op0 = norm(xs[0])
    torch.cuda.synchronize()
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(state(), before)) and int(mod.n.item()) == 0
    check_operand(op0, xs[0])
    assert torch.equal(op0.t[:M, :dim].view(torch.int16), xs[0].to(torch.bfloat16).view(torch.int16))
    # train mode: the buffers are a direct C call's, twice (from n = 0 and from n = M)
    mod.train()
    for i, x in enumerate(xs):
        direct = _State(dim, int(mod.n.item()), mod.mean.cpu(), mod.var.cpu())
        direct.std.copy_(mod.std)
        _update(x, direct)
        op = norm(x)
        torch.cuda.synchronize()
        assert int(mod.n.item()) == (i + 1) * M
        for a, b in zip((mod.mean, mod.var, mod.std, mod.n.reshape(1)), direct.outputs()):
            assert torch.equal(_bits(a), _bits(b)), i
        assert op.t is op0.t                                                                                  # the buffer is persistent
        check_operand(op, x)
    # eval mode: the buffers do not change, the operand follows them
    mod.eval()
    before = state()
    op = norm(xs[0])
    torch.cuda.synchronize()
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(state(), before))
    assert op.t is op0.t
    check_operand(op, xs[0])
    with pytest.raises(ValueError, match="fp32"):
        norm(xs[0][:, :dim - 1])
    with pytest.raises(ValueError, match="fp32"):
        norm(xs[0].double())


# ---------------------------------------------------------------------------------------------------------------- 5: Bf16Operand
def test_a_pass_over_its_own_operand_is_the_pass_over_the_fp32_input_bit_for_bit():
    from smplsim_amd.learning.fused_train import Bf16Operand, FusedMLPTrain
    from smplsim_amd.learning.networks import MLP
    torch.manual_seed(3)
    M, D = 200, 45
    mlp = MLP(D, (64, 64), "silu").cuda()
    head = torch.nn.Linear(64, 3).cuda()
    params = [p for l in list(mlp.affine_layers) + [head] for p in (l.weight, l.bias)]
    net = FusedMLPTrain(mlp.affine_layers, head, "silu", deterministic=True)
    x = torch.randn(M, D, device="cuda") * 2

    def run(inp):
        for p in params:
            p.grad = None
        out = net(inp)
        out.square().sum().backward()
        torch.cuda.synchronize()
        return out.detach().clone(), [p.grad.clone() for p in params]

    out0, g0 = run(x)
    op = net.operand(x)
    assert isinstance(op, Bf16Operand) and (op.M, op.D) == (M, D) and tuple(op.t.shape) == (256, 128) and op.t.dtype == torch.bfloat16
    assert (op.t[:, D:].view(torch.int16) == 0).all() and (op.t[M:].view(torch.int16) == 0).all()
    kept = op.t.clone()
    for _ in range(2):                                                  # (the second pass: the work tensors of the first are reused)
        out1, g1 = run(op)
        assert out1.shape == (M, 3) and torch.equal(_bits(out1), _bits(out0))
        assert all(a.abs().sum() > 0 for a in g0)
        for i, (a, b) in enumerate(zip(g1, g0)):
            assert torch.equal(_bits(a), _bits(b)), (i, tuple(a.shape))
        assert torch.equal(_bits(op.t), _bits(kept)), "the pass wrote its operand"
    with torch.no_grad():
        assert torch.equal(_bits(net(op)), _bits(out0))
    bf = dict(dtype=torch.bfloat16, device="cuda")
    for bad in (Bf16Operand(torch.zeros(128, 128, **bf), M, D),                                    # rows: pad(200, 128) = 256
                Bf16Operand(torch.zeros(256, 64, **bf), M, D),                                     # columns: pad(45, 128) = 128
                Bf16Operand(torch.zeros(256, 128, dtype=torch.float16, device="cuda"), M, D),
                Bf16Operand(torch.zeros(256, 128, **bf), M, D + 1),
                Bf16Operand(torch.zeros(256, 128, dtype=torch.bfloat16), M, D)):                   # on the host
        with pytest.raises(ValueError, match="Bf16Operand"):
            net(bad)
    with pytest.raises(ValueError, match="operand"):
        net.operand(x[:, :D - 1])


# ---------------------------------------------------------------------------------------------------------------- 6: the agent
CFG = dict(hidden=(256, 128, 128), min_batch_size=2048, opt_num_epochs=2, mfma_update=True, deterministic_update=True)


@pytest.fixture(scope="module")
def agents():
    """One env, one rollout, three agents with the same weights: `off` (fused_norm off), `on` and `on2` (on, same seed).  Each runs update_params once on a clone of
    the rollout.  The float64 reference of the policy's statistics (the oracle applied once per optimisation iteration to the batch's states) is formed here, once."""
    from oracle.ppo_oracle import running_norm_update
    from smplsim_amd.agents.ppo import AgentPPO, PPOConfig
    from smplsim_amd.batch import SMPLSimVecEnv
    env = SMPLSimVecEnv(256, task="HumanoidSpeed", autoreset=True, seed=3)
    off = AgentPPO(env, PPOConfig(**CFG), seed=1)
    on, on2 = AgentPPO(env, PPOConfig(fused_norm=True, **CFG), seed=1), AgentPPO(env, PPOConfig(fused_norm=True, **CFG), seed=1)
    for a in (on, on2):
        a.policy_net.load_state_dict(off.policy_net.state_dict()); a.value_net.load_state_dict(off.value_net.state_dict())
    batch = off.sample()
    before = [p.detach().clone() for p in off.policy_net.parameters()]
    info = {}
    for name, a in (("off", off), ("on", on), ("on2", on2)):
        info[name] = a.update_params({k: v.clone() for k, v in batch.items()})
    torch.cuda.synchronize()
    T, N = batch["rewards"].shape
    x64 = batch["states"].reshape(T * N, -1).double().cpu().numpy()
    n, mean, var = 0, np.zeros(x64.shape[1]), np.zeros(x64.shape[1])
    for _ in range(CFG["opt_num_epochs"]):
        n, mean, var = running_norm_update(n, mean, var, x64)
    yield dict(env=env, off=off, on=on, on2=on2, info=info, before=before, ref=dict(n=n, mean=mean, var=var, std=np.sqrt(var)), TN=T * N)
    env.close()


def test_agent_critic_is_unchanged_by_the_flag(agents):
    """The critic does not depend on the policy and its operand is the same cast made once: value net and value loss bit for bit."""
    off, on = agents["off"], agents["on"]
    assert on.lib_norm is not None and off.lib_norm is None
    for (k, a), (_, b) in zip(off.value_net.state_dict().items(), on.value_net.state_dict().items()):
        assert _same_bits(a, b), k
    assert _same_bits(agents["info"]["off"]["value_loss"], agents["info"]["on"]["value_loss"])
    assert float(agents["info"]["on"]["value_loss"]) > 0.0


def test_agent_policy_statistics_follow_float64_as_closely_as_torchs(agents):
    ref = agents["ref"]
    assert ref["n"] == 2 * agents["TN"]
    errs = {}
    for name in ("off", "on"):
        nm = agents[name].policy_net.norm
        assert int(nm.n.item()) == 2 * agents["TN"], name
        errs[name] = {k: float((np.abs(getattr(nm, k).double().cpu().numpy() - ref[k]) / _ulp32(ref[k])).max()) for k in ("mean", "var", "std")}   # in fp32 ulps
    _record("fused_norm_agent_statistics_ulps", **{k: [errs["on"][k], errs["off"][k]] for k in ("mean", "var", "std")})                            # [kernel, e32]
    print(errs)
    for k in ("mean", "var", "std"):
        assert errs["on"][k] <= max(FACTOR * errs["off"][k], 4.0), (k, errs)


def test_agent_losses_and_step_direction_agree_with_the_torch_norm(agents):
    i0, i1 = agents["info"]["off"], agents["info"]["on"]
    assert abs(float(i0["surr_loss"]) - float(i1["surr_loss"])) < 3e-2
    d0 = torch.cat([(p.detach() - b).flatten() for p, b in zip(agents["off"].policy_net.parameters(), agents["before"]) if p.requires_grad])
    d1 = torch.cat([(p.detach() - b).flatten() for p, b in zip(agents["on"].policy_net.parameters(), agents["before"]) if p.requires_grad])
    assert d0.norm() > 0 and d1.norm() > 0
    cos = float((d0 * d1).sum() / (d0.norm() * d1.norm()))
    _record("fused_norm_agent_step", cos=cos, surr_off=float(i0["surr_loss"]), surr_on=float(i1["surr_loss"]))
    assert cos > 0.9, cos


def test_agent_same_seed_same_bits(agents):
    sa, sb = _agent_state(agents["on"]), _agent_state(agents["on2"])
    assert sa.keys() == sb.keys() and {"policy.norm.mean", "policy.norm.var", "policy.norm.std", "policy.norm.n"} <= set(sa)
    differing = [k for k in sa if not _same_bits(sa[k], sb[k])]
    assert not differing, differing


def test_agent_with_every_library_piece_trains_and_its_checkpoint_is_a_plain_agents(agents):
    import math
    from smplsim_amd.agents.ppo import AgentPPO, PPOConfig
    env = agents["env"]
    cfg = dict(hidden=CFG["hidden"], min_batch_size=2048, opt_num_epochs=2)
    a = AgentPPO(env, PPOConfig(mfma_update=True, deterministic_update=True, fused_loss=True, fused_optimizer=True, fused_norm=True, **cfg), seed=2)
    log = a.optimize_policy(2)
    assert len(log) == 2
    for row in log:
        assert math.isfinite(row["surr_loss"]) and math.isfinite(row["value_loss"]) and math.isfinite(row["grad_norm"]), row
    nm = a.policy_net.norm
    assert int(nm.n.item()) == 2 * 2 * a.horizon * env.num_envs and torch.isfinite(nm.mean).all() and (nm.var >= 0).all()
    assert (nm.std - nm.var.sqrt()).abs().max() <= 1e-6 * nm.std.abs().max()
    plain = AgentPPO(env, PPOConfig(**cfg), seed=5)
    plain.set_full_state_weights(a.get_full_state_weights())
    for (k, x), (_, y) in zip(a.policy_net.state_dict().items(), plain.policy_net.state_dict().items()):
        assert _same_bits(x, y), k
    assert plain.epoch == 2
