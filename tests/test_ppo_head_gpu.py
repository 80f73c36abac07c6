"""The PPO loss heads on the GPU (include/smplsim_mlp.h: ss_ppo_policy_head, ss_value_head; learning/fused_loss.py; PPOConfig.fused_loss).

The bound of every comparison against float64 is taken in the test itself: the fp32 torch expression of agents/ppo.py (the path the heads replace) is evaluated on the
same inputs, its largest error against float64 is e32 (per output), and the kernel's largest error must be <= 4 * e32 (a different summation order and exp)."""
import math

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from test_det_update_gpu import _agent_state, _same_bits  # noqa: E402
from test_gemm_kernels_gpu import _lib, _p, _record, _st  # noqa: E402

EPS = 0.2
RATIOS = (0.5, 0.79, 0.81, 0.999, 1.0, 1.001, 1.19, 1.21, 2.0)
FACTOR = 4.0
MARGIN = 512                 # doubles of workspace beyond the documented size: they must keep what they held


def _log_density(mean, log_std, actions):
    """PolicyGaussian.get_log_prob after the network: [M, 1] in the dtype of the arguments."""
    ls = log_std.expand_as(mean)
    z = (actions - mean) * torch.exp(-ls)
    return (-0.5 * z * z - ls - 0.5 * math.log(2.0 * math.pi)).sum(dim=1, keepdim=True)


def _surrogate(logp, adv, old, eps=EPS):
    """AgentPPO.ppo_loss after the log-density."""
    ratio = torch.exp(logp - old)
    clipped = ratio.clamp(1.0 - eps, 1.0 + eps)
    return -torch.minimum(ratio * adv, clipped * adv).mean(), ratio


def _old_logp(logp64, M):
    """old_logp (fp32) such that the true ratio of row i cycles through RATIOS."""
    target = torch.tensor(RATIOS, dtype=torch.float64)[torch.arange(M) % len(RATIOS)]
    return (logp64.reshape(-1) - torch.log(target)).float().reshape(M, 1)


def _adv(M, g):
    adv = torch.randn(M, 1, generator=g)
    adv[::7] = 0.0
    return adv


_INPUTS = {}


def _policy_inputs(M, dim):
    """fp32 inputs on the CPU, with the float64 reference and the fp32 torch result of the same expression (computed once per shape, shared, not modified)."""
    if (M, dim) in _INPUTS:
        return _INPUTS[(M, dim)]
    g = torch.Generator().manual_seed(1000 * M + dim)
    mean = torch.randn(M, dim, generator=g) * 0.3
    log_std = torch.full((1, dim), -2.5)
    actions = mean + torch.exp(log_std) * torch.randn(M, dim, generator=g)
    adv = _adv(M, g)
    old = _old_logp(_log_density(mean.double(), log_std.double(), actions.double()), M)
    out = dict(mean=mean, log_std=log_std, actions=actions, adv=adv, old=old)
    for name, dt in (("ref", torch.float64), ("t32", torch.float32)):
        m, ls = mean.to(dt).requires_grad_(), log_std.to(dt).requires_grad_()
        logp = _log_density(m, ls, actions.to(dt))
        loss, ratio = _surrogate(logp, adv.to(dt), old.to(dt))
        loss.backward()
        out[name] = dict(logp=logp.detach().reshape(-1), dmean=m.grad, dlog_std=ls.grad.reshape(-1), loss=loss.detach().reshape(1),
                         approx_kl=(old.to(dt) - logp.detach()).mean().reshape(1), mean_ratio=ratio.detach().mean().reshape(1),
                         clipped=((ratio.detach() - 1.0).abs() > EPS).sum().item(), ratio=ratio.detach().reshape(-1))
    r = out["ref"]["ratio"]
    assert min((r - (1 - EPS)).abs().min(), (r - (1 + EPS)).abs().min()) > 0.0099         # no row's branch can flip through fp32 rounding
    assert out["ref"]["clipped"] == out["t32"]["clipped"]
    _INPUTS[(M, dim)] = out
    return out


def _strided(t, ld, dtype=torch.float32):
    """t [M, n] in a NaN-filled [M, ld] buffer on the GPU: (buffer, view)."""
    buf = torch.full((t.shape[0], ld), float("nan"), dtype=dtype, device="cuda")
    buf[:, :t.shape[1]] = t.cuda()
    return buf, buf[:, :t.shape[1]]


def _workspace(nbytes, fill="nan"):
    assert nbytes > 0
    n = (nbytes + 7) // 8 + MARGIN
    if fill == "nan":
        return torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    if fill == "ones":
        return torch.ones(n, dtype=torch.float64, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(int(fill))
    return torch.randint(0, 256, (n * 8,), dtype=torch.uint8, device="cuda", generator=g).view(torch.float64)


def _run_policy(inp, pad=(0, 0, 0), bf16=False, fill="nan", kick=None):
    """One call of ss_policy_head; pad = (ldm - dim, lda - dim, ldd - dim).  Returns the outputs (dmean as the full [M + 2, ldd] buffer, NaN-prefilled)."""
    M, dim = inp["mean"].shape
    L = _lib()
    mean, _ = _strided(inp["mean"], dim + pad[0])
    act, _ = _strided(inp["actions"], dim + pad[1])
    ldd = dim + pad[2]
    ls, adv, old = inp["log_std"].reshape(-1).cuda(), inp["adv"].reshape(-1).cuda(), inp["old"].reshape(-1).cuda()
    nan = float("nan")
    logp = torch.full((M + 2,), nan, device="cuda")
    dmean = torch.full((M + 2, ldd), nan, dtype=torch.bfloat16 if bf16 else torch.float32, device="cuda")
    dls = torch.full((dim + 2,), nan, device="cuda")
    stats = torch.full((6,), nan, device="cuda")
    need = L.ss_ppo_policy_head_workspace(M, dim)
    ws = _workspace(need, fill)
    tail = ws[(need + 7) // 8:].clone()
    torch.cuda.synchronize()
    if kick is not None:
        kick()                                                     # work for a second stream, enqueued right before the call under test
    st = _st()
    rc = L.ss_ppo_policy_head(_p(mean), dim + pad[0], _p(act), dim + pad[1], _p(ls), _p(adv), _p(old), M, dim, EPS, _p(logp), _p(dmean), ldd, int(bf16), _p(dls),
                              _p(stats), _p(ws), need, st)
    assert rc == 0, L.ss_last_error()
    torch.cuda.synchronize()
    assert torch.equal(ws[(need + 7) // 8:].view(torch.int64), tail.view(torch.int64)), "a write beyond the documented workspace"
    assert torch.isnan(logp[M:]).all() and torch.isnan(dls[dim:]).all() and torch.isnan(stats[4:]).all()
    assert torch.isnan(dmean[M:]).all() and torch.isnan(dmean[:, dim:]).all(), "dmean written outside [M, dim]"
    return dict(logp=logp[:M], dmean=dmean, dlog_std=dls[:dim], stats=stats[:4], ws=ws[:need // 8])


def _err(x, ref):
    return (x.detach().double().cpu() - ref.double().cpu()).abs().max().item()


def _check_against_e32(tag, got, ref, t32):
    """got, ref, t32: dicts of tensors with the same keys.  Every figure is recorded before anything is asserted."""
    rows = {k: (_err(got[k], ref[k]), _err(t32[k], ref[k])) for k in got}
    _record(tag, **{k: [e, e32] for k, (e, e32) in rows.items()})                                                # [kernel, e32] per output
    print(tag, {k: (f"{e:.3g}", f"{e32:.3g}") for k, (e, e32) in rows.items()})
    for k, (e, e32) in rows.items():
        assert not math.isnan(e) and e <= FACTOR * e32, (tag, k, e, e32)


SHAPES = [(M, 69) for M in (1, 3, 4, 5, 255, 257, 1000, 4100)] + [(257, d) for d in (1, 63, 64, 65, 130)]


# ---------------------------------------------------------------------------------------------------------------- 1: against float64
@pytest.mark.parametrize("pad", [(0, 0, 0), (3, 5, 11)], ids=["dense", "strided"])
@pytest.mark.parametrize("M,dim", SHAPES)
def test_policy_head_against_float64(M, dim, pad):
    inp = _policy_inputs(M, dim)
    out = _run_policy(inp, pad)
    ref, t32 = inp["ref"], inp["t32"]
    got = dict(logp=out["logp"], dmean=out["dmean"][:M, :dim], dlog_std=out["dlog_std"], loss=out["stats"][0:1], approx_kl=out["stats"][2:3],
               mean_ratio=out["stats"][3:4])
    assert not any(torch.isnan(v).any() for v in got.values())
    assert out["stats"][1].item() == torch.tensor(ref["clipped"] / M, dtype=torch.float64).float().item(), (out["stats"][1].item(), ref["clipped"], M)
    _check_against_e32(f"ppo_head_{M}x{dim}_{'s' if pad[0] else 'd'}", got, {k: ref[k] for k in got}, {k: t32[k] for k in got})
    # the partial rows are what the header says: ceil(M / 128) rows of 4 + dim doubles, the clip counts among them whole numbers that add up
    parts = out["ws"].view(-(-M // 128), 4 + dim)
    assert parts[:, 1].sum().item() == ref["clipped"] and not torch.isnan(parts).any()
    assert torch.equal(out["stats"][0:1].cpu(), (-_fold64(parts[:, 0]) / M).float().reshape(1))                # the stated order: ascending from partial 0
    assert torch.equal(out["dlog_std"].cpu(), torch.stack([_fold64(parts[:, 4 + j]) for j in range(dim)]).float())


def _fold64(col):
    """((p0 + p1) + p2) + ... in float64, in that order."""
    s = 0.0
    for v in col.cpu().tolist():
        s = s + v
    return torch.tensor(s, dtype=torch.float64)


_VALUE = {}


def _value_inputs(M):
    if M not in _VALUE:
        g = torch.Generator().manual_seed(77 + M)
        pred, target = torch.randn(M, 1, generator=g) * 3 + 10, torch.randn(M, 1, generator=g) * 3 + 10
        out = dict(pred=pred, target=target)
        for name, dt in (("ref", torch.float64), ("t32", torch.float32)):
            p = pred.to(dt).requires_grad_()
            loss = (p - target.to(dt)).pow(2).mean()                                     # AgentPPO.update_value
            loss.backward()
            out[name] = dict(dpred=p.grad.reshape(-1), loss=loss.detach().reshape(1))
        _VALUE[M] = out
    return _VALUE[M]


def _run_value(inp, ldd=1, bf16=False, fill="nan", kick=None):
    M = inp["pred"].shape[0]
    L = _lib()
    pred, target = inp["pred"].reshape(-1).cuda(), inp["target"].reshape(-1).cuda()
    nan = float("nan")
    dpred = torch.full((M + 2, ldd), nan, dtype=torch.bfloat16 if bf16 else torch.float32, device="cuda")
    loss = torch.full((3,), nan, device="cuda")
    need = L.ss_value_head_workspace(M)
    ws = _workspace(need, fill)
    tail = ws[(need + 7) // 8:].clone()
    torch.cuda.synchronize()
    if kick is not None:
        kick()                                                     # work for a second stream, enqueued right before the call under test
    st = _st()
    assert L.ss_value_head(_p(pred), _p(target), M, _p(dpred), ldd, int(bf16), _p(loss), _p(ws), need, st) == 0, L.ss_last_error()
    torch.cuda.synchronize()
    assert torch.equal(ws[(need + 7) // 8:].view(torch.int64), tail.view(torch.int64)), "a write beyond the documented workspace"
    assert torch.isnan(loss[1:]).all() and torch.isnan(dpred[M:]).all() and torch.isnan(dpred[:, 1:]).all()
    return dict(dpred=dpred, loss=loss[:1], ws=ws[:need // 8])


@pytest.mark.parametrize("ldd", [1, 8], ids=["dense", "strided"])
@pytest.mark.parametrize("M", [1, 255, 257, 4100])
def test_value_head_against_float64(M, ldd):
    inp = _value_inputs(M)
    out = _run_value(inp, ldd)
    got = dict(dpred=out["dpred"][:M, 0], loss=out["loss"])
    _check_against_e32(f"value_head_{M}_{ldd}", got, inp["ref"], inp["t32"])
    assert out["ws"].numel() == -(-M // 1024)
    assert torch.equal(out["loss"].cpu(), (_fold64(out["ws"]) / M).float().reshape(1))


# ---------------------------------------------------------------------------------------------------------------- 2: the bf16 form
@pytest.mark.parametrize("M,dim,ldd", [(257, 69, 72), (4100, 69, 128), (257, 130, 136), (5, 1, 8)])
def test_bf16_gradient_is_the_rounded_fp32_gradient(M, dim, ldd):
    inp = _policy_inputs(M, dim)
    f32 = _run_policy(inp, (0, 0, ldd - dim))
    b16 = _run_policy(inp, (0, 0, ldd - dim), bf16=True)
    assert b16["dmean"].dtype == torch.bfloat16
    want = f32["dmean"][:M, :dim].to(torch.bfloat16)                                    # round to nearest even
    assert torch.equal(b16["dmean"][:M, :dim].contiguous().view(torch.int16), want.contiguous().view(torch.int16))
    for k in ("logp", "dlog_std", "stats"):
        assert torch.equal(b16[k].view(torch.int32), f32[k].view(torch.int32)), k
    v = _value_inputs(4100 if M == 4100 else 257)
    vf, vb = _run_value(v, 8), _run_value(v, 8, bf16=True)
    n = v["pred"].shape[0]
    assert torch.equal(vb["dpred"][:n, 0].contiguous().view(torch.int16), vf["dpred"][:n, 0].to(torch.bfloat16).contiguous().view(torch.int16))
    assert torch.equal(vb["loss"].view(torch.int32), vf["loss"].view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------- 3: reproducible
def test_heads_are_reproducible_whatever_the_workspace_held_and_the_device_does():
    """Five calls at M = 4100, dim = 69 with a workspace of NaN, of ones and of random bytes; two of them while a second stream runs a large unrelated matmul:
    every output has the same bits in all five."""
    inp, v = _policy_inputs(4100, 69), _value_inputs(4100)
    side = torch.cuda.Stream()
    a = torch.randn(4096, 4096, device="cuda")
    outs, vouts = [], []

    def kick():
        with torch.cuda.stream(side):
            for _ in range(4):
                a @ a

    for i, fill in enumerate(["nan", "ones", "12345", "nan", "99"]):
        outs.append(_run_policy(inp, fill=fill, kick=kick if i in (1, 3) else None))
        vouts.append(_run_value(v, fill=fill, kick=kick if i in (1, 3) else None))
    torch.cuda.synchronize()
    for o in outs[1:]:
        for k in ("logp", "dlog_std", "stats"):
            assert torch.equal(o[k].view(torch.int32), outs[0][k].view(torch.int32)), k
        assert torch.equal(o["dmean"][:4100, :69].contiguous().view(torch.int32), outs[0]["dmean"][:4100, :69].contiguous().view(torch.int32))
        assert torch.equal(o["ws"].view(torch.int64), outs[0]["ws"].view(torch.int64))
    for o in vouts[1:]:
        assert torch.equal(o["loss"].view(torch.int32), vouts[0]["loss"].view(torch.int32))
        assert torch.equal(o["dpred"][:4100].contiguous().view(torch.int32), vouts[0]["dpred"][:4100].contiguous().view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------- 4: NaN is not hidden
def test_a_nan_reaches_the_loss_and_its_own_row_only():
    base = _policy_inputs(257, 69)
    inp = dict(base, mean=base["mean"].clone())
    inp["mean"][137, 5] = float("nan")
    out = _run_policy(inp)
    dm = out["dmean"][:257, :69]
    assert torch.isnan(out["stats"][0]) and torch.isnan(out["logp"][137]) and torch.isnan(dm[137]).all()
    keep = torch.arange(257, device="cuda") != 137
    assert torch.isfinite(dm[keep]).all() and torch.isfinite(out["logp"][keep]).all()
    assert torch.equal(dm[keep][:128].view(torch.int32), _run_policy(base)["dmean"][:128, :69].contiguous().view(torch.int32))   # rows of the first workgroup: untouched
    vb = _value_inputs(257)
    v = dict(vb, pred=vb["pred"].clone())
    v["pred"][5] = float("nan")
    vo = _run_value(v)
    assert torch.isnan(vo["loss"]).all() and torch.isnan(vo["dpred"][5, 0])
    keep = torch.arange(257, device="cuda") != 5
    assert torch.isfinite(vo["dpred"][:257, 0][keep]).all()


# ---------------------------------------------------------------------------------------------------------------- 5: the autograd wrappers
def _stub_agent(policy, fused):
    """An AgentPPO with just what ppo_loss reads: the torch network path, the loss heads on or off."""
    from smplsim_amd.agents.ppo import AgentPPO, PPOConfig
    from smplsim_amd.learning.fused_loss import PPOSurrogate
    agent = AgentPPO.__new__(AgentPPO)
    agent.cfg, agent.device, agent.policy_net, agent.fused_policy = PPOConfig(clip_epsilon=EPS), torch.device("cuda"), policy, None
    agent.surrogate = PPOSurrogate() if fused else None
    return agent


def test_ppo_surrogate_gives_the_parameter_gradients_of_the_torch_loss():
    """A small fp32 policy with a learned log-std, M = 1000: the gradient of every parameter through ppo_surrogate and through the existing torch ppo_loss, both
    against a float64 CPU copy of the network; the same 4 * e32 rule per parameter."""
    import copy
    from smplsim_amd.learning.networks import PolicyGaussian
    torch.manual_seed(5)
    M, sd, ad = 1000, 40, 69
    policy = PolicyGaussian(sd, ad, (64, 64), "silu", -2.5, fix_std=False).cuda().eval()
    p64 = copy.deepcopy(policy).cpu().double().eval()
    g = torch.Generator().manual_seed(6)
    states = torch.randn(M, sd, generator=g)
    with torch.no_grad():
        mean64, ls64 = p64.mean_and_log_std(states.double())
        actions = (mean64 + torch.exp(ls64) * torch.randn(M, ad, generator=g).double()).float()
        old = _old_logp(p64.get_log_prob(states.double(), actions.double()), M)
    adv = _adv(M, g)
    loss64, _ = _surrogate(p64.get_log_prob(states.double(), actions.double()), adv.double(), old.double())
    names = [n for n, _ in p64.named_parameters()]
    assert "action_log_std" in names
    ref = dict(zip(names, torch.autograd.grad(loss64, list(p64.parameters()))))
    ref["loss"] = loss64.detach()
    res = {}
    for fused in (False, True):
        agent = _stub_agent(policy, fused)
        loss = agent.ppo_loss(states.cuda(), actions.cuda(), adv.cuda(), old.cuda())
        assert loss.dim() == 0
        res[fused] = dict(zip(names, torch.autograd.grad(loss, list(policy.parameters()))))
        res[fused]["loss"] = loss.detach()
        if fused:
            stats = agent.surrogate.last_stats
            assert stats.shape == (4,) and stats[0].item() == loss.item()
    _check_against_e32("ppo_surrogate_autograd", res[True], ref, res[False])
    # a scaled loss scales the gradients (backward multiplies by the incoming gradient)
    agent = _stub_agent(policy, True)
    g3 = torch.autograd.grad(3.0 * agent.ppo_loss(states.cuda(), actions.cuda(), adv.cuda(), old.cuda()), list(policy.parameters()))
    for n, a in zip(names, g3):
        assert (a - 3.0 * res[True][n]).norm() <= 1e-5 * (3.0 * res[True][n]).norm(), n


def test_value_mse_gives_the_parameter_gradients_of_the_torch_loss():
    import copy
    from smplsim_amd.learning.fused_loss import value_mse
    from smplsim_amd.learning.networks import MLP, Value
    torch.manual_seed(8)
    M, sd = 1000, 40
    net = Value(MLP(sd, (64, 64), "silu")).cuda()
    n64 = copy.deepcopy(net).cpu().double()
    g = torch.Generator().manual_seed(9)
    states, returns = torch.randn(M, sd, generator=g), torch.randn(M, 1, generator=g) * 2 + 1
    names = [n for n, _ in n64.named_parameters()]
    loss64 = (n64(states.double()) - returns.double()).pow(2).mean()
    ref = dict(zip(names, torch.autograd.grad(loss64, list(n64.parameters()))), loss=loss64.detach())
    res = {}
    for fused in (False, True):
        pred = net(states.cuda())
        loss = value_mse(pred, returns.cuda()) if fused else (pred - returns.cuda()).pow(2).mean()
        assert loss.dim() == 0
        res[fused] = dict(zip(names, torch.autograd.grad(loss, list(net.parameters()))), loss=loss.detach())
    _check_against_e32("value_mse_autograd", res[True], ref, res[False])


# ---------------------------------------------------------------------------------------------------------------- 6: the agent
def test_two_agents_with_the_loss_heads_end_an_update_with_the_same_bits():
    """mfma_update, deterministic_update and fused_loss all on: two agents with one seed end update_params with the same bits in every parameter, buffer and
    optimiser state; info carries clip_frac and approx_kl.  With fused_loss off, info has neither."""
    from smplsim_amd.agents.ppo import AgentPPO, PPOConfig
    from smplsim_amd.batch import SMPLSimVecEnv
    env = SMPLSimVecEnv(256, task="HumanoidSpeed", autoreset=True, seed=3)
    cfg = dict(mfma_update=True, deterministic_update=True, hidden=(256, 128, 128), min_batch_size=2048, opt_num_epochs=2)
    a, b = AgentPPO(env, PPOConfig(fused_loss=True, **cfg), seed=1), AgentPPO(env, PPOConfig(fused_loss=True, **cfg), seed=1)
    off = AgentPPO(env, PPOConfig(**cfg), seed=1)
    assert a.surrogate is not None and a.value_mse is not None and off.surrogate is None and off.value_mse is None
    for round_ in range(2):
        batch = a.sample()
        ia = a.update_params({k: v.clone() for k, v in batch.items()})
        ib = b.update_params({k: v.clone() for k, v in batch.items()})
        io = off.update_params({k: v.clone() for k, v in batch.items()})
        torch.cuda.synchronize()
        sa, sb = _agent_state(a), _agent_state(b)
        assert sa.keys() == sb.keys() and any(k.startswith("opt_policy.") and k.endswith("exp_avg_sq") for k in sa)
        differing = [k for k in sa if not _same_bits(sa[k], sb[k])]
        assert not differing, (round_, differing)
        assert "clip_frac" not in io and "approx_kl" not in io and set(ia) == set(io) | {"clip_frac", "approx_kl"}
        for info in (ia, ib):
            assert info["clip_frac"].is_cuda and info["approx_kl"].is_cuda
            assert math.isfinite(float(info["clip_frac"])) and 0.0 <= float(info["clip_frac"]) <= 1.0 and math.isfinite(float(info["approx_kl"])), info
        assert all(_same_bits(ia[k], ib[k]) for k in ia)
        fig = dict(clip_frac=float(ia["clip_frac"]), approx_kl=float(ia["approx_kl"]), surr_fused=float(ia["surr_loss"]), surr_torch=float(io["surr_loss"]),
                   value_fused=float(ia["value_loss"]), value_torch=float(io["value_loss"]))
        _record(f"ppo_head_agent_round{round_}", **fig)
        print(round_, fig)
        if round_ == 0:
            # The wiring (strides, log_std, which mean) against the torch heads.  All three agents start from the same parameters and the losses in info are
            # those of the update's second iteration.  The first steps agree up to the rounding of the gradients (Adam's first step is lr g / (|g| + eps)), so
            # the second iteration's losses differ by rounding-sized amounts.  A mis-wired head drives the ratios out of the clip range, where the surrogate of
            # normalised advantages saturates near mean(max(0, -A)) * (1 - eps) ~ 0.3, and a wrong value gradient moves the MSE by far more than a percent
            # in one step.  The bounds sit between the two: 0.02 absolute on the surrogate (which is near zero), 2 % on the value loss.
            assert abs(fig["surr_fused"] - fig["surr_torch"]) <= 0.02, fig
            assert abs(fig["value_fused"] - fig["value_torch"]) <= 0.02 * abs(fig["value_torch"]), fig
