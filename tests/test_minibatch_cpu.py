"""Mini-batch PPO epochs, host side (-m "not gpu"): the config switches, the blocked layout of learning/minibatch.py filled by torch (the agent's CPU path), the
update against an in-test restatement of the reference's loop (agents/agent_ppo.py:25-46), the sampler's independence of the flag, and the argument checks of
ss_gather_rows (they run before any launch, so no GPU is needed: cf. test_norm_cpu.py; the GPU file repeats them next to a destination that must stay unchanged)."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from oracle import ppo_oracle as PO


class Env:                                                          # what AgentPPO reads of an env before sample() is called
    device, obs_size, nu, num_envs = torch.device("cpu"), 11, 3, 40


def _cpu_gae(rewards, not_done, not_dead, values, gamma, tau, bootstrap=None):
    """estimate_advantages_columns for host tensors (the package's own is a kernel): the oracle's recursion.  The agent and the restatement both get it."""
    adv, ret = PO.gae_columns(rewards.numpy(), not_done.numpy(), not_dead.numpy(), values.numpy(), gamma, tau, None if bootstrap is None else bootstrap.numpy())
    return torch.tensor(adv, dtype=torch.float32), torch.tensor(ret, dtype=torch.float32)


def _batch(T=25, N=40, seed=0, partial_exps=False):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    done = torch.rand(T, N, generator=g) < 0.05
    dead = done & (torch.rand(T, N, generator=g) < 0.5)
    exps = torch.ones(T, N)
    if partial_exps:
        exps[torch.rand(T, N, generator=g) < 0.3] = 0.0
    return dict(states=r(T, N, Env.obs_size).clamp(-5, 5), actions=r(T, N, Env.nu) * 0.1, rewards=torch.rand(T, N, generator=g), not_done=(~done).float(),
                not_dead=(~dead).float(), exps=exps, last_state=r(N, Env.obs_size).clamp(-5, 5))


def _perms(E, M, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randperm(M, generator=g) for _ in range(E)])


# ---------------------------------------------------------------------------------------------------------------- 1: config
def test_config_fields_and_refusals():
    from smplsim_amd.agents.ppo import AgentPPO, PPOConfig
    c = PPOConfig()
    assert c.use_mini_batch is False and c.mini_batch_size == 0
    agent = AgentPPO(Env(), PPOConfig(hidden=(16,)))
    assert agent.gen_update is None                                 # the flag off: no object of the new path exists
    for B in (0, -4):
        with pytest.raises(ValueError, match="mini_batch_size >= 1"):
            AgentPPO(Env(), PPOConfig(use_mini_batch=True, mini_batch_size=B, hidden=(16,)))
    with pytest.raises(ValueError, match="minibatch_gather"):
        AgentPPO(Env(), PPOConfig(use_mini_batch=True, mini_batch_size=8, hidden=(16,), extra={"minibatch_gather": "numpy"}))
    with pytest.raises(ValueError, match="use_mini_batch only"):
        agent.update_params(_batch(), perms=_perms(10, 1000, 0))


def test_mini_batch_larger_than_the_rollout_is_refused_at_update_time(monkeypatch):
    from smplsim_amd.agents import ppo
    monkeypatch.setattr(ppo, "estimate_advantages_columns", _cpu_gae)
    agent = ppo.AgentPPO(Env(), ppo.PPOConfig(use_mini_batch=True, mini_batch_size=1001, hidden=(16,), opt_num_epochs=1))
    before = copy.deepcopy(agent.policy_net.state_dict())
    with pytest.raises(ValueError, match="exceeds the rollout's 1000 rows"):
        agent.update_params(_batch())
    assert all(torch.equal(v, before[k]) for k, v in agent.policy_net.state_dict().items())
    ok = ppo.AgentPPO(Env(), ppo.PPOConfig(use_mini_batch=True, mini_batch_size=1000, hidden=(16,), opt_num_epochs=1))
    assert int(ok.update_params(_batch())["opt_steps"]) == 1
    for bad in (_perms(1, 999, 0), _perms(2, 1000, 0), _perms(1, 1000, 0).int(), _perms(1, 1000, 0) + 1, _perms(1, 1000, 0) - 1):
        with pytest.raises(ValueError, match="perms"):
            ok.update_params(_batch(), perms=bad)


# ---------------------------------------------------------------------------------------------------------------- 2: the layout
def test_shuffled_batch_torch_layout_against_the_row_formula():
    """M = 1000, B = 96: ten blocks, 40 rows sit out.  Every written row equals its source row (the row formula restated in NumPy); every other destination
    element keeps the sentinel written after allocation; block(i) is rows [96 i, 96 i + 96) of the destination."""
    from smplsim_amd.learning.minibatch import ShuffledBatch
    M, B = 1000, 96
    g = torch.Generator().manual_seed(5)
    src = dict(a=torch.randn(M, 7, generator=g), b=torch.randn(M, 1, generator=g))
    wide = torch.randn(M, 12, generator=g)
    src["c"] = wide[:, 2:9]                                         # a strided source (ld 12, offset base)
    sb = ShuffledBatch(src, B, mode="torch")
    assert sb.num_blocks == 10
    for name in src:
        d = sb.destination(name)
        assert tuple(d.shape) == (960, src[name].shape[1]) and d.dtype == torch.float32 and not d.any()
        d.fill_(-77.0)
    perm = torch.randperm(M, generator=g)
    sb.shuffle(perm)
    p = perm.numpy()
    for name, x in src.items():
        d, x = sb.destination(name).numpy(), x.numpy()
        want = np.full_like(d, -77.0)
        for i in range(960):
            want[(i // B) * B + i % B] = x[p[i]]
        assert np.array_equal(d, want), name
    for i in (0, 9):
        blk = sb.block(i)
        assert set(blk) == set(src)
        assert torch.equal(blk["a"], src["a"][perm[i * B:(i + 1) * B]]) and blk["a"].is_contiguous()
    with pytest.raises(IndexError):
        sb.block(10)
    # the same object serves the next update's tensors; other shapes do not
    nxt = {k: v + 1 for k, v in src.items()}
    assert sb.matches(nxt, B, "torch") and not sb.matches(nxt, 95, "torch") and not sb.matches({k: v[:999] for k, v in nxt.items()}, B, "torch")
    sb.bind(nxt)
    sb.shuffle(perm)
    assert torch.equal(sb.block(3)["b"], nxt["b"][perm[3 * B:4 * B]])
    with pytest.raises(ValueError, match="block_rows"):
        ShuffledBatch(src, 1001, mode="torch")
    with pytest.raises(RuntimeError, match="GPU"):
        ShuffledBatch(src, B, mode="kernel")
    with pytest.raises(ValueError, match="perm must be"):
        sb.shuffle(perm[:959])


def test_shuffled_batch_operand_blocks_are_padded_operands():
    """A Bf16Operand source: destination [nb * pad(B, 128), pad(D, 128)], block stride pad(B, 128); block(i) is a contiguous operand of B rows whose pad rows and
    columns are zero (untouched since allocation)."""
    from smplsim_amd.learning.fused_train import Bf16Operand
    from smplsim_amd.learning.minibatch import ShuffledBatch
    M, B, D = 1000, 96, 11
    g = torch.Generator().manual_seed(6)
    t = torch.zeros(1024, 128, dtype=torch.bfloat16)
    t[:M, :D] = torch.randn(M, D, generator=g)
    sb = ShuffledBatch(dict(x=Bf16Operand(t, M, D)), B, mode="torch")
    d = sb.destination("x")
    assert tuple(d.shape) == (10 * 128, 128) and d.dtype == torch.bfloat16 and not d.any()
    perm = torch.randperm(M, generator=g)
    sb.shuffle(perm)
    for i in range(10):
        op = sb.block(i)["x"]
        assert isinstance(op, Bf16Operand) and (op.M, op.D) == (B, D) and tuple(op.t.shape) == (128, 128) and op.t.is_contiguous()
        assert torch.equal(op.t[:B].view(torch.int16), t[perm[i * B:(i + 1) * B]].view(torch.int16))
        assert not op.t[B:].any() and not op.t[:, D:].any()


# ---------------------------------------------------------------------------------------------------------------- 3: the update
def _state(policy, value, opt_p, opt_v):
    out = {}
    for name, net in (("policy", policy), ("value", value)):
        for k, v in net.state_dict().items():
            out[f"{name}.{k}"] = v
    for name, opt in (("opt_policy", opt_p), ("opt_value", opt_v)):
        for i, st in enumerate(opt.state.values()):
            for k, v in st.items():
                if torch.is_tensor(v):
                    out[f"{name}.{i}.{k}"] = v
    return out


def _restated_update(policy, value, opt_p, opt_v, cfg, batch, perms):
    """AgentPG.update_params + AgentPPO.update_policy of the reference with use_mini_batch, as plain torch: values, GAE, normalised advantages and the fixed
    log-probs over the whole batch; then per epoch index by the epoch's permutation, floor(M / B) slices, per slice one critic step on all its rows and one
    clipped-surrogate step on its exploration rows, the networks in train mode."""
    T, N = batch["rewards"].shape
    M, B = T * N, cfg.mini_batch_size
    states, actions = batch["states"].reshape(M, -1), batch["actions"].reshape(M, -1)
    policy.eval(); value.eval()
    with torch.no_grad():
        values = value(states).reshape(T, N)
        boot = value(batch["last_state"]).reshape(N)
    adv, ret = _cpu_gae(batch["rewards"], batch["not_done"], batch["not_dead"], values, cfg.gamma, cfg.tau, boot)
    adv = ((adv - adv.mean()) / adv.std()).reshape(M, 1)
    ret = ret.reshape(M, 1)
    exps = batch["exps"].reshape(M)
    with torch.no_grad():
        flp = policy.get_log_prob(states, actions)
    policy.train(); value.train()
    steps = 0
    for e in range(cfg.opt_num_epochs):
        perm = perms[e]
        s_p, a_p, r_p, adv_p, flp_p, e_p = states[perm].clone(), actions[perm].clone(), ret[perm].clone(), adv[perm].clone(), flp[perm].clone(), exps[perm].clone()
        for i in range(M // B):
            sl = slice(i * B, min((i + 1) * B, M))
            s_b, a_b, r_b, adv_b, flp_b, e_b = s_p[sl], a_p[sl], r_p[sl], adv_p[sl], flp_p[sl], e_p[sl]
            ind = e_b.nonzero(as_tuple=False).squeeze(1)
            for _ in range(cfg.value_opt_niter):
                vloss = (value(s_b) - r_b).pow(2).mean()
                opt_v.zero_grad()
                vloss.backward()
                opt_v.step()
            ratio = torch.exp(policy.get_log_prob(s_b[ind], a_b[ind]) - flp_b[ind])
            ad = adv_b[ind]
            loss = -torch.min(ratio * ad, torch.clamp(ratio, 1.0 - cfg.clip_epsilon, 1.0 + cfg.clip_epsilon) * ad).mean()
            opt_p.zero_grad()
            loss.backward()
            torch.nn.utils.clip_grad_norm_(policy.parameters(), cfg.policy_grad_clip)
            opt_p.step()
            steps += 1
    return steps


@pytest.mark.parametrize("partial_exps", [False, True])
def test_update_equals_the_restated_reference_loop(monkeypatch, partial_exps):
    """M = 1000, B = 96, three epochs with given perms, two updates: parameters, Adam moments and RunningNorm buffers torch.equal to the restatement's (both sides run
    the same CPU ops on the same values in the same order).  30 steps per update; the 40 tail rows of every epoch take no part (norm.n counts 960 per epoch)."""
    from smplsim_amd.agents import ppo
    monkeypatch.setattr(ppo, "estimate_advantages_columns", _cpu_gae)
    cfg = ppo.PPOConfig(use_mini_batch=True, mini_batch_size=96, hidden=(64, 32), opt_num_epochs=3)
    agent = ppo.AgentPPO(Env(), cfg, seed=4)
    policy, value = copy.deepcopy(agent.policy_net), copy.deepcopy(agent.value_net)
    opt_p = torch.optim.Adam(policy.parameters(), lr=cfg.policy_lr, eps=1e-8, weight_decay=cfg.policy_weightdecay)
    opt_v = torch.optim.Adam(value.parameters(), lr=cfg.value_lr, eps=1e-8, weight_decay=cfg.value_weightdecay)
    for round_ in range(2):
        batch, perms = _batch(seed=round_, partial_exps=partial_exps), _perms(3, 1000, 10 + round_)
        info = agent.update_params({k: v.clone() for k, v in batch.items()}, perms=perms)
        steps = _restated_update(policy, value, opt_p, opt_v, cfg, batch, perms)
        assert int(info["opt_steps"]) == steps == 30
        assert {"value_loss", "surr_loss", "mean_reward", "episodes_ended"} <= set(info) and np.isfinite(float(info["surr_loss"]))
        a, b = _state(agent.policy_net, agent.value_net, agent.optimizer_policy, agent.optimizer_value), _state(policy, value, opt_p, opt_v)
        assert a.keys() == b.keys() and {"policy.norm.mean", "policy.norm.n", "opt_policy.0.exp_avg", "opt_value.0.exp_avg_sq"} <= set(a)
        differing = [k for k in a if not torch.equal(a[k], b[k])]
        assert not differing, (round_, differing)
        if not partial_exps:
            assert int(agent.policy_net.norm.n) == (round_ + 1) * 3 * 960
    assert agent._shuffled.num_blocks == 10 and agent._shuffled.mode == "torch"


def test_update_without_given_perms_is_reproducible_and_full_batch_is_untouched(monkeypatch):
    """perms=None: the orders come from the agent's own update generator — two agents with one seed end with the same bits, a third seed differs.  The flag off:
    info['opt_steps'] == opt_num_epochs."""
    from smplsim_amd.agents import ppo
    monkeypatch.setattr(ppo, "estimate_advantages_columns", _cpu_gae)
    cfg = dict(use_mini_batch=True, mini_batch_size=250, hidden=(32,), opt_num_epochs=2)
    a, b, c = (ppo.AgentPPO(Env(), ppo.PPOConfig(**cfg), seed=s) for s in (7, 7, 8))
    c.policy_net.load_state_dict(a.policy_net.state_dict()); c.value_net.load_state_dict(a.value_net.state_dict())
    batch = _batch(seed=3)
    infos = [x.update_params({k: v.clone() for k, v in batch.items()}) for x in (a, b, c)]
    assert [int(i["opt_steps"]) for i in infos] == [8, 8, 8]
    sa, sb, sc = (_state(x.policy_net, x.value_net, x.optimizer_policy, x.optimizer_value) for x in (a, b, c))
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
    assert any(not torch.equal(sa[k], sc[k]) for k in sa)
    off = ppo.AgentPPO(Env(), ppo.PPOConfig(hidden=(32,), opt_num_epochs=2), seed=7)
    assert int(off.update_params({k: v.clone() for k, v in batch.items()})["opt_steps"]) == 2


# ---------------------------------------------------------------------------------------------------------------- 4: the sampler
def test_the_sampler_does_not_depend_on_the_flag():
    """Two agents with one seed, one with the flag: the same sampler generator state, the same global generator state after construction, the same initial
    weights; the update generator exists only with the flag and is not the sampler's."""
    from smplsim_amd.agents.ppo import AgentPPO, PPOConfig
    off = AgentPPO(Env(), PPOConfig(hidden=(64, 32)), seed=9)
    g_off = torch.get_rng_state()
    on = AgentPPO(Env(), PPOConfig(hidden=(64, 32), use_mini_batch=True, mini_batch_size=96), seed=9)
    g_on = torch.get_rng_state()
    assert torch.equal(off.gen.get_state(), on.gen.get_state()) and torch.equal(g_off, g_on)
    for net in ("policy_net", "value_net"):
        so, sn = getattr(off, net).state_dict(), getattr(on, net).state_dict()
        assert so.keys() == sn.keys() and all(torch.equal(so[k], sn[k]) for k in so)
    assert off.gen_update is None and on.gen_update is not None and on.gen_update is not on.gen
    before = on.gen.get_state()
    torch.randperm(1000, generator=on.gen_update)
    assert torch.equal(on.gen.get_state(), before) and torch.equal(torch.get_rng_state(), g_on)


# ---------------------------------------------------------------------------------------------------------------- the entry point's checks
@pytest.fixture(scope="module")
def L():
    from smplsim_amd import _cabi, _lib
    _lib.build()
    lib = _cabi.bind_mlp(ctypes.CDLL(_lib.LIB_PATH))
    lib.ss_last_error.restype = ctypes.c_char_p
    return lib


SRC, DST = 1 << 20, 1 << 30                                         # pointer values that are never dereferenced: every call here fails its checks first


def _gather(L, tensors=((SRC, DST, 4, 7, 7, 7, 96),), count=None, perm=1 << 12, src_rows=1000, rows=960, block_rows=96):
    from smplsim_amd._cabi import GatherTensor
    table = (GatherTensor * max(1, len(tensors)))(*[GatherTensor(*t) for t in tensors]) if tensors is not None else None
    return L.ss_gather_rows(table, len(tensors) if count is None else count, perm, src_rows, rows, block_rows, None)


def test_gather_rows_checks_its_arguments_before_any_launch(L):
    one = (SRC, DST, 4, 7, 7, 7, 96)
    t = lambda **kw: (tuple(kw.get(k, v) for k, v in zip(("src", "dst", "eb", "cols", "ld_src", "ld_dst", "stride"), one)),)
    bad = [(dict(tensors=None, count=1), b"null argument"), (dict(perm=None), b"null argument"), (dict(tensors=t(src=None)), b"null argument"),
           (dict(tensors=t(dst=None)), b"null argument"), (dict(count=0), b"1 <= count <= 8"), (dict(tensors=(one,) * 9), b"1 <= count <= 8"),
           (dict(count=-1), b"1 <= count <= 8"), (dict(tensors=t(eb=1)), b"elem_bytes"), (dict(tensors=t(eb=8)), b"elem_bytes"), (dict(tensors=t(eb=0)), b"elem_bytes"),
           (dict(tensors=t(cols=0)), b"cols >= 1"), (dict(tensors=t(ld_src=6)), b"row strides"), (dict(tensors=t(ld_dst=6)), b"row strides"),
           (dict(tensors=t(stride=95)), b"dst_block_stride"), (dict(src_rows=0), b"src_rows >= 1"), (dict(rows=0), b"rows >= 1"), (dict(rows=-7), b"rows >= 1"),
           (dict(block_rows=0), b"block_rows >= 1"), (dict(tensors=t(src=SRC + 2)), b"aligned to elem_bytes"), (dict(tensors=t(dst=DST + 1)), b"aligned to elem_bytes"),
           (dict(tensors=t(src=SRC + 1, eb=2)), b"aligned to elem_bytes"), (dict(perm=(1 << 12) + 4), b"8-byte aligned"),
           (dict(tensors=t(dst=SRC)), b"must not overlap"), (dict(tensors=t(dst=SRC + 28 * 999)), b"must not overlap"), (dict(tensors=t(src=DST + 28 * 959)), b"must not overlap"),
           (dict(tensors=(one, t(dst=None)[0])), b"null argument")]
    for kw, msg in bad:
        assert _gather(L, **kw) == -1 and msg in L.ss_last_error(), (kw, L.ss_last_error())
