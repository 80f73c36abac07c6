"""Episode statistics, host side (-m "not gpu"): the switch, the float64 host path of learning/episode_stats.py against LoggerRL's start_episode / step /
end_episode restated here and walked over the env columns, one update against two over the halves, the no-episode case, and the argument checks of
ss_episode_stats (they run before any launch, so no GPU is needed: cf. test_norm_cpu.py).

Bounds.  The carries, the counts, total_episode_len and the four extremes are fixed by the definition (an episode's return is the fp64 sum of its fp32 rewards
with t ascending) and are compared exactly.  A sum of n addends x_i in fp64 in ANY order is within n 2^-53 sum|x_i| of the exact sum (first order in 2^-53), so two
such sums differ by at most 2 n 2^-53 sum|x_i|: that is the bound of every sum here, derived, not measured."""
import ctypes
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

U = 2.0 ** -53
NAMES = ("num_steps", "num_episodes", "total_episode_reward", "total_episode_len", "min_episode_reward", "max_episode_reward", "total_reward", "min_reward",
         "max_reward")
EXACT = (0, 1, 3, 4, 5, 7, 8)                                       # indices compared exactly


def _min(a, b):
    return math.nan if (a != a or b != b) else min(a, b)             # torch.amin: a NaN stays


def _max(a, b):
    return math.nan if (a != a or b != b) else max(a, b)


class Logger:
    """LoggerRL (smpl_sim/learning/logger_rl.py) restated: start_episode / step / end_episode with its field names, plus what a rollout of cut episodes needs
    next to it: the length of the episode in flight, total_episode_len, and total_reward over ALL steps (the reference's is over ended episodes: its batches are
    whole episodes).  Python floats: float64."""

    def __init__(self, P):
        self.num_steps = self.num_episodes = self.total_episode_len = 0
        self.total_episode_reward = self.total_reward = 0.0
        self.min_episode_reward = self.min_reward = math.inf
        self.max_episode_reward = self.max_reward = -math.inf
        self.episode_reward, self.episode_len = 0.0, 0
        self.parts = [0.0] * P
        self.abs = {"total_episode_reward": 0.0, "total_reward": 0.0, "parts": [0.0] * P}    # sum |addend| of every sum: what the bounds are made of

    def start_episode(self, episode_reward=0.0, episode_len=0):
        self.episode_reward, self.episode_len = episode_reward, episode_len

    def step(self, reward, parts):
        self.episode_reward += reward
        self.episode_len += 1
        self.min_reward, self.max_reward = _min(self.min_reward, reward), _max(self.max_reward, reward)
        self.num_steps += 1
        self.total_reward += reward
        self.abs["total_reward"] += abs(reward)
        for p, v in enumerate(parts):
            self.parts[p] += v
            self.abs["parts"][p] += abs(v)

    def end_episode(self):
        self.num_episodes += 1
        self.total_episode_reward += self.episode_reward
        self.abs["total_episode_reward"] += abs(self.episode_reward)
        self.total_episode_len += self.episode_len
        self.min_episode_reward = _min(self.min_episode_reward, self.episode_reward)
        self.max_episode_reward = _max(self.max_episode_reward, self.episode_reward)

    def stats(self):
        return np.array([getattr(self, n) for n in NAMES] + self.parts, dtype=np.float64)


def walk(rewards, not_done, parts, ep_return, ep_len):
    """The restatement walked over the env columns, one after the other, each with t ascending: rewards, not_done [T, N] float32 numpy, parts [T, N, P] or None;
    ep_return [N] float64 / ep_len [N] int32 are the carry, updated in place.  Returns the Logger."""
    T, N = rewards.shape
    P = 0 if parts is None else parts.shape[2]
    lg = Logger(P)
    for n in range(N):
        lg.start_episode(float(ep_return[n]), int(ep_len[n]))
        for t in range(T):
            lg.step(float(rewards[t, n]), [float(parts[t, n, p]) for p in range(P)])
            if not_done[t, n] == 0.0:                                # +0 and -0; anything else, a NaN included, continues
                lg.end_episode()
                lg.start_episode()
        ep_return[n], ep_len[n] = lg.episode_reward, lg.episode_len
    return lg


def sum_bounds(lg, T, N):
    """index in stats -> 2 n 2^-53 sum|x| of that sum, n its number of addends."""
    out = {2: 2 * max(lg.num_episodes, 1) * U * lg.abs["total_episode_reward"], 6: 2 * T * N * U * lg.abs["total_reward"]}
    for p, a in enumerate(lg.abs["parts"]):
        out[9 + p] = 2 * T * N * U * a
    return out


def same(a, b):
    """Equal as numbers, a NaN equal to a NaN."""
    return np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=True)


def check_stats(got, lg, T, N, worst=None):
    """got [9 + P] float64 against the restatement: exact where the definition fixes the value, within the derived bound for the sums."""
    want, bounds = lg.stats(), sum_bounds(lg, T, N)
    assert got.shape == want.shape
    for j in EXACT:
        assert same(got[j], want[j]), (NAMES[j], got[j], want[j])
    for j, b in bounds.items():
        if want[j] != want[j]:
            assert got[j] != got[j], (j, got[j])
            continue
        err = abs(got[j] - want[j])
        assert err <= b, (j, got[j], want[j], err, b)
        if worst is not None and b > 0:
            worst[0] = max(worst[0], err / b)


def rollout(T, N, P, seed, rate=0.2):
    g = np.random.default_rng(seed)
    rewards = (g.standard_normal((T, N)) * 0.7 + 0.3).astype(np.float32)
    not_done = (g.random((T, N)) >= rate).astype(np.float32)
    parts = g.random((T, N, P)).astype(np.float32) if P else None
    return rewards, not_done, parts


def _t(x):
    return None if x is None else torch.from_numpy(x.copy())


# ---------------------------------------------------------------------------------------------------------------- 1: the switch
class ToyEnv:
    """What AgentPPO's sampler needs of an env, on the host: N envs, episodes that end by a random death or after LENGTH steps, three reward terms in ONE
    reused buffer (as the imitation env hands them out)."""
    device, obs_size, nu, num_envs = torch.device("cpu"), 8, 2, 5
    reward_part_names = ("a", "b", "c")
    LENGTH = 4

    def __init__(self, seed=0):
        self.g = torch.Generator().manual_seed(seed)
        self.age = torch.zeros(self.num_envs, dtype=torch.int64)
        self.parts = torch.zeros(self.num_envs, 3)

    def _obs(self):
        return torch.randn(self.num_envs, self.obs_size, generator=self.g)

    def reset(self):
        self.age.zero_()
        return self._obs(), {}

    def step(self, actions):
        assert actions.shape == (self.num_envs, self.nu)
        self.age += 1
        self.parts.copy_(torch.rand(self.num_envs, 3, generator=self.g))
        died = torch.rand(self.num_envs, generator=self.g) < 0.15
        timed_out = self.age >= self.LENGTH
        self.age[died | timed_out] = 0
        return self._obs(), self.parts.sum(1) - 1.0, died, timed_out, {"reward_parts": self.parts}


def test_the_flag_is_off_by_default_and_then_nothing_is_new():
    from smplsim_amd.agents.ppo import AgentPPO, PPOConfig
    assert PPOConfig().episode_stats is False
    off = AgentPPO(ToyEnv(), PPOConfig(hidden=(16,)), seed=3)
    assert off.episode_stats is None                               # the flag off: no object of the new path exists
    b_off = off.sample(horizon=6)
    assert set(b_off) == {"states", "actions", "rewards", "not_done", "not_dead", "exps", "last_state"}
    on = AgentPPO(ToyEnv(), PPOConfig(hidden=(16,), episode_stats=True), seed=3)
    b_on = on.sample(horizon=6)
    assert set(b_on) == set(b_off) | {"episode_stats", "reward_parts"}
    for k in b_off:                                                 # the sampler does not depend on the flag
        assert torch.equal(b_off[k], b_on[k]), k


def test_agent_on_the_host_counts_episodes_across_two_rollouts(monkeypatch):
    """Episodes of at most 4 steps, rollouts of 6: episodes end inside a rollout and span two.  batch['episode_stats'] against the restatement walked over the two
    batches with the carry kept; the reward terms copied per step from the env's one buffer; the named values in update_params' info."""
    from smplsim_amd.agents import ppo
    from test_minibatch_cpu import _cpu_gae
    monkeypatch.setattr(ppo, "estimate_advantages_columns", _cpu_gae)
    agent = ppo.AgentPPO(ToyEnv(seed=5), ppo.PPOConfig(hidden=(16,), episode_stats=True, opt_num_epochs=1), seed=1)
    N = ToyEnv.num_envs
    ep_return, ep_len = np.zeros(N), np.zeros(N, np.int32)
    spanned, batches = 0, []
    for k in range(2):
        b = agent.sample(horizon=6, mean_action=bool(k))           # (mean-action rollouts count like any other)
        assert b["episode_stats"].dtype == torch.float64 and b["episode_stats"].shape == (12,)
        assert torch.equal(b["reward_parts"].sum(2) - 1.0, b["rewards"])
        spanned += int((ep_len > 0).sum())
        lg = walk(b["rewards"].numpy(), b["not_done"].numpy(), b["reward_parts"].numpy(), ep_return, ep_len)
        batches.append((b, lg))
        check_stats(b["episode_stats"].numpy(), lg, 6, N)
        assert lg.num_episodes >= N                                 # every env ends at least one episode in 6 steps
        assert np.array_equal(agent.episode_stats.ep_return.numpy(), ep_return) and np.array_equal(agent.episode_stats.ep_len.numpy(), ep_len)
    assert spanned > 0                                              # some episode was in flight when the second rollout began
    b, lg = batches[0]                                              # (the sampled one: a mean-action rollout has no exploration rows to update on)
    info = agent.update_params(b)
    d = agent.episode_stats.as_dict(b["episode_stats"])
    assert set(d) == {"num_steps", "num_episodes", "avg_episode_reward", "avg_episode_len", "min_episode_reward", "max_episode_reward", "avg_reward", "min_reward",
                      "max_reward", "reward_a", "reward_b", "reward_c"}
    for k, v in d.items():
        assert torch.is_tensor(info[k]) and info[k].dim() == 0 and float(info[k]) == v, k
    assert d["num_steps"] == 6 * N and d["avg_episode_len"] == lg.total_episode_len / lg.num_episodes <= ToyEnv.LENGTH
    assert abs(d["reward_a"] - float(b["reward_parts"][:, :, 0].double().mean())) < 1e-12
    agent.episode_stats.reset()
    assert not agent.episode_stats.ep_return.any() and not agent.episode_stats.ep_len.any()


# ---------------------------------------------------------------------------------------------------------------- 2: the host path against the restatement
@pytest.mark.parametrize("T,N,P", [(1, 1, 0), (7, 5, 3), (13, 70, 4), (9, 33, 8)])
@pytest.mark.parametrize("rate", [0.0, 1.0, 0.2], ids=["none", "every_step", "random"])
def test_host_path_against_the_restated_logger(T, N, P, rate):
    from smplsim_amd.learning.episode_stats import EpisodeStats
    rewards, not_done, parts = rollout(T, N, P, seed=T * 100 + N, rate=rate)
    g = np.random.default_rng(1)
    es = EpisodeStats(N, "cpu", part_names=[f"p{i}" for i in range(P)])
    es.ep_return.copy_(torch.from_numpy(g.standard_normal(N) * 3))
    es.ep_len.copy_(torch.from_numpy(g.integers(1, 200, N).astype(np.int32)))
    ep_return, ep_len = es.ep_return.numpy().copy(), es.ep_len.numpy().copy()
    got = es.update(_t(rewards), _t(not_done), _t(parts))
    assert got.dtype == torch.float64 and got.shape == (9 + P,)
    lg = walk(rewards, not_done, parts, ep_return, ep_len)
    check_stats(got.numpy(), lg, T, N)
    assert lg.num_episodes == (0 if rate == 0.0 else T * N if rate == 1.0 else lg.num_episodes)
    assert np.array_equal(es.ep_return.numpy(), ep_return) and np.array_equal(es.ep_len.numpy(), ep_len)
    d = es.as_dict(got)
    assert d["num_steps"] == T * N and d["num_episodes"] == lg.num_episodes
    if lg.num_episodes:
        assert d["avg_episode_len"] == lg.total_episode_len / lg.num_episodes


def test_one_update_equals_two_over_the_halves():
    from smplsim_amd.learning.episode_stats import EpisodeStats
    T1, T2, N, P = 5, 8, 37, 4
    rewards, not_done, parts = rollout(T1 + T2, N, P, seed=11)
    names = ("pos", "rot", "vel", "ang_vel")
    whole, halves = EpisodeStats(N, "cpu", names), EpisodeStats(N, "cpu", names)
    a = whole.update(_t(rewards), _t(not_done), _t(parts)).numpy()
    b1 = halves.update(_t(rewards[:T1]), _t(not_done[:T1]), _t(parts[:T1])).numpy()
    b2 = halves.update(_t(rewards[T1:]), _t(not_done[T1:]), _t(parts[T1:])).numpy()
    assert torch.equal(whole.ep_return, halves.ep_return) and torch.equal(whole.ep_len, halves.ep_len)
    for j in (0, 1, 3):
        assert a[j] == b1[j] + b2[j], NAMES[j]
    for j in (4, 7):
        assert a[j] == min(b1[j], b2[j]), NAMES[j]
    for j in (5, 8):
        assert a[j] == max(b1[j], b2[j]), NAMES[j]
    lg = walk(rewards, not_done, parts, np.zeros(N), np.zeros(N, np.int32))
    assert lg.num_episodes > N and a[1] == lg.num_episodes
    for j, bound in sum_bounds(lg, T1 + T2, N).items():            # (one more addition on the right: the bound's n counts the addends, and every addend is in both sums)
        assert abs(a[j] - (b1[j] + b2[j])) <= bound, (j, a[j], b1[j] + b2[j], bound)


def test_no_episode_ended():
    from smplsim_amd.learning.episode_stats import EpisodeStats
    rewards, not_done, _ = rollout(4, 6, 0, seed=2, rate=0.0)
    es = EpisodeStats(6, "cpu")
    s = es.update(_t(rewards), _t(not_done))
    d = es.as_dict(s)
    assert d["num_episodes"] == 0 and math.isnan(d["avg_episode_reward"]) and math.isnan(d["avg_episode_len"])
    assert d["min_episode_reward"] == math.inf and d["max_episode_reward"] == -math.inf
    assert d["num_steps"] == 24 and math.isfinite(d["avg_reward"]) and d["min_reward"] <= d["avg_reward"] <= d["max_reward"]
    assert (es.ep_len == 4).all() and np.array_equal(es.ep_return.numpy(), np.cumsum(rewards.astype(np.float64), axis=0)[-1])
    t = es.as_tensors(s)                                            # the device form: 0 / 0
    assert all(v.dim() == 0 for v in t.values()) and torch.isnan(t["avg_episode_len"]) and torch.isnan(t["avg_episode_reward"])


def test_wrong_inputs_are_refused():
    from smplsim_amd.learning.episode_stats import EpisodeStats
    es = EpisodeStats(4, "cpu", ("a",))
    r, nd, p = torch.zeros(3, 4), torch.ones(3, 4), torch.zeros(3, 4, 1)
    with pytest.raises(ValueError, match="reward_parts must be given"):
        es.update(r, nd)
    with pytest.raises(ValueError, match="reward_parts must be an fp32"):
        es.update(r, nd, torch.zeros(3, 4, 2))
    with pytest.raises(ValueError, match="rewards must be an fp32"):
        es.update(r.double(), nd, p)
    with pytest.raises(ValueError, match="not_done must be an fp32"):
        es.update(r, torch.ones(3, 5), p)
    with pytest.raises(ValueError, match="at most 8"):
        EpisodeStats(4, "cpu", [str(i) for i in range(9)])
    with pytest.raises(ValueError, match="reward_parts must be None"):
        EpisodeStats(4, "cpu").update(r, nd, p)


# ---------------------------------------------------------------------------------------------------------------- 3: the library's argument checks
@pytest.fixture(scope="module")
def L():
    from smplsim_amd import _cabi, _lib
    _lib.build()
    lib = _cabi.bind_mlp(ctypes.CDLL(_lib.LIB_PATH))
    lib.ss_last_error.restype = ctypes.c_char_p
    return lib


ONE = 16                                                            # a pointer value that is never dereferenced: every call below fails its checks first


def test_workspace_query_is_one_row_per_64_columns(L):
    from smplsim_amd import _cabi
    assert _cabi.EPISODE_MAX_PARTS == 8 and _cabi.EPISODE_STATS == NAMES
    assert "ss_episode_stats" in _cabi.MLP_EXPORTS and "ss_episode_stats_workspace" in _cabi.MLP_EXPORTS
    for N in (1, 63, 64, 65, 4096, 2 ** 31 - 1):
        for P in (0, 4, 8):
            for T in (1, 13):
                assert L.ss_episode_stats_workspace(T, N, P) == -(-N // 64) * (9 + P) * 8, (T, N, P)
    for T, N, P in ((0, 8, 0), (-1, 8, 0), (8, 0, 0), (8, -3, 0), (8, 8, -1), (8, 8, 9)):
        assert L.ss_episode_stats_workspace(T, N, P) < 0 and b"ss_episode_stats_workspace" in L.ss_last_error(), (T, N, P)


def _call(L, rewards=ONE, not_done=ONE, parts=ONE, T=7, N=100, P=4, ep_return=ONE, ep_len=ONE, stats=ONE, ws=ONE, nbytes=1 << 40):
    return L.ss_episode_stats(rewards, not_done, parts, T, N, P, ep_return, ep_len, stats, ws, nbytes, None)


def test_episode_stats_checks_its_arguments_before_any_launch(L):
    need = L.ss_episode_stats_workspace(7, 100, 4)
    assert need == 2 * 13 * 8
    bad = [(dict(rewards=None), b"null argument"), (dict(not_done=None), b"null argument"), (dict(ep_return=None), b"null argument"),
           (dict(ep_len=None), b"null argument"), (dict(stats=None), b"null argument"), (dict(parts=None), b"parts is null with P > 0"),
           (dict(T=0), b"T >= 1"), (dict(T=-2), b"T >= 1"), (dict(N=0), b"N >= 1"), (dict(N=-1), b"N >= 1"), (dict(P=-1), b"0 <= P <= 8"), (dict(P=9), b"0 <= P <= 8"),
           (dict(ws=None), b"null workspace"), (dict(ws=24), b"workspace must be 16-byte aligned"), (dict(nbytes=need - 1), b"workspace is too small"),
           (dict(nbytes=0), b"workspace is too small")]
    for kw, msg in bad:
        assert _call(L, **kw) == -1 and msg in L.ss_last_error(), (kw, L.ss_last_error())
    # what is allowed is not refused by these rules (the workspace is what fails here): no parts at all, parts that are only 4-byte aligned, one step, one env
    for kw in (dict(P=0, parts=None), dict(parts=20), dict(P=3, parts=20), dict(T=1), dict(N=1), dict(P=8)):
        assert _call(L, ws=None, **kw) == -1 and b"null workspace" in L.ss_last_error(), (kw, L.ss_last_error())
