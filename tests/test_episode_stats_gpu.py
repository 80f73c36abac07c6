"""Episode statistics on the GPU (include/smplsim_mlp.h: ss_episode_stats; learning/episode_stats.py; PPOConfig.episode_stats) against the float64 restatement of
LoggerRL in test_episode_stats_cpu.py, walked over the env columns.

What the definition fixes is compared exactly, the carries bit for bit: num_steps, num_episodes, total_episode_len, the four extremes, ep_len, ep_return (an
episode's return is the fp64 sum of its fp32 rewards with t ascending, continued from the carry: one order, one result).  Every other sum is within
2 n 2^-53 sum|x| of the restatement's, n its number of addends: the bound of two fp64 sums of the same addends in any two orders (test_episode_stats_cpu.py), derived,
not measured; the observed worst ratio to it is recorded (`episode_stats_sum_ratio`)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from test_det_update_gpu import _nan_ws, _same_bits  # noqa: E402
from test_episode_stats_cpu import NAMES, check_stats, rollout, same, walk  # noqa: E402
from test_gemm_kernels_gpu import _lib, _p, _record, _st  # noqa: E402

SENT = -12345.0
SENT_I = -777
TAIL = 8
SHAPES = [(1, 1, 0), (7, 63, 0), (7, 64, 4), (5, 65, 3), (9, 257, 4), (13, 300, 8)]     # the column edges of a wavefront and of four, the 16-byte path, a generic P
RATES = {"none": 0.0, "every_step": 1.0, "random": 0.2}
WORST = [0.0]


class _Call:
    """The device side of one ss_episode_stats call: the carries and stats as the heads of sentinel-filled buffers, the workspace NaN-filled with a margin."""

    def __init__(self, rewards, not_done, parts, ep_return, ep_len, parts_offset=0):
        T, N = rewards.shape
        self.T, self.N, self.P = T, N, 0 if parts is None else parts.shape[2]
        self.rewards, self.not_done = torch.from_numpy(rewards).cuda(), torch.from_numpy(not_done).cuda()
        self.parts = None
        if parts is not None:                                       # parts_offset floats into a larger buffer: 1 = a base that is only 4-byte aligned
            buf = torch.full((parts.size + parts_offset,), float("nan"), device="cuda")
            buf[parts_offset:] = torch.from_numpy(parts).cuda().reshape(-1)
            self.parts = buf[parts_offset:]
            assert (self.parts.data_ptr() % 16 == 0) == (parts_offset % 4 == 0)
        self.ret_buf = torch.full((N + TAIL,), SENT, dtype=torch.float64, device="cuda")
        self.len_buf = torch.full((N + TAIL,), SENT_I, dtype=torch.int32, device="cuda")
        self.stats_buf = torch.full((9 + self.P + TAIL,), SENT, dtype=torch.float64, device="cuda")
        self.ret_buf[:N] = torch.from_numpy(ep_return).cuda()
        self.len_buf[:N] = torch.from_numpy(ep_len).cuda()

    def run(self, fill=float("nan")):
        L = _lib()
        need = L.ss_episode_stats_workspace(self.T, self.N, self.P)
        assert need == -(-self.N // 64) * (9 + self.P) * 8, (need, L.ss_last_error())
        ws = _nan_ws(need)
        if fill == fill:
            ws[:need // 4] = fill
        torch.cuda.synchronize()
        rc = L.ss_episode_stats(_p(self.rewards), _p(self.not_done), _p(self.parts), self.T, self.N, self.P, _p(self.ret_buf), _p(self.len_buf), _p(self.stats_buf),
                                _p(ws), need, _st())
        assert rc == 0, L.ss_last_error()
        torch.cuda.synchronize()
        assert torch.isnan(ws[need // 4:]).all(), "a write beyond the documented workspace"
        assert (self.stats_buf[9 + self.P:] == SENT).all(), "a write behind stats[9 + P]"
        assert (self.ret_buf[self.N:] == SENT).all(), "a write behind ep_return[N]"
        assert (self.len_buf[self.N:] == SENT_I).all(), "a write behind ep_len[N]"
        self.workspace = ws[:need // 4].view(torch.float64).view(-1, 9 + self.P)
        return self.stats_buf[:9 + self.P].cpu().numpy(), self.ret_buf[:self.N].cpu().numpy(), self.len_buf[:self.N].cpu().numpy()

    def outputs(self):
        return [self.stats_buf.clone(), self.ret_buf.clone(), self.len_buf.clone()]


def _carries(N, seed):
    g = np.random.default_rng(seed)
    return g.standard_normal(N) * 3.0 + 0.1, g.integers(1, 250, N).astype(np.int32)      # random, non-zero


def _bits64(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


# ---------------------------------------------------------------------------------------------------------------- 1: against the restatement
@pytest.mark.parametrize("pattern", list(RATES))
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_against_the_float64_restatement(shape, pattern):
    T, N, P = shape
    rewards, not_done, parts = rollout(T, N, P, seed=1000 * T + N, rate=RATES[pattern])
    ep_return, ep_len = _carries(N, seed=N)
    call = _Call(rewards, not_done, parts, ep_return, ep_len)
    stats, got_ret, got_len = call.run()
    lg = walk(rewards, not_done, parts, ep_return, ep_len)        # (moves ep_return / ep_len on, in place)
    print("measured", dict(zip(NAMES, stats)), "want", dict(zip(NAMES, lg.stats())))
    check_stats(stats, lg, T, N, WORST)
    assert _bits64(got_ret, ep_return), "ep_return: the order is fixed by the definition"
    assert np.array_equal(got_len, ep_len)
    assert lg.num_episodes == {"none": 0, "every_step": T * N}.get(pattern, lg.num_episodes)
    if pattern == "none":
        assert stats[4] == np.inf and stats[5] == -np.inf
    # the workspace as documented: row g is the statistics of the columns [64 g, 64 g + 64); its counts add up
    w = call.workspace.cpu().numpy()
    assert w.shape[0] == -(-N // 64) and w[:, 0].sum() == T * N and w[:, 1].sum() == lg.num_episodes and w[:, 3].sum() == lg.total_episode_len
    assert w[-1, 0] == T * (N - 64 * (w.shape[0] - 1))
    _record("episode_stats_sum_ratio", worst=WORST[0])


# ---------------------------------------------------------------------------------------------------------------- 2: reproducible
@pytest.mark.parametrize("shape", [(9, 257, 4), (13, 300, 8)], ids=["9x257x4", "13x300x8"])
def test_the_outputs_do_not_depend_on_what_the_workspace_held(shape):
    T, N, P = shape
    rewards, not_done, parts = rollout(T, N, P, seed=5)
    outs = []
    for fill in (float("nan"), 3.0e30):
        call = _Call(rewards, not_done, parts, *_carries(N, seed=9))
        call.run(fill)
        outs.append(call.outputs())
    for a, b in zip(*outs):
        assert _same_bits(a, b)


def test_unaligned_parts_take_the_4_byte_loads_with_the_same_bits():
    """P == 4: a 16-byte aligned base takes the one-load path, any other base the generic one; the additions are the same."""
    T, N, P = 9, 257, 4
    rewards, not_done, parts = rollout(T, N, P, seed=6)
    outs = []
    for off in (0, 1):
        call = _Call(rewards, not_done, parts, *_carries(N, seed=2), parts_offset=off)
        call.run()
        outs.append(call.outputs())
    for a, b in zip(*outs):
        assert _same_bits(a, b)


# ---------------------------------------------------------------------------------------------------------------- 3: NaN and the end flag
@pytest.mark.parametrize("ends", [True, False], ids=["episode_ends", "episode_continues"])
def test_a_nan_reward_stays_in_its_column(ends):
    T, N, P, COL = 6, 70, 0, 5
    rewards, not_done, _ = rollout(T, N, P, seed=8)
    not_done[:, COL] = 1.0
    if ends:
        not_done[4, COL] = 0.0
    clean = rewards.copy()
    rewards[2, COL] = np.nan
    c0, l0 = _carries(N, seed=3)
    stats, got_ret, got_len = _Call(rewards, not_done, None, c0, l0).run()
    ret_nan, len_nan = c0.copy(), l0.copy()
    lg = walk(rewards, not_done, None, ret_nan, len_nan)
    check_stats(stats, lg, T, N)
    ret_clean, len_clean = c0.copy(), l0.copy()
    lg_clean = walk(clean, not_done, None, ret_clean, len_clean)
    s = dict(zip(NAMES, stats))
    # the counts are those of the clean rollout
    assert (s["num_steps"], s["num_episodes"], s["total_episode_len"]) == (T * N, lg_clean.num_episodes, lg_clean.total_episode_len)
    assert np.isnan([s["total_reward"], s["min_reward"], s["max_reward"]]).all()
    ep_nan = np.isnan([s["total_episode_reward"], s["min_episode_reward"], s["max_episode_reward"]])
    assert ep_nan.all() if ends else not ep_nan.any()
    if not ends:                                                    # the episode statistics never saw the NaN: those of the clean rollout, the extremes exactly
        assert s["min_episode_reward"] == lg_clean.min_episode_reward and s["max_episode_reward"] == lg_clean.max_episode_reward
    # every other column's carry is the clean rollout's, bit for bit; the column itself is NaN until its episode ends
    others = np.arange(N) != COL
    assert _bits64(got_ret[others], ret_clean[others]) and np.array_equal(got_len, len_clean)
    assert got_ret[COL] == np.float64(rewards[5, COL]) if ends else np.isnan(got_ret[COL])


def test_only_a_zero_ends_an_episode():
    """not_done of 0.5, -0.0 and NaN next to 1 and +0: +0 and -0 end the episode, everything else continues it."""
    vals = np.array([[1.0, 0.5, -0.0, np.nan, 0.0, 2.0, -1.0],
                     [np.nan, -0.0, 0.5, 0.0, 1.0, -0.0, np.inf],
                     [0.5, np.nan, 1.0, 1.0, -0.0, 0.5, np.nan]], dtype=np.float32)
    T, N = vals.shape
    rewards, _, _ = rollout(T, N, 0, seed=4)
    c0, l0 = _carries(N, seed=4)
    stats, got_ret, got_len = _Call(rewards, vals, None, c0, l0).run()
    ep_return, ep_len = c0.copy(), l0.copy()
    lg = walk(rewards, vals, None, ep_return, ep_len)
    check_stats(stats, lg, T, N)
    assert stats[1] == lg.num_episodes == 6                        # the six +-0 entries
    assert _bits64(got_ret, ep_return) and np.array_equal(got_len, ep_len)
    assert list(got_len) == [l0[0] + 3, 1, 2, 1, 0, 1, l0[6] + 3]


# ---------------------------------------------------------------------------------------------------------------- 4: the agent
def _speed_env(seed=0):
    from smplsim_amd.batch import SMPLSimVecEnv
    return SMPLSimVecEnv(48, task="HumanoidSpeed", episode_length=4, autoreset=True, seed=seed)


def _two_rollouts(agent, N, P):
    """Two sample() calls; every batch's episode_stats against the restatement walked over the batch with the carry kept.  Returns the batches and loggers."""
    ep_return, ep_len = np.zeros(N), np.zeros(N, np.int32)
    out = []
    for k in range(2):
        b = agent.sample(horizon=6)
        in_flight = int((ep_len > 0).sum())
        parts = b["reward_parts"].cpu().numpy() if P else None
        lg = walk(b["rewards"].cpu().numpy(), b["not_done"].cpu().numpy(), parts, ep_return, ep_len)
        stats = b["episode_stats"]
        assert stats.is_cuda and stats.dtype == torch.float64 and stats.shape == (9 + P,)
        check_stats(stats.cpu().numpy(), lg, 6, N, WORST)
        assert _bits64(agent.episode_stats.ep_return.cpu().numpy(), ep_return) and np.array_equal(agent.episode_stats.ep_len.cpu().numpy(), ep_len)
        out.append((b, lg, in_flight))
    return out


def test_agent_counts_episodes_that_end_inside_a_rollout_and_span_two():
    from smplsim_amd.agents.ppo import AgentPPO, PPOConfig
    cfg = dict(hidden=(64, 64), min_batch_size=6 * 48, opt_num_epochs=1)
    on = AgentPPO(_speed_env(), PPOConfig(episode_stats=True, **cfg), seed=2)
    off = AgentPPO(_speed_env(), PPOConfig(**cfg), seed=2)
    assert off.episode_stats is None and on.episode_stats.part_names == ()
    runs = _two_rollouts(on, 48, 0)
    (b0, lg0, _), (b1, lg1, in_flight) = runs
    assert lg0.num_episodes >= 48 and in_flight > 0                # episodes of at most 5 steps (truncated once cur_t > 4) in rollouts of 6: every env ends one inside, some span two
    assert lg1.total_episode_len > 0 and "reward_parts" not in b0
    for b_on in (b0, b1):                                           # the flag changes nothing the sampler computes
        b_off = off.sample(horizon=6)
        assert set(b_on) == set(b_off) | {"episode_stats"}
        for k in ("states", "actions", "rewards"):
            assert _same_bits(b_on[k], b_off[k]), k
    info = on.update_params(b1)
    d = on.episode_stats.as_dict(b1["episode_stats"])
    assert len(d) == 9 and d["num_steps"] == 288 and d["num_episodes"] == lg1.num_episodes and d["avg_episode_len"] == lg1.total_episode_len / lg1.num_episodes <= 5
    for k, v in d.items():
        assert info[k].dim() == 0 and same(float(info[k]), v), k
    assert "avg_episode_len" not in off.update_params(b_off)


def test_pipelined_sampler_counts_like_the_serial_one():
    """sample_pipelined hands the sub-batches' rows to the same _rollout_out: with the flag on both samplers return the same statistics and carries, bit for bit
    (the bf16 MFMA policy: its row results do not depend on the row count, cf. test_gpu_parity.py's pipelined sampler test)."""
    from smplsim_amd.agents.ppo import AgentPPO, PPOConfig
    from smplsim_amd.batch import SMPLSimVecEnv
    from smplsim_amd.pipeline import PipelinedVecEnv
    N, G, T = 128, 2, 6
    kw = dict(task="HumanoidSpeed", episode_length=4, seed=9)
    cfg = PPOConfig(hidden=(256, 128), min_batch_size=N * T, mfma_inference=True, episode_stats=True)
    serial = AgentPPO(SMPLSimVecEnv(N, **kw), cfg, seed=4)
    pipe = PipelinedVecEnv(N, sub_batches=G, **kw)
    piped = AgentPPO(pipe, cfg, seed=4)
    for _ in range(2):
        b1, b2 = serial.sample(), piped.sample_pipelined(pipe)
        torch.cuda.synchronize()
        assert set(b1) == set(b2) and _same_bits(b1["rewards"], b2["rewards"]) and _same_bits(b1["not_done"], b2["not_done"])
        assert float(b1["episode_stats"][1]) >= N and _same_bits(b1["episode_stats"], b2["episode_stats"])
        assert _same_bits(serial.episode_stats.ep_return, piped.episode_stats.ep_return) and torch.equal(serial.episode_stats.ep_len, piped.episode_stats.ep_len)
    pipe.close()


def test_agent_keeps_the_reward_terms_of_an_imitation_env():
    import test_motion_lib as T
    from smplsim_amd.agents.ppo import AgentPPO, PPOConfig
    from smplsim_amd.imitation import SMPLSimImitationVecEnv
    env = SMPLSimImitationVecEnv(32, T.make_lib(None, device=0), seed=1, termination_distance=0.15)
    env.offset[:, 2] = 0.05
    assert env.reward_part_names == ("pos", "rot", "vel", "ang_vel")
    agent = AgentPPO(env, PPOConfig(episode_stats=True, hidden=(64, 64), min_batch_size=6 * 32, opt_num_epochs=1), seed=3)
    for b, lg, _ in _two_rollouts(agent, 32, 4):
        assert b["reward_parts"].shape == (6, 32, 4)
        assert not torch.equal(b["reward_parts"][0], b["reward_parts"][-1])      # every step's row was copied that step (the env reuses one buffer)
        d = agent.episode_stats.as_dict(b["episode_stats"])
        for p, name in enumerate(env.reward_part_names):
            want = float(b["reward_parts"][:, :, p].double().sum()) / (6 * 32)
            assert abs(d["reward_" + name] - want) <= 2 * 6 * 32 * 2.0 ** -53 * float(b["reward_parts"][:, :, p].double().abs().sum()) / (6 * 32), name
    assert torch.equal(b["reward_parts"][-1], env.reward_parts)    # the last step's row is what the env's buffer still holds
    info = agent.update_params(b)
    assert all(k in info for k in ("avg_episode_reward", "avg_episode_len", "avg_reward", "reward_pos", "reward_rot", "reward_vel", "reward_ang_vel"))
    _record("episode_stats_sum_ratio", worst=WORST[0])
