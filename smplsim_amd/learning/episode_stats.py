"""Episode statistics of the sampler on the device (include/smplsim_mlp.h: ss_episode_stats; PPOConfig.episode_stats).

What it replaces: the LoggerRL every worker of the reference's sampler carries through its rollout (smpl_sim/learning/logger_rl.py; agents/agent.py:64-109) and
the training line made of it (agent_humanoid.py:171-193): eps_R_avg, R_avg, R_range, eps_len and the mean of every entry of the env's info (the reward terms).
Here N envs advance in lock step for a fixed horizon, so an episode spans many rollouts: the return and the length of the episode every env is in the middle of
are a carry on the device ([N] float64, [N] int32) that outlives the rollout, and one call walks the rollout's [T, N] rewards / not_done in two launches.

    stats = EpisodeStats(env.num_envs, env.device, part_names=("pos", "rot", "vel", "ang_vel"))
    s = stats.update(batch["rewards"], batch["not_done"], batch["reward_parts"])     # [9 + P] float64 on the device, no host synchronisation
    log = stats.as_dict(s)                                                             # one read-back

What differs from LoggerRL:
  * The reference's batches consist of whole episodes, so its avg_episode_len = num_steps / num_episodes and its avg_reward = total_reward / num_steps, with
    total_reward summed over the ENDED episodes, coincide with the per-episode and per-step means.  A rollout here holds the cut pieces of episodes that began
    before it or end after it, so the two would not: avg_episode_len is total_episode_len / num_episodes over the episodes that ENDED in the rollout (each with
    its full length, the steps of earlier rollouts included), avg_episode_reward likewise, and avg_reward is the sum of all rewards of the rollout / num_steps.
  * LoggerRL.merge takes the MAXIMUM of the workers' min_episode_reward; this takes the minimum over all envs.
  * With no episode ended in the rollout the two episode averages are NaN (the reference divides by zero), min_episode_reward is +inf and max_episode_reward
    -inf (LoggerRL's initial values).

The carries are not part of a checkpoint — the env states are not either —, so after a resume episodes are counted from the resume point.

On a CPU device (the agent's CPU path: the emulator-backed tests, the reference's run.py through the shim) the same definition runs as a plain float64 host
loop: the carries, the counts and the extremes are the same numbers (the definition fixes their order); the sums are float64 sums in another order.
"""
import numpy as np
import torch

from .._cabi import EPISODE_MAX_PARTS, EPISODE_STATS

NFIXED = len(EPISODE_STATS)      # SS_EP_PARTS: the first of the P part sums


def episode_stats_host(rewards, not_done, parts, ep_return, ep_len):
    """The definition of ss_episode_stats in float64 numpy: rewards, not_done [T, N] float32, parts [T, N, P] float32 or None, ep_return [N] float64 and
    ep_len [N] int32 updated in place.  Returns stats [9 + P] float64.  Columns side by side, t ascending; the columns' sums are added by numpy."""
    T, N = rewards.shape
    P = 0 if parts is None else parts.shape[2]
    episodes = np.zeros(N); ep_sum = np.zeros(N); ep_steps = np.zeros(N); r_sum = np.zeros(N)
    ep_min = np.full(N, np.inf); ep_max = np.full(N, -np.inf); r_min = np.full(N, np.inf); r_max = np.full(N, -np.inf)
    for t in range(T):
        r = rewards[t].astype(np.float64)
        ep_return += r
        ep_len += 1
        r_sum += r
        r_min, r_max = np.minimum(r_min, r), np.maximum(r_max, r)          # (numpy's minimum / maximum and min / max propagate a NaN, as torch.amin does)
        end = not_done[t] == 0.0                                      # +0 and -0; a NaN continues the episode
        episodes += end
        ep_sum[end] += ep_return[end]
        ep_steps[end] += ep_len[end]
        ep_min[end], ep_max[end] = np.minimum(ep_min[end], ep_return[end]), np.maximum(ep_max[end], ep_return[end])
        ep_return[end] = 0.0
        ep_len[end] = 0

    stats = np.empty(NFIXED + P)
    stats[:NFIXED] = (float(T) * float(N), episodes.sum(), ep_sum.sum(), ep_steps.sum(), ep_min.min(), ep_max.max(), r_sum.sum(), r_min.min(), r_max.max())
    for p in range(P):
        stats[NFIXED + p] = parts[:, :, p].astype(np.float64).sum(axis=0).sum()
    return stats


class EpisodeStats:
    """Owns the per-env carry (ep_return [N] float64, ep_len [N] int32) and the scratch of ss_episode_stats.  One stream per object."""

    def __init__(self, num_envs, device, part_names=()):
        self.num_envs, self.device, self.part_names = int(num_envs), torch.device(device), tuple(str(n) for n in part_names)
        if self.num_envs < 1:
            raise ValueError("EpisodeStats: num_envs >= 1")
        if len(self.part_names) > EPISODE_MAX_PARTS:
            raise ValueError(f"EpisodeStats: at most {EPISODE_MAX_PARTS} reward parts")
        self.ep_return = torch.zeros(self.num_envs, dtype=torch.float64, device=self.device)
        self.ep_len = torch.zeros(self.num_envs, dtype=torch.int32, device=self.device)
        self._ws = None
        if self.device.type == "cuda":
            from ._scratch import Scratch
            self._ws = Scratch()

    def reset(self):
        """Forget the episodes in flight: the next step of every env is the first of an episode."""
        self.ep_return.zero_()
        self.ep_len.zero_()

    def _inputs(self, rewards, not_done, reward_parts):
        N, P = self.num_envs, len(self.part_names)
        for name, t in (("rewards", rewards), ("not_done", not_done)):
            if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] != N or t.dtype != torch.float32 or t.device != self.ep_return.device:
                raise ValueError(f"EpisodeStats: {name} must be an fp32 [T >= 1, {N}] tensor on {self.ep_return.device}")
        if not_done.shape != rewards.shape:
            raise ValueError("EpisodeStats: rewards and not_done must have one shape")
        if (reward_parts is None) != (P == 0):
            raise ValueError(f"EpisodeStats: built for {P} reward parts {self.part_names}; reward_parts must be {'None' if P == 0 else 'given'}")
        if P:
            want = (rewards.shape[0], N, P)
            if tuple(reward_parts.shape) != want or reward_parts.dtype != torch.float32 or reward_parts.device != rewards.device:
                raise ValueError(f"EpisodeStats: reward_parts must be an fp32 {list(want)} tensor on the rewards' device")
            reward_parts = reward_parts.contiguous()
        return rewards.contiguous(), not_done.contiguous(), reward_parts

    @torch.no_grad()
    def update(self, rewards, not_done, reward_parts=None):
        """One rollout: the carries move on, the statistics of the rollout come back as a [9 + P] float64 tensor on the device (_cabi.EPISODE_STATS, then the part
        sums), enqueued on the current stream without a host synchronisation."""
        rewards, not_done, parts = self._inputs(rewards, not_done, reward_parts)
        T, N, P = rewards.shape[0], self.num_envs, len(self.part_names)
        if self.device.type != "cuda":
            out = episode_stats_host(rewards.numpy(), not_done.numpy(), None if parts is None else parts.numpy(), self.ep_return.numpy(), self.ep_len.numpy())
            return torch.from_numpy(out)
        from .._lib import _check, _launch_stream, _ptr, lib
        L = lib()
        stats = torch.empty(NFIXED + P, dtype=torch.float64, device=self.device)
        ws = self._ws.get(self.device, L.ss_episode_stats_workspace(T, N, P))
        _check(L.ss_episode_stats(_ptr(rewards), _ptr(not_done), _ptr(parts), T, N, P, _ptr(self.ep_return), _ptr(self.ep_len), _ptr(stats), _ptr(ws),
                                  ws.numel() * 8, _launch_stream(self.device)))
        return stats

    def as_tensors(self, stats):
        """The statistics under the reference's names as 0-dim tensors on the device of `stats`, without a read-back: num_steps, num_episodes, avg_episode_reward,
        avg_episode_len, min_episode_reward, max_episode_reward, avg_reward, min_reward, max_reward and reward_<name> (the mean of that reward term per step).
        No episode ended: the two averages are 0 / 0 = NaN."""
        s = dict(zip(EPISODE_STATS, stats[:NFIXED].unbind(0)))
        steps, eps = s["num_steps"], s["num_episodes"]
        out = {"num_steps": steps, "num_episodes": eps, "avg_episode_reward": s["total_episode_reward"] / eps, "avg_episode_len": s["total_episode_len"] / eps,
               "min_episode_reward": s["min_episode_reward"], "max_episode_reward": s["max_episode_reward"], "avg_reward": s["total_reward"] / steps,
               "min_reward": s["min_reward"], "max_reward": s["max_reward"]}
        for name, x in zip(self.part_names, stats[NFIXED:].unbind(0)):
            out["reward_" + name] = x / steps
        return out

    def as_dict(self, stats):
        """as_tensors on the host: ONE read-back of `stats`, then Python numbers (num_steps and num_episodes as int)."""
        out = {k: float(v) for k, v in self.as_tensors(stats.cpu()).items()}
        out["num_steps"], out["num_episodes"] = int(out["num_steps"]), int(out["num_episodes"])
        return out
