"""Failure-weighted clip sampling on the device (include/smplsim_mlp.h: ss_clip_outcomes, ss_clip_sampling_cdf; PPOConfig.clip_sampling).

What it feeds: the bookkeeping MotionLibSMPL restates from the reference (smpl_sim/smpllib/motion_lib_base.py:219-267: _termination_history,
update_soft_sampling_weight, update_sampling_prob, set_termination_history).  The reference's training loop collects the keys of the clips its envs failed on
and re-weights the library on the host; here the motion-imitation step re-initialises a finished env inside its launch, drawing the new clip from
MotionLibSMPL.sampling_cdf, a device array bound into that launch once.  So the tally and the CDF live on the device too:

    co = ClipOutcomes(env.motion_lib, uniform_mix=0.1)
    co.update(batch_clip_ids, dead, done)      # one launch: [M, 3] int64 counters (failed, completed, steps) += the rollout's
    prob = co.apply()                          # one launch: motion_lib.sampling_cdf rewritten IN PLACE (same storage: the fused step's binding stays valid)
    ...
    co.sync_to_host()                          # the one read-back: the library's _termination_history / curr_failed_keys / _sampling_prob follow

The rule: p_m = (1 - u) f_m / sum f + u / M with f_m the failures of loaded clip m (uniform while nothing has failed); u = 0 is the reference's
update_sampling_prob, u > 0 keeps the clips that never failed in play.  Nothing is summed in floating point before the CDF's own running sum, whose order is fixed
(numpy.cumsum's), so the device CDF equals clip_sampling_cdf_host bit for bit.

The counters belong to the clips the library has LOADED (positions in the loaded batch).  When the library loads other clips (load_count moves) the object
re-seeds on its next update / apply: everything zero, then failed[j] = round(_termination_history[_curr_motion_ids[j]]), so that the device CDF continues the host
history.  Failures counted since the last sync_to_host are dropped by a re-seed: sync before load_motions.

On a CPU device (the emulator-backed tests) the two NumPy restatements below are the path; they are also the tests' oracle.
"""
import numpy as np
import torch

from .._cabi import CLIP_COLUMNS

FAILED, COMPLETED, STEPS = range(len(CLIP_COLUMNS))
LAST = np.float32(1.0 + 1e-6)        # the last CDF entry, as MotionLibSMPL.load_motions writes it: a draw below 1 always lands in a clip


def clip_outcomes_host(clip_ids, dead, done, counts):
    """The definition of ss_clip_outcomes in numpy: clip_ids [T, N] int32, dead / done [T, N] bool or bytes (non-zero = set), counts [M, 3] int64 added to in
    place (and returned).  An id outside [0, M) skips its element."""
    clip_ids, dead, done = np.asarray(clip_ids), np.asarray(dead) != 0, np.asarray(done) != 0
    M = counts.shape[0]
    ok = (clip_ids >= 0) & (clip_ids < M)
    for column, sel in ((STEPS, ok), (FAILED, ok & dead), (COMPLETED, ok & ~dead & done)):
        counts[:, column] += np.bincount(clip_ids[sel].astype(np.int64), minlength=M).astype(np.int64)
    return counts


def clip_sampling_cdf_host(counts, uniform_mix):
    """The definition of ss_clip_sampling_cdf in numpy float64, operation by operation: counts [M, 3] int64 -> (cdf [M] float32, prob [M] float64)."""
    u = float(uniform_mix)
    if not 0.0 <= u <= 1.0:
        raise ValueError("uniform_mix must lie in [0, 1]")
    f = np.maximum(np.asarray(counts)[:, FAILED].astype(np.int64), 0)
    M = f.shape[0]
    S = int(f.sum(dtype=np.int64))                                  # an integer sum
    q = f.astype(np.float64) / np.float64(S) if S > 0 else np.full(M, np.float64(1.0) / np.float64(M))
    prob = (np.float64(1.0) - np.float64(u)) * q + np.float64(u) / np.float64(M)      # numpy: one multiplication, then one addition, each rounded
    cdf = np.cumsum(prob).astype(np.float32)                        # sequential, m ascending
    cdf[-1] = LAST
    return cdf, prob


class ClipOutcomes:
    """Owns the [M, 3] int64 counters of the loaded clips (columns _cabi.CLIP_COLUMNS) on the library's device, and `prob` [M] float64, the probabilities of the
    last apply() (before the first: those apply() would give).  One stream per object."""

    def __init__(self, motion_lib, uniform_mix=0.1):
        self.motion_lib, self.uniform_mix = motion_lib, float(uniform_mix)
        if not 0.0 <= self.uniform_mix <= 1.0:
            raise ValueError("ClipOutcomes: uniform_mix must lie in [0, 1]")
        self.device = torch.device(motion_lib.device)
        self._load_count = None
        self._seed()

    # ---- the library's history -> the counters
    def _seed(self):
        ml = self.motion_lib
        if getattr(ml, "_curr_motion_ids", None) is None:
            raise ValueError("ClipOutcomes: the motion library has no clips loaded (load_motions first)")
        if self._load_count == ml.load_count:
            return
        self._ids = np.array(ml._curr_motion_ids, dtype=np.int64)      # loaded position -> unique clip, as of this load
        M = len(self._ids)
        counts = np.zeros((M, len(CLIP_COLUMNS)), np.int64)
        counts[:, FAILED] = np.rint(np.asarray(ml._termination_history, np.float64)[self._ids]).astype(np.int64)
        self._synced = counts[:, FAILED].copy()                         # the failures the host history already holds
        self.counts = torch.from_numpy(counts).to(self.device)
        self.prob = torch.from_numpy(clip_sampling_cdf_host(counts, self.uniform_mix)[1]).to(self.device)
        self.last = torch.zeros(2, dtype=torch.int64, device=self.device)     # failed, completed episodes of the last update
        self._load_count = ml.load_count

    @property
    def num_clips(self):
        return self.counts.shape[0]

    def _inputs(self, clip_ids, dead, done):
        rows = []
        for name, t, kinds in (("clip_ids", clip_ids, (torch.int32,)), ("dead", dead, (torch.bool, torch.uint8)), ("done", done, (torch.bool, torch.uint8))):
            if not torch.is_tensor(t) or t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1 or t.dtype not in kinds or t.device != self.counts.device:
                raise ValueError(f"ClipOutcomes: {name} must be a {' / '.join(str(k) for k in kinds)} [T >= 1, N >= 1] tensor on {self.counts.device}")
            if t.shape != clip_ids.shape:
                raise ValueError("ClipOutcomes: clip_ids, dead and done must have one shape")
            rows.append(t.contiguous())
        return rows

    @torch.no_grad()
    def update(self, clip_ids, dead, done):
        """One rollout ([T, N]: the clip every env was tracking during each step, the sampler's dead and done rows) added to the counters: one launch on the
        current stream, no host synchronisation."""
        self._seed()
        clip_ids, dead, done = self._inputs(clip_ids, dead, done)
        before = self.counts[:, :STEPS].sum(0)
        if self.device.type != "cuda":
            clip_outcomes_host(clip_ids.numpy(), dead.numpy(), done.numpy(), self.counts.numpy())
        else:
            from .._lib import _check, _launch_stream, _ptr, lib
            T, N = clip_ids.shape
            _check(lib().ss_clip_outcomes(_ptr(clip_ids), _ptr(dead), _ptr(done), T, N, self.num_clips, _ptr(self.counts), _launch_stream(self.device)))
        self.last = self.counts[:, :STEPS].sum(0) - before

    @torch.no_grad()
    def apply(self):
        """motion_lib.sampling_cdf rewritten in place from the counters (same storage: whoever holds its address, the fused imitation step among them, reads the new
        CDF from the next launch behind this one on the stream).  Returns `prob` [M] float64 on the device, the object's own tensor, rewritten by every apply."""
        self._seed()
        cdf = self.motion_lib.sampling_cdf
        if cdf.dtype != torch.float32 or tuple(cdf.shape) != (self.num_clips,) or not cdf.is_contiguous() or cdf.device != self.counts.device:
            raise ValueError(f"ClipOutcomes: motion_lib.sampling_cdf must be a dense fp32 [{self.num_clips}] tensor on {self.counts.device}")
        if self.device.type != "cuda":
            c, p = clip_sampling_cdf_host(self.counts.numpy(), self.uniform_mix)
            cdf.copy_(torch.from_numpy(c))
            self.prob.copy_(torch.from_numpy(p))
        else:
            from .._lib import _check, _launch_stream, _ptr, lib
            _check(lib().ss_clip_sampling_cdf(_ptr(self.counts), self.num_clips, self.uniform_mix, _ptr(cdf), _ptr(self.prob), _launch_stream(self.device)))
        return self.prob

    def as_tensors(self):
        """For the log line, 0-dim tensors on the device, without a read-back: clips_failed (loaded clips with a failure on record), failed_episodes and
        completed_episodes (of the last update), min_clip_prob and max_clip_prob (of the last apply)."""
        return {"clips_failed": (self.counts[:, FAILED] > 0).sum(), "failed_episodes": self.last[FAILED], "completed_episodes": self.last[COMPLETED],
                "min_clip_prob": self.prob.min(), "max_clip_prob": self.prob.max()}

    def sync_to_host(self):
        """The one method that reads back.  The failures counted since the previous sync (or the seeding) are added to the library's _termination_history at the
        unique-clip indices (a clip loaded twice adds up), curr_failed_keys becomes the keys of the clips that failed since then, and _sampling_prob /
        _sampling_batch_prob follow by the library's own rule (update_sampling_prob; the batch probabilities as load_motions forms them).  Afterwards
        motion_lib.get_termination_history() is what a caller saves next to a checkpoint, as in the reference.  Returns the counters as an [M, 3] numpy array."""
        ml = self.motion_lib
        counts = self.counts.cpu().numpy()
        delta = counts[:, FAILED] - self._synced
        self._synced = counts[:, FAILED].copy()
        history = np.array(ml._termination_history, dtype=np.float64)
        np.add.at(history, self._ids, delta.astype(np.float64))
        ml._termination_history = history
        ml.curr_failed_keys = ml._motion_data_keys[np.unique(self._ids[delta > 0])].tolist()
        ml.update_sampling_prob(history)
        if self._load_count == ml.load_count:                          # (the loaded batch is still the one the counters belong to)
            p = ml._sampling_prob[self._ids]
            if p.sum() > 0:
                ml._sampling_batch_prob = p / p.sum()
        return counts
