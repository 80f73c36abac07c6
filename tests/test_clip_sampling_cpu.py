"""Failure-weighted clip sampling, host side (-m "not gpu"): the two NumPy restatements of learning/clip_sampling.py (the CPU path of ClipOutcomes and the oracle of
test_clip_sampling_gpu.py) on hand-made rollouts and against the motion library's own host CDF, the owner object and the agent's switch on the emulator-backed
imitation env, and the argument checks of ss_clip_outcomes / ss_clip_sampling_cdf (they run before any launch, so no GPU is needed: cf. test_episode_stats_cpu.py).

Nothing here takes a tolerance: the counters are integers and the CDF is compared bit for bit."""
import ctypes
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAST = np.float32(1.0 + 1e-6)


def _tally(ids, dead, done, M, counts=None):
    from smplsim_amd.learning.clip_sampling import clip_outcomes_host
    counts = np.zeros((M, 3), np.int64) if counts is None else counts
    return clip_outcomes_host(np.array(ids, np.int32), np.array(dead, bool), np.array(done, bool), counts)


def slow_tally(ids, dead, done, counts):
    """The definition element by element (the issue's three sentences), for the vectorised restatement to be checked against."""
    M = counts.shape[0]
    for c, d, e in zip(np.asarray(ids).reshape(-1), np.asarray(dead).reshape(-1), np.asarray(done).reshape(-1)):
        if 0 <= c < M:
            counts[c, 2] += 1
            if d:
                counts[c, 0] += 1
            elif e:
                counts[c, 1] += 1
    return counts


# ---------------------------------------------------------------------------------------------------------------- 1: the tally
def test_tally_of_hand_made_rollouts():
    M = 3
    # [T = 4, N = 4].  env 0: fails at t = 0 on clip 2 (dead and done), then tracks clip 0.  env 1: clip 1 throughout, completes at the last step.
    # env 2: dead without done at t = 1 (a failure all the same), clip 0.  env 3: clip 1 completes at t = 1, then clip 2 fails at t = 3: two episodes, two clips.
    ids = [[2, 1, 0, 1], [0, 1, 0, 1], [0, 1, 0, 2], [0, 1, 0, 2]]
    dead = [[1, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 0], [0, 0, 0, 1]]
    done = [[1, 0, 0, 0], [0, 0, 0, 1], [0, 0, 0, 0], [0, 1, 0, 1]]
    got = _tally(ids, dead, done, M)
    #                  failed completed steps
    assert got.tolist() == [[1, 0, 7], [0, 2, 6], [2, 0, 3]]
    assert got.dtype == np.int64 and got[:, 2].sum() == 16
    assert np.array_equal(got, slow_tally(ids, dead, done, np.zeros((M, 3), np.int64)))
    # a second call adds up, and the array handed in is the one updated
    again = _tally(ids, dead, done, M, counts=got)
    assert again is got and got.tolist() == [[2, 0, 14], [0, 4, 12], [4, 0, 6]]


def test_tally_skips_ids_outside_the_library():
    M = 2
    ids = [[-1, 0, M], [1, 2 ** 31 - 1, -(2 ** 31)]]
    ones = np.ones((2, 3), bool)
    got = _tally(ids, ones, ones, M, counts=np.full((M, 3), 10, np.int64))
    assert got.tolist() == [[11, 10, 11], [11, 10, 11]]            # the two ids inside; nothing else moved
    got = _tally([[-1, M]], [[1, 0]], [[1, 1]], M)
    assert not got.any()


def test_vectorised_tally_equals_the_definition_on_random_rollouts():
    g = np.random.default_rng(3)
    for T, N, M in ((1, 1, 1), (9, 70, 7), (5, 33, 40)):
        ids = g.integers(-2, M + 2, size=(T, N)).astype(np.int32)
        dead, done = g.random((T, N)) < 0.2, g.random((T, N)) < 0.4
        assert np.array_equal(_tally(ids, dead, done, M), slow_tally(ids, dead, done, np.zeros((M, 3), np.int64)))
        assert np.array_equal(_tally(ids, dead.astype(np.uint8) * 255, done.astype(np.uint8) * 2, M), _tally(ids, dead, done, M))   # any non-zero byte is set


# ---------------------------------------------------------------------------------------------------------------- 2: the CDF
def _counts(failed):
    c = np.zeros((len(failed), 3), np.int64)
    c[:, 0] = failed
    c[:, 1:] = 12345                                                # completions and steps play no part
    return c


def test_cdf_of_zero_counts_and_of_full_mix_is_uniform():
    from smplsim_amd.learning.clip_sampling import clip_sampling_cdf_host
    for M in (1, 2, 7, 100):
        uniform = np.full(M, 1.0 / M)
        for counts, u in ((_counts([0] * M), 0.0), (_counts([0] * M), 0.3), (_counts(np.arange(M) * 5), 1.0), (_counts([-4] * M), 0.0)):
            cdf, prob = clip_sampling_cdf_host(counts, u)
            assert cdf.dtype == np.float32 and prob.dtype == np.float64 and cdf.shape == prob.shape == (M,)
            if u in (0.0, 1.0):
                assert np.array_equal(prob, uniform), (M, u)       # (1 * q + 0 and 0 * q + 1 / M are exact)
            else:
                assert np.abs(prob - uniform).max() < 1e-15
            assert cdf[-1] == LAST and (np.diff(cdf) >= 0).all()
            assert np.array_equal(cdf[:-1], np.cumsum(prob).astype(np.float32)[:-1])


def test_cdf_rule_sentinel_and_monotony():
    from smplsim_amd.learning.clip_sampling import clip_sampling_cdf_host
    g = np.random.default_rng(5)
    for M in (1, 2, 7, 4097):
        f = g.integers(0, 50, M) * (g.random(M) < 0.5)
        f[g.integers(0, M)] = 2 ** 40
        if M > 2:
            f[1] = -3                                               # a negative count is 0
        for u in (0.0, 0.25, 1.0):
            cdf, prob = clip_sampling_cdf_host(_counts(f), u)
            fz = np.maximum(f, 0)
            want = (1.0 - u) * (fz / float(int(fz.sum()))) + u / M
            assert np.array_equal(prob, want)
            assert cdf[-1] == LAST == np.float32(1.000001) and (np.diff(cdf) >= 0).all() and abs(float(prob.sum()) - 1.0) < 1e-12
            if u == 0.0:                                            # the invariant: a clip without a failure has probability 0 exactly and no width in the CDF
                z = np.flatnonzero(fz == 0)
                assert (prob[z] == 0).all()
                full = np.cumsum(prob).astype(np.float32)
                assert (full[z[z > 0]] == full[z[z > 0] - 1]).all() and (0 not in z or full[0] == 0)
    with pytest.raises(ValueError):
        clip_sampling_cdf_host(_counts([1]), 1.5)
    with pytest.raises(ValueError):
        clip_sampling_cdf_host(_counts([1]), float("nan"))


def test_cdf_without_mix_is_the_librarys_own_host_cdf(emu_backend):
    """u = 0 against MotionLibSMPL: set_termination_history + load_motions(random_sample=False) give the same float32 sampling_cdf, bit for bit, on the weight sets
    of the resample check; a ClipOutcomes seeded from that history holds those counts and its apply() leaves the library's CDF as it is, in the same storage."""
    import motion_edge_cases as E
    from smplsim_amd.learning.clip_sampling import ClipOutcomes, clip_sampling_cdf_host
    lib, _ = E.build_lib(24)
    for w in E.RESAMPLE_WEIGHTS:
        lib.set_termination_history({"termination_history": np.array(w, np.float64), "failed_keys": []})
        lib.load_motions(random_sample=False)
        want = lib.sampling_cdf.numpy().copy()
        cdf, prob = clip_sampling_cdf_host(_counts(w), 0.0)
        assert np.array_equal(cdf.view(np.uint32), want.view(np.uint32)), w
        assert np.array_equal(prob > 0, np.array(w) > 0)
        co = ClipOutcomes(lib, uniform_mix=0.0)
        assert co.counts.dtype == torch.int64 and co.counts[:, 0].tolist() == list(w) and not co.counts[:, 1:].any()
        ptr = lib.sampling_cdf.data_ptr()
        p = co.apply()
        assert lib.sampling_cdf.data_ptr() == ptr and np.array_equal(lib.sampling_cdf.numpy().view(np.uint32), want.view(np.uint32))
        assert np.array_equal(p.numpy(), prob)


# ---------------------------------------------------------------------------------------------------------------- 3: the owner object on the host
def test_owner_object_on_the_host(emu_backend):
    import motion_edge_cases as E
    from smplsim_amd.learning.clip_sampling import ClipOutcomes, clip_sampling_cdf_host
    lib, _ = E.build_lib(24)
    M = lib.num_current_motions()
    co = ClipOutcomes(lib, uniform_mix=0.25)
    assert co.counts.shape == (M, 3) and not co.counts.any() and torch.equal(co.prob, torch.full((M,), 1.0 / M, dtype=torch.float64))
    ids = torch.tensor([[0, 3, 3], [0, 3, 5], [6, 3, M]], dtype=torch.int32)
    dead = torch.tensor([[0, 1, 0], [0, 0, 0], [0, 1, 1]], dtype=torch.bool)
    done = torch.tensor([[0, 1, 0], [1, 0, 0], [0, 1, 1]], dtype=torch.bool)
    co.update(ids, dead, done)
    want = np.zeros((M, 3), np.int64)
    want[0], want[3], want[5], want[6] = (0, 1, 2), (2, 0, 4), (0, 0, 1), (0, 0, 1)
    assert np.array_equal(co.counts.numpy(), want)
    t = co.as_tensors()
    assert set(t) == {"clips_failed", "failed_episodes", "completed_episodes", "min_clip_prob", "max_clip_prob"} and all(v.dim() == 0 for v in t.values())
    assert (int(t["clips_failed"]), int(t["failed_episodes"]), int(t["completed_episodes"])) == (1, 2, 1)
    ptr = lib.sampling_cdf.data_ptr()
    prob = co.apply()
    cdf, p = clip_sampling_cdf_host(want, 0.25)
    assert lib.sampling_cdf.data_ptr() == ptr and np.array_equal(lib.sampling_cdf.numpy().view(np.uint32), cdf.view(np.uint32)) and np.array_equal(prob.numpy(), p)
    t = co.as_tensors()
    assert float(t["min_clip_prob"]) == 0.25 / M and float(t["max_clip_prob"]) == 0.75 * 1.0 + 0.25 / M
    co.update(ids, dead, done)                                      # the totals are those of the LAST update; the counters add up
    assert np.array_equal(co.counts.numpy(), 2 * want) and int(co.as_tensors()["failed_episodes"]) == 2
    # the one read-back: the host history follows, at the unique-clip indices
    co.sync_to_host()
    h = lib.get_termination_history()
    assert h["termination_history"].tolist() == [0, 0, 0, 4, 0, 0, 0] and h["failed_keys"] == ["d"]
    assert lib._sampling_prob.tolist() == [0, 0, 0, 1, 0, 0, 0] and lib._sampling_batch_prob.tolist() == [0, 0, 0, 1, 0, 0, 0]
    co.sync_to_host()                                               # nothing new: nothing is added twice
    assert lib.get_termination_history()["termination_history"].tolist() == [0, 0, 0, 4, 0, 0, 0] and lib.curr_failed_keys == []
    # wrong inputs
    for bad in ((ids.long(), dead, done), (ids, dead.float(), done), (ids, dead, done[:2]), (ids[0], dead[0], done[0])):
        with pytest.raises(ValueError, match="ClipOutcomes"):
            co.update(*bad)
    with pytest.raises(ValueError, match="uniform_mix"):
        ClipOutcomes(lib, uniform_mix=-0.1)


def test_a_reload_reseeds_from_the_host_history_and_duplicates_add_up(emu_backend):
    import motion_edge_cases as E
    from smplsim_amd.learning.clip_sampling import ClipOutcomes
    lib, _ = E.build_lib(24)
    lib.set_termination_history({"termination_history": np.array([0, 2, 0, 0, 5, 0, 0], np.float64), "failed_keys": []})
    lib.load_motions(num_motions=9, random_sample=False, start_idx=3)          # loaded position j -> unique clip (j + 3) % 7: clips 3 and 4 are loaded twice
    co = ClipOutcomes(lib, uniform_mix=0.0)
    assert lib._curr_motion_ids.tolist() == [3, 4, 5, 6, 0, 1, 2, 3, 4]
    assert co.counts[:, 0].tolist() == [0, 5, 0, 0, 0, 2, 0, 0, 5] and co.num_clips == 9
    ones = torch.ones(1, 3, dtype=torch.bool)
    co.update(torch.tensor([[1, 8, 7]], dtype=torch.int32), ones, ones)        # clip 4 fails on both of its positions, clip 3 on its second
    co.apply()
    assert lib.sampling_cdf.shape == (9,)
    co.sync_to_host()
    assert lib.get_termination_history()["termination_history"].tolist() == [0, 2, 0, 1, 7, 0, 0]
    assert sorted(lib.curr_failed_keys) == ["d", "e"]
    lib.load_motions(random_sample=False)                                       # another batch: the next call re-seeds, with the new size
    co.update(torch.tensor([[0]], dtype=torch.int32), ones[:, :1], ones[:, :1])
    assert co.counts[:, 0].tolist() == [1, 2, 0, 1, 7, 0, 0] and co.counts[:, 2].tolist() == [1, 0, 0, 0, 0, 0, 0]


# ---------------------------------------------------------------------------------------------------------------- 4: the switch
def test_the_flag_is_off_by_default_and_needs_an_imitation_env():
    from smplsim_amd.agents.ppo import AgentPPO, PPOConfig
    from test_episode_stats_cpu import ToyEnv
    assert PPOConfig().clip_sampling is False and PPOConfig().clip_sampling_mix == 0.1
    off = AgentPPO(ToyEnv(), PPOConfig(hidden=(16,)), seed=3)
    assert off.clip_outcomes is None and "clip_ids" not in off.sample(horizon=3)
    with pytest.raises(ValueError, match="clip_sampling"):
        AgentPPO(ToyEnv(), PPOConfig(hidden=(16,), clip_sampling=True), seed=3)

    class WithClips(ToyEnv):
        motion_lib, motion_ids = object(), torch.zeros(ToyEnv.num_envs, dtype=torch.int32)

    for mix in (-0.01, 1.5, float("nan")):
        with pytest.raises(ValueError, match="clip_sampling_mix"):
            AgentPPO(WithClips(), PPOConfig(hidden=(16,), clip_sampling=True, clip_sampling_mix=mix), seed=3)


def test_agent_records_clips_and_reweights_the_env_on_the_emulator(emu_backend, monkeypatch):
    """The agent's glue on the host: buf['clip'] holds motion_ids BEFORE every step, the counters equal the tally of the returned rows, the env's CDF is rewritten
    in its storage, the log line carries the new keys, the pipelined sampler refuses, and recording changes nothing the sampler computes."""
    import motion_edge_cases as E
    from smplsim_amd.agents import ppo
    from smplsim_amd.imitation import SMPLSimImitationVecEnv
    from smplsim_amd.learning.clip_sampling import clip_outcomes_host, clip_sampling_cdf_host
    from test_minibatch_cpu import _cpu_gae
    monkeypatch.setattr(ppo, "estimate_advantages_columns", _cpu_gae)
    N, T = 4, 4
    batches, agents = [], []
    for flag in (True, False):
        lib, _ = E.build_lib(24)
        env = SMPLSimImitationVecEnv(N, lib, seed=2, termination_distance=0.05)      # zero-mean actions of a fresh policy: envs fall behind their clips at once
        agent = ppo.AgentPPO(env, ppo.PPOConfig(hidden=(16,), opt_num_epochs=1, clip_sampling=flag, clip_sampling_mix=0.0), seed=1)
        ptr = lib.sampling_cdf.data_ptr()
        batches.append(agent.sample(horizon=T))
        agents.append(agent)
        assert lib.sampling_cdf.data_ptr() == ptr
    (b_on, b_off), (on, off) = batches, agents
    assert set(b_on) == set(b_off) | {"clip_ids"} and off.clip_outcomes is None
    for k in b_off:
        assert torch.equal(b_on[k], b_off[k]), k
    ids, dead, done = b_on["clip_ids"].numpy(), b_on["not_dead"].numpy() == 0, b_on["not_done"].numpy() == 0
    assert ids.shape == (T, N) and ids.dtype == np.int32 and dead.any()
    M = on.env.motion_lib.num_current_motions()
    want = clip_outcomes_host(ids, dead, done, np.zeros((M, 3), np.int64))
    assert np.array_equal(on.clip_outcomes.counts.numpy(), want) and want[:, 2].sum() == T * N
    assert np.array_equal(on.env.motion_lib.sampling_cdf.numpy().view(np.uint32), clip_sampling_cdf_host(want, 0.0)[0].view(np.uint32))
    # an env that ended at step t tracks, from step t + 1 on, the clip the step drew for it: the recorded id of step t is the one it ENDED on
    nxt = np.concatenate([ids[1:], on.env.motion_ids.numpy()[None]])
    assert (ids[~done] == nxt[~done]).all()
    info = on.update_params(b_on)
    assert int(info["failed_episodes"]) == dead.sum() and int(info["clips_failed"]) == (want[:, 0] > 0).sum() and info["max_clip_prob"].dim() == 0
    assert "clips_failed" not in off.update_params(b_off)
    with pytest.raises(ValueError, match="clip_sampling"):
        on.sample_pipelined(None)


# ---------------------------------------------------------------------------------------------------------------- 5: the library's exports and argument checks
@pytest.fixture(scope="module")
def L():
    from smplsim_amd import _cabi, _lib
    _lib.build()
    lib = _cabi.bind_mlp(ctypes.CDLL(_lib.LIB_PATH))
    lib.ss_last_error.restype = ctypes.c_char_p
    return lib


ONE = 16                                                            # a pointer value that is never dereferenced: every call below fails its checks first


def test_entries_are_exported_and_declared():
    from smplsim_amd import _cabi
    header = open(os.path.join(ROOT, "include", "smplsim_mlp.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("ss_clip_outcomes", "ss_clip_sampling_cdf"):
        assert name in _cabi.MLP_EXPORTS and re.search(r"\bint %s\s*\(" % name, code), name
    assert re.search(r"enum\s*\{\s*SS_CLIP_FAILED,\s*SS_CLIP_COMPLETED,\s*SS_CLIP_STEPS,", code) and _cabi.CLIP_COLUMNS == ("failed", "completed", "steps")


def test_clip_outcomes_checks_its_arguments_before_any_launch(L):
    def call(ids=ONE, dead=ONE, done=ONE, T=3, N=5, M=7, counts=ONE):
        return L.ss_clip_outcomes(ids, dead, done, T, N, M, counts, None)
    bad = [(dict(ids=None), b"null argument"), (dict(dead=None), b"null argument"), (dict(done=None), b"null argument"), (dict(counts=None), b"null argument"),
           (dict(T=0), b"T >= 1"), (dict(T=-1), b"T >= 1"), (dict(N=0), b"N >= 1"), (dict(N=-5), b"N >= 1"), (dict(M=0), b"M >= 1"), (dict(M=-1), b"M >= 1"),
           (dict(counts=20), b"counts must be 8-byte aligned"), (dict(counts=17), b"counts must be 8-byte aligned")]
    for kw, msg in bad:
        assert call(**kw) == -1 and msg in L.ss_last_error(), (kw, L.ss_last_error())


def test_clip_sampling_cdf_checks_its_arguments_before_any_launch(L):
    def call(counts=ONE, M=7, u=0.1, cdf=ONE, prob=ONE):
        return L.ss_clip_sampling_cdf(counts, M, u, cdf, prob, None)
    bad = [(dict(counts=None), b"null argument"), (dict(cdf=None), b"null argument"), (dict(M=0), b"M >= 1"), (dict(M=-2), b"M >= 1"),
           (dict(u=-1e-9), b"uniform_mix must lie in [0, 1]"), (dict(u=1.0000001), b"uniform_mix must lie in [0, 1]"), (dict(u=float("nan")), b"uniform_mix must lie in [0, 1]"),
           (dict(u=float("inf")), b"uniform_mix must lie in [0, 1]")]
    for kw, msg in bad:
        assert call(**kw) == -1 and msg in L.ss_last_error(), (kw, L.ss_last_error())
