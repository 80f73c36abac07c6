"""Failure-weighted clip sampling on the GPU (include/smplsim_mlp.h: ss_clip_outcomes, ss_clip_sampling_cdf; learning/clip_sampling.py; PPOConfig.clip_sampling)
against the NumPy restatements of learning/clip_sampling.py (checked on their own in test_clip_sampling_cpu.py).

Nothing here takes a tolerance: the counters are integers (all 3 M int64 values equal), the CDF and the probabilities are compared bit for bit (uint32 / uint64
views) — every fp64 operation of the definition is rounded on its own and the running sum has numpy.cumsum's order."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from test_gemm_kernels_gpu import _lib, _p, _st  # noqa: E402

I32_MAX = 2 ** 31 - 1
BIG = 2 ** 40
GUARD = -(2 ** 62) - 12345                          # the guard row behind counts
SENT = -7.75e7                                      # behind cdf and prob (exact in float32)
SHAPES = [(1, 1), (37, 65), (26, 515), (3, 64)]     # one element; an odd T with one column beyond a wavefront; nine wavefronts, the last with 3 columns; exactly one, T below the unroll
CLIPS = [1, 7, 5000]                                # the tally has no size switch


def _host():
    from smplsim_amd.learning import clip_sampling
    return clip_sampling


def _rollout(T, N, M, pattern, seed):
    """ids with -1, M and INT32_MAX among them; dead / done random, or all ones, or all zeros."""
    g = np.random.default_rng(seed)
    ids = g.integers(0, M, size=(T, N)).astype(np.int32)
    if M > 1:                                        # runs of one clip, as an env has them: a column keeps its id for a few steps
        keep = g.random((T, N)) < 0.7
        for t in range(1, T):
            ids[t] = np.where(keep[t], ids[t - 1], ids[t])
    odd = g.random((T, N))
    ids[odd < 0.06] = -1
    ids[(odd >= 0.06) & (odd < 0.12)] = M
    ids[(odd >= 0.12) & (odd < 0.18)] = I32_MAX
    ids[(odd >= 0.18) & (odd < 0.2)] = -(2 ** 31)
    if pattern == "random":
        dead, done = g.random((T, N)) < 0.15, g.random((T, N)) < 0.3
    else:
        dead = done = np.full((T, N), pattern == "ones")
    return ids, dead, done


class _Tally:
    """The device side of ss_clip_outcomes: the inputs as the heads of buffers with one more [N] plane behind their last element (valid ids, flags set: a read
    beyond T * N would be counted), the counters preset to 2^40 + j with a guard row behind them."""

    def __init__(self, ids, dead, done, M):
        self.T, self.N, self.M = ids.shape[0], ids.shape[1], M
        pad = lambda a, fill: torch.from_numpy(np.concatenate([a, np.full((1, self.N), fill, a.dtype)])).cuda()  # noqa: E731
        self.ids, self.dead, self.done = pad(ids, 0), pad(dead, True), pad(done, True)
        self.inputs = [t.clone() for t in (self.ids, self.dead, self.done)]
        self.preset = BIG + np.arange(3 * M, dtype=np.int64).reshape(M, 3)
        self.counts = torch.from_numpy(np.concatenate([self.preset, np.full((1, 3), GUARD, np.int64)])).cuda()

    def run(self):
        L = _lib()
        rc = L.ss_clip_outcomes(_p(self.ids), _p(self.dead), _p(self.done), self.T, self.N, self.M, _p(self.counts), _st())
        assert rc == 0, L.ss_last_error()
        torch.cuda.synchronize()
        got = self.counts.cpu().numpy()
        assert (got[self.M] == GUARD).all(), "a write behind counts[M - 1]"
        for a, b in zip(self.inputs, (self.ids, self.dead, self.done)):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), "an input was written"
        return got[:self.M]


# ---------------------------------------------------------------------------------------------------------------- 1: the tally
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_outcomes_equal_the_host_tally(shape):
    T, N = shape
    H = _host()
    for M in CLIPS:
        for pattern in ("random", "ones", "zeros"):
            ids, dead, done = _rollout(T, N, M, pattern, seed=1000 * T + N + M)
            call = _Tally(ids, dead, done, M)
            inc = H.clip_outcomes_host(ids, dead, done, np.zeros((M, 3), np.int64))
            valid = int(((ids >= 0) & (ids < M)).sum())
            assert inc[:, 2].sum() == valid and inc[:, 0].sum() == {"ones": valid, "zeros": 0}.get(pattern, inc[:, 0].sum())
            got = call.run()
            print(f"T={T} N={N} M={M} {pattern}: {valid} of {T * N} ids inside, failed {inc[:, 0].sum()} completed {inc[:, 1].sum()}")
            assert np.array_equal(got, call.preset + inc), (M, pattern)            # 64-bit adds: a 32-bit one would lose the 2^40
            assert np.array_equal(call.run(), call.preset + 2 * inc), (M, pattern)   # accumulated, never zeroed: a second call doubles the increments


def test_outcomes_take_byte_flags_like_bools_and_long_columns():
    """uint8 flags of any non-zero value; T = 70 (no multiple of the unroll) x N = 130 with ONE clip held by every env: a lane holds its steps back in a register until its
    episode ends, and all lanes add to the same three counters."""
    T, N, M = 70, 130, 3
    g = np.random.default_rng(9)
    ids = np.full((T, N), 2, np.int32)
    dead, done = (g.random((T, N)) < 0.02).astype(np.uint8) * 255, (g.random((T, N)) < 0.05).astype(np.uint8) * 2
    call = _Tally(ids, dead, done, M)
    inc = _host().clip_outcomes_host(ids, dead, done, np.zeros((M, 3), np.int64))
    assert inc[2, 2] == T * N and not inc[:2].any()
    assert np.array_equal(call.run(), call.preset + inc)


def test_outcomes_error_paths_leave_the_counters_alone():
    L = _lib()
    ids, dead, done = _rollout(3, 5, 7, "ones", seed=1)
    c = _Tally(ids, dead, done, 7)
    before = c.counts.clone()
    odd = C.c_void_p(c.counts.data_ptr() + 4)
    calls = [(None, _p(c.dead), _p(c.done), 3, 5, 7, _p(c.counts)), (_p(c.ids), None, _p(c.done), 3, 5, 7, _p(c.counts)),
             (_p(c.ids), _p(c.dead), None, 3, 5, 7, _p(c.counts)), (_p(c.ids), _p(c.dead), _p(c.done), 3, 5, 7, None),
             (_p(c.ids), _p(c.dead), _p(c.done), 0, 5, 7, _p(c.counts)), (_p(c.ids), _p(c.dead), _p(c.done), 3, 0, 7, _p(c.counts)),
             (_p(c.ids), _p(c.dead), _p(c.done), 3, 5, 0, _p(c.counts)), (_p(c.ids), _p(c.dead), _p(c.done), -1, 5, 7, _p(c.counts)),
             (_p(c.ids), _p(c.dead), _p(c.done), 3, 5, 7, odd)]
    for args in calls:
        assert L.ss_clip_outcomes(*args, _st()) != 0 and len(L.ss_last_error()) > 0, args
    torch.cuda.synchronize()
    assert torch.equal(c.counts, before)


# ---------------------------------------------------------------------------------------------------------------- 2: the CDF
def _count_sets(M, seed):
    g = np.random.default_rng(seed)
    one = np.zeros(M, np.int64)
    one[g.integers(0, M)] = 3
    rand = g.integers(1, 1000, M) * (g.random(M) < 0.6)
    big = np.where(g.random(M) < 0.5, BIG, 0) + g.integers(0, 3, M)
    neg = rand.copy()
    neg[g.integers(0, M)] = -17
    return dict(zero=np.zeros(M, np.int64), one=one, random=rand, big=big, negative=neg)


def _device_cdf(counts, u, with_prob=True):
    M = counts.shape[0]
    d_counts = torch.from_numpy(counts).cuda()
    cdf = torch.full((M + 3,), SENT, dtype=torch.float32, device="cuda")
    prob = torch.full((M + 3,), SENT, dtype=torch.float64, device="cuda") if with_prob else None
    L = _lib()
    assert L.ss_clip_sampling_cdf(_p(d_counts), M, float(u), _p(cdf), _p(prob), _st()) == 0, L.ss_last_error()
    torch.cuda.synchronize()
    assert (cdf[M:] == SENT).all() and (prob is None or (prob[M:] == SENT).all()), "a write behind cdf[M - 1] / prob[M - 1]"
    assert torch.equal(d_counts, torch.from_numpy(counts).cuda())
    return cdf[:M].cpu().numpy(), None if prob is None else prob[:M].cpu().numpy()


@pytest.mark.parametrize("M", [1, 2, 7, 4097])
def test_cdf_equals_the_numpy_restatement_bit_for_bit(M):
    H = _host()
    for kind, failed in _count_sets(M, seed=M).items():
        counts = np.stack([failed, np.full(M, 777), np.full(M, 99999)], 1).astype(np.int64)       # completions and steps play no part
        for u in (0.0, 0.25, 1.0):
            want_cdf, want_prob = H.clip_sampling_cdf_host(counts, u)
            cdf, prob = _device_cdf(counts, u)
            bad_c, bad_p = int((cdf.view(np.uint32) != want_cdf.view(np.uint32)).sum()), int((prob.view(np.uint64) != want_prob.view(np.uint64)).sum())
            print(f"M={M} {kind} u={u}: cdf entries that differ {bad_c}, prob entries that differ {bad_p}, max |dprob| {np.abs(prob - want_prob).max():.3g}")
            assert bad_c == 0 and bad_p == 0, (kind, u)
            assert cdf[-1] == np.float32(1.0 + 1e-6) and (np.diff(cdf) >= 0).all()
            if u == 0.0 and failed.max() > 0:                          # the zero-weight invariant (with no failure at all the rule is uniform)
                z = np.flatnonzero(failed <= 0)
                assert (prob[z] == 0).all()
        cdf_only, none = _device_cdf(counts, 0.25, with_prob=False)  # prob = NULL
        assert none is None and np.array_equal(cdf_only.view(np.uint32), H.clip_sampling_cdf_host(counts, 0.25)[0].view(np.uint32)), kind


def test_cdf_error_paths_write_nothing():
    L = _lib()
    counts = torch.ones(7, 3, dtype=torch.int64, device="cuda")
    cdf = torch.full((7,), SENT, dtype=torch.float32, device="cuda")
    prob = torch.full((7,), SENT, dtype=torch.float64, device="cuda")
    calls = [(None, 7, 0.1, _p(cdf), _p(prob)), (_p(counts), 7, 0.1, None, _p(prob)), (_p(counts), 0, 0.1, _p(cdf), _p(prob)), (_p(counts), -7, 0.1, _p(cdf), _p(prob)),
             (_p(counts), 7, -0.5, _p(cdf), _p(prob)), (_p(counts), 7, 1.5, _p(cdf), _p(prob)), (_p(counts), 7, float("nan"), _p(cdf), _p(prob))]
    for args in calls:
        assert L.ss_clip_sampling_cdf(*args, _st()) != 0 and len(L.ss_last_error()) > 0, args
    torch.cuda.synchronize()
    assert (cdf == SENT).all() and (prob == SENT).all()


# ---------------------------------------------------------------------------------------------------------------- 3: the invariant
def test_no_draw_below_one_selects_a_clip_that_never_failed():
    """u = 0, counts with zeros: the device CDF searched by ss_motion_resample at its own entries, their float32 neighbours below, 0 and the largest float below 1
    (motion_edge_cases.resample_draws): the ids of oracle.motion_oracle.resample on the same CDF, and never a clip with f = 0 for a draw in [0, 1)."""
    import motion_edge_cases as E
    from oracle import motion_oracle as mo
    from smplsim_amd.learning.clip_sampling import ClipOutcomes
    lib, _ = E.build_lib(24)
    M = lib.num_current_motions()
    co = ClipOutcomes(lib, uniform_mix=0.0)
    rs = np.random.default_rng(41)
    for failed in ([0, 4, 0, 0, 1, 2 ** 40, 0], [3, 0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 9], [1, 1, 0, 1, 1, 0, 1]):
        co.counts.zero_()
        co.counts[:, 0] = torch.tensor(failed, device=co.counts.device)
        prob = co.apply().cpu().numpy()
        cdf = lib.sampling_cdf.cpu().numpy()
        assert np.array_equal(prob > 0, np.array(failed) > 0)
        n = 3 * (2 * M + 2) + 30
        mask = np.ones(n, bool)
        rand = E.resample_draws(rs, cdf, n, mask)
        ids = torch.full((n + E.GUARD,), -5, dtype=torch.int32, device=lib.device)
        t0 = torch.full((n + E.GUARD,), E.SENT, dtype=torch.float32, device=lib.device)
        d_rand = torch.from_numpy(rand).to(lib.device)
        L = _lib()
        assert L.ss_motion_resample(C.byref(lib.data), None, _p(d_rand), _p(lib.sampling_cdf), 0.0, n, _p(ids), _p(t0), lib._stream()) == 0, L.ss_last_error()
        torch.cuda.synchronize()
        ids = ids.cpu().numpy()
        want_ids, _ = mo.resample(rand, cdf, lib._motion_lengths, 0.0)
        assert (ids[n:] == -5).all() and np.array_equal(ids[:n], want_ids), failed
        legit = (rand[:, 0] >= 0) & (rand[:, 0] < 1)
        assert legit.sum() > 2 * M and (np.array(failed)[ids[:n][legit]] > 0).all(), failed
        assert set(np.unique(ids[:n][legit])) == set(np.flatnonzero(np.array(failed) > 0)), failed         # and every clip that failed is drawn


# ---------------------------------------------------------------------------------------------------------------- 4: the agent
def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _agent(flag):
    import motion_edge_cases as E
    from smplsim_amd.agents.ppo import AgentPPO, PPOConfig
    from smplsim_amd.imitation import SMPLSimImitationVecEnv
    lib, _ = E.build_lib(24)
    env = SMPLSimImitationVecEnv(64, lib, seed=5, termination_distance=0.05)      # the mean action of a fresh policy does not track a clip: envs fail within a few steps
    return AgentPPO(env, PPOConfig(hidden=(64, 64), min_batch_size=8 * 64, opt_num_epochs=1, clip_sampling=flag, clip_sampling_mix=0.0), seed=3)


def test_agent_tallies_reweights_and_resamples_end_to_end():
    H = _host()
    on = _agent(True)
    ml, co = on.env.motion_lib, on.clip_outcomes
    M, K = ml.num_current_motions(), 6
    ptr = ml.sampling_cdf.data_ptr()
    b = on.sample(horizon=8)
    ids, dead, done = b["clip_ids"].cpu().numpy(), b["not_dead"].cpu().numpy() == 0, b["not_done"].cpu().numpy() == 0
    want = H.clip_outcomes_host(ids, dead, done, np.zeros((M, 3), np.int64))
    print("counters after the first rollout (failed, completed, steps per clip):", want.tolist())
    assert ids.shape == (8, 64) and dead.sum() >= 8 and want[:, 2].sum() == 8 * 64
    assert np.array_equal(co.counts.cpu().numpy(), want)
    assert ml.sampling_cdf.data_ptr() == ptr and on.env._bound == ml.load_count                         # same storage: no rebind
    assert np.array_equal(ml.sampling_cdf.cpu().numpy().view(np.uint32), H.clip_sampling_cdf_host(want, 0.0)[0].view(np.uint32))
    info = on.update_params(b)
    assert int(info["failed_episodes"]) == dead.sum() and int(info["completed_episodes"]) == (done & ~dead).sum() and int(info["clips_failed"]) == (want[:, 0] > 0).sum()
    assert float(info["max_clip_prob"]) == want[:, 0].max() / want[:, 0].sum()
    # recording changes nothing the sampler computes: the flag off, same seeds, same first rollout
    b_off = _agent(False).sample(horizon=8)
    assert set(b) == set(b_off) | {"clip_ids"}
    for k in ("states", "actions", "rewards", "not_done", "not_dead"):
        assert _bits(b[k], b_off[k]), k
    # only clip K has failed: every env re-initialised from now on tracks clip K
    only = np.zeros((M, 3), np.int64)
    only[K, 0] = 5
    co.counts.copy_(torch.from_numpy(only))
    co.apply()
    b2 = on.sample(horizon=8)
    ids2, done2 = b2["clip_ids"].cpu().numpy(), b2["not_done"].cpu().numpy() == 0
    after = np.concatenate([ids2[1:], on.env.motion_ids.cpu().numpy()[None]])                            # the clip every env tracks AFTER step t
    print("re-initialised in the second rollout:", int(done2.sum()), "clips they got:", np.unique(after[done2]).tolist())
    assert done2.sum() >= 8 and (after[done2] == K).all() and (after[~done2] == ids2[~done2]).all()
    assert ml.sampling_cdf.data_ptr() == ptr
    # the one read-back: the host history is the per-unique-clip sum of the device counters (the library started from a history of zeros)
    counts = co.sync_to_host()
    assert np.array_equal(counts, only + H.clip_outcomes_host(ids2, b2["not_dead"].cpu().numpy() == 0, done2, np.zeros((M, 3), np.int64)))
    hist = np.zeros(ml.num_all_motions())
    np.add.at(hist, ml._curr_motion_ids, counts[:, 0].astype(np.float64))
    got = ml.get_termination_history()
    assert np.array_equal(got["termination_history"], hist) and hist[K] >= 5
    assert sorted(got["failed_keys"]) == sorted(ml._motion_data_keys[np.unique(ml._curr_motion_ids[counts[:, 0] > 0])].tolist())
