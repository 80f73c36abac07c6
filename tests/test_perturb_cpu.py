"""smplsim_amd.perturb.RandomPushes on CPU tensors: the schedule it writes into xfrc_applied (no GPU, no stepper)."""
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from smplsim_amd.perturb import RandomPushes  # noqa: E402

N, NBODY = 7, 24
BODIES, LO, HI, A, B, K = [0, 3, 9], 50.0, 300.0, 5, 9, 3


def _rollout(seed, steps=120, **kw):
    env = types.SimpleNamespace(xfrc_applied=torch.zeros(N, NBODY, 6))
    args = dict(bodies=BODIES, force=(LO, HI), interval=(A, B), duration=K, seed=seed)
    args.update(kw)
    p = RandomPushes(env, **args)
    rec, act = [], []
    for _ in range(steps):
        m = p.before_step()
        rec.append(env.xfrc_applied.clone().numpy()); act.append(m.numpy().copy())
    return np.array(rec), np.array(act)


def test_schedule():
    X, act = _rollout(3)
    mag = np.linalg.norm(X[..., :3], axis=-1)                  # [T, N, nbody]
    pushed = mag.max(axis=-1) > 0
    assert np.array_equal(pushed, act)                         # the returned mask is what was written
    assert not X[..., 3:].any()                                # forces only
    others = [b for b in range(NBODY) if b not in BODIES]
    assert not X[:, :, others].any()                           # only the listed bodies
    assert ((mag > 0).sum(axis=-1) <= 1).all()                 # one body at a time
    seen = set()
    for n in range(N):
        starts = [t for t in range(len(X)) if pushed[t, n] and (t == 0 or not pushed[t - 1, n] or not np.array_equal(X[t, n], X[t - 1, n]))]
        assert len(starts) >= 10
        assert A <= starts[0] <= B                             # the first push: after a drawn interval
        gaps = np.diff(starts)
        assert gaps.min() >= A and gaps.max() <= B             # start to start within [a, b]
        for t in starts:
            if t + K <= len(X):
                for j in range(1, K):
                    assert np.array_equal(X[t + j, n], X[t, n])    # held unchanged for k steps
                assert t + K == len(X) or not pushed[t + K, n] or t + K in starts   # then zero until the next one starts
            m = mag[t, n].max()
            assert LO - 1e-3 <= m <= HI + 1e-3                 # magnitudes within [lo, hi]
            seen.add(int(mag[t, n].argmax()))
        assert pushed[:, n].sum() <= K * len(starts)
    assert seen == set(BODIES)                                 # every listed body is drawn
    assert len({tuple(np.flatnonzero(pushed[:, n])[:12]) for n in range(N)}) > 1   # the envs have schedules of their own


def test_same_seed_same_schedule():
    a, b, c = _rollout(5, 60)[0], _rollout(5, 60)[0], _rollout(6, 60)[0]
    assert np.array_equal(a, b) and not np.array_equal(a, c)


def test_fixed_magnitude_and_every_step_intervals():
    X, act = _rollout(1, 30, force=(80.0, 80.0), interval=(2, 2), duration=2)
    assert act[2:].all() and not act[:2].any()                 # a = b = k: pushed all the time after the first interval
    mag = np.linalg.norm(X[2:, :, :, :3], axis=-1).max(axis=-1)
    assert np.allclose(mag, 80.0, rtol=1e-5)


def test_arguments():
    env = types.SimpleNamespace(xfrc_applied=torch.zeros(2, 4, 6))
    for kw in (dict(bodies=[4]), dict(bodies=[]), dict(bodies=[0], duration=3, interval=(2, 5)), dict(bodies=[0], force=(5.0, 1.0)), dict(bodies=[0], interval=(4, 3))):
        with pytest.raises(ValueError):
            RandomPushes(env, **kw)
    made = []
    env2 = types.SimpleNamespace(xfrc_applied=None, enable_body_wrenches=lambda: made.append(1) or torch.zeros(2, 4, 6),
                                 model=types.SimpleNamespace(mc=types.SimpleNamespace(body_names=["a", "b", "c", "d"])))
    p = RandomPushes(env2, bodies=["c", 1])                    # names are looked up; the input is enabled when it is off
    assert made == [1] and p.bodies.tolist() == [2, 1]
