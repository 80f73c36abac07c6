"""Device bits of the step kernels across the change that requests a tree level's record one level ahead (aba_solve): the control
steps of tests/golden/sweep_prefetch_gpu.npz replayed on the library under test, bit for bit.  The fixture was recorded on an MI355X
with the library of the commit BEFORE the change (tests/golden/make_sweep_prefetch_gpu.py, which imports the cases and the replay from
here): 8 SMPL envs (fixed-layout kernel, levels of 2 4 5 4 4 4 nodes), 4 SMPL-X envs (two passes, 12-node levels) and the 8 SMPL envs
again with body-body contacts (runtime tree, dense solve), 3 control steps each, standing envs and envs dropped onto the floor.  Every
step starts from the pre-step state the fixture holds, so a step that differs does not hide the next."""
import os

import numpy as np
import pytest

from helpers import GOLDEN, model_const

FIXTURE = os.path.join(GOLDEN, "sweep_prefetch_gpu.npz")
STEPS = 3
PRE = ("qpos", "qvel", "qpos_prev", "qvel_prev", "qacc_warm")
POST = ("qpos", "qvel", "solver_iters")
# name: (humanoid, envs, self_collision, seed, root heights)
CASES = {"smpl": ("smpl_humanoid", 8, False, 31, (0.94, 0.93, 0.92, 0.60, 0.45, 0.30, 0.95, 0.70)),
         "smplx": ("smplx_humanoid", 4, False, 32, (0.94, 0.92, 0.60, 0.35)),
         "smpl_selfcol": ("smpl_humanoid", 8, True, 33, (0.94, 0.93, 0.92, 0.60, 0.45, 0.30, 0.95, 0.70))}


def make_env(name):
    from smplsim_amd.batch import SMPLSimVecEnv
    humanoid, n, selfcol, _, _ = CASES[name]
    env = SMPLSimVecEnv(n, humanoid=humanoid, autoreset=False, self_collision=selfcol)
    env.reset()
    return env


def start_state(name, env):
    """Start state and actions of a case (the generator's side: the test takes them from the fixture)."""
    humanoid, n, _, seed, heights = CASES[name]
    mc = model_const(humanoid)
    rs = np.random.default_rng(seed)
    acts = rs.uniform(-0.5, 0.5, (STEPS, n, mc.nu)).astype(np.float32)
    q = env.qpos.cpu().numpy().copy()
    q[:, 2] = heights
    q[:, 7:] += rs.uniform(-0.1, 0.1, (n, mc.nq - 7)).astype(np.float32)
    v = (rs.normal(size=(n, mc.nv)) * 0.2).astype(np.float32)
    return q.astype(np.float32), v, acts


def step_from(env, pre, act):
    """One control step from the pre-step state `pre` (arrays by the names of PRE): the post-step arrays by the names of POST."""
    import torch
    env.set_state(pre["qpos"], pre["qvel"], pre["qpos_prev"], pre["qvel_prev"], pre["qacc_warm"])
    env.step(torch.as_tensor(act, dtype=torch.float32, device=env.device))
    torch.cuda.synchronize()
    return {k: getattr(env, k).cpu().numpy().copy() for k in POST}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_recorded_steps_keep_their_device_bits(name):
    pytest.importorskip("torch")
    fx = np.load(FIXTURE)                                     # (a missing fixture is an error)
    env = make_env(name)
    for t in range(STEPS):
        pre = {k: fx[f"{name}/pre{t}/{k}"] for k in PRE}
        post = step_from(env, pre, fx[f"{name}/act{t}"])
        iters = fx[f"{name}/post{t}/solver_iters"]
        print(name, "step", t, "Newton iterations recorded", iters.tolist(), "now", post["solver_iters"].tolist())
        for k in POST:
            want = fx[f"{name}/post{t}/{k}"]
            assert post[k].dtype == want.dtype and np.array_equal(bits(post[k]), bits(want)), (name, t, k)
    # the fixture does what it is for: contacts (more than one Newton iteration per mj_step) in the dropped envs, finite states
    assert min(fx[f"{name}/post{t}/solver_iters"].max() for t in range(2)) > 15 and np.isfinite(fx[f"{name}/post{STEPS - 1}/qpos"]).all()
