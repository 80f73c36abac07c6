"""Device bits of the step kernels across the change that turns the row code around the articulated-body solve (newton_prepare,
newton_finish, ls_eval, eval_rows, row_dcost) into straight-line code: the control steps of tests/golden/newton_rows_gpu.npz replayed
on the library under test, bit for bit.  The fixture was recorded on an MI355X with the library of the commit BEFORE the change
(tests/golden/make_newton_rows_gpu.py, which imports the cases and the replay from here), 3 control steps per case:

  smpl            8 SMPL envs (fixed-layout kernel): standing, dropped onto the floor, and two dropped envs with a joint beyond its
                  range, one in the first dof pass (dof 10) and one in the last (dof 70 of dofs 64 to 74)
  smplx           4 SMPL-X envs (three dof passes): the limit poses at dof 10 and dof 150
  smpl_selfcol    the 8 SMPL envs with body-body contacts
  getup           8 envs of the getup task from their Fall reset: lying on the floor, many contact rows
  smpl_iters3     the 8 SMPL envs with newton_iters = 3: the cap ends the loop

Every step starts from a state the fixture holds, so a step that differs does not hide the next: step 0 from start/<qpos qvel
qacc_warm>, step t + 1 from the recorded post-step state of step t, the stale copies (qpos_prev, qvel_prev) set to the same state as
a reset leaves them.  Start states and actions are multiples of 2^-8 where the case draws them, which keeps the file small."""
import os

import numpy as np
import pytest

from helpers import GOLDEN, model_const

FIXTURE = os.path.join(GOLDEN, "newton_rows_gpu.npz")
STEPS = 3
STATE = ("qpos", "qvel", "qacc_warm")
POST = STATE + ("solver_iters",)
BEYOND = 3.3                                                  # every hinge of both humanoids ends at +-pi (or +-4 pi)
SMPL_HEIGHTS = (0.94, 0.93, 0.92, 0.60, 0.45, 0.30, 0.55, 0.50)
SMPL_BEYOND = {6: (10, 1.0), 7: (70, -1.0)}                   # env: (dof beyond its range, sign)
# name: (humanoid, envs, seed, root heights or None = the state the reset left, {env: (dof, sign)}, env keywords)
CASES = {"smpl": ("smpl_humanoid", 8, 51, SMPL_HEIGHTS, SMPL_BEYOND, {}),
         "smplx": ("smplx_humanoid", 4, 52, (0.94, 0.60, 0.55, 0.50), {2: (10, -1.0), 3: (150, 1.0)}, {}),
         "smpl_selfcol": ("smpl_humanoid", 8, 53, SMPL_HEIGHTS, SMPL_BEYOND, {"self_collision": True}),
         "getup": ("smpl_humanoid", 8, 54, None, {}, {"task": "HumanoidGetup", "state_init": "Fall"}),
         "smpl_iters3": ("smpl_humanoid", 8, 55, SMPL_HEIGHTS, SMPL_BEYOND, {"newton_iters": 3})}


def make_env(name):
    from smplsim_amd.batch import SMPLSimVecEnv
    humanoid, n, _, _, _, kw = CASES[name]
    env = SMPLSimVecEnv(n, humanoid=humanoid, autoreset=False, **kw)
    env.reset()
    return env


def start_state(name, env):
    """Start state and actions of a case (the generator's side: the test takes them from the fixture)."""
    humanoid, n, seed, heights, beyond, _ = CASES[name]
    mc = model_const(humanoid)
    rs = np.random.default_rng(seed)
    coarse = lambda x: (np.round(x * 256) / 256).astype(np.float32)
    acts = coarse(rs.uniform(-0.5, 0.5, (STEPS, n, mc.nu)))
    q = env.qpos.cpu().numpy().copy()
    if heights is not None:
        q[:, 2] = heights
        q[:, 7:] += coarse(rs.uniform(-0.1, 0.1, (n, mc.nq - 7)))
    v = coarse(rs.normal(size=(n, mc.nv)) * 0.2)
    for e, (dof, sign) in beyond.items():
        q[e, dof + 1] = sign * BEYOND
    return {"qpos": q.astype(np.float32), "qvel": v, "qacc_warm": env.qacc_warm.cpu().numpy().copy()}, acts


def step_from(env, pre, act):
    """One control step from the state `pre` (arrays by the names of STATE): the post-step arrays by the names of POST."""
    import torch
    env.set_state(pre["qpos"], pre["qvel"], pre["qpos"], pre["qvel"], pre["qacc_warm"])
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
        pre = {k: fx[f"{name}/start/{k}" if t == 0 else f"{name}/post{t - 1}/{k}"] for k in STATE}
        post = step_from(env, pre, fx[f"{name}/act{t}"])
        iters = fx[f"{name}/post{t}/solver_iters"]
        print(name, "step", t, "Newton iterations recorded", iters.tolist(), "now", post["solver_iters"].tolist())
        for k in POST:
            want = fx[f"{name}/post{t}/{k}"]
            assert post[k].dtype == want.dtype and np.array_equal(bits(post[k]), bits(want)), (name, t, k)
    # the fixture does what it is for: the recorded steps did iterate (more than one Newton iteration per mj_step), finite states
    assert min(fx[f"{name}/post{t}/solver_iters"].max() for t in range(STEPS)) > 15 and np.isfinite(fx[f"{name}/post{STEPS - 1}/qpos"]).all()
