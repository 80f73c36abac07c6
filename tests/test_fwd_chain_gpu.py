"""Device bits of the forward pass across the change that moves forward_kin's chain sums onto one packed chain record per node
(ss_tables.h chain_records; the ancestor walk on the same record moved these bits and is not in the tree): the cases of tests/golden/fwd_chain_gpu.npz replayed on the library under test, bit for
bit.  The fixture was recorded on an MI355X with the library of the commit BEFORE the change (tests/golden/make_fwd_chain_gpu.py, which
imports the cases and the replay from here).  Per case, from the start state the fixture holds: ss_debug_forward (mass matrix, bias,
acceleration), ss_kinematics (positions, orientations), then 2 control steps with the post-step state, the body velocities, the
Newton iterations and the observation of each:

  smpl            8 SMPL envs (fixed-layout kernel)
  smplx           4 SMPL-X envs
  shaped          8 SMPL envs of three body shapes: the walk takes its offsets from the env's own table
  bodyout         the 8 SMPL envs with the power output: the body-output instantiation
  getup           8 envs of the getup task; their Fall reset runs on the library under test (draws: reset_draws), and the state it
                  leaves is compared too (the reset's forward passes)
  selfcol         the 8 SMPL envs with body-body contacts

Joint angles, velocities and the warm start are non-zero multiples of 2^-8 in every body; env 1 of every case has the joints on the
chain to its deepest body (a hand, a finger tip) turned by 0.5 to 1 rad each, so that the product of rotations the walk forms is far
from the identity.  Every step starts from a state the fixture holds (the recorded post-step state of the step before)."""
import os

import numpy as np
import pytest

from helpers import GOLDEN, model_const

FIXTURE = os.path.join(GOLDEN, "fwd_chain_gpu.npz")
STEPS = 2
STATE = ("qpos", "qvel", "qacc_warm")
POST = STATE + ("solver_iters", "body_vel", "obs")
FORWARD = ("M", "bias", "qacc", "xpos", "xmat")
SMPL_HEIGHTS = (0.94, 0.93, 0.60, 0.45, 0.92, 0.30, 0.55, 0.50)
SHAPES = ((1.0, {}), (0.9, {"L_Knee": 1.1, "R_Knee": 1.1}), (1.08, {"Chest": 0.9, "L_Elbow": 1.2}))
# name: (humanoid, envs, seed, root heights or None = the state the reset left, env keywords)
CASES = {"smpl": ("smpl_humanoid", 8, 61, SMPL_HEIGHTS, {}),
         "smplx": ("smplx_humanoid", 4, 62, (0.94, 0.60, 0.55, 0.50), {}),
         "shaped": ("smpl_humanoid", 8, 63, SMPL_HEIGHTS, {}),
         "bodyout": ("smpl_humanoid", 8, 64, SMPL_HEIGHTS, {}),
         "getup": ("smpl_humanoid", 8, 65, None, {"task": "HumanoidGetup", "state_init": "Fall"}),
         "selfcol": ("smpl_humanoid", 8, 66, SMPL_HEIGHTS, {"self_collision": True})}


def deepest_chain_dofs(mc):
    """Hinge dofs (indices into qvel) of the bodies on the chain from the root to the deepest body, the root's own excluded."""
    parent = [int(p) for p in mc.body_parent]
    depth = [0] * mc.nbody
    for b in range(1, mc.nbody):
        depth[b] = depth[parent[b]] + 1
    b, dofs = int(np.argmax(depth)), []
    while b > 0:
        dofs += [6 + 3 * (b - 1) + j for j in range(3)]
        b = parent[b]
    return sorted(dofs)


def reset_draws(name):
    """The uniform draws of the case's reset (Fall actions, task targets) and of its steps' task targets, or None where the case has none."""
    humanoid, n, seed, _, kw = CASES[name]
    rs = np.random.default_rng(1000 + seed)
    fall = rs.uniform(size=(n, 3, model_const(humanoid).nu)).astype(np.float32)
    task = rs.uniform(size=(1 + STEPS, n, 4)).astype(np.float32)
    return (fall if kw.get("state_init") == "Fall" else None), (task if "task" in kw else None)


def make_env(name):
    """The case's env after its reset."""
    import torch
    from smplsim_amd.batch import ShardModel, SMPLSimVecEnv
    from smplsim_amd.mjcf_writer import scaled_xml_str
    humanoid, n, _, _, kw = CASES[name]
    if name == "shaped":
        env = SMPLSimVecEnv(n, model=ShardModel(xmls=[scaled_xml_str(humanoid, s, d) for s, d in SHAPES]), autoreset=False, **kw)
    else:
        env = SMPLSimVecEnv(n, humanoid=humanoid, autoreset=False, **kw)
    if name == "bodyout":
        env.enable_power_usage()
    fall, task = reset_draws(name)
    as_t = lambda x: None if x is None else torch.as_tensor(x, dtype=torch.float32, device=env.device)
    env.reset(fall_actions=as_t(fall), task_rand=as_t(None if task is None else task[0]))
    torch.cuda.synchronize()
    return env


def start_state(name, env):
    """Start state and actions of a case (the generator's side: the test takes them from the fixture)."""
    humanoid, n, seed, heights, _ = CASES[name]
    mc = model_const(humanoid)
    rs = np.random.default_rng(seed)
    coarse = lambda x: (np.round(x * 256) / 256).astype(np.float32)
    nonzero = lambda x: np.where(x == 0, np.float32(1.0 / 256), x).astype(np.float32)
    acts = coarse(rs.uniform(-0.5, 0.5, (STEPS, n, mc.nu)))
    q = env.qpos.cpu().numpy().copy()
    if heights is not None:
        q[:, 2] = heights
    q[:, 7:] += nonzero(coarse(rs.uniform(-0.1, 0.1, (n, mc.nq - 7))))
    chain = np.array(deepest_chain_dofs(mc))
    far = coarse(rs.uniform(0.5, 1.0, len(chain)) * rs.choice([-1.0, 1.0], len(chain)))
    q[1, chain + 1] = far
    v = nonzero(coarse(rs.normal(size=(n, mc.nv)) * 0.2))
    warm = nonzero(coarse(rs.normal(size=(n, mc.nv)) * 2.0))
    return {"qpos": q.astype(np.float32), "qvel": v, "qacc_warm": warm}, acts


def forward_from(env, pre):
    """ss_debug_forward and ss_kinematics at the state `pre`: the arrays by the names of FORWARD."""
    import torch
    env.set_state(pre["qpos"], pre["qvel"], pre["qpos"], pre["qvel"], pre["qacc_warm"])
    M, bias, qacc = env.debug_forward(torch.zeros(env.num_envs, env.nu, device=env.device))
    xpos, xmat = env.kinematics()
    torch.cuda.synchronize()
    return {k: x.cpu().numpy().copy() for k, x in zip(FORWARD, (M, bias, qacc, xpos, xmat))}


def step_from(env, pre, act, task_rand=None):
    """One control step from the state `pre` (arrays by the names of STATE): the post-step arrays by the names of POST."""
    import torch
    env.set_state(pre["qpos"], pre["qvel"], pre["qpos"], pre["qvel"], pre["qacc_warm"])
    tr = None if task_rand is None else torch.as_tensor(task_rand, dtype=torch.float32, device=env.device)
    obs = env.step(torch.as_tensor(act, dtype=torch.float32, device=env.device), task_rand=tr)[0]
    torch.cuda.synchronize()
    post = {k: getattr(env, k).cpu().numpy().copy() for k in POST if k != "obs"}
    post["obs"] = obs.cpu().numpy().copy()
    return post


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(bits(got), bits(want))


@pytest.fixture(scope="module")
def fixture():
    return np.load(FIXTURE)                                   # (a missing fixture is an error)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_forward_pass_keeps_its_device_bits(name, fixture):
    pytest.importorskip("torch")
    fx = fixture
    env = make_env(name)
    task = reset_draws(name)[1]
    for k in STATE:                                           # the state the reset left (getup: 45 mj_steps of the Fall reset)
        assert same(getattr(env, k).cpu().numpy(), fx[f"{name}/reset/{k}"]), (name, "reset", k)
    pre = {k: fx[f"{name}/start/{k}"] for k in STATE}
    fwd = forward_from(env, pre)
    for k in FORWARD:
        assert same(fwd[k], fx[f"{name}/forward/{k}"]), (name, "forward", k)
    for t in range(STEPS):
        post = step_from(env, pre, fx[f"{name}/act{t}"], None if task is None else task[1 + t])
        print(name, "step", t, "Newton iterations recorded", fx[f"{name}/post{t}/solver_iters"].tolist(), "now", post["solver_iters"].tolist())
        for k in POST:
            assert same(post[k], fx[f"{name}/post{t}/{k}"]), (name, t, k)
        pre = {k: fx[f"{name}/post{t}/{k}"] for k in STATE}


def test_the_fixture_holds_what_the_cases_are_for(fixture):
    fx = fixture
    for name, (humanoid, n, _, _, _) in CASES.items():
        mc = model_const(humanoid)
        q, v, a = (fx[f"{name}/start/{k}"] for k in STATE)
        assert q.shape == (n, mc.nq) and (q[:, 7:] != 0).all() and (v != 0).all() and (a != 0).all(), name
        for x in (q[:, 7:] if CASES[name][3] is not None else v, v, a):
            assert np.array_equal(x * 256, np.round(x * 256)), name       # multiples of 2^-8
        chain = np.array(deepest_chain_dofs(mc))
        assert len(chain) >= 21 and (np.abs(q[1, chain + 1]) >= 0.4).all(), name
        for t in range(STEPS):
            assert np.isfinite(fx[f"{name}/post{t}/qpos"]).all() and np.isfinite(fx[f"{name}/post{t}/obs"]).all(), name
            assert fx[f"{name}/post{t}/solver_iters"].max() > 15, name    # contacts: more than one Newton iteration per mj_step
        assert np.isfinite(fx[f"{name}/forward/M"]).all() and np.abs(fx[f"{name}/forward/xmat"][1] - np.eye(3).ravel()).max() > 0.5, name
