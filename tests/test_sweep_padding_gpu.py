"""The SMPL and SMPL-X cases of tests/test_sweep_padding_emu.py replayed on the device: every control step of the fixture, from the
pre-step state the fixture holds, against the float64 oracle at the per-control-step tolerance of tests/parity_tools.py (emulator
bits are not GPU bits: the sums of a group run in another order, so the device is held to the oracle, not to the fixture).  The
SMPL case runs the fixed-layout step kernel with levels of 2 4 5 4 4 4 nodes out of 8 groups, SMPL-X the two-pass one with 12-node
levels; one env of each is dropped onto the floor."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import parity_tools as P  # noqa: E402
from test_sweep_padding_emu import FIXTURE, N, PRE, STEPS, humanoid_inputs  # noqa: E402


@pytest.mark.parametrize("name,humanoid,seed", [("smpl", "smpl_humanoid", 21), ("smplx", "smplx_humanoid", 22)])
def test_fixture_steps_on_the_device_match_the_oracle(name, humanoid, seed):
    from smplsim_amd.batch import SMPLSimVecEnv
    fx = np.load(FIXTURE)
    mc, acts, _, _ = humanoid_inputs(humanoid, seed)
    env = SMPLSimVecEnv(N, humanoid=humanoid, autoreset=False)
    env.reset()
    for t in range(STEPS):
        pre = {k: fx[f"{name}/{k}_pre{t}"].astype(np.float64) for k in PRE}
        env.set_state(*[pre[k] for k in PRE])
        env.step(torch.tensor(acts[t], dtype=torch.float32, device=env.device))
        torch.cuda.synchronize()
        post = dict(qpos=env.qpos.cpu().numpy().astype(np.float64), qvel=env.qvel.cpu().numpy().astype(np.float64))
        orc = P.oracle_step(pre, acts[t], humanoid)
        err = P.rel_err(post, orc)
        print(name, "step", t, "rel. error (qpos, qvel) per env", err.tolist(), "Newton iterations", env.solver_iters.cpu().tolist())
        assert np.isfinite(post["qpos"]).all() and (orc["nwarn"] == 0).all()
        assert P.within_tol(err, P.TOL_STEP).all(), (name, t, err)
        # the emulator's result of the same step, recorded with the predicated sweeps: same arithmetic, another summation order
        emu = dict(qpos=fx[f"{name}/qpos_{t}"].astype(np.float64), qvel=fx[f"{name}/qvel_{t}"].astype(np.float64))
        assert P.within_tol(P.rel_err(post, emu), P.TOL_STEP).all()
