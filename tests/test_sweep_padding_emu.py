"""The tree sweeps of aba_solve run their loads and arithmetic on all 64 lanes — padding groups redo the level's last node,
padding rows redo row 5 — and guard only the stores and the inputs of the group sums.  That must not move a bit of any
result: short rollouts on the wavefront emulator against tests/golden/sweep_padding_emu.npz, which was recorded with the
predicated sweeps (the commit before the change; `python tests/test_sweep_padding_emu.py --record` rewrites it from
whatever kernel source the emulator is built from, so only do that on purpose).

4 envs, 2 control steps per case; the cases are the smallest shapes at which the change can go wrong:
  smpl / smpl_generic     levels of 2 4 5 4 4 4 nodes out of 8 groups, fixed-layout and runtime-layout instantiation
  smplx                   12-node levels: a partially filled second pass (groups 4..7 of pass 1 are padding)
  chain15 / comb8 / two   synthetic trees: 1-node levels, a level of exactly 8 nodes (no padding group), the smallest tree
  selfcol_coupled         SELFCOL with a forced coupled set: the cmask branches on a padding group's clamped body
  nonfinite               one env driven to a non-finite state and one non-finite action: the autoreset path, NaNs in LDS
"""
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.dont_write_bytecode = True
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from helpers import FEET, GOLDEN, model_const, pd_tables  # noqa: E402
from smplsim_amd.mjcf import compile_mjcf  # noqa: E402
from smplsim_amd.mjcf_writer import table_to_mjcf  # noqa: E402

FIXTURE = os.path.join(GOLDEN, "sweep_padding_emu.npz")
N, STEPS = 4, 2
PRE = ("qpos", "qvel", "qpos_prev", "qvel_prev", "qacc_warm")
OUT = ("qpos", "qvel", "qacc_warm", "obs", "reward", "terminated", "truncated", "solver_iters", "nwarn")
CASES = ("smpl", "smpl_generic", "smplx", "chain15", "comb8", "two", "selfcol_coupled", "nonfinite")
HEIGHTS = (0.94, 0.93, 0.92, 0.60)                            # standing, and one env dropped onto the floor (contacts, limits)


def humanoid_inputs(humanoid, seed):
    """Start state and actions of the humanoid cases (shared with the GPU replay in test_sweep_padding_gpu.py)."""
    mc = model_const(humanoid)
    rs = np.random.default_rng(seed)
    acts = rs.uniform(-0.5, 0.5, (STEPS, N, mc.nu))
    qj = rs.uniform(-0.1, 0.1, (N, mc.nq - 7))
    v = rs.normal(size=(N, mc.nv)) * 0.2
    return mc, acts, qj, v


def _humanoid(humanoid, seed, **cfg):
    from wave_emu import emu
    mc, acts, qj, v = humanoid_inputs(humanoid, seed)
    eb = emu.EmuBatch(mc, pd_tables(mc), N, legal_bodies=FEET, **cfg)
    eb.reset()
    q = eb.qpos.copy(); q[:, 2] = HEIGHTS; q[:, 7:] += qj
    eb.set_state(q, v)
    return eb, acts


def _synthetic(name):
    from test_synthetic_trees_emu import _chain, _comb
    from wave_emu import emu
    table, z = {"chain15": (_chain(14), 2.8), "comb8": (_comb(8), 0.40), "two": (_chain(2), 0.3)}[name]
    mc = compile_mjcf(table_to_mjcf(table))
    nu = mc.nu
    tables = (np.full(nu, 60.0), np.full(nu, 6.0), np.full(nu, 40.0), np.full(nu, 2.0), np.zeros(nu))
    eb = emu.EmuBatch(mc, tables, N, legal_bodies=tuple(mc.body_names))
    rs = np.random.default_rng(len(name))
    q = np.zeros((N, mc.nq)); q[:, 2] = z; q[:, 3] = 1.0
    q[:, 7:] = rs.uniform(-0.3, 0.3, (N, mc.nq - 7))
    eb.set_state(q, rs.normal(size=(N, mc.nv)) * 0.3)
    return eb, rs.uniform(-0.3, 0.3, (STEPS, N, nu))


def run_case(name, monkeypatch=None):
    """{"<field>_pre<t>" | "<field>_<t>": array} of one case's rollout on the emulator."""
    setenv = (lambda k, v: monkeypatch.setenv(k, v)) if monkeypatch is not None else os.environ.__setitem__
    if name == "smpl_generic":
        setenv("SS_EMU_GENERIC", "1")
    if name == "selfcol_coupled":
        setenv("SS_EMU_FORCE_COUPLED", "%x" % ((1 << 7) | (1 << 12) | (1 << 23)))   # a leg, the trunk, a hand: three levels, two limbs
    if name in ("smpl", "smpl_generic"):
        eb, acts = _humanoid("smpl_humanoid", 21)
    elif name == "smplx":
        eb, acts = _humanoid("smplx_humanoid", 22)
    elif name == "selfcol_coupled":
        eb, acts = _humanoid("smpl_humanoid", 23, self_collision=True)
    elif name == "nonfinite":
        eb, acts = _humanoid("smpl_humanoid", 24)
        eb.qvel[2, 10] = np.nan                               # env 2 starts non-finite; env 1 gets a non-finite action in step 1
        acts[1, 1, 5] = np.inf
    else:
        eb, acts = _synthetic(name)
    rec = {}
    for t in range(STEPS):
        for k in PRE:
            rec[f"{k}_pre{t}"] = getattr(eb, k).copy()
        eb.step(acts[t])
        for k in OUT:
            rec[f"{k}_{t}"] = getattr(eb, k).copy()
    return rec


@pytest.fixture(scope="module")
def fixture():
    return np.load(FIXTURE)


@pytest.mark.parametrize("name", CASES)
def test_rollout_bits_are_those_of_the_predicated_sweeps(name, fixture, monkeypatch):
    rec = run_case(name, monkeypatch)
    for t in range(STEPS):
        for k in OUT:
            assert np.array_equal(rec[f"{k}_{t}"], fixture[f"{name}/{k}_{t}"], equal_nan=True), (name, k, t)


def test_the_cases_exercise_what_they_are_for(fixture):
    assert fixture["smpl/solver_iters_1"].max() > 15 and fixture["smplx/solver_iters_1"].max() > 15      # contacts: more than one Newton iteration per mj_step
    assert fixture["nonfinite/nwarn_0"][2] >= 1 and fixture["nonfinite/nwarn_1"][1] >= 1                # both autoresets ran
    assert fixture["nonfinite/nwarn_1"][[0, 3]].tolist() == [0, 0]
    for name in CASES:
        assert np.isfinite(fixture[f"{name}/qpos_{STEPS - 1}"]).all(), name
    for k in OUT:                                                                                       # fixed == generic, as recorded
        assert np.array_equal(fixture[f"smpl/{k}_1"], fixture[f"smpl_generic/{k}_1"])


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], "usage: python tests/test_sweep_padding_emu.py --record"
    out = {}
    for name in CASES:
        os.environ.pop("SS_EMU_GENERIC", None); os.environ.pop("SS_EMU_FORCE_COUPLED", None)
        for k, v in run_case(name).items():
            if "_pre" not in k or name in ("smpl", "smplx"):   # the pre-step states are what the GPU test replays
                out[f"{name}/{k}"] = v
        print(name, "iters", out[f"{name}/solver_iters_{STEPS - 1}"], "nwarn", out[f"{name}/nwarn_{STEPS - 1}"])
    np.savez_compressed(FIXTURE, **out)
    print("wrote", FIXTURE, os.path.getsize(FIXTURE), "bytes")
