"""Bits of the forward pass on the wavefront emulator across the change that moves forward_kin's chain sums onto the packed chain
records (ss_tables.h chain_records): ss_debug_forward (mass matrix, bias, acceleration), ss_kinematics, the body
velocities and one control step, against tests/golden/fwd_chain_emu.npz, recorded from the commit before the change
(tests/golden/make_fwd_chain_emu.py, which imports the cases from here):

  smpl      4 SMPL envs (fixed-layout instantiation: the record-based code)
  smplx     2 SMPL-X envs (fixed layout, 12 levels in the one record unit)
  comb9     2 envs of the 9-branch comb of tests/test_synthetic_trees_emu.py: a runtime tree, which keeps the table loops

Joint angles, velocities and the warm start are non-zero multiples of 2^-8 in every body; env 1 has the joints on the chain to its
deepest body (hand, finger tip, branch end) turned by 0.5 to 1 rad each: the walk's product of rotations is far from the identity."""
import os

import numpy as np
import pytest

from helpers import FEET, GOLDEN, model_const, pd_tables

FIXTURE = os.path.join(GOLDEN, "fwd_chain_emu.npz")
# name: (envs, seed, root heights: env 0 standing or clear of the floor, the others dropped onto it)
CASES = {"smpl": (4, 71, (0.94, 0.60, 0.45, 0.30)), "smplx": (2, 72, (0.94, 0.55)), "comb9": (2, 73, (0.40, 0.37))}
OUT = ("M", "bias", "qacc", "xpos", "xmat", "body_vel_forward", "qpos", "qvel", "qacc_warm", "solver_iters", "body_vel", "obs")


def _model(name):
    if name == "comb9":
        from smplsim_amd.mjcf import compile_mjcf
        from smplsim_amd.mjcf_writer import table_to_mjcf
        from test_synthetic_trees_emu import _comb
        mc = compile_mjcf(table_to_mjcf(_comb(9)))
        nu = mc.nu
        return mc, (np.full(nu, 60.0), np.full(nu, 6.0), np.full(nu, 40.0), np.full(nu, 2.0), np.zeros(nu)), tuple(mc.body_names)
    mc = model_const(name + "_humanoid")
    return mc, pd_tables(mc), FEET


def inputs(name, q0):
    """Start state (qpos, qvel, warm start) and the action of the case; q0: the pose the reset left (root orientation)."""
    from test_fwd_chain_gpu import deepest_chain_dofs
    n, seed, heights = CASES[name]
    mc = _model(name)[0]
    rs = np.random.default_rng(seed)
    coarse = lambda x: (np.round(x * 256) / 256).astype(np.float32)
    nonzero = lambda x: np.where(x == 0, np.float32(1.0 / 256), x).astype(np.float32)
    q = np.array(q0, np.float32); q[:, 2] = heights
    q[:, 7:] = nonzero(coarse(rs.uniform(-0.1, 0.1, (n, mc.nq - 7))))
    chain = np.array(deepest_chain_dofs(mc))
    q[1, chain + 1] = coarse(rs.uniform(0.5, 1.0, len(chain)) * rs.choice([-1.0, 1.0], len(chain)))
    v = nonzero(coarse(rs.normal(size=(n, mc.nv)) * 0.2))
    warm = nonzero(coarse(rs.normal(size=(n, mc.nv)) * 2.0))
    act = coarse(rs.uniform(-0.5, 0.5, (n, mc.nu)))
    return q, v, warm, act


def run_case(name):
    from wave_emu import emu
    mc, tables, legal = _model(name)
    n = CASES[name][0]
    eb = emu.EmuBatch(mc, tables, n, legal_bodies=legal)
    eb.reset()
    q, v, warm, act = inputs(name, np.tile(mc.qpos0, (n, 1)) if name == "comb9" else eb.qpos)   # (the reset poses every model as the humanoids)
    eb.set_state(q, v, warm=warm)
    out = {}
    out["M"], out["bias"], out["qacc"] = eb.debug_forward(np.zeros((n, mc.nu), np.float32))
    out["body_vel_forward"] = eb.body_vel.copy()
    out["xpos"], out["xmat"] = eb.kinematics()
    eb.set_state(q, v, warm=warm)
    out["obs"] = eb.step(act)[0]
    for k in ("qpos", "qvel", "qacc_warm", "solver_iters", "body_vel"):
        out[k] = getattr(eb, k).copy()
    return out


@pytest.fixture(scope="module")
def fixture():
    return np.load(FIXTURE)                                   # (a missing fixture is an error)


@pytest.mark.parametrize("name", sorted(CASES))
def test_forward_pass_keeps_the_recorded_bits(name, fixture, monkeypatch):
    monkeypatch.delenv("SS_EMU_GENERIC", raising=False)
    got = run_case(name)
    for k in OUT:
        want = fixture[f"{name}/{k}"]
        assert got[k].dtype == want.dtype and got[k].shape == want.shape, (name, k)
        assert np.array_equal(got[k].view(np.uint32) if got[k].dtype == np.float32 else got[k], want.view(np.uint32) if want.dtype == np.float32 else want), (name, k)


def test_the_fixture_holds_what_the_cases_are_for(fixture):
    from test_fwd_chain_gpu import deepest_chain_dofs
    for name in CASES:
        q, v, warm, _ = inputs(name, np.zeros((CASES[name][0], _model(name)[0].nq)))
        for x in (q[:, 7:], v, warm):
            assert (x != 0).all() and np.array_equal(x * 256, np.round(x * 256)), name
        chain = np.array(deepest_chain_dofs(_model(name)[0]))
        assert (np.abs(q[1, chain + 1]) >= 0.5).all(), name
        assert np.abs(fixture[f"{name}/xmat"][1, chain[-1] // 3 - 1] - np.eye(3).ravel()).max() > 0.5, name
        assert all(np.isfinite(fixture[f"{name}/{k}"]).all() for k in OUT), name
        assert fixture[f"{name}/solver_iters"].max() > 15, name           # a dropped env: contacts, more than one Newton iteration per mj_step
        assert np.abs(fixture[f"{name}/body_vel_forward"]).max() > 0 and np.abs(fixture[f"{name}/M"]).max() > 0, name
