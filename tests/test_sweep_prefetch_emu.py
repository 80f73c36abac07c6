"""aba_solve requests a level's record (word 0) one level ahead, before the hand-off that precedes the level, and keeps a node's
(W, y) rows by record index instead of by body where nobody else reads them.  The new thing that can go wrong is the index of
the request: the next level's clamp  g < nk' - 1 ? g : nk' - 1  must use the NEXT level's width, and there is no next level behind
the last one.  Short rollouts on the wavefront emulator, 2 envs, 2 control steps, the second env dropped onto the floor:

  smpl, smplx             fixed-layout against runtime-layout instantiation, bit for bit, and both against the rows of
                          tests/golden/sweep_padding_emu.npz (recorded with the lane-predicated sweeps: envs 0 and 3 of its cases)
  comb9 comb17 chain15    the synthetic trees of tests/test_synthetic_trees_emu.py (runtime layout only): levels that grow and shrink
  tree1 tree2 tree3       from one level to the next, two passes (comb17), one-node levels; no level at all, one level, two levels —
                          "the next level" does not exist, or is the last

The synthetic cases are held to tests/golden/sweep_prefetch_emu.npz, recorded from the commit before the change
(`python tests/test_sweep_prefetch_emu.py --record` rewrites it from whatever kernel source the emulator is built from, so
only do that on purpose)."""
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.dont_write_bytecode = True
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from helpers import FEET, GOLDEN, pd_tables  # noqa: E402
from smplsim_amd.mjcf import compile_mjcf  # noqa: E402
from smplsim_amd.mjcf_writer import table_to_mjcf  # noqa: E402
from test_sweep_padding_emu import FIXTURE as PADDING_FIXTURE, HEIGHTS, humanoid_inputs  # noqa: E402

FIXTURE = os.path.join(GOLDEN, "sweep_prefetch_emu.npz")
N, STEPS = 2, 2
ROWS = [0, 3]                                                 # of the 4 envs of the padding cases: standing, dropped onto the floor
OUT = ("qpos", "qvel", "qacc_warm", "solver_iters")
HUMANOIDS = {"smpl": ("smpl_humanoid", 21), "smplx": ("smplx_humanoid", 22)}
# name: (bodies of the chain | branches of the comb, root height of env 0, of env 1 — its lowest geom starts below the floor's margin)
SYNTHETIC = {"comb9": ("comb", 9, 0.40, 0.37), "comb17": ("comb", 17, 0.40, 0.37), "chain15": ("chain", 14, 2.8, 2.1),
             "tree1": ("chain", 1, 0.26, 0.05), "tree2": ("chain", 2, 0.46, 0.24), "tree3": ("chain", 3, 0.66, 0.43)}


def _rollout(eb, acts):
    rec = {}
    for t in range(STEPS):
        eb.step(acts[t])
        for k in OUT:
            rec[f"{k}_{t}"] = getattr(eb, k).copy()
    return rec


def run_humanoid(name, generic, setenv, delenv):
    from wave_emu import emu
    humanoid, seed = HUMANOIDS[name]
    if generic:
        setenv("SS_EMU_GENERIC", "1")
    else:
        delenv("SS_EMU_GENERIC")
    mc, acts, qj, v = humanoid_inputs(humanoid, seed)
    eb = emu.EmuBatch(mc, pd_tables(mc), N, legal_bodies=FEET)
    eb.reset()
    q = eb.qpos.copy(); q[:, 2] = np.asarray(HEIGHTS)[ROWS]; q[:, 7:] += qj[ROWS]
    eb.set_state(q, v[ROWS])
    return _rollout(eb, acts[:, ROWS])


def run_synthetic(name):
    from test_synthetic_trees_emu import _chain, _comb
    from wave_emu import emu
    kind, n, z0, z1 = SYNTHETIC[name]
    mc = compile_mjcf(table_to_mjcf(_comb(n) if kind == "comb" else _chain(n)))
    nu = mc.nu
    tables = (np.full(nu, 60.0), np.full(nu, 6.0), np.full(nu, 40.0), np.full(nu, 2.0), np.zeros(nu))
    eb = emu.EmuBatch(mc, tables, N, legal_bodies=tuple(mc.body_names))
    rs = np.random.default_rng(100 + len(name) + n)
    q = np.zeros((N, mc.nq)); q[:, 2] = (z0, z1); q[:, 3] = 1.0
    q[:, 7:] = rs.uniform(-0.3, 0.3, (N, mc.nq - 7))
    eb.set_state(q, rs.normal(size=(N, mc.nv)) * 0.3)
    return _rollout(eb, rs.uniform(-0.3, 0.3, (STEPS, N, nu)))


@pytest.fixture(scope="module")
def padding_fixture():
    return np.load(PADDING_FIXTURE)


@pytest.fixture(scope="module")
def fixture():
    return np.load(FIXTURE)                                   # (a missing fixture is an error)


@pytest.mark.parametrize("name", sorted(HUMANOIDS))
def test_fixed_and_generic_sweeps_agree_and_keep_the_recorded_bits(name, padding_fixture, monkeypatch):
    fixed = run_humanoid(name, False, monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False))
    generic = run_humanoid(name, True, monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False))
    for t in range(STEPS):
        for k in OUT:
            assert np.array_equal(fixed[f"{k}_{t}"], generic[f"{k}_{t}"]), (name, k, t)
            assert np.array_equal(fixed[f"{k}_{t}"], padding_fixture[f"{name}/{k}_{t}"][ROWS]), (name, k, t)
    assert fixed[f"solver_iters_{STEPS - 1}"][1] > 15         # the dropped env: contacts, more than one Newton iteration per mj_step


@pytest.mark.parametrize("name", sorted(SYNTHETIC))
def test_synthetic_trees_keep_the_recorded_bits(name, fixture):
    rec = run_synthetic(name)
    for t in range(STEPS):
        for k in OUT:
            assert np.array_equal(rec[f"{k}_{t}"], fixture[f"{name}/{k}_{t}"]), (name, k, t)


def test_the_synthetic_cases_exercise_what_they_are_for(fixture):
    for name in SYNTHETIC:
        assert np.isfinite(fixture[f"{name}/qpos_{STEPS - 1}"]).all() and np.isfinite(fixture[f"{name}/qvel_{STEPS - 1}"]).all(), name
        assert fixture[f"{name}/solver_iters_{STEPS - 1}"][1] > 15, name   # the dropped env is in contact


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], "usage: python tests/test_sweep_prefetch_emu.py --record"
    out = {}
    for name in SYNTHETIC:
        for k, v in run_synthetic(name).items():
            out[f"{name}/{k}"] = v
        print(name, "iters", out[f"{name}/solver_iters_{STEPS - 1}"], "finite", np.isfinite(out[f"{name}/qpos_{STEPS - 1}"]).all())
    np.savez_compressed(FIXTURE, **out)
    print("wrote", FIXTURE, os.path.getsize(FIXTURE), "bytes")
