"""The code around the articulated-body solve of a Newton iteration (newton_prepare, newton_finish, ls_eval, eval_rows, row_dcost)
evaluates its contact and limit rows as straight-line code: a row that does not exist, or a lane without a dof or a body, is made
inert by what is selected, not by a branch.  That must not move a bit of any result.  Short rollouts on the wavefront emulator, 2
control steps per case, against tests/golden/newton_rows_emu.npz, which was recorded from the commit before the change
(`python tests/test_newton_rows_emu.py --record` rewrites it from whatever kernel source the emulator is built from, so only do
that on purpose):

  smpl               4 envs: standing, dropped onto the floor, and two dropped envs with a joint beyond its range — a dof of the first
                     dof pass (dof 10) and one of the last (dof 70, SMPL's second pass holds dofs 64 to 74); fixed-layout against
                     runtime-layout instantiation, bit for bit, and both against the fixture
  smplx              3 envs, three dof passes: dropped, a joint beyond its range in the first pass (dof 10) and in the last (dof 150)
  selfcol_coupled    2 envs with body-body contacts and a forced coupled set
  nonfinite          3 envs: standing, a NaN in the first action, a start state that diverges inside the first control step
  overflow           2 envs with large but legal start velocities: one whose Newton direction is not a descent direction (the exit
                     with the decrement at rounding level), one whose decrement overflows to NaN (the bad-state reset of newton_finish)
  iters1, iters3     2 envs, newton_iters 1 and 3: the cap ends the loop (at 1 in every mj_step of the dropped env), not the termination test

The recorder builds the emulator with SS_TRACE_NEWTON and refuses to write a fixture whose recorded steps do not contain every
outcome of newton_finish that the trace names: an accepted al = 1, a line search that expands beyond 1, one that ends below 1, a
full step that changes the active set (a row turned active or inactive: the trace does not say which), an exit with the decrement
at rounding level and a bad-state reset (a non-finite decrement; the env's warning count goes up)."""
import os
import re
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.dont_write_bytecode = True
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from helpers import FEET, GOLDEN, default_qpos, model_const, pd_tables  # noqa: E402

FIXTURE = os.path.join(GOLDEN, "newton_rows_emu.npz")
STEPS = 2
OUT = ("qpos", "qvel", "qacc_warm", "solver_iters")
BEYOND = 3.3                                                  # every hinge of both humanoids ends at +-pi (or +-4 pi)
# name: (humanoid, seed, root heights, {env: (dof beyond its range, sign)}, emulator cfg)
CASES = {"smpl": ("smpl_humanoid", 41, (0.94, 0.60, 0.55, 0.50), {2: (10, 1.0), 3: (70, -1.0)}, {}),
         "smplx": ("smplx_humanoid", 42, (0.60, 0.55, 0.50), {1: (10, -1.0), 2: (150, 1.0)}, {}),
         "selfcol_coupled": ("smpl_humanoid", 43, (0.94, 0.60), {}, {"self_collision": True}),
         "nonfinite": ("smpl_humanoid", 44, (0.94, 0.93, 0.92), {}, {}),
         "overflow": ("smpl_humanoid", 44, (0.94, 0.94), {}, {}),
         "iters1": ("smpl_humanoid", 45, (0.94, 0.30), {}, {"newton_iters": 1}),
         "iters3": ("smpl_humanoid", 45, (0.94, 0.30), {}, {"newton_iters": 3})}
NAN_ENV, DIVERGING_ENV = 1, 2                                 # of "nonfinite", inputs as in tests/placement_cases.py
FORCE_COUPLED = "%x" % ((1 << 7) | (1 << 12) | (1 << 23))     # a leg, the trunk, a hand


def run_case(name, generic=False, setenv=os.environ.__setitem__, delenv=lambda k: os.environ.pop(k, None)):
    """{"<field>_<t>": array} of one case's rollout on the emulator, plus "nwarn" after the last step."""
    from wave_emu import emu
    humanoid, seed, heights, beyond, cfg = CASES[name]
    delenv("SS_EMU_GENERIC"); delenv("SS_EMU_FORCE_COUPLED")
    if generic:
        setenv("SS_EMU_GENERIC", "1")
    if name == "selfcol_coupled":
        setenv("SS_EMU_FORCE_COUPLED", FORCE_COUPLED)
    mc, n = model_const(humanoid), len(heights)
    rs = np.random.default_rng(seed)
    acts = rs.uniform(-0.5, 0.5, (STEPS, n, mc.nu))
    q = np.tile(default_qpos(mc.nq), (n, 1))
    q[:, 2] = heights
    q[:, 7:] += rs.uniform(-0.1, 0.1, (n, mc.nq - 7))
    v = rs.normal(size=(n, mc.nv)) * 0.2
    for e, (dof, sign) in beyond.items():
        q[e, dof + 1] = sign * BEYOND
    if name == "nonfinite":
        v[DIVERGING_ENV, [3, 8, 20, 40]] *= 1e4
        acts[0, NAN_ENV, 5] = np.nan
    if name == "overflow":                                    # (mj_checkVel's bound is 1e10: both states are stepped, not reset at once)
        v[0, [3, 8, 20, 40]] *= 1e5
        v[1, 3:] = np.clip(v[1, 3:] * 1e10, -9e9, 9e9)
    eb = emu.EmuBatch(mc, pd_tables(mc), n, legal_bodies=FEET, **cfg)
    eb.reset()
    eb.set_state(q, v)
    rec = {}
    for t in range(STEPS):
        eb.step(acts[t])
        for k in OUT:
            rec[f"{k}_{t}"] = getattr(eb, k).copy()
    rec["nwarn"] = eb.nwarn.copy()
    return rec


@pytest.fixture(scope="module")
def fixture():
    return np.load(FIXTURE)                                   # (a missing fixture is an error)


def _same(rec, fixture, name):
    for t in range(STEPS):
        for k in OUT:
            want = fixture[f"{name}/{k}_{t}"]
            assert rec[f"{k}_{t}"].dtype == want.dtype and np.array_equal(rec[f"{k}_{t}"], want, equal_nan=True), (name, k, t)


@pytest.mark.parametrize("name", sorted(CASES))
def test_rollout_keeps_the_recorded_bits(name, fixture, monkeypatch):
    _same(run_case(name, False, monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False)), fixture, name)


@pytest.mark.parametrize("name", ["smpl", "smplx"])
def test_runtime_layout_keeps_the_recorded_bits_of_the_fixed_layout(name, fixture, monkeypatch):
    _same(run_case(name, True, monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False)), fixture, name)


def test_the_cases_exercise_what_they_are_for(fixture):
    for name in CASES:
        if name not in ("nonfinite", "overflow"):
            assert np.isfinite(fixture[f"{name}/qpos_{STEPS - 1}"]).all() and np.isfinite(fixture[f"{name}/qvel_{STEPS - 1}"]).all(), name
    for name in ("smpl", "smplx", "selfcol_coupled"):                                     # contacts: the iteration did iterate
        assert fixture[f"{name}/solver_iters_{STEPS - 1}"].max() > 15, name
    mjsteps = 15                                                                           # control_freq_inv: mj_steps per control step
    # the dropped env wants more than one iteration per mj_step (iters3, same inputs), so in iters1 the cap ended its loops
    assert (fixture["iters1/solver_iters_1"] == mjsteps).all() and mjsteps < fixture["iters3/solver_iters_1"][1] <= 3 * mjsteps
    assert fixture["nonfinite/nwarn"][DIVERGING_ENV] >= 1 and fixture["nonfinite/nwarn"][NAN_ENV] >= 1 and fixture["nonfinite/nwarn"][0] == 0
    assert fixture["overflow/nwarn"][1] >= 1
    # the poses beyond a joint's range are still beyond it, or came back through the limit row, inside the recorded steps
    for name in ("smpl", "smplx"):
        for e, (dof, sign) in CASES[name][3].items():
            assert sign * fixture[f"{name}/qvel_0"][e, dof] < 0, (name, e)                # the limit row pushes the joint back


# ------------------------------------------------------------------------------------------------ recorder
def _trace_library(tmp):
    """The emulator built with SS_TRACE_NEWTON (flags of tests/wave_emu/Makefile), under `tmp`."""
    import subprocess
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "wave_emu")
    flags = next(ln.split("?=", 1)[1].split() for ln in open(os.path.join(here, "Makefile")) if ln.startswith("CXXFLAGS"))
    out = os.path.join(tmp, "libss_emu_trace.so")
    subprocess.check_call([os.environ.get("CXX", "g++"), *flags, "-DSS_TRACE_NEWTON", "-shared", "-o", out, os.path.join(here, "emu.cpp")])
    return out


def coverage(trace):
    """Which outcomes of newton_finish the SS_TRACE_NEWTON lines of `trace` contain."""
    steps = [(float(m.group(1)), int(m.group(2)), int(m.group(3))) for m in re.finditer(r" al (\S+) exact (\d) piece_min (\d)", trace)]
    noise = re.findall(r"dg (\S+) dgabs (\S+) : decrement at rounding level", trace)
    return {"accepted al = 1": any(al == 1.0 and ex == 1 for al, ex, _ in steps),
            "line search expands beyond 1": any(al > 1.0 for al, _, _ in steps),
            "line search ends below 1": any(0.0 < al < 1.0 for al, _, _ in steps),
            "full step changes the active set": any(ex == 1 and pm == 0 for _, ex, pm in steps),
            "full step inside one piece": any(pm == 1 for _, _, pm in steps),
            "decrement at rounding level": any(np.isfinite(float(a)) and np.isfinite(float(b)) for a, b in noise),
            "bad-state reset": any(np.isnan(float(a)) or np.isnan(float(b)) for a, b in noise)}


if __name__ == "__main__":
    import ctypes
    import tempfile
    assert sys.argv[1:] == ["--record"], "usage: python tests/test_newton_rows_emu.py --record"
    from smplsim_amd import _cabi
    from wave_emu import emu
    with tempfile.TemporaryDirectory() as tmp:
        emu._LIBS["libss_emu.so"] = _cabi.bind(ctypes.CDLL(_trace_library(tmp)))
        log = os.path.join(tmp, "trace.txt")
        saved, fd = os.dup(2), os.open(log, os.O_WRONLY | os.O_CREAT | os.O_TRUNC)
        os.dup2(fd, 2)                                        # the library traces to the C stderr
        try:
            out = {}
            for name in CASES:
                for k, v in run_case(name).items():
                    out[f"{name}/{k}"] = v
        finally:
            ctypes.CDLL(None).fflush(None)
            os.dup2(saved, 2); os.close(fd); os.close(saved)
        trace = open(log).read()
    for name in CASES:
        print(name, "iters", out[f"{name}/solver_iters_{STEPS - 1}"], "nwarn", out[f"{name}/nwarn"])
    cov = coverage(trace)
    print(len(trace.splitlines()), "trace lines;", cov)
    missing = [k for k, v in cov.items() if not v]
    assert not missing, f"the recorded steps lack: {missing}; nothing written"
    np.savez_compressed(FIXTURE, **out)
    print("wrote", FIXTURE, os.path.getsize(FIXTURE), "bytes")
