"""dense_solve (smplsim_amd/csrc/ss_kernel.h) on the wavefront emulator against the float64 oracle at every system size the cases of
tests/dense_solve_cases.py hold: one to five and more tile rows, the full last tile row, both sides of the own region / shared block
edge, the staging fallback in rounds, both wave uses of the tree part (test_dense_solve_cpu.py shows that the cases take these paths).

All cases of a humanoid run in ONE batch through ss_debug_forward, once from a zero warm start (several Newton iterations, coupled
sets that grow) and once from the oracle's converged acceleration (the iteration begins on the final active set).  Gates: the project's
own for this quantity — max |qacc - ref| / max |ref| below 1e-10 on the float64 build and below 3e-5 on the float32 build
(test_selfcol_emu.py) — and the oracle's contact count.  The mass matrix and the bias do not depend on the flag.  GPU twin:
test_dense_solve_gpu.py (5e-5)."""
import functools

import numpy as np
import pytest

import dense_solve_cases as DC
from helpers import FEET, model_const, pd_tables
from wave_emu import emu

TOL = {True: 1e-10, False: 3e-5}


@functools.lru_cache(maxsize=None)
def run(which, f64, self_collision=True):
    """{warm: (M, bias, qacc, self_contacts)} of all cases of a humanoid in one batch."""
    c, mc = DC.load(which), model_const(DC.HUMANOIDS[which])
    n = len(c["size"])
    eb = emu.EmuBatch(mc, pd_tables(mc), n, legal_bodies=FEET, f64=f64, self_collision=self_collision)
    out = {}
    for warm in (False, True):
        eb.set_state(c["qpos"], c["qvel"], warm=c["warm"] if warm else np.zeros((n, mc.nv)))
        M, bias, qacc = eb.debug_forward(c["ctrl"])
        out[warm] = (M, bias, qacc, eb.self_contacts.copy())
    return out


@pytest.mark.parametrize("which", list(DC.HUMANOIDS))
@pytest.mark.parametrize("f64", [True, False], ids=["f64", "f32"])
@pytest.mark.parametrize("warm", [False, True], ids=["from_zero", "from_the_solution"])
def test_constrained_acceleration_at_every_system_size(which, f64, warm):
    c = DC.load(which)
    _, _, qacc, nself = run(which, f64)[warm]
    assert np.array_equal(nself, c["nself"])
    err = DC.rel_err(qacc, c["qacc"])
    print("worst per bin:", {str(b): float(err[c["bin"] == b].max()) for b in dict.fromkeys(c["bin"])})
    assert np.isfinite(qacc).all() and (err < TOL[f64]).all(), [(i, str(c["bin"][i]), float(err[i])) for i in np.flatnonzero(~(err < TOL[f64]))]


@pytest.mark.parametrize("which", list(DC.HUMANOIDS))
@pytest.mark.parametrize("f64", [True, False], ids=["f64", "f32"])
def test_mass_matrix_and_bias_do_not_depend_on_the_flag(which, f64):
    """The same states without body-body contacts: the same mass matrix and bias, bit for bit, another acceleration."""
    on, off = run(which, f64)[False], run(which, f64, self_collision=False)[False]
    assert np.array_equal(on[0], off[0]) and np.array_equal(on[1], off[1])
    assert (off[3] == 0).all() and (np.abs(on[2] - off[2]).max(axis=1) > 1e-6 * np.abs(on[2]).max(axis=1)).all()
    warm_on, warm_off = run(which, f64)[True], run(which, f64, self_collision=False)[True]
    assert np.array_equal(warm_on[0], on[0]) and np.array_equal(warm_on[1], on[1]) and np.array_equal(warm_off[0], on[0])
