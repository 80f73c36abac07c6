"""dense_solve (smplsim_amd/csrc/ss_kernel.h) on the GPU against the float64 oracle at every system size: the cases of
tests/golden/dense_solve_cases.npz (tests/dense_solve_cases.py: one to five and more tile rows, the full last tile row at 16 / 64 / 112
matrix rows, both sides of the own region / shared block edge, the staging fallback in rounds, SMPL's two lanes per body and SMPL-X's
one; test_dense_solve_cpu.py shows on the kernel's counters that the cases take these paths, test_dense_solve_emu.py holds the emulator
builds of the same source to 1e-10 and 3e-5).  What only the GPU build has — the matrix instruction's operand layout, v_readlane
pivots, the lock of the shared block — is held here to the project's gate for this quantity on the device, 5e-5 of the largest
acceleration (test_gpu_parity.py), per case, with the oracle's contact count.

Per humanoid one batch of all cases through ss_debug_forward, from a zero warm start and from the oracle's converged acceleration;
then the same again with every wavefront of ONE full workgroup walking the cases through the hand-out counter, so that the pooled
cases meet at one shared block and its lock: the same bytes.  Reads the fixture only."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import dense_solve_cases as DC  # noqa: E402

TOL = 5e-5


def _np(t):
    return t.detach().cpu().numpy()


def _forward(env, c, warm):
    n = len(c["size"])
    env.set_state(c["qpos"], c["qvel"], warm=c["warm"] if warm else np.zeros_like(c["warm"]))
    M, bias, qacc = env.debug_forward(torch.tensor(c["ctrl"], device=env.device))
    torch.cuda.synchronize()
    assert M.shape[0] == n
    return _np(M), _np(bias), _np(qacc), _np(env.self_contacts).copy()


@pytest.mark.parametrize("which", list(DC.HUMANOIDS))
def test_constrained_acceleration_at_every_system_size(which):
    from smplsim_amd._lib import lib
    from smplsim_amd.batch import SMPLSimVecEnv
    from test_gpu_parity import _record
    c = DC.load(which)
    n = len(c["size"])
    env = SMPLSimVecEnv(n, humanoid=DC.HUMANOIDS[which], autoreset=False, self_collision=True)
    try:
        max_epw = env.launch_info()["envs_per_workgroup"]
        auto = {warm: _forward(env, c, warm) for warm in (False, True)}
        assert lib().ss_set_launch_geometry(env.handle, max_epw, 1) == 0         # one workgroup: one shared block for every pooled case
        one_wg = {warm: _forward(env, c, warm) for warm in (False, True)}
        assert lib().ss_set_launch_geometry(env.handle, 0, 0) == 0
    finally:
        env.close()
    bins = list(dict.fromkeys(c["bin"]))
    failures = []
    for warm in (False, True):
        _, _, qacc, nself = auto[warm]
        err = DC.rel_err(qacc, c["qacc"])
        worst = {str(b): float(np.nan_to_num(err[c["bin"] == b], nan=np.inf).max()) for b in bins}
        _record("dense_solve_%s_%s" % (which, "from_the_solution" if warm else "from_zero"), envs_per_workgroup=max_epw, **{"bin_" + b: e for b, e in worst.items()})
        print("per case:", " ".join("%d:%s:%.1e" % (i, c["bin"][i], err[i]) for i in range(n)))
        for i in range(n):
            if nself[i] != c["nself"][i] or not err[i] < TOL:
                failures.append((warm, i, str(c["bin"][i]), int(c["size"][i]), int(nself[i]), int(c["nself"][i]), float(err[i])))
        for a, b, what in zip(auto[warm], one_wg[warm], ("M", "bias", "qacc", "self_contacts")):
            rows = np.flatnonzero((a.reshape(n, -1).view(np.uint8) != b.reshape(n, -1).view(np.uint8)).any(axis=1)) if a.dtype != np.int32 else np.flatnonzero(a != b)
            if len(rows):
                failures.append((warm, "one workgroup of %d wavefronts moves the bytes of %s" % (max_epw, what), [(int(r), str(c["bin"][r])) for r in rows]))
    assert not failures, failures
