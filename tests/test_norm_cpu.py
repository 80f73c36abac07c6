"""The RunningNorm update, host side (-m "not gpu"): the workspace query of ss_running_norm_update against the block rule of include/smplsim_mlp.h, its argument
checks (they run before any launch, so no GPU is needed: cf. test_optim_cpu.py), and the Python switches."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def L():
    import torch  # noqa: F401  (always before the library: one HIP runtime per process)
    from smplsim_amd import _cabi, _lib
    _lib.build()
    lib = _cabi.bind_mlp(ctypes.CDLL(_lib.LIB_PATH))
    lib.ss_last_error.restype = ctypes.c_char_p
    return lib


ONE = 16                                                            # a pointer value that is never dereferenced: every call in this file fails its checks first


def test_workspace_query_is_one_pair_of_doubles_per_block_and_column(L):
    from smplsim_amd._cabi import NORM_BLOCK_ROWS as R
    assert R == 256
    for M in (1, R - 1, R, R + 1, 3 * R + 37):
        for dim in (1, 64, 289):
            assert L.ss_running_norm_workspace(M, dim) == -(-M // R) * dim * 16, (M, dim)
    assert L.ss_running_norm_workspace(2 ** 31 - 1, 289) == 2 ** 23 * 289 * 16          # the block count is formed in 64 bits
    for M, dim in ((0, 8), (-3, 8), (8, 0), (8, -1)):
        assert L.ss_running_norm_workspace(M, dim) < 0 and b"ss_running_norm_workspace" in L.ss_last_error(), (M, dim)


def _call(L, x=ONE, M=300, dim=8, ldx=None, mean=ONE, var=ONE, std=ONE, n=ONE, ws=ONE, nbytes=1 << 40):
    return L.ss_running_norm_update(x, M, dim, dim if ldx is None else ldx, mean, var, std, n, ws, nbytes, None)


def test_running_norm_update_checks_its_arguments_before_any_launch(L):
    odd = 24
    need = L.ss_running_norm_workspace(300, 8)
    assert need == 2 * 8 * 16
    bad = [(dict(x=None), b"null argument"), (dict(mean=None), b"null argument"), (dict(var=None), b"null argument"), (dict(std=None), b"null argument"),
           (dict(n=None), b"null argument"), (dict(M=0), b"M >= 1"), (dict(M=-5), b"M >= 1"), (dict(dim=0, ldx=8), b"dim >= 1"), (dict(dim=-2, ldx=8), b"dim >= 1"),
           (dict(ldx=7), b"row strides"), (dict(ldx=0), b"row strides"),
           (dict(ws=None), b"null workspace"), (dict(ws=odd), b"workspace must be 16-byte aligned"), (dict(nbytes=need - 1), b"workspace is too small"),
           (dict(nbytes=0), b"workspace is too small"), (dict(M=2 ** 31 - 1, dim=289), b"2^24 workgroups")]
    for kw, msg in bad:
        assert _call(L, **kw) == -1 and msg in L.ss_last_error(), (kw, L.ss_last_error())
    # the three workspace messages are the deterministic entries' own
    one = ctypes.c_void_p(ONE)
    for ws, nbytes in [(None, need), (odd, need), (ONE, need - 1)]:
        assert _call(L, ws=ws, nbytes=nbytes) == -1
        m0 = L.ss_last_error()
        assert L.ss_wgrad_bf16_det(one, one, one, 1024, 64, 64, 64, 64, 64, ws, min(nbytes, 100), None) == -1 and L.ss_last_error() == m0, m0
    # what is allowed is not refused by these rules (the workspace is what fails here): a padded row stride, a base that is only 4-byte aligned, one row, one column
    for kw in (dict(ldx=300), dict(x=20), dict(M=1), dict(dim=1, ldx=1), dict(M=2 ** 31 - 1, dim=64)):
        assert _call(L, ws=None, **kw) == -1 and b"null workspace" in L.ss_last_error(), (kw, L.ss_last_error())


def test_python_switches_refuse_what_they_cannot_honour():
    import torch
    from smplsim_amd.agents.ppo import AgentPPO, PPOConfig
    from smplsim_amd.learning.fused_norm import LibRunningNorm
    from smplsim_amd.learning.networks import RunningNorm
    assert PPOConfig().fused_norm is False

    class Env:                                                      # AgentPPO reads these before it builds anything
        device, obs_size, nu, num_envs = torch.device("cpu"), 8, 2, 4

    with pytest.raises(ValueError, match="mfma_update"):
        AgentPPO(Env(), PPOConfig(fused_norm=True, hidden=(16,)))
    with pytest.raises(RuntimeError, match="no CPU path"):
        AgentPPO(Env(), PPOConfig(fused_norm=True, mfma_update=True, hidden=(16,)))
    agent = AgentPPO(Env(), PPOConfig(hidden=(16,)))                # the flag off: no object of the new path exists
    assert agent.lib_norm is None
    with pytest.raises(ValueError, match="demean"):
        LibRunningNorm(RunningNorm(8, demean=False))
    with pytest.raises(ValueError, match="destd"):
        LibRunningNorm(RunningNorm(8, destd=False))
    with pytest.raises(RuntimeError, match="no CPU path"):
        LibRunningNorm(RunningNorm(8))
