"""The deterministic PPO update, host side (-m "not gpu"): the workspace size queries against the formulas of include/smplsim_mlp.h, the argument
checks of ss_wgrad_bf16_det / ss_linear_bf16_dx_det (they run before any launch, so no GPU is needed: cf. test_host_logic.py), and the Python
switches."""
import ctypes

import pytest


def split_256(tiles, nkt):
    """smplsim_mlp.hip's split_256 restated: (K shares, K tiles per share)."""
    ks = max(1, min(256 // tiles, nkt // 8))
    kper = (nkt + ks - 1) // ks
    kper += kper & 1
    return (nkt + kper - 1) // kper, kper


def wgrad_shares(Mb, n_out, n_in):
    return split_256(((n_in + 255) // 256) * ((n_out + 255) // 256), Mb // 64)


# (n_out, n_in, shares) at the production widths, batch 53 248 rows: the table of the design document
PRODUCTION = [(2048, 384, 16), (1536, 2048, 5), (1024, 1536, 10), (1024, 1024, 16), (512, 1024, 32), (512, 512, 60), (72, 512, 104)]


@pytest.fixture(scope="module")
def L():
    import torch  # noqa: F401  (always before the library: one HIP runtime per process)
    from smplsim_amd import _cabi, _lib
    _lib.build()
    lib = _cabi.bind_mlp(ctypes.CDLL(_lib.LIB_PATH))
    lib.ss_last_error.restype = ctypes.c_char_p
    return lib


def test_workspace_queries_equal_the_documented_formulas(L):
    for n_out, n_in, shares in PRODUCTION:
        S, kper = wgrad_shares(53248, n_out, n_in)
        assert S == shares and (S - 1) * kper < 832 <= S * kper, (n_out, n_in, S, kper)     # no empty share
        assert L.ss_wgrad_bf16_det_workspace(53248, n_out, n_in) == S * n_out * n_in * 4
    assert max(L.ss_wgrad_bf16_det_workspace(53248, o, i) for o, i, _ in PRODUCTION) == 16 * 1024 * 1024 * 4        # 67 MB: one workspace per network
    for Mb, n_out, n_in in [(128, 72, 136), (3200, 72, 136), (256, 8, 8), (8192, 256, 256), (1024, 520, 264), (4224, 2048, 384), (4224, 72, 8)]:
        S, _ = wgrad_shares(Mb, n_out, n_in)
        assert L.ss_wgrad_bf16_det_workspace(Mb, n_out, n_in) == S * n_out * n_in * 4, (Mb, n_out, n_in)
    assert wgrad_shares(128, 72, 136)[0] == 1 and wgrad_shares(3200, 72, 136) == (5, 10) and wgrad_shares(8192, 256, 256) == (16, 8)
    for M, N, K in [(53248, 2048, 1536), (2049, 300, 384), (4100, 1024, 640), (2048, 256, 128), (4224, 512, 128)]:
        assert L.ss_linear_bf16_dx_det_workspace(M, N, K) == 2 * ((M + 255) // 256) * N * 4, (M, N, K)
    assert L.ss_linear_bf16_dx_det_workspace(53248, 2048, 1536) == 416 * 2048 * 4
    # invalid arguments: negative, with a message
    for args in [(1000, 64, 64), (0, 64, 64), (1024, 60, 64), (1024, 64, 0)]:
        assert L.ss_wgrad_bf16_det_workspace(*args) < 0 and b"ss_wgrad_bf16_det_workspace" in L.ss_last_error(), args
    for args in [(1000, 512, 256), (4096, 128, 256), (4096, 512, 192), (4096, 512, 0)]:
        assert L.ss_linear_bf16_dx_det_workspace(*args) < 0 and b"ss_linear_bf16_dx_det_workspace" in L.ss_last_error(), args


def test_det_entries_check_their_workspace_before_any_launch(L):
    one, odd = ctypes.c_void_p(16), ctypes.c_void_p(24)            # never dereferenced: every call below fails its checks first
    need = L.ss_wgrad_bf16_det_workspace(1024, 64, 64)
    assert need == 2 * 64 * 64 * 4
    assert L.ss_wgrad_bf16_det(one, one, one, 1024, 64, 64, 64, 64, 64, None, need, None) == -1 and b"null workspace" in L.ss_last_error()
    assert L.ss_wgrad_bf16_det(one, one, one, 1024, 64, 64, 64, 64, 64, one, need - 1, None) == -1 and b"too small" in L.ss_last_error()
    assert L.ss_wgrad_bf16_det(one, one, one, 1024, 64, 64, 64, 64, 64, one, 0, None) == -1 and b"too small" in L.ss_last_error()
    assert L.ss_wgrad_bf16_det(one, one, one, 1024, 64, 64, 64, 64, 64, odd, need, None) == -1 and b"16-byte aligned" in L.ss_last_error()
    need = L.ss_linear_bf16_dx_det_workspace(4096, 512, 256)
    assert need == 32 * 512 * 4
    assert L.ss_linear_bf16_dx_det(one, one, one, one, one, 4096, 512, 256, 512, None, need, None) == -1 and b"null workspace" in L.ss_last_error()
    assert L.ss_linear_bf16_dx_det(one, one, one, one, one, 4096, 512, 256, 512, one, need - 1, None) == -1 and b"too small" in L.ss_last_error()
    assert L.ss_linear_bf16_dx_det(one, one, one, one, one, 4096, 512, 256, 512, one, 0, None) == -1 and b"too small" in L.ss_last_error()
    assert L.ss_linear_bf16_dx_det(one, one, one, one, one, 4096, 512, 256, 512, odd, need, None) == -1 and b"16-byte aligned" in L.ss_last_error()


def test_det_entries_apply_the_argument_rules_of_their_default_twins(L):
    """The same bad arguments to both forms (the deterministic one with a workspace that would pass): the same status and the same message."""
    one, odd = ctypes.c_void_p(16), ctypes.c_void_p(24)
    big = 1 << 40
    # (dz, h, dw, Mb, n_out, n_in, ldz, ldh, ldw)
    wgrad_bad = [(one, None, one, 1024, 64, 64, 64, 64, 64), (None, one, one, 1024, 64, 64, 64, 64, 64), (one, one, None, 1024, 64, 64, 64, 64, 64),
                 (one, one, one, 1000, 64, 64, 64, 64, 64), (one, one, one, 0, 64, 64, 64, 64, 64), (one, one, one, 1024, 60, 64, 64, 64, 64),
                 (one, one, one, 1024, 64, 60, 64, 64, 64), (one, one, one, 1024, 64, 64, 32, 64, 64), (one, one, one, 1024, 64, 64, 64, 32, 64),
                 (one, one, one, 1024, 64, 64, 64, 64, 56), (one, one, one, 1024, 64, 64, 68, 64, 64), (one, one, one, 1024, 64, 64, 64, 68, 64),
                 (odd, one, one, 1024, 64, 64, 64, 64, 64), (one, odd, one, 1024, 64, 64, 64, 64, 64), (one, one, one, 1 << 20, 64, 64, 4096, 64, 64)]
    for a in wgrad_bad:
        r0 = L.ss_wgrad_bf16(*a, None); m0 = L.ss_last_error()
        r1 = L.ss_wgrad_bf16_det(*a, one, big, None); m1 = L.ss_last_error()
        assert r0 == r1 == -1 and m0 == m1, (a[3:], r0, r1, m0, m1)
    # (x, w, mul, y, colsum, M, N, K, ldy)
    dx_bad = [(one, one, None, one, one, 4096, 512, 256, 512), (one, one, one, None, one, 4096, 512, 256, 512), (one, one, one, one, None, 4096, 512, 256, 512),
              (None, one, one, one, one, 4096, 512, 256, 512), (one, None, one, one, one, 4096, 512, 256, 512), (one, one, one, one, one, 1000, 512, 256, 512),
              (one, one, one, one, one, 4096, 128, 256, 128), (one, one, one, one, one, 4096, 512, 192, 512), (one, one, one, one, one, 4096, 512, 100, 512),
              (one, one, one, one, one, 4096, 512, 256, 500), (one, one, one, one, one, 4096, 512, 0, 512), (one, one, one, one, one, 1 << 24, 512, 256, 512)]
    for a in dx_bad:
        r0 = L.ss_linear_bf16_dx(*a, None); m0 = L.ss_last_error()
        r1 = L.ss_linear_bf16_dx_det(*a, one, big, None); m1 = L.ss_last_error()
        assert r0 == r1 == -1 and m0 == m1, (a[5:], r0, r1, m0, m1)


def test_python_switches_refuse_what_they_cannot_honour():
    import torch
    from smplsim_amd.agents.ppo import AgentPPO, PPOConfig
    from smplsim_amd.learning.fused_train import FusedMLPTrain
    assert PPOConfig().deterministic_update is False

    class Env:                                                      # AgentPPO reads these before it builds anything
        device, obs_size, nu, num_envs = torch.device("cpu"), 8, 2, 4

    with pytest.raises(ValueError, match="mfma_update"):
        AgentPPO(Env(), PPOConfig(deterministic_update=True, hidden=(16,)))
    hidden = [torch.nn.Linear(8, 64), torch.nn.Linear(64, 64)]
    with pytest.raises(RuntimeError, match="no CPU path"):
        FusedMLPTrain(hidden, torch.nn.Linear(64, 2), "silu", deterministic=True)
