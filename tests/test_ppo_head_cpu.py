"""The PPO loss heads, host side (-m "not gpu"): the workspace queries of ss_ppo_policy_head / ss_value_head against the formulas of include/smplsim_mlp.h,
their argument checks (they run before any launch, so no GPU is needed: cf. test_det_update_cpu.py), and the Python switches."""
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


def test_workspace_queries_follow_the_documented_formulas(L):
    prev = 0
    for M in (1, 2, 127, 128, 129, 1000, 4100, 53248, 1 << 24):
        n = L.ss_ppo_policy_head_workspace(M, 69)
        assert n == -(-M // 128) * (4 + 69) * 8 and n >= prev and n > 0, (M, n)
        prev = n
    assert L.ss_ppo_policy_head_workspace(53248, 69) == 416 * 73 * 8
    for dim in (1, 63, 64, 65, 130, 256):
        assert L.ss_ppo_policy_head_workspace(257, dim) == 3 * (4 + dim) * 8
    prev = 0
    for M in (1, 1023, 1024, 1025, 4100, 53248, 1 << 24):
        n = L.ss_value_head_workspace(M)
        assert n == -(-M // 1024) * 8 and n >= prev and n > 0, (M, n)
        prev = n
    for args in [(0, 69), (-5, 69), (100, 0), (100, -1), (100, 257)]:
        assert L.ss_ppo_policy_head_workspace(*args) < 0 and b"ss_ppo_policy_head" in L.ss_last_error(), args
    for M in (0, -1):
        assert L.ss_value_head_workspace(M) < 0 and b"ss_value_head" in L.ss_last_error(), M


# (mean, ldm, actions, lda, log_std, adv, old_logp, M, dim, clip_eps, logp, dmean, ldd, dmean_is_bf16, dlog_std, stats, workspace, bytes)
def _policy_args(**kw):
    one = ctypes.c_void_p(16)                                      # never dereferenced: every call in this file fails its checks first
    a = dict(mean=one, ldm=72, actions=one, lda=72, log_std=one, adv=one, old_logp=one, M=1000, dim=69, clip_eps=0.2, logp=one, dmean=one, ldd=72,
             bf16=0, dlog_std=one, stats=one, ws=one, bytes=1 << 40)
    assert set(kw) <= set(a)
    a.update(kw)
    return tuple(a.values()) + (None,)


def test_policy_head_checks_its_arguments_before_any_launch(L):
    odd, mis = ctypes.c_void_p(24), ctypes.c_void_p(18)
    need = L.ss_ppo_policy_head_workspace(1000, 69)
    bad = [(dict(mean=None), b"null argument"), (dict(actions=None), b"null argument"), (dict(log_std=None), b"null argument"), (dict(adv=None), b"null argument"),
           (dict(old_logp=None), b"null argument"), (dict(dmean=None), b"null argument"), (dict(stats=None), b"null argument"),
           (dict(M=0), b"M >= 1"), (dict(M=-3), b"M >= 1"), (dict(dim=0), b"1 <= dim"), (dict(dim=257, ldm=512, lda=512, ldd=512), b"dim <= 256"),
           (dict(ldm=68), b"row strides"), (dict(lda=68), b"row strides"), (dict(ldd=68), b"row strides"), (dict(ldd=64, bf16=1), b"row strides"),
           (dict(clip_eps=0.0), b"clip_eps"), (dict(clip_eps=1.0), b"clip_eps"), (dict(clip_eps=-0.2), b"clip_eps"), (dict(clip_eps=1.5), b"clip_eps"),
           (dict(clip_eps=float("nan")), b"clip_eps"),
           (dict(bf16=1, ldd=76), b"multiple of 8"), (dict(bf16=1, ldd=69), b"multiple of 8"), (dict(bf16=1, dmean=odd), b"16-byte aligned base"),
           (dict(bf16=1, dmean=mis), b"16-byte aligned base"),
           (dict(ws=None), b"null workspace"), (dict(ws=odd), b"workspace must be 16-byte aligned"), (dict(bytes=need - 1), b"workspace is too small"),
           (dict(bytes=0), b"workspace is too small")]
    for kw, msg in bad:
        assert L.ss_ppo_policy_head(*_policy_args(**kw)) == -1 and msg in L.ss_last_error(), (kw, L.ss_last_error())
    # the three workspace messages are the deterministic entries' own
    one = ctypes.c_void_p(16)
    for ws, nbytes in [(None, need), (odd, need), (one, need - 1)]:
        assert L.ss_ppo_policy_head(*_policy_args(ws=ws, bytes=nbytes)) == -1
        m0 = L.ss_last_error()
        assert L.ss_wgrad_bf16_det(one, one, one, 1024, 64, 64, 64, 64, 64, ws, min(nbytes, 100), None) == -1 and L.ss_last_error() == m0, m0
    # what is allowed is not refused by these rules: an f32 dmean may have any ldd >= dim and any alignment (the workspace is what fails here)
    assert L.ss_ppo_policy_head(*_policy_args(ldd=69, dmean=mis, logp=None, dlog_std=None, ws=None)) == -1 and b"null workspace" in L.ss_last_error()


def test_value_head_checks_its_arguments_before_any_launch(L):
    one, odd = ctypes.c_void_p(16), ctypes.c_void_p(24)
    need = L.ss_value_head_workspace(5000)
    assert need == 5 * 8

    def call(pred=one, target=one, M=5000, dpred=one, ldd=1, bf16=0, loss=one, ws=one, nbytes=1 << 40):
        return L.ss_value_head(pred, target, M, dpred, ldd, bf16, loss, ws, nbytes, None)

    bad = [(dict(pred=None), b"null argument"), (dict(target=None), b"null argument"), (dict(dpred=None), b"null argument"), (dict(loss=None), b"null argument"),
           (dict(M=0), b"M >= 1"), (dict(ldd=0), b"row strides"), (dict(bf16=1, ldd=1), b"multiple of 8"), (dict(bf16=1, ldd=12), b"multiple of 8"),
           (dict(bf16=1, ldd=8, dpred=odd), b"16-byte aligned base"),
           (dict(ws=None), b"null workspace"), (dict(ws=odd), b"workspace must be 16-byte aligned"), (dict(nbytes=need - 1), b"workspace is too small"),
           (dict(nbytes=0), b"workspace is too small")]
    for kw, msg in bad:
        assert call(**kw) == -1 and msg in L.ss_last_error(), (kw, L.ss_last_error())


def test_python_switches_refuse_what_they_cannot_honour():
    import torch
    from smplsim_amd.agents.ppo import AgentPPO, PPOConfig
    from smplsim_amd.learning.fused_loss import ppo_surrogate, value_mse
    assert PPOConfig().fused_loss is False

    class Env:                                                      # AgentPPO reads these before it builds anything
        device, obs_size, nu, num_envs = torch.device("cpu"), 8, 2, 4

    with pytest.raises(RuntimeError, match="no CPU path"):
        AgentPPO(Env(), PPOConfig(fused_loss=True, hidden=(16,)))
    agent = AgentPPO(Env(), PPOConfig(hidden=(16,)))                # the flag off: the agent is built as before, without the heads
    assert agent.surrogate is None and agent.value_mse is None
    mean = torch.zeros(5, 2, requires_grad=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ppo_surrogate(mean, torch.zeros(1, 2), torch.zeros(5, 2), torch.zeros(5, 1), torch.zeros(5, 1), 0.2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        value_mse(torch.zeros(5, 1, requires_grad=True), torch.zeros(5, 1))
