"""The optimiser step, host side (-m "not gpu"): the workspace query of ss_adam_step against the tile rule of include/smplsim_mlp.h, its argument checks (they
run before any launch, so no GPU is needed: cf. test_ppo_head_cpu.py), and the Python switches."""
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


def _table(*descs):
    """descs: dicts over the fields of ss_adam_tensor; the defaults describe a valid dense [rows, cols] tensor without images."""
    from smplsim_amd._cabi import AdamTensor
    t = (AdamTensor * max(1, len(descs)))()
    for i, d in enumerate(descs):
        a = dict(p=ONE, m=ONE, v=ONE, g=ONE, w_bf16=None, wt_bf16=None, rows=64, cols=64, ldg=None, ld_w=0, ld_wt=0)
        assert set(d) <= set(a)
        a.update(d)
        if a["ldg"] is None:
            a["ldg"] = a["cols"]
        t[i] = AdamTensor(*a.values())
    return t


def test_workspace_query_counts_tiles_of_64_by_64(L):
    # tiles by hand: 1x1 -> 1; 64x64 -> 1; 65x64 -> 2 x 1; 69x512 -> 2 x 8; 2048x289 -> 32 x 5
    tiles = {(1, 1): 1, (64, 64): 1, (65, 64): 2, (69, 512): 16, (2048, 289): 160}
    for (r, c), n in tiles.items():
        assert L.ss_adam_step_workspace(_table(dict(rows=r, cols=c)), 1) == (n + 1) * 8, (r, c)
        assert L.ss_adam_step_workspace(_table(dict(rows=c, cols=r)), 1) == (n + 1) * 8, (c, r)
    shapes = list(tiles)
    assert L.ss_adam_step_workspace(_table(*[dict(rows=r, cols=c) for r, c in shapes]), len(shapes)) == (1 + 1 + 2 + 16 + 160 + 1) * 8
    assert L.ss_adam_step_workspace(_table(*[dict(rows=r, cols=c) for r, c in shapes[::-1]]), len(shapes)) == 181 * 8
    # strides and images do not change the count
    assert L.ss_adam_step_workspace(_table(dict(rows=69, cols=512, ldg=640, w_bf16=ONE, ld_w=512, wt_bf16=ONE, ld_wt=128)), 1) == 17 * 8
    # 32 tensors are served, 33 are not
    assert L.ss_adam_step_workspace(_table(*[dict(rows=1, cols=65)] * 32), 32) == (64 + 1) * 8
    for t, n in [(_table(*[dict()] * 33), 33), (_table(dict()), 0), (_table(dict()), -1)]:
        assert L.ss_adam_step_workspace(t, n) < 0 and b"count" in L.ss_last_error(), n
    assert L.ss_adam_step_workspace(None, 1) < 0 and b"null argument" in L.ss_last_error()
    for d, msg in [(dict(rows=0), b"rows >= 1"), (dict(cols=-1, ldg=1), b"cols >= 1"), (dict(p=None), b"null argument"), (dict(ldg=63), b"row strides"),
                   (dict(w_bf16=ONE, ld_w=60), b"row strides")]:
        assert L.ss_adam_step_workspace(_table(d), 1) < 0 and msg in L.ss_last_error(), d


def _call(L, table=None, count=1, step=1, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.0, max_norm=1.0, norm=ONE, ws=ONE, nbytes=1 << 40):
    table = _table(dict()) if table is None else table
    return L.ss_adam_step(table, count, step, lr, beta1, beta2, eps, wd, max_norm, norm, ws, nbytes, None)


def test_adam_step_checks_its_arguments_before_any_launch(L):
    odd, mis = 24, 18
    nan = float("nan")
    bad_desc = [(dict(p=None), b"null argument"), (dict(m=None), b"null argument"), (dict(v=None), b"null argument"), (dict(g=None), b"null argument"),
                (dict(rows=0), b"rows >= 1"), (dict(rows=-4), b"rows >= 1"), (dict(cols=0, ldg=8), b"cols >= 1"),
                (dict(ldg=63), b"row strides"), (dict(rows=69, cols=1, ldg=0), b"row strides"),
                (dict(w_bf16=ONE, ld_w=56), b"row strides"), (dict(wt_bf16=ONE, ld_wt=56), b"row strides"), (dict(rows=69, cols=8, wt_bf16=ONE, ld_wt=64), b"row strides"),
                (dict(w_bf16=ONE, ld_w=68), b"multiple of 8"), (dict(wt_bf16=ONE, ld_wt=65), b"multiple of 8"),
                (dict(w_bf16=odd, ld_w=64), b"16-byte aligned base"), (dict(wt_bf16=mis, ld_wt=64), b"16-byte aligned base"),
                (dict(w_bf16=ONE, ld_w=64, wt_bf16=odd, ld_wt=64), b"16-byte aligned base")]
    for d, msg in bad_desc:
        assert _call(L, _table(d)) == -1 and msg in L.ss_last_error(), (d, L.ss_last_error())
        assert _call(L, _table(dict(), d), count=2) == -1 and msg in L.ss_last_error(), (d, L.ss_last_error())      # the second descriptor is checked like the first
    assert L.ss_adam_step(None, 1, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, ONE, ONE, 1 << 40, None) == -1 and b"null argument" in L.ss_last_error()
    need = L.ss_adam_step_workspace(_table(dict()), 1)
    assert need == 16
    bad = [(dict(count=0), b"count"), (dict(count=-2), b"count"), (dict(table=_table(*[dict()] * 33), count=33), b"count <= 32"),
           (dict(step=0), b"step >= 1"), (dict(step=-1), b"step >= 1"),
           (dict(beta1=1.0), b"betas"), (dict(beta1=-0.1), b"betas"), (dict(beta2=1.0), b"betas"), (dict(beta2=-1e-3), b"betas"), (dict(beta1=nan), b"betas"),
           (dict(beta2=nan), b"betas"), (dict(eps=-1e-8), b"eps >= 0"), (dict(eps=nan), b"eps >= 0"),
           (dict(lr=nan), b"NaN"), (dict(wd=nan), b"NaN"), (dict(max_norm=nan), b"NaN"),
           (dict(ws=None), b"null workspace"), (dict(ws=odd), b"workspace must be 16-byte aligned"), (dict(nbytes=need - 1), b"workspace is too small"),
           (dict(nbytes=0), b"workspace is too small")]
    for kw, msg in bad:
        assert _call(L, **kw) == -1 and msg in L.ss_last_error(), (kw, L.ss_last_error())
    # the three workspace messages are the deterministic entries' own
    one = ctypes.c_void_p(ONE)
    for ws, nbytes in [(None, need), (odd, need), (ONE, need - 1)]:
        assert _call(L, ws=ws, nbytes=nbytes) == -1
        m0 = L.ss_last_error()
        assert L.ss_wgrad_bf16_det(one, one, one, 1024, 64, 64, 64, 64, 64, ws, min(nbytes, 100), None) == -1 and L.ss_last_error() == m0, m0
    # what is allowed is not refused by these rules (the workspace is what fails here): no clipping in its three spellings, no grad_norm, a strided column
    # gradient, images with padded strides, 32 tensors, eps = 0, beta = 0
    ok = [dict(max_norm=0.0), dict(max_norm=-1.0), dict(max_norm=float("inf")), dict(norm=None), dict(eps=0.0, beta1=0.0, beta2=0.0, wd=0.01, step=1 << 30),
          dict(table=_table(dict(rows=69, cols=1, ldg=8))), dict(table=_table(dict(rows=69, cols=512, ldg=640, w_bf16=ONE, ld_w=512, wt_bf16=ONE, ld_wt=128))),
          dict(table=_table(dict(g=mis, p=mis))), dict(table=_table(*[dict(rows=1, cols=65)] * 32), count=32)]
    for kw in ok:
        assert _call(L, ws=None, **kw) == -1 and b"null workspace" in L.ss_last_error(), (kw, L.ss_last_error())


def test_python_switches_refuse_what_they_cannot_honour():
    import torch
    from smplsim_amd.agents.ppo import AgentPPO, PPOConfig
    from smplsim_amd.learning.fused_optim import LibAdam
    assert PPOConfig().fused_optimizer is False

    class Env:                                                      # AgentPPO reads these before it builds anything
        device, obs_size, nu, num_envs = torch.device("cpu"), 8, 2, 4

    with pytest.raises(RuntimeError, match="no CPU path"):
        AgentPPO(Env(), PPOConfig(fused_optimizer=True, hidden=(16,)))
    agent = AgentPPO(Env(), PPOConfig(hidden=(16,)))                # the flag off: plain torch optimisers, as before
    assert type(agent.optimizer_policy) is torch.optim.Adam and type(agent.optimizer_value) is torch.optim.Adam
    params = [torch.nn.Parameter(torch.zeros(3, 5)), torch.nn.Parameter(torch.zeros(5))]
    lib_opt, ref = LibAdam(params, lr=1e-4, max_grad_norm=2.0), torch.optim.Adam(params)
    assert lib_opt.param_groups[0].keys() == ref.param_groups[0].keys() and list(lib_opt.param_groups[0]) == list(ref.param_groups[0])
    assert "max_grad_norm" not in lib_opt.param_groups[0] and lib_opt.max_grad_norm == 2.0 and lib_opt.last_grad_norm is None
    assert lib_opt.state_dict()["param_groups"][0].keys() == ref.state_dict()["param_groups"][0].keys()
    for kw in (dict(amsgrad=True), dict(maximize=True), dict(capturable=True), dict(differentiable=True), dict(fused=True), dict(foreach=True)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            LibAdam(params, **kw)
    params[0].grad = torch.ones(3, 5)
    with pytest.raises(RuntimeError, match="no CPU path"):
        lib_opt.step()
    # a state saved by a plain Adam loads (its `step` stays a CPU fp32 tensor), and an option the kernel does not implement is refused at load time too
    params[1].grad = torch.ones(5)
    ref.step()
    lib_opt.load_state_dict(ref.state_dict())
    st = lib_opt.state[params[0]]
    assert st["step"].device.type == "cpu" and st["step"].dtype == torch.float32 and float(st["step"]) == 1.0 and set(st) == {"step", "exp_avg", "exp_avg_sq"}
    sd = ref.state_dict()
    sd["param_groups"][0]["amsgrad"] = True
    with pytest.raises(ValueError, match="amsgrad"):
        lib_opt.load_state_dict(sd)
