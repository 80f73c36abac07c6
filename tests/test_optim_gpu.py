"""The optimiser step on the GPU (include/smplsim_mlp.h: ss_adam_step; learning/fused_optim.py: LibAdam; FusedMLPTrain(weight_images=True); PPOConfig.fused_optimizer).

The bound of every comparison against float64 is taken in the test itself, as in test_ppo_head_gpu.py: torch's own fp32 path (clip_grad_norm_ + torch.optim.Adam) runs on
the same inputs, its largest error against float64 is e32 (per output kind), and the kernel's largest error must be <= FACTOR * e32."""
import copy
import ctypes as C
import math

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from test_det_update_gpu import _agent_state, _same_bits  # noqa: E402
from test_gemm_kernels_gpu import _lib, _p, _record, _st  # noqa: E402

FACTOR = 4.0                 # test_ppo_head_gpu.py's: a different order of operations than torch's fp32 path, not a different precision class
MARGIN = 512                 # doubles of workspace beyond the documented size: they must keep what they held
LR, B1, B2, EPS = 5e-5, 0.9, 0.999, 1e-8
NAN = float("nan")

# (rows, cols, ldg): edge tiles in both directions, a single-row head, a strided bias gradient ([69, 1] as dbh[:69, 0] of an [72, 8] buffer)
SET = [(1, 1, 1), (69, 1, 8), (1, 69, 69), (69, 512, 640), (257, 300, 384), (64, 64, 64), (1, 512, 512)]
# (rows, cols, ldg, ld_w, ld_wt or None)
IMAGE_SET = [(69, 512, 640, 512, 128), (257, 300, 384, 384, 264), (1, 512, 512, 512, 8), (2048, 289, 384, 384, None)]


def _tiles(rows, cols):
    return -(-rows // 64) * -(-cols // 64)


def _bits(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


class _Tensors:
    """The device side of one call: p, m, v dense; each g inside a NaN-filled [rows + 1, ldg] buffer; the images (where asked for) NaN-filled with two extra rows."""

    def __init__(self, shapes, p, m, v, g):
        from smplsim_amd._cabi import AdamTensor
        self.shapes = shapes
        self.p, self.m, self.v = [[t.clone().cuda().contiguous() for t in ts] for ts in (p, m, v)]
        self.gbuf, self.w, self.wt = [], [], []
        self.table = (AdamTensor * len(shapes))()
        for i, s in enumerate(shapes):
            rows, cols, ldg = s[:3]
            ld_w, ld_wt = (s[3], s[4]) if len(s) > 3 else (None, None)
            gb = torch.full((rows + 1, ldg), NAN, device="cuda")
            gb[:rows, :cols] = g[i].cuda()
            self.gbuf.append(gb)
            bf = dict(dtype=torch.bfloat16, device="cuda")
            self.w.append(torch.full((rows + 2, ld_w), NAN, **bf) if ld_w else None)
            self.wt.append(torch.full((cols + 2, ld_wt), NAN, **bf) if ld_wt else None)
            ptr = lambda t: None if t is None else t.data_ptr()
            self.table[i] = AdamTensor(self.p[i].data_ptr(), self.m[i].data_ptr(), self.v[i].data_ptr(), gb.data_ptr(), ptr(self.w[i]), ptr(self.wt[i]), rows, cols, ldg,
                                       ld_w or 0, ld_wt or 0)
        self.g0 = [gb.clone() for gb in self.gbuf]
        self.T = sum(_tiles(s[0], s[1]) for s in shapes)

    def g(self, i):
        rows, cols = self.shapes[i][:2]
        return self.gbuf[i][:rows, :cols]


def _workspace(nbytes, fill="nan"):
    assert nbytes > 0
    n = nbytes // 8 + MARGIN
    if fill == "nan":
        return torch.full((n,), NAN, dtype=torch.float64, device="cuda")
    if fill == "ones":
        return torch.ones(n, dtype=torch.float64, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(int(fill))
    return torch.randint(0, 256, (n * 8,), dtype=torch.uint8, device="cuda", generator=gen).view(torch.float64)


def _step(ts, step, wd=0.0, max_norm=0.0, fill="nan", kick=None):
    """One ss_adam_step call over ts (in place).  Returns (grad_norm [1], workspace[:T + 1]); checks that nothing beyond the documented workspace and no gradient was written."""
    L = _lib()
    need = L.ss_adam_step_workspace(ts.table, len(ts.shapes))
    assert need == (ts.T + 1) * 8, (need, ts.T, L.ss_last_error())
    ws = _workspace(need, fill)
    tail = ws[need // 8:].clone()
    norm = torch.full((3,), NAN, device="cuda")
    torch.cuda.synchronize()
    if kick is not None:
        kick()                                                     # work for a second stream, enqueued right before the call under test
    rc = L.ss_adam_step(ts.table, len(ts.shapes), step, LR, B1, B2, EPS, wd, max_norm, _p(norm), _p(ws), need, _st())
    assert rc == 0, L.ss_last_error()
    torch.cuda.synchronize()
    assert torch.equal(_bits(ws[need // 8:]), _bits(tail)), "a write beyond the documented workspace"
    assert torch.isnan(norm[1:]).all()
    for gb, g0 in zip(ts.gbuf, ts.g0):
        assert torch.equal(_bits(gb), _bits(g0)), "a gradient buffer was modified"
    return norm[:1], ws[:need // 8]


def _adam64(p, m, v, g, step, wd, max_norm):
    """The header's formula in float64 on lists of fp32 CPU tensors: (p', m', v', norm) in float64."""
    p, m, v, g = [[t.double() for t in ts] for ts in (p, m, v, g)]
    S = sum((x * x).sum() for x in g)
    norm = torch.sqrt(S)
    c = min(1.0, max_norm / (norm.item() + 1e-6)) if 0 < max_norm < math.inf else 1.0
    out = ([], [], [])
    for pi, mi, vi, gi in zip(p, m, v, g):
        g1 = c * gi + wd * pi
        m1 = B1 * mi + (1 - B1) * g1
        v1 = B2 * vi + (1 - B2) * g1 * g1
        p1 = pi - (LR / (1 - B1 ** step)) * m1 / (torch.sqrt(v1) / math.sqrt(1 - B2 ** step) + EPS)
        for o, t in zip(out, (p1, m1, v1)):
            o.append(t)
    return (*out, norm.reshape(1))


def _adam32(p, m, v, g, step, wd, max_norm):
    """clip_grad_norm_ + torch.optim.Adam(foreach=False) on the CPU in fp32 from the same inputs, the state injected: (p', m', v', norm)."""
    ps = [torch.nn.Parameter(t.clone()) for t in p]
    opt = torch.optim.Adam(ps, lr=LR, betas=(B1, B2), eps=EPS, weight_decay=wd, foreach=False)
    for q, mi, vi, gi in zip(ps, m, v, g):
        opt.state[q] = dict(step=torch.tensor(float(step - 1)), exp_avg=mi.clone(), exp_avg_sq=vi.clone())
        q.grad = gi.clone()
    norm = torch.nn.utils.clip_grad_norm_(ps, max_norm if max_norm > 0 else math.inf, foreach=False)      # (off: the coefficient clamps to 1, the norm is still formed)
    opt.step()
    return [q.detach() for q in ps], [opt.state[q]["exp_avg"] for q in ps], [opt.state[q]["exp_avg_sq"] for q in ps], norm.reshape(1)


def _maxerr(xs, refs):
    return max((x.detach().double().cpu().reshape(-1) - r.double().reshape(-1)).abs().max().item() for x, r in zip(xs, refs))


# ---------------------------------------------------------------------------------------------------------------- 1: against float64, step by step
@pytest.mark.parametrize("max_norm", [0.5, 1e9, 0.0], ids=["clip", "noclip", "off"])
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_three_steps_against_float64(wd, max_norm):
    gen = torch.Generator().manual_seed(1)
    p = [torch.randn(r, c, generator=gen) * 0.05 for r, c, _ in SET]
    m, v = [torch.zeros_like(t) for t in p], [torch.zeros_like(t) for t in p]
    for step in (1, 2, 3):
        g = [torch.randn(r, c, generator=gen) * 10.0 ** (1 - step) for r, c, _ in SET]
        ts = _Tensors(SET, p, m, v, g)
        norm, _ = _step(ts, step, wd, max_norm)
        ref, t32 = _adam64(p, m, v, g, step, wd, max_norm), _adam32(p, m, v, g, step, wd, max_norm)
        if step == 1 and max_norm == 0.5:
            assert ref[3].item() > 0.5                                                                   # clipping is active
        got = (ts.p, ts.m, ts.v, [norm])
        rows = {k: (_maxerr(got[i], ref[i]), _maxerr(t32[i], ref[i])) for i, k in enumerate(("p", "m", "v"))}
        rows["norm"] = (_maxerr([norm], [ref[3]]), _maxerr([t32[3]], [ref[3]]))
        tag = f"adam_step{step}_wd{wd}_max{max_norm}"
        _record(tag, **{k: [e, e32] for k, (e, e32) in rows.items()})                                    # [kernel, e32] per output kind
        print(tag, {k: (f"{e:.3g}", f"{e32:.3g}") for k, (e, e32) in rows.items()})
        for k, (e, e32) in rows.items():
            assert not math.isnan(e) and e <= FACTOR * e32, (tag, k, e, e32)
        p, m, v = [[t.cpu() for t in x] for x in (ts.p, ts.m, ts.v)]                                      # the next step starts from what the kernel stored


# ---------------------------------------------------------------------------------------------------------------- 2: the images
def _image_inputs(seed=2):
    gen = torch.Generator().manual_seed(seed)
    p = [torch.randn(s[0], s[1], generator=gen) * 0.05 for s in IMAGE_SET]
    m = [torch.randn(s[0], s[1], generator=gen) * 0.01 for s in IMAGE_SET]
    v = [torch.rand(s[0], s[1], generator=gen) * 1e-3 for s in IMAGE_SET]
    g = [torch.randn(s[0], s[1], generator=gen) * 0.1 for s in IMAGE_SET]
    return p, m, v, g


def test_images_are_the_rounded_stored_weights_and_nothing_else_is_written():
    ts = _Tensors(IMAGE_SET, *_image_inputs())
    p_old = [t.clone() for t in ts.p]
    _step(ts, 4, 0.01, 1.0)
    for i, (rows, cols, _, _, ld_wt) in enumerate(IMAGE_SET):
        pn = ts.p[i]
        assert not torch.equal(pn, p_old[i]) and torch.isfinite(pn).all()
        w = ts.w[i]
        assert torch.equal(_bits(w[:rows, :cols]), _bits(pn.to(torch.bfloat16))), (i, "w_bf16")
        assert torch.isnan(w[rows:]).all() and torch.isnan(w[:, cols:]).all(), (i, "w_bf16 written outside [rows, cols]")
        if ld_wt is None:
            continue
        wt = ts.wt[i]
        assert torch.equal(_bits(wt[:cols, :rows]), _bits(pn.t().to(torch.bfloat16))), (i, "wt_bf16")
        assert torch.isnan(wt[cols:]).all() and torch.isnan(wt[:, rows:]).all(), (i, "wt_bf16 written outside [cols, rows]")


# ---------------------------------------------------------------------------------------------------------------- 3: the stated order
def _fold64(vals):
    s = 0.0
    for x in vals:
        s = s + x
    return s


def _tile_sum_in_kernel_order(t64):
    """The header's in-tile order on one [<= 64, <= 64] float64 tile (zero padded to 64 x 64: adding +0.0 to a sum of squares changes nothing): thread t owns rows
    (t >> 4) + 16 k and columns 4 (t & 15) .. + 3; k ascending, columns ascending; xor butterfly 32 .. 1 per wavefront; ((w0 + w1) + w2) + w3."""
    import numpy as np
    a = np.zeros((64, 64))
    a[:t64.shape[0], :t64.shape[1]] = t64.numpy()
    sq = a * a                                                       # exact: the inputs are fp32 values
    t = np.arange(256)
    acc = np.zeros(256)
    for k in range(4):
        for j in range(4):
            acc = acc + sq[(t >> 4) + 16 * k, 4 * (t & 15) + j]
    for msk in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[(t & ~63) | ((t & 63) ^ msk)]
    return float(((acc[0] + acc[64]) + acc[128]) + acc[192])


def test_workspace_holds_the_tile_sums_and_their_ascending_fold():
    gen = torch.Generator().manual_seed(3)
    p = [torch.randn(r, c, generator=gen) * 0.05 for r, c, _ in SET]
    g = [torch.randn(r, c, generator=gen) for r, c, _ in SET]
    ts = _Tensors(SET, p, [torch.zeros_like(t) for t in p], [torch.zeros_like(t) for t in p], g)
    assert ts.T == 1 + 2 + 2 + 16 + 25 + 1 + 8
    norm, ws = _step(ts, 1, 0.0, 0.5)
    part = ws[:ts.T].cpu().tolist()
    tiles = [gi.double()[r0:r0 + 64, c0:c0 + 64] for gi in g for r0 in range(0, gi.shape[0], 64) for c0 in range(0, gi.shape[1], 64)]   # descriptor order, row-major
    assert len(tiles) == ts.T
    for i, t64 in enumerate(tiles):
        exact = math.fsum((t64 * t64).reshape(-1).tolist())
        assert abs(part[i] - exact) <= 1e-15 * exact, (i, part[i], exact)
        assert part[i] == _tile_sum_in_kernel_order(t64), (i, "the in-tile order is not the documented one")
    S = ws[ts.T].item()
    assert S == _fold64(part)
    assert norm.item() == torch.tensor(math.sqrt(S), dtype=torch.float64).float().item()


# ---------------------------------------------------------------------------------------------------------------- 4: reproducible
def test_twenty_calls_give_the_same_bits_whatever_the_workspace_held_and_the_device_does():
    shapes = IMAGE_SET + [(69, 1, 8), (1, 69, 69)]
    inp = _image_inputs()
    gen = torch.Generator().manual_seed(4)
    inp = tuple(x + [torch.randn(69, 1, generator=gen) * 0.05, torch.randn(1, 69, generator=gen) * 0.05] for x in inp)
    inp[2][-2].abs_(); inp[2][-1].abs_()
    side = torch.cuda.Stream()
    a = torch.randn(4096, 4096, device="cuda")

    def kick():
        with torch.cuda.stream(side):
            for _ in range(4):
                a @ a

    first = None
    for i in range(20):
        ts = _Tensors(shapes, *inp)
        norm, ws = _step(ts, 7, 0.01, 0.05, fill=["nan", "ones", str(100 + i)][i % 3], kick=kick if i % 4 == 1 else None)
        out = [norm, ws] + ts.p + ts.m + ts.v + [t for t in ts.w + ts.wt if t is not None]
        if first is None:
            first = out
            assert torch.isfinite(norm).all() and norm.item() > 0.05                                      # clipping is active
            continue
        differing = [j for j, (x, y) in enumerate(zip(out, first)) if not torch.equal(_bits(x), _bits(y))]
        assert not differing, (i, differing)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- 5: NaN is not hidden
def test_a_nan_gradient_reaches_every_parameter_through_the_clip_and_only_its_own_element_without():
    gen = torch.Generator().manual_seed(5)
    p = [torch.randn(r, c, generator=gen) * 0.05 for r, c, _ in SET]
    z = [torch.zeros_like(t) for t in p]
    g = [torch.randn(r, c, generator=gen) for r, c, _ in SET]
    g[4][200, 17] = NAN
    ts = _Tensors(SET, p, z, z, g)
    norm, _ = _step(ts, 1, 0.0, 0.5)
    assert torch.isnan(norm).all()
    for x in ts.p + ts.m + ts.v:
        assert torch.isnan(x).all()
    ts = _Tensors(SET, p, z, z, g)
    norm, _ = _step(ts, 1, 0.0, 0.0)                                   # clipping off: the norm is still NaN, the parameters are touched where the NaN is
    assert torch.isnan(norm).all()
    for i, x in enumerate(ts.p):
        bad = torch.isnan(x)
        if i == 4:
            assert bad[200, 17] and bad.sum().item() == 1 and torch.isnan(ts.m[i][200, 17]) and torch.isnan(ts.v[i][200, 17])
        else:
            assert not bad.any()


# ---------------------------------------------------------------------------------------------------------------- 6: LibAdam against torch
def _dist(net, net64):
    return max((a.detach().double().cpu() - b.detach()).abs().max().item() for a, b in zip(net.parameters(), net64.parameters()))


def test_libadam_tracks_float64_adam_and_exchanges_state_with_torch():
    from smplsim_amd.learning.fused_optim import LibAdam
    from smplsim_amd.learning.networks import MLP, Value
    torch.manual_seed(11)
    lr, clip = 3e-4, 1.0
    net_a = Value(MLP(40, (256, 128), "silu")).cuda()
    net_b, net_r = copy.deepcopy(net_a), copy.deepcopy(net_a).cpu().double()
    opt_a = LibAdam(net_a.parameters(), lr=lr, max_grad_norm=clip)
    opt_b = torch.optim.Adam(net_b.parameters(), lr=lr, fused=True)
    opt_r = torch.optim.Adam(net_r.parameters(), lr=lr, foreach=False)
    gen = torch.Generator().manual_seed(12)
    shapes = [tuple(q.shape) for q in net_a.parameters()]
    default_keys = set(torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))]).state_dict()["param_groups"][0])

    def one_step(sides):
        """sides: [(net, opt, clips_itself)]; the same fixed random gradients for every side."""
        grads = [torch.randn(s, generator=gen) for s in shapes]
        for net, opt, own_clip in sides:
            for q, gr in zip(net.parameters(), grads):
                q.grad = gr.to(device=q.device, dtype=q.dtype).clone()
            if not own_clip:
                torch.nn.utils.clip_grad_norm_(net.parameters(), clip)
            opt.step()

    def check(tag, nets):
        torch.cuda.synchronize()
        d_b = _dist(net_b, net_r)
        ds = {k: _dist(n, net_r) for k, n in nets.items()}
        _record(tag, torch_fused=d_b, **ds)
        print(tag, d_b, ds)
        assert d_b > 0.0
        for k, d in ds.items():
            assert d <= FACTOR * d_b, (tag, k, d, d_b)

    base = [(net_a, opt_a, True), (net_b, opt_b, False), (net_r, opt_r, False)]
    for _ in range(5):
        one_step(base)
    check("libadam_5_steps", dict(lib=net_a))
    assert opt_a.last_grad_norm.is_cuda and math.isfinite(float(opt_a.last_grad_norm))
    st = opt_a.state[next(net_a.parameters())]
    assert st["step"].device.type == "cpu" and st["step"].dtype == torch.float32 and float(st["step"]) == 5.0
    sd = opt_a.state_dict()
    assert set(sd["param_groups"][0]) == default_keys and sd["param_groups"][0]["fused"] is None
    # LibAdam -> plain torch.optim.Adam
    net_c = copy.deepcopy(net_a)
    opt_c = torch.optim.Adam(net_c.parameters(), lr=lr)
    opt_c.load_state_dict(copy.deepcopy(sd))                            # (as through a checkpoint file: torch's load keeps the tensors it is given, and two live optimisers must not share moments)
    one_step(base + [(net_c, opt_c, False)])
    check("libadam_to_plain", dict(lib=net_a, plain=net_c))
    # ... and back
    net_d = copy.deepcopy(net_c)
    opt_d = LibAdam(net_d.parameters(), lr=lr, max_grad_norm=clip)
    opt_d.load_state_dict(copy.deepcopy(opt_c.state_dict()))
    assert float(opt_d.state[next(net_d.parameters())]["step"]) == 6.0
    one_step(base + [(net_c, opt_c, False), (net_d, opt_d, True)])
    check("plain_to_libadam", dict(lib=net_a, plain=net_c, back=net_d))
    # the way in from a fused=True state: a device-tensor step and fused=True in the saved group
    sd_b = opt_b.state_dict()
    assert sd_b["param_groups"][0]["fused"] is True and sd_b["state"][0]["step"].is_cuda
    net_e = copy.deepcopy(net_b)
    opt_e = LibAdam(net_e.parameters(), lr=lr, max_grad_norm=clip)
    opt_e.load_state_dict(copy.deepcopy(sd_b))
    st = opt_e.state[next(net_e.parameters())]
    assert st["step"].device.type == "cpu" and st["step"].dtype == torch.float32 and float(st["step"]) == 7.0
    sd_e = opt_e.state_dict()
    assert set(sd_e["param_groups"][0]) == default_keys and sd_e["param_groups"][0]["fused"] is None and sd_e["param_groups"][0]["foreach"] is None
    assert not sd_e["state"][0]["step"].is_cuda
    one_step(base + [(net_e, opt_e, True)])
    check("fused_to_libadam", dict(lib=net_a, from_fused=net_e))
    assert float(opt_e.state[next(net_e.parameters())]["step"]) == 8.0


# ---------------------------------------------------------------------------------------------------------------- 7: the agent
def _old_way_images(layer, i, nl):
    """The bf16 images of one layer as FusedMLPTrain's passes build them without weight_images: W cast into [n_out, kpad] (zero pad), W^T into [kpad, n_out (head: padded to 128)]."""
    w = layer.weight.detach()
    n_out, n_in = w.shape
    kpad = -(-n_in // 128) * 128 if i == 0 else -(-n_in // 64) * 64
    wb = torch.zeros(n_out, kpad, dtype=torch.bfloat16, device=w.device)
    wb[:, :n_in] = w
    if i == 0:
        return wb, None
    wt = torch.zeros(kpad, -(-n_out // 128) * 128 if i == nl - 1 else n_out, dtype=torch.bfloat16, device=w.device)
    wt[:, :n_out] = wb.t()
    return wb, wt


def test_agent_with_the_fused_optimizer():
    from smplsim_amd.agents.ppo import AgentPPO, PPOConfig
    from smplsim_amd.batch import SMPLSimVecEnv
    from smplsim_amd.learning.fused_optim import LibAdam
    from smplsim_amd.learning.fused_train import FusedMLPTrain
    env = SMPLSimVecEnv(256, task="HumanoidSpeed", autoreset=True, seed=3)
    cfg = dict(hidden=(512, 256, 256), mfma_update=True, deterministic_update=True, fused_loss=True, fused_optimizer=True, min_batch_size=4100, opt_num_epochs=2)
    a, b = AgentPPO(env, PPOConfig(**cfg), seed=1), AgentPPO(env, PPOConfig(**cfg), seed=1)
    other = AgentPPO(env, PPOConfig(**cfg), seed=2)
    assert type(a.optimizer_policy) is LibAdam and type(a.optimizer_value) is LibAdam
    assert a.optimizer_policy.max_grad_norm == 25.0 and a.optimizer_value.max_grad_norm is None
    x = torch.randn(256, a.state_dim, generator=torch.Generator().manual_seed(9)).cuda()
    infos = []
    for round_ in range(2):
        batch = a.sample()
        ia = a.update_params({k: v.clone() for k, v in batch.items()})
        b.update_params({k: v.clone() for k, v in batch.items()})
        torch.cuda.synchronize()
        infos.append(ia)
        # (b) same seed, same bits — the moments and the CPU step counters among them
        sa, sb = _agent_state(a), _agent_state(b)
        assert sa.keys() == sb.keys() and any(k.startswith("opt_policy.") and k.endswith("exp_avg_sq") for k in sa) and any(k.endswith(".step") for k in sa)
        differing = [k for k in sa if not _same_bits(sa[k], sb[k])]
        assert not differing, (round_, differing)
        # (a) every image is its layer's weight, cast and padded the old way; the pass over the images is the pass over fresh casts
        for net, hidden, head in ((a.fused_policy, a.policy_net.net.affine_layers, a.policy_net.action_mean), (a.fused_value, a.value_net.net.affine_layers, a.value_net.value_head)):
            imgs = net.images()
            assert len(imgs) == 4
            for i, (w, wb, wt) in enumerate(imgs):
                assert w._version == net.weight_images.versions[i]                                        # the step did not go through torch
                wb0, wt0 = _old_way_images(net.layers[i], i, len(imgs))
                assert wb.shape == wb0.shape and torch.equal(_bits(wb), _bits(wb0)), (round_, i, "W image")
                assert (wt is None) == (wt0 is None)
                if wt is not None:
                    assert wt.shape == wt0.shape and torch.equal(_bits(wt), _bits(wt0)), (round_, i, "W^T image")
            fresh = FusedMLPTrain(hidden, head, a.cfg.activation, deterministic=True, weight_images=False)
            with torch.no_grad():
                assert torch.equal(_bits(net(x)), _bits(fresh(x)))
        # (d)
        assert ia["grad_norm"].is_cuda and math.isfinite(float(ia["grad_norm"])) and float(ia["grad_norm"]) > 0.0
        assert math.isfinite(float(ia["surr_loss"])) and math.isfinite(float(ia["value_loss"]))
        _record(f"fused_optimizer_agent_round{round_}", grad_norm=float(ia["grad_norm"]), surr=float(ia["surr_loss"]), value=float(ia["value_loss"]))
    # checkpoints are plain Adam's: CPU step counters, no key beyond torch's defaults
    state = a.get_full_state_weights()
    default_keys = set(torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))]).state_dict()["param_groups"][0])
    for k in ("optimizer_policy", "optimizer_value"):
        assert set(state[k]["param_groups"][0]) == default_keys and not state[k]["param_groups"][0]["fused"]
        assert all(not s["step"].is_cuda for s in state[k]["state"].values())
    # (c) another agent takes this one's state through torch (load_state_dict writes the weights in place): the version counters notice, the images follow
    with torch.no_grad():
        assert not torch.equal(_bits(other.fused_policy(x)), _bits(a.fused_policy(x)))
    other.set_full_state_weights(copy.deepcopy(state))
    with torch.no_grad():
        assert torch.equal(_bits(other.fused_policy(x)), _bits(a.fused_policy(x))) and torch.equal(_bits(other.fused_value(x)), _bits(a.fused_value(x)))
    # ... and goes on exactly as this one does
    batch = a.sample()
    a.update_params({k: v.clone() for k, v in batch.items()})
    other.update_params({k: v.clone() for k, v in batch.items()})
    torch.cuda.synchronize()
    sa, so = _agent_state(a), _agent_state(other)
    differing = [k for k in sa if not _same_bits(sa[k], so[k])]
    assert not differing, differing
