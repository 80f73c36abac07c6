"""Every bf16 GEMM instantiation (csrc/ss_gemm128.h, csrc/ss_gemm256_kernels.h) the host dispatch of smplsim_mlp.hip can launch, against a float64 reference on the device computed from
the same bf16 operands, with an element-wise error bound derived from the arithmetic (not from max |ref|).  Each case asserts, through
ss_debug_last_gemm, that it reached the instantiation it is meant to cover; sentinels around every output check that nothing is written
outside the output's region; row strides that are not multiples of 8 and pointers offset by one element take the scalar epilogues.

Error model.  With bf16 operands (exact in fp32) and fp32 accumulation in an unknown order, the pre-activation z = x W^T (+ b) (* mul)
is within
    E = C_ACC * 2^-24 * (K * (|x| @ |w|^T) + |b|) * |mul|
of the exact value.  Outputs are then bounded element-wise by
    fp32:  F = L_act * E + 2^-20 |ref| + ACT_ABS      (the activation's own fp32 evaluation: __expf, v_rcp_f32 — a few ulp, plus an
                                                       absolute 2^-21 for the cancellation in tanh's / silu's (1 - e) near zero)
    bf16:  (1 + 2^-8) F + 2^-8 |ref|                   (round to nearest even: half an ulp of the fp32 value, at most 2^-8 of it)
    act':  |act''|max * E + 2^-8 |ref| + 2^-20         (relu: elements whose pre-activation lies within E of 0 are skipped)
C_ACC is the worst-case constant 1 scaled down to what was measured (see C_ACC below); the largest observed error / bound ratio of
every family is printed and recorded by `_record` when the suite runs (the bf16 families sit near 1 by construction: their bound is
dominated by the rounding term, which RNE reaches)."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

# Measured on the MI355X (one run of this file with C_ACC = 1, `measured gemm_ratio_acc_*` lines): the largest |err| / (K 2^-24 (|x| @ |w|^T))
# over the fp32 outputs was 8.8e-3 (ss_linear_bf16, fp32 head), 2.6e-3 (ss_wgrad_bf16), 4.2e-5 (the accumulating form); C_ACC is ~3.5x the largest.
C_ACC = 1.0 / 32
U = 2.0 ** -24
ACTS = ("silu", "tanh", "relu", "none")
ACT_ID = {"none": 0, "silu": 1, "tanh": 2, "relu": 3}
L_ACT = {"silu": 1.0998, "tanh": 1.0, "relu": 1.0, "none": 1.0}          # max |act'|
D2_ACT = {"silu": 0.5, "tanh": 0.7699, "relu": 0.0, "none": 0.0}         # max |act''|
ACT_ABS = {"silu": 2.0 ** -21, "tanh": 2.0 ** -21, "relu": 0.0, "none": 0.0}
SENT_BF16 = -768.0                                                       # exact in bf16: what every unwritten element must still hold
SENT_F32 = -12345.0

# The instantiations smplsim_mlp.hip launches (hand list: a new variant needs a row in DISPATCH_MAP below, or the map test fails).
# The string is ss_debug_last_gemm's description without its K-split fields.
INSTANTIATIONS = sorted(
    [f"linear mode=- bn={bn} bk={bk} waves={wv} out={o}" for bn in (64, 128) for bk, wv in ((64, 8), (32, 4)) for o in ("bf16", "f32")]
    + [f"glds mode=- bn={bn} bk=64 waves=8 out={o}" for bn in (64, 128, 192, 256) for o in ("bf16", "f32")]
    + [f"train mode=- bn={bn} bk=64 waves=8 out={o}" for bn in (64, 128, 192, 256) for o in ("bf16", "f32acc")]
    + [f"gemm256 mode={m} bn=256 bk=64 waves=8 out={'f32acc' if m == 'ACCUM' else 'bf16'}" for m in ("ACCUM", "PLAIN", "FWD", "DX", "FWDN", "DXN")]
    + ["wgrad mode=- bn=256 bk=64 waves=8 out=f32acc"])


def _lib():
    from smplsim_amd._lib import lib
    return lib()


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def last_gemm():
    buf = C.create_string_buffer(256)
    n = _lib().ss_debug_last_gemm(buf, 256)
    assert 0 <= n < 256
    return buf.value.decode()


def _key(desc):
    return desc.split(" ksplit=")[0]


def _record(name, **vals):
    from test_gpu_parity import _record as rec
    rec(name, **vals)


RATIOS = {}


def _note(family, ratio):
    RATIOS[family] = max(RATIOS.get(family, 0.0), float(ratio))
    _record("gemm_ratio_" + family, ratio=RATIOS[family])


def _operands(M, N, K, seed, scale=8.0):
    """x [M, K], w [N, K] bf16 with pre-activations up to |z| ~ 20 (tanh / silu saturate), asymmetric (a row / column swap cannot pass),
    an all-zero row of x and an all-zero row of w (pre-activation exactly the bias); bias [N] fp32."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g) + torch.linspace(-0.5, 1.0, K)[None, :]
    w = (torch.randn(N, K, generator=g) + torch.linspace(-0.3, 0.6, N)[:, None]) * (scale / K ** 0.5)
    x[min(3, M - 1)] = 0.0
    w[min(5, N - 1)] = 0.0
    b = torch.randn(N, generator=g) * 2.0
    return x.to(torch.bfloat16).cuda(), w.to(torch.bfloat16).cuda(), b.cuda()


def _act64(z, act):
    if act == "silu":
        return z * torch.sigmoid(z)
    if act == "tanh":
        return torch.tanh(z)
    if act == "relu":
        return torch.relu(z)
    return z


def _dact64(z, act):
    if act == "silu":
        s = torch.sigmoid(z)
        return s * (1 + z * (1 - s))
    if act == "tanh":
        return 1 - torch.tanh(z) ** 2
    if act == "relu":
        return (z > 0).double()
    return torch.ones_like(z)


class Ref:
    """The exact product of the bf16 operands (float64 on the device) and its bound E; bias / mul applied per call."""

    def __init__(self, x, w):
        self.xd, self.wd = x.double(), w.double()
        self.K = x.shape[1]
        self.z0 = self.xd @ self.wd.T
        self.a0 = self.xd.abs() @ self.wd.abs().T

    def pre(self, bias=None, mul=None):
        z = self.z0 + (0 if bias is None else bias.double()[None, :])
        e = C_ACC * U * (self.K * self.a0 + (0 if bias is None else bias.double().abs()[None, :]))
        if mul is not None:
            z = z * mul.double()
            e = e * mul.double().abs()
        return z, e


def check_out(got, z, e, act, bf16, family, what=""):
    """got (the written region, any dtype) against act(z) within the element-wise bound; returns the largest error / bound ratio."""
    ref = _act64(z, act)
    g = got.double()
    err = (g - ref).abs()
    bound = L_ACT[act] * e + 2.0 ** -20 * ref.abs() + ACT_ABS[act]
    if bf16:
        bound = (1 + 2.0 ** -8) * bound + 2.0 ** -8 * ref.abs()
    bad = ~(err <= bound)
    if bad.any():
        i = bad.nonzero()[0].tolist()
        raise AssertionError(f"{family}{what}: {int(bad.sum())} elements out of bound, first {i}: got {g[tuple(i)].item()!r} "
                             f"ref {ref[tuple(i)].item()!r} bound {bound[tuple(i)].item():.3g} (z {z[tuple(i)].item():.4g})")
    if not bf16:
        # the accumulation-order error alone, against the worst case K 2^-24 (|x| @ |w|^T) (what C_ACC is set from)
        lin = L_ACT[act] * e / C_ACC
        r = ((err - 2.0 ** -20 * ref.abs() - ACT_ABS[act]).clamp_min(0) / lin.clamp_min(1e-300)).max().item()
        _note("acc_" + family, r)
    r = (err / bound.clamp_min(1e-300)).max().item()
    _note(family, r)
    return r


def check_dact(got, z, e, act, family):
    ref = _dact64(z, act)
    err = (got.double() - ref).abs()
    bound = D2_ACT[act] * e + 2.0 ** -8 * ref.abs() + 2.0 ** -20
    keep = ~(z.abs() < e) if act == "relu" else torch.ones_like(err, dtype=torch.bool)
    bad = keep & ~(err <= bound)
    if bad.any():
        i = bad.nonzero()[0].tolist()
        raise AssertionError(f"{family} act': {int(bad.sum())} out of bound, first {i}: got {got[tuple(i)].item()!r} ref {ref[tuple(i)].item()!r}")
    _note(family + "_dact", (err / bound)[keep].max().item() if keep.any() else 0.0)


def out_buf(rows, cols, ld, dtype, offset):
    """A sentinel-filled [rows, ld] buffer (plus a margin) and the [rows, cols] view the kernel writes, `offset` elements into it."""
    sent = SENT_BF16 if dtype == torch.bfloat16 else SENT_F32
    flat = torch.full((rows * ld + offset + 64,), sent, dtype=dtype, device="cuda")
    full = flat[offset:offset + rows * ld].view(rows, ld)
    return flat, full


def check_untouched(flat, full, cols, offset):
    """Everything of `flat` outside columns 0 .. cols - 1 of the rows of `full` still holds the sentinel."""
    sent = SENT_BF16 if flat.dtype == torch.bfloat16 else SENT_F32
    mask = torch.ones_like(flat, dtype=torch.bool)
    mask[offset:offset + full.numel()].view(full.shape)[:, :cols] = False
    assert (flat[mask] == sent).all(), "a write outside the output's region"


def _lin(bn, bk, wv, out):
    return f"linear mode=- bn={bn} bk={bk} waves={wv} out={out} ksplit=1 kper=0"


def _glds(bn, out):
    return f"glds mode=- bn={bn} bk=64 waves=8 out={out} ksplit=1 kper=0"


def _train(bn, out="bf16", ks=1, kper=0):
    return f"train mode=- bn={bn} bk=64 waves=8 out={out} ksplit={ks} kper={kper}"


def _g256(mode, ks=1, kper=0):
    return f"gemm256 mode={mode} bn=256 bk=64 waves=8 out={'f32acc' if mode == 'ACCUM' else 'bf16'} ksplit={ks} kper={kper}"


# (entry point, arguments, expected ss_debug_last_gemm): one row per instantiation.  linear: (M, N, K, fp32 out); train: (M, N, K, outputs, accumulate)
# with outputs a subset of "y", "yt", "d" (dact), "m" (mul); dx: (M, N, K); wgrad: (Mb, n_out, n_in)
DISPATCH_MAP = [
    ("linear", (100, 64, 512, 0), _glds(64, "bf16")), ("linear", (100, 64, 512, 1), _glds(64, "f32")),
    ("linear", (4096, 520, 512, 0), _glds(128, "bf16")), ("linear", (4096, 520, 512, 1), _glds(128, "f32")),
    ("linear", (8191, 520, 512, 0), _glds(192, "bf16")), ("linear", (8191, 520, 512, 1), _glds(192, "f32")),
    ("linear", (8191, 1000, 512, 0), _glds(256, "bf16")), ("linear", (8191, 1000, 512, 1), _glds(256, "f32")),
    ("linear", (100, 64, 320, 0), _lin(64, 64, 8, "bf16")), ("linear", (100, 64, 320, 1), _lin(64, 64, 8, "f32")),
    ("linear", (4096, 520, 320, 0), _lin(128, 64, 8, "bf16")), ("linear", (4096, 520, 320, 1), _lin(128, 64, 8, "f32")),
    ("linear", (100, 64, 96, 0), _lin(64, 32, 4, "bf16")), ("linear", (100, 64, 96, 1), _lin(64, 32, 4, "f32")),
    ("linear", (4096, 520, 96, 0), _lin(128, 32, 4, "bf16")), ("linear", (4096, 520, 96, 1), _lin(128, 32, 4, "f32")),
    ("linear", (16000, 1024, 512, 0), _g256("PLAIN")),
    ("train", (100, 64, 64, "y", 0), _train(64)), ("train", (2000, 1536, 64, "y", 0), _train(128)),
    ("train", (8192, 576, 576, "y", 0), _train(192)), ("train", (8192, 1536, 576, "y", 0), _train(256)),
    ("train", (128, 64, 512, "y", 1), _train(64, "f32acc", 1, 8)), ("train", (128, 128, 5184, "y", 1), _train(128, "f32acc", 10, 9)),
    ("train", (128, 192, 512, "y", 1), _train(192, "f32acc", 1, 8)), ("train", (128, 256, 512, "y", 1), _train(256, "f32acc", 1, 8)),
    ("train", (256, 256, 8192, "y", 1), _g256("ACCUM", 16, 8)), ("train", (2049, 512, 128, "y", 0), _g256("PLAIN")),
    ("train", (4100, 1000, 640, "y yt d", 0), _g256("FWD")), ("train", (4100, 1000, 640, "y m yt", 0), _g256("DX")),
    ("train", (4096, 256, 128, "y d", 0), _g256("FWDN")), ("train", (2048, 300, 384, "y m", 0), _g256("DXN")),
    ("dx", (2049, 300, 384), _g256("DXN")),
    ("wgrad", (128, 72, 136), "wgrad mode=- bn=256 bk=64 waves=8 out=f32acc ksplit=1 kper=2"),
    ("wgrad", (3200, 72, 136), "wgrad mode=- bn=256 bk=64 waves=8 out=f32acc ksplit=5 kper=10"),     # 6 shares of 9 tiles -> 5 of 10
]


def _launch_zero(entry, args):
    """One launch of `entry` on zero-filled operands; returns the status."""
    z = lambda *s, dt=torch.bfloat16: torch.zeros(*s, dtype=dt, device="cuda")
    L, st = _lib(), _st()
    if entry == "linear":
        M, N, K, f32 = args
        return L.ss_linear_bf16(_p(z(M, K)), _p(z(N, K)), None, _p(z(M, N, dt=torch.float32 if f32 else torch.bfloat16)), M, N, K, N, 0, f32, st)
    if entry == "train":
        M, N, K, outs, acc = args
        outs = outs.split()
        y = z(M, N, dt=torch.float32 if acc else torch.bfloat16) if "y" in outs else None
        return L.ss_linear_bf16_train(_p(z(M, K)), _p(z(N, K)), None, _p(z(M, N) if "m" in outs else None), _p(y), _p(z(N, M) if "yt" in outs else None),
                                      _p(z(M, N) if "d" in outs else None), M, N, K, N, M, 0, acc, st)
    if entry == "dx":
        M, N, K = args
        return L.ss_linear_bf16_dx(_p(z(M, K)), _p(z(N, K)), _p(z(M, N)), _p(z(M, N)), _p(z(N, dt=torch.float32)), M, N, K, N, st)
    Mb, no, ni = args
    return L.ss_wgrad_bf16(_p(z(Mb, no)), _p(z(Mb, ni)), _p(z(no, ni, dt=torch.float32)), Mb, no, ni, no, ni, ni, st)


def test_dispatch_map_covers_every_instantiation():
    """Each row of DISPATCH_MAP reaches the instantiation it names (ss_debug_last_gemm, the host thread's last launch), and the rows together
    reach every instantiation of the hand-written list — a new kernel variant without a row here fails this test."""
    assert sorted({_key(e) for _, _, e in DISPATCH_MAP}) == INSTANTIATIONS
    for entry, args, expect in DISPATCH_MAP:
        assert _launch_zero(entry, args) == 0, (entry, args)
        assert last_gemm() == expect, (entry, args)
    torch.cuda.synchronize()
    assert _lib().ss_debug_last_gemm(None, 0) == -1


# ---------------------------------------------------------------------------------------------------------------- ss_linear_bf16
# (M, N, K, expected bf16-out description, expected fp32-out description): every instantiation in both output types, ragged M at 128 +- 1 and
# 256 +- 1, the two head widths 69 and 1
LINEAR_CASES = [
    ((100, 64, 512), _glds(64, "bf16"), _glds(64, "f32")),
    ((129, 69, 512), _glds(64, "bf16"), _glds(64, "f32")),
    ((255, 1, 512), _glds(64, "bf16"), _glds(64, "f32")),
    ((4096, 520, 512), _glds(128, "bf16"), _glds(128, "f32")),
    ((8191, 520, 512), _glds(192, "bf16"), _glds(192, "f32")),
    ((8191, 1000, 512), _glds(256, "bf16"), _glds(256, "f32")),
    ((100, 64, 320), _lin(64, 64, 8, "bf16"), _lin(64, 64, 8, "f32")),
    ((257, 69, 320), _lin(64, 64, 8, "bf16"), _lin(64, 64, 8, "f32")),
    ((4096, 520, 320), _lin(128, 64, 8, "bf16"), _lin(128, 64, 8, "f32")),
    ((100, 64, 96), _lin(64, 32, 4, "bf16"), _lin(64, 32, 4, "f32")),
    ((127, 1, 96), _lin(64, 32, 4, "bf16"), _lin(64, 32, 4, "f32")),
    ((4096, 520, 96), _lin(128, 32, 4, "bf16"), _lin(128, 32, 4, "f32")),
    ((16000, 1024, 512), _g256("PLAIN"), _glds(256, "f32")),
]


@pytest.mark.parametrize("case", range(len(LINEAR_CASES)))
def test_linear_bf16_every_instantiation(case):
    """ss_linear_bf16 in both output types: the vector epilogue (ldy a multiple of 8, aligned, a bias) and the scalar one (ldy = N + 3 or + 1,
    the output one element off its alignment, no bias), sentinels around the output, every activation, two launches bit-identical (bf16)."""
    (M, N, K), want16, want32 = LINEAR_CASES[case]
    x, w, b = _operands(M, N, K, seed=case)
    ref = Ref(x, w)
    L, st = _lib(), _st()
    for vi, scalar in enumerate((False, True)):
        bias = None if scalar else b
        z, e = ref.pre(bias)
        for f32 in (0, 1):
            act = ACTS[(case + 2 * vi + f32) % 4]
            dt = torch.float32 if f32 else torch.bfloat16
            ld = (N + 3 if (N + 3) % 8 else N + 1) if scalar else (N + 7) // 8 * 8 + 8
            off = 1 if scalar else 0
            outs = []
            for rep in range(1 if f32 else 2):
                flat, full = out_buf(M, N, ld, dt, off)
                assert L.ss_linear_bf16(_p(x), _p(w), _p(bias), _p(full), M, N, K, ld, ACT_ID[act], f32, st) == 0
                assert last_gemm() == (want32 if f32 else want16)
                torch.cuda.synchronize()
                check_untouched(flat, full, N, off)
                outs.append(full[:, :N].clone())
            if not f32:
                assert torch.equal(outs[0], outs[1])
            check_out(outs[0], z, e, act, not f32, "linear_f32" if f32 else "linear_bf16", f" {want32 if f32 else want16} {act} scalar={scalar}")


@pytest.mark.parametrize("f32", [0, 1])
def test_linear_bf16_nan_row_stays_in_its_row(f32):
    """A NaN in one row of x reaches that output row only; the other rows are bit-identical to the launch without it."""
    M, N, K = 300, 200, 512
    x, w, b = _operands(M, N, K, seed=77)
    L, st = _lib(), _st()
    dt = torch.float32 if f32 else torch.bfloat16
    y0 = torch.zeros(M, N, dtype=dt, device="cuda"); y1 = torch.zeros_like(y0)
    assert L.ss_linear_bf16(_p(x), _p(w), _p(b), _p(y0), M, N, K, N, ACT_ID["silu"], f32, st) == 0
    xn = x.clone(); xn[130, 17] = float("nan")
    assert L.ss_linear_bf16(_p(xn), _p(w), _p(b), _p(y1), M, N, K, N, ACT_ID["silu"], f32, st) == 0
    torch.cuda.synchronize()
    assert torch.isnan(y1[130]).all()
    keep = torch.ones(M, dtype=torch.bool, device="cuda"); keep[130] = False
    assert torch.equal(y0[keep], y1[keep])


# ---------------------------------------------------------------------------------------------------------------- ss_linear_bf16_train, bf16 form
def _odd_ld(n):
    return n + 3 if (n + 3) % 8 else n + 1


def _run_train(x, w, b, ref, outs, act, scalar, want, family, seed=0):
    """One ss_linear_bf16_train call (bf16 form) over the outputs `outs` (subset of y, yt, d, m), launched twice: each output against the f64
    reference, sentinels around every output, the two launches bit-identical.  scalar: ldy / ldyt not multiples of 8, y / yt / dact one element
    off their alignment."""
    M, K = x.shape
    N = w.shape[0]
    L, st = _lib(), _st()
    ldy = _odd_ld(N) if scalar else (N + 7) // 8 * 8 + 8
    ldt = _odd_ld(M) if scalar else (M + 7) // 8 * 8 + 8
    off = 1 if scalar else 0
    mul = None
    if "m" in outs:
        g = torch.Generator().manual_seed(seed + 1)
        mulbuf = torch.full((M, ldy), float("nan"), dtype=torch.bfloat16)           # what lies beyond column N must not reach the result
        mulbuf[:, :N] = torch.rand(M, N, generator=g) * 1.5 + 0.25
        mulbuf[min(7, M - 1), :N] = 0.0
        mulbuf = mulbuf.cuda()
        mul = mulbuf[:, :N]
    z, e = ref.pre(b, mul)
    got = []
    for rep in range(2):
        bufs = {k: out_buf(M, N, ldy, torch.bfloat16, off) for k in ("y", "d") if k in outs}
        if "yt" in outs:
            bufs["yt"] = out_buf(N, M, ldt, torch.bfloat16, off)
        ptr = lambda k: _p(bufs[k][1]) if k in bufs else None
        assert L.ss_linear_bf16_train(_p(x), _p(w), _p(b), _p(mulbuf) if mul is not None else None, ptr("y"), ptr("yt"), ptr("d"), M, N, K, ldy, ldt,
                                      ACT_ID[act], 0, st) == 0, L.ss_last_error()
        assert last_gemm() == want, (outs, scalar)
        torch.cuda.synchronize()
        for k, (flat, full) in bufs.items():
            check_untouched(flat, full, M if k == "yt" else N, off)
        got.append({k: full[:, :(M if k == "yt" else N)].clone() for k, (flat, full) in bufs.items()})
    for k in got[0]:
        assert torch.equal(got[0][k], got[1][k]), k
    o = got[0]
    if "y" in o:
        check_out(o["y"], z, e, act, True, family, f" {want} {outs} {act}")
        if "yt" in o:
            assert torch.equal(o["yt"], o["y"].t())                     # the transposed image is the same rounding of the same numbers
    elif "yt" in o:
        check_out(o["yt"].t(), z, e, act, True, family, f" {want} yt-only {act}")
    if "d" in o:
        check_dact(o["d"], z, e, act, family)


SUBSETS = ("y", "y d", "y yt", "yt", "y m", "y m yt d")


@pytest.mark.parametrize("shape,bn", [((100, 64, 64), 64), ((2000, 1536, 64), 128), ((8192, 576, 576), 192), ((8192, 1536, 576), 256)])
def test_linear_bf16_train_128_row_kernel_every_output_subset(shape, bn):
    """The 128-row training kernel at each tile width over every output subset, with and without a bias, all four activations, the vector and
    the scalar epilogues."""
    M, N, K = shape
    x, w, b = _operands(M, N, K, seed=M + N + K)
    ref = Ref(x, w)
    for j, outs in enumerate(SUBSETS):
        _run_train(x, w, b if j % 3 != 1 else None, ref, outs.split(), ACTS[(bn // 64 + j) % 4], j % 2 == 1, _train(bn), "train_bf16", seed=j)


@pytest.mark.parametrize("mode,shape,outs,scalar", [
    ("FWDN", (4096, 256, 128), "y d", False), ("FWD", (4100, 1000, 640), "y yt d", True), ("DX", (4100, 1000, 640), "y m yt", False),
    ("DXN", (2048, 300, 384), "y m", True), ("PLAIN", (2049, 512, 128), "y", True)])
def test_gemm256_modes_at_natural_shapes(mode, shape, outs, scalar):
    """The 256 x 256 kernel's bf16 modes as the dispatch picks them: ragged M (256 k + 4, 256 k + 1) and N (not a multiple
    of the tile, N = 300 not a multiple of 8), vector and edge stores, a bias, two launches bit-identical."""
    M, N, K = shape
    x, w, b = _operands(M, N, K, seed=M + 3 * N + K)
    ref = Ref(x, w)
    act = {"FWDN": "silu", "FWD": "tanh", "DX": "none", "DXN": "none", "PLAIN": "relu"}[mode]
    _run_train(x, w, b, ref, outs.split(), act, scalar, _g256(mode), "gemm256_bf16", seed=M)


# ---------------------------------------------------------------------------------------------------------------- accumulating fp32 form
@pytest.mark.parametrize("shape,want", [((128, 128, 5184), _train(128, "f32acc", 10, 9)), ((300, 576, 8192), _g256("ACCUM", 16, 8))])
def test_accumulating_form_adds_the_bias_once_and_accumulates(shape, want):
    """y += x W^T + b with the K split over workgroups: (128, 128, 5184) cuts 81 K tiles into 10 shares of 9, the last one EMPTY; the bias is added
    by one share only; a second call doubles the result; ldy = N + 3, sentinels beyond column N."""
    M, N, K = shape
    x, w, b = _operands(M, N, K, seed=K)
    ref = Ref(x, w)
    L, st = _lib(), _st()
    ld = N + 3
    flat, full = out_buf(M, N, ld, torch.float32, 0)
    full[:, :N] = 0.0
    z, e = ref.pre(b)
    for rep in (1, 2):
        assert L.ss_linear_bf16_train(_p(x), _p(w), _p(b), None, _p(full), None, None, M, N, K, ld, 0, 0, 1, st) == 0
        assert last_gemm() == want
        torch.cuda.synchronize()
        check_untouched(flat, full, N, 0)
        # (a bias added by every share instead of share 0 alone fails here: 10 b)
        check_out(full[:, :N] / rep, z, e, "none", False, "accum", f" {want} call {rep}")
    ks, kper = int(want.split("ksplit=")[1].split()[0]), int(want.split("kper=")[1])
    if shape == (128, 128, 5184):
        assert (ks - 1) * kper >= K // 64                              # the case it stands for: a trailing share with no K tiles


# ---------------------------------------------------------------------------------------------------------------- ss_linear_bf16_dx
def test_linear_bf16_dx_ragged_and_column_sums():
    """ss_linear_bf16_dx on N = 300 (not a multiple of 8, ldy = 304) and M = 2049: y = (x W^T) * mul within its bound, the padding of y untouched,
    NaN in the padding of mul kept out, and colsum = (its prior contents) + the f64 column sums over rows < M only."""
    M, N, K, ldy = 2049, 300, 384, 304
    x, w, _ = _operands(M, N, K, seed=5)
    ref = Ref(x, w)
    L, st = _lib(), _st()
    g = torch.Generator().manual_seed(6)
    mulbuf = torch.full((M, ldy), float("nan"), dtype=torch.bfloat16)
    mulbuf[:, :N] = torch.rand(M, N, generator=g) + 0.5
    mulbuf = mulbuf.cuda()
    z, e = ref.pre(None, mulbuf[:, :N])
    prior = (torch.randn(N, generator=g) * 10).cuda()
    flat, full = out_buf(M, N, ldy, torch.bfloat16, 0)
    cs = prior.clone()
    assert L.ss_linear_bf16_dx(_p(x), _p(w), _p(mulbuf), _p(full), _p(cs), M, N, K, ldy, st) == 0
    assert last_gemm() == _g256("DXN")
    torch.cuda.synchronize()
    check_untouched(flat, full, N, 0)
    check_out(full[:, :N], z, e, "none", True, "dx_bf16")
    # the column sums: each row's error E, plus fp32 additions of depth 64 (a lane's rows) + 1 (its partner) + one atomic per 128 rows
    depth = 64 + 1 + (M + 127) // 128
    csr = prior.double() + z.sum(0)
    bound = e.sum(0) + depth * U * (z.abs().sum(0) + prior.double().abs())
    err = (cs.double() - csr).abs()
    assert (err <= bound).all(), (err / bound).max().item()
    _note("dx_colsum", (err / bound).max().item())


# ---------------------------------------------------------------------------------------------------------------- ss_wgrad_bf16
@pytest.mark.parametrize("Mb,n_out,n_in,ldz,ldh,ldw,want", [
    (128, 72, 136, 80, 144, 139, (1, 2)),            # one share of two K tiles
    (3200, 72, 136, 80, 144, 139, (5, 10)),          # 6 shares of 9 tiles, rounded to even counts: 5 shares of 10
    (256, 8, 8, 16, 16, 13, (1, 4))])                # the narrowest operands, ldw > n_in
def test_wgrad_bf16_shares_strides_and_poisoned_padding(Mb, n_out, n_in, ldz, ldh, ldw, want):
    """dW += dZ^T h: against the f64 product of the used columns; the columns of dZ / h beyond n_out / n_in hold NaN and Inf and none may reach
    dW; dW accumulates onto its prior contents; its padding columns keep their sentinel."""
    g = torch.Generator().manual_seed(Mb + n_out)
    dz = torch.randn(Mb, ldz, generator=g) + torch.linspace(-1, 1, ldz)[None, :] * 0.3
    h = torch.randn(Mb, ldh, generator=g) + torch.linspace(1, -1, Mb)[:, None] * 0.3
    dz[:, n_out:] = float("nan"); dz[::2, n_out:] = float("inf")
    h[:, n_in:] = float("-inf"); h[1::3, n_in:] = float("nan")
    dz, h = dz.to(torch.bfloat16).cuda(), h.to(torch.bfloat16).cuda()
    L, st = _lib(), _st()
    flat, full = out_buf(n_out, n_in, ldw, torch.float32, 0)
    prior = torch.randn(n_out, n_in, generator=g).cuda()
    full[:, :n_in] = prior
    assert L.ss_wgrad_bf16(_p(dz), _p(h), _p(full), Mb, n_out, n_in, ldz, ldh, ldw, st) == 0
    assert last_gemm() == f"wgrad mode=- bn=256 bk=64 waves=8 out=f32acc ksplit={want[0]} kper={want[1]}"
    torch.cuda.synchronize()
    check_untouched(flat, full, n_in, 0)
    a, hh = dz[:, :n_out].double(), h[:, :n_in].double()
    z = prior.double() + a.T @ hh
    e = C_ACC * U * (Mb * (a.abs().T @ hh.abs()) + prior.double().abs())
    check_out(full[:, :n_in], z, e, "none", False, "wgrad")


# ---------------------------------------------------------------------------------------------------------------- ss_obs_to_bf16
def _bits(t):
    return t.view(torch.int16)


def test_obs_to_bf16_rounding_normalisation_and_padding():
    """Without normalisation the conversion is bit-for-bit torch.clamp(...).to(bfloat16) (ties to even, values at bf16's overflow point); with it,
    within one bf16 ulp of the fp32 expression; NaN stays NaN; columns dim .. kpad are zero; norm_n = 0 skips the normalisation."""
    M, dim, stride, kpad = 37, 45, 50, 64
    g = torch.Generator().manual_seed(9)
    obs = torch.randn(M, stride, generator=g) * 4
    one = 1.0 + 2.0 ** -8                                           # halfway between 1 and 1 + 2^-7: ties to even -> 1
    specials = [one, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), 3.3895313892515355e38, 3.3961775292304e38, 3.4028234663852886e38, -3.4e38,
                0.0, -0.0, 6.0, -6.0]                               # (bf16's largest value, the tie above it, fp32's largest: both round to inf)
    obs[0, :len(specials)] = torch.tensor(specials)
    obs[2, 4] = float("nan")
    obs = obs.cuda()
    L, st = _lib(), _st()
    nan_mask = torch.zeros(M, dim, dtype=torch.bool, device="cuda"); nan_mask[2, 4] = True

    def run(lo, hi, mean=None, sd=None, n=None, clip=5.0):
        out = torch.full((M, kpad), SENT_BF16, dtype=torch.bfloat16, device="cuda")
        assert L.ss_obs_to_bf16(_p(obs), M, dim, stride, _p(mean), _p(sd), _p(n), lo, hi, clip, _p(out), kpad, st) == 0
        torch.cuda.synchronize()
        assert (_bits(out[:, dim:]) == 0).all()                     # the padding: +0.0
        assert torch.isnan(out[:, :dim][nan_mask]).all()
        return out[:, :dim]

    o = obs[:, :dim]
    for lo, hi in ((-3.4028234663852886e38, 3.4028234663852886e38), (-5.0, 5.0)):
        got = run(lo, hi)
        want = torch.clamp(o, lo, hi).to(torch.bfloat16)
        assert torch.equal(_bits(got)[~nan_mask], _bits(want)[~nan_mask]), (lo, hi)
    assert run(-1e30, 1e30)[0, 0].item() == 1.0 and run(-1e30, 1e30)[0, 1].item() == 1.0 + 2.0 ** -6
    mean = (torch.randn(dim, generator=g) * 0.5).cuda()
    sd = (torch.rand(dim, generator=g) + 0.5).cuda()
    n0 = torch.zeros(1, dtype=torch.int64, device="cuda")
    assert torch.equal(_bits(run(-5.0, 5.0, mean, sd, n0)), _bits(run(-5.0, 5.0)))   # n = 0: no statistics yet, no normalisation
    n = torch.full((1,), 7, dtype=torch.int64, device="cuda")
    got = run(-5.0, 5.0, mean, sd, n, clip=3.0).float()
    want = torch.clamp((torch.clamp(o, -5.0, 5.0) - mean) / (sd + 1e-8), -3.0, 3.0)
    ok = ~nan_mask
    ulp = 2.0 ** (torch.floor(torch.log2(want.abs().clamp_min(2.0 ** -126))) - 7)
    assert ((got - want).abs()[ok] <= ulp[ok]).all()


# ---------------------------------------------------------------------------------------------------------------- the fused update at production width
# Measured on the MI355X (one run, `measured fused_update_*`): output 6.2e-3 and weight gradients 1.2e-2 (relative norm, worst: the 1-wide
# head); bias gradients 1.4e-4 by norm and 1.4e-2 element-wise, against the sum of the magnitudes of their terms.  Bounds ~2.5-3.5x those,
# none looser than 3e-2.
FUSED_REL = 3e-2
FUSED_BIAS_REL = 5e-4
FUSED_BIAS = 3e-2


@pytest.mark.parametrize("out_dim", [69, 1])
def test_fused_update_at_production_width_against_fp64_autograd(out_dim):
    """FusedMLPTrain at the production widths (289 -> 2048 -> 1536 -> 1024 -> 1024 -> 512 -> 512 -> head), M = 4100 (Mp = 4224: FWDN forward
    layers, DXN with column sums, the weight-gradient kernel) against fp64 autograd over the SAME bf16-rounded weights and inputs: the output
    and every parameter gradient by relative norm, the bias gradients element by element."""
    from smplsim_amd.agents.ppo import PPOConfig
    from smplsim_amd.learning.fused_train import FusedMLPTrain
    from smplsim_amd.learning.networks import MLP
    hidden = PPOConfig().hidden
    assert hidden == (2048, 1536, 1024, 1024, 512, 512)
    M = 4100
    torch.manual_seed(out_dim)
    net = MLP(289, hidden, "silu").cuda()
    head = torch.nn.Linear(hidden[-1], out_dim).cuda()
    layers = list(net.affine_layers) + [head]
    with torch.no_grad():
        for l in layers:
            l.weight.copy_(l.weight.to(torch.bfloat16).float())      # the operands the kernels see
    x = (torch.randn(M, 289, device="cuda") * 2).to(torch.bfloat16).float()
    target = torch.randn(M, out_dim, device="cuda").to(torch.bfloat16).float()   # dL/dy: bf16-exact (the head's dZ)
    params = [p for l in layers for p in (l.weight, l.bias)]
    fused = FusedMLPTrain(net.affine_layers, head, "silu")
    y = fused(x)
    g = torch.autograd.grad((y * target).sum(), params)
    p64 = [p.detach().double().requires_grad_(True) for p in params]
    h, zs = x.double(), []
    for i in range(len(layers)):
        z = h @ p64[2 * i].T + p64[2 * i + 1]
        z.retain_grad()
        zs.append(z)
        h = torch.nn.functional.silu(z) if i < len(layers) - 1 else z
    y64 = h
    (y64 * target.double()).sum().backward()
    g64 = [p.grad for p in p64]
    rel_y = ((y.double() - y64).norm() / y64.norm()).item()
    # a bias gradient is a sum over the batch of terms of both signs: its error is measured against the sum of their magnitudes (the terms carry
    # the bf16 rounding of every activation below them, which a cancelling sum does not average away); the weight gradients by their own norm
    scale = {2 * i + 1: zs[i].grad.abs().sum(0) for i in range(len(layers))}
    rels = [((a.double() - b).norm() / (scale[i] if i in scale else b).norm()).item() for i, (a, b) in enumerate(zip(g, g64))]
    bias_r = [((g[i].double() - g64[i]).abs() / scale[i]).max().item() for i in sorted(scale)]
    _record(f"fused_update_{out_dim}", rel_y=rel_y, rel_grads=rels, bias_elem=bias_r)
    assert rel_y < FUSED_REL, rel_y
    for i, r in enumerate(rels):
        assert r < (FUSED_BIAS_REL if i in scale else FUSED_REL), (i, tuple(params[i].shape), r)
    assert max(bias_r) < FUSED_BIAS, bias_r
