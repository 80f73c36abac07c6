"""The PPO update's network passes on this library's own matrix-core GEMMs (include/smplsim_mlp.h: ss_linear_bf16_train, ss_wgrad_bf16).

What it replaces: autograd over torch.nn.Linear + activation under bf16 autocast (hipBLASLt GEMMs plus separate bias, activation,
cast and transpose launches) in the reference's update_policy / update_value (agents/agent_ppo.py:20-83).  The loss, the optimiser
and the gradient clipping are not here (learning/fused_loss.py and learning/fused_optim.py have them; learning/fused_norm.py has the RunningNorm in front of the
policy, which hands its result over as a Bf16Operand); only `y = head(MLP(x))` and its backward are:

  forward, per hidden layer   h = act(z), g = act'(z)   with z = h_below W^T + b     ONE launch: the result and the activation's derivative from one tile
  head                        y = h W^T + b in fp32 (the inference kernel: the action mean must not be rounded to bf16)
  backward, per layer         dW = dZ^T h_below     -> ss_wgrad_bf16: both operands as they lie ([batch, features] row-major), contraction over their ROWS
                                                      (fragments by ds_read_b64_tr_b16), split along the batch, fp32 partial sums by hardware atomics
                              dZ_below = (dZ W) * g_below   -> ss_linear_bf16_dx on (dZ, W^T): the multiply in its epilogue, and the column sums of
                                                               the fp32 result = db of the layer below from the same launch

No transposed copies of activations or gradients exist: the forward and dX products are bound by the bytes they WRITE (profiles/r06_gemm256.txt: 2.1 TB/s), and
the first version of this file wrote h^T and dZ^T next to h and dZ so that the weight gradient could be the K-contiguous `x W^T` kernel — 1.35 of the 3.4 GB a
pass wrote.  bf16 operands, fp32 accumulation: the precision class of the autocast path it replaces (weights, activations and gradients of activations rounded
to bf16; weight gradients and the head's output fp32).  No CPU path: the package has none.

deterministic=True: the default backward pass is not reproducible from run to run — the batch split of every weight gradient and the per-wave column sums
meet in their outputs by fp32 atomics, in the order the workgroups finish.  The deterministic pass calls ss_wgrad_bf16_det / ss_linear_bf16_dx_det instead:
the same products, their partial sums stored into one workspace (the largest request of the pass, ~67 MB at the production widths) and added in a fixed order
by a second launch, each reduce finishing in stream order before the next product writes its partials.
"""
import torch

from .. import _cabi
from .._lib import lib
from ..batch import _check, _launch_stream, _ptr


def _pad(n, m):
    return (n + m - 1) // m * m


def _linear_train(x, w, bias, mul, y, yt, dact, M, N, K, ldy, ldyt, act, accumulate, stream):
    _check(lib().ss_linear_bf16_train(_ptr(x), _ptr(w), _ptr(bias), _ptr(mul), _ptr(y), _ptr(yt), _ptr(dact), M, N, K, ldy, ldyt, act, int(accumulate), stream))


class _Buffers:
    """Work tensors of one FusedMLPTrain, kept between calls (a pass allocated and zero-filled ~1 GB of activations and transposes: allocator
    round trips and memsets of tensors the kernels overwrite completely).  A forward pass that starts while the previous pass's backward has not run
    (two graphs alive) gets fresh tensors instead."""

    def __init__(self):
        self.t = {}
        self.busy = False

    def get(self, key, shape, dtype, device, fresh, init=None):
        if fresh:
            t = torch.zeros(shape, dtype=dtype, device=device)
            if init is not None:
                init(t)
            return t
        k = (key, tuple(shape), dtype)
        t = self.t.get(k)
        if t is None:
            t = self.t[k] = torch.zeros(shape, dtype=dtype, device=device)
            if init is not None:
                init(t)
        return t


class Bf16Operand:
    """The first layer's operand of a FusedMLPTrain pass, made by the caller: t [pad(M, 128), pad(D, 128)] bf16, contiguous, rows >= M and columns >= D zero —
    what the pass builds from an fp32 [M, D] input by `t[:M, :D] = x`.  The pass reads it in its forward AND in its backward (the first layer's weight gradient)
    and never writes it: it must stay unchanged until that pass's backward has run (in stream order), or for good if no backward follows."""
    __slots__ = ("t", "M", "D")

    def __init__(self, t, M, D):
        self.t, self.M, self.D = t, int(M), int(D)


class _FusedMLP(torch.autograd.Function):
    """y = Linear_{L+1}(act(Linear_L(... act(Linear_1(x))))) with x [M, D] fp32 or a Bf16Operand; params = W_1, b_1, ..., W_{L+1}, b_{L+1} (fp32, torch.nn.Linear layout)."""

    @staticmethod
    def forward(ctx, x, act, bufs, track, det, images, *params):
        given = x if isinstance(x, Bf16Operand) else None          # (checked by FusedMLPTrain.__call__)
        dev = given.t.device if given is not None else x.device
        st = _launch_stream(dev)
        ws, bs = params[0::2], params[1::2]
        nl = len(ws)
        M, D = (given.M, given.D) if given is not None else x.shape
        Mp = _pad(M, 128)                                          # the batch is the K of the weight-gradient products; its pad rows are zero in every
                                                                   # dZ (zero rows of the head's gradient stay zero through (dZ W) * g), so what the
                                                                   # forward pass leaves in the pad rows of h (act(bias)) never reaches a gradient
        kpad = [_pad(w.shape[1], 128) if i == 0 else _pad(w.shape[1], 64) for i, w in enumerate(ws)]   # a layer's input width as a K (the first: a whole number of K-tile pairs for the 256-tile kernel)
        fresh = track and bufs.busy                                # (track: a backward pass will follow and release the tensors)
        if track and not fresh:
            bufs.busy = True
        ctx.bufs = bufs if track and not fresh else None
        bf = torch.bfloat16
        if given is not None:
            h = given.t                                            # read here and by the backward pass's first weight gradient; never written
        else:
            h = bufs.get("x", (Mp, kpad[0]), bf, dev, fresh)       # (pad rows and columns stay zero: only [:M, :D] is ever written)
            h[:M, :D] = x
        hs, gs, wbs = [h], [], []
        # the layers' weights in bf16, all by one multi-tensor copy (they change with every optimiser step; 7 launches a pass otherwise)
        # (weight_images: the owner's persistent images, kept current by the optimiser step: no copy here)
        if images is not None:
            wb_all = images.w
        else:
            wb_all = [bufs.get(("w", i), (ws[i].shape[0], kpad[i]), bf, dev, fresh) for i in range(nl)]
            torch._foreach_copy_([wb_all[i][:, :ws[i].shape[1]] for i in range(nl)], [w_.detach() for w_ in ws])
        for i in range(nl - 1):
            w = ws[i]
            N = w.shape[0]
            assert N % 64 == 0 and kpad[i + 1] == N, "hidden widths must be multiples of 64"
            wb = wb_all[i]
            y = bufs.get(("h", i), (Mp, N), bf, dev, fresh)
            g = bufs.get(("g", i), (Mp, N), bf, dev, fresh) if track else None   # no backward pass will follow (GAE's value pass): the result alone
            _linear_train(h, wb, bs[i].detach().float().contiguous(), None, y, None, g, Mp, N, kpad[i], N, 0, act, False, st)
            wbs.append(wb); hs.append(y); gs.append(g)
            h = y
        w = ws[-1]
        wb = wb_all[-1]
        wbs.append(wb)
        out = torch.empty(Mp, w.shape[0], dtype=torch.float32, device=dev)
        _check(lib().ss_linear_bf16(_ptr(h), _ptr(wb), _ptr(bs[-1].detach().float().contiguous()), _ptr(out), Mp, w.shape[0], kpad[-1], w.shape[0],
                                    _cabi.ACTIVATIONS["none"], 1, st))
        ctx.act, ctx.M, ctx.Mp, ctx.kpad, ctx.dims = act, M, Mp, kpad, [(w_.shape[0], w_.shape[1]) for w_ in ws]
        ctx.det = det
        ctx.wts = images.wt if images is not None else None
        ctx.hs, ctx.gs, ctx.wbs = hs, gs, wbs
        return out[:M]

    @staticmethod
    def backward(ctx, grad_out):
        dev, st = grad_out.device, _launch_stream(grad_out.device)
        M, Mp, kpad, dims = ctx.M, ctx.Mp, ctx.kpad, ctx.dims
        nl = len(dims)
        bufs = ctx.bufs if ctx.bufs is not None else _Buffers()
        fresh = ctx.bufs is None
        bf = torch.bfloat16
        none = _cabi.ACTIVATIONS["none"]
        # the head's dZ: the caller's gradient, rounded to bf16, its width padded to a K
        nh = dims[-1][0]
        nhp = _pad(nh, 128)
        dz = bufs.get("dz_head", (Mp, nhp), bf, dev, fresh)
        dz[:M, :nh] = grad_out
        grads = [None] * (2 * nl)
        # the head's bias gradient (its dZ is the caller's tensor): dZ^T 1 by the weight-gradient kernel against a column of ones (torch's column reduction of a
        # [53 248, 69] tensor took 180 us, a matrix-vector product through rocBLAS 175)
        ones = bufs.get("ones", (Mp, 8), bf, dev, fresh, lambda t: t[:, 0].fill_(1.0))
        dbh = torch.zeros(_pad(nh, 8), 8, dtype=torch.float32, device=dev)
        no8s = [_pad(d[0], 8) for d in dims]
        # dX products the 256 x 256 kernel serves (column sums from the same launch); the others leave the bias gradient to torch
        dx256 = [i > 0 and Mp >= 2048 and kpad[i] >= 256 and (nhp if i == nl - 1 else dims[i][0]) % 128 == 0 for i in range(nl)]
        L = lib()
        if ctx.det:
            # one workspace for every product of the pass, the largest request; reused in stream order (a reduce ends before the next product starts)
            need = [L.ss_wgrad_bf16_det_workspace(Mp, no8s[-1], 8)] + [L.ss_wgrad_bf16_det_workspace(Mp, no8s[i], kpad[i]) for i in range(nl)]
            need += [L.ss_linear_bf16_dx_det_workspace(Mp, kpad[i], nhp if i == nl - 1 else dims[i][0]) for i in range(1, nl) if dx256[i]]
            assert min(need) > 0, need
            wsp = bufs.get("det_ws", (max(need) // 4,), torch.float32, dev, fresh)
            wgrad, dx, tail = L.ss_wgrad_bf16_det, L.ss_linear_bf16_dx_det, (_ptr(wsp), wsp.numel() * 4, st)
        else:
            wgrad, dx, tail = L.ss_wgrad_bf16, L.ss_linear_bf16_dx, (st,)
        _check(wgrad(_ptr(dz), _ptr(ones), _ptr(dbh), Mp, no8s[-1], 8, nhp, 8, 8, *tail))
        db = dbh[:nh, 0]
        # every weight and bias gradient of the pass in ONE zero-filled tensor (the kernels accumulate into them: 13 memsets otherwise).  Not kept between
        # passes: the optimiser holds the views as .grad until the next backward
        sizes = [no8s[i] * kpad[i] for i in range(nl)] + [kpad[i] for i in range(1, nl)]
        offs = [0]
        for z in sizes:
            offs.append(offs[-1] + _pad(z, 64))
        flat = torch.zeros(offs[-1], dtype=torch.float32, device=dev)
        # W^T of every layer but the first (the "W" operand of the dX products), all by one multi-tensor copy
        wts = ctx.wts
        if wts is None:
            wts = {i: bufs.get(("wt", i), (kpad[i], nhp if i == nl - 1 else dims[i][0]), bf, dev, fresh) for i in range(1, nl)}
            torch._foreach_copy_([wts[i][:, :dims[i][0]] for i in range(1, nl)], [ctx.wbs[i].t() for i in range(1, nl)])
        for i in range(nl - 1, -1, -1):
            n_out, n_in = dims[i]
            n_outp = dz.shape[1]
            # dW [n_out, kpad_i] = dZ^T h_below with both operands as they lie (ss_wgrad_bf16 contracts over their rows); db = the column sums of dZ
            no8 = no8s[i]
            dw = flat[offs[i]:offs[i] + no8 * kpad[i]].view(no8, kpad[i])
            _check(wgrad(_ptr(dz), _ptr(ctx.hs[i]), _ptr(dw), Mp, no8, kpad[i], n_outp, kpad[i], kpad[i], *tail))
            grads[2 * i] = dw[:n_out, :n_in]
            grads[2 * i + 1] = db if db is not None else dz[:, :n_out].sum(0, dtype=torch.float32)
            if i > 0:
                # dZ_below = (dZ W) * act'(z_below): W^T [kpad_i, n_outp] as the kernel's "W", contraction over this layer's outputs; the column sums of
                # the fp32 result (the bias gradient of the layer below) come out of the same launch where the 256 x 256 kernel serves the product
                wt = wts[i]
                nb = kpad[i]
                dzb = bufs.get(("dz", i), (Mp, nb), bf, dev, fresh)
                if dx256[i]:
                    db = flat[offs[nl + i - 1]:offs[nl + i - 1] + nb]
                    _check(dx(_ptr(dz), _ptr(wt), _ptr(ctx.gs[i - 1]), _ptr(dzb), _ptr(db), Mp, nb, n_outp, nb, *tail))
                else:
                    db = None
                    _linear_train(dz, wt, None, ctx.gs[i - 1], dzb, None, None, Mp, nb, n_outp, nb, 0, none, False, st)
                dz = dzb
        ctx.hs = ctx.gs = ctx.wbs = ctx.wts = None
        if ctx.bufs is not None:
            ctx.bufs.busy = False
        return (None, None, None, None, None, None, *grads)


class _WeightImages:
    """Persistent bf16 images of a FusedMLPTrain's weights, in the layouts the passes read: w[i] = W_i [n_out, kpad_i] for the forward products, wt[i] = W_i^T
    [kpad_i, n_out (the head's padded to 128)] for the dX products of every layer but the first.  The pads are zeroed once, here, and never written again.  Not
    part of _Buffers' fresh / busy logic: a graph whose backward runs after a later optimiser step sees that step's W^T."""

    def __init__(self, layers):
        nl = len(layers)
        dev, bf = layers[0].weight.device, torch.bfloat16
        dims = [tuple(l.weight.shape) for l in layers]
        kpad = [_pad(d[1], 128) if i == 0 else _pad(d[1], 64) for i, d in enumerate(dims)]
        self.layers = layers
        self.w = [torch.zeros(dims[i][0], kpad[i], dtype=bf, device=dev) for i in range(nl)]
        self.wt = {i: torch.zeros(kpad[i], _pad(dims[i][0], 128) if i == nl - 1 else dims[i][0], dtype=bf, device=dev) for i in range(1, nl)}
        self.versions = [None] * nl                                # each weight's torch version when its images were last known current

    def refresh_moved(self):
        """Re-cast the images of every weight that torch has written in place since they were last current (load_state_dict, a torch optimiser): the copies the
        passes made before.  The library's optimiser step writes weight and images together through raw pointers and leaves the version alone, so the usual
        call costs one integer compare per layer and no launch."""
        moved = [i for i, l in enumerate(self.layers) if l.weight._version != self.versions[i]]
        if not moved:
            return
        ws = [self.layers[i].weight.detach() for i in moved]
        torch._foreach_copy_([self.w[i][:, :w.shape[1]] for i, w in zip(moved, ws)], ws)
        tr = [i for i in moved if i > 0]
        if tr:
            torch._foreach_copy_([self.wt[i][:self.layers[i].weight.shape[1], :self.layers[i].weight.shape[0]] for i in tr], [self.w[i][:, :self.layers[i].weight.shape[1]].t() for i in tr])
        for i in moved:
            self.versions[i] = self.layers[i].weight._version


class FusedMLPTrain:
    """Callable over an existing stack of torch.nn.Linear layers (the hidden ones followed by `act`, then the head): differentiable with
    respect to the layers' parameters, not to the input (the update's inputs are rollout states).

    weight_images=True: the bf16 images of the weights (W and W^T, which every pass otherwise re-casts from the fp32 weights) are persistent and expected to be
    kept current by the optimiser: `images()` lists them for LibAdam.attach_images (learning/fused_optim.py), whose step writes them next to the fp32 weight.
    A weight that torch itself writes in place is noticed by its version counter and its images are re-cast before the next pass."""

    def __init__(self, hidden_layers, head, activation_name, deterministic=False, weight_images=False):
        if activation_name not in _cabi.ACTIVATIONS or activation_name == "none":
            raise ValueError(f"activation {activation_name!r} has no fused epilogue (silu, tanh, relu)")
        self.layers = list(hidden_layers) + [head]
        self.act = _cabi.ACTIVATIONS[activation_name]
        dev = self.layers[0].weight.device
        if dev.type != "cuda":
            raise RuntimeError("FusedMLPTrain needs the networks on a GPU (there is no CPU path)")
        self.deterministic = bool(deterministic)                  # the backward pass's reductions in a fixed order (module docstring)
        self.bufs, self.bufs_nograd = _Buffers(), _Buffers()
        self.weight_images = _WeightImages(self.layers) if weight_images else None

    def images(self):
        """[(weight, w_bf16, wt_bf16 or None)] per layer: the arguments of LibAdam.attach_images."""
        if self.weight_images is None:
            raise RuntimeError("FusedMLPTrain was built without weight_images")
        return [(l.weight, self.weight_images.w[i], self.weight_images.wt.get(i)) for i, l in enumerate(self.layers)]

    def operand(self, x):
        """The pass's own first-layer operand of an fp32 [M, D] input, made once for several passes over the same input (the critic's states: every iteration of an
        update reads them unchanged): a fresh zeroed [pad(M, 128), pad(D, 128)] bf16 tensor with the cast the pass does (`t[:M, :D] = x`).  `net(net.operand(x))` is
        `net(x)` bit for bit.  The operand must stay unchanged until the backward of every pass that took it has run (Bf16Operand)."""
        D = self.layers[0].weight.shape[1]
        if x.dim() != 2 or x.shape[1] != D or x.shape[0] < 1:
            raise ValueError(f"FusedMLPTrain.operand: an [M >= 1, {D}] input")
        M = x.shape[0]
        t = torch.zeros(_pad(M, 128), _pad(D, 128), dtype=torch.bfloat16, device=self.layers[0].weight.device)
        t[:M, :D] = x.detach().float()
        return Bf16Operand(t, M, D)

    def _check_operand(self, op):
        D, dev = self.layers[0].weight.shape[1], self.layers[0].weight.device
        t = op.t
        if not torch.is_tensor(t) or t.dtype != torch.bfloat16:
            raise ValueError("Bf16Operand: the tensor must be bf16")
        if t.device != dev:
            raise ValueError(f"Bf16Operand: the tensor must be on the network's device ({dev})")
        if op.D != D or op.M < 1 or tuple(t.shape) != (_pad(op.M, 128), _pad(D, 128)) or not t.is_contiguous():
            raise ValueError(f"Bf16Operand: a contiguous [pad(M, 128), {_pad(D, 128)}] tensor with D = {D} (got {tuple(t.shape)}, M = {op.M}, D = {op.D})")

    def __call__(self, x):
        """x: an fp32 [M, D] tensor, or a Bf16Operand (operand(); LibRunningNorm of learning/fused_norm.py) that the pass then uses as it is, without the cast."""
        if self.weight_images is not None:
            self.weight_images.refresh_moved()
        params = []
        for l in self.layers:
            params += [l.weight, l.bias]
        track = torch.is_grad_enabled()                           # (inside Function.forward the grad mode is always off)
        if isinstance(x, Bf16Operand):
            self._check_operand(x)
        else:
            x = x.detach().float()
        return _FusedMLP.apply(x, self.act, self.bufs if track else self.bufs_nograd, track, self.deterministic, self.weight_images, *params)
