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

Work tensors (activations, their derivatives, the dZ chain: ~1 GB a pass at the production widths) are leased from the object's _WorkSets.  A set belongs to ONE row
count M and starts zero-filled, so no pad row ever holds a longer batch's values.  A tracked pass holds its set until its backward has run or its graph is gone (a weak
reference to the autograd ctx: no flag to clear); a pass that finds the set of its M held gets a new zeroed one; a no-grad pass holds nothing after it returns.  At most
three sets are kept, least recently used first out: per network a PPO update passes T N rows (GAE, full-batch passes), N (the bootstrap) and the mini-batch size.
"""
import weakref

import torch

from .. import _cabi
from .._lib import _check, _launch_stream, _ptr, lib
from ._scratch import Scratch


def _pad(n, m):
    return (n + m - 1) // m * m


def _linear_train(x, w, bias, mul, y, dact, M, N, K, act, stream):
    _check(lib().ss_linear_bf16_train(_ptr(x), _ptr(w), _ptr(bias), _ptr(mul), _ptr(y), None, _ptr(dact), M, N, K, N, 0, act, 0, stream))


class _Plan:
    """What follows from the layers' shapes alone, computed once per FusedMLPTrain and read by its passes, its weight images and its operand checks."""

    def __init__(self, layers):
        self.dims = dims = [tuple(l.weight.shape) for l in layers]   # (n_out, n_in) of W_i
        self.nl = nl = len(dims)
        self.kpad = kpad = [_pad(d[1], 128 if i == 0 else 64) for i, d in enumerate(dims)]   # a layer's input width as a K (the first: whole K-tile pairs of the 256-tile kernel)
        self.no8 = [_pad(d[0], 8) for d in dims]                   # n_out as the weight-gradient kernel's output rows
        self.nhp = _pad(dims[-1][0], 128)                          # the head's width as a K
        self.n_outp = [d[0] for d in dims[:-1]] + [self.nhp]      # the width of layer i's dZ: the K of the dX product below it
        self.w_shapes = [(dims[i][0], kpad[i]) for i in range(nl)]   # the bf16 images: W_i for the forward products,
        self.wt_shapes = {i: (kpad[i], self.n_outp[i]) for i in range(1, nl)}   # W_i^T (the "W" operand of the dX products) of every layer but the first
        self.offs = [0]                                            # in a backward pass's flat gradient: dW_0 .. dW_{nl-1}, then db_0 .. db_{nl-2}
        for z in [self.no8[i] * kpad[i] for i in range(nl)] + [kpad[i] for i in range(1, nl)]:
            self.offs.append(self.offs[-1] + _pad(z, 64))

    def per_rows(self, Mp, deterministic):
        """dx256[i]: at Mp rows the 256 x 256 kernel serves layer i's dX product (column sums from its launch; else torch sums dZ), and the deterministic workspace's bytes."""
        dx256 = [i > 0 and Mp >= 2048 and self.kpad[i] >= 256 and self.n_outp[i] % 128 == 0 for i in range(self.nl)]
        if not deterministic:
            return dx256, 0
        L = lib()
        need = [L.ss_wgrad_bf16_det_workspace(Mp, self.no8[-1], 8)] + [L.ss_wgrad_bf16_det_workspace(Mp, self.no8[i], self.kpad[i]) for i in range(self.nl)]
        need += [L.ss_linear_bf16_dx_det_workspace(Mp, self.kpad[i], self.n_outp[i]) for i in range(1, self.nl) if dx256[i]]
        return dx256, min(need) if min(need) < 0 else max(need)   # (a refused query: Scratch.get raises the library's message)


class _WorkSet:
    """The work tensors of the passes with ONE row count M, zero-filled (and initialised by `init`) on first request.  held: a weak reference to what keeps the pass alive."""

    def __init__(self, M, device, per_rows):
        self.M, self.Mp, self.device, self.t, self.held = M, _pad(M, 128), device, {}, None
        self.dx256, self.det_bytes = per_rows(self.Mp)            # (_Plan.per_rows)

    def get(self, key, shape, dtype, init=None):
        t = self.t.get(key)
        if t is None:
            t = self.t[key] = torch.zeros(shape, dtype=dtype, device=self.device)
            if init is not None:
                init(t)
        return t


class _WorkSets:
    """The owner of a FusedMLPTrain's work tensors (module docstring): take(M, holder) lends the set of exactly M rows."""

    def __init__(self, device, per_rows):
        self.device, self.per_rows = device, per_rows
        self.sets = {}                                            # M -> _WorkSet, least recently used first

    def take(self, M, holder=None):
        """holder: what lives as long as the pass may read the set (a tracked pass's autograd ctx; None: stream order is enough).  A set whose holder is alive stays out of reach."""
        s = self.sets.pop(M, None)
        if s is None or (s.held is not None and s.held() is not None):
            s = _WorkSet(M, self.device, self.per_rows)
        self.sets[M] = s                                           # (the most recently used last)
        if len(self.sets) > 3:                                     # T N, N and the mini-batch size: the row counts of one network in one PPO update
            del self.sets[next(iter(self.sets))]
        s.held = weakref.ref(holder) if holder is not None else None
        return s


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
    def forward(ctx, x, net, track, *params):
        M = x.M if isinstance(x, Bf16Operand) else x.shape[0]       # (checked by FusedMLPTrain.__call__)
        work = net.work.take(M, ctx if track else None)            # (track: the set is this pass's until its backward has run or ctx is gone: an exception here too)
        p, act, dev = net.plan, net.act, work.device
        st = _launch_stream(dev)
        ws, bs = params[0::2], params[1::2]
        # the batch is the K of the weight-gradient products; its pad rows are zero in every dZ (zero rows of the head's gradient stay zero through (dZ W) * g),
        # so what the forward pass leaves in the pad rows of h (act(bias)) never reaches a gradient
        Mp, kpad = work.Mp, p.kpad
        bf = torch.bfloat16
        if isinstance(x, Bf16Operand):
            h = x.t                                                # read here and by the backward pass's first weight gradient; never written
        else:
            h = work.get("x", (Mp, kpad[0]), bf)                   # (pad rows and columns stay zero: the set is this M's, only [:M, :D] is ever written)
            h[:M, :x.shape[1]] = x
        hs, gs = [h], []
        # the layers' weights in bf16, all by one multi-tensor copy (they change with every optimiser step; 7 launches a pass otherwise)
        # (weight_images: the owner's persistent images, kept current by the optimiser step: no copy here)
        wbs = net.weight_images.w if net.weight_images is not None else [work.get(("w", i), p.w_shapes[i], bf) for i in range(p.nl)]
        if net.weight_images is None:
            torch._foreach_copy_([wbs[i][:, :p.dims[i][1]] for i in range(p.nl)], [w_.detach() for w_ in ws])
        for i in range(p.nl - 1):
            N = p.dims[i][0]
            y = work.get(("h", i), (Mp, N), bf)
            g = work.get(("g", i), (Mp, N), bf) if track else None   # no backward pass will follow (GAE's value pass): the result alone
            _linear_train(hs[-1], wbs[i], bs[i].detach().float().contiguous(), None, y, g, Mp, N, kpad[i], act, st)
            hs.append(y); gs.append(g)
        nh = p.dims[-1][0]
        out = torch.empty(Mp, nh, dtype=torch.float32, device=dev)
        _check(lib().ss_linear_bf16(_ptr(hs[-1]), _ptr(wbs[-1]), _ptr(bs[-1].detach().float().contiguous()), _ptr(out), Mp, nh, kpad[-1], nh,
                                    _cabi.ACTIVATIONS["none"], 1, st))
        if track:
            ctx.net, ctx.work, ctx.hs, ctx.gs, ctx.wbs = net, work, hs, gs, wbs
        return out[:M]

    @staticmethod
    def backward(ctx, grad_out):
        work, ctx.work = ctx.work, None
        assert work is not None, "FusedMLPTrain: the backward pass of this forward pass has already run"
        try:
            dev, st = grad_out.device, _launch_stream(grad_out.device)
            net, p, M, Mp = ctx.net, ctx.net.plan, work.M, work.Mp
            nl, dims, kpad, offs = p.nl, p.dims, p.kpad, p.offs
            bf = torch.bfloat16
            # the head's dZ: the caller's gradient, rounded to bf16, its width padded to a K
            nh = dims[-1][0]
            dz = work.get("dz_head", (Mp, p.nhp), bf)
            dz[:M, :nh] = grad_out
            grads = [None] * (2 * nl)
            # the head's bias gradient (its dZ is the caller's tensor): dZ^T 1 by the weight-gradient kernel against a column of ones (torch's column reduction of a
            # [53 248, 69] tensor took 180 us, a matrix-vector product through rocBLAS 175)
            ones = work.get("ones", (Mp, 8), bf, lambda t: t[:, 0].fill_(1.0))
            dbh = torch.zeros(p.no8[-1], 8, dtype=torch.float32, device=dev)
            L = lib()
            if net.deterministic:
                # the object's one workspace, reused in stream order (a reduce ends before the next product starts)
                wsp = net.scratch.get(dev, work.det_bytes)
                wgrad, dx, tail = L.ss_wgrad_bf16_det, L.ss_linear_bf16_dx_det, (_ptr(wsp), wsp.numel() * 8, st)
            else:
                wgrad, dx, tail = L.ss_wgrad_bf16, L.ss_linear_bf16_dx, (st,)
            _check(wgrad(_ptr(dz), _ptr(ones), _ptr(dbh), Mp, p.no8[-1], 8, p.nhp, 8, 8, *tail))
            db = dbh[:nh, 0]
            # every weight and bias gradient of the pass in ONE zero-filled tensor (the kernels accumulate into them: 13 memsets otherwise).  Not kept between
            # passes: the optimiser holds the views as .grad until the next backward
            flat = torch.zeros(offs[-1], dtype=torch.float32, device=dev)
            # W^T of every layer but the first (the "W" operand of the dX products), all by one multi-tensor copy
            if net.weight_images is not None:
                wts = net.weight_images.wt
            else:
                wts = {i: work.get(("wt", i), p.wt_shapes[i], bf) for i in range(1, nl)}
                torch._foreach_copy_([wts[i][:, :dims[i][0]] for i in range(1, nl)], [ctx.wbs[i].t() for i in range(1, nl)])
            for i in range(nl - 1, -1, -1):
                n_out, n_in = dims[i]
                # dW [n_out, kpad_i] = dZ^T h_below with both operands as they lie (ss_wgrad_bf16 contracts over their rows); db = the column sums of dZ
                no8, n_outp = p.no8[i], p.n_outp[i]
                dw = flat[offs[i]:offs[i] + no8 * kpad[i]].view(no8, kpad[i])
                _check(wgrad(_ptr(dz), _ptr(ctx.hs[i]), _ptr(dw), Mp, no8, kpad[i], n_outp, kpad[i], kpad[i], *tail))
                grads[2 * i] = dw[:n_out, :n_in]
                grads[2 * i + 1] = db if db is not None else dz[:, :n_out].sum(0, dtype=torch.float32)
                if i > 0:
                    # dZ_below = (dZ W) * act'(z_below): W^T [kpad_i, n_outp] as the kernel's "W", contraction over this layer's outputs; the column sums of
                    # the fp32 result (the bias gradient of the layer below) come out of the same launch where the 256 x 256 kernel serves the product
                    nb = kpad[i]
                    dzb = work.get(("dz", i), (Mp, nb), bf)
                    if work.dx256[i]:
                        db = flat[offs[nl + i - 1]:offs[nl + i - 1] + nb]
                        _check(dx(_ptr(dz), _ptr(wts[i]), _ptr(ctx.gs[i - 1]), _ptr(dzb), _ptr(db), Mp, nb, n_outp, nb, *tail))
                    else:
                        db = None
                        _linear_train(dz, wts[i], None, ctx.gs[i - 1], dzb, None, Mp, nb, n_outp, _cabi.ACTIVATIONS["none"], st)
                    dz = dzb
            return (None, None, None, *grads)
        finally:
            ctx.hs = ctx.gs = ctx.wbs = None
            work.held = None


class _WeightImages:
    """Persistent bf16 images of a FusedMLPTrain's weights, in the layouts the passes read: w[i] = W_i [n_out, kpad_i] for the forward products, wt[i] = W_i^T
    [kpad_i, n_out (the head's padded to 128)] for the dX products of every layer but the first.  The pads are zeroed once, here, and never written again.  Not
    leased like the work tensors: a graph whose backward runs after a later optimiser step sees that step's W^T."""

    def __init__(self, layers, plan):
        dev, bf = layers[0].weight.device, torch.bfloat16
        self.layers, self.dims = layers, plan.dims
        self.w = [torch.zeros(s, dtype=bf, device=dev) for s in plan.w_shapes]
        self.wt = {i: torch.zeros(s, dtype=bf, device=dev) for i, s in plan.wt_shapes.items()}
        self.versions = [None] * plan.nl                           # each weight's torch version when its images were last known current

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
            torch._foreach_copy_([self.wt[i][:self.dims[i][1], :self.dims[i][0]] for i in tr], [self.w[i][:, :self.dims[i][1]].t() for i in tr])
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
        self.device = dev = self.layers[0].weight.device
        if dev.type != "cuda":
            raise RuntimeError("FusedMLPTrain needs the networks on a GPU (there is no CPU path)")
        self.plan = plan = _Plan(self.layers)
        assert all(d[0] % 64 == 0 for d in plan.dims[:-1]), "hidden widths must be multiples of 64"   # (a hidden layer's output is the next one's K as it lies)
        self.deterministic = bool(deterministic)                  # the backward pass's reductions in a fixed order (module docstring)
        self.work, self.scratch = _WorkSets(dev, lambda Mp: plan.per_rows(Mp, self.deterministic)), Scratch()
        self.weight_images = _WeightImages(self.layers, plan) if weight_images else None

    def images(self):
        """[(weight, w_bf16, wt_bf16 or None)] per layer: the arguments of LibAdam.attach_images."""
        if self.weight_images is None:
            raise RuntimeError("FusedMLPTrain was built without weight_images")
        return [(l.weight, self.weight_images.w[i], self.weight_images.wt.get(i)) for i, l in enumerate(self.layers)]

    def operand(self, x):
        """The pass's own first-layer operand of an fp32 [M, D] input, made once for several passes over the same input (the critic's states: every iteration of an
        update reads them unchanged): a fresh zeroed [pad(M, 128), pad(D, 128)] bf16 tensor with the cast the pass does (`t[:M, :D] = x`).  `net(net.operand(x))` is
        `net(x)` bit for bit.  The operand must stay unchanged until the backward of every pass that took it has run (Bf16Operand)."""
        D = self.plan.dims[0][1]
        if x.dim() != 2 or x.shape[1] != D or x.shape[0] < 1:
            raise ValueError(f"FusedMLPTrain.operand: an [M >= 1, {D}] input")
        M = x.shape[0]
        t = torch.zeros(_pad(M, 128), self.plan.kpad[0], dtype=torch.bfloat16, device=self.device)
        t[:M, :D] = x.detach().float()
        return Bf16Operand(t, M, D)

    def _check_operand(self, op):
        D, kp, t = self.plan.dims[0][1], self.plan.kpad[0], op.t
        if not torch.is_tensor(t) or t.dtype != torch.bfloat16:
            raise ValueError("Bf16Operand: the tensor must be bf16")
        if t.device != self.device:
            raise ValueError(f"Bf16Operand: the tensor must be on the network's device ({self.device})")
        if op.D != D or op.M < 1 or tuple(t.shape) != (_pad(op.M, 128), kp) or not t.is_contiguous():
            raise ValueError(f"Bf16Operand: a contiguous [pad(M, 128), {kp}] tensor with D = {D} (got {tuple(t.shape)}, M = {op.M}, D = {op.D})")

    def __call__(self, x):
        """x: an fp32 [M, D] tensor, or a Bf16Operand (operand(); LibRunningNorm of learning/fused_norm.py) that the pass then uses as it is, without the cast."""
        if self.weight_images is not None:
            self.weight_images.refresh_moved()
        params = [p for l in self.layers for p in (l.weight, l.bias)]
        track = torch.is_grad_enabled()                           # (inside Function.forward the grad mode is always off)
        if isinstance(x, Bf16Operand):
            self._check_operand(x)
        else:
            x = x.detach().float()
        return _FusedMLP.apply(x, self, track, *params)
