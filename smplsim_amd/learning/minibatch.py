"""The shuffled order of a mini-batch epoch of the PPO update (include/smplsim_mlp.h: ss_gather_rows).

What it replaces: the reference's agents/agent_ppo.py:26-46 — per epoch `states[perm].clone(), critic_states[perm].clone(), ...` for seven tensors, then a slice of
each per mini-batch — and, on the library's network passes, the two copies per mini-batch that would put a slice into the padded bf16 operand of a pass.  Here the
batch is put into its shuffled order ONCE per epoch, by one launch, straight into a blocked layout whose blocks are what the passes take:

    sb = ShuffledBatch(dict(states=states, ret=ret, critic=Bf16Operand(...)), block_rows=B)
    for every epoch:
        sb.shuffle(perm)                                     # one ss_gather_rows call over the first nb * B entries of perm, nb = floor(M / B)
        for i in range(sb.num_blocks):
            blk = sb.block(i)                                # views: fp32 [B, cols] row slices; Bf16Operand([pad(B, 128), pad(D, 128)], B, D)

An fp32 source [M, cols] gets a destination [nb * B, cols] (block stride B).  A Bf16Operand source gets [nb * pad(B, 128), pad(D, 128)] (block stride pad(B, 128)):
block i is contiguous, of the exact shape FusedMLPTrain wants, and its pad rows are zero because they were zeroed when the destination was allocated and nothing
writes them afterwards.  Of an operand the first pad(D, 8) columns are moved (the source's columns >= D are zero by Bf16Operand's contract, and so stay the
destination's): rows of 16-byte units instead of 2-byte elements.  The rows perm[nb * B:] sit the epoch out (the reference's floor).

mode "torch" fills the same layout by torch indexing: the CPU path of the agent, the control of the GPU tests and the baseline of profiles/ppo_minibatch.txt.
The destinations are allocated zeroed once and reused by every shuffle; bind() points the object at the tensors of the next update when their shapes are the same.
A block must not be needed any more when the next shuffle is enqueued (same stream).
"""
import torch

from .fused_train import Bf16Operand, _pad


class _Source:
    __slots__ = ("name", "operand", "src", "dst", "cols", "gcols", "stride", "D")


class ShuffledBatch:
    def __init__(self, sources, block_rows, mode="kernel"):
        if mode not in ("kernel", "torch"):
            raise ValueError(f"ShuffledBatch: mode {mode!r} (kernel, torch)")
        if not sources:
            raise ValueError("ShuffledBatch: at least one source")
        self.B = int(block_rows)
        self.mode = mode
        self.items = []
        self.M = self.device = None
        for name, x in sources.items():
            s = _Source()
            s.name, s.operand = name, isinstance(x, Bf16Operand)
            t, M = self._source_tensor(x)
            if self.M is None:
                self.M, self.device = M, t.device
                if self.B < 1 or self.B > M:
                    raise ValueError(f"ShuffledBatch: 1 <= block_rows <= M (block_rows = {self.B}, M = {M})")
                self.num_blocks = M // self.B
            elif M != self.M or t.device != self.device:
                raise ValueError(f"ShuffledBatch: source {name!r} has {M} rows on {t.device}; the first has {self.M} on {self.device}")
            if s.operand:
                s.D, s.cols, s.gcols, s.stride = x.D, t.shape[1], _pad(x.D, 8), _pad(self.B, 128)
            else:
                s.D, s.cols, s.gcols, s.stride = None, t.shape[1], t.shape[1], self.B
            s.src = t
            s.dst = torch.zeros(self.num_blocks * s.stride, s.cols, dtype=t.dtype, device=t.device)
            self.items.append(s)
        if mode == "kernel":
            from .. import _cabi
            if self.device.type != "cuda":
                raise RuntimeError("ShuffledBatch: ss_gather_rows needs the sources on a GPU (mode='torch' is the CPU path)")
            if len(self.items) > _cabi.GATHER_MAX_TENSORS:
                raise ValueError(f"ShuffledBatch: at most {_cabi.GATHER_MAX_TENSORS} sources in one ss_gather_rows call")

    @staticmethod
    def _source_tensor(x):
        if isinstance(x, Bf16Operand):
            t = x.t
            if t.dtype != torch.bfloat16 or t.dim() != 2 or not t.is_contiguous() or tuple(t.shape) != (_pad(x.M, 128), _pad(x.D, 128)):
                raise ValueError("ShuffledBatch: a Bf16Operand source must be a contiguous bf16 [pad(M, 128), pad(D, 128)] tensor")
            return t, x.M
        if not torch.is_tensor(x) or x.dtype != torch.float32 or x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1:
            raise ValueError("ShuffledBatch: a source is an fp32 [M, cols] tensor or a Bf16Operand")
        x = x.detach()
        return (x if x.stride(1) == 1 and x.stride(0) >= x.shape[1] else x.contiguous()), x.shape[0]

    def matches(self, sources, block_rows, mode):
        """True if bind(sources) would succeed for this block size and mode."""
        if int(block_rows) != self.B or mode != self.mode or list(sources) != [s.name for s in self.items]:
            return False
        for s, x in zip(self.items, sources.values()):
            if isinstance(x, Bf16Operand) != s.operand:
                return False
            if s.operand:
                if x.M != self.M or x.D != s.D or x.t.device != self.device:
                    return False
            elif not torch.is_tensor(x) or x.dim() != 2 or tuple(x.shape) != (self.M, s.cols) or x.device != self.device:
                return False
        return True

    def bind(self, sources):
        """The sources of the next update (same names, kinds and shapes): the destinations stay."""
        if not self.matches(sources, self.B, self.mode):
            raise ValueError("ShuffledBatch.bind: the sources differ in name, kind or shape from those the object was built for")
        for s, x in zip(self.items, sources.values()):
            s.src = self._source_tensor(x)[0]

    @torch.no_grad()
    def shuffle(self, perm):
        """Destination row (i // B) * stride + i % B of every source = its row perm[i], for i < nb * B.  perm: int64 [>= nb * B] on the sources' device."""
        n = self.num_blocks * self.B
        if not torch.is_tensor(perm) or perm.dtype != torch.int64 or perm.dim() != 1 or perm.shape[0] < n or perm.device != self.device:
            raise ValueError(f"ShuffledBatch.shuffle: perm must be an int64 [>= {n}] tensor on {self.device}")
        if self.mode == "torch":
            idx = perm[:n]
            for s in self.items:
                rows = s.src[:self.M].index_select(0, idx)
                s.dst.view(self.num_blocks, s.stride, s.cols)[:, :self.B, :s.gcols] = rows.view(self.num_blocks, self.B, s.cols)[:, :, :s.gcols]
            return
        from .. import _cabi
        from .._lib import _check, _launch_stream, _ptr, lib
        perm = perm if perm.is_contiguous() else perm.contiguous()
        table = (_cabi.GatherTensor * len(self.items))()
        for j, s in enumerate(self.items):
            table[j] = _cabi.GatherTensor(src=s.src.data_ptr(), dst=s.dst.data_ptr(), elem_bytes=s.src.element_size(), cols=s.gcols, ld_src=s.src.stride(0),
                                          ld_dst=s.dst.stride(0), dst_block_stride=s.stride)
        _check(lib().ss_gather_rows(table, len(self.items), _ptr(perm), self.M, n, self.B, _launch_stream(self.device)))
        for s in self.items:
            torch.autograd.graph.increment_version(s.dst)          # written in place behind torch's back: say so

    def destination(self, name):
        """The whole destination tensor of a source (all blocks and what lies between them)."""
        for s in self.items:
            if s.name == name:
                return s.dst
        raise KeyError(name)

    def block(self, i):
        """{name: view} of block i: fp32 [B, cols] row slices; for an operand source a Bf16Operand over its [pad(B, 128), pad(D, 128)] slice."""
        if not 0 <= i < self.num_blocks:
            raise IndexError(f"ShuffledBatch.block: 0 <= i < {self.num_blocks}")
        out = {}
        for s in self.items:
            v = s.dst[i * s.stride:(i + 1) * s.stride]
            out[s.name] = Bf16Operand(v, self.B, s.D) if s.operand else v
        return out
