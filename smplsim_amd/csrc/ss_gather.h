// ss_gather.h — the shuffle of a mini-batch epoch of the PPO update (include/smplsim_mlp.h: ss_gather_rows): the rows perm[i] of up to MAX_TENSORS tensors copied
// into a blocked layout by ONE launch — instead of one index_select per tensor per epoch and two copies per mini-batch into padded operand buffers
// (agents/agent_ppo.py:26-46 -> states[perm].clone(), ... and the slices of the loop; learning/minibatch.py).
//
// The tensors of a call come as a table of descriptors that travels BY VALUE in the kernel arguments, as in ss_optim.h.  Every tensor is cut into tiles of
// tile_rows destination rows, numbered in descriptor order; a workgroup finds its tensor by a linear search over the table's tile offsets (wave-uniform).
//
// A tensor is moved in units of 16, 4 or 2 bytes (the host picks the widest its bases, strides and row width allow).  A row of `upr` units is served by
// lpr = min(64, the next power of two >= upr) neighbouring lanes, so a 256-thread workgroup is on 256 / lpr rows at a time: a 1,156-byte row has a whole wavefront
// on 256 contiguous bytes per instruction, a one-column tensor has one THREAD per row (64 rows per wavefront, the index loads and the stores coalesced).  A thread
// works on four rows at a time (four index loads, then four unit loads per column step before the first store), and a tile holds four such rows per thread where a
// row takes a lane several units and eight where it takes one: with eight workgroups resident per CU that keeps tens of KiB of loads in flight per CU, what an HBM
// miss needs to be covered.  No value is interpreted: the units are integers.
//
// Bounds: a row index is compared with [0, src_rows) as an unsigned 64-bit value BEFORE any address is formed from it; a row that fails is skipped in every tensor.
#ifndef SS_GATHER_H
#define SS_GATHER_H
#include <hip/hip_runtime.h>

namespace gather {

constexpr int MAX_TENSORS = 8;
constexpr int THREADS = 256;
constexpr int ROWS_IN_FLIGHT = 4;        // rows a thread has loads outstanding for

struct Tensor {
  const char *src;
  char *dst;
  long long ld_src, ld_dst;              // row strides in BYTES
  int upr;                               // units per row
  int unit;                              // bytes per unit: 16, 4 or 2
  int lpr_log2;                          // lanes on one row = 1 << lpr_log2 (<= 64)
  int tile_rows;                         // destination rows per workgroup, a multiple of ROWS_IN_FLIGHT * (THREADS >> lpr_log2)
  int dst_block_stride;
  int tile0;                             // number of the tensor's first tile
};

struct Table {
  Tensor t[MAX_TENSORS];
  int count;
};

// the tensor that holds tile `tile`: the last one whose first tile is not beyond it
__device__ __forceinline__ int find_tensor(const Table &tb, int tile) {
  int k = 0;
  for (int i = 1; i < tb.count; i++) k = tb.t[i].tile0 <= tile ? i : k;
  return k;
}

template <typename U>
struct Row {
  const U *s;
  U *d;
  bool ok;
};

// A thread's share of a tile: the rows i, i + rpp, i + 2 rpp, ... of its lane group, FOUR at a time — their four index loads are issued together, then per unit
// column four loads, then four stores.  A row beyond the tile, or one whose index is out of range, is pointed at source row 0 (src_rows >= 1: a valid address) and
// only its stores are switched off: every load is unconditional, so nothing waits on a branch.
template <typename U>
__device__ __forceinline__ void copy_tile(const Tensor &T, const long long *__restrict__ perm, int src_rows, int rows, int block_rows, int r0) {
  const int t = threadIdx.x, lpr = 1 << T.lpr_log2, j0 = t & (lpr - 1), rpp = THREADS >> T.lpr_log2;
  const int n = (rows - r0 > T.tile_rows ? T.tile_rows : rows - r0) - (t >> T.lpr_log2);   // rows from this thread's first one to the tile's end
  if (j0 >= T.upr) return;
  const int first = r0 + (t >> T.lpr_log2);
  for (int o = 0; o < n; o += ROWS_IN_FLIGHT * rpp) {      // (offsets, not row numbers: rows may be INT32_MAX)
    auto row = [&](int k) {
      const int ok = o + k * rpp;
      const bool in = ok < n;
      const int i = first + (in ? ok : o);
      const long long p = perm[i];
      const bool good = in && (unsigned long long)p < (unsigned long long)src_rows;
      const long long drow = (long long)(i / block_rows) * T.dst_block_stride + i % block_rows;
      return Row<U>{reinterpret_cast<const U *>(T.src + (good ? p : 0) * T.ld_src), reinterpret_cast<U *>(T.dst + drow * T.ld_dst), good};
    };
    const Row<U> a = row(0), b = row(1), c = row(2), e = row(3);
    for (int j = j0; j < T.upr; j += lpr) {
      const U va = a.s[j], vb = b.s[j], vc = c.s[j], ve = e.s[j];
      if (a.ok) a.d[j] = va;
      if (b.ok) b.d[j] = vb;
      if (c.ok) c.d[j] = vc;
      if (e.ok) e.d[j] = ve;
    }
  }
}

__global__ void __launch_bounds__(THREADS) ss_gather_rows_kernel(const Table tb, const long long *__restrict__ perm, int src_rows, int rows, int block_rows) {
  const int tile = blockIdx.x;
  const Tensor &T = tb.t[find_tensor(tb, tile)];
  const long long r0 = (long long)(tile - T.tile0) * T.tile_rows;
  if (r0 >= rows) return;
  if (T.unit == 16) copy_tile<uint4>(T, perm, src_rows, rows, block_rows, (int)r0);      // (wave-uniform: one tensor per workgroup)
  else if (T.unit == 4) copy_tile<unsigned>(T, perm, src_rows, rows, block_rows, (int)r0);
  else copy_tile<unsigned short>(T, perm, src_rows, rows, block_rows, (int)r0);
}

}  // namespace gather
#endif
