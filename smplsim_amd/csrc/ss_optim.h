// ss_optim.h — the optimiser step of the PPO update (include/smplsim_mlp.h: ss_adam_step): the global gradient norm, clip_grad_norm_'s coefficient, Adam's
// update of p, exp_avg and exp_avg_sq, and the bf16 images of the new weights (W as the forward products read it, W^T as the dX products read it) in
// three launches for ALL tensors of a network — instead of torch's foreach-norm / stack / norm / clamp / foreach-mul chain, its fused Adam, and two
// multi-tensor bf16 copies per network pass (agents/agent_ppo.py:85-88 -> torch.optim.Adam; learning/fused_train.py).
//
// The tensors of a call come as a table of at most MAX_TENSORS descriptors that travels BY VALUE in the kernel arguments (72 bytes each): no host-to-device
// copy, nothing to keep alive after the call returns.  Every tensor is cut into tiles of 64 x 64 elements, numbered in descriptor order and row-major
// within a tensor; a workgroup finds its tensor by a linear search over the table's tile offsets (wave-uniform, scalar loads of the kernel arguments).
//
// Arithmetic as in ss_ppo_head.h: every value is formed in fp64 from the fp32 inputs and rounded to fp32 once, when it is stored.  Reproducible by
// construction: no atomics; a tile's sum of squares is formed in an order fixed by the thread that owns an element (below), whichever loads fetched it; the
// tiles' partials are added ascending from tile 0 by ONE wavefront.
#ifndef SS_OPTIM_H
#define SS_OPTIM_H
#include <hip/hip_runtime.h>

namespace optim {

constexpr int MAX_TENSORS = 32;
constexpr int TILE = 64;

struct Tensor {
  float *p, *m, *v;
  const float *g;
  unsigned short *w, *wt;                // the bf16 images (bit patterns), or null
  int rows, cols, ldg, ldw, ldwt;
  int tile0;                             // number of the tensor's first tile
};

struct Table {
  Tensor t[MAX_TENSORS];
  int count;
};

struct Hyper {
  double max_norm;                       // <= 0: clipping off
  double wd, b1, b2, step_size, bc2_sqrt, eps;   // step_size = lr / (1 - beta1^step), bc2_sqrt = sqrt(1 - beta2^step): formed on the host, in fp64
};

__device__ __forceinline__ double wave_sum(double v) {
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// the tensor that holds tile `tile`: the last one whose first tile is not beyond it
__device__ __forceinline__ int find_tensor(const Table &tb, int tile) {
  int k = 0;
  for (int i = 1; i < tb.count; i++) k = tb.t[i].tile0 <= tile ? i : k;
  return k;
}

__device__ __forceinline__ bool aligned16(const void *p) { return (reinterpret_cast<size_t>(p) & 15) == 0; }

// round-to-nearest-even bf16 of an fp32 value, on its bits; a NaN becomes the canonical quiet NaN 0x7FC0 (what torch's float -> bfloat16 copy writes on the device)
__device__ __forceinline__ unsigned bf16_bits(float f) {
  const unsigned u = __float_as_uint(f);
  return f != f ? 0x7FC0u : (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

// ---- launch 1: one fp64 partial per tile.  Thread t owns the tile's rows (t >> 4) + 16 k, k = 0 .. 3, and in each the columns 4 (t & 15) .. 4 (t & 15) + 3; it adds
// the squares of its elements with k ascending and the columns ascending within a row (elements outside the tensor are skipped); the 64 lanes of a wavefront meet by
// the xor butterfly (32, 16, ..., 1); then ((w0 + w1) + w2) + w3.  A thread's four columns come by one 16-byte load where the row stride and the base allow it.
__global__ void __launch_bounds__(256) ss_adam_sumsq_kernel(const Table tb, double *__restrict__ part) {
  const int tile = blockIdx.x;
  const Tensor &T = tb.t[find_tensor(tb, tile)];
  const int tpr = (T.cols + TILE - 1) / TILE, local = tile - T.tile0;
  const int r0 = (local / tpr) * TILE, c0 = (local % tpr) * TILE;
  const bool gvec = (T.ldg & 3) == 0 && aligned16(T.g);
  const int c = c0 + 4 * (threadIdx.x & 15);
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int r = r0 + (threadIdx.x >> 4) + 16 * k;
    if (r >= T.rows || c >= T.cols) continue;
    const float *row = T.g + (size_t)r * T.ldg + c;
    if (gvec && c + 3 < T.cols) {
      const float4 x = *reinterpret_cast<const float4 *>(row);
      acc += (double)x.x * (double)x.x;
      acc += (double)x.y * (double)x.y;
      acc += (double)x.z * (double)x.z;
      acc += (double)x.w * (double)x.w;
    } else {
      for (int j = 0; j < 4 && c + j < T.cols; j++) acc += (double)row[j] * (double)row[j];
    }
  }
  acc = wave_sum(acc);
  __shared__ double sh[4];
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[tile] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// ---- launch 2: S = (((part_0 + part_1) + part_2) + ...) ascending, by one wavefront: the lanes fetch 64 partials at a time (the next 64 are in flight while the current
// ones are added), every lane adds them in the same order (lane i's value by a broadcast), lane 0 stores.  part[ntiles] = S; grad_norm = float(sqrt(S)).
__global__ void __launch_bounds__(64) ss_adam_reduce_kernel(double *__restrict__ part, int ntiles, float *__restrict__ grad_norm) {
  const int lane = threadIdx.x;
  double sum = 0.0;
  double cur = lane < ntiles ? part[lane] : 0.0;
  for (int base = 0; base < ntiles; base += 64) {
    const int nb = base + 64 + lane;
    const double next = nb < ntiles ? part[nb] : 0.0;
    const int n = min(64, ntiles - base);
    if (n == 64) {   // (unrolled: the source lane is a constant, and only the 64 additions form a chain)
#pragma unroll
      for (int i = 0; i < 64; i++) sum += __shfl(cur, i, 64);
    } else {
      for (int i = 0; i < n; i++) sum += __shfl(cur, i, 64);
    }
    cur = next;
  }
  if (lane == 0) {
    part[ntiles] = sum;
    if (grad_norm) *grad_norm = (float)sqrt(sum);
  }
}

// ---- launch 3: the step
struct Elem { float p, m, v; };

__device__ __forceinline__ Elem adam(float p, float m, float v, float g, double c, const Hyper &h) {
  const double gd = c * (double)g + h.wd * (double)p;
  const double md = h.b1 * (double)m + (1.0 - h.b1) * gd;
  const double vd = h.b2 * (double)v + (1.0 - h.b2) * gd * gd;
  const double pd = (double)p - h.step_size * md / (sqrt(vd) / h.bc2_sqrt + h.eps);
  return Elem{(float)pd, (float)md, (float)vd};
}

// The W^T image goes through LDS: the tile's new fp32 values are kept as [64][64] floats, element (r, c) at r * 64 + ((c + 4 (r >> 3)) & 63).  The rotation by four
// columns per eight rows stands where a row pad would: a 32-lane half of the column read holds 4 neighbouring columns x 8 row groups (rows 8 q + j at step j), whose
// banks ((c + 4 q) mod 32) are 32 different ones — a pad alone cannot do that (rows 8 q apart are a multiple of 8 dwords apart for every pitch: four bank classes for
// eight row groups) — and the float4 writes of the row pass stay whole (the rotation is a multiple of four columns).
__device__ __forceinline__ int lds_at(int r, int c) { return r * TILE + ((c + 4 * (r >> 3)) & (TILE - 1)); }

__global__ void __launch_bounds__(256) ss_adam_step_kernel(const Table tb, const double *__restrict__ part, int ntiles, const Hyper h) {
  __shared__ __attribute__((aligned(16))) float tilebuf[TILE * TILE];
  const int tile = blockIdx.x, t = threadIdx.x;
  const Tensor &T = tb.t[find_tensor(tb, tile)];
  const int tpr = (T.cols + TILE - 1) / TILE, local = tile - T.tile0;
  const int r0 = (local / tpr) * TILE, c0 = (local % tpr) * TILE;
  // clip_grad_norm_'s coefficient: clamp(max_norm / (norm + 1e-6), max = 1), a NaN kept (torch.clamp)
  double c = 1.0;
  if (h.max_norm > 0.0) {
    const double coef = h.max_norm / (sqrt(part[ntiles]) + 1e-6);
    c = coef != coef ? coef : fmin(coef, 1.0);
  }
  const bool full = r0 + TILE <= T.rows && c0 + TILE <= T.cols && (T.cols & 3) == 0 && aligned16(T.p) && aligned16(T.m) && aligned16(T.v);
  if (full) {
    // a whole tile of a tensor whose rows start 16-byte aligned: thread t takes the columns 8 (t & 7) .. + 7 of the rows (t >> 3) and (t >> 3) + 32
    const bool gvec = (T.ldg & 3) == 0 && aligned16(T.g);
    const int cl = 8 * (t & 7);
#pragma unroll
    for (int pass = 0; pass < 2; pass++) {
      const int rl = (t >> 3) + 32 * pass;
      const size_t o = (size_t)(r0 + rl) * T.cols + c0 + cl;
      const float *gr = T.g + (size_t)(r0 + rl) * T.ldg + c0 + cl;
      float p[8], m[8], v[8], g[8];
      *reinterpret_cast<float4 *>(p) = *reinterpret_cast<const float4 *>(T.p + o);
      *reinterpret_cast<float4 *>(p + 4) = *reinterpret_cast<const float4 *>(T.p + o + 4);
      *reinterpret_cast<float4 *>(m) = *reinterpret_cast<const float4 *>(T.m + o);
      *reinterpret_cast<float4 *>(m + 4) = *reinterpret_cast<const float4 *>(T.m + o + 4);
      *reinterpret_cast<float4 *>(v) = *reinterpret_cast<const float4 *>(T.v + o);
      *reinterpret_cast<float4 *>(v + 4) = *reinterpret_cast<const float4 *>(T.v + o + 4);
      if (gvec) {
        *reinterpret_cast<float4 *>(g) = *reinterpret_cast<const float4 *>(gr);
        *reinterpret_cast<float4 *>(g + 4) = *reinterpret_cast<const float4 *>(gr + 4);
      } else {
#pragma unroll
        for (int j = 0; j < 8; j++) g[j] = gr[j];
      }
      unsigned b[8];
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const Elem e = adam(p[j], m[j], v[j], g[j], c, h);
        p[j] = e.p; m[j] = e.m; v[j] = e.v;
        b[j] = bf16_bits(e.p);
      }
      *reinterpret_cast<float4 *>(T.p + o) = *reinterpret_cast<const float4 *>(p);
      *reinterpret_cast<float4 *>(T.p + o + 4) = *reinterpret_cast<const float4 *>(p + 4);
      *reinterpret_cast<float4 *>(T.m + o) = *reinterpret_cast<const float4 *>(m);
      *reinterpret_cast<float4 *>(T.m + o + 4) = *reinterpret_cast<const float4 *>(m + 4);
      *reinterpret_cast<float4 *>(T.v + o) = *reinterpret_cast<const float4 *>(v);
      *reinterpret_cast<float4 *>(T.v + o + 4) = *reinterpret_cast<const float4 *>(v + 4);
      if (T.w)   // ld_w a multiple of 8 and the base 16-byte aligned (checked by the host): eight bf16 by one store
        *reinterpret_cast<uint4 *>(T.w + (size_t)(r0 + rl) * T.ldw + c0 + cl) = make_uint4(b[0] | b[1] << 16, b[2] | b[3] << 16, b[4] | b[5] << 16, b[6] | b[7] << 16);
      if (T.wt) {
        *reinterpret_cast<float4 *>(&tilebuf[lds_at(rl, cl)]) = *reinterpret_cast<const float4 *>(p);
        *reinterpret_cast<float4 *>(&tilebuf[lds_at(rl, cl + 4)]) = *reinterpret_cast<const float4 *>(p + 4);
      }
    }
    if (T.wt) {   // (wave-uniform: the same tensor for the whole workgroup)
      __syncthreads();
      // row c0 + cc of W^T holds this tile's column cc: 64 bf16 = eight 16-byte segments, neighbouring lanes on neighbouring segments
#pragma unroll
      for (int k = 0; k < 2; k++) {
        const int idx = t + 256 * k, cc = idx >> 3, q = idx & 7;
        unsigned b[8];
#pragma unroll
        for (int j = 0; j < 8; j++) b[j] = bf16_bits(tilebuf[lds_at(8 * q + j, cc)]);
        *reinterpret_cast<uint4 *>(T.wt + (size_t)(c0 + cc) * T.ldwt + r0 + 8 * q) = make_uint4(b[0] | b[1] << 16, b[2] | b[3] << 16, b[4] | b[5] << 16, b[6] | b[7] << 16);
      }
    }
    return;
  }
  // an edge tile, or a tensor whose rows do not start 16-byte aligned (cols not a multiple of 4): element by element, a wavefront on 64 neighbouring columns of a row
  for (int k = 0; k < TILE * TILE / 256; k++) {
    const int idx = t + 256 * k, r = r0 + (idx >> 6), cc = c0 + (idx & 63);
    if (r >= T.rows || cc >= T.cols) continue;
    const size_t o = (size_t)r * T.cols + cc;
    const Elem e = adam(T.p[o], T.m[o], T.v[o], T.g[(size_t)r * T.ldg + cc], c, h);
    T.p[o] = e.p; T.m[o] = e.m; T.v[o] = e.v;
    const unsigned short b = (unsigned short)bf16_bits(e.p);
    if (T.w) T.w[(size_t)r * T.ldw + cc] = b;
    if (T.wt) T.wt[(size_t)cc * T.ldwt + r] = b;
  }
}

}  // namespace optim
#endif
