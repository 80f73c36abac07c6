// ss_gemm256_kernels.h — the kernels on the K loops of ss_gemm256.h: the 256 x 256 GEMM of the PPO update in its output modes (G256_*), the weight
// gradient from operands as they lie, its deterministic form and the fixed-order reduce of the deterministic forms.
#pragma once
#include "ss_gemm128.h"
#include "ss_gemm256.h"

namespace gemm256 {

using gemm128::u32x4;
using gemm128::pack_bf16x2;
using gemm128::store_chunk_edge;
using gemm128::load_chunk_edge;
using gemm128::xcd_tile;
using gemm128::c_row;

template <int MODE>
__global__ void __launch_bounds__(512) ss_gemm256_kernel(const LinearTrainArgs a) {
  extern __shared__ __attribute__((aligned(16))) __bf16 lds_g[];
  constexpr int T = gemm256::TILE;
  const int M = a.M, N = a.N, K = a.K;
  int bx = blockIdx.x, by = blockIdx.y;
  xcd_tile(bx, by, a.xcd_remap & 1);
  const int m0 = by * T, n0 = bx * T;
  const int nkt_all = K / 64, per = a.kper > 0 ? a.kper : nkt_all, kt0 = (int)blockIdx.z * per, kt1 = kt0 + per < nkt_all ? kt0 + per : nkt_all;
  const int nkt = kt1 - kt0;
  if (nkt < 2 || (nkt & 1)) return;                           // (the host cuts K into shares of an even number of tiles)
  f32x16 acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[i][j][r] = 0.f;
  gemm256::Loop L;
  L.init(a.X, a.W, M, N, K, m0, n0, kt0, reinterpret_cast<char *>(lds_g));
  L.run(acc, nkt);
  const int tid = threadIdx.x, lane = L.lane, wr = L.wr, wc = L.wc;
  const int col_l = wc * 64 + (lane & 31), row_l = wr * 128 + 4 * (lane >> 5);   // + tn * 32 resp. + tm * 32 + c_row(r)
  if constexpr (MODE == G256_ACCUM) {
    float *Yf = reinterpret_cast<float *>(a.Y);
#pragma unroll
    for (int tn = 0; tn < 2; tn++) {
      const int col = n0 + col_l + tn * 32;
      const float bv = (a.bias && col < N && blockIdx.z == 0) ? a.bias[col] : 0.f;
#pragma unroll
      for (int tm = 0; tm < 4; tm++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
          const int row = m0 + row_l + tm * 32 + c_row(r);
          if (row < M && col < N) unsafeAtomicAdd(Yf + (size_t)row * a.ldy + col, acc[tm][tn][r] + bv);
        }
    }
  } else {
    constexpr bool HAS_MUL = MODE == G256_DX || MODE == G256_DXN || MODE == G256_DXN_DET, HAS_D = MODE == G256_FWD || MODE == G256_FWDN, HAS_T = MODE == G256_FWD || MODE == G256_DX;
    constexpr int CS = T + 8, CPR = T / 8;
    constexpr int HALF_IMG = 128 * CS;                        // elements of one half image (128 rows)
    __bf16 *Cs = lds_g;
    __bf16 *Yb = reinterpret_cast<__bf16 *>(a.Y);
    const bool rows_vec = (a.ldy & 7) == 0 && (reinterpret_cast<size_t>(Yb) & 15) == 0 && (!HAS_D || (reinterpret_cast<size_t>(a.Dact) & 15) == 0) &&
                          (!HAS_MUL || (reinterpret_cast<size_t>(a.mul) & 15) == 0);
    // ---- the multiplying operand: the tile by 16-byte row loads into LDS, from there into the accumulators
    if constexpr (HAS_MUL) {
      if (m0 + T <= M && n0 + T <= N && rows_vec) {
        // a tile inside the matrix: eight loads in flight, NO control flow between them.  With the bounds tests around every load the compiler put each load in
        // its own branch region and waited (vmcnt(0)) before entering the next: 16 HBM round trips one after the other, 30 us per tile, +110 us on a 53 248 x 1024
        // product (profiles/r06_gemm256.txt)
        const __bf16 *src = a.mul + (size_t)(m0 + tid / CPR) * a.ldy + n0 + (tid % CPR) * 8;
        __bf16 *dst = Cs + (tid / CPR) * CS + (tid % CPR) * 8;
        const size_t rstep = (size_t)(512 / CPR) * a.ldy;     // 512 threads cover 16 rows per step
#pragma unroll
        for (int i0 = 0; i0 < T * CPR / 512; i0 += 8) {
          u32x4 v[8];
#pragma unroll
          for (int i = 0; i < 8; i++) v[i] = *reinterpret_cast<const u32x4 *>(src + (size_t)(i0 + i) * rstep);
#pragma unroll
          for (int i = 0; i < 8; i++) *reinterpret_cast<u32x4 *>(dst + (i0 + i) * (512 / CPR) * CS) = v[i];
        }
      } else {
#pragma unroll 1
        for (int i = 0; i < T * CPR / 512; i++) {
          const int id = tid + 512 * i, rl = id / CPR, cc = (id % CPR) * 8, row = m0 + rl, col = n0 + cc;
          u32x4 v = {0u, 0u, 0u, 0u};
          if (row < M && col < N) {
            const __bf16 *src = a.mul + (size_t)row * a.ldy + col;
            if (rows_vec && col + 8 <= N) v = *reinterpret_cast<const u32x4 *>(src);
            else v = load_chunk_edge(src, N - col);
          }
          *reinterpret_cast<u32x4 *>(Cs + rl * CS + cc) = v;
        }
      }
      __syncthreads();
    }
#pragma unroll
    for (int tn = 0; tn < 2; tn++) {
      const int col = n0 + col_l + tn * 32;
      const float bv = (a.bias && col < N) ? a.bias[col] : 0.f;
#pragma unroll
      for (int tm = 0; tm < 4; tm++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
          float v = acc[tm][tn][r] + bv;
          if constexpr (HAS_MUL) v *= (float)Cs[(row_l + tm * 32 + c_row(r)) * CS + col_l + tn * 32];
          acc[tm][tn][r] = v;
        }
    }
    if constexpr (HAS_MUL) {
      constexpr bool COLSUM_DET = MODE == G256_DXN_DET;       // a.colsum is the [2 * row tiles, N] image of partial sums: row 2 * (row tile) + (wave row), stored
      if (COLSUM_DET || a.colsum) {
        // bias gradient of the layer below: the column sums of dZ, from the fp32 values in the accumulators (a lane holds 64 rows of each of its two columns;
        // its partner 32 lanes on holds the other 64 of this wave's 128), one atomic per column and wave
#pragma unroll
        for (int tn = 0; tn < 2; tn++) {
          float sum = 0.f;
#pragma unroll
          for (int tm = 0; tm < 4; tm++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
              const int row = m0 + row_l + tm * 32 + c_row(r);
              sum += row < M ? acc[tm][tn][r] : 0.f;
            }
          sum += __shfl_xor(sum, 32, 64);
          const int col = n0 + col_l + tn * 32;
          if constexpr (COLSUM_DET) {
            if (lane < 32 && col < N) a.colsum[(size_t)(2 * by + wr) * N + col] = sum;
          } else {
            if (lane < 32 && col < N) unsafeAtomicAdd(a.colsum + col, sum);
          }
        }
      }
      __syncthreads();
    }
    // ---- result (and derivative) in two halves of the tile — each wave's upper 64 rows, then its lower 64 — so that a half's two images sit in
    // LDS side by side and the exponential is evaluated ONCE per element; the accumulators keep the activated values for the transposed image
    auto half_rows = [&](__bf16 *dst, const __bf16 *img, int half) {
      u32x4 v[8];
#pragma unroll
      for (int i = 0; i < 8; i++) {
        const int id = tid + 512 * i, lr = id / CPR, cc = (id % CPR) * 8;
        v[i] = *reinterpret_cast<const u32x4 *>(img + lr * CS + cc);
      }
#pragma unroll
      for (int i = 0; i < 8; i++) {
        const int id = tid + 512 * i, lr = id / CPR, cc = (id % CPR) * 8, row = m0 + (lr >> 6) * 128 + half * 64 + (lr & 63), col = n0 + cc;
        if (row >= M || col >= N) continue;
        if (rows_vec && col + 8 <= N) *reinterpret_cast<u32x4 *>(dst + (size_t)row * a.ldy + col) = v[i];
        else store_chunk_edge(dst + (size_t)row * a.ldy + col, v[i], N - col);
      }
    };
    auto halves = [&](auto fn2) {
#pragma unroll
      for (int half = 0; half < 2; half++) {
#pragma unroll
        for (int tml = 0; tml < 2; tml++)
#pragma unroll
          for (int tn = 0; tn < 2; tn++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
              float h, d;
              fn2(acc[2 * half + tml][tn][r], h, d);
              acc[2 * half + tml][tn][r] = h;
              const int at = c_row(wr * 64 + tml * 32, r, lane) * CS + col_l + tn * 32;
              Cs[at] = (__bf16)h;
              if constexpr (HAS_D) Cs[HALF_IMG + at] = (__bf16)d;
            }
        __syncthreads();
        half_rows(Yb, Cs, half);
        if constexpr (HAS_D) half_rows(a.Dact, Cs + HALF_IMG, half);
        __syncthreads();
      }
    };
    if (a.act == SS_ACT_SILU) halves([](float v, float &h, float &d) { const float sg = __builtin_amdgcn_rcpf(1.f + __expf(-v)); h = v * sg; d = sg * (1.f + v * (1.f - sg)); });
    else if (a.act == SS_ACT_TANH) halves([](float v, float &h, float &d) { const float e = __expf(-2.f * fabsf(v)); const float t = (1.f - e) * __builtin_amdgcn_rcpf(1.f + e); h = v < 0.f ? -t : t; d = 1.f - t * t; });
    else if (a.act == SS_ACT_RELU) halves([](float v, float &h, float &d) { h = v > 0.f ? v : 0.f; d = v > 0.f ? 1.f : 0.f; });
    else halves([](float v, float &h, float &d) { h = v; d = 1.f; });
    // ---- transposed image: an accumulator's registers r .. r + 3 are four consecutive rows of one column = 8 contiguous bytes of it
    if constexpr (HAS_T) {
      typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
#pragma unroll
      for (int tm = 0; tm < 4; tm++)
#pragma unroll
        for (int tn = 0; tn < 2; tn++)
#pragma unroll
          for (int r = 0; r < 16; r += 4) {
            u32x2 v;
            v[0] = pack_bf16x2(acc[tm][tn][r], acc[tm][tn][r + 1]); v[1] = pack_bf16x2(acc[tm][tn][r + 2], acc[tm][tn][r + 3]);
            *reinterpret_cast<u32x2 *>(Cs + (col_l + tn * 32) * CS + row_l + tm * 32 + 8 * (r >> 2)) = v;
          }
      __syncthreads();
      const bool cols_vec = (a.ldyt & 7) == 0 && (reinterpret_cast<size_t>(a.Yt) & 15) == 0;
#pragma unroll
      for (int i0 = 0; i0 < T * CPR / 512; i0 += 8) {
        u32x4 v[8];
#pragma unroll
        for (int i = 0; i < 8; i++) {
          const int id = tid + 512 * (i0 + i), cl = id / CPR, rc = (id % CPR) * 8;
          v[i] = *reinterpret_cast<const u32x4 *>(Cs + cl * CS + rc);
        }
#pragma unroll
        for (int i = 0; i < 8; i++) {
          const int id = tid + 512 * (i0 + i), cl = id / CPR, rc = (id % CPR) * 8, col = n0 + cl, row = m0 + rc;
          if (col >= N || row >= M) continue;
          if (cols_vec && row + 8 <= M) *reinterpret_cast<u32x4 *>(a.Yt + (size_t)col * a.ldyt + row) = v[i];
          else store_chunk_edge(a.Yt + (size_t)col * a.ldyt + row, v[i], M - row);
        }
      }
    }
  }
}

__global__ void __launch_bounds__(512) ss_wgrad_tn_kernel(const WgradArgs a) {
  extern __shared__ __attribute__((aligned(16))) __bf16 lds_g[];
  const int i0 = blockIdx.y * 256, j0 = blockIdx.x * 256;
  const int kt0 = (int)blockIdx.z * a.kper, kt1 = kt0 + a.kper < a.nkt ? kt0 + a.kper : a.nkt, nkt = kt1 - kt0;
  if (nkt < 2 || (nkt & 1)) return;
  f32x16 acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[i][j][r] = 0.f;
  gemm256::LoopTN L;
  L.init(a.Z, a.H, a.ldz, a.ldh, a.NI, a.NJ, i0, j0, kt0, reinterpret_cast<char *>(lds_g));
  L.run(acc, nkt);
  const int lane = L.lane;
#pragma unroll
  for (int tn = 0; tn < 2; tn++) {
    const int col = j0 + L.wc * 64 + tn * 32 + (lane & 31);
#pragma unroll
    for (int tm = 0; tm < 4; tm++)
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int row = c_row(i0 + L.wr * 128 + tm * 32, r, lane);
        if (row < a.NI && col < a.NJ) unsafeAtomicAdd(a.dW + (size_t)row * a.ldw + col, acc[tm][tn][r]);
      }
  }
}

// ss_wgrad_bf16_det: the same K loop and K split, but the tile of partial sums of K share blockIdx.z is STORED into the share's own dense [NI, NJ] image of
// the workspace (a.dW, a.ldw = NJ) instead of added to dW — no atomics, no read of the output; ss_reduce_shares_kernel then adds the images to dW in a fixed
// order.  A share without K tiles stores zeros (split_256 leaves none; the reduce pass reads every share).  A kernel of its own, not a template parameter of
// the one above: wrapped in a shared body the default kernel's scalar prologue came out in a different order.
__global__ void __launch_bounds__(512) ss_wgrad_tn_det_kernel(const WgradArgs a) {
  extern __shared__ __attribute__((aligned(16))) __bf16 lds_g[];
  const int i0 = blockIdx.y * 256, j0 = blockIdx.x * 256;
  const int kt0 = (int)blockIdx.z * a.kper, kt1 = kt0 + a.kper < a.nkt ? kt0 + a.kper : a.nkt, nkt = kt1 - kt0;
  f32x16 acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[i][j][r] = 0.f;
  gemm256::LoopTN L;
  L.init(a.Z, a.H, a.ldz, a.ldh, a.NI, a.NJ, i0, j0, kt0, reinterpret_cast<char *>(lds_g));
  if (nkt >= 2 && !(nkt & 1)) L.run(acc, nkt);
  const int lane = L.lane;
  float *out = a.dW + (size_t)blockIdx.z * a.NI * a.NJ;
#pragma unroll
  for (int tn = 0; tn < 2; tn++) {
    const int col = j0 + L.wc * 64 + tn * 32 + (lane & 31);
#pragma unroll
    for (int tm = 0; tm < 4; tm++)
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int row = c_row(i0 + L.wr * 128 + tm * 32, r, lane);
        if (row < a.NI && col < a.NJ) out[(size_t)row * a.ldw + col] = acc[tm][tn][r];
      }
  }
}

// Fixed-order reduce of the deterministic forms: out[r, c] += ((p_0 + p_1) + p_2) + ... + p_{S-1} at [r, c], p_s the dense [rows, cols] image at
// part + s * rows * cols.  The sum over the shares is formed first, in ascending share order, in fp32, starting from p_0; out (row stride ldo >= cols, its
// padding untouched) is read and written once.  One element per thread; the loads of eight shares are issued together and only the additions form a chain.
__global__ void __launch_bounds__(256) ss_reduce_shares_kernel(const float *__restrict__ part, float *__restrict__ out, int rows, int cols, int ldo, int S) {
  const int n = rows * cols, idx = (int)blockIdx.x * 256 + threadIdx.x;   // (the host keeps rows * cols below 2^31)
  if (idx >= n) return;
  const float *p = part + idx;
  float sum = p[0];
  int s = 1;
  for (; s + 8 <= S; s += 8) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; j++) v[j] = p[(size_t)(s + j) * n];
#pragma unroll
    for (int j = 0; j < 8; j++) sum += v[j];
  }
  for (; s < S; s++) sum += p[(size_t)s * n];
  float *o = out + (size_t)(idx / cols) * ldo + idx % cols;
  *o += sum;
}

}  // namespace gemm256
