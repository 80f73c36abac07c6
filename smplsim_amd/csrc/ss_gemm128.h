// ss_gemm128.h — the 128-row bf16 GEMM kernels of the policy MLP for gfx950: y = act(x W^T + b) on the matrix cores
// (v_mfma_f32_32x32x16_bf16: bf16 operands, fp32 accumulation), bias and activation fused into the epilogue; and the pieces the
// kernels of every tile size share (activations, 16-byte chunk helpers, XCD tile order, the MFMA C layout).
//
// Tiling for 64-wide wavefronts: a workgroup of 8 waves (4 x 2) owns a 128 x BN output tile (BN = 64 / 128 / 192 / 256: the one whose
// tile count fills the 256 CUs in whole rounds), each wave 32 x BN/2 of it = 1 x BN/64 MFMA tiles of 32 x 32 in 16 .. 64 accumulator
// registers (8 waves instead of 4 with twice the tile each: -16 % on the whole MLP — at 4096 rows there are only ~1.5 workgroups
// per CU, and the K loop's barrier and load latency need waves to hide behind; a 16-wave split measured the same as 8).  Both operands are K-contiguous (activations row-major, weights in torch.nn.Linear's [out, in] layout), so a lane's
// MFMA fragment — 8 consecutive k of one row — is one 16-byte LDS read; K advances 64 per LDS tile (four MFMA K-steps), the next
// tile's global loads are in flight while the current one is multiplied (register double buffer, two LDS buffers, one barrier per
// tile).  LDS rows are padded by 8 bf16 (16 B) so that the 32 rows a fragment read touches spread over the banks.
// What bounds it (round 4, profiles/r04_mlp_gemm.txt): not the matrix cores — a 4-wave variant with 64 x 96 wave tiles (0.83 instead of 1.33
// fragment reads per MFMA, accumulators in AGPRs) ran 58 us against 41 us on the 2048 -> 1536 layer and was not faster with its MFMAs
// REMOVED (61.6 vs 61.4 us); without its LDS stores 40.6 us, without the global loads of the loop 47.6 us.  The K loop is a chain of
// global-load -> LDS-store -> barrier -> fragment-read latencies that only resident waves hide, and the 92-111 KB of LDS of a wide tile
// allow one workgroup per CU.  The 8-wave kernel stays; the wide tiles give 616 (was 570) TFLOP/s on that layer = 0.25 of the dense peak.
// The A and B fragments use the same lane -> k assignment (k = k16 + 8 * (lane / 32) + j), which is all the instruction needs for
// the products to pair up; the C layout is col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/smplsim_mlp.h"
#include "ss_gemm256.h"

namespace gemm128 {

using gemm256::LinearTrainArgs;

using gemm256::bf16x8;
using gemm256::f32x16;
using gemm256::gvoid;
using gemm256::lvoid;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;   // 16-byte staging register (a native vector: HIP's uint4 class kept loop-carried stages in scratch)

constexpr int BM = 128;

// Epilogue arithmetic with the activation chosen ONCE (round 5: the per-element `switch` with an IEEE division behind it was ~75
// instructions per output element, 3600 per wave for a 32 x 96 wave tile — a quarter of the kernel's time on the wide layers);
// reciprocal by v_rcp_f32 (1 ulp: invisible behind the bf16 rounding of the result).
struct ActNone { __device__ __forceinline__ float operator()(float v) const { return v; } };
struct ActSilu { __device__ __forceinline__ float operator()(float v) const { return v * __builtin_amdgcn_rcpf(1.f + __expf(-v)); } };
struct ActTanh { __device__ __forceinline__ float operator()(float v) const { const float e = __expf(-2.f * fabsf(v)); const float t = (1.f - e) * __builtin_amdgcn_rcpf(1.f + e); return v < 0.f ? -t : t; } };
struct ActRelu { __device__ __forceinline__ float operator()(float v) const { return v > 0.f ? v : 0.f; } };
template <class F> __device__ __forceinline__ void with_activation(int act, F &&f) {
  if (act == SS_ACT_SILU) f(ActSilu{}); else if (act == SS_ACT_TANH) f(ActTanh{}); else if (act == SS_ACT_RELU) f(ActRelu{}); else f(ActNone{});
}

__device__ __forceinline__ unsigned pack_bf16x2(float lo, float hi) {
  union { __bf16 h[2]; unsigned u; } c;
  c.h[0] = (__bf16)lo; c.h[1] = (__bf16)hi;
  return c.u;
}
// the first min(n, 8) elements of a 16-byte chunk, 2 bytes at a time (static indices: a dynamically indexed chunk lives in scratch)
__device__ __forceinline__ void store_chunk_edge(__bf16 *dst, const u32x4 &v, int n) {
#pragma unroll
  for (int j = 0; j < 8; j++)
    if (j < n) reinterpret_cast<unsigned short *>(dst)[j] = (unsigned short)((j & 1) ? (v[j >> 1] >> 16) : (v[j >> 1] & 0xffffu));
}
__device__ __forceinline__ u32x4 load_chunk_edge(const __bf16 *src, int n) {
  u32x4 v = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int j = 0; j < 8; j++)
    if (j < n) v[j >> 1] |= (unsigned)reinterpret_cast<const unsigned short *>(src)[j] << (16 * (j & 1));
  return v;
}

// XCD-aware tile order: workgroups are dealt round-robin to the 8 XCDs (id % 8), each with its own 4 MB L2.  Give XCD x the
// row-blocks [x gy/8, (x+1) gy/8) and walk them column-block-major inside the XCD: its activations (gy/8 row-blocks) stay in
// its L2 across all column-blocks and the weights stream through once per XCD — instead of every XCD touching every row-block
// (the kernels are bound by L2 / fabric traffic: 64 FLOP per byte at 128 x 128 tiles).  (bx, by) = (blockIdx.x, blockIdx.y) on entry; `on`: the caller's switch.
__device__ __forceinline__ void xcd_tile(int &bx, int &by, bool on) {
  const int gx = gridDim.x, gy = gridDim.y;
  if (on && gy % 8 == 0) {
    const int id = by * gx + bx, xcd = id & 7, idx = id >> 3, rows_per = gy >> 3;
    by = xcd * rows_per + idx % rows_per;
    bx = idx / rows_per;
  }
}

// MFMA C layout (col = lane & 31): the row of accumulator register r on this lane, row0 the first row of its 32 x 32 tile; and the
// register's part of it alone, for callers that keep the lane's part in row0
__device__ __forceinline__ constexpr int c_row(int r) { return (r & 3) + 8 * (r >> 2); }
__device__ __forceinline__ constexpr int c_row(int row0, int r, int lane) { return row0 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

// The bf16 rows of a 128 x BN tile staged in LDS (row stride BN + 8) to dst [M, ld], by the NT threads of the workgroup: 16-byte chunks,
// element-wise where ld or dst is not aligned (per destination: two images of a tile may differ) or the chunk crosses column N.
template <int BN, int NT>
__device__ __forceinline__ void store_tile_rows(const __bf16 *Cs, __bf16 *dst, int ld, int m0, int n0, int M, int N, int tid) {
  constexpr int CS = BN + 8, CPR = BN / 8;                    // 16-byte chunks per tile row
  const bool vec_ok = (ld & 7) == 0 && (reinterpret_cast<size_t>(dst) & 15) == 0;
#pragma unroll
  for (int i = 0; i < BM * CPR / NT; i++) {
    const int id = tid + NT * i, rl = id / CPR, cc = (id % CPR) * 8, row = m0 + rl, col = n0 + cc;
    if (row >= M || col >= N) continue;
    const u32x4 v = *reinterpret_cast<const u32x4 *>(Cs + rl * CS + cc);
    if (vec_ok && col + 8 <= N) *reinterpret_cast<u32x4 *>(dst + (size_t)row * ld + col) = v;
    else store_chunk_edge(dst + (size_t)row * ld + col, v, N - col);
  }
}

template <int BN, int BK, bool F32OUT, int WM, int WN = 2>
__global__ void __launch_bounds__(64 * WM * WN) ss_linear_kernel(const __bf16 *__restrict__ X, const __bf16 *__restrict__ W, const float *__restrict__ bias,
                                                        void *__restrict__ Y, int M, int N, int K, int ldy, int act, int xcd_remap) {
  constexpr int TN = BN / (32 * WN);                         // MFMA tiles per wave along N (WM x WN waves, each (128 / WM) x (BN / WN))
  constexpr int LDS_STRIDE = BK + 8;                         // K per LDS tile (64, or 32 when K is an odd multiple of 32); rows padded by 16 bytes
  constexpr int NT = 64 * WM * WN;
  constexpr int TM = BM / (32 * WM);                         // MFMA tiles per wave along M (2 for 4 waves, 1 for 8)
  constexpr int CPR = BK / 8;                                // 16-byte chunks per tile row
  constexpr int ACH = BM * CPR / NT, BCH = BN * CPR / NT;    // chunks per thread

  // dynamic LDS (the 192- and 256-column tiles need 92 / 111 KB: above the 64 KB of static __shared__): A buffers, then B buffers
  extern __shared__ __attribute__((aligned(16))) __bf16 lds_ab[];
  __bf16(*As)[BM * LDS_STRIDE] = reinterpret_cast<__bf16(*)[BM * LDS_STRIDE]>(lds_ab);
  __bf16(*Bs)[BN * LDS_STRIDE] = reinterpret_cast<__bf16(*)[BN * LDS_STRIDE]>(lds_ab + 2 * BM * LDS_STRIDE);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave / WN, wn = wave % WN;
  int bx = blockIdx.x, by = blockIdx.y;
  xcd_tile(bx, by, xcd_remap);
  const int m0 = by * BM, n0 = bx * BN;
  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; i++)
#pragma unroll
    for (int j = 0; j < TN; j++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[i][j][r] = 0.f;
  // global -> registers -> LDS: 16-byte chunk c of a tile = row c / CPR, k offset (c % CPR) * 8; rows beyond the matrix re-read its
  // last row.  The row of chunk tid + 256 i is the row of chunk tid plus 256 i / CPR, the k offset is the same.
  const int crow = tid / CPR, ckc = (tid % CPR) * 8, soff0 = crow * LDS_STRIDE + ckc;
  constexpr int RSTEP = NT / CPR;                           // rows between a thread's consecutive chunks
  // Two register stages: the loads of tile t + 2 are issued while tile t is multiplied and are written to LDS one step later, so a
  // load has two steps to land (one step — ~16 MFMAs per wave — is shorter than the memory latency; with a single stage every
  // step waited for its own load: 1.6 us per step).  The K loop is unrolled by two so that the stages are fixed registers.
  // (the stages are structs of named registers: arrays indexed by unrolled loops were left in scratch by the compiler here)
  struct Stage { u32x4 a0, a1, a2, a3, b0, b1, b2, b3; };
  Stage s0, s1;
  const int nkt = K / BK;
  const __bf16 *xrow[4], *wrow[4];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int ra = m0 + crow + RSTEP * (i < ACH ? i : 0), rb = n0 + crow + RSTEP * (i < BCH ? i : 0);
    xrow[i] = X + (size_t)(ra < M ? ra : M - 1) * K + ckc;
    wrow[i] = W + (size_t)(rb < N ? rb : N - 1) * K + ckc;
  }
#define SS_LD(p) (*reinterpret_cast<const u32x4 *>(p))
#define SS_LOAD(S, T)                                                                                                          \
  {                                                                                                                            \
    const int ko_ = ((T) < nkt ? (T) : nkt - 1) * BK;                                                                          \
    S.a0 = SS_LD(xrow[0] + ko_); if (ACH > 1) S.a1 = SS_LD(xrow[1] + ko_); if (ACH > 2) S.a2 = SS_LD(xrow[2] + ko_); if (ACH > 3) S.a3 = SS_LD(xrow[3] + ko_); \
    S.b0 = SS_LD(wrow[0] + ko_); if (BCH > 1) S.b1 = SS_LD(wrow[1] + ko_); if (BCH > 2) S.b2 = SS_LD(wrow[2] + ko_); if (BCH > 3) S.b3 = SS_LD(wrow[3] + ko_); \
  }
#define SS_ST(base, i, v) (*reinterpret_cast<u32x4 *>(&base[soff0 + RSTEP * (i) * LDS_STRIDE]) = (v))
#define SS_STORE(S, BUF)                                                                                                       \
  {                                                                                                                            \
    SS_ST(As[BUF], 0, S.a0); if (ACH > 1) SS_ST(As[BUF], 1, S.a1); if (ACH > 2) SS_ST(As[BUF], 2, S.a2); if (ACH > 3) SS_ST(As[BUF], 3, S.a3); \
    SS_ST(Bs[BUF], 0, S.b0); if (BCH > 1) SS_ST(Bs[BUF], 1, S.b1); if (BCH > 2) SS_ST(Bs[BUF], 2, S.b2); if (BCH > 3) SS_ST(Bs[BUF], 3, S.b3); \
  }
#define SS_COMPUTE(BUF)                                                                                                        \
  _Pragma("unroll") for (int k16 = 0; k16 < BK; k16 += 16) {                                                                   \
    const int ko_ = k16 + 8 * (lane >> 5);                                                                                     \
    bf16x8 a[TM], b[TN];                                                                                                       \
    _Pragma("unroll") for (int tm = 0; tm < TM; tm++) a[tm] = *reinterpret_cast<const bf16x8 *>(&As[BUF][(wm * (32 * TM) + tm * 32 + (lane & 31)) * LDS_STRIDE + ko_]); \
    _Pragma("unroll") for (int tn = 0; tn < TN; tn++) b[tn] = *reinterpret_cast<const bf16x8 *>(&Bs[BUF][(wn * (BN / WN) + tn * 32 + (lane & 31)) * LDS_STRIDE + ko_]); \
    _Pragma("unroll") for (int tm = 0; tm < TM; tm++)                                                                          \
      _Pragma("unroll") for (int tn = 0; tn < TN; tn++) acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[tm], b[tn], acc[tm][tn], 0, 0, 0); \
  }
  SS_LOAD(s0, 0)
  SS_STORE(s0, 0)
  SS_LOAD(s1, 1)
  __syncthreads();
  for (int kt = 0; kt < nkt; kt += 2) {
    SS_LOAD(s0, kt + 2)                                       // tile kt + 2 -> stage 0 (in flight for two steps)
    SS_COMPUTE(0)                                            // tile kt
    SS_STORE(s1, 1)                                           // tile kt + 1 (requested a step ago) -> the other LDS buffer
    __syncthreads();
    SS_LOAD(s1, kt + 3)                                       // (past the end the loads re-read the last tile: unconditional)
    if (kt + 1 < nkt) { SS_COMPUTE(1) }
    SS_STORE(s0, 0)
    __syncthreads();
  }
#undef SS_LD
#undef SS_ST
#undef SS_LOAD
#undef SS_STORE
#undef SS_COMPUTE
  // epilogue: bias + activation (chosen once), bf16 (the next layer's operand; staged through LDS so that a lane stores 16 contiguous
  // bytes of a row) or f32 (the head: a few columns, stored directly)
  float bv[TN];
#pragma unroll
  for (int tn = 0; tn < TN; tn++) {
    const int col = n0 + wn * (BN / WN) + tn * 32 + (lane & 31);
    bv[tn] = (bias && col < N) ? bias[col] : 0.f;
  }
  if constexpr (F32OUT) {
    with_activation(act, [&](auto fn) {
#pragma unroll
      for (int tm = 0; tm < TM; tm++)
#pragma unroll
        for (int tn = 0; tn < TN; tn++) {
          const int col = n0 + wn * (BN / WN) + tn * 32 + (lane & 31);
#pragma unroll
          for (int r = 0; r < 16; r++) {
            const int row = c_row(m0 + wm * (32 * TM) + tm * 32, r, lane);
            if (row < M && col < N) reinterpret_cast<float *>(Y)[(size_t)row * ldy + col] = fn(acc[tm][tn][r] + bv[tn]);
          }
        }
    });
  } else {
    constexpr int CS = BN + 8;
    __bf16 *Cs = lds_ab;                                       // (the K loop ended with a barrier: its buffers are free)
    with_activation(act, [&](auto fn) {
#pragma unroll
      for (int tm = 0; tm < TM; tm++)
#pragma unroll
        for (int tn = 0; tn < TN; tn++) {
          const int cl = wn * (BN / WN) + tn * 32 + (lane & 31);
#pragma unroll
          for (int r = 0; r < 16; r++) Cs[c_row(wm * (32 * TM) + tm * 32, r, lane) * CS + cl] = (__bf16)fn(acc[tm][tn][r] + bv[tn]);
        }
    });
    __syncthreads();
    store_tile_rows<BN, NT>(Cs, reinterpret_cast<__bf16 *>(Y), ldy, m0, n0, M, N, tid);
  }
}

// ---- round 5: the same GEMM with asynchronous global -> LDS copies (global_load_lds_dwordx4) and three K tiles in flight.
// What round 4 measured (profiles/r04_mlp_gemm.txt): the register-staged K loop above is a chain global load -> LDS store -> barrier ->
// fragment read that one workgroup per CU cannot hide.  Here a tile goes from global memory straight into LDS (no staging registers,
// no ds_write pass), is requested two K steps before it is multiplied, and one barrier per K step remains:
//     wait until tile t has landed (s_waitcnt vmcnt(loads of tile t + 1)) -> barrier -> request tile t + 2 -> multiply tile t
// (the barrier proves that every wave has finished multiplying tile t - 1, whose LDS stage tile t + 2 overwrites).
// LDS layout: a tile row is 64 bf16 = eight 16-byte chunks, rows dense (the copy writes wave-base + lane * 16: 8 rows of 8 chunks per
// wave instruction, no padding possible); chunk c of row r sits at position c ^ ((r >> 1) & 7) — two rows fill the 64 banks, so the 16
// rows a quarter of a fragment read touches need 8 distinct positions per row parity — the XOR is applied to the per-lane SOURCE
// address of the copy (within the row's one 128-byte line) and to the fragment reads' addresses, so that the 32 rows a fragment
// read touches spread over all banks (a ds_read_b128 of 64 lanes takes its four cycles, no more).
// The loop is shared by ss_linear_glds_kernel (kt0 = 0) and ss_linear_train_kernel (kt0 = the first K tile of the workgroup's share).
template <int BN> struct GldsLoop {
  static constexpr int BK = 64, WM = 4, WN = 2, NST = 3;
  static constexpr int TN = BN / (32 * WN);                  // MFMA tiles per wave along N (a wave owns 32 x BN/2 of the 128 x BN tile)
  static constexpr int STAGE = (BM + BN) * BK;               // bf16 elements of one stage: A rows, then B rows
  static constexpr int NI = (BM + BN) / 64;                  // copy instructions per wave and tile (8 rows each, 8 waves)
  const __bf16 *src[NI];
  int dst[NI];
  __bf16 *lds;
  int tid, lane, wave, wm, wn, kt0;

  __device__ __forceinline__ void init(const __bf16 *__restrict__ X, const __bf16 *__restrict__ W, int M, int N, int K, int m0, int n0, int kt0_, __bf16 *lds_) {
    lds = lds_; kt0 = kt0_;
    tid = threadIdx.x; lane = tid & 63; wave = __builtin_amdgcn_readfirstlane(tid >> 6); wm = wave / WN; wn = wave % WN;
    // this wave's copy instructions: instruction i covers tile rows 8 (wave + 8 i) .. + 8 of the stacked (A | B) tile; lane -> row
    // lane / 8, chunk position lane % 8, source chunk (lane % 8) ^ (lane / 8)
#pragma unroll
    for (int i = 0; i < NI; i++) {
      const int blk = wave + 8 * i, row = 8 * blk + (lane >> 3), chunk = (lane & 7) ^ ((row >> 1) & 7);
      if (row < BM) { const int g = m0 + row; src[i] = X + (size_t)(g < M ? g : M - 1) * K + chunk * 8; }
      else { const int g = n0 + row - BM; src[i] = W + (size_t)(g < N ? g : N - 1) * K + chunk * 8; }
      dst[i] = 8 * blk * BK;                                   // wave-uniform; the lane's 16 bytes follow at lane * 16
    }
  }

  __device__ __forceinline__ void request(int t) {
    __bf16 *stage = lds + (t % NST) * STAGE;
#pragma unroll
    for (int i = 0; i < NI; i++) __builtin_amdgcn_global_load_lds((gvoid *)(src[i] + (size_t)(kt0 + t) * BK), (lvoid *)(stage + dst[i]), 16, 0, 0);
  }

  // nkt >= 1 K tiles from kt0 on; on return no copy is in flight, but other waves may still be multiplying the last tile
  __device__ __forceinline__ void run(f32x16 (&acc)[TN], int nkt) {
    request(0);
    if (nkt > 1) request(1);
    const int arow = wm * 32 + (lane & 31), ax = (arow >> 1) & 7, half = lane >> 5;
    for (int kt = 0; kt < nkt; kt++) {
      if (kt + 1 < nkt) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NI) : "memory");   // tile kt landed (tile kt + 1 may still be on its way)
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();                             // ... for every wave's share of it, and tile kt - 1 is multiplied everywhere
      if (kt + 2 < nkt) request(kt + 2);
      const __bf16 *As = lds + (kt % NST) * STAGE, *Bs = As + BM * BK;
      // fragments of k16 step ks + 1 are requested before step ks is multiplied (two register sets): the LDS latency of a step hides
      // behind the previous step's MFMAs instead of in front of its own
      bf16x8 fa[2], fb[2][TN];
      auto frags = [&](int ks, int set) {
        const int c = 2 * ks + half;                           // this lane's chunk of the k16 step: k = 16 ks + 8 (lane / 32) ..
        fa[set] = *reinterpret_cast<const bf16x8 *>(As + arow * BK + ((c ^ ax) << 3));
#pragma unroll
        for (int tn = 0; tn < TN; tn++) {
          const int brow = wn * (BN / WN) + tn * 32 + (lane & 31);
          fb[set][tn] = *reinterpret_cast<const bf16x8 *>(Bs + brow * BK + ((c ^ ((brow >> 1) & 7)) << 3));
        }
      };
      frags(0, 0);
#pragma unroll
      for (int ks = 0; ks < 4; ks++) {
        if (ks < 3) frags(ks + 1, (ks + 1) & 1);
        __builtin_amdgcn_sched_barrier(0);                      // (the scheduler would sink the reads back in front of their own MFMAs)
#pragma unroll
        for (int tn = 0; tn < TN; tn++) acc[tn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[ks & 1], fb[ks & 1][tn], acc[tn], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }
  // (Round 5 also built the deeper pipeline — a whole tile's fragments of tile t + 1 read during tile t's MFMAs, three tiles in flight,
  // the copy instructions spread behind the MFMAs: correct, and not faster (35.1-35.5 us against 34.6 on the 2048 -> 1536 layer).  With
  // the K loop's copies removed the same loop runs 28.3 us: what is left is the L2 -> LDS traffic itself, 335 MB per GEMM at 128 x 192
  // tiles = ~12 TB/s over the eight L2s; fewer bytes per flop need 256-wide tiles, of which this layer has 96-128 for 256 CUs.
  // profiles/r05_mlp_gemm.txt)
};

template <int BN, bool F32OUT>
__global__ void __launch_bounds__(512) ss_linear_glds_kernel(const __bf16 *__restrict__ X, const __bf16 *__restrict__ W, const float *__restrict__ bias,
                                                             void *__restrict__ Y, int M, int N, int K, int ldy, int act, int xcd_remap) {
  constexpr int WN = 2, TN = GldsLoop<BN>::TN;
  extern __shared__ __attribute__((aligned(16))) __bf16 lds_g[];
  int bx = blockIdx.x, by = blockIdx.y;
  xcd_tile(bx, by, xcd_remap);
  const int m0 = by * BM, n0 = bx * BN;
  f32x16 acc[TN];
#pragma unroll
  for (int j = 0; j < TN; j++)
#pragma unroll
    for (int r = 0; r < 16; r++) acc[j][r] = 0.f;
  GldsLoop<BN> L;
  L.init(X, W, M, N, K, m0, n0, 0, lds_g);
  L.run(acc, K / 64);
  const int tid = L.tid, lane = L.lane, wm = L.wm, wn = L.wn;
  // ---- epilogue: bias + activation, then the tile goes through LDS (the stages are free) so that every lane stores 16 contiguous
  // bytes of an output row (the MFMA's C layout puts one column per lane: 2-byte stores, 48 store instructions per wave before)
  float bv[TN];
#pragma unroll
  for (int tn = 0; tn < TN; tn++) {
    const int col = n0 + wn * (BN / WN) + tn * 32 + (lane & 31);
    bv[tn] = (bias && col < N) ? bias[col] : 0.f;
  }
  if constexpr (F32OUT) {
    with_activation(act, [&](auto fn) {
#pragma unroll
      for (int tn = 0; tn < TN; tn++) {
        const int col = n0 + wn * (BN / WN) + tn * 32 + (lane & 31);
#pragma unroll
        for (int r = 0; r < 16; r++) {
          const int row = c_row(m0 + wm * 32, r, lane);
          if (row < M && col < N) reinterpret_cast<float *>(Y)[(size_t)row * ldy + col] = fn(acc[tn][r] + bv[tn]);
        }
      }
    });
  } else {
    constexpr int CS = BN + 8;                               // row stride of the staged tile (16 bytes of padding: the column-per-lane writes spread over the banks)
    __bf16 *Cs = lds_g;
    __builtin_amdgcn_s_barrier();                             // every wave has multiplied the last tile: the stages may be overwritten
    with_activation(act, [&](auto fn) {
#pragma unroll
      for (int tn = 0; tn < TN; tn++) {
        const int cl = wn * (BN / WN) + tn * 32 + (lane & 31);
#pragma unroll
        for (int r = 0; r < 16; r++) Cs[c_row(wm * 32, r, lane) * CS + cl] = (__bf16)fn(acc[tn][r] + bv[tn]);
      }
    });
    __syncthreads();
    store_tile_rows<BN, 512>(Cs, reinterpret_cast<__bf16 *>(Y), ldy, m0, n0, M, N, tid);
  }
}

// ---- round 6: the GEMM of the PPO update (reference agent_ppo.py:20-83 runs the same three products per layer through
// autograd).  The asynchronous-copy K loop of ss_linear_glds_kernel with (a) a K split over blockIdx.z for products whose output is small and whose
// contraction is the batch (dW = dZ^T h: 2048 x 1536 outputs over K = 53248 rows), partial sums added to the fp32 output by hardware atomics;
// (b) an epilogue that multiplies by a second operand (the stored activation derivative: dZ = (dZ' W) * act'(z)) and / or applies the activation;
// (c) up to three bf16 outputs of the same tile staged through LDS at once: the result, its TRANSPOSE (every product of the backward pass
// contracts over what the forward pass has as rows: with h^T and dZ^T written here, all three products of a layer are the one K-contiguous
// "x W^T" kernel — no transposing loads, no separate transpose launches), and the activation's derivative at the pre-activation.
// Arguments: LinearTrainArgs (ss_gemm256.h).
template <int BN, bool F32ATOMIC>
__global__ void __launch_bounds__(512) ss_linear_train_kernel(const LinearTrainArgs a) {
  constexpr int WN = 2, TN = GldsLoop<BN>::TN;
  extern __shared__ __attribute__((aligned(16))) __bf16 lds_g[];
  const int M = a.M, N = a.N, K = a.K;
  int bx = blockIdx.x, by = blockIdx.y;
  xcd_tile(bx, by, a.xcd_remap);
  const int m0 = by * BM, n0 = bx * BN;
  f32x16 acc[TN];
#pragma unroll
  for (int j = 0; j < TN; j++)
#pragma unroll
    for (int r = 0; r < 16; r++) acc[j][r] = 0.f;
  // this workgroup's share of the K tiles (the host's kper, as in ss_gemm256_kernel; 0: the whole of K)
  const int nkt_all = K / 64, per = a.kper > 0 ? a.kper : nkt_all, kt0 = (int)blockIdx.z * per, kt1 = kt0 + per < nkt_all ? kt0 + per : nkt_all;
  const int nkt = kt1 - kt0;
  if (nkt <= 0) return;
  GldsLoop<BN> L;
  L.init(a.X, a.W, M, N, K, m0, n0, kt0, lds_g);
  L.run(acc, nkt);
  const int tid = L.tid, lane = L.lane, wm = L.wm, wn = L.wn;
  if constexpr (F32ATOMIC) {
    // partial sums of this K share: hardware fp32 atomics, 32 adjacent columns per wave instruction (the bias, if any, is added by share 0)
    float *Yf = reinterpret_cast<float *>(a.Y);
#pragma unroll
    for (int tn = 0; tn < TN; tn++) {
      const int col = n0 + wn * (BN / WN) + tn * 32 + (lane & 31);
      const float bv = (a.bias && col < N && blockIdx.z == 0) ? a.bias[col] : 0.f;
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int row = c_row(m0 + wm * 32, r, lane);
        if (row < M && col < N) unsafeAtomicAdd(Yf + (size_t)row * a.ldy + col, acc[tn][r] + bv);
      }
    }
  } else {
    // up to three bf16 images of the tile, one after the other through the same LDS (rows | derivative rows | transposed): each pass
    // re-evaluates the epilogue arithmetic from the accumulators (~10 instructions per element against a K loop of thousands of cycles)
    constexpr int CS = BN + 8, CST = BM + 8;
    __bf16 *Cs = lds_g;
    const bool want_d = a.Dact != nullptr, want_t = a.Yt != nullptr;
    auto value = [&](int tn, int r, float &v) {              // bias, multiplying operand; returns through v the pre-activation
      const int cl = wn * (BN / WN) + tn * 32 + (lane & 31), col = n0 + cl;
      const int rl = c_row(wm * 32, r, lane), row = m0 + rl;
      v = acc[tn][r] + ((a.bias && col < N) ? a.bias[col] : 0.f);
      if (a.mul) v *= (row < M && col < N) ? (float)a.mul[(size_t)row * a.ldy + col] : 0.f;
    };
    // the multiplying operand is read once: fold it (and the bias) into the accumulators
#pragma unroll
    for (int tn = 0; tn < TN; tn++)
#pragma unroll
      for (int r = 0; r < 16; r++) { float v; value(tn, r, v); acc[tn][r] = v; }
    if (a.Y) {
      __builtin_amdgcn_s_barrier();
      with_activation(a.act, [&](auto fn) {
#pragma unroll
        for (int tn = 0; tn < TN; tn++)
#pragma unroll
          for (int r = 0; r < 16; r++)
            Cs[c_row(wm * 32, r, lane) * CS + wn * (BN / WN) + tn * 32 + (lane & 31)] = (__bf16)fn(acc[tn][r]);
      });
      __syncthreads();
      store_tile_rows<BN, 512>(Cs, reinterpret_cast<__bf16 *>(a.Y), a.ldy, m0, n0, M, N, tid);
    }
    if (want_d) {
      __syncthreads();
#pragma unroll
      for (int tn = 0; tn < TN; tn++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
          const float v = acc[tn][r];
          float d = 1.f;
          if (a.act == SS_ACT_SILU) { const float sg = __builtin_amdgcn_rcpf(1.f + __expf(-v)); d = sg * (1.f + v * (1.f - sg)); }
          else if (a.act == SS_ACT_TANH) { const float e = __expf(-2.f * fabsf(v)); const float t = (1.f - e) * __builtin_amdgcn_rcpf(1.f + e); d = 1.f - t * t; }
          else if (a.act == SS_ACT_RELU) d = v > 0.f ? 1.f : 0.f;
          Cs[c_row(wm * 32, r, lane) * CS + wn * (BN / WN) + tn * 32 + (lane & 31)] = (__bf16)d;
        }
      __syncthreads();
      store_tile_rows<BN, 512>(Cs, a.Dact, a.ldy, m0, n0, M, N, tid);
    }
    if (want_t) {
      __bf16 *Ct = lds_g;
      __syncthreads();
      with_activation(a.act, [&](auto fn) {
#pragma unroll
        for (int tn = 0; tn < TN; tn++)
#pragma unroll
          for (int r = 0; r < 16; r++)
            Ct[(wn * (BN / WN) + tn * 32 + (lane & 31)) * CST + c_row(wm * 32, r, lane)] = (__bf16)fn(acc[tn][r]);
      });
      __syncthreads();
      constexpr int RPC = BM / 8;                             // 16-byte chunks per transposed tile row (a column of the result: 128 rows)
      const bool vec_ok = (a.ldyt & 7) == 0 && (reinterpret_cast<size_t>(a.Yt) & 15) == 0;
#pragma unroll
      for (int i = 0; i < BN * RPC / 512; i++) {
        const int id = tid + 512 * i, cl = id / RPC, rc = (id % RPC) * 8, col = n0 + cl, row = m0 + rc;
        if (col >= N || row >= M) continue;
        const u32x4 v = *reinterpret_cast<const u32x4 *>(Ct + cl * CST + rc);
        if (vec_ok && row + 8 <= M) *reinterpret_cast<u32x4 *>(a.Yt + (size_t)col * a.ldyt + row) = v;
        else store_chunk_edge(a.Yt + (size_t)col * a.ldyt + row, v, M - row);
      }
    }
  }
}

}  // namespace gemm128
