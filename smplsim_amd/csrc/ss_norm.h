// ss_norm.h — RunningNorm.update on the device (include/smplsim_mlp.h: ss_running_norm_update): the biased column statistics of a batch [M, dim] merged into the
// running mean / var / std / n of learning/networks.py (the reference's running_norm.py:22-29), in two launches instead of torch's var_mean plus about eight small
// launches for the merge.
//
// By bytes this is one read of the batch (M * dim * 4) and nothing else of any size, so every value is formed in fp64 from the fp32 inputs and rounded to fp32 ONCE
// when it is stored, as in ss_ppo_head.h and ss_optim.h.  Reproducible by construction: no atomics.  A thread adds its rows in ascending order, a workgroup adds its
// four wavefronts ascending and STORES one (mean, M2) pair per column; the second launch folds the pairs ascending from block 0 (Chan's pairwise update) and applies
// the running merge.
#ifndef SS_NORM_H
#define SS_NORM_H
#include <hip/hip_runtime.h>

#include "../../include/smplsim_mlp.h"

namespace run_norm {

constexpr int BLOCK_ROWS = SS_NORM_BLOCK_ROWS;   // rows per workgroup of the partials launch = per (mean, M2) pair
constexpr int WAVES = 4;
constexpr int WAVE_ROWS = BLOCK_ROWS / WAVES;    // consecutive rows of one wavefront
constexpr int COLS = 64;                         // columns per workgroup: one per lane, so that a row's loads coalesce
constexpr int UNROLL = 8;                        // loads issued together; only the additions form a chain
static_assert(BLOCK_ROWS % WAVES == 0 && WAVE_ROWS % UNROLL == 0, "a wavefront's rows in whole groups of loads");

// Workgroup (b, g): rows [b * BLOCK_ROWS, min((b + 1) * BLOCK_ROWS, M)), columns 64 g .. 64 g + 63.  Lane l of wavefront w owns column 64 g + l and the rows
// b * BLOCK_ROWS + WAVE_ROWS * w .. + WAVE_ROWS - 1 (those below M); it adds d = x - K and d * d over them in ascending row order, in fp64, K being the block's first
// row in that column (no division per element; a constant column has d = 0 in every row, hence M2 = 0 and mean = K exactly).  The four wavefronts meet as
// ((w0 + w1) + w2) + w3, then   mean = K + S1 / rows,   M2 = S2 - S1 * S1 / rows   (a negative M2, which only rounding can produce, stored as 0; a NaN stays one).
__global__ void __launch_bounds__(256) ss_norm_partials_kernel(const float *__restrict__ x, int M, int dim, int ldx, int col_groups, double *__restrict__ part) {
  const int b = (int)(blockIdx.x / (unsigned)col_groups), g = (int)(blockIdx.x % (unsigned)col_groups);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int c = g * COLS + lane;
  const long long first = (long long)b * BLOCK_ROWS;                      // in 64 bits: the last block's end may pass INT32_MAX
  const int rows = (int)min((long long)BLOCK_ROWS, (long long)M - first);
  const int r0 = min(wave * WAVE_ROWS, rows), r1 = min(r0 + WAVE_ROWS, rows);
  double s1 = 0.0, s2 = 0.0, K = 0.0;
  if (c < dim) {
    const float *col = x + (size_t)first * ldx + c;
    K = (double)col[0];
    int r = r0;
    for (; r + UNROLL <= r1; r += UNROLL) {
      float v[UNROLL];
#pragma unroll
      for (int j = 0; j < UNROLL; j++) v[j] = col[(size_t)(r + j) * ldx];
#pragma unroll
      for (int j = 0; j < UNROLL; j++) {
        const double d = (double)v[j] - K;
        s1 += d;
        s2 += d * d;
      }
    }
    for (; r < r1; r++) {
      const double d = (double)col[(size_t)r * ldx] - K;
      s1 += d;
      s2 += d * d;
    }
  }
  __shared__ double sh[WAVES][2][COLS];
  sh[wave][0][lane] = s1;
  sh[wave][1][lane] = s2;
  __syncthreads();
  if (wave == 0 && c < dim) {
    const double S1 = ((sh[0][0][lane] + sh[1][0][lane]) + sh[2][0][lane]) + sh[3][0][lane];
    const double S2 = ((sh[0][1][lane] + sh[1][1][lane]) + sh[2][1][lane]) + sh[3][1][lane];
    const double m2 = S2 - S1 * S1 / (double)rows;
    double2 out;
    out.x = K + S1 / (double)rows;
    out.y = m2 < 0.0 ? 0.0 : m2;                                          // (not fmax: a NaN must stay one)
    reinterpret_cast<double2 *>(part)[(size_t)b * dim + c] = out;
  }
}

// One workgroup; thread t owns the columns t, t + 256, ...  Per column the P blocks are folded ascending from block 0 (a = what is folded so far, b = the next block,
// n_a and n_b their row counts):   f = n_b / (n_a + n_b);  delta = mean_b - mean_a;  mean_a += delta * f;  M2_a += M2_b + delta * delta * (n_a * f).
// Then bm = mean_a, bv = M2_a / M and the running merge of RunningNorm.update with w = n / (n + M).  Every thread reads *n before the barrier, thread 0 stores it after.
__global__ void __launch_bounds__(256) ss_norm_merge_kernel(const double *__restrict__ part, int P, int M, int dim, float *__restrict__ mean, float *__restrict__ var,
                                                            float *__restrict__ sd, long long *n) {
  const long long n_old = *n;
  const double w = (double)n_old / (double)(n_old + M), w_new = 1.0 - w;
  const double2 *p2 = reinterpret_cast<const double2 *>(part);
  for (int c = threadIdx.x; c < dim; c += 256) {
    const double2 *p = p2 + c;
    double2 acc = p[0];
    double n_a = (double)min(BLOCK_ROWS, M);
    int s = 1;
    for (; s + UNROLL <= P; s += UNROLL) {
      double2 v[UNROLL];
#pragma unroll
      for (int j = 0; j < UNROLL; j++) v[j] = p[(size_t)(s + j) * dim];
#pragma unroll
      for (int j = 0; j < UNROLL; j++) {
        const double n_b = (double)min((long long)BLOCK_ROWS, (long long)M - (long long)(s + j) * BLOCK_ROWS);
        const double f = n_b / (n_a + n_b), delta = v[j].x - acc.x;
        acc.x += delta * f;
        acc.y += v[j].y + delta * delta * (n_a * f);
        n_a += n_b;
      }
    }
    for (; s < P; s++) {
      const double2 v = p[(size_t)s * dim];
      const double n_b = (double)min((long long)BLOCK_ROWS, (long long)M - (long long)s * BLOCK_ROWS);
      const double f = n_b / (n_a + n_b), delta = v.x - acc.x;
      acc.x += delta * f;
      acc.y += v.y + delta * delta * (n_a * f);
      n_a += n_b;
    }
    const double bm = acc.x, bv = acc.y / (double)M;
    const double m_old = (double)mean[c], shift = bm - m_old;
    const float v_new = (float)(w * (double)var[c] + w_new * bv + w * w_new * shift * shift);
    var[c] = v_new;
    mean[c] = (float)(w * m_old + w_new * bm);
    sd[c] = (float)sqrt((double)v_new);                                   // of the STORED variance: a checkpoint's std is var.sqrt() to 1 ulp
  }
  __syncthreads();
  if (threadIdx.x == 0) *n = n_old + M;
}

}  // namespace run_norm
#endif
