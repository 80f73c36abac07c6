// ss_ppo_head.h — the PPO update's loss heads (include/smplsim_mlp.h: ss_ppo_policy_head, ss_value_head): the step between the networks' forward passes and
// their backward products — log-density, clipped surrogate and its gradient with respect to the Gaussian head's mean and log-std; the critic's MSE and
// its gradient — in two launches each instead of ~15 torch launches forward and as many through autograd (agents/agent_ppo.py:20-83).
//
// By bytes both are small (the policy head reads mean and actions and writes dmean: 3 * M * dim * 4 bytes), so every per-element and per-row value is
// formed in fp64 from the fp32 inputs and rounded to fp32 ONCE when it is stored: the results are the correctly rounded ones up to the last few ulps
// of fp64, whatever the order of the sums.  What that costs is not derived here: a row's chain (the loads, six fp64 shuffle steps, one software fp64
// exp, the stores) is serial and a wavefront walks its 32 rows one after the other, so the chain rather than the bytes may well set the kernel's time.
// profiles/ppo_head.txt holds what was measured.
//
// Reproducible by construction: no atomics.  A row's sum is formed inside one wavefront (lane-local over the column trips, ascending; then the xor
// butterfly 32, 16, ..., 1: every lane ends with the same bits); a wavefront adds its rows in ascending row order; a workgroup adds its four
// wavefronts ascending and STORES one partial row; a second launch adds the partial rows ascending from partial 0.
#ifndef SS_PPO_HEAD_H
#define SS_PPO_HEAD_H
#include <hip/hip_runtime.h>

namespace ppo_head {

// Four column trips of a wavefront, their per-column state (inv_std, cst, dls, z: fp64) in registers.  The widest head in use has 69 columns (two trips)
// and the tests go to 130 (three); four was taken as the next round figure.  A trip beyond the row's width costs its registers and LDS only: its
// loads, arithmetic and stores are skipped by wave-uniform branches.
constexpr int MAX_DIM = 256;
constexpr int TRIPS = MAX_DIM / 64;
constexpr int POLICY_ROWS = 128;         // rows per workgroup of the policy head = per partial row: 4 wavefronts x 32 consecutive rows
constexpr int WAVE_ROWS = POLICY_ROWS / 4;
constexpr int VALUE_ROWS = 1024;         // rows per workgroup of the value head = per partial: 256 threads x 4 rows
constexpr int NSTATS = 4;                // loss, clip_frac, approx_kl, mean_ratio
constexpr double LOG_SQRT_2PI = 0.91893853320467274178;

// torch.clamp semantics: a NaN stays a NaN
__device__ __forceinline__ double clamp_keep_nan(double v, double lo, double hi) { return v != v ? v : fmin(fmax(v, lo), hi); }

__device__ __forceinline__ double wave_sum(double v) {
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

template <bool BF16> __device__ __forceinline__ void store_grad(void *out, size_t idx, double v) {
  const float f = (float)v;              // the fp32 result; the bf16 form is its round-to-nearest-even
  if (!BF16) { static_cast<float *>(out)[idx] = f; return; }
  // Rounded on the fp32 bits.  (__bf16)(float)v is not that: the compiler merges the two conversions into one rounding of the fp64 value, which differs
  // from the rounded fp32 value wherever that one lies exactly between two bf16 values (about one element in 2^17).
  const unsigned u = __float_as_uint(f);
  const unsigned r = f != f ? (u >> 16) | 0x40u : (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;   // a NaN stays one (quiet, sign kept); else ties to even
  static_cast<unsigned short *>(out)[idx] = (unsigned short)r;
}

struct PolicyHeadArgs {
  const float *mean, *actions, *log_std, *adv, *old_logp;
  float *logp;
  void *dmean;
  double *part;                          // [ceil(M / POLICY_ROWS), NSTATS + dim]
  int M, dim, ldm, lda, ldd;
  double lo, hi, inv_m;                  // the clip bounds 1 -+ clip_eps, 1 / M
};

struct RowIn { float a[TRIPS], m[TRIPS], adv, old; };

__device__ __forceinline__ RowIn load_row(const PolicyHeadArgs &p, int row, int lane) {
  RowIn r;
#pragma unroll
  for (int t = 0; t < TRIPS; t++) {
    const int j = lane + 64 * t;
    const bool in = j < p.dim;
    r.a[t] = in ? p.actions[(size_t)row * p.lda + j] : 0.f;
    r.m[t] = in ? p.mean[(size_t)row * p.ldm + j] : 0.f;
  }
  r.adv = p.adv[row];
  r.old = p.old_logp[row];
  return r;
}

// One wavefront per row, 32 consecutive rows per wavefront (the next row's loads are issued before the current row's arithmetic).  dim = 69 makes the second
// column trip mostly idle, as in ss_gaussian_sample_kernel; the trips beyond the row's width are skipped by a wave-uniform branch.
template <bool BF16> __global__ void __launch_bounds__(256) ss_ppo_policy_head_kernel(const PolicyHeadArgs p) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long first = (long long)blockIdx.x * POLICY_ROWS + wave * WAVE_ROWS;      // in 64 bits: the last workgroup's may pass INT32_MAX
  const int r0 = (int)min(first, (long long)p.M), r1 = (int)min(first + WAVE_ROWS, (long long)p.M);
  double inv_std[TRIPS], cst[TRIPS], dls[TRIPS];
#pragma unroll
  for (int t = 0; t < TRIPS; t++) {
    const int j = lane + 64 * t;
    const double ls = j < p.dim ? (double)p.log_std[j] : 0.0;
    inv_std[t] = exp(-ls);
    cst[t] = -ls - LOG_SQRT_2PI;
    dls[t] = 0.0;
  }
  double s_min = 0.0, s_clip = 0.0, s_kl = 0.0, s_ratio = 0.0;
  RowIn cur;
  if (r0 < r1) cur = load_row(p, r0, lane);
  for (int row = r0; row < r1; row++) {
    RowIn next = cur;
    if (row + 1 < r1) next = load_row(p, row + 1, lane);
    double z[TRIPS], acc = 0.0;
#pragma unroll
    for (int t = 0; t < TRIPS; t++) {
      z[t] = 0.0;
      if (64 * t < p.dim && lane + 64 * t < p.dim) {
        z[t] = ((double)cur.a[t] - (double)cur.m[t]) * inv_std[t];
        acc += -0.5 * z[t] * z[t] + cst[t];
      }
    }
    const double logp = wave_sum(acc);
    const double ratio = exp(logp - (double)cur.old), A = (double)cur.adv;
    const double s1 = ratio * A, s2 = clamp_keep_nan(ratio, p.lo, p.hi) * A;
    // torch.minimum semantics: a NaN on either side is the result (fmin would return the other side)
    const double surr = (s1 != s1 || s2 != s2) ? s1 + s2 : fmin(s1, s2);
    // dloss / dlogp: the unclipped branch carries the gradient wherever it is the minimum, ties included (autograd of torch.minimum over clamp)
    const double g = -p.inv_m * ratio * (s1 <= s2 ? A : 0.0);
    s_min += surr;
    s_clip += (ratio < p.lo || ratio > p.hi) ? 1.0 : 0.0;
    s_kl += (double)cur.old - logp;
    s_ratio += ratio;
    if (p.logp && lane == 0) p.logp[row] = (float)logp;
#pragma unroll
    for (int t = 0; t < TRIPS; t++)
      if (64 * t < p.dim && lane + 64 * t < p.dim) {
        store_grad<BF16>(p.dmean, (size_t)row * p.ldd + lane + 64 * t, g * z[t] * inv_std[t]);
        dls[t] += g * (z[t] * z[t] - 1.0);
      }
    cur = next;
  }
  // the workgroup's partial row: wavefronts 0..3 added in that order (a wavefront without rows contributes zeros)
  __shared__ double sh[4][NSTATS + MAX_DIM];
  if (lane == 0) { sh[wave][0] = s_min; sh[wave][1] = s_clip; sh[wave][2] = s_kl; sh[wave][3] = s_ratio; }
#pragma unroll
  for (int t = 0; t < TRIPS; t++)
    if (64 * t < p.dim) sh[wave][NSTATS + lane + 64 * t] = dls[t];
  __syncthreads();
  const int W = NSTATS + p.dim;
  for (int c = threadIdx.x; c < W; c += 256)
    p.part[(size_t)blockIdx.x * W + c] = ((sh[0][c] + sh[1][c]) + sh[2][c]) + sh[3][c];
}

// Thread t of workgroup b owns rows 1024 b + t + 256 k, k = 0..3 (coalesced), and adds their squares in that order; then the butterfly; then the four wavefronts.
template <bool BF16> __global__ void __launch_bounds__(256) ss_value_head_kernel(const float *__restrict__ pred, const float *__restrict__ target, int M, void *dpred,
                                                                                 int ldd, double *__restrict__ part, double inv_m) {
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < VALUE_ROWS / 256; k++) {
    const long long i = (long long)blockIdx.x * VALUE_ROWS + k * 256 + threadIdx.x;
    if (i < M) {
      const double d = (double)pred[i] - (double)target[i];
      store_grad<BF16>(dpred, (size_t)i * ldd, 2.0 * d * inv_m);
      acc += d * d;
    }
  }
  acc = wave_sum(acc);
  __shared__ double sh[4];
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// Second launch of both heads: column c of the P partial rows (W doubles each) added ascending from row 0 in fp64, one thread per column; the loads of eight
// rows are issued together and only the additions form a chain.  Columns below nstats are divided by the batch size m (column 0 negated for the surrogate: sign0 = -1)
// and go to stats, the others are sums as they are and go to tail (when given).  Every output is overwritten.
__global__ void __launch_bounds__(64) ss_head_reduce_kernel(const double *__restrict__ part, int P, int W, float *__restrict__ stats, int nstats, float *__restrict__ tail,
                                                            double m, double sign0) {
  const int c = (int)blockIdx.x * 64 + threadIdx.x;
  if (c >= W) return;
  const double *p = part + c;
  double sum = p[0];
  int s = 1;
  for (; s + 8 <= P; s += 8) {
    double v[8];
#pragma unroll
    for (int j = 0; j < 8; j++) v[j] = p[(size_t)(s + j) * W];
#pragma unroll
    for (int j = 0; j < 8; j++) sum += v[j];
  }
  for (; s < P; s++) sum += p[(size_t)s * W];
  if (c < nstats) stats[c] = (float)((c == 0 ? sign0 : 1.0) * sum / m);
  else if (tail) tail[c - nstats] = (float)sum;
}

}  // namespace ppo_head
#endif
