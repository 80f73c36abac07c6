// ss_episode.h — episode statistics of a rollout on the device (include/smplsim_mlp.h: ss_episode_stats): what the reference's sampler collects step by step in a
// LoggerRL (smpl_sim/learning/logger_rl.py: start_episode / step / end_episode) — episode returns and lengths, reward extremes, the sums of the reward terms —
// from the rollout's rewards / not_done [T, N] in two launches.  An episode spans many rollouts here (N envs in lock step for T steps), so the return and the
// length of the episode every env is in the middle of live in a per-env carry that the call reads and rewrites.
//
// By bytes this is one read of T * N * (2 + P) floats; a lane's work is a chain of T dependent fp64 additions on its column.  Reproducible by construction: no
// atomics.  Lane l of workgroup g owns column 64 g + l and walks it with t ascending; every row access [t, 64 g .. 64 g + 63] is one coalesced segment.  The 64
// lanes meet by the xor butterfly (32, 16, ..., 1) and lane 0 STORES one partial row; the second launch folds the partial rows ascending from workgroup 0.
//
// Workgroup width: ONE wavefront (64 lanes).  The scan has only N columns to hand out; at 4096 columns that is 64 workgroups on 64 CUs instead of 16 of 256 lanes
// on 16, each wavefront with a CU's memory pipeline to itself for its serial walk, and the workgroup needs neither LDS nor a barrier.  This launch has not been timed.
#ifndef SS_EPISODE_H
#define SS_EPISODE_H
#include <hip/hip_runtime.h>

#include "../../include/smplsim_mlp.h"

namespace episode {

constexpr int LANES = 64;                        // columns per workgroup = per partial row: one per lane of its only wavefront
constexpr int MAX_PARTS = SS_EPISODE_MAX_PARTS;
constexpr int NFIXED = SS_EP_PARTS;              // the nine fixed statistics in front of the P part sums
constexpr int UNROLL = 4;                        // steps whose loads are issued together; only the additions form a chain

// torch.amin / amax semantics: a NaN on either side gives a NaN
__device__ __forceinline__ double min_nan(double a, double b) { return (a != a || b != b) ? __builtin_nan("") : (b < a ? b : a); }
__device__ __forceinline__ double max_nan(double a, double b) { return (a != a || b != b) ? __builtin_nan("") : (b > a ? b : a); }

__device__ __forceinline__ double wave_sum(double v) {
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
__device__ __forceinline__ double wave_min(double v) {
  for (int m = 32; m >= 1; m >>= 1) v = min_nan(v, __shfl_xor(v, m, 64));
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
  for (int m = 32; m >= 1; m >>= 1) v = max_nan(v, __shfl_xor(v, m, 64));
  return v;
}

struct ScanArgs {
  const float *rewards, *not_done, *parts;       // [T, N], [T, N], [T, N, P] or null
  double *ep_return;                             // [N]
  int *ep_len;                                   // [N]
  double *part;                                  // [ceil(N / LANES), NFIXED + P]
  int T, N, P;
};

// VEC4: P == 4 and parts 16-byte aligned — a step's four terms by one 16-byte load.  Otherwise P loads of 4 bytes (P is uniform: the guards are scalar branches).
template <bool VEC4> __device__ __forceinline__ void add_parts(double (&ps)[MAX_PARTS], const float *parts, size_t idx, int P) {
  if (VEC4) {
    const float4 v = reinterpret_cast<const float4 *>(parts)[idx];
    ps[0] += (double)v.x;
    ps[1] += (double)v.y;
    ps[2] += (double)v.z;
    ps[3] += (double)v.w;
  } else {
    const float *row = parts + idx * (size_t)P;
#pragma unroll
    for (int p = 0; p < MAX_PARTS; p++)
      if (p < P) ps[p] += (double)row[p];
  }
}

// Workgroup g: columns 64 g .. 64 g + 63 (those below N; a lane beyond N reads and writes nothing and brings the identities 0, +inf, -inf to the butterfly).
// Partial row g, in the layout of `stats`: [0] the steps of its columns, [1] episodes ended, [2] the sum of their returns, [3] the sum of their lengths,
// [4] / [5] their smallest / largest return, [6] the sum of all rewards, [7] / [8] the smallest / largest reward, [9 + p] the sum of part p.  A lane adds with t
// ascending (an episode's return into the lane's sum at the step that ends it); counts and lengths are integers held in fp64 (exact below 2^53).
template <bool VEC4> __global__ void __launch_bounds__(LANES) ss_episode_scan_kernel(const ScanArgs a) {
  const int lane = threadIdx.x;
  const long long col = (long long)blockIdx.x * LANES + lane;
  const double inf = __builtin_huge_val();
  double episodes = 0.0, ep_sum = 0.0, ep_steps = 0.0, ep_min = inf, ep_max = -inf, r_sum = 0.0, r_min = inf, r_max = -inf;
  double ps[MAX_PARTS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (col < a.N) {
    const size_t n = (size_t)col, N = (size_t)a.N;
    double ret = a.ep_return[n];
    int len = a.ep_len[n];
    for (int t0 = 0; t0 < a.T; t0 += UNROLL) {
      const int k = min(UNROLL, a.T - t0);
      float r[UNROLL], nd[UNROLL];
#pragma unroll
      for (int j = 0; j < UNROLL; j++) {
        if (j < k) {
          const size_t idx = (size_t)(t0 + j) * N + n;
          r[j] = a.rewards[idx];
          nd[j] = a.not_done[idx];
        }
      }
#pragma unroll
      for (int j = 0; j < UNROLL; j++) {
        if (j < k) {
          const double rd = (double)r[j];
          ret += rd;
          len += 1;
          r_sum += rd;
          r_min = min_nan(r_min, rd);
          r_max = max_nan(r_max, rd);
          if (a.P > 0) add_parts<VEC4>(ps, a.parts, (size_t)(t0 + j) * N + n, a.P);
          if (nd[j] == 0.0f) {                   // +0 and -0 end the episode; any other value, a NaN included, continues it
            episodes += 1.0;
            ep_sum += ret;
            ep_steps += (double)len;
            ep_min = min_nan(ep_min, ret);
            ep_max = max_nan(ep_max, ret);
            ret = 0.0;
            len = 0;
          }
        }
      }
    }
    a.ep_return[n] = ret;
    a.ep_len[n] = len;
  }
  episodes = wave_sum(episodes);
  ep_sum = wave_sum(ep_sum);
  ep_steps = wave_sum(ep_steps);
  ep_min = wave_min(ep_min);
  ep_max = wave_max(ep_max);
  r_sum = wave_sum(r_sum);
  r_min = wave_min(r_min);
  r_max = wave_max(r_max);
#pragma unroll
  for (int p = 0; p < MAX_PARTS; p++)
    if (p < a.P) ps[p] = wave_sum(ps[p]);
  if (lane == 0) {
    const long long cols = min((long long)LANES, (long long)a.N - (long long)blockIdx.x * LANES);
    double *out = a.part + (size_t)blockIdx.x * (NFIXED + a.P);
    out[SS_EP_NUM_STEPS] = (double)a.T * (double)cols;
    out[SS_EP_NUM_EPISODES] = episodes;
    out[SS_EP_TOTAL_EPISODE_REWARD] = ep_sum;
    out[SS_EP_TOTAL_EPISODE_LEN] = ep_steps;
    out[SS_EP_MIN_EPISODE_REWARD] = ep_min;
    out[SS_EP_MAX_EPISODE_REWARD] = ep_max;
    out[SS_EP_TOTAL_REWARD] = r_sum;
    out[SS_EP_MIN_REWARD] = r_min;
    out[SS_EP_MAX_REWARD] = r_max;
#pragma unroll
    for (int p = 0; p < MAX_PARTS; p++)
      if (p < a.P) out[NFIXED + p] = ps[p];
  }
}

// One wavefront; lane j < W = NFIXED + P owns statistic j and folds the G partial rows ascending from row 0: (((P_0 + P_1) + P_2) + ...), the minima and maxima
// likewise.  num_steps is T * N from the arguments.  Nothing behind stats[W - 1] is written.
__global__ void __launch_bounds__(LANES) ss_episode_reduce_kernel(const double *__restrict__ part, int G, int W, double steps, double *__restrict__ stats) {
  const int j = threadIdx.x;
  if (j >= W) return;
  if (j == SS_EP_NUM_STEPS) {
    stats[j] = steps;
    return;
  }
  const bool is_min = j == SS_EP_MIN_EPISODE_REWARD || j == SS_EP_MIN_REWARD, is_max = j == SS_EP_MAX_EPISODE_REWARD || j == SS_EP_MAX_REWARD;
  double acc = part[j];
  for (int g = 1; g < G; g++) {
    const double v = part[(size_t)g * W + j];
    acc = is_min ? min_nan(acc, v) : is_max ? max_nan(acc, v) : acc + v;
  }
  stats[j] = acc;
}

}  // namespace episode
#endif
