// ss_clip_sampling.h — failure-weighted clip sampling on the device (include/smplsim_mlp.h: ss_clip_outcomes, ss_clip_sampling_cdf): the bookkeeping of the
// reference's motion library (smpl_sim/smpllib/motion_lib_base.py:219-267: termination_history, update_soft_sampling_weight, update_sampling_prob) fed from the
// rollout the sampler already keeps.  ss_clip_outcomes tallies which clip every env was tracking when it fell, finished or merely stepped, into [M, 3] int64
// counters; ss_clip_sampling_cdf turns the failure column into the float32 CDF that the resampling kernels (ss_motion.h: resample_elem) search, in place.
//
// Tally: by bytes one read of T * N * 6; the scan structure of ss_episode.h — ONE wavefront per workgroup, lane l of workgroup g owns env column 64 g + l and
// walks it with t ascending, so that every [t, :] row access is a coalesced segment (256 B of ids, 64 B of each flag plane).  A lane counts the steps of the clip
// it is on in a register and adds them to the clip's counter only when the id changes, when an episode ends (the failure / completion is added then anyway) and at
// the end of its column: episodes + N adds per rollout instead of T * N — a few dozen clips would otherwise take tens of thousands of adds on a handful of
// addresses.  The adds are 64-bit INTEGER vector atomics (global_atomic_add_x2, no return value): integer addition is exact and commutative, so the counters
// are a function of the input bytes alone, whatever order the workgroups run in.  No float is summed.  Measured (profiles/clip_sampling.txt; 25 x 2048, device events
// over back-to-back calls): 12 us with 256 clips and episodes of ~17 steps, 25 us when every step ends an episode, 37 us with 7 clips — what is left is the adds that
// meet on one address (2048 adds on ONE counter: 30 us); a rollout of the sampler is 27 ms.
//
// Bounds: an id is compared with [0, M) as an unsigned value BEFORE any address is formed from it; an element that fails is skipped entirely.
//
// CDF: one workgroup of 256 threads.  S, the sum of the failure counts, is an integer sum (strided per thread, then a tree in LDS: any order gives the same
// integer).  Then chunks of 256 clips: every thread forms its clip's probability p_m — each fp64 operation rounded on its own, contraction switched off —, thread 0
// adds the chunk's 256 values onto the running sum ONE AFTER THE OTHER in ascending m (np.cumsum's order: the contract; a parallel scan would change the bits),
// and every thread stores its clip's entry.  The chain is M dependent fp64 additions on one lane, once per rollout: 7 us up to 256 clips, 78 us at 4096, 0.93 ms at
// 50 000 (18.5 ns per clip; same measurement).
#ifndef SS_CLIP_SAMPLING_H
#define SS_CLIP_SAMPLING_H
#include <hip/hip_runtime.h>

#include "../../include/smplsim_mlp.h"

namespace clip_sampling {

constexpr int LANES = 64;                        // env columns per workgroup of the tally: one per lane of its only wavefront
constexpr int UNROLL = 4;                        // steps whose loads are issued together
constexpr int COLS = SS_CLIP_COLUMNS;            // counters per clip
constexpr int CDF_THREADS = 256;                 // the CDF's only workgroup = clips per chunk

__device__ __forceinline__ void add_count(long long *counts, int clip, int column, long long v) {
  atomicAdd(reinterpret_cast<unsigned long long *>(counts + (size_t)clip * COLS + column), (unsigned long long)v);   // (two's complement: the signed sum)
}

// Workgroup g: columns 64 g .. 64 g + 63 (a lane beyond N reads and writes nothing).  `cur` is the clip whose steps the lane is holding back (-1: none, also for
// an id outside [0, M): such an element neither counts nor is counted).
__global__ void __launch_bounds__(LANES) ss_clip_outcomes_kernel(const int *__restrict__ clip_ids, const unsigned char *__restrict__ dead,
                                                                 const unsigned char *__restrict__ done, int T, int N, int M, long long *counts) {
  const long long col = (long long)blockIdx.x * LANES + threadIdx.x;
  if (col >= N) return;
  const size_t n = (size_t)col, ld = (size_t)N;
  int cur = -1;
  long long steps = 0;
  for (int t0 = 0; t0 < T; t0 += UNROLL) {
    const int k = min(UNROLL, T - t0);
    int c[UNROLL];
    unsigned char d[UNROLL], e[UNROLL];
#pragma unroll
    for (int j = 0; j < UNROLL; j++) {
      if (j < k) {
        const size_t idx = (size_t)(t0 + j) * ld + n;
        c[j] = clip_ids[idx];
        d[j] = dead[idx];
        e[j] = done[idx];
      }
    }
#pragma unroll
    for (int j = 0; j < UNROLL; j++) {
      if (j < k) {
        const int id = (unsigned)c[j] < (unsigned)M ? c[j] : -1;     // the range check, before any address
        if (id != cur) {
          if (cur >= 0) add_count(counts, cur, SS_CLIP_STEPS, steps);
          cur = id;
          steps = 0;
        }
        if (id >= 0) {
          steps += 1;
          if (d[j] | e[j]) {
            add_count(counts, id, d[j] ? SS_CLIP_FAILED : SS_CLIP_COMPLETED, 1);
            add_count(counts, id, SS_CLIP_STEPS, steps);
            steps = 0;
          }
        }
      }
    }
  }
  if (cur >= 0 && steps > 0) add_count(counts, cur, SS_CLIP_STEPS, steps);
}

// p_m of one clip: every operation rounded on its own (no FMA: the result is compared bit for bit with a NumPy restatement)
__device__ __forceinline__ double clip_prob(long long f, long long S, double s, double uniform, double keep, double floor_) {
#pragma clang fp contract(off)
  const double q = S > 0 ? (double)(f > 0 ? f : 0) / s : uniform;
  const double kq = keep * q;
  return kq + floor_;
}

// One workgroup.  uniform = 1 / M, keep = 1 - u, floor_ = u / M: formed on the host in fp64, each by one IEEE operation.
__global__ void __launch_bounds__(CDF_THREADS) ss_clip_sampling_cdf_kernel(const long long *__restrict__ counts, int M, double uniform, double keep,
                                                                           double floor_, float *__restrict__ cdf, double *__restrict__ prob) {
#pragma clang fp contract(off)
  __shared__ long long part[CDF_THREADS];
  __shared__ double p[CDF_THREADS], c[CDF_THREADS];
  __shared__ double carry;
  const int t = threadIdx.x;
  long long mine = 0;
  for (int m = t; m < M; m += CDF_THREADS) {
    const long long f = counts[(size_t)m * COLS + SS_CLIP_FAILED];
    mine += f > 0 ? f : 0;
  }
  part[t] = mine;
  __syncthreads();
  for (int w = CDF_THREADS / 2; w >= 1; w >>= 1) {
    if (t < w) part[t] += part[t + w];
    __syncthreads();
  }
  const long long S = part[0];
  const double s = (double)S;
  for (int m0 = 0; m0 < M; m0 += CDF_THREADS) {            // (uniform bounds: every thread reaches every barrier)
    const int m = m0 + t, k = min(CDF_THREADS, M - m0);
    double pm = 0.0;
    if (m < M) pm = clip_prob(counts[(size_t)m * COLS + SS_CLIP_FAILED], S, s, uniform, keep, floor_);
    p[t] = pm;
    __syncthreads();
    if (t == 0) {
      double acc = m0 == 0 ? p[0] : carry + p[0];         // c_0 = p_0; c_m = c_{m-1} + p_m
      c[0] = acc;
      for (int j = 1; j < k; j++) {
        acc = acc + p[j];
        c[j] = acc;
      }
      carry = acc;
    }
    __syncthreads();
    if (m < M) {
      cdf[m] = m < M - 1 ? (float)c[t] : (float)(1.0 + 1e-6);     // the last entry: the sentinel MotionLibSMPL.load_motions writes, so that a draw below 1 lands in a clip
      if (prob) prob[m] = pm;
    }
    __syncthreads();                                       // (p and c are rewritten by the next chunk)
  }
}

}  // namespace clip_sampling
#endif
