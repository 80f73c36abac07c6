// ss_sampler.h — the element-wise kernels around the sampler's MLP (include/smplsim_mlp.h: ss_obs_to_bf16, ss_gaussian_sample).
#pragma once
#include <hip/hip_runtime.h>

namespace sampler {

// torch.clamp semantics: a NaN stays a NaN (fminf / fmaxf would return the bound and hide a diverged policy or observation from the env)
__device__ __forceinline__ float clamp_keep_nan(float v, float lo, float hi) { return v != v ? v : fminf(fmaxf(v, lo), hi); }

__global__ void __launch_bounds__(256) ss_obs_to_bf16_kernel(const float *obs, int M, int dim, int stride, const float *mean, const float *sd,
                                                             const long long *n, float lo, float hi, float clip, __bf16 *out, int kpad) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)M * kpad) return;
  const int row = (int)(idx / kpad), c = (int)(idx % kpad);
  float v = 0.f;
  if (c < dim) {
    v = clamp_keep_nan(obs[(size_t)row * stride + c], lo, hi);
    if (mean && sd && n && *n > 0) v = clamp_keep_nan((v - mean[c]) / (sd[c] + 1e-8f), -clip, clip);
  }
  out[idx] = (__bf16)v;
}

// Gaussian policy head of the sampler, one wavefront per env row: a = mean + exp(log_std) * noise (the product and the sum rounded
// separately, like the torch expression it replaces), its clipped copy for the env, and the log-density of the draw.
__global__ void __launch_bounds__(256) ss_gaussian_sample_kernel(const float *mean, const float *noise, const float *log_std, int M, int dim,
                                                                 float *action, int lda, float *action_env, int lde, float lo, float hi, float *logp) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= M) return;
  float acc = 0.f;
  for (int j = lane; j < dim; j += 64) {
    const float ls = log_std[j], z = noise[(size_t)row * dim + j];
    const float a = __fadd_rn(mean[(size_t)row * dim + j], __fmul_rn(__expf(ls), z));
    action[(size_t)row * lda + j] = a;
    if (action_env) action_env[(size_t)row * lde + j] = clamp_keep_nan(a, lo, hi);
    acc += -0.5f * z * z - 0.91893853320467274f - ls;          // - log sqrt(2 pi)
  }
  if (logp) {
    for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, 64);
    if (lane == 0) logp[row] = acc;
  }
}

}  // namespace sampler
