// smplsim_mlp.hip — host side of the policy MLP and the PPO update on gfx950: the launch planning of the bf16 GEMMs and the C ABI
// (include/smplsim_mlp.h) of every learning entry point.  The kernels are in headers: ss_gemm128.h (128-row tiles, shared pieces),
// ss_gemm256.h / ss_gemm256_kernels.h (256 x 256 tiles, weight gradient), ss_sampler.h, ss_ppo_head.h, ss_optim.h, ss_norm.h, ss_gather.h, ss_episode.h,
// ss_clip_sampling.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <string>

#include "../../include/smplsim_hip.h"
#include "../../include/smplsim_mlp.h"
#include "ss_api.h"
#include "ss_gemm128.h"
#include "ss_gemm256_kernels.h"
#include "ss_sampler.h"
#include "ss_ppo_head.h"
#include "ss_optim.h"
#include "ss_norm.h"
#include "ss_gather.h"
#include "ss_episode.h"
#include "ss_clip_sampling.h"

namespace {

using namespace gemm128;   // BM and the 128-row kernels
using namespace gemm256;   // TILE, the G256_* modes, LinearTrainArgs, WgradArgs and the 256-tile kernels
using sampler::ss_gaussian_sample_kernel;
using sampler::ss_obs_to_bf16_kernel;

int fail(int code, const char *msg) { ss::last_error() = msg; return code; }
// the status of the launches an entry point has just made
int launched() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? SS_OK : fail(SS_ERR_HIP, hipGetErrorString(e));
}

// ---- host dispatch: every GEMM launch is planned from the entry point's arguments alone, one function per decision, and launched by
// launch_gemm, which knows exactly the instantiations these plans can name
enum GemmFamily { GEMM_GLDS, GEMM_LINEAR, GEMM_TRAIN, GEMM_256, GEMM_WGRAD };
struct GemmPlan {
  GemmFamily family;
  bool f32;                           // fp32 output (GEMM_GLDS, GEMM_LINEAR) or fp32 partial sums added by atomics (the others)
  int mode = -1;                      // GEMM_256: G256_*
  int bn = 256, bk = 64, waves = 8;   // tile width, K tile, waves per workgroup (64 * waves threads)
  dim3 grid;
  size_t lds = 0;                     // dynamic LDS bytes
  int ksplit = 1, kper = 0;           // K shares over grid.z and 64-wide K tiles per share (the accumulating forms)
  bool det = false;                   // GEMM_WGRAD: the shares' partial sums stored into a workspace (ss_wgrad_bf16_det) instead of added by atomics
};

// Tile width of the 128-row kernels: the one whose tile count fills the chip's 256 CUs in whole rounds (4096 x 2048 -> 256 columns, x 1536 ->
// 192, x 1024 -> 128, x 512 -> 64: exactly one 128-row tile per CU each; round 3 used 128 x 128 for the two widest layers = 1.5 rounds of
// workgroups, a third of the chip idle in the second), ties to the wider tile (more MFMAs per LDS byte and per barrier).  Widths above 128
// only when `wide`, above 64 only up to N.  `whole`: every round counts as full, only the columns wasted by the last tile count (the
// accumulating form fills the chip with its K split, and so does a batch of thousands of rows: there the widest tile wins on every product
// measured, profiles/r06_train_gemm_sweep.txt).
int fill_bn(int M, int N, bool wide, bool whole) {
  const int gm = (M + BM - 1) / BM;
  int bn = 64;
  double best = -1;
  for (const int c : {256, 192, 128, 64}) {
    if ((c > 128 && !wide) || (c > 64 && N < c)) continue;
    const long long tiles = (long long)((N + c - 1) / c) * gm, rounds = (tiles + 255) / 256;
    const double fill = (whole ? 1.0 : (double)tiles / (double)(rounds * 256)) * ((double)N / (double)(((N + c - 1) / c) * c));
    if (fill > best + 1e-9) { best = fill; bn = c; }
  }
  return bn;
}

// what the 256 x 256 kernel (ss_gemm256_kernels.h) takes besides its row and output counts: whole pairs of K tiles, 32-bit source offsets
bool fits_256(int M, int N, int K) { return K >= 128 && K % 128 == 0 && (long long)M * K < (1ll << 32) && (long long)N * K < (1ll << 32); }

// K split of the 256 x 256 kernels' accumulating forms: as many shares as fill ONE round of the 256 CUs (one workgroup per CU; 28 tiles x
// 19 shares = 532 workgroups ran as three rounds), at least 8 K tiles each, then shares of an even number of K tiles (nkt is even: the last too)
void split_256(GemmPlan &p, long long tiles, int nkt) {
  p.ksplit = std::max(1, std::min((int)(256 / tiles), nkt / 8));
  p.kper = (nkt + p.ksplit - 1) / p.ksplit;
  p.kper += p.kper & 1;
  p.ksplit = (nkt + p.kper - 1) / p.kper;
}

GemmPlan plan_256(int M, int N, int K, int mode) {
  constexpr int T = gemm256::TILE;
  GemmPlan p{GEMM_256, mode == G256_ACCUM, mode};
  const int gx = (N + T - 1) / T, gy = (M + T - 1) / T;
  if (p.f32) split_256(p, (long long)gx * gy, K / 64);
  p.grid = dim3(gx, gy, p.ksplit);
  p.lds = p.f32 ? gemm256::LOOP_LDS_BYTES : (size_t)T * (T + 8) * sizeof(__bf16);
  return p;
}

// ss_linear_bf16.  Thousands of rows (the update's and GAE's passes over the whole rollout): the 256 x 256 kernel, 1.19 PFLOP/s on 53 248 x 1536
// x 2048 against 0.60 for the 128-row tiles; at the sampler's 4096 rows it has at most 128 tiles for 256 CUs and stays out.  The wide tiles need
// the K tile of 64 and a deep K (289 -> 2048 has 5 K tiles: the 256-column tile's longer prologue / epilogue made it 24 vs 18 us).
GemmPlan plan_linear(int M, int N, int K, bool f32) {
  if (!f32 && (long long)((M + 255) / 256) * ((N + 255) / 256) >= 230 && N % 256 == 0 && K >= 256 && fits_256(M, N, K)) return plan_256(M, N, K, G256_PLAIN);
  // round 5: asynchronous global -> LDS copies, three K tiles in flight.  A shallow K keeps the two-stage kernel (two workgroups per CU hide
  // its short loop better): 8 waves of 32 x BN/2 each, twice the waves per SIMD; K an odd multiple of 32: 4 waves with K tiles of 32
  const bool k64 = K % 64 == 0, glds = k64 && K >= 512;
  GemmPlan p{glds ? GEMM_GLDS : GEMM_LINEAR, f32};
  p.bn = fill_bn(M, N, glds, false);
  p.bk = k64 ? 64 : 32;
  p.waves = k64 ? 8 : 4;
  p.grid = dim3((N + p.bn - 1) / p.bn, (M + BM - 1) / BM);
  // the two-stage kernel: the K loop's two stages; the epilogue stages the output tile in the same memory
  p.lds = glds ? (size_t)3 * (BM + p.bn) * 64 * sizeof(__bf16) : std::max((size_t)2 * (BM + p.bn) * (p.bk + 8), (size_t)BM * (p.bn + 8)) * sizeof(__bf16);
  return p;
}

// ss_linear_bf16_train's 128-row kernel: the tile width as above, then the K split of the accumulating form: products whose output has fewer
// tiles than CUs and a deep contraction (the weight gradients: K = the batch) are cut along K into as many shares as fill about two rounds
GemmPlan plan_train(int M, int N, int K, bool acc) {
  const int gm = (M + BM - 1) / BM, nkt = K / 64;
  GemmPlan p{GEMM_TRAIN, acc};
  p.bn = fill_bn(M, N, K >= 512, acc || gm >= 64);
  if (acc) {
    const long long tiles = (long long)((N + p.bn - 1) / p.bn) * gm;
    p.ksplit = std::max(1, std::min((int)((512 + tiles - 1) / tiles), nkt / 8));   // at least 8 K tiles per share
    p.kper = (nkt + p.ksplit - 1) / p.ksplit;
  }
  p.grid = dim3((N + p.bn - 1) / p.bn, gm, p.ksplit);
  const size_t loop = (size_t)3 * (BM + p.bn) * 64 * sizeof(__bf16), epi = (size_t)std::max(BM * (p.bn + 8), p.bn * (BM + 8)) * sizeof(__bf16);
  p.lds = acc ? loop : std::max(loop, epi);
  return p;
}

// the kernel of a plan: exactly the instantiations the plans above can name
const void *gemm_kernel(const GemmPlan &p) {
  typedef const void *F;
  const int w = p.bn / 64 - 1, o = p.f32;   // BN 64 / 128 / 192 / 256
  switch (p.family) {
  case GEMM_GLDS: {
    static const F k[4][2] = {{F(ss_linear_glds_kernel<64, false>), F(ss_linear_glds_kernel<64, true>)}, {F(ss_linear_glds_kernel<128, false>), F(ss_linear_glds_kernel<128, true>)},
                              {F(ss_linear_glds_kernel<192, false>), F(ss_linear_glds_kernel<192, true>)}, {F(ss_linear_glds_kernel<256, false>), F(ss_linear_glds_kernel<256, true>)}};
    return k[w][o];
  }
  case GEMM_LINEAR: {   // BN 64 / 128: 8 waves (4 x 2) with K tiles of 64, 4 waves (2 x 2) with K tiles of 32
    static const F k[2][2][2] = {{{F(ss_linear_kernel<64, 64, false, 4>), F(ss_linear_kernel<64, 64, true, 4>)}, {F(ss_linear_kernel<128, 64, false, 4>), F(ss_linear_kernel<128, 64, true, 4>)}},
                                 {{F(ss_linear_kernel<64, 32, false, 2>), F(ss_linear_kernel<64, 32, true, 2>)}, {F(ss_linear_kernel<128, 32, false, 2>), F(ss_linear_kernel<128, 32, true, 2>)}}};
    return k[p.bk == 32][w][o];
  }
  case GEMM_TRAIN: {
    static const F k[4][2] = {{F(ss_linear_train_kernel<64, false>), F(ss_linear_train_kernel<64, true>)}, {F(ss_linear_train_kernel<128, false>), F(ss_linear_train_kernel<128, true>)},
                              {F(ss_linear_train_kernel<192, false>), F(ss_linear_train_kernel<192, true>)}, {F(ss_linear_train_kernel<256, false>), F(ss_linear_train_kernel<256, true>)}};
    return k[w][o];
  }
  case GEMM_256: {
    static const F k[7] = {F(ss_gemm256_kernel<G256_ACCUM>), F(ss_gemm256_kernel<G256_PLAIN>), F(ss_gemm256_kernel<G256_FWD>), F(ss_gemm256_kernel<G256_DX>),
                           F(ss_gemm256_kernel<G256_FWDN>), F(ss_gemm256_kernel<G256_DXN>), F(ss_gemm256_kernel<G256_DXN_DET>)};
    return k[p.mode];
  }
  case GEMM_WGRAD: return p.det ? F(ss_wgrad_tn_det_kernel) : F(ss_wgrad_tn_kernel);
  }
  return nullptr;
}

// ss_debug_last_gemm: which instantiation the host dispatch launched last on this thread (tests assert it)
thread_local std::string last_gemm;

int launch_gemm(const GemmPlan &p, void **args, hipStream_t st) {
  const void *kern = gemm_kernel(p);
  // per launch: the attribute belongs to the (kernel, device) pair and the call is a table write (a process-wide flag left
  // the wide tiles of a second GPU at the 64 KB default: ADVICE r4)
  if (hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds) != hipSuccess) return fail(SS_ERR_HIP, "cannot size the GEMM's LDS");
  static const char *const family[] = {"glds", "linear", "train", "gemm256", "wgrad"}, *const mode[] = {"ACCUM", "PLAIN", "FWD", "DX", "FWDN", "DXN", "DXN"};
  char b[160];
  snprintf(b, sizeof b, "%s mode=%s bn=%d bk=%d waves=%d out=%s ksplit=%d kper=%d%s", family[p.family], p.family == GEMM_256 ? mode[p.mode] : "-", p.bn, p.bk,
           p.waves, !p.f32 ? "bf16" : p.family <= GEMM_LINEAR ? "f32" : p.det ? "f32det" : "f32acc", p.ksplit, p.kper, p.mode == G256_DXN_DET ? " colsum=det" : "");
  last_gemm = b;
  (void)hipLaunchKernel(kern, p.grid, dim3(64 * p.waves), args, p.lds, st);
  return launched();
}

// the second launch of the deterministic forms (ss_debug_last_gemm keeps describing the GEMM)
int launch_reduce(const float *part, float *out, int rows, int cols, int ldo, int S, hipStream_t st) {
  hipLaunchKernelGGL(ss_reduce_shares_kernel, dim3((unsigned)((rows * cols + 255) / 256)), dim3(256), 0, st, part, out, rows, cols, ldo, S);
  return launched();
}

int check_workspace(const void *ws, int64_t bytes, int64_t need) {
  if (!ws) return fail(SS_ERR_INVALID, "deterministic form: null workspace");
  if (reinterpret_cast<size_t>(ws) & 15) return fail(SS_ERR_INVALID, "deterministic form: the workspace must be 16-byte aligned");
  if (bytes < need) return fail(SS_ERR_INVALID, "deterministic form: the workspace is too small (see the _workspace query)");
  return SS_OK;
}

bool dx_served(int M, int N, int K) { return N >= 256 && M >= 2048 && fits_256(M, N, K); }   // ss_linear_bf16_dx: the 256 x 256 kernel only

}  // namespace

extern "C" {

int ss_linear_bf16(const void *x, const void *w, const float *bias, void *y, int32_t M, int32_t N, int32_t K, int32_t ldy, int32_t act,
                   int32_t y_is_f32, void *stream) {
  if (!x || !w || !y) return fail(SS_ERR_INVALID, "null argument");
  if (M < 1 || N < 1 || K < 32 || K % 32 || ldy < N) return fail(SS_ERR_INVALID, "ss_linear_bf16: K must be a positive multiple of 32, ldy >= N");
  if (act < SS_ACT_NONE || act > SS_ACT_RELU) return fail(SS_ERR_INVALID, "unknown activation");
  const __bf16 *X = static_cast<const __bf16 *>(x), *Wt = static_cast<const __bf16 *>(w);
  int remap = 1;   // XCD-aware tile order
  const GemmPlan p = plan_linear(M, N, K, y_is_f32);
  if (p.family == GEMM_256) {
    LinearTrainArgs a{X, Wt, bias, nullptr, y, nullptr, nullptr, M, N, K, ldy, 0, act, remap};
    void *args[] = {&a};
    return launch_gemm(p, args, (hipStream_t)stream);
  }
  void *args[] = {&X, &Wt, &bias, &y, &M, &N, &K, &ldy, &act, &remap};
  return launch_gemm(p, args, (hipStream_t)stream);
}

static int linear_train_impl(const void *x, const void *w, const float *bias, const void *mul, void *y, void *yt, void *dact, int32_t M, int32_t N, int32_t K,
                             int32_t ldy, int32_t ldyt, int32_t act, int32_t y_is_f32_accumulate, float *colsum, void *stream, bool det = false,
                             void *colsum_ws = nullptr, int64_t colsum_ws_bytes = 0) {   // det: ss_linear_bf16_dx_det (partial column sums into colsum_ws, reduced into colsum by a second launch)
  if (!x || !w || (!y && !yt)) return fail(SS_ERR_INVALID, "null argument");
  if (M < 1 || N < 1 || K < 64 || K % 64 || (y && ldy < N) || (yt && ldyt < M)) return fail(SS_ERR_INVALID, "ss_linear_bf16_train: K must be a positive multiple of 64, ldy >= N, ldyt >= M");
  if (act < SS_ACT_NONE || act > SS_ACT_RELU) return fail(SS_ERR_INVALID, "unknown activation");
  if (y_is_f32_accumulate && (yt || dact || mul || act != SS_ACT_NONE || !y)) return fail(SS_ERR_INVALID, "ss_linear_bf16_train: the accumulating fp32 form has no other outputs, operand or activation");
  if ((mul || dact) && !y) return fail(SS_ERR_INVALID, "ss_linear_bf16_train: mul / dact share y's row stride: y must be given");
  // the 256 x 256 kernel (ss_gemm256_kernels.h): products with thousands of rows or a K split to fill the chip with
  // (measured, profiles/r06_gemm256.txt: thousands of rows -> 1.5-2 x the 128-row kernel; weight gradients with the batch as K -> 1.05-2.2 x once the K split fills ONE round)
  // the set of outputs it is built for (the other combinations keep the 128-row kernel)
  const int mode256 = y_is_f32_accumulate ? G256_ACCUM : (y && !mul && !yt && !dact) ? G256_PLAIN : (y && !mul && yt && dact) ? G256_FWD : (y && mul && yt && !dact) ? G256_DX :
                      (y && !mul && !yt && dact) ? G256_FWDN : (y && mul && !yt && !dact) ? G256_DXN : -1;
  const bool big = mode256 >= 0 && N >= 256 && M >= 256 && fits_256(M, N, K) && (y_is_f32_accumulate ? K >= 8192 : M >= 2048);
  if (colsum && !(big && (mode256 == G256_DX || mode256 == G256_DXN)))
    return fail(SS_ERR_INVALID, "ss_linear_bf16_dx: column sums come from the 256 x 256 kernel only (M >= 2048, N >= 256, K a multiple of 128, mul and y given)");
  const int prows = 2 * ((M + 255) / 256);   // one row of partial column sums per 128 rows of the batch
  if (det && check_workspace(colsum_ws, colsum_ws_bytes, (int64_t)prows * N * 4) != SS_OK) return SS_ERR_INVALID;
  const GemmPlan p = big ? plan_256(M, N, K, det ? G256_DXN_DET : mode256) : plan_train(M, N, K, y_is_f32_accumulate);
  LinearTrainArgs a{static_cast<const __bf16 *>(x), static_cast<const __bf16 *>(w), bias, static_cast<const __bf16 *>(mul), y, static_cast<__bf16 *>(yt),
                    static_cast<__bf16 *>(dact), M, N, K, ldy, ldyt, act, 1, p.kper};
  a.colsum = det ? static_cast<float *>(colsum_ws) : colsum;
  void *args[] = {&a};
  const int rc = launch_gemm(p, args, (hipStream_t)stream);
  if (rc != SS_OK || !det) return rc;
  return launch_reduce(a.colsum, colsum, 1, N, N, prows, (hipStream_t)stream);
}

int ss_linear_bf16_train(const void *x, const void *w, const float *bias, const void *mul, void *y, void *yt, void *dact, int32_t M, int32_t N, int32_t K,
                         int32_t ldy, int32_t ldyt, int32_t act, int32_t y_is_f32_accumulate, void *stream) {
  return linear_train_impl(x, w, bias, mul, y, yt, dact, M, N, K, ldy, ldyt, act, y_is_f32_accumulate, nullptr, stream);
}

int ss_linear_bf16_dx(const void *x, const void *w, const void *mul, void *y, float *colsum, int32_t M, int32_t N, int32_t K, int32_t ldy, void *stream) {
  if (!mul || !y || !colsum) return fail(SS_ERR_INVALID, "null argument");
  return linear_train_impl(x, w, nullptr, mul, y, nullptr, nullptr, M, N, K, ldy, 0, SS_ACT_NONE, 0, colsum, stream);
}

int ss_linear_bf16_dx_det(const void *x, const void *w, const void *mul, void *y, float *colsum, int32_t M, int32_t N, int32_t K, int32_t ldy, void *workspace,
                          int64_t workspace_bytes, void *stream) {
  if (!mul || !y || !colsum) return fail(SS_ERR_INVALID, "null argument");
  return linear_train_impl(x, w, nullptr, mul, y, nullptr, nullptr, M, N, K, ldy, 0, SS_ACT_NONE, 0, colsum, stream, true, workspace, workspace_bytes);
}

int64_t ss_linear_bf16_dx_det_workspace(int32_t M, int32_t N, int32_t K) {
  if (M < 1 || N < 1 || K < 64 || K % 64 || !dx_served(M, N, K)) {
    fail(SS_ERR_INVALID, "ss_linear_bf16_dx_det_workspace: M >= 2048, N >= 256, K a multiple of 128 (the shapes ss_linear_bf16_dx serves)");
    return -1;
  }
  return (int64_t)2 * ((M + 255) / 256) * N * 4;
}

static int wgrad_impl(const void *dz, const void *h, float *dw, int32_t Mb, int32_t n_out, int32_t n_in, int32_t ldz, int32_t ldh, int32_t ldw, void *stream, bool det,
                      void *workspace, int64_t workspace_bytes) {
  if (!dz || !h || !dw) return fail(SS_ERR_INVALID, "null argument");
  if (Mb < 128 || Mb % 128 || n_out < 1 || n_in < 1 || ldz < n_out || ldh < n_in || ldw < n_in || (ldz & 7) || (ldh & 7) || (n_out & 7) || (n_in & 7) ||
      (reinterpret_cast<size_t>(dz) & 15) || (reinterpret_cast<size_t>(h) & 15))
    return fail(SS_ERR_INVALID, "ss_wgrad_bf16: the batch a multiple of 128 rows; n_out, n_in, ldz, ldh multiples of 8; 16-byte aligned operands; ldw >= n_in");
  if ((long long)Mb * ldz >= (1ll << 32) || (long long)Mb * ldh >= (1ll << 32)) return fail(SS_ERR_INVALID, "ss_wgrad_bf16: operands beyond 2^32 elements");
  const int gx = (n_in + 255) / 256, gy = (n_out + 255) / 256, nkt = Mb / 64;
  GemmPlan p{GEMM_WGRAD, true};
  split_256(p, (long long)gx * gy, nkt);
  p.grid = dim3(gx, gy, p.ksplit);
  p.lds = gemm256::LoopTN::LDS_BYTES;
  p.det = det;
  if (det) {
    if ((long long)n_out * n_in > (1ll << 30)) return fail(SS_ERR_INVALID, "ss_wgrad_bf16_det: more than 2^30 outputs");
    if (check_workspace(workspace, workspace_bytes, (int64_t)p.ksplit * n_out * n_in * 4) != SS_OK) return SS_ERR_INVALID;
  }
  // the deterministic form: the shares' images dense in the workspace (row stride n_in), then one fixed-order pass adds them to dw
  WgradArgs a{static_cast<const __bf16 *>(dz), static_cast<const __bf16 *>(h), det ? static_cast<float *>(workspace) : dw, n_out, n_in, ldz, ldh, det ? n_in : ldw, nkt, p.kper};
  void *args[] = {&a};
  const int rc = launch_gemm(p, args, (hipStream_t)stream);
  if (rc != SS_OK || !det) return rc;
  return launch_reduce(a.dW, dw, n_out, n_in, ldw, p.ksplit, (hipStream_t)stream);
}

int ss_wgrad_bf16(const void *dz, const void *h, float *dw, int32_t Mb, int32_t n_out, int32_t n_in, int32_t ldz, int32_t ldh, int32_t ldw, void *stream) {
  return wgrad_impl(dz, h, dw, Mb, n_out, n_in, ldz, ldh, ldw, stream, false, nullptr, 0);
}

int ss_wgrad_bf16_det(const void *dz, const void *h, float *dw, int32_t Mb, int32_t n_out, int32_t n_in, int32_t ldz, int32_t ldh, int32_t ldw, void *workspace,
                      int64_t workspace_bytes, void *stream) {
  return wgrad_impl(dz, h, dw, Mb, n_out, n_in, ldz, ldh, ldw, stream, true, workspace, workspace_bytes);
}

int64_t ss_wgrad_bf16_det_workspace(int32_t Mb, int32_t n_out, int32_t n_in) {
  if (Mb < 128 || Mb % 128 || n_out < 1 || n_in < 1 || (n_out & 7) || (n_in & 7) || (long long)n_out * n_in > (1ll << 30)) {
    fail(SS_ERR_INVALID, "ss_wgrad_bf16_det_workspace: the batch a multiple of 128 rows; n_out, n_in multiples of 8");
    return -1;
  }
  GemmPlan p{GEMM_WGRAD, true};
  split_256(p, (long long)((n_in + 255) / 256) * ((n_out + 255) / 256), Mb / 64);
  return (int64_t)p.ksplit * n_out * n_in * 4;
}

int ss_debug_last_gemm(char *buf, int32_t len) {
  if (!buf || len < 1) return fail(SS_ERR_INVALID, "null argument");
  snprintf(buf, (size_t)len, "%s", last_gemm.c_str());
  return (int)last_gemm.size();
}

int ss_gaussian_sample(const float *mean, const float *noise, const float *log_std, int32_t M, int32_t dim, float *action, int32_t lda,
                       float *action_env, int32_t lde, float clip_lo, float clip_hi, float *logp, void *stream) {
  if (!mean || !noise || !log_std || !action) return fail(SS_ERR_INVALID, "null argument");
  if (M < 1 || dim < 1 || lda < dim || (action_env && lde < dim)) return fail(SS_ERR_INVALID, "ss_gaussian_sample: row strides must be >= dim");
  hipLaunchKernelGGL(ss_gaussian_sample_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, (hipStream_t)stream, mean, noise, log_std, M, dim, action, lda,
                     action_env, lde, clip_lo, clip_hi, logp);
  return launched();
}

int ss_obs_to_bf16(const float *obs, int32_t M, int32_t dim, int32_t obs_stride, const float *mean, const float *sd, const int64_t *n,
                   float lo, float hi, float clip, void *out, int32_t kpad, void *stream) {
  if (!obs || !out) return fail(SS_ERR_INVALID, "null argument");
  if (M < 1 || dim < 1 || kpad < dim || kpad % 32 || obs_stride < dim) return fail(SS_ERR_INVALID, "ss_obs_to_bf16: kpad must be a multiple of 32 and >= dim");
  const long long total = (long long)M * kpad;
  hipLaunchKernelGGL(ss_obs_to_bf16_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, obs, M, dim, obs_stride, mean, sd,
                     reinterpret_cast<const long long *>(n), lo, hi, clip, static_cast<__bf16 *>(out), kpad);
  return launched();
}

// ---- the PPO loss heads (ss_ppo_head.h): two launches each on `stream`, the heads' partial rows into the caller's workspace, then the fixed-order reduce
static int64_t row_groups(int32_t M, int rows) { return ((int64_t)M + rows - 1) / rows; }             // in 64 bits: M + rows - 1 may pass INT32_MAX
static int64_t policy_head_bytes(int32_t M, int32_t dim) { return row_groups(M, ppo_head::POLICY_ROWS) * (ppo_head::NSTATS + dim) * 8; }
static int64_t value_head_bytes(int32_t M) { return row_groups(M, ppo_head::VALUE_ROWS) * 8; }
static bool bad_bf16_grad(const void *g, int32_t ldd) { return (ldd & 7) || (reinterpret_cast<size_t>(g) & 15); }

int64_t ss_ppo_policy_head_workspace(int32_t M, int32_t dim) {
  if (M < 1 || dim < 1 || dim > ppo_head::MAX_DIM) {
    fail(SS_ERR_INVALID, "ss_ppo_policy_head_workspace: M >= 1, 1 <= dim <= 256");
    return -1;
  }
  return policy_head_bytes(M, dim);
}

int ss_ppo_policy_head(const float *mean, int32_t ldm, const float *actions, int32_t lda, const float *log_std, const float *adv, const float *old_logp, int32_t M,
                       int32_t dim, float clip_eps, float *logp, void *dmean, int32_t ldd, int32_t dmean_is_bf16, float *dlog_std, float *stats, void *workspace,
                       int64_t workspace_bytes, void *stream) {
  if (!mean || !actions || !log_std || !adv || !old_logp || !dmean || !stats) return fail(SS_ERR_INVALID, "null argument");
  if (M < 1 || dim < 1 || dim > ppo_head::MAX_DIM) return fail(SS_ERR_INVALID, "ss_ppo_policy_head: M >= 1, 1 <= dim <= 256");
  if (ldm < dim || lda < dim || ldd < dim) return fail(SS_ERR_INVALID, "ss_ppo_policy_head: row strides must be >= dim");
  if (!(clip_eps > 0.f && clip_eps < 1.f)) return fail(SS_ERR_INVALID, "ss_ppo_policy_head: clip_eps must lie in (0, 1)");
  if (dmean_is_bf16 && bad_bf16_grad(dmean, ldd)) return fail(SS_ERR_INVALID, "ss_ppo_policy_head: a bf16 dmean needs ldd a multiple of 8 and a 16-byte aligned base");
  if (check_workspace(workspace, workspace_bytes, policy_head_bytes(M, dim)) != SS_OK) return SS_ERR_INVALID;
  const int P = (int)row_groups(M, ppo_head::POLICY_ROWS), W = ppo_head::NSTATS + dim;
  const ppo_head::PolicyHeadArgs a{mean, actions, log_std, adv, old_logp, logp, dmean, static_cast<double *>(workspace), M, dim, ldm, lda, ldd,
                                   1.0 - (double)clip_eps, 1.0 + (double)clip_eps, 1.0 / M};
  hipStream_t st = (hipStream_t)stream;
  if (dmean_is_bf16) hipLaunchKernelGGL(ppo_head::ss_ppo_policy_head_kernel<true>, dim3((unsigned)P), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(ppo_head::ss_ppo_policy_head_kernel<false>, dim3((unsigned)P), dim3(256), 0, st, a);
  hipLaunchKernelGGL(ppo_head::ss_head_reduce_kernel, dim3((unsigned)((W + 63) / 64)), dim3(64), 0, st, a.part, P, W, stats, ppo_head::NSTATS, dlog_std, (double)M, -1.0);
  return launched();
}

int64_t ss_value_head_workspace(int32_t M) {
  if (M < 1) {
    fail(SS_ERR_INVALID, "ss_value_head_workspace: M >= 1");
    return -1;
  }
  return value_head_bytes(M);
}

int ss_value_head(const float *pred, const float *target, int32_t M, void *dpred, int32_t ldd, int32_t dpred_is_bf16, float *loss, void *workspace,
                  int64_t workspace_bytes, void *stream) {
  if (!pred || !target || !dpred || !loss) return fail(SS_ERR_INVALID, "null argument");
  if (M < 1) return fail(SS_ERR_INVALID, "ss_value_head: M >= 1");
  if (ldd < 1) return fail(SS_ERR_INVALID, "ss_value_head: row strides must be >= 1");
  if (dpred_is_bf16 && bad_bf16_grad(dpred, ldd)) return fail(SS_ERR_INVALID, "ss_value_head: a bf16 dpred needs ldd a multiple of 8 and a 16-byte aligned base");
  if (check_workspace(workspace, workspace_bytes, value_head_bytes(M)) != SS_OK) return SS_ERR_INVALID;
  const int P = (int)row_groups(M, ppo_head::VALUE_ROWS);
  double *part = static_cast<double *>(workspace);
  hipStream_t st = (hipStream_t)stream;
  if (dpred_is_bf16) hipLaunchKernelGGL(ppo_head::ss_value_head_kernel<true>, dim3((unsigned)P), dim3(256), 0, st, pred, target, M, dpred, ldd, part, 1.0 / M);
  else hipLaunchKernelGGL(ppo_head::ss_value_head_kernel<false>, dim3((unsigned)P), dim3(256), 0, st, pred, target, M, dpred, ldd, part, 1.0 / M);
  hipLaunchKernelGGL(ppo_head::ss_head_reduce_kernel, dim3(1), dim3(64), 0, st, part, P, 1, loss, 1, static_cast<float *>(nullptr), (double)M, 1.0);
  return launched();
}

// ---- the optimiser step (ss_optim.h): three launches on `stream`, the descriptor table by value in the kernel arguments
// Checks the descriptors and fills the kernels' table; returns the number of tiles, or -1 (ss_last_error set).
static int64_t adam_table(const ss_adam_tensor *tensors, int32_t count, optim::Table &tb) {
  if (!tensors) return fail(SS_ERR_INVALID, "null argument");
  if (count < 1 || count > optim::MAX_TENSORS) return fail(SS_ERR_INVALID, "ss_adam_step: 1 <= count <= 32 tensors in one call");
  int64_t tiles = 0;
  for (int i = 0; i < count; i++) {
    const ss_adam_tensor &d = tensors[i];
    if (!d.p || !d.m || !d.v || !d.g) return fail(SS_ERR_INVALID, "null argument");
    if (d.rows < 1 || d.cols < 1) return fail(SS_ERR_INVALID, "ss_adam_step: rows >= 1, cols >= 1");
    if (d.ldg < d.cols || (d.w_bf16 && d.ld_w < d.cols) || (d.wt_bf16 && d.ld_wt < d.rows))
      return fail(SS_ERR_INVALID, "ss_adam_step: row strides must be >= the row's width (ldg, ld_w >= cols; ld_wt >= rows)");
    if ((d.w_bf16 && bad_bf16_grad(d.w_bf16, d.ld_w)) || (d.wt_bf16 && bad_bf16_grad(d.wt_bf16, d.ld_wt)))
      return fail(SS_ERR_INVALID, "ss_adam_step: a bf16 image needs its row stride a multiple of 8 and a 16-byte aligned base");
    tb.t[i] = optim::Tensor{d.p, d.m, d.v, d.g, static_cast<unsigned short *>(d.w_bf16), static_cast<unsigned short *>(d.wt_bf16), d.rows, d.cols, d.ldg,
                            d.w_bf16 ? d.ld_w : 0, d.wt_bf16 ? d.ld_wt : 0, (int)tiles};
    tiles += row_groups(d.rows, optim::TILE) * row_groups(d.cols, optim::TILE);
    if (tiles > (1ll << 30)) return fail(SS_ERR_INVALID, "ss_adam_step: more than 2^30 tiles in one call");
  }
  tb.count = count;
  return tiles;
}

int64_t ss_adam_step_workspace(const ss_adam_tensor *tensors, int32_t count) {
  optim::Table tb{};
  const int64_t tiles = adam_table(tensors, count, tb);
  return tiles < 0 ? -1 : (tiles + 1) * 8;
}

int ss_adam_step(const ss_adam_tensor *tensors, int32_t count, int32_t step, double lr, double beta1, double beta2, double eps, double weight_decay,
                 double max_grad_norm, float *grad_norm, void *workspace, int64_t workspace_bytes, void *stream) {
  optim::Table tb{};
  const int64_t tiles = adam_table(tensors, count, tb);
  if (tiles < 0) return SS_ERR_INVALID;
  if (step < 1) return fail(SS_ERR_INVALID, "ss_adam_step: step >= 1");
  if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) return fail(SS_ERR_INVALID, "ss_adam_step: the betas must lie in [0, 1)");
  if (!(eps >= 0.0)) return fail(SS_ERR_INVALID, "ss_adam_step: eps >= 0");
  if (lr != lr || weight_decay != weight_decay || max_grad_norm != max_grad_norm) return fail(SS_ERR_INVALID, "ss_adam_step: lr, weight_decay and max_grad_norm must not be NaN");
  if (check_workspace(workspace, workspace_bytes, (tiles + 1) * 8) != SS_OK) return SS_ERR_INVALID;
  const bool clip = max_grad_norm > 0.0 && max_grad_norm < HUGE_VAL;
  const optim::Hyper h{clip ? max_grad_norm : 0.0, weight_decay, beta1, beta2, lr / (1.0 - pow(beta1, (double)step)), sqrt(1.0 - pow(beta2, (double)step)), eps};
  double *part = static_cast<double *>(workspace);
  hipStream_t st = (hipStream_t)stream;
  const int T = (int)tiles;
  hipLaunchKernelGGL(optim::ss_adam_sumsq_kernel, dim3((unsigned)T), dim3(256), 0, st, tb, part);
  hipLaunchKernelGGL(optim::ss_adam_reduce_kernel, dim3(1), dim3(64), 0, st, part, T, grad_norm);
  hipLaunchKernelGGL(optim::ss_adam_step_kernel, dim3((unsigned)T), dim3(256), 0, st, tb, static_cast<const double *>(part), T, h);
  return launched();
}

// ---- RunningNorm.update (ss_norm.h): two launches on `stream`, the blocks' (mean, M2) pairs into the caller's workspace, then the fixed-order fold and the running merge
static int64_t running_norm_bytes(int32_t M, int32_t dim) { return row_groups(M, run_norm::BLOCK_ROWS) * dim * 16; }

int64_t ss_running_norm_workspace(int32_t M, int32_t dim) {
  if (M < 1 || dim < 1) {
    fail(SS_ERR_INVALID, "ss_running_norm_workspace: M >= 1, dim >= 1");
    return -1;
  }
  return running_norm_bytes(M, dim);
}

int ss_running_norm_update(const float *x, int32_t M, int32_t dim, int32_t ldx, float *mean, float *var, float *sd, int64_t *n, void *workspace,
                           int64_t workspace_bytes, void *stream) {
  if (!x || !mean || !var || !sd || !n) return fail(SS_ERR_INVALID, "null argument");
  if (M < 1 || dim < 1) return fail(SS_ERR_INVALID, "ss_running_norm_update: M >= 1, dim >= 1");
  if (ldx < dim) return fail(SS_ERR_INVALID, "ss_running_norm_update: row strides must be >= dim");
  if (check_workspace(workspace, workspace_bytes, running_norm_bytes(M, dim)) != SS_OK) return SS_ERR_INVALID;
  const int64_t P = row_groups(M, run_norm::BLOCK_ROWS), groups = row_groups(dim, run_norm::COLS);
  if (P * groups >= (1ll << 24)) return fail(SS_ERR_INVALID, "ss_running_norm_update: more than 2^24 workgroups (M / 256 row blocks x dim / 64 column groups)");
  double *part = static_cast<double *>(workspace);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(run_norm::ss_norm_partials_kernel, dim3((unsigned)(P * groups)), dim3(256), 0, st, x, M, dim, ldx, (int)groups, part);
  hipLaunchKernelGGL(run_norm::ss_norm_merge_kernel, dim3(1), dim3(256), 0, st, static_cast<const double *>(part), (int)P, M, dim, mean, var, sd,
                     reinterpret_cast<long long *>(n));
  return launched();
}

// ---- episode statistics of a rollout (ss_episode.h): two launches on `stream`, one partial row per 64 env columns into the caller's workspace, then the fixed-order fold
static int64_t episode_stats_bytes(int32_t N, int32_t P) { return row_groups(N, episode::LANES) * (episode::NFIXED + P) * 8; }

int64_t ss_episode_stats_workspace(int32_t T, int32_t N, int32_t P) {
  if (T < 1 || N < 1 || P < 0 || P > SS_EPISODE_MAX_PARTS) {
    fail(SS_ERR_INVALID, "ss_episode_stats_workspace: T >= 1, N >= 1, 0 <= P <= 8");
    return -1;
  }
  return episode_stats_bytes(N, P);
}

int ss_episode_stats(const float *rewards, const float *not_done, const float *parts, int32_t T, int32_t N, int32_t P, double *ep_return, int32_t *ep_len,
                     double *stats, void *workspace, int64_t workspace_bytes, void *stream) {
  if (!rewards || !not_done || !ep_return || !ep_len || !stats) return fail(SS_ERR_INVALID, "null argument");
  if (T < 1 || N < 1 || P < 0 || P > SS_EPISODE_MAX_PARTS) return fail(SS_ERR_INVALID, "ss_episode_stats: T >= 1, N >= 1, 0 <= P <= 8");
  if (P > 0 && !parts) return fail(SS_ERR_INVALID, "ss_episode_stats: parts is null with P > 0");
  if (check_workspace(workspace, workspace_bytes, episode_stats_bytes(N, P)) != SS_OK) return SS_ERR_INVALID;
  const int G = (int)row_groups(N, episode::LANES), W = episode::NFIXED + P;
  const episode::ScanArgs a{rewards, not_done, P > 0 ? parts : nullptr, ep_return, ep_len, static_cast<double *>(workspace), T, N, P};
  hipStream_t st = (hipStream_t)stream;
  if (P == 4 && !(reinterpret_cast<size_t>(parts) & 15)) hipLaunchKernelGGL(episode::ss_episode_scan_kernel<true>, dim3((unsigned)G), dim3(episode::LANES), 0, st, a);
  else hipLaunchKernelGGL(episode::ss_episode_scan_kernel<false>, dim3((unsigned)G), dim3(episode::LANES), 0, st, a);
  hipLaunchKernelGGL(episode::ss_episode_reduce_kernel, dim3(1), dim3(episode::LANES), 0, st, static_cast<const double *>(a.part), G, W, (double)T * (double)N, stats);
  return launched();
}

// ---- failure-weighted clip sampling (ss_clip_sampling.h): the tally of a rollout by integer atomics, one launch; the CDF of the failure counts, one workgroup
int ss_clip_outcomes(const int32_t *clip_ids, const uint8_t *dead, const uint8_t *done, int32_t T, int32_t N, int32_t M, int64_t *counts, void *stream) {
  if (!clip_ids || !dead || !done || !counts) return fail(SS_ERR_INVALID, "null argument");
  if (T < 1 || N < 1 || M < 1) return fail(SS_ERR_INVALID, "ss_clip_outcomes: T >= 1, N >= 1, M >= 1");
  if (reinterpret_cast<size_t>(counts) & 7) return fail(SS_ERR_INVALID, "ss_clip_outcomes: counts must be 8-byte aligned");
  hipLaunchKernelGGL(clip_sampling::ss_clip_outcomes_kernel, dim3((unsigned)row_groups(N, clip_sampling::LANES)), dim3(clip_sampling::LANES), 0, (hipStream_t)stream,
                     clip_ids, dead, done, T, N, M, reinterpret_cast<long long *>(counts));
  return launched();
}

int ss_clip_sampling_cdf(const int64_t *counts, int32_t M, double uniform_mix, float *cdf, double *prob, void *stream) {
  if (!counts || !cdf) return fail(SS_ERR_INVALID, "null argument");
  if (M < 1) return fail(SS_ERR_INVALID, "ss_clip_sampling_cdf: M >= 1");
  if (!(uniform_mix >= 0.0 && uniform_mix <= 1.0)) return fail(SS_ERR_INVALID, "ss_clip_sampling_cdf: uniform_mix must lie in [0, 1]");
  const double keep = 1.0 - uniform_mix, floor_ = uniform_mix / (double)M, uniform = 1.0 / (double)M;   // each ONE fp64 operation, formed once, here
  hipLaunchKernelGGL(clip_sampling::ss_clip_sampling_cdf_kernel, dim3(1), dim3(clip_sampling::CDF_THREADS), 0, (hipStream_t)stream,
                     reinterpret_cast<const long long *>(counts), M, uniform, keep, floor_, cdf, prob);
  return launched();
}

// ---- the rows of a mini-batch epoch (ss_gather.h): one launch on `stream` for all tensors, the descriptor table by value in the kernel arguments
int ss_gather_rows(const ss_gather_tensor *tensors, int32_t count, const int64_t *perm, int32_t src_rows, int32_t rows, int32_t block_rows, void *stream) {
  if (!tensors || !perm) return fail(SS_ERR_INVALID, "null argument");
  if (count < 1 || count > gather::MAX_TENSORS) return fail(SS_ERR_INVALID, "ss_gather_rows: 1 <= count <= 8 tensors in one call");
  if (src_rows < 1 || rows < 1 || block_rows < 1) return fail(SS_ERR_INVALID, "ss_gather_rows: src_rows >= 1, rows >= 1, block_rows >= 1");
  if (reinterpret_cast<size_t>(perm) & 7) return fail(SS_ERR_INVALID, "ss_gather_rows: perm must be 8-byte aligned");
  gather::Table tb{};
  int64_t tiles = 0;
  const int64_t last = (int64_t)(rows - 1) / block_rows, last_in = (int64_t)(rows - 1) % block_rows;
  for (int i = 0; i < count; i++) {
    const ss_gather_tensor &d = tensors[i];
    if (!d.src || !d.dst) return fail(SS_ERR_INVALID, "null argument");
    if (d.elem_bytes != 2 && d.elem_bytes != 4) return fail(SS_ERR_INVALID, "ss_gather_rows: elem_bytes must be 2 or 4");
    if (d.cols < 1) return fail(SS_ERR_INVALID, "ss_gather_rows: cols >= 1");
    if (d.ld_src < d.cols || d.ld_dst < d.cols) return fail(SS_ERR_INVALID, "ss_gather_rows: row strides must be >= cols");
    if (d.dst_block_stride < block_rows) return fail(SS_ERR_INVALID, "ss_gather_rows: dst_block_stride >= block_rows");
    const size_t s = reinterpret_cast<size_t>(d.src), t = reinterpret_cast<size_t>(d.dst), eb = (size_t)d.elem_bytes;
    if ((s | t) & (eb - 1)) return fail(SS_ERR_INVALID, "ss_gather_rows: src and dst must be aligned to elem_bytes");
    // the bytes the call may read and those it may write must not meet (src == dst is the simplest case)
    const size_t s_end = s + (((size_t)src_rows - 1) * d.ld_src + d.cols) * eb;
    const size_t t_end = t + (((size_t)last * d.dst_block_stride + last_in) * d.ld_dst + d.cols) * eb;
    if (s < t_end && t < s_end) return fail(SS_ERR_INVALID, "ss_gather_rows: src and dst must not overlap");
    const size_t lds = (size_t)d.ld_src * eb, ldd = (size_t)d.ld_dst * eb, width = (size_t)d.cols * eb, all = s | t | lds | ldd | width;
    const int unit = !(all & 15) ? 16 : !(all & 3) ? 4 : (int)eb;
    const int upr = (int)(width / unit);
    int l2 = 0;
    while (l2 < 6 && (1 << l2) < upr) l2++;
    const int per_row = (upr + (1 << l2) - 1) >> l2;                       // units a lane moves per row
    const int tile_rows = (gather::THREADS >> l2) * gather::ROWS_IN_FLIGHT * (per_row == 1 ? 2 : 1);
    tb.t[i] = gather::Tensor{static_cast<const char *>(d.src), static_cast<char *>(d.dst), (long long)lds, (long long)ldd, upr, unit, l2, tile_rows,
                             d.dst_block_stride, (int)tiles};
    tiles += row_groups(rows, tile_rows);
    if (tiles > INT32_MAX) return fail(SS_ERR_INVALID, "ss_gather_rows: more than 2^31 - 1 workgroups in one call");
  }
  tb.count = count;
  hipLaunchKernelGGL(gather::ss_gather_rows_kernel, dim3((unsigned)tiles), dim3(gather::THREADS), 0, (hipStream_t)stream, tb,
                     reinterpret_cast<const long long *>(perm), src_rows, rows, block_rows);
  return launched();
}

}
