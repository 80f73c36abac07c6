// smplsim_hip_im.hip — the step kernel's instantiations of ss_imitation_step_fused (IMIT = true: imitation task and reference-state
// re-initialisation inside the step launch, ss_imfused.h): a translation unit of its own, compiled next to smplsim_hip.hip
// (ss_env_kernel.h).
#include "ss_env_kernel.h"

namespace ss {

kern_t pick_kernel_imitation(const KernelKey &key, const Hdr &h, const HdrC &hc) {
  const int variant = key.variant;
  if (key.cforce) {                                              // optional I/O: contact-force output, body-wrench input (ss_env_kernel.h)
    if (variant == 0) return key.shaped ? ss_env_kernel<2, 2, 1, 1, SS_MAX_THREADS, true, true, HdrRuntime, false, true, true> : ss_env_kernel<2, 2, 1, 1, SS_MAX_THREADS, true, false, HdrRuntime, false, true, true>;
    if (variant == 1) return key.shaped ? ss_env_kernel<3, 3, 2, 2, SS_MAX_THREADS_X, true, true, HdrRuntime, false, true, true> : ss_env_kernel<3, 3, 2, 2, SS_MAX_THREADS_X, true, false, HdrRuntime, false, true, true>;
    return nullptr;
  }
  if (key.shaped) {                                              // per-env body shapes (PHC-style: every env tracks clips with its own body)
    if (variant == 0) return ss_env_kernel<2, 2, 1, 1, SS_MAX_THREADS, true, true, HdrRuntime, false, true>;
    if (variant == 1) return ss_env_kernel<3, 3, 2, 2, SS_MAX_THREADS_X, true, true, HdrRuntime, false, true>;
    return nullptr;
  }
#ifndef SS_NO_FIXED_LAYOUT
  if (variant == 0 && HdrSmpl::matches(h, hc)) return ss_env_kernel<2, 2, 1, 1, SS_MAX_THREADS, true, false, HdrSmpl, false, true>;
#endif
  if (variant == 0) return ss_env_kernel<2, 2, 1, 1, SS_MAX_THREADS, true, false, HdrRuntime, false, true>;
  if (variant == 1) return ss_env_kernel<3, 3, 2, 2, SS_MAX_THREADS_X, true, false, HdrRuntime, false, true>;
  return nullptr;
}

// The imitation step with body-body contacts (SMPL size class, one shape).  Lives here, not with the other body-body-contact kernels
// (smplsim_hip_sc.hip is built -O3): at -O3 this one instantiation — the only one with two inlined run_env bodies — loses the
// observation row pointer between the top of the step pass and its use (hipcc 7.2: the value is spilled and comes back zero; seen as
// an all-zero self observation in tests/test_gpu_parity.py::test_fused_imitation_step_with_body_body_contacts_on_gpu); the flags of
// this unit compile it correctly.
kern_t pick_kernel_imitation_selfcol(const KernelKey &key, const Hdr &, const HdrC &) {
  if (key.variant == 0 && !key.shaped && key.cforce) return ss_env_kernel<2, 2, 1, 1, SS_MAX_THREADS_SC, true, false, HdrRuntime, true, true, true>;
  if (key.variant == 0 && !key.shaped) return ss_env_kernel<2, 2, 1, 1, SS_MAX_THREADS_SC, true, false, HdrRuntime, true, true>;
  return nullptr;
}

}  // namespace ss
