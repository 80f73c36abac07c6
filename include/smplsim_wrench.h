/* smplsim_wrench.h — C ABI of the external body wrenches of libsmplsim_hip.so: the optional input of the step launches that restates
 * mjData.xfrc_applied.  A header of its own next to smplsim_hip.h (whose handles and conventions it uses), so that the list of entry
 * points a caller binds from that header stays what it was; smplsim_amd/_cabi.py binds this one with bind_wrench().
 */
#ifndef SMPLSIM_WRENCH_H
#define SMPLSIM_WRENCH_H

#ifdef __cplusplus
extern "C" {
#endif

struct ss_batch;

/* Optional input of ss_step / ss_step_autoreset / ss_imitation_step_fused / ss_substep / ss_debug_forward: an external wrench on
 * every body, MuJoCo's mjData.xfrc_applied: wrench [N, nbody, 6], float32, caller-owned, indexed by env id (NULL = off, the default).
 * Columns 0-2 are a force in newtons applied at the body's centre of mass (xipos), columns 3-5 a torque in N m, both in the world
 * frame.  The launch reads the buffer and never writes it.  The wrench is constant over the launch, i.e. over all mj_steps of the
 * control step, and is applied at the moving centre of mass in each of them.  As in mj_step it is part of the smooth force only:
 * qfrc_bias does not contain it (the bias of ss_debug_forward is without it, its qacc with it), so the Stable-PD controller, which
 * reads the bias, does not see it.  It is never applied by a reset: not by ss_reset (the mj_steps of StateInit Fall run without it)
 * and not by the in-launch reset of an env whose episode ended — the reference resets mjData before those.  The one deviation from
 * MuJoCo: mj_resetData zeroes xfrc_applied, and since the caller's buffer is not written, an env that a bad state resets inside a
 * launch (mj_checkPos / mj_checkVel / mj_checkAcc) ignores the wrench for the rest of THAT launch; the next launch applies it again.
 * Like ss_set_contact_force_output (smplsim_hip.h) it selects the kernel instantiation with the optional inputs and outputs.
 * Errors as there: 0, or a negative ss_status with the message in ss_last_error(). */
int ss_set_body_wrench_input(struct ss_batch *b, const float *wrench);

#ifdef __cplusplus
}
#endif
#endif
