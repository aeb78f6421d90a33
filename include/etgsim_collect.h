/* etgsim_collect.h -- n_steps closed-loop control steps of every robot, restarts included, in one launch.
 *
 * Continuous SAC collection (run_train_episode, train.py:129-179, batched without episode boundaries) takes one
 * etg_step_policy launch per control step, and a launch lasts as long as its slowest wave.  etg_collect_policy keeps a wave
 * with its 4 robots for n_steps control steps: per step the actor on the robots' current rows, the control step, the records
 * of the transition, and the restart of a robot whose episode ended; the next step acts on the reset row.  One call with
 * n_steps = K leaves bit for bit what K calls with n_steps = 1 leave: records, obs and the simulator's state.  The same
 * library as etgsim.h (its ABI version, 2, is unchanged); this header declares the one entry point that is not part of it.
 *
 * Contract of etg_collect_policy:
 *   h, policy            the simulator (after etg_reset) and a loaded policy on the same device, as etg_step_policy.
 *   act_scale            the action a step takes is the actor's output times act_scale.
 *   precision            0 (fp32).  Other values are refused.
 *   obs_col0             the actor reads the observation columns [obs_col0, obs_col0 + in_dim).
 *   n_steps              K >= 1 control steps.
 *   bootstrap_from       rec_terminal is 1 from this (1-based) episode step on whatever `done` says (train.py:148-149: 2000).
 *   noise [K,N,12]       NULL: predict, action = tanh(mean).  Non-NULL: sample on the caller's N(0,1) draws,
 *                        action = tanh(mean + exp(clamp(log_std, -20, 2)) * noise); needs etg_policy_load_std.
 *   donef [K,N]          optional forced episode ends (bytes) per step, as etg_step.
 *   obs [N,49]           in: the rows the first step acts on.  out: the rows the next step would act on (reset rows of the
 *                        robots the last step restarted).
 *   rec_obs [K,N,49]     the rows each step's actor acted on.
 *   rec_action [K,N,12]  the UNSCALED action of each step (what the replay memory stores, train.py:159).
 *   rec_reward [K,N], rec_done [K,N] (bytes)   as etg_step writes them.
 *   rec_next_obs [K,N,49]  each step's observation of EVERY robot before any restart (next_obs of the transition).
 *   rec_terminal [K,N]   the bootstrap flag of the transition: ep_len >= bootstrap_from ? 1 : 1 - done.
 *   rec_ep_ret [K,N], rec_ep_len [K,N] (int32)   the robot's episode return and 1-based episode step after the step, before
 *                        a restart.
 *   stream               hipStream_t, or NULL.
 * Pointers are device pointers; all eight record arrays are required.  The kernel covers what etg_step_policy covers (the
 * 16-lanes-per-robot mapping, num_envs % 16 == 0, POSITION / TORQUE motor mode, no sensor noise, in_dim <= 64) with a fused
 * restart: every robot needs a cached settle, and a handle with prepared next-episode dynamics (etg_prepare_next_dynamics)
 * is refused -- a second restart inside the launch would find no prepared row.  Every refusal comes before any launch and
 * leaves the handle as it was: ETG_ERR_BAD_ARG for a null handle, policy, obs or record array, n_steps < 1 and what
 * etg_step_policy refuses with it; ETG_ERR_STATE for a call before etg_reset, noise without etg_policy_load_std, prepared
 * next-episode dynamics, or a robot without a cached settle.  The reason is in etg_last_error().  The sensor-noise stream
 * advances by 2 * n_steps, as n_steps etg_step_policy calls with a fused restart advance it.                          */
#ifndef ETGSIM_COLLECT_H_
#define ETGSIM_COLLECT_H_

#include "etgsim.h"

#ifdef __cplusplus
extern "C" {
#endif

int etg_collect_policy(EtgHandle* h, EtgPolicy* policy, float act_scale, int precision, int obs_col0, int n_steps,
                       int bootstrap_from, const float* noise, const uint8_t* donef, float* obs, float* rec_obs,
                       float* rec_action, float* rec_reward, uint8_t* rec_done, float* rec_next_obs, float* rec_terminal,
                       float* rec_ep_ret, int32_t* rec_ep_len, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ETGSIM_COLLECT_H_ */
