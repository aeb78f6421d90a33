/* etgsim_step_policy.h -- one closed-loop control step of every robot in one launch: actor, control step, auto-reset.
 *
 * The SAC data path (run_train_episode, train.py:129-179) batched as continuous collection: each call runs the actor on
 * every robot's current observation, steps every robot with that action, and restarts the robots whose episode ended,
 * keeping the observation their last step produced (the next_obs of their terminal transition).  The same library as
 * etgsim.h (its ABI version, 2, is unchanged); this header declares the one entry point that is not part of etgsim.h.
 *
 * Contract of etg_step_policy:
 *   h, policy            the simulator (after etg_reset) and a loaded policy on the same device.  The actor reads the
 *                        observation columns [obs_col0, obs_col0 + in_dim) and has 12 outputs (as etg_rollout_policy).
 *   act_scale            the action the step takes is the actor's output times act_scale (train.py:159 `action_bound`).
 *   precision            0 (fp32).  Other values are refused.
 *   auto_reset           0: obs receives the step's observation, as etg_step.  1: robots whose step ended their episode
 *                        restart (etg_step_autoreset: one launch while every robot has a cached settle, otherwise the step
 *                        followed by etg_reset masked by `done`); their obs row holds the reset observation.
 *   noise [N,12]         NULL: predict, action = tanh(mean).  Non-NULL: sample on the caller's N(0,1) draws,
 *                        action = tanh(mean + exp(clamp(log_std, -20, 2)) * noise); needs etg_policy_load_std.
 *   donef [N]            optional forced episode ends (bytes), as etg_step.
 *   obs [N,49]           in: the observation the actor acts on.  out: the next observation (reset rows for restarted robots).
 *   act [N,12]           optional: the UNSCALED action of every robot (what the replay memory stores, train.py:159).
 *   act_obs [N,49]       optional: a copy of the observation row the actor acted on.
 *   terminal_obs [N,49]  required: the step's observation of EVERY robot, before any restart (next_obs of the transition).
 *   reward [N], done [N] required; info [N,64] optional -- all three exactly as etg_step writes them.
 *   stream               hipStream_t, or NULL.
 * Pointers are device pointers.  The kernel covers the 16-lanes-per-robot mapping, num_envs % 16 == 0, POSITION / TORQUE
 * motor mode, the plain 49-float observation without sensor noise, and a policy the per-wave tile of etg_rollout_policy
 * takes (in_dim <= 64).  Anything else returns ETG_ERR_BAD_ARG with the reason in etg_last_error(); a null handle, policy,
 * obs, terminal_obs, reward or done returns ETG_ERR_BAD_ARG; a call before etg_reset, or noise without
 * etg_policy_load_std, returns ETG_ERR_STATE.                                                                       */
#ifndef ETGSIM_STEP_POLICY_H_
#define ETGSIM_STEP_POLICY_H_

#include "etgsim.h"

#ifdef __cplusplus
extern "C" {
#endif

int etg_step_policy(EtgHandle* h, EtgPolicy* policy, float act_scale, int precision, int obs_col0, int auto_reset,
                    const float* noise, const uint8_t* donef, float* obs, float* act, float* act_obs, float* terminal_obs,
                    float* reward, uint8_t* done, float* info, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ETGSIM_STEP_POLICY_H_ */
