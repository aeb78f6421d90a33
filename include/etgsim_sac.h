/* etgsim_sac.h -- the SAC learner on the device: agent.learn(batch) of the reference's training loop (alg/sac.py:77-118 on
 * model/mujoco_model.py: actor obs -> 256 -> 256 -> act + act, two critics obs + act -> 256 -> 256 -> 1).
 *
 * One update, in the reference's order and in fp32 (f32-input MFMA):
 *   critic step   a', logp' = sample(actor, next_obs; eps_next)
 *                 y = reward + gamma * terminal * (min(Q1t, Q2t)(next_obs, a') - alpha * logp')     terminal = 1 - done
 *                 L_c = mean((Q1(obs, action) - y)^2) + mean((Q2(obs, action) - y)^2),  Adam step on the 12 critic tensors
 *   actor step    a, logp = sample(actor, obs; eps_cur),  L_a = mean(alpha * logp - min(Q1, Q2)(obs, a)) with the critics just
 *                 updated,  Adam step on the 8 actor tensors
 *   target        target <- tau * online + (1 - tau) * target                                (the two target critics)
 * Adam is torch.optim.Adam with its defaults (betas 0.9 / 0.999, eps 1e-8, bias correction by the optimizer's own step count, the
 * critic and the actor optimizer counting separately).  The step counts, the moments, the losses and everything else an update
 * reads live in device memory: updates are plain launches on the caller's stream and k of them can be enqueued back to back.
 * No reduction uses floating-point atomics: the same state, batch and noise give the same bits.
 *
 * The same library as etgsim.h (its ABI version, 2, is unchanged); this header declares the entry points that are not part of
 * etgsim.h.  All data pointers are device pointers; `tensors` / `grads` are HOST arrays of 20 device pointers in the order of the
 * reference's state_dict, torch [out, in] layout:
 *   actor_model.{l1,l2,mean_linear,std_linear}.{weight,bias}  (8),  critic_model.{l1 .. l6}.{weight,bias}  (12).
 * Errors: ETG_ERR_BAD_ARG with a message in etg_last_error() for a null handle, n < 1, n > max_batch, a null required pointer,
 * unsupported dimensions (obs_dim 1..64, act_dim 12, hidden 256) or a policy whose dimensions differ.                          */
#ifndef ETGSIM_SAC_H_
#define ETGSIM_SAC_H_

#include "etgsim.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct EtgSac EtgSac;

#define ETG_SAC_TENSORS 20

int etg_sac_create(int obs_dim, int act_dim, int hidden, int max_batch, int device, EtgSac** out);
int etg_sac_destroy(EtgSac* h);
/* may be called between updates; an update uses the values in force when it is enqueued */
int etg_sac_set_hyper(EtgSac* h, double gamma, double tau, double alpha, double actor_lr, double critic_lr);
/* load: the 20 online tensors; also sets target = online (sync_target(decay=0)) and zeroes Adam's moments and step counts */
int etg_sac_load(EtgSac* h, const float* const* tensors, int n, void* stream);
int etg_sac_store(EtgSac* h, float* const* tensors, int n, void* stream);
/* resuming a run: target (the 12 critic tensors, flat, in state_dict order), exp_avg and exp_avg_sq (all 20 tensors, flat, in
 * state_dict order), steps[2] = {actor optimizer's step count, critic optimizer's}; a NULL pointer skips that part */
int etg_sac_load_opt(EtgSac* h, const float* target, const float* exp_avg, const float* exp_avg_sq, const long long* steps,
                     void* stream);
int etg_sac_store_opt(EtgSac* h, float* target, float* exp_avg, float* exp_avg_sq, long long* steps, void* stream);
/* one update on the caller's batch: obs / next_obs [n, obs_dim], act [n, act_dim], reward / terminal [n], eps_* [n, act_dim]
 * N(0,1) draws; losses2 (may be NULL) receives {critic loss, actor loss} */
int etg_sac_learn(EtgSac* h, const float* obs, const float* act, const float* reward, const float* next_obs,
                  const float* terminal, int n, const float* eps_next, const float* eps_cur, float* losses2, void* stream);
/* the same on rows idx[0..n) of a replay ring (rows are read in place, nothing is gathered) */
int etg_sac_learn_replay(EtgSac* h, const float* mem_obs, const float* mem_act, const float* mem_reward,
                         const float* mem_next_obs, const float* mem_terminal, const long long* idx, int n,
                         const float* eps_next, const float* eps_cur, float* losses2, void* stream);
/* test hook: the 20 gradients of the update that etg_sac_learn would apply, the actor's taken at the CURRENT critics; no
 * parameter, moment or step count changes */
int etg_sac_grads(EtgSac* h, const float* obs, const float* act, const float* reward, const float* next_obs,
                  const float* terminal, int n, const float* eps_next, const float* eps_cur, float* const* grads, void* stream);
/* etg_policy_load + etg_policy_load_std from the current actor, device to device */
int etg_sac_sync_policy(EtgSac* h, EtgPolicy* p, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ETGSIM_SAC_H_ */
