/* etgsim_bc.h -- the behaviour-cloning learner on the device: BClearn(obs, ref_obs, ref_agent) of the reference's third training
 * stage (alg/BC.py:53-72 on model/mujoco_model.py), a student (actor obs -> 256 -> 256 -> act + act, two critics) distilled from
 * a frozen teacher of the same architecture on an observation of its own width.
 *
 * One update, in the reference's order and in fp32 (f32-input MFMA):
 *   actor step    mean, log_std = actor(obs) (log_std clamped to [-20, 2]),  a_ref = tanh(teacher actor's mean(ref_obs))
 *                 L_a = -mean over all n * act_dim elements of Normal(mean, exp(log_std)).log_prob(a_ref),
 *                 Adam step on the 8 actor tensors.  eps_a is the draw the reference's sample() consumes here; it does not enter
 *                 the loss and is not read
 *   critic step   a_now = tanh(mean' + exp(log_std') * eps_c) from the actor just updated,  rq1, rq2 = teacher critics(ref_obs, a_now)
 *                 L_c = mean((Q1(obs, a_now) - rq1)^2) + mean((Q2(obs, a_now) - rq2)^2),  Adam step on the 12 critic tensors
 * There is no target network.  Adam is torch.optim.Adam with its defaults, the two optimizers counting their steps separately.
 * Step counts, moments and losses live in device memory: updates are plain launches on the caller's stream, nothing waits for
 * the host, and no reduction uses floating-point atomics -- the same state, batch and noise give the same bits.
 *
 * The same library as etgsim.h (ABI version 2, unchanged).  All data pointers are device pointers; `tensors` / `grads` are HOST
 * arrays of 20 device pointers in the order of the reference's state_dict (etgsim_sac.h).
 * Errors: ETG_ERR_BAD_ARG with a message in etg_last_error() for a null handle, n < 1, n > max_batch, a null required pointer,
 * unsupported dimensions (both observation widths 1..64, act_dim 12, hidden 256) or a policy whose dimensions differ;
 * ETG_ERR_STATE for an update before etg_bc_set_teacher.                                                                        */
#ifndef ETGSIM_BC_H_
#define ETGSIM_BC_H_

#include "etgsim_sac.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct EtgBc EtgBc;

#define ETG_BC_TENSORS 20

int etg_bc_create(int student_obs_dim, int teacher_obs_dim, int act_dim, int hidden, int max_batch, int device, EtgBc** out);
int etg_bc_destroy(EtgBc* h);
/* may be called between updates; an update uses the values in force when it is enqueued */
int etg_bc_set_hyper(EtgBc* h, double actor_lr, double critic_lr);
/* the student's 20 tensors; load also zeroes Adam's moments and step counts */
int etg_bc_load(EtgBc* h, const float* const* tensors, int n, void* stream);
int etg_bc_store(EtgBc* h, float* const* tensors, int n, void* stream);
/* resuming a run: exp_avg and exp_avg_sq (all 20 tensors, flat, in state_dict order), steps[2] = {actor optimizer's step count,
 * critic optimizer's}; a NULL pointer skips that part */
int etg_bc_load_opt(EtgBc* h, const float* exp_avg, const float* exp_avg_sq, const long long* steps, void* stream);
int etg_bc_store_opt(EtgBc* h, float* exp_avg, float* exp_avg_sq, long long* steps, void* stream);
/* a device-to-device COPY of the teacher's 20 tensors (observation width teacher_obs_dim) into the handle: later changes of the
 * caller's tensors do not reach the learner until this is called again.  Of the 20, l1, l2, the mean head and the two critics
 * are read by an update */
int etg_bc_set_teacher(EtgBc* h, const float* const* tensors, void* stream);
/* one update: obs [n, student_obs_dim], ref_obs [n, teacher_obs_dim], eps_a (not read; may be NULL) and eps_c [n, act_dim]
 * N(0,1) draws; losses2 (may be NULL) receives {critic loss, actor loss} */
int etg_bc_learn(EtgBc* h, const float* obs, const float* ref_obs, int n, const float* eps_a, const float* eps_c, float* losses2,
                 void* stream);
/* the same on rows idx[0..n) of a pair memory (obs field = student observation, action field = teacher observation), read in
 * place */
int etg_bc_learn_replay(EtgBc* h, const float* mem_obs, const float* mem_ref_obs, const long long* idx, int n, const float* eps_a,
                        const float* eps_c, float* losses2, void* stream);
/* test hook: the 20 gradients of the update etg_bc_learn would apply, the critics' taken with a_now from the CURRENT actor; no
 * parameter, moment or step count changes */
int etg_bc_grads(EtgBc* h, const float* obs, const float* ref_obs, int n, const float* eps_a, const float* eps_c,
                 float* const* grads, void* stream);
/* etg_policy_load + etg_policy_load_std from the student's current actor, device to device */
int etg_bc_sync_policy(EtgBc* h, EtgPolicy* p, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ETGSIM_BC_H_ */
