/* etgsim_ppo.h -- the on-policy learner on the device: PPO (clipped surrogate) with GAE on the model of the other two learners
 * (actor obs -> 256 -> 256 -> act + act, two critics obs + act -> 256 -> 256 -> 1), fp32 throughout.  The definition is
 * paddlerobotics_amd/ppo.py (DevicePPO(fused=False)) and DESIGN.md "The PPO learner"; in short:
 *
 *   value         V(s) = (Q1 + Q2)(s, 0) / 2: the twin critic on [obs | 12 zeros].  The zeros are a buffer of the handle that
 *                 nothing writes, so the action columns of the critics' first layers get an exactly zero gradient and never move
 *   prepare       head_old = (mean, raw log_std) of the current actor on the rollout's obs,
 *                 logp_old = sum_c (-eps^2 / 2 - ls - log sqrt(2 pi)),  ls = clamp(raw log_std, -20, 2)   (the exact-eps form),
 *                 v = V(obs), v_next = V(next_obs) of every row
 *   gae           backwards over t with A_T = 0, every product and sum rounded on its own (no fma):
 *                   delta_t = (r_t + (gamma * terminal_t) * v_next_t) - v_t
 *                   A_t     = delta_t + (gamma_lam * (1 - done_t)) * A_{t+1},      ret_t = A_t + v_t
 *   norm_adv      A <- (A - mean) / (std + 1e-8), population mean and std accumulated in double in a fixed order
 *   one update    z = ((mean_old - mean) + exp(ls_old) eps) exp(-ls),  logp = sum_c (-z^2 / 2 - ls - log sqrt(2 pi)),
 *                 rho = exp(logp - logp_old)                                  (the pre-squash Gaussian: tanh's Jacobian cancels)
 *                 L_a = -mean(min(rho A, clip(rho, 1 - c, 1 + c) A)) - ent_coef mean(sum_c (ls + 1/2 + log sqrt(2 pi))),
 *                 Adam step on the 8 actor tensors;
 *                 L_v = mean((Q1(obs, 0) - ret)^2) + mean((Q2(obs, 0) - ret)^2),  Adam step on the 12 critic tensors
 *                 stats4 = {L_v, L_a, approx_kl = mean(logp_old - logp), clip_frac = mean(|rho - 1| > c)}
 * Adam is torch.optim.Adam with its defaults, the two optimizers counting their steps separately.  Step counts, moments, the
 * rollout's buffers and the stats live in device memory: every call enqueues plain launches on the caller's stream, nothing waits
 * for the host, and no reduction uses floating-point atomics -- the same state, rollout and index vectors give the same bits.
 *
 * The same library as etgsim.h (ABI version 2, unchanged).  All data pointers are device pointers; `tensors` / `grads` are HOST
 * arrays of 20 device pointers in the order of the model's state_dict (actor l1, l2, mean, std, then the critics' l1 .. l6, weight
 * before bias).
 * Errors: ETG_ERR_BAD_ARG with a message in etg_last_error() for a null handle, a row count outside its range (n outside
 * 1..max_batch for an update, outside 1..max_rollout for the rollout's calls), a null required pointer, unsupported dimensions
 * (obs_dim 1..64, act_dim 12, hidden 256) or a policy whose dimensions differ.                                                   */
#ifndef ETGSIM_PPO_H_
#define ETGSIM_PPO_H_

#include "etgsim_sac.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct EtgPpo EtgPpo;

#define ETG_PPO_TENSORS 20
#define ETG_PPO_STATS 4

/* max_batch: the most rows of one update (and of one chunk of prepare); max_rollout: the most rows T * N of a rollout */
int etg_ppo_create(int obs_dim, int act_dim, int hidden, int max_batch, int max_rollout, int device, EtgPpo** out);
int etg_ppo_destroy(EtgPpo* h);
/* may be called between updates; an update uses the values in force when it is enqueued */
int etg_ppo_set_hyper(EtgPpo* h, double actor_lr, double critic_lr, double clip, double ent_coef);
/* the 20 tensors; load also zeroes Adam's moments and step counts */
int etg_ppo_load(EtgPpo* h, const float* const* tensors, int n, void* stream);
int etg_ppo_store(EtgPpo* h, float* const* tensors, int n, void* stream);
/* resuming a run: exp_avg and exp_avg_sq (all 20 tensors, flat, in state_dict order), steps[2] = {actor optimizer's step count,
 * critic optimizer's}; a NULL pointer skips that part */
int etg_ppo_load_opt(EtgPpo* h, const float* exp_avg, const float* exp_avg_sq, const long long* steps, void* stream);
int etg_ppo_store_opt(EtgPpo* h, float* exp_avg, float* exp_avg_sq, long long* steps, void* stream);
/* etg_policy_load + etg_policy_load_std from the current actor, device to device */
int etg_ppo_sync_policy(EtgPpo* h, EtgPolicy* p, void* stream);

/* the rollout's buffers of the handle from n = T * N rows, step-major: obs / next_obs [n, obs_dim], eps [n, act_dim] the N(0,1)
 * draws the actions were sampled with.  Writes head_old [n, 24], logp_old, v, v_next [n]; runs in chunks of max_batch rows */
int etg_ppo_prepare(EtgPpo* h, const float* obs, const float* next_obs, const float* eps, int n, void* stream);
/* reward, terminal [T, N] float, done [T, N] bytes (0 / 1); gamma and gamma_lam as the caller rounded them to fp32.
 * v, v_next, adv, ret [T, N]: all four given, or all four NULL = the handle's buffers (then T * N <= max_rollout, after prepare) */
int etg_ppo_gae(EtgPpo* h, const float* reward, const float* terminal, const unsigned char* done, int T, int N, float gamma,
                float gamma_lam, const float* v, const float* v_next, float* adv, float* ret, void* stream);
/* in place on adv [n]; NULL = the handle's adv */
int etg_ppo_norm_adv(EtgPpo* h, float* adv, int n, void* stream);
/* what the handle's rollout buffers hold in their first n rows, copied out; a NULL pointer skips that part */
int etg_ppo_fetch(EtgPpo* h, int n, float* head_old, float* logp_old, float* v, float* v_next, float* adv, float* ret, void* stream);

/* one update on the caller's n contiguous rows: obs [n, obs_dim], head_old [n, 24], eps [n, act_dim], logp_old, adv, ret [n];
 * stats4 (may be NULL) receives {value loss, policy loss, approx_kl, clip_frac} */
int etg_ppo_learn(EtgPpo* h, const float* obs, const float* head_old, const float* eps, const float* logp_old, const float* adv,
                  const float* ret, int n, float* stats4, void* stream);
/* the same on rows idx[0..n) of the rollout: obs and eps are the arrays etg_ppo_prepare was given, the other four the handle's
 * buffers; every row is read in place through idx (values in 0 .. rows prepared - 1; repeats allowed), nothing is gathered */
int etg_ppo_learn_rows(EtgPpo* h, const float* obs, const float* eps, const long long* idx, int n, float* stats4, void* stream);
/* test hook: the 20 gradients of the update etg_ppo_learn would apply (the critics' do not depend on the actor's step); no
 * parameter, moment or step count changes */
int etg_ppo_grads(EtgPpo* h, const float* obs, const float* head_old, const float* eps, const float* logp_old, const float* adv,
                  const float* ret, int n, float* const* grads, void* stream);

/* ---- Controls: gradient-norm clipping, value clipping and a KL rule, all off (0) by default.  With all three off every entry
 * point above enqueues the launches and gives the bits it gave before these existed.  With one on, an update's clip coefficient,
 * its learning-rate scale and whether it is applied at all are decided ON THE DEVICE, from device memory, so an update still
 * enqueues plain launches, waits for nothing and gives the same bits from the same inputs.  (The entry points of this part carry
 * a 2 in their names: the 15 above are the base list, which stays as it is.)
 *
 *   max_grad_norm  per optimizer (the actor's 8 tensors, then the critics' 12): sq = the sum of squares of the group's gradients
 *                  accumulated in double in a fixed order, norm = (float) sqrt(sq), coef = min(1, max_grad_norm / (norm + 1e-6)) in
 *                  fp32, every gradient * coef, rounded once, before Adam            (torch.nn.utils.clip_grad_norm_)
 *   clip_value     PPO2's clipped value loss against v_old, the value at collection time.  Per critic i: d = Q_i - v_old,
 *                  inside = |d| <= c, vclip = v_old + clamp(d, -c, c), e1 = (Q_i - ret)^2, e2 = (vclip - ret)^2; the row's loss is e1
 *                  with dQ_i = 2 (Q_i - ret) / n where inside or e1 >= e2, otherwise e2, a constant of the row, with dQ_i = 0.
 *                  stats4[0] is the mean of the chosen terms, summed over the critics
 *   target_kl      judged between the actor's backward pass and its Adam step on kl = this update's approx_kl, summed as stats4[2] is:
 *                    ETG_PPO_KL_STOP      kl > 1.5 target_kl sets the stop flag.  While it is set an update still evaluates its
 *                                         losses and stats, but parameters, moments and step counts of both optimizers stay
 *                                         as they are.  etg_ppo2_reset_stop clears it
 *                    ETG_PPO_KL_ADAPTIVE  kl > 2 target_kl: lr_scale /= 1.5; else 0 < kl < target_kl / 2: lr_scale *= 1.5; then
 *                                         lr_scale is clamped so that actor_lr * lr_scale lies in [lr_lo, lr_hi].  Both optimizers
 *                                         step with lr * lr_scale (a double; the product in double), from this update on
 * Errors, beside the ones above: ETG_ERR_BAD_ARG for a negative or non-finite setting, lr_lo > lr_hi, an unknown mode (all three
 * checked before the handle), and for an update with value clipping on and no v_old.                                              */
#define ETG_PPO_KL_STOP 0
#define ETG_PPO_KL_ADAPTIVE 1

/* may be called between updates, like etg_ppo_set_hyper */
int etg_ppo2_set_controls(EtgPpo* h, double max_grad_norm, double clip_value, double target_kl, int kl_mode, double lr_lo, double lr_hi);
/* etg_ppo_learn / etg_ppo_grads with v_old [n] (may be NULL while value clipping is off).  etg_ppo_learn_rows needs no variant:
 * it reads the handle's v, which etg_ppo_prepare wrote, through idx.  The gradients of etg_ppo2_grads are the unclipped ones */
int etg_ppo2_learn(EtgPpo* h, const float* obs, const float* head_old, const float* eps, const float* logp_old, const float* adv,
                   const float* ret, const float* v_old, int n, float* stats4, void* stream);
int etg_ppo2_grads(EtgPpo* h, const float* obs, const float* head_old, const float* eps, const float* logp_old, const float* adv,
                   const float* ret, const float* v_old, int n, float* const* grads, void* stream);
/* clears the stop flag: enqueued, nothing waits */
int etg_ppo2_reset_stop(EtgPpo* h, void* stream);
/* the control state.  set: lr_scale (> 0) and the stop flag, enqueued.  get WAITS for the stream, then reads into HOST memory (a
 * NULL pointer skips that part): lr_scale, the stop flag, steps2 = both optimizers' step counts, grad_norms2 = the actor's and
 * the critics' gradient norm of the last applied update with gradient clipping on (0 before the first) */
int etg_ppo2_set_state(EtgPpo* h, double lr_scale, int stopped, void* stream);
int etg_ppo2_get_state(EtgPpo* h, double* lr_scale, int* stopped, long long* steps2, double* grad_norms2, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ETGSIM_PPO_H_ */
