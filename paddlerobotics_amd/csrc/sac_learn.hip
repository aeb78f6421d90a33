// sac_learn.hip -- one SAC update on the device (include/etgsim_sac.h): alg/sac.py:77-118 of the reference on
// model/mujoco_model.py (actor obs -> 256 -> 256 -> 12 + 12, two critics obs + 12 -> 256 -> 256 -> 1), fp32 throughout.
//
// The handle's common part, the arena and the launch chains of the contractions are ac_learner.h's; run_update below is the list of
// them.  What this update adds: the target critics (an arena of 2 csize floats that k_adam blends in the critics' pass), the
// elementwise kernels TD target + critic loss rows (k_td), actor loss rows (k_actor_dq) and the squashed-Gaussian sample's
// backward (k_head_bwd), and the path from the actor's loss through the critics to the action, da.
#include "ac_learner.h"

namespace {
using namespace sac;

struct Batch {
  const float *obs, *act, *rew, *nobs, *term;
  const long long* idx;
};

}  // namespace

struct EtgSac : ac::Learner {
  double gamma, tau, alpha;
  float *T, *qt, *da;                  // target critics [2 csize]; their q [2,B]; the actor loss's gradient at the action [B,12]
};

namespace {

std::vector<ac::Buf> own_buffers(EtgSac* h) {
  const size_t B = h->maxb;
  return {{(void**)&h->T, 2 * h->csize * 4}, {(void**)&h->qt, 2 * B * 4}, {(void**)&h->da, B * ACT * 4}};
}

int run_update(EtgSac* h, const Batch& b, int n, const float* eps_next, const float* eps_cur, bool apply, float* losses2,
               hipStream_t s) {
  const int d = h->d, B = h->maxb;
  const long zs = (long)h->csize, zh = (long)B * HID;
  float* PC = h->P + h->asize;   // online critics
  // ---- critic step
  ac::actor_heads(h, s, n, b.nobs, b.idx);
  ac::sample(h, s, n, eps_next);
  ac::critic_forward(h, s, n, b.nobs, b.idx, d, h->asmp, nullptr, zs, h->T, h->qt);
  ac::critic_forward(h, s, n, b.obs, b.idx, d, b.act, b.idx, zs, PC, h->q);
  hipLaunchKernelGGL(k_td, dim3((n + 255) / 256), dim3(256), 0, s, n, B, b.rew, b.term, b.idx, h->qt, h->logp, h->q,
                     (float)h->gamma, (float)h->alpha, h->dq, h->rows_c, apply ? h->steps + 1 : nullptr, h->bc + 2);
  ac::critic_backward(h, s, n, InCat<true>{b.obs, b.idx, d, b.act, b.idx, ACT});
  if (apply) ac::adam_critics(h, s, h->T, (float)(1.0 - (1.0 - h->tau)), (float)(1.0 - h->tau));
  // ---- actor step (with the critics just updated)
  ac::actor_heads(h, s, n, b.obs, b.idx);
  ac::sample(h, s, n, eps_cur);
  ac::critic_forward(h, s, n, b.obs, b.idx, d, h->asmp, nullptr, zs, PC, h->q);
  hipLaunchKernelGGL(k_actor_dq, dim3((n + 255) / 256), dim3(256), 0, s, n, B, h->q, h->logp, (float)h->alpha, h->dq, h->rows_a,
                     apply ? h->steps : nullptr, h->bc);
  // through the critics to the action: dY1 per critic, da = sum over both critics of dY1 W1[:, obs_dim:]
  ac::critic_dy1(h, s, n);
  ac::gemm(s, n, ACT, 2 * HID, 1, Cat2{h->dy1, zh}, W1Act{PC, zs, d + ACT, d}, StPlain{h->da, ACT});
  hipLaunchKernelGGL(k_head_bwd, dim3((n * ACT + 255) / 256), dim3(256), 0, s, h->head, eps_cur, h->da, n, (float)h->alpha, h->dhead);
  ac::actor_backward(h, s, n, b.obs, b.idx);
  if (apply) ac::adam_actor(h, s);
  return ac::finish(h, s, n, losses2, "etg_sac");
}

int check_batch(EtgSac* h, const Batch& b, int n, const float* e1, const float* e2, const char* who) {
  return ac::check_batch(h, n, b.obs && b.act && b.rew && b.nobs && b.term && e1 && e2, who);
}

}  // namespace

extern "C" int etg_sac_create(int obs_dim, int act_dim, int hidden, int max_batch, int device, EtgSac** out) {
  if (!out || obs_dim < 1 || obs_dim > 64 || act_dim != ACT || hidden != HID || max_batch < 1 || max_batch > (1 << 20))
    return ac::fail(ETG_ERR_BAD_ARG, "etg_sac_create: need obs_dim 1..64, act_dim 12, hidden 256, max_batch 1..2^20");
  if (int rc = ac::open_device(device, "etg_sac_create")) return rc;
  EtgSac* h = new EtgSac();
  h->gamma = 0.99; h->tau = 0.005; h->alpha = 0.2;
  int rc = ac::init(h, device, obs_dim, max_batch, "etg_sac_create");
  if (!rc) rc = ac::alloc(own_buffers(h), "etg_sac_create");
  if (rc) { etg_sac_destroy(h); return rc; }
  *out = h;
  return ETG_OK;
}

extern "C" int etg_sac_destroy(EtgSac* h) {
  if (int rc = ac::check_handle(h, "etg_sac_destroy")) return rc;
  (void)hipSetDevice(h->device);
  ac::release(ac::buffers(h));
  ac::release(own_buffers(h));
  delete h;
  return ETG_OK;
}

extern "C" int etg_sac_set_hyper(EtgSac* h, double gamma, double tau, double alpha, double actor_lr, double critic_lr) {
  if (int rc = ac::check_handle(h, "etg_sac_set_hyper")) return rc;
  h->gamma = gamma; h->tau = tau; h->alpha = alpha; h->actor_lr = actor_lr; h->critic_lr = critic_lr;
  return ETG_OK;
}

extern "C" int etg_sac_load(EtgSac* h, const float* const* tensors, int n, void* stream) {
  if (int rc = ac::load(h, tensors, n, stream, "etg_sac_load")) return rc;
  return ac::copy(h->T, h->P + h->asize, 2 * h->csize * 4, stream, "etg_sac_load");   // target = online
}

extern "C" int etg_sac_store(EtgSac* h, float* const* tensors, int n, void* stream) {
  return ac::store(h, tensors, n, stream, "etg_sac_store");
}

extern "C" int etg_sac_load_opt(EtgSac* h, const float* target, const float* exp_avg, const float* exp_avg_sq, const long long* steps,
                                void* stream) {
  if (int rc = ac::load_opt(h, exp_avg, exp_avg_sq, steps, stream, "etg_sac_load_opt")) return rc;
  return ac::copy(h->T, target, 2 * h->csize * 4, stream, "etg_sac_load_opt");
}

extern "C" int etg_sac_store_opt(EtgSac* h, float* target, float* exp_avg, float* exp_avg_sq, long long* steps, void* stream) {
  if (int rc = ac::store_opt(h, exp_avg, exp_avg_sq, steps, stream, "etg_sac_store_opt")) return rc;
  return ac::copy(target, h->T, 2 * h->csize * 4, stream, "etg_sac_store_opt");
}

extern "C" int etg_sac_learn(EtgSac* h, const float* obs, const float* act, const float* reward, const float* next_obs,
                             const float* terminal, int n, const float* eps_next, const float* eps_cur, float* losses2, void* stream) {
  const Batch b{obs, act, reward, next_obs, terminal, nullptr};
  if (int rc = check_batch(h, b, n, eps_next, eps_cur, "etg_sac_learn")) return rc;
  return run_update(h, b, n, eps_next, eps_cur, true, losses2, (hipStream_t)stream);
}

extern "C" int etg_sac_learn_replay(EtgSac* h, const float* mem_obs, const float* mem_act, const float* mem_reward,
                                    const float* mem_next_obs, const float* mem_terminal, const long long* idx, int n,
                                    const float* eps_next, const float* eps_cur, float* losses2, void* stream) {
  const Batch b{mem_obs, mem_act, mem_reward, mem_next_obs, mem_terminal, idx};
  if (int rc = check_batch(h, b, n, eps_next, eps_cur, "etg_sac_learn_replay")) return rc;
  if (!idx) return ac::fail(ETG_ERR_BAD_ARG, "etg_sac_learn_replay: null index vector");
  return run_update(h, b, n, eps_next, eps_cur, true, losses2, (hipStream_t)stream);
}

extern "C" int etg_sac_grads(EtgSac* h, const float* obs, const float* act, const float* reward, const float* next_obs,
                             const float* terminal, int n, const float* eps_next, const float* eps_cur, float* const* grads, void* stream) {
  const Batch b{obs, act, reward, next_obs, terminal, nullptr};
  if (int rc = check_batch(h, b, n, eps_next, eps_cur, "etg_sac_grads")) return rc;
  if (int rc = ac::check_tensors(grads, "etg_sac_grads", "null pointer")) return rc;
  if (int rc = run_update(h, b, n, eps_next, eps_cur, false, nullptr, (hipStream_t)stream)) return rc;
  return ac::gather(h->G, h->off, h->len, grads, stream, "etg_sac_grads");
}

extern "C" int etg_sac_sync_policy(EtgSac* h, EtgPolicy* p, void* stream) {
  return ac::sync_policy(h, p, stream, "etg_sac_sync_policy");
}
