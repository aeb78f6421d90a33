// ppo_learn.hip -- the on-policy learner on the device (include/etgsim_ppo.h): PPO's clipped surrogate with GAE on the model of
// the SAC and BC learners, fp32 throughout.  The definition is paddlerobotics_amd/ppo.py (DevicePPO(fused=False)).
//
// The pieces are the SAC learner's (sac_core.h, and ac_learner.h for the host side): every contraction is sac::k_gemm with its
// loader / store functors and Adam is k_adam without a target.  What this learner adds (ppo_core.h): the rollout's preparation
// (old head, logp_old, V of obs and next_obs), the GAE scan, the advantage normalisation, the clipped surrogate's backward at the
// head, the value regression onto the return, and the four stats.  V(s) = (Q1 + Q2)(s, 0) / 2: the critics' action input is
// h->zact, [max_batch, 12] zeros that nothing writes, through the InCat loader.  The launch list of one update (20 launches and one
// 16-byte copy):
//   actor step    actor l1, l2, heads (3 gemm), k_ppo_bwd                                    -> dhead, loss / kl / clip rows, actor step count
//                 head dW, dh2, l2 dW, dh1, l1 dW (5 gemm), k_adam on the actor's region
//   value step    critics on [obs | 0] (3 gemm), k_value_dq                                  -> dq, loss rows, critic step count
//                 dW3, dW2, dY1, dW1 (4 gemm), k_adam on both critics' region
//   k_ppo_stats
// etg_ppo_learn_rows reads the rollout's rows in place: obs and eps through idx in the first layers' loaders and in k_ppo_bwd, the
// handle's head_old, logp_old, adv and ret through idx in k_ppo_bwd / k_value_dq.
// With a control on (etg_ppo2_set_controls: gradient-norm clipping, value clipping, a KL rule) the list is run_update_ctl's: the
// same contractions, k_ppo_ctl after the actor's backward pass, k_sqnorm + k_adam_ctl for k_adam, k_value_dq_clip for k_value_dq
// (23 launches).  With none on, the list above is enqueued exactly as it was.
#include "../../include/etgsim_ppo.h"
#include "ppo_core.h"
#include "ac_learner.h"

#include <cfloat>
#include <cstring>

static_assert(ETG_PPO_TENSORS == ac::TENSORS, "one layout for the three learners");

namespace {
using namespace sac;

struct Rows {   // the rows of one update: the caller's contiguous ones, or the rollout's through idx
  const float *obs, *head_old, *eps, *logp_old, *adv, *ret;
  const long long* idx;
  const float* v_old = nullptr;        // the value at collection time: read when value clipping is on
};

}  // namespace

struct EtgPpo : ac::Learner {
  int maxr;                            // the most rows of a rollout
  double clip, ent_coef;
  float* zact;                         // the zero action [B,12]: nothing writes it
  float *head_old, *logp_old, *v, *vn, *adv, *ret;   // the rollout: [R,24], [R] x 5
  float *rows_kl, *rows_clip, *stats;  // per-row stats [B] x 2; {value loss, policy loss, approx_kl, clip_frac}
  double* red;                         // the advantage statistics' partial sums [2 * RED_BLOCKS]
  // the controls (etg_ppo2_set_controls; 0 = off) and their device state
  double max_grad_norm, clip_value, target_kl, lr_lo, lr_hi;
  int kl_mode;                         // 0 stop, 1 adaptive
  double* part;                        // squared-norm partials [2 * NORM_BLOCKS]: the actor's, the critics'
  double* ctl;                         // [4]: lr_scale, the actor's and the critics' gradient norm of the last applied step
  int* flag;                           // [2]: flag[0] = the updates are stopped
};

namespace {

std::vector<ac::Buf> own_buffers(EtgPpo* h) {
  const size_t B = h->maxb, R = h->maxr;
  return {{(void**)&h->zact, B * ACT * 4}, {(void**)&h->head_old, R * 2 * ACT * 4}, {(void**)&h->logp_old, R * 4}, {(void**)&h->v, R * 4},
          {(void**)&h->vn, R * 4}, {(void**)&h->adv, R * 4}, {(void**)&h->ret, R * 4}, {(void**)&h->rows_kl, B * 4},
          {(void**)&h->rows_clip, B * 4}, {(void**)&h->stats, ETG_PPO_STATS * 4}, {(void**)&h->red, 2 * ppo::RED_BLOCKS * 8},
          {(void**)&h->part, 2 * ppo::NORM_BLOCKS * 8}, {(void**)&h->ctl, 4 * 8}, {(void**)&h->flag, 2 * 4}};
}

// V of n <= max_batch rows of x: the twin critic on [x | 0], halved sum
void value(EtgPpo* h, hipStream_t s, int n, const float* x, float* out) {
  ac::critic_forward(h, s, n, x, nullptr, h->d, h->zact, nullptr, (long)h->csize, h->P + h->asize, h->q);
  hipLaunchKernelGGL(ppo::k_value, dim3((n + 255) / 256), dim3(256), 0, s, n, h->maxb, h->q, out);
}

int launched(const char* who) {
  return hipGetLastError() == hipSuccess ? ETG_OK : ac::fail(ETG_ERR_HIP, who, "a launch failed");
}

// the library is built with -ffinite-math-only, under which isfinite() folds to true, and so does a test of the exponent's bits
// that the optimiser recognises as one (it caught NaN and let infinity through): the bits are read through a volatile
bool finite_bits(double v) {
  volatile unsigned long long u;
  memcpy((void*)&u, &v, 8);
  return ((u >> 52) & 0x7ff) != 0x7ff;
}

bool controlled(const EtgPpo* h) { return h->max_grad_norm > 0.0 || h->clip_value > 0.0 || h->target_kl > 0.0; }

// both critics' value regression on the controlled path: k_value_dq without a step count, or its clipped variant
void value_dq(EtgPpo* h, hipStream_t s, int n, const Rows& b) {
  if (h->clip_value > 0.0)
    hipLaunchKernelGGL(ppo::k_value_dq_clip, dim3((n + 255) / 256), dim3(256), 0, s, n, h->maxb, h->q, b.ret, b.v_old, b.idx,
                       (float)h->clip_value, h->dq, h->rows_c);
  else
    hipLaunchKernelGGL(ppo::k_value_dq, dim3((n + 255) / 256), dim3(256), 0, s, n, h->maxb, h->q, b.ret, b.idx, h->dq, h->rows_c,
                       (long long*)nullptr, h->bc + 2);
}

// Adam on one of the two regions under the controls: the squared-norm reduction first when gradient clipping is on
void adam_ctl(EtgPpo* h, hipStream_t s, int which) {
  const size_t o = which ? h->asize : 0;
  const long n = which ? (long)(2 * h->csize) : (long)h->asize;
  double* part = nullptr;
  if (h->max_grad_norm > 0.0) {
    part = h->part + which * ppo::NORM_BLOCKS;
    hipLaunchKernelGGL(ppo::k_sqnorm, dim3(ppo::NORM_BLOCKS), dim3(256), 0, s, h->G + o, n, part);
  }
  hipLaunchKernelGGL(ppo::k_adam_ctl, dim3(512), dim3(256), 0, s, h->P + o, h->G + o, h->M + o, h->V + o, n,
                     which ? h->critic_lr : h->actor_lr, h->bc + 2 * which, part, (float)h->max_grad_norm, h->ctl, h->flag,
                     h->ctl + 1 + which);
}

// The update with a control on.  The launch list of run_update with: null step pointers (the controller counts the steps, and only
// of an update that is applied), k_ppo_ctl after the actor's backward pass, k_sqnorm + k_adam_ctl in k_adam's place, and
// k_value_dq_clip in k_value_dq's when value clipping is on.  apply = false (etg_ppo_grads) judges nothing and counts nothing.
int run_update_ctl(EtgPpo* h, const Rows& b, int n, bool apply, float* stats4, hipStream_t s) {
  const int B = h->maxb;
  ac::actor_heads(h, s, n, b.obs, b.idx);
  hipLaunchKernelGGL(ppo::k_ppo_bwd, dim3((n + 15) / 16), dim3(256), 0, s, h->head, b.head_old, b.eps, b.logp_old, b.adv, b.idx, n,
                     (float)h->clip, (float)h->ent_coef, h->dhead, h->rows_a, h->rows_kl, h->rows_clip, (long long*)nullptr, h->bc);
  ac::actor_backward(h, s, n, b.obs, b.idx);
  if (apply) {
    const bool bounded = h->actor_lr > 0.0;
    hipLaunchKernelGGL(ppo::k_ppo_ctl, dim3(1), dim3(256), 0, s, n, h->rows_kl, h->target_kl, h->kl_mode,
                       bounded ? h->lr_lo / h->actor_lr : 0.0, bounded ? h->lr_hi / h->actor_lr : DBL_MAX, h->ctl, h->flag, h->steps, h->bc);
    adam_ctl(h, s, 0);
  }
  ac::critic_forward(h, s, n, b.obs, b.idx, h->d, h->zact, nullptr, (long)h->csize, h->P + h->asize, h->q);
  value_dq(h, s, n, b);
  ac::critic_backward(h, s, n, InCat<true>{b.obs, b.idx, h->d, h->zact, nullptr, ACT});
  if (apply) adam_ctl(h, s, 1);
  hipLaunchKernelGGL(ppo::k_ppo_stats, dim3(1), dim3(256), 0, s, n, B, h->rows_c, h->rows_a, h->rows_kl, h->rows_clip, h->stats);
  if (stats4 && hipMemcpyAsync(stats4, h->stats, ETG_PPO_STATS * 4, hipMemcpyDeviceToDevice, s) != hipSuccess)
    return ac::fail(ETG_ERR_HIP, "etg_ppo", "copying the stats failed");
  return launched("etg_ppo");
}

int run_update(EtgPpo* h, const Rows& b, int n, bool apply, float* stats4, hipStream_t s) {
  if (controlled(h)) return run_update_ctl(h, b, n, apply, stats4, s);
  const int B = h->maxb;
  // ---- actor step
  ac::actor_heads(h, s, n, b.obs, b.idx);
  hipLaunchKernelGGL(ppo::k_ppo_bwd, dim3((n + 15) / 16), dim3(256), 0, s, h->head, b.head_old, b.eps, b.logp_old, b.adv, b.idx, n,
                     (float)h->clip, (float)h->ent_coef, h->dhead, h->rows_a, h->rows_kl, h->rows_clip, apply ? h->steps : nullptr, h->bc);
  ac::actor_backward(h, s, n, b.obs, b.idx);
  if (apply) ac::adam_actor(h, s);
  // ---- value step
  ac::critic_forward(h, s, n, b.obs, b.idx, h->d, h->zact, nullptr, (long)h->csize, h->P + h->asize, h->q);
  hipLaunchKernelGGL(ppo::k_value_dq, dim3((n + 255) / 256), dim3(256), 0, s, n, B, h->q, b.ret, b.idx, h->dq, h->rows_c,
                     apply ? h->steps + 1 : nullptr, h->bc + 2);
  ac::critic_backward(h, s, n, InCat<true>{b.obs, b.idx, h->d, h->zact, nullptr, ACT});
  if (apply) ac::adam_critics(h, s);
  hipLaunchKernelGGL(ppo::k_ppo_stats, dim3(1), dim3(256), 0, s, n, B, h->rows_c, h->rows_a, h->rows_kl, h->rows_clip, h->stats);
  if (stats4 && hipMemcpyAsync(stats4, h->stats, ETG_PPO_STATS * 4, hipMemcpyDeviceToDevice, s) != hipSuccess)
    return ac::fail(ETG_ERR_HIP, "etg_ppo", "copying the stats failed");
  return launched("etg_ppo");
}

int check_rows(EtgPpo* h, int n, bool ptrs, const char* who) {   // a rollout's row count and pointers, then the device
  static thread_local char msg[160];
  if (int rc = ac::check_handle(h, who)) return rc;
  if (n < 1 || n > h->maxr) { snprintf(msg, sizeof msg, "%s: %d rows outside 1..max_rollout = %d", who, n, h->maxr); return ac::fail(ETG_ERR_BAD_ARG, msg); }
  if (!ptrs) return ac::fail(ETG_ERR_BAD_ARG, who, "null pointer");
  return ac::set_device(h);
}

}  // namespace

extern "C" int etg_ppo_create(int obs_dim, int act_dim, int hidden, int max_batch, int max_rollout, int device, EtgPpo** out) {
  if (!out || obs_dim < 1 || obs_dim > 64 || act_dim != ACT || hidden != HID || max_batch < 1 || max_batch > (1 << 20) ||
      max_rollout < 1 || max_rollout > (1 << 24))
    return ac::fail(ETG_ERR_BAD_ARG, "etg_ppo_create: need obs_dim 1..64, act_dim 12, hidden 256, max_batch 1..2^20, max_rollout 1..2^24");
  if (int rc = ac::open_device(device, "etg_ppo_create")) return rc;
  EtgPpo* h = new EtgPpo();
  h->maxr = max_rollout; h->clip = 0.2; h->ent_coef = 0.0;
  int rc = ac::init(h, device, obs_dim, max_batch, "etg_ppo_create");
  if (!rc) rc = ac::alloc(own_buffers(h), "etg_ppo_create");
  h->lr_lo = 1e-5; h->lr_hi = 1e-2;
  const double one = 1.0;                                   // lr_scale
  if (!rc && hipMemcpy(h->ctl, &one, 8, hipMemcpyHostToDevice) != hipSuccess) rc = ac::fail(ETG_ERR_HIP, "etg_ppo_create", "hipMemcpy failed");
  if (rc) { etg_ppo_destroy(h); return rc; }
  *out = h;
  return ETG_OK;
}

extern "C" int etg_ppo_destroy(EtgPpo* h) {
  if (int rc = ac::check_handle(h, "etg_ppo_destroy")) return rc;
  (void)hipSetDevice(h->device);
  ac::release(ac::buffers(h));
  ac::release(own_buffers(h));
  delete h;
  return ETG_OK;
}

extern "C" int etg_ppo_set_hyper(EtgPpo* h, double actor_lr, double critic_lr, double clip, double ent_coef) {
  if (int rc = ac::check_handle(h, "etg_ppo_set_hyper")) return rc;
  h->actor_lr = actor_lr; h->critic_lr = critic_lr; h->clip = clip; h->ent_coef = ent_coef;
  return ETG_OK;
}

extern "C" int etg_ppo_load(EtgPpo* h, const float* const* tensors, int n, void* stream) {
  return ac::load(h, tensors, n, stream, "etg_ppo_load");
}

extern "C" int etg_ppo_store(EtgPpo* h, float* const* tensors, int n, void* stream) {
  return ac::store(h, tensors, n, stream, "etg_ppo_store");
}

extern "C" int etg_ppo_load_opt(EtgPpo* h, const float* exp_avg, const float* exp_avg_sq, const long long* steps, void* stream) {
  return ac::load_opt(h, exp_avg, exp_avg_sq, steps, stream, "etg_ppo_load_opt");
}

extern "C" int etg_ppo_store_opt(EtgPpo* h, float* exp_avg, float* exp_avg_sq, long long* steps, void* stream) {
  return ac::store_opt(h, exp_avg, exp_avg_sq, steps, stream, "etg_ppo_store_opt");
}

extern "C" int etg_ppo_sync_policy(EtgPpo* h, EtgPolicy* p, void* stream) {
  return ac::sync_policy(h, p, stream, "etg_ppo_sync_policy");
}

extern "C" int etg_ppo_prepare(EtgPpo* h, const float* obs, const float* next_obs, const float* eps, int n, void* stream) {
  if (int rc = check_rows(h, n, obs && next_obs && eps, "etg_ppo_prepare")) return rc;
  hipStream_t s = (hipStream_t)stream;
  for (int o = 0; o < n; o += h->maxb) {
    const int m = n - o < h->maxb ? n - o : h->maxb;
    const float* x = obs + (size_t)o * h->d;
    ac::actor_heads(h, s, m, x, nullptr);
    hipLaunchKernelGGL(ppo::k_ppo_prepare, dim3((m + 15) / 16), dim3(256), 0, s, h->head, eps + (size_t)o * ACT, m,
                       h->head_old + (size_t)o * 2 * ACT, h->logp_old + o);
    value(h, s, m, x, h->v + o);
    value(h, s, m, next_obs + (size_t)o * h->d, h->vn + o);
  }
  return launched("etg_ppo_prepare");
}

extern "C" int etg_ppo_gae(EtgPpo* h, const float* reward, const float* terminal, const unsigned char* done, int T, int N, float gamma,
                           float gamma_lam, const float* v, const float* v_next, float* adv, float* ret, void* stream) {
  if (int rc = ac::check_handle(h, "etg_ppo_gae")) return rc;
  const bool own = !v && !v_next && !adv && !ret;
  const long long rows = (long long)T * N;
  if (T < 1 || N < 1 || rows > (1LL << 30)) return ac::fail(ETG_ERR_BAD_ARG, "etg_ppo_gae: need T >= 1, N >= 1, T * N <= 2^30");
  if (!own && !(v && v_next && adv && ret)) return ac::fail(ETG_ERR_BAD_ARG, "etg_ppo_gae: v, v_next, adv and ret are given together or not at all");
  if (own) {
    if (rows > h->maxr) return ac::fail(ETG_ERR_BAD_ARG, "etg_ppo_gae: T * N rows exceed max_rollout, the size of the handle's buffers");
    v = h->v; v_next = h->vn; adv = h->adv; ret = h->ret;
  }
  if (!reward || !terminal || !done) return ac::fail(ETG_ERR_BAD_ARG, "etg_ppo_gae", "null pointer");
  if (int rc = ac::set_device(h)) return rc;
  hipLaunchKernelGGL(ppo::k_gae, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, T, N, reward, terminal, done, v, v_next, gamma,
                     gamma_lam, adv, ret);
  return launched("etg_ppo_gae");
}

extern "C" int etg_ppo_norm_adv(EtgPpo* h, float* adv, int n, void* stream) {
  if (int rc = ac::check_handle(h, "etg_ppo_norm_adv")) return rc;
  if (adv) {
    if (n < 1) return ac::fail(ETG_ERR_BAD_ARG, "etg_ppo_norm_adv: need n >= 1");
    if (int rc = ac::set_device(h)) return rc;
  } else {
    if (int rc = check_rows(h, n, true, "etg_ppo_norm_adv")) return rc;
    adv = h->adv;
  }
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(ppo::k_adv_stats, dim3(ppo::RED_BLOCKS), dim3(256), 0, s, adv, (long)n, h->red);
  const int blocks = (n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024;
  hipLaunchKernelGGL(ppo::k_adv_apply, dim3(blocks), dim3(256), 0, s, adv, (long)n, h->red);
  return launched("etg_ppo_norm_adv");
}

extern "C" int etg_ppo_fetch(EtgPpo* h, int n, float* head_old, float* logp_old, float* v, float* v_next, float* adv, float* ret,
                             void* stream) {
  if (int rc = check_rows(h, n, true, "etg_ppo_fetch")) return rc;
  const size_t r = (size_t)n * 4;
  if (int rc = ac::copy(head_old, h->head_old, r * 2 * ACT, stream, "etg_ppo_fetch")) return rc;
  if (int rc = ac::copy(logp_old, h->logp_old, r, stream, "etg_ppo_fetch")) return rc;
  if (int rc = ac::copy(v, h->v, r, stream, "etg_ppo_fetch")) return rc;
  if (int rc = ac::copy(v_next, h->vn, r, stream, "etg_ppo_fetch")) return rc;
  if (int rc = ac::copy(adv, h->adv, r, stream, "etg_ppo_fetch")) return rc;
  return ac::copy(ret, h->ret, r, stream, "etg_ppo_fetch");
}

namespace {

// the bodies of etg_ppo_learn / etg_ppo2_learn and of etg_ppo_grads / etg_ppo2_grads: v_old is required when value clipping is on
int learn(EtgPpo* h, const float* obs, const float* head_old, const float* eps, const float* logp_old, const float* adv, const float* ret,
          const float* v_old, int n, float* stats4, void* stream, const char* who) {
  if (int rc = ac::check_batch(h, n, obs && head_old && eps && logp_old && adv && ret, who)) return rc;
  if (h->clip_value > 0.0 && !v_old) return ac::fail(ETG_ERR_BAD_ARG, who, "value clipping is on and v_old is null");
  return run_update(h, Rows{obs, head_old, eps, logp_old, adv, ret, nullptr, v_old}, n, true, stats4, (hipStream_t)stream);
}

int grads(EtgPpo* h, const float* obs, const float* head_old, const float* eps, const float* logp_old, const float* adv, const float* ret,
          const float* v_old, int n, float* const* out, void* stream, const char* who) {
  if (int rc = ac::check_batch(h, n, obs && head_old && eps && logp_old && adv && ret, who)) return rc;
  if (int rc = ac::check_tensors(out, who, "null pointer")) return rc;
  if (h->clip_value > 0.0 && !v_old) return ac::fail(ETG_ERR_BAD_ARG, who, "value clipping is on and v_old is null");
  if (int rc = run_update(h, Rows{obs, head_old, eps, logp_old, adv, ret, nullptr, v_old}, n, false, nullptr, (hipStream_t)stream)) return rc;
  return ac::gather(h->G, h->off, h->len, out, stream, who);
}

}  // namespace

extern "C" int etg_ppo_learn(EtgPpo* h, const float* obs, const float* head_old, const float* eps, const float* logp_old, const float* adv,
                             const float* ret, int n, float* stats4, void* stream) {
  return learn(h, obs, head_old, eps, logp_old, adv, ret, nullptr, n, stats4, stream, "etg_ppo_learn");
}

extern "C" int etg_ppo_learn_rows(EtgPpo* h, const float* obs, const float* eps, const long long* idx, int n, float* stats4, void* stream) {
  if (int rc = ac::check_batch(h, n, obs && eps, "etg_ppo_learn_rows")) return rc;
  if (!idx) return ac::fail(ETG_ERR_BAD_ARG, "etg_ppo_learn_rows: null index vector");
  return run_update(h, Rows{obs, h->head_old, eps, h->logp_old, h->adv, h->ret, idx, h->v}, n, true, stats4, (hipStream_t)stream);
}

extern "C" int etg_ppo_grads(EtgPpo* h, const float* obs, const float* head_old, const float* eps, const float* logp_old, const float* adv,
                             const float* ret, int n, float* const* out, void* stream) {
  return grads(h, obs, head_old, eps, logp_old, adv, ret, nullptr, n, out, stream, "etg_ppo_grads");
}

// ------------------------------------------------------------------------------------------------- the controls
extern "C" int etg_ppo2_set_controls(EtgPpo* h, double max_grad_norm, double clip_value, double target_kl, int kl_mode, double lr_lo,
                                     double lr_hi) {
  const char* who = "etg_ppo2_set_controls";
  const double x[5] = {max_grad_norm, clip_value, target_kl, lr_lo, lr_hi};
  for (double v : x)
    if (!finite_bits(v) || v < 0.0) return ac::fail(ETG_ERR_BAD_ARG, who, "a setting is negative or not finite");
  if (lr_lo > lr_hi) return ac::fail(ETG_ERR_BAD_ARG, who, "the learning-rate bounds have lo > hi");
  if (kl_mode != ETG_PPO_KL_STOP && kl_mode != ETG_PPO_KL_ADAPTIVE) return ac::fail(ETG_ERR_BAD_ARG, who, "unknown KL mode");
  if (int rc = ac::check_handle(h, who)) return rc;
  h->max_grad_norm = max_grad_norm; h->clip_value = clip_value; h->target_kl = target_kl; h->kl_mode = kl_mode;
  h->lr_lo = lr_lo; h->lr_hi = lr_hi;
  return ETG_OK;
}

extern "C" int etg_ppo2_learn(EtgPpo* h, const float* obs, const float* head_old, const float* eps, const float* logp_old, const float* adv,
                              const float* ret, const float* v_old, int n, float* stats4, void* stream) {
  return learn(h, obs, head_old, eps, logp_old, adv, ret, v_old, n, stats4, stream, "etg_ppo2_learn");
}

extern "C" int etg_ppo2_grads(EtgPpo* h, const float* obs, const float* head_old, const float* eps, const float* logp_old, const float* adv,
                              const float* ret, const float* v_old, int n, float* const* out, void* stream) {
  return grads(h, obs, head_old, eps, logp_old, adv, ret, v_old, n, out, stream, "etg_ppo2_grads");
}

extern "C" int etg_ppo2_reset_stop(EtgPpo* h, void* stream) {
  if (int rc = ac::check_handle(h, "etg_ppo2_reset_stop")) return rc;
  if (int rc = ac::set_device(h)) return rc;
  hipLaunchKernelGGL(ppo::k_ctl_set, dim3(1), dim3(64), 0, (hipStream_t)stream, h->ctl, h->flag, 2, 0.0, 0);
  return launched("etg_ppo2_reset_stop");
}

extern "C" int etg_ppo2_set_state(EtgPpo* h, double lr_scale, int stopped, void* stream) {
  const char* who = "etg_ppo2_set_state";
  if (!finite_bits(lr_scale) || lr_scale <= 0.0) return ac::fail(ETG_ERR_BAD_ARG, who, "lr_scale must be positive and finite");
  if (int rc = ac::check_handle(h, who)) return rc;
  if (int rc = ac::set_device(h)) return rc;
  hipLaunchKernelGGL(ppo::k_ctl_set, dim3(1), dim3(64), 0, (hipStream_t)stream, h->ctl, h->flag, 3, lr_scale, stopped ? 1 : 0);
  return launched(who);
}

extern "C" int etg_ppo2_get_state(EtgPpo* h, double* lr_scale, int* stopped, long long* steps2, double* grad_norms2, void* stream) {
  const char* who = "etg_ppo2_get_state";
  if (int rc = ac::check_handle(h, who)) return rc;
  if (int rc = ac::set_device(h)) return rc;
  double c[3];
  int f = 0;
  long long st[2];
  const bool ok = hipStreamSynchronize((hipStream_t)stream) == hipSuccess && hipMemcpy(c, h->ctl, sizeof c, hipMemcpyDeviceToHost) == hipSuccess &&
                  hipMemcpy(&f, h->flag, sizeof f, hipMemcpyDeviceToHost) == hipSuccess &&
                  hipMemcpy(st, h->steps, sizeof st, hipMemcpyDeviceToHost) == hipSuccess;
  if (!ok) return ac::fail(ETG_ERR_HIP, who, "reading the control state failed");
  if (lr_scale) *lr_scale = c[0];
  if (stopped) *stopped = f;
  if (steps2) { steps2[0] = st[0]; steps2[1] = st[1]; }
  if (grad_norms2) { grad_norms2[0] = c[1]; grad_norms2[1] = c[2]; }
  return ETG_OK;
}
