// bc_learn.hip -- one behaviour-cloning update on the device (include/etgsim_bc.h): alg/BC.py:53-72 of the reference on
// model/mujoco_model.py, a student of observation width ds distilled from a frozen teacher of width dt, fp32 throughout.
//
// The pieces are the SAC learner's (sac_core.h, and ac_learner.h for the host side): every contraction is sac::k_gemm with its
// loader / store functors, the sample is k_sample, Adam is k_adam without a target, the losses are reduced by k_loss.  What this
// update adds (bc_core.h): the teacher's tanh(mean), the Gaussian negative log-likelihood's backward at the head, and the critics'
// regression onto the teacher's critics.  There is no target network.  The launch list of one update (31 launches and one 8-byte copy):
//   actor step    teacher actor l1, l2, mean head (3 gemm), k_tanh                          -> aref
//                 student actor l1, l2, heads (3 gemm), k_nll_bwd                           -> dhead, loss rows, actor step count
//                 head dW, dh2, l2 dW, dh1, l1 dW (5 gemm), k_adam on the actor's region
//   critic step   student actor again (3 gemm), k_sample with eps_c                         -> a_now
//                 teacher critics on [ref_obs | a_now] (3 gemm, grid.z = 2)                 -> rq   (first: it shares ch1 / ch2)
//                 student critics on [obs | a_now] (3 gemm)                                 -> q, ch1, ch2 kept for the backward
//                 k_regress, dW3, dW2, dY1, dW1 (4 gemm), k_adam on both critics' region
//   k_loss
//
// The student is the handle's common part (ac_learner.h: d = ds); the teacher's 20 tensors lie in an arena of the same layout for
// width dt.
#include "../../include/etgsim_bc.h"
#include "bc_core.h"
#include "ac_learner.h"

static_assert(ETG_BC_TENSORS == ac::TENSORS, "one layout for the student and the teacher");

namespace {
using namespace sac;

struct Pairs {
  const float *obs, *ref;
  const long long* idx;
};

}  // namespace

struct EtgBc : ac::Learner {
  int dt;
  bool teacher;
  size_t tasize, tcsize;               // floats: the teacher's actor, ONE of its critics
  float *TP, *aref, *rq;               // the teacher's parameters [toff[20]]; its tanh(mean) [B,12]; its critics' q [2,B]
  size_t toff[ETG_BC_TENSORS + 1], tlen[ETG_BC_TENSORS];
};

namespace {

std::vector<ac::Buf> own_buffers(EtgBc* h) {
  const size_t B = h->maxb;
  return {{(void**)&h->TP, h->toff[ETG_BC_TENSORS] * 4}, {(void**)&h->aref, B * ACT * 4}, {(void**)&h->rq, 2 * B * 4}};
}

int run_update(EtgBc* h, const Pairs& b, int n, const float* eps_c, bool apply, float* losses2, hipStream_t s) {
  const int ds = h->d, dt = h->dt, B = h->maxb;
  // ---- actor step
  const float* thw = ac::actor_hidden(h, s, n, b.ref, b.idx, dt, h->TP);
  ac::gemm(s, n, ACT, HID, 1, Mat<false>{h->ah2, 0, HID}, Mat<false>{thw, 0, HID}, StAct<false>{h->aref, 0, ACT, thw + (size_t)ACT * HID, 0});
  hipLaunchKernelGGL(bc::k_tanh, dim3((n * ACT + 255) / 256), dim3(256), 0, s, h->aref, n * ACT);
  ac::actor_heads(h, s, n, b.obs, b.idx);
  hipLaunchKernelGGL(bc::k_nll_bwd, dim3((n + 15) / 16), dim3(256), 0, s, h->head, h->aref, n, h->dhead, h->rows_a,
                     apply ? h->steps : nullptr, h->bc);
  ac::actor_backward(h, s, n, b.obs, b.idx);
  if (apply) ac::adam_actor(h, s);
  // ---- critic step (with the actor just updated)
  ac::actor_heads(h, s, n, b.obs, b.idx);
  ac::sample(h, s, n, eps_c);
  ac::critic_forward(h, s, n, b.ref, b.idx, dt, h->asmp, nullptr, (long)h->tcsize, h->TP + h->tasize, h->rq);
  ac::critic_forward(h, s, n, b.obs, b.idx, ds, h->asmp, nullptr, (long)h->csize, h->P + h->asize, h->q);
  hipLaunchKernelGGL(bc::k_regress, dim3((n + 255) / 256), dim3(256), 0, s, n, B, h->q, h->rq, h->dq, h->rows_c,
                     apply ? h->steps + 1 : nullptr, h->bc + 2);
  ac::critic_backward(h, s, n, InCat<true>{b.obs, b.idx, ds, h->asmp, nullptr, ACT});
  if (apply) ac::adam_critics(h, s);
  return ac::finish(h, s, n, losses2, "etg_bc");
}

int check_batch(EtgBc* h, const Pairs& b, int n, const float* eps_c, const char* who) {
  if (int rc = ac::check_batch(h, n, b.obs && b.ref && eps_c, who)) return rc;
  return h->teacher ? ETG_OK : ac::fail(ETG_ERR_STATE, who, "no teacher has been set (etg_bc_set_teacher)");
}

}  // namespace

extern "C" int etg_bc_create(int student_obs_dim, int teacher_obs_dim, int act_dim, int hidden, int max_batch, int device, EtgBc** out) {
  if (!out || student_obs_dim < 1 || student_obs_dim > 64 || teacher_obs_dim < 1 || teacher_obs_dim > 64 || act_dim != ACT ||
      hidden != HID || max_batch < 1 || max_batch > (1 << 20))
    return ac::fail(ETG_ERR_BAD_ARG, "etg_bc_create: need student and teacher obs_dim 1..64, act_dim 12, hidden 256, max_batch 1..2^20");
  if (int rc = ac::open_device(device, "etg_bc_create")) return rc;
  EtgBc* h = new EtgBc();
  h->dt = teacher_obs_dim;
  ac::layout(h->dt, h->toff, h->tlen);
  h->tasize = h->toff[8]; h->tcsize = h->toff[14] - h->toff[8];
  int rc = ac::init(h, device, student_obs_dim, max_batch, "etg_bc_create");
  if (!rc) rc = ac::alloc(own_buffers(h), "etg_bc_create");
  if (rc) { etg_bc_destroy(h); return rc; }
  *out = h;
  return ETG_OK;
}

extern "C" int etg_bc_destroy(EtgBc* h) {
  if (int rc = ac::check_handle(h, "etg_bc_destroy")) return rc;
  (void)hipSetDevice(h->device);
  ac::release(ac::buffers(h));
  ac::release(own_buffers(h));
  delete h;
  return ETG_OK;
}

extern "C" int etg_bc_set_hyper(EtgBc* h, double actor_lr, double critic_lr) {
  if (int rc = ac::check_handle(h, "etg_bc_set_hyper")) return rc;
  h->actor_lr = actor_lr; h->critic_lr = critic_lr;
  return ETG_OK;
}

extern "C" int etg_bc_load(EtgBc* h, const float* const* tensors, int n, void* stream) {
  return ac::load(h, tensors, n, stream, "etg_bc_load");
}

extern "C" int etg_bc_store(EtgBc* h, float* const* tensors, int n, void* stream) {
  return ac::store(h, tensors, n, stream, "etg_bc_store");
}

extern "C" int etg_bc_load_opt(EtgBc* h, const float* exp_avg, const float* exp_avg_sq, const long long* steps, void* stream) {
  return ac::load_opt(h, exp_avg, exp_avg_sq, steps, stream, "etg_bc_load_opt");
}

extern "C" int etg_bc_store_opt(EtgBc* h, float* exp_avg, float* exp_avg_sq, long long* steps, void* stream) {
  return ac::store_opt(h, exp_avg, exp_avg_sq, steps, stream, "etg_bc_store_opt");
}

extern "C" int etg_bc_set_teacher(EtgBc* h, const float* const* tensors, void* stream) {
  if (int rc = ac::check_handle(h, "etg_bc_set_teacher")) return rc;
  if (int rc = ac::check_tensors(tensors, "etg_bc_set_teacher", "need the teacher's 20 tensors")) return rc;
  if (int rc = ac::set_device(h)) return rc;
  if (int rc = ac::scatter(h->TP, h->toff, h->tlen, tensors, stream, "etg_bc_set_teacher")) return rc;
  h->teacher = true;
  return ETG_OK;
}

extern "C" int etg_bc_learn(EtgBc* h, const float* obs, const float* ref_obs, int n, const float* eps_a, const float* eps_c,
                            float* losses2, void* stream) {
  (void)eps_a;   // drawn by the reference's sample() in the actor step; the loss does not depend on it
  const Pairs b{obs, ref_obs, nullptr};
  if (int rc = check_batch(h, b, n, eps_c, "etg_bc_learn")) return rc;
  return run_update(h, b, n, eps_c, true, losses2, (hipStream_t)stream);
}

extern "C" int etg_bc_learn_replay(EtgBc* h, const float* mem_obs, const float* mem_ref_obs, const long long* idx, int n,
                                   const float* eps_a, const float* eps_c, float* losses2, void* stream) {
  (void)eps_a;
  const Pairs b{mem_obs, mem_ref_obs, idx};
  if (int rc = check_batch(h, b, n, eps_c, "etg_bc_learn_replay")) return rc;
  if (!idx) return ac::fail(ETG_ERR_BAD_ARG, "etg_bc_learn_replay: null index vector");
  return run_update(h, b, n, eps_c, true, losses2, (hipStream_t)stream);
}

extern "C" int etg_bc_grads(EtgBc* h, const float* obs, const float* ref_obs, int n, const float* eps_a, const float* eps_c,
                            float* const* grads, void* stream) {
  (void)eps_a;
  const Pairs b{obs, ref_obs, nullptr};
  if (int rc = check_batch(h, b, n, eps_c, "etg_bc_grads")) return rc;
  if (int rc = ac::check_tensors(grads, "etg_bc_grads", "null pointer")) return rc;
  if (int rc = run_update(h, b, n, eps_c, false, nullptr, (hipStream_t)stream)) return rc;
  return ac::gather(h->G, h->off, h->len, grads, stream, "etg_bc_grads");
}

extern "C" int etg_bc_sync_policy(EtgBc* h, EtgPolicy* p, void* stream) {
  return ac::sync_policy(h, p, stream, "etg_bc_sync_policy");
}
