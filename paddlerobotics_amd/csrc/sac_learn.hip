// sac_learn.hip -- one SAC update on the device (include/etgsim_sac.h): alg/sac.py:77-118 of the reference on
// model/mujoco_model.py (actor obs -> 256 -> 256 -> 12 + 12, two critics obs + 12 -> 256 -> 256 -> 1), fp32 throughout.
//
// Every contraction of the update -- forward Y = X W^T, input gradient dX = dY W, weight gradient dW = dY^T X -- is the ONE
// tiled kernel k_gemm (sac_core.h: 32 x 32 output tile per workgroup, v_mfma_f32_16x16x4_f32, the whole reduction inside the
// workgroup, so no split K and no atomics); what differs between the uses is how an operand element is fetched and how a
// result element is stored, and those are small functors:
//   * the first layers read [obs | action] (and the replay ring through an index vector) in their loader, nothing is gathered
//     or concatenated in memory;
//   * bias + ReLU, the ReLU mask of the backward pass and the bias gradient are epilogues / loaders: the bias gradient is the
//     column of dW that a ones column appended to X produces;
//   * dY of a critic's second layer, dq * w3 * [h2 > 0], is formed by the loader from the 256 -> 1 layer's weights;
//   * the two critics are grid.z = 2 of one launch in every pass.
// The elementwise kernels: squashed-Gaussian sample and its backward, TD target + critic loss rows, actor loss rows, a
// fixed-order loss reduction, Adam (+ soft target update) over the flat parameter arena.
//
// Arena (floats), state_dict order: actor l1.w l1.b l2.w l2.b mean.w mean.b std.w std.b | critic l1.w l1.b l2.w l2.b l3.w l3.b
// l4.w .. l6.b.  Q2's tensors lie one critic's size after Q1's, so a per-critic pointer is base + z * csize.
#include <hip/hip_runtime.h>

#include "../../include/etgsim_sac.h"
#include "policy_core.h"
#include "sac_core.h"

extern "C" void etg_set_last_error_(const char* msg);

namespace {
using namespace sac;

int sfail(int code, const char* msg) {
  etg_set_last_error_(msg);
  return code;
}

struct Batch {
  const float *obs, *act, *rew, *nobs, *term;
  const long long* idx;
};

}  // namespace

struct EtgSac {
  int device, d, maxb;
  double gamma, tau, alpha, actor_lr, critic_lr;
  size_t asize, csize, total;          // floats: the actor, ONE critic, everything
  float *P, *G, *M, *V, *T;            // parameters, gradients, Adam moments [total]; target critics [2 csize]
  float *ah1, *ah2, *head, *asmp, *logp;                  // actor pass: [B,256] x 2, [B,24], [B,12], [B]
  float *ch1, *ch2, *q, *qt, *dq, *dy1;                   // critic passes: [2,B,256] x 2, [2,B] x 3, [2,B,256]
  float *da, *dhead, *dh2, *dh1, *rows_c, *rows_a;        // actor backward: [B,12], [B,24], [B,256] x 2; loss rows [2,B], [B]
  float* losses;                                          // [2]
  long long* steps;                                       // [2]: actor, critic optimizer
  double* bc;                                             // [4]: 1 - beta1^t, sqrt(1 - beta2^t) of actor, critic
  size_t off[ETG_SAC_TENSORS], len[ETG_SAC_TENSORS];
};

namespace {

template <class FA, class FB, class ST>
void gemm(hipStream_t s, int M, int N, int K, int Z, FA fa, FB fb, ST st) {
  dim3 grid((N + TN - 1) / TN, (M + TM - 1) / TM, Z);
  hipLaunchKernelGGL((k_gemm<FA, FB, ST>), grid, dim3(256), 0, s, M, N, K, fa, fb, st);
}

// critic forward on [obs rows | act rows] with the weights at `w` (online arena or target): h1, h2 -> h->ch1, h->ch2, q -> qout
void critic_forward(EtgSac* h, hipStream_t s, int n, const float* obs, const long long* oidx, const float* act,
                    const long long* aidx, const float* w, float* qout) {
  const int d = h->d, kin = d + ACT;
  const long zs = (long)h->csize, zh = (long)h->maxb * HID;
  const float* l1w = w;
  const float* l1b = l1w + (size_t)HID * kin;
  const float* l2w = l1b + HID;
  const float* l2b = l2w + (size_t)HID * HID;
  const float* l3w = l2b + HID;
  const float* l3b = l3w + HID;
  gemm(s, n, HID, kin, 2, InCat<false>{obs, oidx, d, act, aidx, ACT}, Mat<false>{l1w, zs, kin},
       StAct<true>{h->ch1, zh, HID, l1b, zs});
  gemm(s, n, HID, HID, 2, Mat<false>{h->ch1, zh, HID}, Mat<false>{l2w, zs, HID}, StAct<true>{h->ch2, zh, HID, l2b, zs});
  gemm(s, n, 1, HID, 2, Mat<false>{h->ch2, zh, HID}, Mat<false>{l3w, zs, HID}, StAct<false>{qout, (long)h->maxb, 1, l3b, zs});
}

// actor forward + sample on obs rows: h->ah1, h->ah2, h->head, h->asmp, h->logp
void actor_forward(EtgSac* h, hipStream_t s, int n, const float* obs, const long long* oidx, const float* eps) {
  const int d = h->d;
  const float* l1w = h->P;
  const float* l1b = l1w + (size_t)HID * d;
  const float* l2w = l1b + HID;
  const float* l2b = l2w + (size_t)HID * HID;
  const float* hw = l2b + HID;
  gemm(s, n, HID, d, 1, InCat<false>{obs, oidx, d, nullptr, nullptr, 0}, Mat<false>{l1w, 0, d}, StAct<true>{h->ah1, 0, HID, l1b, 0});
  gemm(s, n, HID, HID, 1, Mat<false>{h->ah1, 0, HID}, Mat<false>{l2w, 0, HID}, StAct<true>{h->ah2, 0, HID, l2b, 0});
  gemm(s, n, 2 * ACT, HID, 1, Mat<false>{h->ah2, 0, HID}, HeadW<false>{hw}, StHead{h->head, hw});
  hipLaunchKernelGGL(k_sample, dim3((n + 15) / 16), dim3(256), 0, s, h->head, eps, n, h->asmp, h->logp);
}

int run_update(EtgSac* h, const Batch& b, int n, const float* eps_next, const float* eps_cur, bool apply, float* losses2,
               hipStream_t s) {
  const int d = h->d, kin = d + ACT, B = h->maxb;
  const long zs = (long)h->csize, zh = (long)B * HID;
  float* PC = h->P + h->asize;   // online critics
  float* GC = h->G + h->asize;
  // ---- critic step
  actor_forward(h, s, n, b.nobs, b.idx, eps_next);
  critic_forward(h, s, n, b.nobs, b.idx, h->asmp, nullptr, h->T, h->qt);
  critic_forward(h, s, n, b.obs, b.idx, b.act, b.idx, PC, h->q);
  hipLaunchKernelGGL(k_td, dim3((n + 255) / 256), dim3(256), 0, s, n, B, b.rew, b.term, b.idx, h->qt, h->logp, h->q,
                     (float)h->gamma, (float)h->alpha, h->dq, h->rows_c, apply ? h->steps + 1 : nullptr, h->bc + 2);
  {
    const size_t o_l1w = 0, o_l2w = (size_t)HID * kin + HID, o_l3w = o_l2w + (size_t)HID * HID + HID;
    // dW3 | db3 = dq^T [h2 | 1]
    gemm(s, 1, HID + 1, n, 2, Mat<true>{h->dq, (long)B, 1}, MatAug{h->ch2, zh, HID, HID}, StGrad{GC + o_l3w, zs, 1, HID, 0});
    // dW2 | db2 = dY2^T [h1 | 1],  dY2 = dq w3 [h2 > 0]
    DQ<true> dy2t{h->dq, (long)B, PC + o_l3w, zs, h->ch2, zh};
    gemm(s, HID, HID + 1, n, 2, dy2t, MatAug{h->ch1, zh, HID, HID}, StGrad{GC + o_l2w, zs, HID, HID, 0});
    // dY1 = (dY2 W2) [h1 > 0]
    DQ<false> dy2{h->dq, (long)B, PC + o_l3w, zs, h->ch2, zh};
    gemm(s, n, HID, HID, 2, dy2, Mat<true>{PC + o_l2w, zs, HID}, StMask{h->dy1, zh, HID, h->ch1});
    // dW1 | db1 = dY1^T [obs | act | 1]
    gemm(s, HID, kin + 1, n, 2, Mat<true>{h->dy1, zh, HID}, InCat<true>{b.obs, b.idx, d, b.act, b.idx, ACT},
         StGrad{GC + o_l1w, zs, HID, kin, 0});
  }
  if (apply)
    hipLaunchKernelGGL(k_adam, dim3(512), dim3(256), 0, s, PC, GC, h->M + h->asize, h->V + h->asize, (long)(2 * h->csize),
                       h->critic_lr, h->bc + 2, h->T, (float)(1.0 - (1.0 - h->tau)), (float)(1.0 - h->tau));
  // ---- actor step (with the critics just updated)
  actor_forward(h, s, n, b.obs, b.idx, eps_cur);
  critic_forward(h, s, n, b.obs, b.idx, h->asmp, nullptr, PC, h->q);
  hipLaunchKernelGGL(k_actor_dq, dim3((n + 255) / 256), dim3(256), 0, s, n, B, h->q, h->logp, (float)h->alpha, h->dq, h->rows_a,
                     apply ? h->steps : nullptr, h->bc);
  {
    const size_t c_l2w = (size_t)HID * kin + HID, c_l3w = c_l2w + (size_t)HID * HID + HID;
    // through the critics to the action: dY1 = (dY2 W2) [h1 > 0] per critic, da = sum over both critics of dY1 W1[:, obs_dim:]
    DQ<false> dy2{h->dq, (long)B, PC + c_l3w, zs, h->ch2, zh};
    gemm(s, n, HID, HID, 2, dy2, Mat<true>{PC + c_l2w, zs, HID}, StMask{h->dy1, zh, HID, h->ch1});
    gemm(s, n, ACT, 2 * HID, 1, Cat2{h->dy1, zh}, W1Act{PC, zs, kin, d}, StPlain{h->da, ACT});
    hipLaunchKernelGGL(k_head_bwd, dim3((n * ACT + 255) / 256), dim3(256), 0, s, h->head, eps_cur, h->da, n, (float)h->alpha,
                       h->dhead);
    const size_t a_l2w = (size_t)HID * d + HID, a_hw = a_l2w + (size_t)HID * HID + HID;
    // head: dW | db of both heads = dhead^T [h2 | 1];  dh2 = (dhead Whead) [h2 > 0]
    gemm(s, 2 * ACT, HID + 1, n, 1, Mat<true>{h->dhead, 0, 2 * ACT}, MatAug{h->ah2, 0, HID, HID},
         StGrad{h->G + a_hw, 0, ACT, HID, (long)ACT * HID + ACT});
    gemm(s, n, HID, 2 * ACT, 1, Mat<false>{h->dhead, 0, 2 * ACT}, HeadW<true>{h->P + a_hw}, StMask{h->dh2, 0, HID, h->ah2});
    gemm(s, HID, HID + 1, n, 1, Mat<true>{h->dh2, 0, HID}, MatAug{h->ah1, 0, HID, HID}, StGrad{h->G + a_l2w, 0, HID, HID, 0});
    gemm(s, n, HID, HID, 1, Mat<false>{h->dh2, 0, HID}, Mat<true>{h->P + a_l2w, 0, HID}, StMask{h->dh1, 0, HID, h->ah1});
    gemm(s, HID, d + 1, n, 1, Mat<true>{h->dh1, 0, HID}, InCat<true>{b.obs, b.idx, d, nullptr, nullptr, 0},
         StGrad{h->G, 0, HID, d, 0});
  }
  if (apply)
    hipLaunchKernelGGL(k_adam, dim3(512), dim3(256), 0, s, h->P, h->G, h->M, h->V, (long)h->asize, h->actor_lr, h->bc,
                       (float*)nullptr, 0.0f, 0.0f);
  hipLaunchKernelGGL(k_loss, dim3(1), dim3(256), 0, s, n, B, h->rows_c, h->rows_a, h->losses);
  if (losses2 && hipMemcpyAsync(losses2, h->losses, 8, hipMemcpyDeviceToDevice, s) != hipSuccess)
    return sfail(ETG_ERR_HIP, "etg_sac: copying the losses failed");
  if (hipGetLastError() != hipSuccess) return sfail(ETG_ERR_HIP, "etg_sac: a launch failed");
  return ETG_OK;
}

int check_batch(EtgSac* h, const Batch& b, int n, const float* e1, const float* e2, const char* who) {
  static thread_local char msg[160];
  if (!h) { snprintf(msg, sizeof msg, "%s: null handle", who); return sfail(ETG_ERR_BAD_ARG, msg); }
  if (n < 1 || n > h->maxb) { snprintf(msg, sizeof msg, "%s: n = %d outside 1..max_batch = %d", who, n, h->maxb); return sfail(ETG_ERR_BAD_ARG, msg); }
  if (!b.obs || !b.act || !b.rew || !b.nobs || !b.term || !e1 || !e2) { snprintf(msg, sizeof msg, "%s: null pointer", who); return sfail(ETG_ERR_BAD_ARG, msg); }
  if (hipSetDevice(h->device) != hipSuccess) return sfail(ETG_ERR_HIP, "hipSetDevice");
  return ETG_OK;
}

}  // namespace

extern "C" int etg_sac_create(int obs_dim, int act_dim, int hidden, int max_batch, int device, EtgSac** out) {
  if (!out || obs_dim < 1 || obs_dim > 64 || act_dim != ACT || hidden != HID || max_batch < 1 || max_batch > (1 << 20))
    return sfail(ETG_ERR_BAD_ARG, "etg_sac_create: need obs_dim 1..64, act_dim 12, hidden 256, max_batch 1..2^20");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return sfail(ETG_ERR_NO_DEVICE, "etg_sac_create: no HIP device");
  if (device < 0 || device >= ndev) return sfail(ETG_ERR_BAD_ARG, "etg_sac_create: bad device");
  if (hipSetDevice(device) != hipSuccess) return sfail(ETG_ERR_HIP, "hipSetDevice");
  EtgSac* h = new EtgSac();
  h->device = device; h->d = obs_dim; h->maxb = max_batch;
  h->gamma = 0.99; h->tau = 0.005; h->alpha = 0.2; h->actor_lr = 3e-4; h->critic_lr = 3e-4;
  const size_t d = obs_dim, kin = d + ACT;
  const size_t lens[ETG_SAC_TENSORS] = {HID * d, HID, (size_t)HID * HID, HID, ACT * HID, ACT, ACT * HID, ACT,
                                        HID * kin, HID, (size_t)HID * HID, HID, HID, 1, HID * kin, HID, (size_t)HID * HID, HID, HID, 1};
  size_t o = 0;
  for (int i = 0; i < ETG_SAC_TENSORS; i++) { h->off[i] = o; h->len[i] = lens[i]; o += lens[i]; }
  h->total = o; h->asize = h->off[8]; h->csize = h->off[14] - h->off[8];
  const size_t B = max_batch;
  struct { void** p; size_t bytes; } a[] = {
      {(void**)&h->P, h->total * 4}, {(void**)&h->G, h->total * 4}, {(void**)&h->M, h->total * 4}, {(void**)&h->V, h->total * 4},
      {(void**)&h->T, 2 * h->csize * 4}, {(void**)&h->ah1, B * HID * 4}, {(void**)&h->ah2, B * HID * 4}, {(void**)&h->head, B * 2 * ACT * 4},
      {(void**)&h->asmp, B * ACT * 4}, {(void**)&h->logp, B * 4}, {(void**)&h->ch1, 2 * B * HID * 4}, {(void**)&h->ch2, 2 * B * HID * 4},
      {(void**)&h->q, 2 * B * 4}, {(void**)&h->qt, 2 * B * 4}, {(void**)&h->dq, 2 * B * 4}, {(void**)&h->dy1, 2 * B * HID * 4},
      {(void**)&h->da, B * ACT * 4}, {(void**)&h->dhead, B * 2 * ACT * 4}, {(void**)&h->dh2, B * HID * 4}, {(void**)&h->dh1, B * HID * 4},
      {(void**)&h->rows_c, 2 * B * 4}, {(void**)&h->rows_a, B * 4}, {(void**)&h->losses, 8}, {(void**)&h->steps, 16}, {(void**)&h->bc, 32}};
  for (auto& x : a) {
    if (hipMalloc(x.p, x.bytes) != hipSuccess) { etg_sac_destroy(h); return sfail(ETG_ERR_ALLOC, "etg_sac_create: hipMalloc failed"); }
    if (hipMemset(*x.p, 0, x.bytes) != hipSuccess) { etg_sac_destroy(h); return sfail(ETG_ERR_HIP, "etg_sac_create: hipMemset failed"); }
  }
  *out = h;
  return ETG_OK;
}

extern "C" int etg_sac_destroy(EtgSac* h) {
  if (!h) return sfail(ETG_ERR_BAD_ARG, "etg_sac_destroy: null handle");
  (void)hipSetDevice(h->device);
  void* ptrs[] = {h->P, h->G, h->M, h->V, h->T, h->ah1, h->ah2, h->head, h->asmp, h->logp, h->ch1, h->ch2, h->q, h->qt, h->dq,
                  h->dy1, h->da, h->dhead, h->dh2, h->dh1, h->rows_c, h->rows_a, h->losses, h->steps, h->bc};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  delete h;
  return ETG_OK;
}

extern "C" int etg_sac_set_hyper(EtgSac* h, double gamma, double tau, double alpha, double actor_lr, double critic_lr) {
  if (!h) return sfail(ETG_ERR_BAD_ARG, "etg_sac_set_hyper: null handle");
  h->gamma = gamma; h->tau = tau; h->alpha = alpha; h->actor_lr = actor_lr; h->critic_lr = critic_lr;
  return ETG_OK;
}

extern "C" int etg_sac_load(EtgSac* h, const float* const* tensors, int n, void* stream) {
  if (!h) return sfail(ETG_ERR_BAD_ARG, "etg_sac_load: null handle");
  if (!tensors || n != ETG_SAC_TENSORS) return sfail(ETG_ERR_BAD_ARG, "etg_sac_load: need the 20 tensors");
  for (int i = 0; i < n; i++)
    if (!tensors[i]) return sfail(ETG_ERR_BAD_ARG, "etg_sac_load: null tensor");
  if (hipSetDevice(h->device) != hipSuccess) return sfail(ETG_ERR_HIP, "hipSetDevice");
  hipStream_t s = (hipStream_t)stream;
  bool ok = true;
  for (int i = 0; i < n; i++) ok &= hipMemcpyAsync(h->P + h->off[i], tensors[i], h->len[i] * 4, hipMemcpyDeviceToDevice, s) == hipSuccess;
  ok &= hipMemcpyAsync(h->T, h->P + h->asize, 2 * h->csize * 4, hipMemcpyDeviceToDevice, s) == hipSuccess;
  ok &= hipMemsetAsync(h->M, 0, h->total * 4, s) == hipSuccess;
  ok &= hipMemsetAsync(h->V, 0, h->total * 4, s) == hipSuccess;
  ok &= hipMemsetAsync(h->steps, 0, 16, s) == hipSuccess;
  return ok ? ETG_OK : sfail(ETG_ERR_HIP, "etg_sac_load: copy failed");
}

extern "C" int etg_sac_store(EtgSac* h, float* const* tensors, int n, void* stream) {
  if (!h) return sfail(ETG_ERR_BAD_ARG, "etg_sac_store: null handle");
  if (!tensors || n != ETG_SAC_TENSORS) return sfail(ETG_ERR_BAD_ARG, "etg_sac_store: need the 20 tensors");
  for (int i = 0; i < n; i++)
    if (!tensors[i]) return sfail(ETG_ERR_BAD_ARG, "etg_sac_store: null tensor");
  if (hipSetDevice(h->device) != hipSuccess) return sfail(ETG_ERR_HIP, "hipSetDevice");
  bool ok = true;
  for (int i = 0; i < n; i++)
    ok &= hipMemcpyAsync(tensors[i], h->P + h->off[i], h->len[i] * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream) == hipSuccess;
  return ok ? ETG_OK : sfail(ETG_ERR_HIP, "etg_sac_store: copy failed");
}

extern "C" int etg_sac_load_opt(EtgSac* h, const float* target, const float* exp_avg, const float* exp_avg_sq, const long long* steps,
                                void* stream) {
  if (!h) return sfail(ETG_ERR_BAD_ARG, "etg_sac_load_opt: null handle");
  if (hipSetDevice(h->device) != hipSuccess) return sfail(ETG_ERR_HIP, "hipSetDevice");
  hipStream_t s = (hipStream_t)stream;
  bool ok = true;
  if (target) ok &= hipMemcpyAsync(h->T, target, 2 * h->csize * 4, hipMemcpyDeviceToDevice, s) == hipSuccess;
  if (exp_avg) ok &= hipMemcpyAsync(h->M, exp_avg, h->total * 4, hipMemcpyDeviceToDevice, s) == hipSuccess;
  if (exp_avg_sq) ok &= hipMemcpyAsync(h->V, exp_avg_sq, h->total * 4, hipMemcpyDeviceToDevice, s) == hipSuccess;
  if (steps) ok &= hipMemcpyAsync(h->steps, steps, 16, hipMemcpyDeviceToDevice, s) == hipSuccess;
  return ok ? ETG_OK : sfail(ETG_ERR_HIP, "etg_sac_load_opt: copy failed");
}

extern "C" int etg_sac_store_opt(EtgSac* h, float* target, float* exp_avg, float* exp_avg_sq, long long* steps, void* stream) {
  if (!h) return sfail(ETG_ERR_BAD_ARG, "etg_sac_store_opt: null handle");
  if (hipSetDevice(h->device) != hipSuccess) return sfail(ETG_ERR_HIP, "hipSetDevice");
  hipStream_t s = (hipStream_t)stream;
  bool ok = true;
  if (target) ok &= hipMemcpyAsync(target, h->T, 2 * h->csize * 4, hipMemcpyDeviceToDevice, s) == hipSuccess;
  if (exp_avg) ok &= hipMemcpyAsync(exp_avg, h->M, h->total * 4, hipMemcpyDeviceToDevice, s) == hipSuccess;
  if (exp_avg_sq) ok &= hipMemcpyAsync(exp_avg_sq, h->V, h->total * 4, hipMemcpyDeviceToDevice, s) == hipSuccess;
  if (steps) ok &= hipMemcpyAsync(steps, h->steps, 16, hipMemcpyDeviceToDevice, s) == hipSuccess;
  return ok ? ETG_OK : sfail(ETG_ERR_HIP, "etg_sac_store_opt: copy failed");
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
  if (!idx) return sfail(ETG_ERR_BAD_ARG, "etg_sac_learn_replay: null index vector");
  return run_update(h, b, n, eps_next, eps_cur, true, losses2, (hipStream_t)stream);
}

extern "C" int etg_sac_grads(EtgSac* h, const float* obs, const float* act, const float* reward, const float* next_obs,
                             const float* terminal, int n, const float* eps_next, const float* eps_cur, float* const* grads, void* stream) {
  const Batch b{obs, act, reward, next_obs, terminal, nullptr};
  if (int rc = check_batch(h, b, n, eps_next, eps_cur, "etg_sac_grads")) return rc;
  if (!grads) return sfail(ETG_ERR_BAD_ARG, "etg_sac_grads: null pointer");
  for (int i = 0; i < ETG_SAC_TENSORS; i++)
    if (!grads[i]) return sfail(ETG_ERR_BAD_ARG, "etg_sac_grads: null tensor");
  if (int rc = run_update(h, b, n, eps_next, eps_cur, false, nullptr, (hipStream_t)stream)) return rc;
  bool ok = true;
  for (int i = 0; i < ETG_SAC_TENSORS; i++)
    ok &= hipMemcpyAsync(grads[i], h->G + h->off[i], h->len[i] * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream) == hipSuccess;
  return ok ? ETG_OK : sfail(ETG_ERR_HIP, "etg_sac_grads: copy failed");
}

extern "C" int etg_sac_sync_policy(EtgSac* h, EtgPolicy* p, void* stream) {
  if (!h) return sfail(ETG_ERR_BAD_ARG, "etg_sac_sync_policy: null handle");
  if (!p) return sfail(ETG_ERR_BAD_ARG, "etg_sac_sync_policy: null policy");
  if (p->in_dim > 64) return sfail(ETG_ERR_BAD_ARG, "etg_sac_sync_policy: the learner and its policy sync take observations of in_dim <= 64");
  if (p->in_dim != h->d || p->hidden != HID || p->out_dim != ACT || p->device != h->device)
    return sfail(ETG_ERR_BAD_ARG, "etg_sac_sync_policy: the policy's dimensions or device differ from the learner's");
  const float* P = h->P;
  if (int rc = etg_policy_load(p, P + h->off[0], P + h->off[1], P + h->off[2], P + h->off[3], P + h->off[4], P + h->off[5], stream)) return rc;
  return etg_policy_load_std(p, P + h->off[6], P + h->off[7], stream);
}
