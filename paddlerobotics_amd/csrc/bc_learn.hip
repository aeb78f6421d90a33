// bc_learn.hip -- one behaviour-cloning update on the device (include/etgsim_bc.h): alg/BC.py:53-72 of the reference on
// model/mujoco_model.py, a student of observation width ds distilled from a frozen teacher of width dt, fp32 throughout.
//
// The pieces are the SAC learner's (sac_core.h): every contraction is sac::k_gemm with its loader / store functors, the sample is
// k_sample, Adam is k_adam without a target, the losses are reduced by k_loss.  What this update adds (bc_core.h): the teacher's
// tanh(mean), the Gaussian negative log-likelihood's backward at the head, and the critics' regression onto the teacher's critics.
// There is no target network.  The launch list of one update (31 launches and one 8-byte copy):
//   actor step    teacher actor l1, l2, mean head (3 gemm), k_tanh                          -> aref
//                 student actor l1, l2, heads (3 gemm), k_nll_bwd                           -> dhead, loss rows, actor step count
//                 head dW, dh2, l2 dW, dh1, l1 dW (5 gemm), k_adam on the actor's region
//   critic step   student actor again (3 gemm), k_sample with eps_c                         -> a_now
//                 teacher critics on [ref_obs | a_now] (3 gemm, grid.z = 2)                 -> rq   (first: it shares ch1 / ch2)
//                 student critics on [obs | a_now] (3 gemm)                                 -> q, ch1, ch2 kept for the backward
//                 k_regress, dW3, dW2, dY1, dW1 (4 gemm), k_adam on both critics' region
//   k_loss
//
// Student arena (floats), state_dict order, as sac_learn.hip's: the actor's 8 tensors, then Q1's 6, then Q2's 6 one critic's size
// later.  The actor's size 256 ds + 72216 is a multiple of 4, so both regions k_adam walks (the actor; the two critics together,
// an even number of floats) start 16-byte aligned for its float4 loop, and its scalar tail takes the critics' last 2 floats.
// The teacher's 20 tensors lie in an arena of the same layout for width dt.
#include <hip/hip_runtime.h>

#include "../../include/etgsim_bc.h"
#include "bc_core.h"
#include "policy_core.h"

extern "C" void etg_set_last_error_(const char* msg);

namespace {
using namespace sac;

int bfail(int code, const char* msg) {
  etg_set_last_error_(msg);
  return code;
}

struct Pairs {
  const float *obs, *ref;
  const long long* idx;
};

void layout(size_t d, size_t* off, size_t* len) {
  const size_t kin = d + ACT;
  const size_t lens[ETG_BC_TENSORS] = {HID * d, HID, (size_t)HID * HID, HID, ACT * HID, ACT, ACT * HID, ACT,
                                       HID * kin, HID, (size_t)HID * HID, HID, HID, 1, HID * kin, HID, (size_t)HID * HID, HID, HID, 1};
  size_t o = 0;
  for (int i = 0; i < ETG_BC_TENSORS; i++) { off[i] = o; len[i] = lens[i]; o += lens[i]; }
  off[ETG_BC_TENSORS] = o;
}

}  // namespace

struct EtgBc {
  int device, ds, dt, maxb;
  bool teacher;
  double actor_lr, critic_lr;
  size_t asize, csize, total;          // floats: the student's actor, ONE of its critics, everything
  size_t tasize, tcsize, ttotal;       // the same of the teacher
  float *P, *G, *M, *V, *TP;           // parameters, gradients, Adam moments [total]; the teacher's parameters [ttotal]
  float *ah1, *ah2, *head, *aref, *asmp, *logp;           // actor passes: [B,256] x 2, [B,24], [B,12], [B,12], [B]
  float *ch1, *ch2, *q, *rq, *dq, *dy1;                   // critic passes: [2,B,256] x 2, [2,B] x 3, [2,B,256]
  float *dhead, *dh2, *dh1, *rows_c, *rows_a;             // actor backward: [B,24], [B,256] x 2; loss rows [2,B], [B]
  float* losses;                                          // [2]
  long long* steps;                                       // [2]: actor, critic optimizer
  double* bc;                                             // [4]: 1 - beta1^t, sqrt(1 - beta2^t) of actor, critic
  size_t off[ETG_BC_TENSORS + 1], len[ETG_BC_TENSORS], toff[ETG_BC_TENSORS + 1], tlen[ETG_BC_TENSORS];
};

namespace {

template <class FA, class FB, class ST>
void gemm(hipStream_t s, int M, int N, int K, int Z, FA fa, FB fb, ST st) {
  dim3 grid((N + TN - 1) / TN, (M + TM - 1) / TM, Z);
  hipLaunchKernelGGL((k_gemm<FA, FB, ST>), grid, dim3(256), 0, s, M, N, K, fa, fb, st);
}

// the two hidden layers of an actor of input width d with the weights at `w`, on rows of `x` (through idx when given): h->ah1, h->ah2.
// Returns the head's weights (mean.w, mean.b, std.w, std.b).
const float* actor_hidden(EtgBc* h, hipStream_t s, int n, const float* x, const long long* idx, int d, const float* w) {
  const float* l1w = w;
  const float* l1b = l1w + (size_t)HID * d;
  const float* l2w = l1b + HID;
  const float* l2b = l2w + (size_t)HID * HID;
  gemm(s, n, HID, d, 1, InCat<false>{x, idx, d, nullptr, nullptr, 0}, Mat<false>{l1w, 0, d}, StAct<true>{h->ah1, 0, HID, l1b, 0});
  gemm(s, n, HID, HID, 1, Mat<false>{h->ah1, 0, HID}, Mat<false>{l2w, 0, HID}, StAct<true>{h->ah2, 0, HID, l2b, 0});
  return l2b + HID;
}

// two critics of observation width d, one critic's size cs, with the weights at `w`, on [x rows | h->asmp]: h->ch1, h->ch2, qout
void critic_forward(EtgBc* h, hipStream_t s, int n, const float* x, const long long* idx, int d, long cs, const float* w, float* qout) {
  const int kin = d + ACT;
  const long zh = (long)h->maxb * HID;
  const float* l1w = w;
  const float* l1b = l1w + (size_t)HID * kin;
  const float* l2w = l1b + HID;
  const float* l2b = l2w + (size_t)HID * HID;
  const float* l3w = l2b + HID;
  const float* l3b = l3w + HID;
  gemm(s, n, HID, kin, 2, InCat<false>{x, idx, d, h->asmp, nullptr, ACT}, Mat<false>{l1w, cs, kin}, StAct<true>{h->ch1, zh, HID, l1b, cs});
  gemm(s, n, HID, HID, 2, Mat<false>{h->ch1, zh, HID}, Mat<false>{l2w, cs, HID}, StAct<true>{h->ch2, zh, HID, l2b, cs});
  gemm(s, n, 1, HID, 2, Mat<false>{h->ch2, zh, HID}, Mat<false>{l3w, cs, HID}, StAct<false>{qout, (long)h->maxb, 1, l3b, cs});
}

int run_update(EtgBc* h, const Pairs& b, int n, const float* eps_c, bool apply, float* losses2, hipStream_t s) {
  const int ds = h->ds, dt = h->dt, kin = ds + ACT, B = h->maxb;
  const long zs = (long)h->csize, zh = (long)B * HID;
  float* PC = h->P + h->asize;   // the student's critics
  float* GC = h->G + h->asize;
  // ---- actor step
  {
    const float* thw = actor_hidden(h, s, n, b.ref, b.idx, dt, h->TP);
    gemm(s, n, ACT, HID, 1, Mat<false>{h->ah2, 0, HID}, Mat<false>{thw, 0, HID}, StAct<false>{h->aref, 0, ACT, thw + (size_t)ACT * HID, 0});
    hipLaunchKernelGGL(bc::k_tanh, dim3((n * ACT + 255) / 256), dim3(256), 0, s, h->aref, n * ACT);
    const float* hw = actor_hidden(h, s, n, b.obs, b.idx, ds, h->P);
    gemm(s, n, 2 * ACT, HID, 1, Mat<false>{h->ah2, 0, HID}, HeadW<false>{hw}, StHead{h->head, hw});
    hipLaunchKernelGGL(bc::k_nll_bwd, dim3((n + 15) / 16), dim3(256), 0, s, h->head, h->aref, n, h->dhead, h->rows_a,
                       apply ? h->steps : nullptr, h->bc);
    const size_t a_l2w = (size_t)HID * ds + HID, a_hw = a_l2w + (size_t)HID * HID + HID;
    // head: dW | db of both heads = dhead^T [h2 | 1];  dh2 = (dhead Whead) [h2 > 0];  then the two hidden layers
    gemm(s, 2 * ACT, HID + 1, n, 1, Mat<true>{h->dhead, 0, 2 * ACT}, MatAug{h->ah2, 0, HID, HID},
         StGrad{h->G + a_hw, 0, ACT, HID, (long)ACT * HID + ACT});
    gemm(s, n, HID, 2 * ACT, 1, Mat<false>{h->dhead, 0, 2 * ACT}, HeadW<true>{h->P + a_hw}, StMask{h->dh2, 0, HID, h->ah2});
    gemm(s, HID, HID + 1, n, 1, Mat<true>{h->dh2, 0, HID}, MatAug{h->ah1, 0, HID, HID}, StGrad{h->G + a_l2w, 0, HID, HID, 0});
    gemm(s, n, HID, HID, 1, Mat<false>{h->dh2, 0, HID}, Mat<true>{h->P + a_l2w, 0, HID}, StMask{h->dh1, 0, HID, h->ah1});
    gemm(s, HID, ds + 1, n, 1, Mat<true>{h->dh1, 0, HID}, InCat<true>{b.obs, b.idx, ds, nullptr, nullptr, 0}, StGrad{h->G, 0, HID, ds, 0});
    if (apply)
      hipLaunchKernelGGL(k_adam, dim3(512), dim3(256), 0, s, h->P, h->G, h->M, h->V, (long)h->asize, h->actor_lr, h->bc,
                         (float*)nullptr, 0.0f, 0.0f);
  }
  // ---- critic step (with the actor just updated)
  {
    const float* hw = actor_hidden(h, s, n, b.obs, b.idx, ds, h->P);
    gemm(s, n, 2 * ACT, HID, 1, Mat<false>{h->ah2, 0, HID}, HeadW<false>{hw}, StHead{h->head, hw});
    hipLaunchKernelGGL(k_sample, dim3((n + 15) / 16), dim3(256), 0, s, h->head, eps_c, n, h->asmp, h->logp);
    critic_forward(h, s, n, b.ref, b.idx, dt, (long)h->tcsize, h->TP + h->tasize, h->rq);
    critic_forward(h, s, n, b.obs, b.idx, ds, zs, PC, h->q);
    hipLaunchKernelGGL(bc::k_regress, dim3((n + 255) / 256), dim3(256), 0, s, n, B, h->q, h->rq, h->dq, h->rows_c,
                       apply ? h->steps + 1 : nullptr, h->bc + 2);
    const size_t o_l1w = 0, o_l2w = (size_t)HID * kin + HID, o_l3w = o_l2w + (size_t)HID * HID + HID;
    // dW3 | db3 = dq^T [h2 | 1]
    gemm(s, 1, HID + 1, n, 2, Mat<true>{h->dq, (long)B, 1}, MatAug{h->ch2, zh, HID, HID}, StGrad{GC + o_l3w, zs, 1, HID, 0});
    // dW2 | db2 = dY2^T [h1 | 1],  dY2 = dq w3 [h2 > 0]
    DQ<true> dy2t{h->dq, (long)B, PC + o_l3w, zs, h->ch2, zh};
    gemm(s, HID, HID + 1, n, 2, dy2t, MatAug{h->ch1, zh, HID, HID}, StGrad{GC + o_l2w, zs, HID, HID, 0});
    // dY1 = (dY2 W2) [h1 > 0]
    DQ<false> dy2{h->dq, (long)B, PC + o_l3w, zs, h->ch2, zh};
    gemm(s, n, HID, HID, 2, dy2, Mat<true>{PC + o_l2w, zs, HID}, StMask{h->dy1, zh, HID, h->ch1});
    // dW1 | db1 = dY1^T [obs | a_now | 1]
    gemm(s, HID, kin + 1, n, 2, Mat<true>{h->dy1, zh, HID}, InCat<true>{b.obs, b.idx, ds, h->asmp, nullptr, ACT},
         StGrad{GC + o_l1w, zs, HID, kin, 0});
    if (apply)
      hipLaunchKernelGGL(k_adam, dim3(512), dim3(256), 0, s, PC, GC, h->M + h->asize, h->V + h->asize, (long)(2 * h->csize),
                         h->critic_lr, h->bc + 2, (float*)nullptr, 0.0f, 0.0f);
  }
  hipLaunchKernelGGL(k_loss, dim3(1), dim3(256), 0, s, n, B, h->rows_c, h->rows_a, h->losses);
  if (losses2 && hipMemcpyAsync(losses2, h->losses, 8, hipMemcpyDeviceToDevice, s) != hipSuccess)
    return bfail(ETG_ERR_HIP, "etg_bc: copying the losses failed");
  if (hipGetLastError() != hipSuccess) return bfail(ETG_ERR_HIP, "etg_bc: a launch failed");
  return ETG_OK;
}

int check_batch(EtgBc* h, const Pairs& b, int n, const float* eps_c, const char* who) {
  static thread_local char msg[160];
  if (!h) { snprintf(msg, sizeof msg, "%s: null handle", who); return bfail(ETG_ERR_BAD_ARG, msg); }
  if (n < 1 || n > h->maxb) { snprintf(msg, sizeof msg, "%s: n = %d outside 1..max_batch = %d", who, n, h->maxb); return bfail(ETG_ERR_BAD_ARG, msg); }
  if (!b.obs || !b.ref || !eps_c) { snprintf(msg, sizeof msg, "%s: null pointer", who); return bfail(ETG_ERR_BAD_ARG, msg); }
  if (!h->teacher) { snprintf(msg, sizeof msg, "%s: no teacher has been set (etg_bc_set_teacher)", who); return bfail(ETG_ERR_STATE, msg); }
  if (hipSetDevice(h->device) != hipSuccess) return bfail(ETG_ERR_HIP, "hipSetDevice");
  return ETG_OK;
}

}  // namespace

extern "C" int etg_bc_create(int student_obs_dim, int teacher_obs_dim, int act_dim, int hidden, int max_batch, int device, EtgBc** out) {
  if (!out || student_obs_dim < 1 || student_obs_dim > 64 || teacher_obs_dim < 1 || teacher_obs_dim > 64 || act_dim != ACT ||
      hidden != HID || max_batch < 1 || max_batch > (1 << 20))
    return bfail(ETG_ERR_BAD_ARG, "etg_bc_create: need student and teacher obs_dim 1..64, act_dim 12, hidden 256, max_batch 1..2^20");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return bfail(ETG_ERR_NO_DEVICE, "etg_bc_create: no HIP device");
  if (device < 0 || device >= ndev) return bfail(ETG_ERR_BAD_ARG, "etg_bc_create: bad device");
  if (hipSetDevice(device) != hipSuccess) return bfail(ETG_ERR_HIP, "hipSetDevice");
  EtgBc* h = new EtgBc();
  h->device = device; h->ds = student_obs_dim; h->dt = teacher_obs_dim; h->maxb = max_batch;
  h->teacher = false;
  h->actor_lr = 3e-4; h->critic_lr = 3e-4;
  layout(h->ds, h->off, h->len);
  layout(h->dt, h->toff, h->tlen);
  h->total = h->off[ETG_BC_TENSORS]; h->asize = h->off[8]; h->csize = h->off[14] - h->off[8];
  h->ttotal = h->toff[ETG_BC_TENSORS]; h->tasize = h->toff[8]; h->tcsize = h->toff[14] - h->toff[8];
  const size_t B = max_batch;
  struct { void** p; size_t bytes; } a[] = {
      {(void**)&h->P, h->total * 4}, {(void**)&h->G, h->total * 4}, {(void**)&h->M, h->total * 4}, {(void**)&h->V, h->total * 4},
      {(void**)&h->TP, h->ttotal * 4}, {(void**)&h->ah1, B * HID * 4}, {(void**)&h->ah2, B * HID * 4}, {(void**)&h->head, B * 2 * ACT * 4},
      {(void**)&h->aref, B * ACT * 4}, {(void**)&h->asmp, B * ACT * 4}, {(void**)&h->logp, B * 4}, {(void**)&h->ch1, 2 * B * HID * 4},
      {(void**)&h->ch2, 2 * B * HID * 4}, {(void**)&h->q, 2 * B * 4}, {(void**)&h->rq, 2 * B * 4}, {(void**)&h->dq, 2 * B * 4},
      {(void**)&h->dy1, 2 * B * HID * 4}, {(void**)&h->dhead, B * 2 * ACT * 4}, {(void**)&h->dh2, B * HID * 4}, {(void**)&h->dh1, B * HID * 4},
      {(void**)&h->rows_c, 2 * B * 4}, {(void**)&h->rows_a, B * 4}, {(void**)&h->losses, 8}, {(void**)&h->steps, 16}, {(void**)&h->bc, 32}};
  for (auto& x : a) {
    if (hipMalloc(x.p, x.bytes) != hipSuccess) { etg_bc_destroy(h); return bfail(ETG_ERR_ALLOC, "etg_bc_create: hipMalloc failed"); }
    if (hipMemset(*x.p, 0, x.bytes) != hipSuccess) { etg_bc_destroy(h); return bfail(ETG_ERR_HIP, "etg_bc_create: hipMemset failed"); }
  }
  *out = h;
  return ETG_OK;
}

extern "C" int etg_bc_destroy(EtgBc* h) {
  if (!h) return bfail(ETG_ERR_BAD_ARG, "etg_bc_destroy: null handle");
  (void)hipSetDevice(h->device);
  void* ptrs[] = {h->P, h->G, h->M, h->V, h->TP, h->ah1, h->ah2, h->head, h->aref, h->asmp, h->logp, h->ch1, h->ch2, h->q, h->rq,
                  h->dq, h->dy1, h->dhead, h->dh2, h->dh1, h->rows_c, h->rows_a, h->losses, h->steps, h->bc};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  delete h;
  return ETG_OK;
}

extern "C" int etg_bc_set_hyper(EtgBc* h, double actor_lr, double critic_lr) {
  if (!h) return bfail(ETG_ERR_BAD_ARG, "etg_bc_set_hyper: null handle");
  h->actor_lr = actor_lr; h->critic_lr = critic_lr;
  return ETG_OK;
}

extern "C" int etg_bc_load(EtgBc* h, const float* const* tensors, int n, void* stream) {
  if (!h) return bfail(ETG_ERR_BAD_ARG, "etg_bc_load: null handle");
  if (!tensors || n != ETG_BC_TENSORS) return bfail(ETG_ERR_BAD_ARG, "etg_bc_load: need the 20 tensors");
  for (int i = 0; i < n; i++)
    if (!tensors[i]) return bfail(ETG_ERR_BAD_ARG, "etg_bc_load: null tensor");
  if (hipSetDevice(h->device) != hipSuccess) return bfail(ETG_ERR_HIP, "hipSetDevice");
  hipStream_t s = (hipStream_t)stream;
  bool ok = true;
  for (int i = 0; i < n; i++) ok &= hipMemcpyAsync(h->P + h->off[i], tensors[i], h->len[i] * 4, hipMemcpyDeviceToDevice, s) == hipSuccess;
  ok &= hipMemsetAsync(h->M, 0, h->total * 4, s) == hipSuccess;
  ok &= hipMemsetAsync(h->V, 0, h->total * 4, s) == hipSuccess;
  ok &= hipMemsetAsync(h->steps, 0, 16, s) == hipSuccess;
  return ok ? ETG_OK : bfail(ETG_ERR_HIP, "etg_bc_load: copy failed");
}

extern "C" int etg_bc_store(EtgBc* h, float* const* tensors, int n, void* stream) {
  if (!h) return bfail(ETG_ERR_BAD_ARG, "etg_bc_store: null handle");
  if (!tensors || n != ETG_BC_TENSORS) return bfail(ETG_ERR_BAD_ARG, "etg_bc_store: need the 20 tensors");
  for (int i = 0; i < n; i++)
    if (!tensors[i]) return bfail(ETG_ERR_BAD_ARG, "etg_bc_store: null tensor");
  if (hipSetDevice(h->device) != hipSuccess) return bfail(ETG_ERR_HIP, "hipSetDevice");
  bool ok = true;
  for (int i = 0; i < n; i++)
    ok &= hipMemcpyAsync(tensors[i], h->P + h->off[i], h->len[i] * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream) == hipSuccess;
  return ok ? ETG_OK : bfail(ETG_ERR_HIP, "etg_bc_store: copy failed");
}

extern "C" int etg_bc_load_opt(EtgBc* h, const float* exp_avg, const float* exp_avg_sq, const long long* steps, void* stream) {
  if (!h) return bfail(ETG_ERR_BAD_ARG, "etg_bc_load_opt: null handle");
  if (hipSetDevice(h->device) != hipSuccess) return bfail(ETG_ERR_HIP, "hipSetDevice");
  hipStream_t s = (hipStream_t)stream;
  bool ok = true;
  if (exp_avg) ok &= hipMemcpyAsync(h->M, exp_avg, h->total * 4, hipMemcpyDeviceToDevice, s) == hipSuccess;
  if (exp_avg_sq) ok &= hipMemcpyAsync(h->V, exp_avg_sq, h->total * 4, hipMemcpyDeviceToDevice, s) == hipSuccess;
  if (steps) ok &= hipMemcpyAsync(h->steps, steps, 16, hipMemcpyDeviceToDevice, s) == hipSuccess;
  return ok ? ETG_OK : bfail(ETG_ERR_HIP, "etg_bc_load_opt: copy failed");
}

extern "C" int etg_bc_store_opt(EtgBc* h, float* exp_avg, float* exp_avg_sq, long long* steps, void* stream) {
  if (!h) return bfail(ETG_ERR_BAD_ARG, "etg_bc_store_opt: null handle");
  if (hipSetDevice(h->device) != hipSuccess) return bfail(ETG_ERR_HIP, "hipSetDevice");
  hipStream_t s = (hipStream_t)stream;
  bool ok = true;
  if (exp_avg) ok &= hipMemcpyAsync(exp_avg, h->M, h->total * 4, hipMemcpyDeviceToDevice, s) == hipSuccess;
  if (exp_avg_sq) ok &= hipMemcpyAsync(exp_avg_sq, h->V, h->total * 4, hipMemcpyDeviceToDevice, s) == hipSuccess;
  if (steps) ok &= hipMemcpyAsync(steps, h->steps, 16, hipMemcpyDeviceToDevice, s) == hipSuccess;
  return ok ? ETG_OK : bfail(ETG_ERR_HIP, "etg_bc_store_opt: copy failed");
}

extern "C" int etg_bc_set_teacher(EtgBc* h, const float* const* tensors, void* stream) {
  if (!h) return bfail(ETG_ERR_BAD_ARG, "etg_bc_set_teacher: null handle");
  if (!tensors) return bfail(ETG_ERR_BAD_ARG, "etg_bc_set_teacher: need the teacher's 20 tensors");
  for (int i = 0; i < ETG_BC_TENSORS; i++)
    if (!tensors[i]) return bfail(ETG_ERR_BAD_ARG, "etg_bc_set_teacher: null tensor");
  if (hipSetDevice(h->device) != hipSuccess) return bfail(ETG_ERR_HIP, "hipSetDevice");
  bool ok = true;
  for (int i = 0; i < ETG_BC_TENSORS; i++)
    ok &= hipMemcpyAsync(h->TP + h->toff[i], tensors[i], h->tlen[i] * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream) == hipSuccess;
  if (!ok) return bfail(ETG_ERR_HIP, "etg_bc_set_teacher: copy failed");
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
  if (!idx) return bfail(ETG_ERR_BAD_ARG, "etg_bc_learn_replay: null index vector");
  return run_update(h, b, n, eps_c, true, losses2, (hipStream_t)stream);
}

extern "C" int etg_bc_grads(EtgBc* h, const float* obs, const float* ref_obs, int n, const float* eps_a, const float* eps_c,
                            float* const* grads, void* stream) {
  (void)eps_a;
  const Pairs b{obs, ref_obs, nullptr};
  if (int rc = check_batch(h, b, n, eps_c, "etg_bc_grads")) return rc;
  if (!grads) return bfail(ETG_ERR_BAD_ARG, "etg_bc_grads: null pointer");
  for (int i = 0; i < ETG_BC_TENSORS; i++)
    if (!grads[i]) return bfail(ETG_ERR_BAD_ARG, "etg_bc_grads: null tensor");
  if (int rc = run_update(h, b, n, eps_c, false, nullptr, (hipStream_t)stream)) return rc;
  bool ok = true;
  for (int i = 0; i < ETG_BC_TENSORS; i++)
    ok &= hipMemcpyAsync(grads[i], h->G + h->off[i], h->len[i] * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream) == hipSuccess;
  return ok ? ETG_OK : bfail(ETG_ERR_HIP, "etg_bc_grads: copy failed");
}

extern "C" int etg_bc_sync_policy(EtgBc* h, EtgPolicy* p, void* stream) {
  if (!h) return bfail(ETG_ERR_BAD_ARG, "etg_bc_sync_policy: null handle");
  if (!p) return bfail(ETG_ERR_BAD_ARG, "etg_bc_sync_policy: null policy");
  if (p->in_dim > 64) return bfail(ETG_ERR_BAD_ARG, "etg_bc_sync_policy: the learner and its policy sync take observations of in_dim <= 64");
  if (p->in_dim != h->ds || p->hidden != HID || p->out_dim != ACT || p->device != h->device)
    return bfail(ETG_ERR_BAD_ARG, "etg_bc_sync_policy: the policy's dimensions or device differ from the learner's");
  const float* P = h->P;
  if (int rc = etg_policy_load(p, P + h->off[0], P + h->off[1], P + h->off[2], P + h->off[3], P + h->off[4], P + h->off[5], stream)) return rc;
  return etg_policy_load_std(p, P + h->off[6], P + h->off[7], stream);
}
