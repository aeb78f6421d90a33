// ac_learner.h -- the host side that the actor-critic learners (sac_learn.hip, bc_learn.hip) share: the handle's common part, the
// parameter arena, and the launch chains of an update over model/mujoco_model.py of the reference (actor obs -> 256 -> 256 ->
// 12 + 12, two critics obs + 12 -> 256 -> 256 -> 1), fp32 throughout.  Everything here is host code; the kernels are sac_core.h's.
//
// Every contraction of an update -- forward Y = X W^T, input gradient dX = dY W, weight gradient dW = dY^T X -- is the ONE
// tiled kernel k_gemm (sac_core.h: 32 x 32 output tile per workgroup, v_mfma_f32_16x16x4_f32, the whole reduction inside the
// workgroup, so no split K and no atomics); what differs between the uses is how an operand element is fetched and how a
// result element is stored, and those are small functors:
//   * the first layers read [obs | action] (and the replay ring through an index vector) in their loader, nothing is gathered
//     or concatenated in memory;
//   * bias + ReLU, the ReLU mask of the backward pass and the bias gradient are epilogues / loaders: the bias gradient is the
//     column of dW that a ones column appended to X produces;
//   * dY of a critic's second layer, dq * w3 * [h2 > 0], is formed by the loader from the 256 -> 1 layer's weights;
//   * the two critics are grid.z = 2 of one launch in every pass.
// A learner's run_update is a list of the launch chains at the end of this file plus its own elementwise kernels.
//
// Arena (floats), state_dict order: actor l1.w l1.b l2.w l2.b mean.w mean.b std.w std.b | critic l1.w l1.b l2.w l2.b l3.w l3.b
// l4.w .. l6.b.  Q2's tensors lie one critic's size after Q1's, so a per-critic pointer is base + z * csize.  The actor's size
// 256 d + 72216 is a multiple of 4, so both regions k_adam walks (the actor; the two critics together, an even number of floats)
// start 16-byte aligned for its float4 loop, and its scalar tail takes the critics' last 2 floats.
#ifndef AC_LEARNER_H_
#define AC_LEARNER_H_

#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

#include "../../include/etgsim_sac.h"
#include "dev_buffers.h"
#include "policy_core.h"
#include "sac_core.h"

namespace ac {
using namespace sac;

constexpr int TENSORS = ETG_SAC_TENSORS;

// what EtgSac and EtgBc have in common: the learner's own model, its optimizer state and the workspace both updates use
struct Learner {
  int device, d, maxb;                 // d: the observation width of the model that learns
  double actor_lr, critic_lr;
  size_t asize, csize, total;          // floats: the actor, ONE critic, everything
  float *P, *G, *M, *V;                // parameters, gradients, Adam moments [total]
  float *ah1, *ah2, *head, *asmp, *logp;                  // actor pass: [B,256] x 2, [B,24], [B,12], [B]
  float *ch1, *ch2, *q, *dq, *dy1;                        // critic passes: [2,B,256] x 2, [2,B] x 2, [2,B,256]
  float *dhead, *dh2, *dh1, *rows_c, *rows_a;             // actor backward: [B,24], [B,256] x 2; loss rows [2,B], [B]
  float* losses;                                          // [2]
  long long* steps;                                       // [2]: actor, critic optimizer
  double* bc;                                             // [4]: 1 - beta1^t, sqrt(1 - beta2^t) of actor, critic
  size_t off[TENSORS + 1], len[TENSORS];
};

using dev::Buf;

namespace {   // each learner's translation unit gets its own copy, as it does of sac_core.h's static kernels

using dev::alloc; using dev::fail; using dev::release;   // dev_buffers.h: a handle's buffers, allocated + zeroed / freed from one list

// offsets and lengths of the 20 tensors of a model of observation width d; off[TENSORS] = the arena's size
void layout(size_t d, size_t* off, size_t* len) {
  const size_t kin = d + ACT;
  const size_t lens[TENSORS] = {HID * d, HID, (size_t)HID * HID, HID, ACT * HID, ACT, ACT * HID, ACT,
                                HID * kin, HID, (size_t)HID * HID, HID, HID, 1, HID * kin, HID, (size_t)HID * HID, HID, HID, 1};
  size_t o = 0;
  for (int i = 0; i < TENSORS; i++) { off[i] = o; len[i] = lens[i]; o += lens[i]; }
  off[TENSORS] = o;
}

// ------------------------------------------------------------------------------------------------- creating and destroying
std::vector<Buf> buffers(Learner* h) {
  const size_t B = h->maxb, n = h->total * 4;
  return {{(void**)&h->P, n}, {(void**)&h->G, n}, {(void**)&h->M, n}, {(void**)&h->V, n},
          {(void**)&h->ah1, B * HID * 4}, {(void**)&h->ah2, B * HID * 4}, {(void**)&h->head, B * 2 * ACT * 4}, {(void**)&h->asmp, B * ACT * 4},
          {(void**)&h->logp, B * 4}, {(void**)&h->ch1, 2 * B * HID * 4}, {(void**)&h->ch2, 2 * B * HID * 4}, {(void**)&h->q, 2 * B * 4},
          {(void**)&h->dq, 2 * B * 4}, {(void**)&h->dy1, 2 * B * HID * 4}, {(void**)&h->dhead, B * 2 * ACT * 4}, {(void**)&h->dh2, B * HID * 4},
          {(void**)&h->dh1, B * HID * 4}, {(void**)&h->rows_c, 2 * B * 4}, {(void**)&h->rows_a, B * 4}, {(void**)&h->losses, 8},
          {(void**)&h->steps, 16}, {(void**)&h->bc, 32}};
}

int open_device(int device, const char* who) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(ETG_ERR_NO_DEVICE, who, "no HIP device");
  if (device < 0 || device >= ndev) return fail(ETG_ERR_BAD_ARG, who, "bad device");
  if (hipSetDevice(device) != hipSuccess) return fail(ETG_ERR_HIP, "hipSetDevice");
  return ETG_OK;
}

// the common fields of a value-initialised handle on the device just opened, and the common buffers (zeroed)
int init(Learner* h, int device, int d, int maxb, const char* who) {
  h->device = device; h->d = d; h->maxb = maxb;
  h->actor_lr = 3e-4; h->critic_lr = 3e-4;
  layout(d, h->off, h->len);
  h->total = h->off[TENSORS]; h->asize = h->off[8]; h->csize = h->off[14] - h->off[8];
  return alloc(buffers(h), who);
}

int check_handle(const void* h, const char* who) { return h ? ETG_OK : fail(ETG_ERR_BAD_ARG, who, "null handle"); }

int set_device(Learner* h) { return hipSetDevice(h->device) == hipSuccess ? ETG_OK : fail(ETG_ERR_HIP, "hipSetDevice"); }

// an update's arguments: the handle, n, the learner's own required pointers (ptrs = all of them are there), then the device
int check_batch(Learner* h, int n, bool ptrs, const char* who) {
  static thread_local char msg[160];
  if (int rc = check_handle(h, who)) return rc;
  if (n < 1 || n > h->maxb) { snprintf(msg, sizeof msg, "%s: n = %d outside 1..max_batch = %d", who, n, h->maxb); return fail(ETG_ERR_BAD_ARG, msg); }
  if (!ptrs) return fail(ETG_ERR_BAD_ARG, who, "null pointer");
  return set_device(h);
}

// a host array of 20 device pointers; `missing` is the message when the array itself is not there
int check_tensors(const float* const* tensors, const char* who, const char* missing) {
  if (!tensors) return fail(ETG_ERR_BAD_ARG, who, missing);
  for (int i = 0; i < TENSORS; i++)
    if (!tensors[i]) return fail(ETG_ERR_BAD_ARG, who, "null tensor");
  return ETG_OK;
}

int copy(void* dst, const void* src, size_t bytes, void* stream, const char* who) {   // a null side skips the copy
  if (!dst || !src || hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream) == hipSuccess) return ETG_OK;
  return fail(ETG_ERR_HIP, who, "copy failed");
}

int scatter(float* arena, const size_t* off, const size_t* len, const float* const* tensors, void* stream, const char* who) {
  for (int i = 0; i < TENSORS; i++)
    if (int rc = copy(arena + off[i], tensors[i], len[i] * 4, stream, who)) return rc;
  return ETG_OK;
}

int gather(const float* arena, const size_t* off, const size_t* len, float* const* tensors, void* stream, const char* who) {
  for (int i = 0; i < TENSORS; i++)
    if (int rc = copy(tensors[i], arena + off[i], len[i] * 4, stream, who)) return rc;
  return ETG_OK;
}

// ------------------------------------------------------------------------------------------------- the entry points' bodies
// the 20 tensors into P; Adam's moments and step counts start afresh
int load(Learner* h, const float* const* tensors, int n, void* stream, const char* who) {
  if (int rc = check_handle(h, who)) return rc;
  if (int rc = check_tensors(n == TENSORS ? tensors : nullptr, who, "need the 20 tensors")) return rc;
  if (int rc = set_device(h)) return rc;
  if (int rc = scatter(h->P, h->off, h->len, tensors, stream, who)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const bool ok = hipMemsetAsync(h->M, 0, h->total * 4, s) == hipSuccess && hipMemsetAsync(h->V, 0, h->total * 4, s) == hipSuccess &&
                  hipMemsetAsync(h->steps, 0, 16, s) == hipSuccess;
  return ok ? ETG_OK : fail(ETG_ERR_HIP, who, "copy failed");
}

int store(Learner* h, float* const* tensors, int n, void* stream, const char* who) {
  if (int rc = check_handle(h, who)) return rc;
  if (int rc = check_tensors(n == TENSORS ? tensors : nullptr, who, "need the 20 tensors")) return rc;
  if (int rc = set_device(h)) return rc;
  return gather(h->P, h->off, h->len, tensors, stream, who);
}

// M, V and the step counts, into the handle (load_opt) or out of it (store_opt); a null pointer skips that part
int load_opt(Learner* h, const float* exp_avg, const float* exp_avg_sq, const long long* steps, void* stream, const char* who) {
  if (int rc = check_handle(h, who)) return rc;
  if (int rc = set_device(h)) return rc;
  if (int rc = copy(h->M, exp_avg, h->total * 4, stream, who)) return rc;
  if (int rc = copy(h->V, exp_avg_sq, h->total * 4, stream, who)) return rc;
  return copy(h->steps, steps, 16, stream, who);
}

int store_opt(Learner* h, float* exp_avg, float* exp_avg_sq, long long* steps, void* stream, const char* who) {
  if (int rc = check_handle(h, who)) return rc;
  if (int rc = set_device(h)) return rc;
  if (int rc = copy(exp_avg, h->M, h->total * 4, stream, who)) return rc;
  if (int rc = copy(exp_avg_sq, h->V, h->total * 4, stream, who)) return rc;
  return copy(steps, h->steps, 16, stream, who);
}

int sync_policy(Learner* h, EtgPolicy* p, void* stream, const char* who) {
  if (int rc = check_handle(h, who)) return rc;
  if (!p) return fail(ETG_ERR_BAD_ARG, who, "null policy");
  if (p->in_dim > 64) return fail(ETG_ERR_BAD_ARG, who, "the learner and its policy sync take observations of in_dim <= 64");
  if (p->in_dim != h->d || p->hidden != HID || p->out_dim != ACT || p->device != h->device)
    return fail(ETG_ERR_BAD_ARG, who, "the policy's dimensions or device differ from the learner's");
  const float* P = h->P;
  if (int rc = etg_policy_load(p, P + h->off[0], P + h->off[1], P + h->off[2], P + h->off[3], P + h->off[4], P + h->off[5], stream)) return rc;
  return etg_policy_load_std(p, P + h->off[6], P + h->off[7], stream);
}

// ------------------------------------------------------------------------------------------------- the launch chains
template <class FA, class FB, class ST>
void gemm(hipStream_t s, int M, int N, int K, int Z, FA fa, FB fb, ST st) {
  dim3 grid((N + TN - 1) / TN, (M + TM - 1) / TM, Z);
  hipLaunchKernelGGL((k_gemm<FA, FB, ST>), grid, dim3(256), 0, s, M, N, K, fa, fb, st);
}

// the two hidden layers of an actor of input width d with the weights at `w`, on rows of `x` (through idx when given): h->ah1, h->ah2.
// Returns the head's weights (mean.w, mean.b, std.w, std.b).
const float* actor_hidden(Learner* h, hipStream_t s, int n, const float* x, const long long* idx, int d, const float* w) {
  const float* l1w = w;
  const float* l1b = l1w + (size_t)HID * d;
  const float* l2w = l1b + HID;
  const float* l2b = l2w + (size_t)HID * HID;
  gemm(s, n, HID, d, 1, InCat<false>{x, idx, d, nullptr, nullptr, 0}, Mat<false>{l1w, 0, d}, StAct<true>{h->ah1, 0, HID, l1b, 0});
  gemm(s, n, HID, HID, 1, Mat<false>{h->ah1, 0, HID}, Mat<false>{l2w, 0, HID}, StAct<true>{h->ah2, 0, HID, l2b, 0});
  return l2b + HID;
}

// the learner's own actor up to both heads, mean and clamped log_std: h->head
void actor_heads(Learner* h, hipStream_t s, int n, const float* x, const long long* idx) {
  const float* hw = actor_hidden(h, s, n, x, idx, h->d, h->P);
  gemm(s, n, 2 * ACT, HID, 1, Mat<false>{h->ah2, 0, HID}, HeadW<false>{hw}, StHead{h->head, hw});
}

// the squashed-Gaussian sample of h->head with the caller's N(0,1) draw: h->asmp, h->logp
void sample(Learner* h, hipStream_t s, int n, const float* eps) {
  hipLaunchKernelGGL(k_sample, dim3((n + 15) / 16), dim3(256), 0, s, h->head, eps, n, h->asmp, h->logp);
}

// two critics of observation width d, one critic's size cs, with the weights at `w` (the online arena, a target, a teacher), on
// [x rows (through idx) | a rows (through aidx)]: h->ch1, h->ch2, qout
void critic_forward(Learner* h, hipStream_t s, int n, const float* x, const long long* idx, int d, const float* a, const long long* aidx,
                    long cs, const float* w, float* qout) {
  const int kin = d + ACT;
  const long zh = (long)h->maxb * HID;
  const float* l1w = w;
  const float* l1b = l1w + (size_t)HID * kin;
  const float* l2w = l1b + HID;
  const float* l2b = l2w + (size_t)HID * HID;
  const float* l3w = l2b + HID;
  const float* l3b = l3w + HID;
  gemm(s, n, HID, kin, 2, InCat<false>{x, idx, d, a, aidx, ACT}, Mat<false>{l1w, cs, kin}, StAct<true>{h->ch1, zh, HID, l1b, cs});
  gemm(s, n, HID, HID, 2, Mat<false>{h->ch1, zh, HID}, Mat<false>{l2w, cs, HID}, StAct<true>{h->ch2, zh, HID, l2b, cs});
  gemm(s, n, 1, HID, 2, Mat<false>{h->ch2, zh, HID}, Mat<false>{l3w, cs, HID}, StAct<false>{qout, (long)h->maxb, 1, l3b, cs});
}

// the online critics' offsets of l2.w and l3.w within one critic
size_t critic_l2w(const Learner* h) { return (size_t)HID * (h->d + ACT) + HID; }
size_t critic_l3w(const Learner* h) { return critic_l2w(h) + (size_t)HID * HID + HID; }

// dY1 = (dY2 W2) [h1 > 0] of both online critics from h->dq and the forward pass kept in h->ch1, h->ch2,  dY2 = dq w3 [h2 > 0]: h->dy1
void critic_dy1(Learner* h, hipStream_t s, int n) {
  const long zs = (long)h->csize, zh = (long)h->maxb * HID;
  const float* PC = h->P + h->asize;
  DQ<false> dy2{h->dq, (long)h->maxb, PC + critic_l3w(h), zs, h->ch2, zh};
  gemm(s, n, HID, HID, 2, dy2, Mat<true>{PC + critic_l2w(h), zs, HID}, StMask{h->dy1, zh, HID, h->ch1});
}

// the online critics' 12 gradients from h->dq; `in1` loads the first layer's input [x | a | 1] transposed
void critic_backward(Learner* h, hipStream_t s, int n, InCat<true> in1) {
  const int kin = h->d + ACT;
  const long B = h->maxb, zs = (long)h->csize, zh = B * HID;
  const float* PC = h->P + h->asize;
  float* GC = h->G + h->asize;
  // dW3 | db3 = dq^T [h2 | 1]
  gemm(s, 1, HID + 1, n, 2, Mat<true>{h->dq, B, 1}, MatAug{h->ch2, zh, HID, HID}, StGrad{GC + critic_l3w(h), zs, 1, HID, 0});
  // dW2 | db2 = dY2^T [h1 | 1]
  DQ<true> dy2t{h->dq, B, PC + critic_l3w(h), zs, h->ch2, zh};
  gemm(s, HID, HID + 1, n, 2, dy2t, MatAug{h->ch1, zh, HID, HID}, StGrad{GC + critic_l2w(h), zs, HID, HID, 0});
  critic_dy1(h, s, n);
  // dW1 | db1 = dY1^T [x | a | 1]
  gemm(s, HID, kin + 1, n, 2, Mat<true>{h->dy1, zh, HID}, in1, StGrad{GC, zs, HID, kin, 0});
}

// the actor's 8 gradients from h->dhead and the forward pass kept in h->ah1, h->ah2, on rows of `x` (through idx when given)
void actor_backward(Learner* h, hipStream_t s, int n, const float* x, const long long* idx) {
  const int d = h->d;
  const size_t a_l2w = (size_t)HID * d + HID, a_hw = a_l2w + (size_t)HID * HID + HID;
  // head: dW | db of both heads = dhead^T [h2 | 1];  dh2 = (dhead Whead) [h2 > 0];  then the two hidden layers
  gemm(s, 2 * ACT, HID + 1, n, 1, Mat<true>{h->dhead, 0, 2 * ACT}, MatAug{h->ah2, 0, HID, HID},
       StGrad{h->G + a_hw, 0, ACT, HID, (long)ACT * HID + ACT});
  gemm(s, n, HID, 2 * ACT, 1, Mat<false>{h->dhead, 0, 2 * ACT}, HeadW<true>{h->P + a_hw}, StMask{h->dh2, 0, HID, h->ah2});
  gemm(s, HID, HID + 1, n, 1, Mat<true>{h->dh2, 0, HID}, MatAug{h->ah1, 0, HID, HID}, StGrad{h->G + a_l2w, 0, HID, HID, 0});
  gemm(s, n, HID, HID, 1, Mat<false>{h->dh2, 0, HID}, Mat<true>{h->P + a_l2w, 0, HID}, StMask{h->dh1, 0, HID, h->ah1});
  gemm(s, HID, d + 1, n, 1, Mat<true>{h->dh1, 0, HID}, InCat<true>{x, idx, d, nullptr, nullptr, 0}, StGrad{h->G, 0, HID, d, 0});
}

void adam_actor(Learner* h, hipStream_t s) {
  hipLaunchKernelGGL(k_adam, dim3(512), dim3(256), 0, s, h->P, h->G, h->M, h->V, (long)h->asize, h->actor_lr, h->bc, (float*)nullptr,
                     0.0f, 0.0f);
}

// both critics; with a target, target <- t_new * (the critics just stepped) + t_old * target in the same pass
void adam_critics(Learner* h, hipStream_t s, float* target = nullptr, float t_new = 0.0f, float t_old = 0.0f) {
  hipLaunchKernelGGL(k_adam, dim3(512), dim3(256), 0, s, h->P + h->asize, h->G + h->asize, h->M + h->asize, h->V + h->asize,
                     (long)(2 * h->csize), h->critic_lr, h->bc + 2, target, t_new, t_old);
}

// the end of an update: both losses from their rows, copied out when asked for; `who` is the learner's prefix, "etg_sac" / "etg_bc"
int finish(Learner* h, hipStream_t s, int n, float* losses2, const char* who) {
  hipLaunchKernelGGL(k_loss, dim3(1), dim3(256), 0, s, n, h->maxb, h->rows_c, h->rows_a, h->losses);
  if (losses2 && hipMemcpyAsync(losses2, h->losses, 8, hipMemcpyDeviceToDevice, s) != hipSuccess)
    return fail(ETG_ERR_HIP, who, "copying the losses failed");
  if (hipGetLastError() != hipSuccess) return fail(ETG_ERR_HIP, who, "a launch failed");
  return ETG_OK;
}

}  // namespace
}  // namespace ac
#endif  // AC_LEARNER_H_
