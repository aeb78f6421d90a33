// ppo_core.h -- the kernels that the PPO learner (ppo_learn.hip) adds to those of sac_core.h: the rollout's preparation, the GAE
// scan, the advantage normalisation, the clipped surrogate's backward at the head, the value regression and the update's stats.
#ifndef PPO_CORE_H_
#define PPO_CORE_H_

#include "sac_core.h"

namespace ppo {

using sac::ACT;
using sac::bump_step;

constexpr float LOG_SQRT_2PI = 0.9189385332046727f;
constexpr int RED_BLOCKS = 64;   // workgroups of the advantage statistics' first stage: red[2 * RED_BLOCKS] doubles

// Rollout preparation of one chunk: the head's pre-activations [n, 24] = {mean, raw log_std} are kept as head_old, and
// logp_old[row] = sum_c (-eps^2 / 2 - ls - log sqrt(2 pi)), ls = clamp(raw, -20, 2): the exact-eps form (sac_core.h: k_sample), not
// one through u = mean + exp(ls) eps, which has lost eps where std is tiny.  16 lanes per row, a fixed butterfly.
static __global__ void __launch_bounds__(256) k_ppo_prepare(const float* __restrict__ head, const float* __restrict__ eps, int n,
                                                            float* __restrict__ head_old, float* __restrict__ logp_old) {
  const int row = blockIdx.x * 16 + (threadIdx.x >> 4), c = threadIdx.x & 15;
  const bool live = row < n && c < ACT;
  float lp = 0.0f;
  if (live) {
    const long i = (long)row * 2 * ACT + c;
    const float mean = head[i], raw = head[i + ACT];
    const float ls = fminf(fmaxf(raw, -20.0f), 2.0f), e = eps[(long)row * ACT + c];
    head_old[i] = mean;
    head_old[i + ACT] = raw;
    lp = -0.5f * e * e - ls - LOG_SQRT_2PI;
  }
  lp += __shfl_xor(lp, 1); lp += __shfl_xor(lp, 2); lp += __shfl_xor(lp, 4); lp += __shfl_xor(lp, 8);
  if (row < n && c == 0) logp_old[row] = lp;
}

// V = (Q1 + Q2) / 2 of a chunk's rows from the twin critic's output q [2, B]
static __global__ void __launch_bounds__(256) k_value(int n, int B, const float* __restrict__ q, float* __restrict__ v) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b < n) v[b] = 0.5f * (q[b] + q[B + b]);
}

// a product rounded to fp32 on its own: __fmul_rn / __fadd_rn are plain * and + to the compiler, whose default contraction mode fuses
// them into one fma in the backend whatever a pragma says; the empty asm (no instruction, no wait state: etg_nstep.hip's
// mul_then_add) hides where the product came from
__device__ __forceinline__ float mul_alone(float x, float y) {
  float p = __fmul_rn(x, y);
  asm volatile("" : "+v"(p));
  return p;
}

// GAE on step-major [T, N] arrays: one lane per robot walks t = T - 1 .. 0, so a wave's loads of one step are 64 neighbours.
//   delta = (r + (gamma * terminal) * v_next) - v,   A = delta + (gl * (1 - done)) * A_next,   ret = A + v
// with every product and sum rounded on its own, never an fma, which is what makes the result the bits of the stock-torch
// definition.
static __global__ void __launch_bounds__(256) k_gae(int T, int N, const float* __restrict__ rew, const float* __restrict__ term,
                                                    const unsigned char* __restrict__ done, const float* __restrict__ v,
                                                    const float* __restrict__ vn, float gamma, float gl, float* __restrict__ adv,
                                                    float* __restrict__ ret) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= N) return;
  float a = 0.0f;
  for (int t = T - 1; t >= 0; t--) {
    const long i = (long)t * N + r;
    const float vi = v[i];
    const float delta = __fsub_rn(__fadd_rn(rew[i], mul_alone(mul_alone(gamma, term[i]), vn[i])), vi);
    a = __fadd_rn(delta, mul_alone(mul_alone(gl, done[i] ? 0.0f : 1.0f), a));
    adv[i] = a;
    ret[i] = __fadd_rn(a, vi);
  }
}

// the pairwise sum of a workgroup's 256 (sum, sum of squares) pairs in a fixed order; the result is in sm[0][0], sm[1][0]
__device__ inline void reduce2(double (*sm)[256], int t) {
  for (int w = 128; w > 0; w >>= 1) {
    __syncthreads();
    if (t < w) { sm[0][t] += sm[0][t + w]; sm[1][t] += sm[1][t + w]; }
  }
  __syncthreads();
}

// Advantage statistics, first stage: workgroup g of RED_BLOCKS sums x and x^2 in double over the elements g * 256 + t + k * 256 *
// RED_BLOCKS and writes red[2 g], red[2 g + 1].  No atomics: the second stage (k_adv_apply) adds the RED_BLOCKS pairs in a fixed order.
static __global__ void __launch_bounds__(256) k_adv_stats(const float* __restrict__ x, long n, double* __restrict__ red) {
  __shared__ double sm[2][256];
  const int t = threadIdx.x;
  double s = 0.0, ss = 0.0;
  for (long i = (long)blockIdx.x * 256 + t; i < n; i += 256L * RED_BLOCKS) {
    const double xi = (double)x[i];
    s += xi; ss += xi * xi;
  }
  sm[0][t] = s; sm[1][t] = ss;
  reduce2(sm, t);
  if (t == 0) { red[2 * blockIdx.x] = sm[0][0]; red[2 * blockIdx.x + 1] = sm[1][0]; }
}

// second stage and the scaling: every workgroup adds the RED_BLOCKS pairs the same way, mean = s / n, var = ss / n - mean^2 (in
// double: the inputs are fp32, so the cancellation costs nothing an fp32 result sees), then x <- (x - mean) / (sqrt(var) + 1e-8)
// in double, rounded once
static __global__ void __launch_bounds__(256) k_adv_apply(float* __restrict__ x, long n, const double* __restrict__ red) {
  __shared__ double sm[2][256];
  const int t = threadIdx.x;
  sm[0][t] = t < RED_BLOCKS ? red[2 * t] : 0.0;
  sm[1][t] = t < RED_BLOCKS ? red[2 * t + 1] : 0.0;
  reduce2(sm, t);
  const double mean = sm[0][0] / (double)n;
  const double var = fmax(sm[1][0] / (double)n - mean * mean, 0.0);
  const double denom = sqrt(var) + 1e-8;
  for (long i = (long)blockIdx.x * 256 + t; i < n; i += 256L * gridDim.x) x[i] = (float)(((double)x[i] - mean) / denom);
}

// Backward of the clipped surrogate at the head's pre-activations [n, 24]; 16 lanes per row, the row's old head, eps, logp_old and
// advantage read through idx when given.  With z = ((mean_old - mean) + exp(ls_old) eps) exp(-ls):
//   logp = sum_c (-z^2 / 2 - ls - log sqrt(2 pi)),   rho = exp(logp - logp_old),
//   L = -mean(min(rho A, clip(rho, 1 - c, 1 + c) A)) - ent_coef mean(sum_c (ls + 1/2 + log sqrt(2 pi)))
// Storing eps and the old head (not u) keeps z = eps to rounding under unchanged parameters at every log_std: at the lower clamp
// u == mean in fp32.  The row's logp is needed before any dhead, so the butterfly comes first; every lane of the row then holds it.
// The unclipped branch is the active one when A >= 0 and rho <= 1 + c, or A < 0 and rho >= 1 - c: w = rho A / n and
//   d / d mean_c = -w z exp(-ls),   d / d raw_c = -w (z^2 - 1) - ent_coef / n inside the clamp, 0 outside;
// otherwise the surrogate is a constant of the row and only the entropy term remains.
// rows_a[b] = the row's loss term, rows_kl[b] = logp_old - logp, rows_clip[b] = [|rho - 1| > c]: k_ppo_stats takes their means.
static __global__ void __launch_bounds__(256) k_ppo_bwd(const float* __restrict__ head, const float* __restrict__ head_old,
                                                        const float* __restrict__ eps, const float* __restrict__ logp_old,
                                                        const float* __restrict__ adv, const long long* __restrict__ idx, int n,
                                                        float clip, float ent_coef, float* __restrict__ dhead, float* __restrict__ rows_a,
                                                        float* __restrict__ rows_kl, float* __restrict__ rows_clip, long long* step,
                                                        double* bc) {
  const int row = blockIdx.x * 16 + (threadIdx.x >> 4), c = threadIdx.x & 15;
  if (blockIdx.x == 0 && threadIdx.x == 0 && step) bump_step(step, bc);
  const bool live = row < n && c < ACT;
  const long long r = row < n ? (idx ? idx[row] : (long long)row) : 0;
  float lp = 0.0f, ent = 0.0f, z = 0.0f, is = 0.0f, raw = 0.0f;
  if (live) {
    const long i = (long)row * 2 * ACT + c;
    const long long io = r * 2 * ACT + c;
    const float mean = head[i];
    raw = head[i + ACT];
    const float ls = fminf(fmaxf(raw, -20.0f), 2.0f);
    const float lso = fminf(fmaxf(head_old[io + ACT], -20.0f), 2.0f);
    is = expf(-ls);
    z = ((head_old[io] - mean) + expf(lso) * eps[r * ACT + c]) * is;
    lp = -0.5f * z * z - ls - LOG_SQRT_2PI;
    ent = ls + 0.5f + LOG_SQRT_2PI;
  }
  lp += __shfl_xor(lp, 1); lp += __shfl_xor(lp, 2); lp += __shfl_xor(lp, 4); lp += __shfl_xor(lp, 8);
  ent += __shfl_xor(ent, 1); ent += __shfl_xor(ent, 2); ent += __shfl_xor(ent, 4); ent += __shfl_xor(ent, 8);
  if (row >= n) return;
  const float lpo = logp_old[r], a = adv[r];
  const float rho = expf(lp - lpo);
  const bool active = a >= 0.0f ? rho <= 1.0f + clip : rho >= 1.0f - clip;
  const float inv_n = 1.0f / (float)n;
  if (live) {
    const float w = active ? rho * a * inv_n : 0.0f;
    const long i = (long)row * 2 * ACT + c;
    dhead[i] = -(w * z) * is;
    dhead[i + ACT] = (raw >= -20.0f && raw <= 2.0f) ? -w * (z * z - 1.0f) - ent_coef * inv_n : 0.0f;
  }
  if (c == 0) {
    const float rc = fminf(fmaxf(rho, 1.0f - clip), 1.0f + clip);
    rows_a[row] = -fminf(rho * a, rc * a) - ent_coef * ent;
    rows_kl[row] = lpo - lp;
    rows_clip[row] = fabsf(rho - 1.0f) > clip ? 1.0f : 0.0f;
  }
}

// the value regression of both critics onto the one target row ret (through idx when given): dq[c] = 2 (q[c] - ret) / n,
// rows[c] = (q[c] - ret)^2;  q, dq, rows [2, B]
static __global__ void __launch_bounds__(256) k_value_dq(int n, int B, const float* __restrict__ q, const float* __restrict__ ret,
                                                         const long long* __restrict__ idx, float* __restrict__ dq,
                                                         float* __restrict__ rows, long long* step, double* bc) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b == 0 && step) bump_step(step, bc);
  if (b >= n) return;
  const float y = ret[idx ? idx[b] : (long long)b];
  const float e1 = q[b] - y, e2 = q[B + b] - y;
  const float s = 2.0f / (float)n;
  dq[b] = e1 * s;
  dq[B + b] = e2 * s;
  rows[b] = e1 * e1;
  rows[B + b] = e2 * e2;
}

// stats = {mean(rows_c[0]) + mean(rows_c[1]), mean(rows_a), mean(rows_kl), mean(rows_clip)}: one workgroup, a fixed summation order
static __global__ void __launch_bounds__(256) k_ppo_stats(int n, int B, const float* __restrict__ rows_c, const float* __restrict__ rows_a,
                                                          const float* __restrict__ rows_kl, const float* __restrict__ rows_clip,
                                                          float* __restrict__ stats) {
  __shared__ float sm[5][256];
  const int t = threadIdx.x;
  float s[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  for (int b = t; b < n; b += 256) { s[0] += rows_c[b]; s[1] += rows_c[B + b]; s[2] += rows_a[b]; s[3] += rows_kl[b]; s[4] += rows_clip[b]; }
#pragma unroll
  for (int j = 0; j < 5; j++) sm[j][t] = s[j];
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) {
#pragma unroll
      for (int j = 0; j < 5; j++) sm[j][t] += sm[j][t + w];
    }
    __syncthreads();
  }
  if (t == 0) {
    stats[0] = sm[0][0] / (float)n + sm[1][0] / (float)n;
    stats[1] = sm[2][0] / (float)n;
    stats[2] = sm[3][0] / (float)n;
    stats[3] = sm[4][0] / (float)n;
  }
}

// ------------------------------------------------------------------------------------------------- the update's controls
// Gradient-norm clipping, value clipping and the KL rule (include/etgsim_ppo.h "Controls").  What they decide -- the clip
// coefficient, the learning-rate scale, whether the update is applied -- is decided on the device from device memory:
//   ctl[0] = lr_scale, ctl[1] / ctl[2] = the gradient norm of the actor's / the critics' last applied step (doubles)
//   flag[0] = 1 while the updates are stopped (int)
constexpr int NORM_BLOCKS = 64;   // workgroups of the squared-norm reduction: part[NORM_BLOCKS] doubles per region

// Sum of squares of a flat region of G, first stage: workgroup g sums, in double, the float4s g * 256 + t + k * 256 * NORM_BLOCKS,
// workgroup 0's first lanes add the region's tail (n & 3 floats), the workgroup's 256 sums are added in the LDS tree's fixed order
// and part[g] gets the result.  No atomics: the second stage (k_adam_ctl) adds the NORM_BLOCKS partials in a fixed order.
static __global__ void __launch_bounds__(256) k_sqnorm(const float* __restrict__ G, long n, double* __restrict__ part) {
  __shared__ double sm[256];
  const int t = threadIdx.x;
  const long n4 = n >> 2;
  double s = 0.0;
  for (long i = (long)blockIdx.x * 256 + t; i < n4; i += 256L * NORM_BLOCKS) {
    const float4 g = ((const float4*)G)[i];
    s += (double)g.x * (double)g.x; s += (double)g.y * (double)g.y; s += (double)g.z * (double)g.z; s += (double)g.w * (double)g.w;
  }
  if (blockIdx.x == 0 && (n4 << 2) + t < n) {
    const double x = (double)G[(n4 << 2) + t];
    s += x * x;
  }
  sm[t] = s;
  for (int w = 128; w > 0; w >>= 1) {
    __syncthreads();
    if (t < w) sm[t] += sm[t + w];
  }
  if (t == 0) part[blockIdx.x] = sm[0];
}

// The controller, one workgroup, between the actor's backward pass and its Adam step.  kl = mean(rows_kl) is summed exactly as
// k_ppo_stats sums it (lane t takes rows t, t + 256, ..; the same tree; / (float) n), so the number judged is the number reported.
//   mode 0 (stop):      kl > 1.5 target sets flag[0]
//   mode 1 (adaptive):  kl > 2 target: scale /= 1.5;  else 0 < kl < target / 2: scale *= 1.5;  then scale into [smin, smax]
// (target <= 0: no rule).  With the flag clear afterwards, both optimizers' step counts and bias corrections are bumped: this
// update will be applied.  With it set nothing is counted, and k_adam_ctl writes nothing.
static __global__ void __launch_bounds__(256) k_ppo_ctl(int n, const float* __restrict__ rows_kl, double target, int mode, double smin,
                                                        double smax, double* __restrict__ ctl, int* __restrict__ flag,
                                                        long long* __restrict__ steps, double* __restrict__ bc) {
  __shared__ float sm[256];
  const int t = threadIdx.x;
  float s = 0.0f;
  for (int b = t; b < n; b += 256) s += rows_kl[b];
  sm[t] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) sm[t] += sm[t + w];
    __syncthreads();
  }
  if (t != 0) return;
  const double kl = (double)(sm[0] / (float)n);
  int stopped = flag[0];
  if (target > 0.0 && !stopped) {
    if (mode == 0) {
      if (kl > 1.5 * target) { stopped = 1; flag[0] = 1; }
    } else {
      double scale = ctl[0];
      if (kl > 2.0 * target) scale /= 1.5;
      else if (kl > 0.0 && kl < target / 2.0) scale *= 1.5;
      ctl[0] = fmin(fmax(scale, smin), smax);
    }
  }
  if (!stopped) { bump_step(steps, bc); bump_step(steps + 1, bc + 2); }
}

// k_adam (sac_core.h) without a target, adam1 call for call, under the controls: nothing is written while flag[0] is set; the
// gradient is g * coef, rounded once, with coef = min(1, max_norm / (norm + 1e-6)) in fp32 from norm = (float) sqrt(sum of the
// NORM_BLOCKS partials of k_sqnorm), every workgroup adding them in the same tree (part == NULL: coef = 1); the step is
// -(float)((lr * lr_scale) / bc[0]) with the product formed in double.  coef == 1, lr_scale == 1 and a clear flag give k_adam's bits:
// g * 1.0f is g and lr * 1.0 is lr.  Workgroup 0 leaves the norm in *norm_out.
static __global__ void __launch_bounds__(256) k_adam_ctl(float* __restrict__ P, const float* __restrict__ G, float* __restrict__ M,
                                                         float* __restrict__ V, long n, double lr, const double* __restrict__ bc,
                                                         const double* __restrict__ part, float max_norm, const double* __restrict__ ctl,
                                                         const int* __restrict__ flag, double* __restrict__ norm_out) {
  __shared__ double sm[NORM_BLOCKS];
  if (flag[0]) return;   // the same word for every lane of the launch: nobody is left at the barriers below
  float coef = 1.0f;
  if (part) {
    const int t = threadIdx.x;
    if (t < NORM_BLOCKS) sm[t] = part[t];
    for (int w = NORM_BLOCKS / 2; w > 0; w >>= 1) {
      __syncthreads();
      if (t < w) sm[t] += sm[t + w];
    }
    __syncthreads();
    const float norm = (float)sqrt(sm[0]);
    coef = fminf(1.0f, __fdiv_rn(max_norm, __fadd_rn(norm, 1e-6f)));
    if (blockIdx.x == 0 && t == 0) *norm_out = (double)norm;
  }
  const float nstep = -(float)((lr * ctl[0]) / bc[0]), bc2s = (float)bc[1];
  const long n4 = n >> 2, stride = (long)gridDim.x * 256;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
    float4 p = ((float4*)P)[i], m = ((float4*)M)[i], v = ((float4*)V)[i];
    const float4 g = ((const float4*)G)[i];
    sac::adam1(p.x, __fmul_rn(g.x, coef), m.x, v.x, nstep, bc2s); sac::adam1(p.y, __fmul_rn(g.y, coef), m.y, v.y, nstep, bc2s);
    sac::adam1(p.z, __fmul_rn(g.z, coef), m.z, v.z, nstep, bc2s); sac::adam1(p.w, __fmul_rn(g.w, coef), m.w, v.w, nstep, bc2s);
    ((float4*)P)[i] = p; ((float4*)M)[i] = m; ((float4*)V)[i] = v;
  }
  const long i = (n4 << 2) + (long)blockIdx.x * 256 + threadIdx.x;   // the region's tail (fewer than 4 floats)
  if (i < n) {
    float p = P[i], m = M[i], v = V[i];
    sac::adam1(p, __fmul_rn(G[i], coef), m, v, nstep, bc2s);
    P[i] = p; M[i] = m; V[i] = v;
  }
}

// k_value_dq with PPO2's clipped value loss against v_old, the value at collection time (through idx when given), clip range c:
//   d = q - v_old,  inside = |d| <= c,  vclip = v_old + clamp(d, -c, c),  e1 = (q - ret)^2,  e2 = (vclip - ret)^2
// the row's loss is e1 with dq = 2 (q - ret) / n where inside or e1 >= e2; otherwise e2, a constant of the row, with dq = 0
static __global__ void __launch_bounds__(256) k_value_dq_clip(int n, int B, const float* __restrict__ q, const float* __restrict__ ret,
                                                              const float* __restrict__ v_old, const long long* __restrict__ idx,
                                                              float c, float* __restrict__ dq, float* __restrict__ rows) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= n) return;
  const long long r = idx ? idx[b] : (long long)b;
  const float y = ret[r], vo = v_old[r];
  const float s = 2.0f / (float)n;
#pragma unroll
  for (int z = 0; z < 2; z++) {
    const float qi = q[z * B + b];
    const float d = qi - vo, e = qi - y;
    const float ec = (vo + fminf(fmaxf(d, -c), c)) - y;
    const float e1 = e * e, e2 = ec * ec;
    const bool first = fabsf(d) <= c || e1 >= e2;
    dq[z * B + b] = first ? e * s : 0.0f;
    rows[z * B + b] = first ? e1 : e2;
  }
}

// the control state written from the host without a copy from its memory: which & 1 sets lr_scale, which & 2 the stop flag
static __global__ void k_ctl_set(double* __restrict__ ctl, int* __restrict__ flag, int which, double scale, int stopped) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (which & 1) ctl[0] = scale;
  if (which & 2) flag[0] = stopped;
}

}  // namespace ppo
#endif  // PPO_CORE_H_
