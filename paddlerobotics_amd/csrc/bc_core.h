// bc_core.h -- the elementwise kernels that the behaviour-cloning update (bc_learn.hip) adds to those of sac_core.h.
#ifndef BC_CORE_H_
#define BC_CORE_H_

#include "sac_core.h"

namespace bc {

using sac::ACT;
using sac::bump_step;

// the teacher's action: a_ref = tanh(mean), in place on the mean head's output [n, 12]
static __global__ void __launch_bounds__(256) k_tanh(float* __restrict__ x, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) x[i] = tanhf(x[i]);
}

// Backward of L_a = -mean over n * 12 elements of Normal(mean, exp(ls)).log_prob(a_ref), ls = clamp(raw, -20, 2), from the head's
// pre-activations [n, 24]; 16 lanes per row.  With z = (a_ref - mean) * exp(-ls):
//   -log_prob = z^2 / 2 + ls + log sqrt(2 pi),   d / d mean = -z exp(-ls) / (12 n),   d / d raw = -(z^2 - 1) / (12 n) inside the clamp
// z is formed first and squared afterwards: at the lower clamp exp(-ls) = e^20 and z^2 reaches 1e17, inside fp32's range, whereas
// std^2 = e^-40 is formed nowhere (a quotient by it would round twice more and, for the gradient to the mean, would need
// (a_ref - mean) / std^2 in one step).  rows[b] = the row's 12 terms summed (a fixed butterfly) / 12: k_loss then divides by n.
static __global__ void __launch_bounds__(256) k_nll_bwd(const float* __restrict__ head, const float* __restrict__ aref, int n,
                                                        float* __restrict__ dhead, float* __restrict__ rows, long long* step,
                                                        double* bc) {
  const int row = blockIdx.x * 16 + (threadIdx.x >> 4), c = threadIdx.x & 15;
  if (blockIdx.x == 0 && threadIdx.x == 0 && step) bump_step(step, bc);
  const bool live = row < n && c < ACT;
  float l = 0.0f;
  if (live) {
    const float mean = head[(long)row * 2 * ACT + c], raw = head[(long)row * 2 * ACT + ACT + c];
    const float ls = fminf(fmaxf(raw, -20.0f), 2.0f);
    const float is = expf(-ls), z = (aref[(long)row * ACT + c] - mean) * is;
    const float w = 1.0f / (float)(ACT * n);
    l = 0.5f * z * z + ls + 0.9189385332046727f;
    dhead[(long)row * 2 * ACT + c] = -(z * is) * w;
    dhead[(long)row * 2 * ACT + ACT + c] = (raw >= -20.0f && raw <= 2.0f) ? -(z * z - 1.0f) * w : 0.0f;
  }
  l += __shfl_xor(l, 1); l += __shfl_xor(l, 2); l += __shfl_xor(l, 4); l += __shfl_xor(l, 8);
  if (row < n && c == 0) rows[row] = l / (float)ACT;
}

// critic regression onto the teacher's critics: dq[c] = 2 (q[c] - rq[c]) / n,  rows[c] = (q[c] - rq[c])^2;  q, rq, dq, rows [2, B]
static __global__ void __launch_bounds__(256) k_regress(int n, int B, const float* __restrict__ q, const float* __restrict__ rq,
                                                        float* __restrict__ dq, float* __restrict__ rows, long long* step,
                                                        double* bc) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b == 0 && step) bump_step(step, bc);
  if (b >= n) return;
  const float e1 = q[b] - rq[b], e2 = q[B + b] - rq[B + b];
  const float s = 2.0f / (float)n;
  dq[b] = e1 * s;
  dq[B + b] = e2 * s;
  rows[b] = e1 * e1;
  rows[B + b] = e2 * e2;
}

}  // namespace bc
#endif  // BC_CORE_H_
