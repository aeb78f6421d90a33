// sac_core.h -- device side of the SAC learner (sac_learn.hip): the tiled fp32-MFMA contraction with functor loaders / stores, and
// the elementwise kernels of one update.
#ifndef SAC_CORE_H_
#define SAC_CORE_H_

#include <hip/hip_runtime.h>

namespace sac {

typedef float v4f __attribute__((ext_vector_type(4)));

constexpr int HID = 256, ACT = 12;
constexpr int TM = 32, TN = 32, TK = 32, LS = TK + 1;   // workgroup tile, k chunk, LDS row stride (odd: no bank conflicts)
constexpr int HEADB = ACT * HID + ACT;                  // floats from mean_linear.weight to std_linear.weight in the arena

// ---------------------------------------------------------------------------------------------------------------- operands
// An operand functor is f(z, r, k): element (row r of the output tile's side, reduction index k) of batch entry z (the critic).
// kfast() says which of r / k is the contiguous one in memory, so that the staging loop reads coalesced.

template <bool T>
struct Mat {   // T = false: p[z][r][k];  T = true: p[z][k][r]
  const float* p; long zs; int ld;
  __device__ bool kfast() const { return !T; }
  __device__ float operator()(int z, int r, int k) const { return T ? p[z * zs + (long)k * ld + r] : p[z * zs + (long)r * ld + k]; }
};

struct MatAug {   // [X | 1] transposed: r < k0 ? p[z][k][r] : 1 -- the ones column turns the bias gradient into a column of dW
  const float* p; long zs; int ld, k0;
  __device__ bool kfast() const { return false; }
  __device__ float operator()(int z, int r, int k) const { return r < k0 ? p[z * zs + (long)k * ld + r] : 1.0f; }
};

template <bool T>
struct InCat {   // [obs | act | 1] of batch row b (through the row indices when given); T = false: (r, k) = (b, c), T = true: (c, b)
  const float* obs; const long long* oidx; int d;
  const float* act; const long long* aidx; int na;
  __device__ bool kfast() const { return !T; }
  __device__ float operator()(int, int r, int k) const {
    const int b = T ? k : r, c = T ? r : k;
    if (c < d) return obs[(oidx ? oidx[b] : (long long)b) * d + c];
    if (c < d + na) return act[(aidx ? aidx[b] : (long long)b) * na + (c - d)];
    return 1.0f;
  }
};

template <bool T>
struct DQ {   // dY of a critic's second layer: dq[z][b] * w3[z][j] * [h2[z][b][j] > 0];  T = false: (r, k) = (b, j), T = true: (j, b)
  const float* dq; long zq; const float* w3; long zw; const float* h2; long zh;
  __device__ bool kfast() const { return !T; }
  __device__ float operator()(int z, int r, int k) const {
    const int b = T ? k : r, j = T ? r : k;
    return h2[z * zh + (long)b * HID + j] > 0.0f ? dq[z * zq + b] * w3[z * zw + j] : 0.0f;
  }
};

template <bool T>
struct HeadW {   // the two 12 x 256 heads as one 24 x 256 matrix;  T = false: (r, k) = (n24, col), T = true: (col, n24)
  const float* w;
  __device__ bool kfast() const { return !T; }
  __device__ float operator()(int, int r, int k) const {
    const int n = T ? k : r, c = T ? r : k;
    return w[(n / ACT) * HEADB + (n % ACT) * HID + c];
  }
};

struct Cat2 {   // both critics' dY1 side by side: [b][512]
  const float* p; long zs;
  __device__ bool kfast() const { return true; }
  __device__ float operator()(int, int r, int k) const { return p[(k >> 8) * zs + (long)r * HID + (k & 255)]; }
};

struct W1Act {   // the action columns of both critics' first layers: (r, k) = (action i, 256 critic + neuron)
  const float* w; long zs; int kin, d;
  __device__ bool kfast() const { return false; }
  __device__ float operator()(int, int r, int k) const { return w[(k >> 8) * zs + (long)(k & 255) * kin + d + r]; }
};

// ------------------------------------------------------------------------------------------------------------------ stores
template <bool RELU>
struct StAct {   // out[z][m][n] = act(acc + bias[z][n])
  float* out; long zs; int ld; const float* bias; long zb;
  __device__ void operator()(int z, int m, int n, float v) const {
    v += bias[z * zb + n];
    out[z * zs + (long)m * ld + n] = RELU ? fmaxf(v, 0.0f) : v;
  }
};

struct StHead {   // head[m][24] = acc + {mean, std} bias
  float* out; const float* w;
  __device__ void operator()(int, int m, int n, float v) const { out[(long)m * 2 * ACT + n] = v + w[(n / ACT) * HEADB + ACT * HID + n % ACT]; }
};

struct StMask {   // out = [h > 0] acc, same shape
  float* out; long zs; int ld; const float* h;
  __device__ void operator()(int z, int m, int n, float v) const {
    const long i = z * zs + (long)m * ld + n;
    out[i] = h[i] > 0.0f ? v : 0.0f;
  }
};

struct StGrad {   // weight [rb, k0] followed by bias [rb], repeated every bs floats for row blocks of rb rows; column k0 = the bias
  float* g; long zs; int rb, k0; long bs;
  __device__ void operator()(int z, int m, int n, float v) const {
    const int blk = m / rb, mr = m % rb;
    g[z * zs + blk * bs + (n < k0 ? (long)mr * k0 + n : (long)rb * k0 + mr)] = v;
  }
};

struct StPlain {
  float* out; int ld;
  __device__ void operator()(int, int m, int n, float v) const { out[(long)m * ld + n] = v; }
};

// -------------------------------------------------------------------------------------------------------------------- GEMM
// C[z][m][n] = sum_k fa(z, m, k) * fb(z, n, k), one 32 x 32 tile per workgroup of 4 waves (a 16 x 16 MFMA tile each), the whole
// k range in the workgroup in a fixed order: 32 products per partial sum, 16 partial sums per middle sum, middle sums into the total
// (a plain chain over a batch of 256 .. 4096 rows loses more bits in the bias gradients than torch's pairwise reductions do).
// v_mfma_f32_16x16x4_f32: lane l holds A[i = l & 15][k slot l >> 4] and B[k slot l >> 4][j = l & 15]; D[row 4 (l >> 4) + r][col l & 15].
// Elements outside M / N / K are zeros and are not fetched.
template <class FA, class FB, class ST>
__global__ void __launch_bounds__(256) k_gemm(int M, int N, int K, FA fa, FB fb, ST st) {
  __shared__ float As[TM * LS];
  __shared__ float Bs[TN * LS];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int z = blockIdx.z, m0 = blockIdx.y * TM, n0 = blockIdx.x * TN;
  const int wm = (wave >> 1) * 16, wn = (wave & 1) * 16;
  const bool akf = fa.kfast(), bkf = fb.kfast();
  v4f acc = {0.0f, 0.0f, 0.0f, 0.0f}, mid = acc;
  for (int k0 = 0, chunk = 1; k0 < K; k0 += TK, chunk++) {
    v4f part = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int e = 0; e < (TM * TK) / 256; e++) {
      const int idx = tid + 256 * e, lo = idx & 31, hi = idx >> 5;
      {
        const int i = akf ? hi : lo, kk = akf ? lo : hi;
        float v = 0.0f;
        if (m0 + i < M && k0 + kk < K) v = fa(z, m0 + i, k0 + kk);
        As[i * LS + kk] = v;
      }
      {
        const int j = bkf ? hi : lo, kk = bkf ? lo : hi;
        float v = 0.0f;
        if (n0 + j < N && k0 + kk < K) v = fb(z, n0 + j, k0 + kk);
        Bs[j * LS + kk] = v;
      }
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < TK / 4; s++) {
      const int kk = 4 * s + (lane >> 4);
      part = __builtin_amdgcn_mfma_f32_16x16x4f32(As[(wm + (lane & 15)) * LS + kk], Bs[(wn + (lane & 15)) * LS + kk], part, 0, 0, 0);
    }
    mid += part;
    if ((chunk & 15) == 0 || k0 + TK >= K) { acc += mid; mid = v4f{0.0f, 0.0f, 0.0f, 0.0f}; }
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int m = m0 + wm + 4 * (lane >> 4) + r, n = n0 + wn + (lane & 15);
    if (m < M && n < N) st(z, m, n, acc[r]);
  }
}

// ------------------------------------------------------------------------------------------------------------- elementwise
// The elementwise kernels are `static`: sac_learn.hip and bc_learn.hip both include this header, and each gets its own copy.
// SAC.sample (alg/sac.py:65-76) from the head's pre-activations [n, 24] = {mean, log_std before the clamp}: 16 lanes per row.
// A deliberate departure from the reference's fp32 arithmetic: Normal.log_prob evaluates -(x_t - mean)^2 / (2 std^2) with
// x_t = mean + std * eps already rounded, so where std is tiny (log_std clamped at -20) x_t == mean in fp32 and its term is 0; here
// the term is -eps^2 / 2, its exact value (what an fp64 run of the reference gives), as csrc/policy_mlp.hip's sample does.  It
// enters logp' of the TD target and the reported actor loss; the gradients do not depend on it.
static __global__ void __launch_bounds__(256) k_sample(const float* __restrict__ head, const float* __restrict__ eps, int n,
                                                       float* __restrict__ act, float* __restrict__ logp) {
  const int row = blockIdx.x * 16 + (threadIdx.x >> 4), c = threadIdx.x & 15;
  const bool live = row < n && c < ACT;
  float lp = 0.0f;
  if (live) {
    const float mean = head[(long)row * 2 * ACT + c];
    const float ls = fminf(fmaxf(head[(long)row * 2 * ACT + ACT + c], -20.0f), 2.0f);
    const float e = eps[(long)row * ACT + c];
    const float a = tanhf(mean + expf(ls) * e);
    act[(long)row * ACT + c] = a;
    lp = (-0.5f * e * e - ls - 0.9189385332046727f) - logf((1.0f - a * a) + 1e-6f);
  }
  lp += __shfl_xor(lp, 1); lp += __shfl_xor(lp, 2); lp += __shfl_xor(lp, 4); lp += __shfl_xor(lp, 8);
  if (row < n && c == 0) logp[row] = lp;
}

// a new optimizer step: the count and its two bias corrections (torch.optim.Adam: 1 - beta1^t and sqrt(1 - beta2^t), in double)
__device__ inline void bump_step(long long* step, double* bc) {
  const long long t = *step + 1;
  *step = t;
  bc[0] = 1.0 - pow(0.9, (double)t);
  bc[1] = sqrt(1.0 - pow(0.999, (double)t));
}

// y = reward + gamma * terminal * (min(Q1t, Q2t) - alpha * logp');  dq[c] = 2 (q[c] - y) / n;  rows[c] = (q[c] - y)^2
static __global__ void __launch_bounds__(256) k_td(int n, int B, const float* __restrict__ rew, const float* __restrict__ term,
                                                   const long long* __restrict__ idx, const float* __restrict__ qt,
                                                   const float* __restrict__ logp, const float* __restrict__ q, float gamma, float alpha,
                                                   float* __restrict__ dq, float* __restrict__ rows, long long* step, double* bc) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b == 0 && step) bump_step(step, bc);
  if (b >= n) return;
  const long long r = idx ? idx[b] : (long long)b;
  const float tq = fminf(qt[b], qt[B + b]) - alpha * logp[b];
  const float y = rew[r] + gamma * term[r] * tq;
  const float e1 = q[b] - y, e2 = q[B + b] - y;
  const float s = 2.0f / (float)n;
  dq[b] = e1 * s;
  dq[B + b] = e2 * s;
  rows[b] = e1 * e1;
  rows[B + b] = e2 * e2;
}

// actor loss rows alpha * logp - min(Q1, Q2) and d loss / d q: -1 / n on the smaller critic of the row
static __global__ void __launch_bounds__(256) k_actor_dq(int n, int B, const float* __restrict__ q, const float* __restrict__ logp,
                                                         float alpha, float* __restrict__ dq, float* __restrict__ rows, long long* step,
                                                         double* bc) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b == 0 && step) bump_step(step, bc);
  if (b >= n) return;
  const float q1 = q[b], q2 = q[B + b], g = -1.0f / (float)n;
  const bool first = q1 <= q2;
  dq[b] = first ? g : 0.0f;
  dq[B + b] = first ? 0.0f : g;
  rows[b] = alpha * logp[b] - fminf(q1, q2);
}

// backward of the sample: da = d loss / d action through the critics;  x = mean + exp(ls) eps, a = tanh(x),
// logp_j = -eps^2 / 2 - ls - c - log(1 - a^2 + 1e-6):  d logp / d x = 2 a (1 - a^2) / (1 - a^2 + 1e-6),  d logp / d ls = -1 directly;
// the clamp of log_std passes a gradient inside [-20, 2] only
static __global__ void __launch_bounds__(256) k_head_bwd(const float* __restrict__ head, const float* __restrict__ eps,
                                                         const float* __restrict__ da, int n, float alpha, float* __restrict__ dhead) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n * ACT) return;
  const int row = i / ACT, c = i % ACT;
  const float mean = head[(long)row * 2 * ACT + c], raw = head[(long)row * 2 * ACT + ACT + c];
  const float ls = fminf(fmaxf(raw, -20.0f), 2.0f), e = eps[i];
  const float sd = expf(ls), a = tanhf(mean + sd * e);
  const float w = alpha / (float)n, om = 1.0f - a * a;
  const float gx = da[i] * om + w * (2.0f * a * om / (om + 1e-6f));
  dhead[(long)row * 2 * ACT + c] = gx;
  dhead[(long)row * 2 * ACT + ACT + c] = (raw >= -20.0f && raw <= 2.0f) ? gx * sd * e - w : 0.0f;
}

// losses = {mean(rows_c[0]) + mean(rows_c[1]), mean(rows_a)}: one workgroup, a fixed summation order
static __global__ void __launch_bounds__(256) k_loss(int n, int B, const float* __restrict__ rows_c, const float* __restrict__ rows_a,
                                                     float* __restrict__ losses) {
  __shared__ float sm[3][256];
  const int t = threadIdx.x;
  float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
  for (int b = t; b < n; b += 256) { s0 += rows_c[b]; s1 += rows_c[B + b]; s2 += rows_a[b]; }
  sm[0][t] = s0; sm[1][t] = s1; sm[2][t] = s2;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) { sm[0][t] += sm[0][t + w]; sm[1][t] += sm[1][t + w]; sm[2][t] += sm[2][t + w]; }
    __syncthreads();
  }
  if (t == 0) {
    losses[0] = sm[0][0] / (float)n + sm[1][0] / (float)n;
    losses[1] = sm[2][0] / (float)n;
  }
}

// torch.optim.Adam (defaults) on a flat region, and when `target` is given the soft update target <- tau p + (1 - tau) target
// of the same region with the parameters just stepped.  Products and sums are rounded one by one as torch's separate kernels do.
__device__ inline void adam1(float& p, float g, float& m, float& v, float nstep, float bc2s) {
  m = __fadd_rn(m, __fmul_rn(0.1f, __fsub_rn(g, m)));
  v = __fadd_rn(__fmul_rn(v, 0.999f), __fmul_rn(__fmul_rn(0.001f, g), g));
  const float denom = __fadd_rn(__fdiv_rn(__fsqrt_rn(v), bc2s), 1e-8f);
  p = __fadd_rn(p, __fmul_rn(nstep, __fdiv_rn(m, denom)));
}

static __global__ void __launch_bounds__(256) k_adam(float* __restrict__ P, const float* __restrict__ G, float* __restrict__ M,
                                                     float* __restrict__ V, long n, double lr, const double* __restrict__ bc,
                                                     float* __restrict__ target, float tau, float decay) {
  const float nstep = -(float)(lr / bc[0]), bc2s = (float)bc[1];
  const long n4 = n >> 2, stride = (long)gridDim.x * 256;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
    float4 p = ((float4*)P)[i], m = ((float4*)M)[i], v = ((float4*)V)[i];
    const float4 g = ((const float4*)G)[i];
    adam1(p.x, g.x, m.x, v.x, nstep, bc2s); adam1(p.y, g.y, m.y, v.y, nstep, bc2s);
    adam1(p.z, g.z, m.z, v.z, nstep, bc2s); adam1(p.w, g.w, m.w, v.w, nstep, bc2s);
    ((float4*)P)[i] = p; ((float4*)M)[i] = m; ((float4*)V)[i] = v;
    if (target) {
      float4 t = ((float4*)target)[i];
      t.x = __fadd_rn(__fmul_rn(tau, p.x), __fmul_rn(decay, t.x)); t.y = __fadd_rn(__fmul_rn(tau, p.y), __fmul_rn(decay, t.y));
      t.z = __fadd_rn(__fmul_rn(tau, p.z), __fmul_rn(decay, t.z)); t.w = __fadd_rn(__fmul_rn(tau, p.w), __fmul_rn(decay, t.w));
      ((float4*)target)[i] = t;
    }
  }
  const long i = (n4 << 2) + (long)blockIdx.x * 256 + threadIdx.x;   // the region's tail (fewer than 4 floats)
  if (i < n) {
    float p = P[i], m = M[i], v = V[i];
    adam1(p, G[i], m, v, nstep, bc2s);
    P[i] = p; M[i] = m; V[i] = v;
    if (target) target[i] = __fadd_rn(__fmul_rn(tau, p), __fmul_rn(decay, target[i]));
  }
}

}  // namespace sac
#endif  // SAC_CORE_H_
