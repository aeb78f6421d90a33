// policy_mlp.hip -- the residual-policy forward (the one dense contraction of the path):
//   act = tanh(W3 relu(W2 relu(W1 obs + b1) + b2) + b3) * act_scale
// reference: model/mujoco_model.py:44-60 (Actor.forward, mean head), alg/sac.py:60-63
// (predict = tanh(mean)), train.py:320 (act_bound scaling).  Weights keep torch's
// [out, in] row-major fp32 layout (mujoco_agent.py:61-65 state_dict keys l1/l2/mean_linear).
//
// One launch fuses the three layers.  A workgroup (NW waves, 16 by default) owns 16 consecutive robots;
// its activations (16 x 256 fp32) never leave LDS; the 327 KB of weights are streamed
// from L2 (they are shared by all workgroups and stay L2/MALL-resident).  At 4096 robots
// that is 256 workgroups = one per CU.
//   precision 0: v_mfma_f32_16x16x4_f32  -- exact fp32 (bitwise an fmaf chain)
//   precision 1: v_mfma_f32_16x16x32_bf16 -- operands rounded to bf16 (RNE) in registers
// MFMA operand mapping (16x16 tiles, wave64): lane l holds A[i = l&15][k-slot l>>4] and
// B[k-slot l>>4][j = l&15]; D[row = 4*(l>>4)+r][col = l&15].  The k index a slot covers is
// free as long as A and B agree, so each lane loads a CONTIGUOUS float4 (fp32 path) or
// 8 floats (bf16 path) of its row and feeds one component per MFMA.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/etgsim.h"
#include "dev_buffers.h"
#include "policy_core.h"

namespace {

using namespace pol;
#ifndef ETG_POLICY_WAVES
#define ETG_POLICY_WAVES 16   // measured at 4096 rows: 4 waves 10.6 us, 8 waves 10.1 us, 16 waves 9.5 us (fp32)
#endif
constexpr int NW = ETG_POLICY_WAVES;          // waves per workgroup
constexpr int THREADS = 64 * NW;

// Weights are re-laid out once (etg_policy_load) into MFMA-fragment order so that every wave-level
// weight fetch is ONE fully coalesced 1-KiB global_load_dwordx4:
//   packed[((tile * nkb + kb) * 64 + lane) * 4 + c] = W[tile*16 + (lane & 15)][kb*16 + 4*(lane >> 4) + c]
// (zero outside the matrix).  torch's [out, in] layout stays the API format.
__global__ void k_pack_weights(const float* __restrict__ w, int nout, int kdim, int ntiles, int nkb, float* __restrict__ out) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  const int total = ntiles * nkb * 64 * 4;
  if (idx >= total) return;
  const int c = idx & 3, lane = (idx >> 2) & 63, blk = idx >> 8;
  const int kb = blk % nkb, tile = blk / nkb;
  const int n = tile * 16 + (lane & 15), k = kb * 16 + 4 * (lane >> 4) + c;
  out[idx] = (n < nout && k < kdim) ? w[(size_t)n * kdim + k] : 0.0f;
}

// the per-wave tile's packing of the two hidden layers as ONE stream of k-groups (policy_core.h: wave_hidden12):
//   out[((g * NCHW + chunk) * 64 + lane) * 4 + c] = W[64 chunk + lane][4 k + c],  W = W1, k = g for g < KQ1;  W = W2, k = g - KQ1 after
// (zero outside the matrices): a wave's fetch of one k-group is four coalesced 1-KiB loads at consecutive addresses
__global__ void k_pack_wave12(const float* __restrict__ w1, int in_dim, const float* __restrict__ w2, float* __restrict__ out) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= pol::KG * pol::NCHW * 256) return;
  const int c = idx & 3, lane = (idx >> 2) & 63, blk = idx >> 8;
  const int chunk = blk % pol::NCHW, g = blk / pol::NCHW;
  const int n = 64 * chunk + lane;
  float v;
  if (g < pol::KQ1) { const int k = 4 * g + c; v = k < in_dim ? w1[(size_t)n * in_dim + k] : 0.0f; }
  else { const int k = 4 * (g - pol::KQ1) + c; v = w2[(size_t)n * pol::HID + k]; }
  out[idx] = v;
}

// the per-wave head's packing (policy_core.h: wave_head): out[(kq * 64 + lane) * 4 + c] = W[4 nb + j][64 slice + 4 kq + c] with
// lane = 4 (3 slice + nb) + j, nb < 3, slice < 4; zeros on lanes 48..63 and for neurons >= nout
__global__ void k_pack_head(const float* __restrict__ w, int nout, int kdim, float* __restrict__ out) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= pol::KQH * 256) return;
  const int c = idx & 3, lane = (idx >> 2) & 63, kq = idx >> 8;
  const int blk = lane >> 2, j = lane & 3, slice = blk / 3, nb = blk % 3;
  const int n = 4 * nb + j, k = 64 * slice + 4 * kq + c;
  out[idx] = (slice < 4 && n < nout && k < kdim) ? w[(size_t)n * kdim + k] : 0.0f;
}

// bf16 fragments from the fp32 ones: out[(tile * nkb / 2 + kp) * 64 + lane] = pack_bf16(in[(tile * nkb + 2 kp) * 64 + lane],
// in[(tile * nkb + 2 kp + 1) * 64 + lane]) -- the B operand of v_mfma_f32_16x16x32_bf16 as the kernels used to build it per use
__global__ void k_pack_bf16(const float4* __restrict__ in, int ntiles, int nkb, float4* __restrict__ out) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  const int nkp = nkb / 2;
  if (idx >= ntiles * nkp * 64) return;
  const int lane = idx & 63, blk = idx >> 6;
  const int kp = blk % nkp, tile = blk / nkp;
  const bf16x8 v = pack_bf16(in[(size_t)(tile * nkb + 2 * kp) * 64 + lane], in[(size_t)(tile * nkb + 2 * kp + 1) * 64 + lane]);
  out[idx] = __builtin_bit_cast(float4, v);
}

// SAMPLE = false: act = tanh(mean) * scale                                  (SAC.predict, alg/sac.py:60-63)
// SAMPLE = true : x = mean + exp(clamp(log_std, -20, 2)) * eps, act = tanh(x) * scale, and optionally
//                 logp = sum_j [N(x_j; mean_j, std_j) log-density - log(1 - tanh(x_j)^2 + 1e-6)]
//                 (SAC.sample, alg/sac.py:65-76; clamp of model/mujoco_model.py:58-59); eps is the caller's N(0,1)
template <bool BF16, bool SAMPLE>
__global__ void __launch_bounds__(THREADS) k_policy(const float* __restrict__ obs, int n, int in_dim,
                                                    const float4* __restrict__ w1p, const float* __restrict__ b1,
                                                    const float4* __restrict__ w2p, const float* __restrict__ b2,
                                                    const float4* __restrict__ w3p, const float* __restrict__ b3,
                                                    const float4* __restrict__ w3sp, const float* __restrict__ b3s,
                                                    const float* __restrict__ eps, int out_dim, float scale,
                                                    float* __restrict__ act, float* __restrict__ logp) {
  __shared__ __attribute__((aligned(16))) float bufA[TM * HS];
  __shared__ __attribute__((aligned(16))) float bufB[TM * HS];
  __shared__ float part[SAMPLE ? 2 : 1][NW][TM][16];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int row0 = blockIdx.x * TM;
  // obs tile -> LDS, zero padded (rows past n, columns past in_dim up to the 64-wide padded K)
  for (int idx = tid; idx < TM * 64; idx += THREADS) {
    const int r = idx >> 6, c = idx & 63;
    float v = 0.0f;
    if (c < in_dim && row0 + r < n) v = obs[(size_t)(row0 + r) * in_dim + c];
    bufA[r * HS + c] = v;
  }
  __syncthreads();
  hidden_layer<BF16, 4, NW>(bufA, w1p, b1, bufB, wave, lane);    // K padded to 64 = 4 k-blocks
  __syncthreads();
  hidden_layer<BF16, HID / 16, NW>(bufB, w2p, b2, bufA, wave, lane);
  __syncthreads();
  // output layer: one 16x16 tile per head (out_dim <= 16), K split over the waves
  output_partial<BF16, NW>(bufA, w3p, wave, lane, part[0]);
  if constexpr (SAMPLE) output_partial<BF16, NW>(bufA, w3sp, wave, lane, part[1]);
  __syncthreads();
  {
    const int r = tid >> 4, cidx = tid & 15;  // first 256 threads = 16 rows x 16 cols; a row = one 16-lane DPP row
    if (r >= TM) return;
    const bool live = cidx < out_dim && row0 + r < n;
    // fixed summation order over the NW K-slices
    float v = 0.0f;
#pragma unroll
    for (int q = 0; q < NW; q += 2) v += part[0][q][r][cidx] + part[0][q + 1][r][cidx];
    v += live ? b3[cidx] : 0.0f;
    float lp = 0.0f;
    if constexpr (SAMPLE) {
      float ls = 0.0f;
#pragma unroll
      for (int q = 0; q < NW; q += 2) ls += part[1][q][r][cidx] + part[1][q + 1][r][cidx];
      ls += live ? b3s[cidx] : 0.0f;
      ls = fminf(fmaxf(ls, -20.0f), 2.0f);
      const float e = live ? eps[(size_t)(row0 + r) * out_dim + cidx] : 0.0f;
      v = v + expf(ls) * e;
      const float a = tanhf(v);
      lp = live ? (-0.5f * e * e - ls - 0.9189385332046727f) - logf((1.0f - a * a) + 1e-6f) : 0.0f;
      if (live) act[(size_t)(row0 + r) * out_dim + cidx] = a * scale;
      if (logp) {   // sum over the row's 16 lanes (butterfly inside the DPP row)
        lp += __shfl_xor(lp, 1); lp += __shfl_xor(lp, 2); lp += __shfl_xor(lp, 4); lp += __shfl_xor(lp, 8);
        if (cidx == 0 && row0 + r < n) logp[row0 + r] = lp;
      }
    } else {
      if (live) act[(size_t)(row0 + r) * out_dim + cidx] = tanhf(v) * scale;
    }
  }
}

// ---- observations of 65 .. MAX_IN columns (privileged-dynamics rows, stacked history): k_policy_wide ----
// The same tile as k_policy -- 16 robots per workgroup, NW waves, activations in LDS -- with the observation tile in an LDS
// buffer of its own (16 x Kpad, Kpad = in_dim rounded up to 32 so that the bf16 path's k-block pairs stay whole) and layer 1's K
// in a runtime loop over Kpad / 32 pairs of k-blocks.  w1p holds Kpad / 16 k-blocks per tile (etg_policy_create / _load).
constexpr int MAX_IN = 512;
constexpr int XS = MAX_IN + 4;   // row stride of the observation tile (as HS: rotates the 16-byte slots by one per row)

// out[16][this wave's 16 * TPW columns] = relu(x[16][32 nkp] W1^T + b1).  The accumulators stay in registers over the whole loop;
// the weight fragments of R - 1 pairs are in flight in a register ring of R slots (pair kp lives in slot kp % R; the loop runs in
// groups of R pairs so that the slots are static, and the last nkp % R pairs follow it: their fragments are in the ring by then).
// Summation order of precision 0, per output: ONE fmaf chain (v_mfma_f32_16x16x4_f32 is bitwise an fmaf chain) that starts at
// 0, takes the 16-column k-blocks in ascending order and, inside a k-block, the columns k = 16 kb + 4 g + c with c = 0..3 outer
// and the instruction's four k-slots g = 0..3 inner (the order hidden_layer has); the bias is added after the last block.
template <bool BF16>
__device__ __forceinline__ void wide_layer1(const float* x, const float4* __restrict__ wp, const float* __restrict__ b, float* out,
                                            int nkp, int wave, int lane) {
  constexpr int TPW = (HID / 16) / NW;
  constexpr int R = TPW <= 2 ? 4 : 2;
  constexpr int F = BF16 ? 1 : 2;   // 16-byte fragments per pair and tile: one bf16x8, or the fp32 ones of its two k-blocks
  const int i = lane & 15, g = lane >> 4;
  f32x4 acc[TPW];
#pragma unroll
  for (int t = 0; t < TPW; t++) acc[t] = {0.f, 0.f, 0.f, 0.f};
  const float* xr = x + i * XS + 4 * g;
  const int tstride = nkp * F * 64;
  const float4* base = wp + (size_t)(TPW * wave) * tstride + lane;
  float4 w[R][F][TPW];
  auto fetch = [&](int slot, int kp) {
    const int kq = kp < nkp ? kp : nkp - 1;   // (past the end: the last pair again, unused)
#pragma unroll
    for (int f = 0; f < F; f++)
#pragma unroll
      for (int t = 0; t < TPW; t++) w[slot][f][t] = base[t * tstride + (kq * F + f) * 64];
  };
  auto mac = [&](int slot, int kp) {
    const float4 a0 = *reinterpret_cast<const float4*>(xr + 32 * kp);
    const float4 a1 = *reinterpret_cast<const float4*>(xr + 32 * kp + 16);
    if constexpr (!BF16) {
#pragma unroll
      for (int f = 0; f < F; f++) {
        const float4 a = f ? a1 : a0;
#pragma unroll
        for (int t = 0; t < TPW; t++) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, w[slot][f][t].x, acc[t], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < TPW; t++) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, w[slot][f][t].y, acc[t], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < TPW; t++) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, w[slot][f][t].z, acc[t], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < TPW; t++) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, w[slot][f][t].w, acc[t], 0, 0, 0);
      }
    } else {
      const bf16x8 av = pack_bf16(a0, a1);
#pragma unroll
      for (int t = 0; t < TPW; t++) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, as_bf16x8(w[slot][0][t]), acc[t], 0, 0, 0);
    }
  };
#pragma unroll
  for (int p = 0; p < R - 1; p++) fetch(p, p);
  int kp0 = 0;
#pragma unroll 1
  for (; kp0 + R <= nkp; kp0 += R) {
#pragma unroll
    for (int j = 0; j < R; j++) {
      fetch((j + R - 1) % R, kp0 + j + R - 1);   // into the slot the step before this one read
      __builtin_amdgcn_sched_barrier(0);         // keep the fetches R - 1 pairs ahead (see hidden_layer)
      mac(j, kp0 + j);
    }
  }
#pragma unroll
  for (int j = 0; j < R - 1; j++)
    if (kp0 + j < nkp) mac(j, kp0 + j);   // (wave-uniform)
#pragma unroll
  for (int t = 0; t < TPW; t++) {
    const int col = 16 * TPW * wave + 16 * t + i;
    const float bias = b[col];
#pragma unroll
    for (int r = 0; r < 4; r++) out[(4 * g + r) * HS + col] = fmaxf(acc[t][r] + bias, 0.0f);
  }
}

// Layers 2 and 3 and the head's epilogue of a 16-robot tile whose layer-1 activations are in bufB: the part of the forward that
// does not depend on the observation's width, as k_policy has it (same calls, same order of every sum).  k_policy keeps its
// own text so that the code generated for the <= 64-column path does not move.
template <bool BF16, bool SAMPLE>
__device__ __forceinline__ void policy_tail(float* bufA, float* bufB, float (*part)[NW][TM][16], int tid, int wave, int lane, int n, int row0,
                                            const float4* __restrict__ w2p, const float* __restrict__ b2,
                                            const float4* __restrict__ w3p, const float* __restrict__ b3,
                                            const float4* __restrict__ w3sp, const float* __restrict__ b3s,
                                            const float* __restrict__ eps, int out_dim, float scale,
                                            float* __restrict__ act, float* __restrict__ logp) {
  hidden_layer<BF16, HID / 16, NW>(bufB, w2p, b2, bufA, wave, lane);
  __syncthreads();
  // output layer: one 16x16 tile per head (out_dim <= 16), K split over the waves
  output_partial<BF16, NW>(bufA, w3p, wave, lane, part[0]);
  if constexpr (SAMPLE) output_partial<BF16, NW>(bufA, w3sp, wave, lane, part[1]);
  __syncthreads();
  {
    const int r = tid >> 4, cidx = tid & 15;  // first 256 threads = 16 rows x 16 cols; a row = one 16-lane DPP row
    if (r >= TM) return;
    const bool live = cidx < out_dim && row0 + r < n;
    // fixed summation order over the NW K-slices
    float v = 0.0f;
#pragma unroll
    for (int q = 0; q < NW; q += 2) v += part[0][q][r][cidx] + part[0][q + 1][r][cidx];
    v += live ? b3[cidx] : 0.0f;
    float lp = 0.0f;
    if constexpr (SAMPLE) {
      float ls = 0.0f;
#pragma unroll
      for (int q = 0; q < NW; q += 2) ls += part[1][q][r][cidx] + part[1][q + 1][r][cidx];
      ls += live ? b3s[cidx] : 0.0f;
      ls = fminf(fmaxf(ls, -20.0f), 2.0f);
      const float e = live ? eps[(size_t)(row0 + r) * out_dim + cidx] : 0.0f;
      v = v + expf(ls) * e;
      const float a = tanhf(v);
      lp = live ? (-0.5f * e * e - ls - 0.9189385332046727f) - logf((1.0f - a * a) + 1e-6f) : 0.0f;
      if (live) act[(size_t)(row0 + r) * out_dim + cidx] = a * scale;
      if (logp) {   // sum over the row's 16 lanes (butterfly inside the DPP row)
        lp += __shfl_xor(lp, 1); lp += __shfl_xor(lp, 2); lp += __shfl_xor(lp, 4); lp += __shfl_xor(lp, 8);
        if (cidx == 0 && row0 + r < n) logp[row0 + r] = lp;
      }
    } else {
      if (live) act[(size_t)(row0 + r) * out_dim + cidx] = tanhf(v) * scale;
    }
  }
}

template <bool BF16, bool SAMPLE>
__global__ void __launch_bounds__(THREADS) k_policy_wide(const float* __restrict__ obs, int n, int in_dim,
                                                         const float4* __restrict__ w1p, const float* __restrict__ b1,
                                                         const float4* __restrict__ w2p, const float* __restrict__ b2,
                                                         const float4* __restrict__ w3p, const float* __restrict__ b3,
                                                         const float4* __restrict__ w3sp, const float* __restrict__ b3s,
                                                         const float* __restrict__ eps, int out_dim, float scale,
                                                         float* __restrict__ act, float* __restrict__ logp) {
  __shared__ __attribute__((aligned(16))) float xbuf[TM * XS];
  __shared__ __attribute__((aligned(16))) float bufA[TM * HS];
  __shared__ __attribute__((aligned(16))) float bufB[TM * HS];
  __shared__ float part[SAMPLE ? 2 : 1][NW][TM][16];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int row0 = blockIdx.x * TM;
  const int kpad = (in_dim + 31) & ~31;   // <= MAX_IN (etg_policy_create)
  // obs tile -> LDS: a wave per row, its lanes along the row.  Rows lie in_dim floats apart, so for most widths they are not
  // 16-byte aligned: 4-byte loads, coalesced.  Rows past n and columns in_dim .. kpad - 1 are written as zeros (the weights
  // are zero there, but 0 x whatever the LDS held is not 0)
  for (int r = wave; r < TM; r += NW) {
    const bool live = row0 + r < n;
    const float* src = obs + (size_t)(row0 + r) * in_dim;
    for (int c = lane; c < kpad; c += 64) xbuf[r * XS + c] = (live && c < in_dim) ? src[c] : 0.0f;
  }
  __syncthreads();
  wide_layer1<BF16>(xbuf, w1p, b1, bufB, kpad / 32, wave, lane);
  __syncthreads();
  policy_tail<BF16, SAMPLE>(bufA, bufB, part, tid, wave, lane, n, row0, w2p, b2, w3p, b3, w3sp, b3s, eps, out_dim, scale, act, logp);
}

}  // namespace

static size_t packed_floats(int ntiles, int nkb) { return (size_t)ntiles * nkb * 64 * 4; }

// k-blocks of layer 1 in w1 / w1h: the 64 padded columns of k_policy (and of the closed-loop kernels that read w1), or k_policy_wide's
// Kpad / 16
static int l1_kblocks(int in_dim) { return in_dim <= 64 ? 4 : 2 * ((in_dim + 31) / 32); }

static int pfail(int code, const char* msg) { return dev::fail(code, msg); }   // (one etg_last_error() serves the whole ABI)

// every device array of a policy (sizes in floats), for etg_policy_create and etg_policy_destroy: the packed fp32 weights and the
// biases, the bf16 copies (half the floats), the per-wave tile's packings
static std::vector<dev::Buf> policy_buffers(EtgPolicy* p) {
  const size_t w1 = packed_floats(HID / 16, l1_kblocks(p->in_dim)), w2 = packed_floats(HID / 16, HID / 16), w3 = packed_floats(1, HID / 16);
  const size_t hid = p->hidden, out = p->out_dim, w12q = (size_t)KG * NCHW * 256, w3q = (size_t)KQH * 256;
  auto buf = [](float*& slot, size_t floats) { return dev::Buf{(void**)&slot, floats * 4}; };
  return {buf(p->w1, w1),      buf(p->b1, hid),     buf(p->w2, w2),      buf(p->b2, hid),      buf(p->w3, w3),
          buf(p->b3, out),     buf(p->w3s, w3),     buf(p->b3s, out),    buf(p->w1h, w1 / 2),  buf(p->w2h, w2 / 2),
          buf(p->w3h, w3 / 2), buf(p->w3sh, w3 / 2), buf(p->w12q, w12q), buf(p->w3q, w3q),     buf(p->w3sq, w3q)};
}

extern "C" int etg_policy_create(int in_dim, int hidden, int out_dim, int device, EtgPolicy** out) {
  if (!out || in_dim <= 0 || in_dim > MAX_IN || hidden != HID || out_dim <= 0 || out_dim > 16)
    return pfail(ETG_ERR_BAD_ARG, "etg_policy_create: need in_dim<=512, hidden==256, out_dim<=16");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return pfail(ETG_ERR_NO_DEVICE, "etg_policy_create: no HIP device");
  if (device < 0 || device >= ndev) return pfail(ETG_ERR_BAD_ARG, "etg_policy_create: bad device");
  if (hipSetDevice(device) != hipSuccess) return pfail(ETG_ERR_HIP, "hipSetDevice");
  EtgPolicy* p = new EtgPolicy();   // (value-initialised: has_std = 0, every pointer null)
  p->device = device; p->in_dim = in_dim; p->hidden = hidden; p->out_dim = out_dim;
  if (int rc = dev::alloc(policy_buffers(p), "etg_policy_create")) { etg_policy_destroy(p); return rc; }
  *out = p;
  return ETG_OK;
}

extern "C" int etg_policy_load(EtgPolicy* p, const float* w1, const float* b1, const float* w2, const float* b2,
                               const float* w3, const float* b3, void* stream) {
  if (!p || !w1 || !b1 || !w2 || !b2 || !w3 || !b3) return pfail(ETG_ERR_BAD_ARG, "etg_policy_load: null");
  if (hipSetDevice(p->device) != hipSuccess) return pfail(ETG_ERR_HIP, "hipSetDevice");
  hipStream_t s = (hipStream_t)stream;
  struct { float* d; const float* src; int nout, kdim, ntiles, nkb; float* dh; } pk[] = {
      {p->w1, w1, p->hidden, p->in_dim, HID / 16, l1_kblocks(p->in_dim), p->w1h},
      {p->w2, w2, p->hidden, p->hidden, HID / 16, HID / 16, p->w2h},
      {p->w3, w3, p->out_dim, p->hidden, 1, HID / 16, p->w3h}};
  for (auto& x : pk) {
    const int total = x.ntiles * x.nkb * 256;
    hipLaunchKernelGGL(k_pack_weights, dim3((total + 255) / 256), dim3(256), 0, s, x.src, x.nout, x.kdim, x.ntiles, x.nkb, x.d);
    const int th = x.ntiles * (x.nkb / 2) * 64;
    hipLaunchKernelGGL(k_pack_bf16, dim3((th + 255) / 256), dim3(256), 0, s, (const float4*)x.d, x.ntiles, x.nkb, (float4*)x.dh);
  }
  // the per-wave tile's packing (closed-loop kernels, precision 0; observation rows of up to pol::WS columns)
  if (p->in_dim <= 4 * KQ1)
    hipLaunchKernelGGL(k_pack_wave12, dim3(KG * NCHW), dim3(256), 0, s, w1, p->in_dim, w2, p->w12q);
  hipLaunchKernelGGL(k_pack_head, dim3(KQH), dim3(256), 0, s, w3, p->out_dim, p->hidden, p->w3q);
  struct { float* d; const float* src; size_t n; } c[] = {{p->b1, b1, (size_t)p->hidden}, {p->b2, b2, (size_t)p->hidden},
                                                         {p->b3, b3, (size_t)p->out_dim}};
  for (auto& x : c)
    if (hipMemcpyAsync(x.d, x.src, x.n * 4, hipMemcpyDeviceToDevice, s) != hipSuccess)
      return pfail(ETG_ERR_HIP, "etg_policy_load: hipMemcpyAsync failed");
  if (hipGetLastError() != hipSuccess) return pfail(ETG_ERR_HIP, "etg_policy_load: pack launch failed");
  return ETG_OK;
}

extern "C" int etg_policy_load_std(EtgPolicy* p, const float* w_std, const float* b_std, void* stream) {
  if (!p || !w_std || !b_std) return pfail(ETG_ERR_BAD_ARG, "etg_policy_load_std: null");
  if (hipSetDevice(p->device) != hipSuccess) return pfail(ETG_ERR_HIP, "hipSetDevice");
  hipStream_t s = (hipStream_t)stream;
  const int total = (HID / 16) * 256;
  hipLaunchKernelGGL(k_pack_weights, dim3((total + 255) / 256), dim3(256), 0, s, w_std, p->out_dim, p->hidden, 1, HID / 16, p->w3s);
  hipLaunchKernelGGL(k_pack_bf16, dim3(((HID / 32) * 64 + 255) / 256), dim3(256), 0, s, (const float4*)p->w3s, 1, HID / 16, (float4*)p->w3sh);
  hipLaunchKernelGGL(k_pack_head, dim3(KQH), dim3(256), 0, s, w_std, p->out_dim, p->hidden, p->w3sq);
  if (hipMemcpyAsync(p->b3s, b_std, (size_t)p->out_dim * 4, hipMemcpyDeviceToDevice, s) != hipSuccess)
    return pfail(ETG_ERR_HIP, "etg_policy_load_std: hipMemcpyAsync failed");
  if (hipGetLastError() != hipSuccess) return pfail(ETG_ERR_HIP, "etg_policy_load_std: pack launch failed");
  p->has_std = 1;
  return ETG_OK;
}

#define ETG_POLICY_ARGS obs, n, p->in_dim, (const float4*)p->w1, p->b1, (const float4*)p->w2, p->b2, (const float4*)p->w3, p->b3, \
                        (const float4*)p->w3s, p->b3s
#define ETG_POLICY_ARGS_BF16 obs, n, p->in_dim, (const float4*)p->w1h, p->b1, (const float4*)p->w2h, p->b2, (const float4*)p->w3h, p->b3, \
                             (const float4*)p->w3sh, p->b3s
extern "C" int etg_policy_forward(EtgPolicy* p, const float* obs, int n, float act_scale, int precision, float* act,
                                  void* stream) {
  if (!p || !obs || !act || n <= 0) return pfail(ETG_ERR_BAD_ARG, "etg_policy_forward: bad arguments");
  if (hipSetDevice(p->device) != hipSuccess) return pfail(ETG_ERR_HIP, "hipSetDevice");
  dim3 grid((n + TM - 1) / TM), block(THREADS);
  const bool wide = p->in_dim > 64;   // (<= 64: k_policy, launched exactly as before k_policy_wide existed)
  const auto k32 = wide ? k_policy_wide<false, false> : k_policy<false, false>;
  const auto k16 = wide ? k_policy_wide<true, false> : k_policy<true, false>;
  if (precision == 0)
    hipLaunchKernelGGL(k32, grid, block, 0, (hipStream_t)stream, ETG_POLICY_ARGS, nullptr, p->out_dim, act_scale, act, nullptr);
  else
    hipLaunchKernelGGL(k16, grid, block, 0, (hipStream_t)stream, ETG_POLICY_ARGS_BF16, nullptr, p->out_dim, act_scale, act, nullptr);
  if (hipGetLastError() != hipSuccess) return pfail(ETG_ERR_HIP, "etg_policy_forward: launch failed");
  return ETG_OK;
}

extern "C" int etg_policy_sample(EtgPolicy* p, const float* obs, int n, const float* noise, float act_scale, int precision,
                                 float* act, float* logp, void* stream) {
  if (!p || !obs || !act || !noise || n <= 0) return pfail(ETG_ERR_BAD_ARG, "etg_policy_sample: bad arguments");
  if (!p->has_std) return pfail(ETG_ERR_STATE, "etg_policy_sample: etg_policy_load_std() first");
  if (hipSetDevice(p->device) != hipSuccess) return pfail(ETG_ERR_HIP, "hipSetDevice");
  dim3 grid((n + TM - 1) / TM), block(THREADS);
  const bool wide = p->in_dim > 64;   // (<= 64: k_policy, launched exactly as before k_policy_wide existed)
  const auto k32 = wide ? k_policy_wide<false, true> : k_policy<false, true>;
  const auto k16 = wide ? k_policy_wide<true, true> : k_policy<true, true>;
  if (precision == 0)
    hipLaunchKernelGGL(k32, grid, block, 0, (hipStream_t)stream, ETG_POLICY_ARGS, noise, p->out_dim, act_scale, act, logp);
  else
    hipLaunchKernelGGL(k16, grid, block, 0, (hipStream_t)stream, ETG_POLICY_ARGS_BF16, noise, p->out_dim, act_scale, act, logp);
  if (hipGetLastError() != hipSuccess) return pfail(ETG_ERR_HIP, "etg_policy_sample: launch failed");
  return ETG_OK;
}
#undef ETG_POLICY_ARGS
#undef ETG_POLICY_ARGS_BF16

extern "C" void etg_policy_destroy(EtgPolicy* p) {
  if (!p) return;
  (void)hipSetDevice(p->device);
  dev::release(policy_buffers(p));
  delete p;
}
