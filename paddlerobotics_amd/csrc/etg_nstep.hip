// etg_nstep.hip -- the n-step writer of the replay memory (include/etgsim_nstep.h): from the records of K control steps and
// the history of the n-1 steps before them, the rows that close in those steps -- the discounted reward sum, the discounted
// bootstrap flag, the start step's obs / action and the closing step's next_obs -- compacted into the ring.
//
// The same kind of work as etg_replay.hip and etg_monitor.hip: HBM-bound counting, scanning and row copies (about 0.9 KB
// moved per row at 49 + 12 columns).  Three launches per feed, no atomics:
//
//   k_nstep_scan   one workgroup per step: every robot's number of closing rows (0..n), scanned per group of 64 robots with
//                  shuffles and across the groups through LDS: per (step, robot) the rows that close in the step at robots
//                  before it, and the step's total
//   k_nstep_rows   one wave per (step, robot), the lane is the column: the wave walks back from the closing step, R and g
//                  one multiply and one add per step (all lanes alike; lane j fetched the reward of step j back), and copies a row where
//                  one closes: every start of a finished episode, or the one start n-1 steps back.  A step before the fed
//                  ones is read from the history ring.  Row number = pos + (rows of earlier steps) + (rows at robots before
//                  it) + (older starts of the robot): closing step, robot, start ascending, whatever order the waves run in
//   k_nstep_tail   the last min(K, n-1) fed steps into the history ring (row = step number % (n-1)), next_obs / terminal of
//                  the newest step, every robot's pending starts, and pos_count
//
// The rows kernel only reads the history ring and pos_count; the tail kernel, behind it on the stream, writes them.  A flush
// is the same scan and rows kernels over one virtual step whose rows all come from the ring, and a one-wave pos_count update.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/etgsim_nstep.h"
#include "dev_buffers.h"

namespace {

constexpr int SCAN_BLOCK = 1024, ROW_BLOCK = 256, ROW_WAVES = ROW_BLOCK / 64;

struct Args {
  int N, K, n, hist, D, A;
  int ring0;                       // step0 % (n - 1): the history ring's row of the first fed step (0 with n = 1)
  float gamma;
  long long max_size;
  const float *rec_obs, *rec_act, *rec_rew, *rec_next, *rec_term;
  const uint8_t* rec_done;
  const int* rec_len;
  float *h_obs, *h_act, *h_rew, *tail_next, *tail_term;
  int* pend;
  float *m_obs, *m_act, *m_rew, *m_next, *m_term;
  long long* pc;
  int* scratch;                    // [K] rows closing per step, then [K,N] rows closing in the step at robots before this one
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// steps of the robot's running episode the writer has seen up to fed step s, cut at n: min(n, avail)
__device__ __forceinline__ int seen(const Args& a, int s, int i) {
  const long long upto = (long long)a.hist + s + 1;             // min(t + 1, n - 1 + s + 1): the same once cut at n
  const int have = (int)min(upto, (long long)a.n);
  return clampi(a.rec_len[(size_t)s * a.N + i], 0, have);
}
// rows that close at fed step s of robot i
template <bool FLUSH>
__device__ __forceinline__ int closing(const Args& a, int s, int i) {
  if (FLUSH) return clampi(a.pend[i], 0, a.hist);
  const int m = seen(a, s, i);
  return a.rec_done[(size_t)s * a.N + i] != 0 ? m : (m >= a.n ? 1 : 0);
}

template <bool FLUSH>
__global__ void __launch_bounds__(SCAN_BLOCK) k_nstep_scan(Args a) {
  __shared__ int wave_sum[SCAN_BLOCK / 64];
  __shared__ int carry;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, s = blockIdx.x;
  if (tid == 0) carry = 0;
  __syncthreads();
  int* before = a.scratch + a.K + (size_t)s * a.N;
  for (int base = 0; base < a.N; base += SCAN_BLOCK) {
    const int i = base + tid;
    const int cnt = i < a.N ? closing<FLUSH>(a, s, i) : 0;
    int incl = cnt;                                               // inclusive scan over the 64 robots of the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int up = __shfl_up(incl, d);
      if (lane >= d) incl += up;
    }
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    int off = carry;
    for (int w = 0; w < wave; w++) off += wave_sum[w];
    if (i < a.N) before[i] = off + incl - cnt;
    __syncthreads();
    if (tid == 0) {
      int tot = 0;
      for (int w = 0; w < SCAN_BLOCK / 64; w++) tot += wave_sum[w];
      carry += tot;
    }
    __syncthreads();
  }
  if (tid == 0) a.scratch[s] = carry;
}

// sum of tot[0 .. upto) over the wave; every lane gets it
__device__ __forceinline__ long long rows_before_step(const int* tot, int upto, int lane) {
  long long b = 0;
  for (int q = lane; q < upto; q += 64) b += tot[q];
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) b += __shfl_xor(b, d);
  return b;
}

// where step q (relative to the first fed step; negative: before it) of robot i lives: the records, or the history ring
struct Where {
  const float *obs, *act, *rew;
};
__device__ __forceinline__ Where where(const Args& a, int q, int i) {
  Where w;
  if (q >= 0) {
    const size_t r = (size_t)q * a.N + i;
    w.obs = a.rec_obs + r * a.D;
    w.act = a.rec_act + r * a.A;
    w.rew = a.rec_rew + r;
  } else {
    const int row = a.ring0 + q;                                  // (q < 0 only with n > 1, and q >= -(n - 1))
    const size_t r = (size_t)(row < 0 ? row + a.n - 1 : row) * a.N + i;
    w.obs = a.h_obs + r * a.D;
    w.act = a.h_act + r * a.A;
    w.rew = a.h_rew + r;
  }
  return w;
}

// r + gamma * R as the definition has it: the product rounded to fp32, then the sum.  __fmul_rn / __fadd_rn are plain * and +
// to the compiler, and its default contraction mode fuses them into one fma in the backend whatever a pragma says: the empty
// asm hides where the product came from (no instruction, no wait state).
__device__ __forceinline__ float mul_then_add(float r, float gamma, float R) {
  float p = __fmul_rn(gamma, R);
  asm volatile("" : "+v"(p));
  return __fadd_rn(r, p);
}

// The kernel is latency-bound (a wave moves under 1 KB), so what a wave needs first -- the robot's ep_len and done, its offsets,
// pos, and the up to n rewards of the walk back, lane j holding the reward of step c - j -- is loaded before any of it is
// used; the rows' loads follow in a second round.
template <bool FLUSH>
__global__ void __launch_bounds__(ROW_BLOCK) k_nstep_rows(Args a) {
  const int lane = threadIdx.x & 63;
  const unsigned w = blockIdx.x * ROW_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // (K * N is below 2^31)
  if (w >= (unsigned)(FLUSH ? 1 : a.K) * (unsigned)a.N) return;
  const int s = (int)(w / (unsigned)a.N), i = (int)(w - (unsigned)s * (unsigned)a.N);
  const size_t si = (size_t)s * a.N + i;
  const int c = FLUSH ? -1 : s;                                   // the closing step, relative to the first fed step
  const int reach = FLUSH ? a.hist : (int)min((long long)a.hist + s + 1, (long long)a.n);   // steps back that exist
  // round one
  const int len = FLUSH ? a.pend[i] : a.rec_len[si];
  const bool all = FLUSH || a.rec_done[si] != 0;                  // every start closes; otherwise only the one n-1 steps back
  const int before = a.scratch[a.K + si];
  const long long pos = a.pc[0];
  const float term = FLUSH ? a.tail_term[i] : a.rec_term[si];
  const float mine = lane < reach ? where(a, c - lane, i).rew[0] : 0.0f;
  const float* next = FLUSH ? a.tail_next + (size_t)i * a.D : a.rec_next + si * a.D;
  const float next0 = lane < a.D ? next[lane] : 0.0f;             // (the closing step's row: the same for every start)
  const long long earlier = FLUSH ? 0 : rows_before_step(a.scratch, s, lane);

  const int m = clampi(len, 0, reach);
  const int cnt = all ? m : (m >= a.n ? 1 : 0);                   // = closing<FLUSH>(a, s, i)
  if (cnt == 0) return;
  const int back = all ? cnt : a.n;
  // one 64-bit modulo per wave: a robot's rows (at most n, and max_size is at least that) then wrap by one subtraction
  long long first = (pos + earlier + before) % a.max_size;
  if (first < 0) first += a.max_size;                             // (a pos below zero: still a slot of the ring)
  float R = 0.0f, g = 1.0f;
  for (int j = 0; j < back; j++) {                                // start c - j, m = j + 1 steps
    const float r = __shfl(mine, j);
    R = j == 0 ? r : mul_then_add(r, a.gamma, R);
    g = j == 0 ? 1.0f : __fmul_rn(g, a.gamma);
    if (!all && j != a.n - 1) continue;
    const Where src = where(a, c - j, i);
    const long long at = first + (all ? cnt - 1 - j : 0);
    const size_t slot = (size_t)(at >= a.max_size ? at - a.max_size : at);
    for (int col0 = 0; col0 < a.D || col0 < a.A; col0 += 64) {    // every load of the pass before its first store
      const int col = col0 + lane;
      const bool in_obs = col < a.D, in_act = col < a.A;
      const float o = in_obs ? src.obs[col] : 0.0f;
      const float x = col0 == 0 ? next0 : in_obs ? next[col] : 0.0f;
      const float u = in_act ? src.act[col] : 0.0f;
      if (in_obs) {
        a.m_obs[slot * a.D + col] = o;
        a.m_next[slot * a.D + col] = x;
      }
      if (in_act) a.m_act[slot * a.A + col] = u;
    }
    if (lane == 0) {
      a.m_rew[slot] = R;
      a.m_term[slot] = __fmul_rn(term, g);
    }
  }
  if (FLUSH && lane == 0) a.pend[i] = 0;
}

__device__ __forceinline__ void advance(const Args& a, long long total, int lane) {
  if (lane == 0) {
    a.pc[0] = (a.pc[0] + total) % a.max_size;
    a.pc[1] += total;
  }
}

// job < keep: fed step K - keep + job into the history ring; job == keep: the newest step's next_obs, terminal and pending
__global__ void __launch_bounds__(ROW_BLOCK) k_nstep_tail(Args a, int keep) {
  const int lane = threadIdx.x & 63;
  const unsigned w = blockIdx.x * ROW_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (w >= (unsigned)(keep + 1) * (unsigned)a.N) return;
  const int job = (int)(w / (unsigned)a.N), i = (int)(w - (unsigned)job * (unsigned)a.N);
  if (w == 0) advance(a, rows_before_step(a.scratch, a.K, lane), lane);
  if (job < keep) {
    const int s = a.K - keep + job;
    const size_t from = (size_t)s * a.N + i, to = (size_t)((a.ring0 + s) % (a.n - 1)) * a.N + i;
    for (int col = lane; col < a.D; col += 64) a.h_obs[to * a.D + col] = a.rec_obs[from * a.D + col];
    for (int col = lane; col < a.A; col += 64) a.h_act[to * a.A + col] = a.rec_act[from * a.A + col];
    if (lane == 0) a.h_rew[to] = a.rec_rew[from];
  } else {
    const int s = a.K - 1;
    const size_t from = (size_t)s * a.N + i;
    for (int col = lane; col < a.D; col += 64) a.tail_next[(size_t)i * a.D + col] = a.rec_next[from * a.D + col];
    if (lane == 0) {
      a.tail_term[i] = a.rec_term[from];
      const long long upto = (long long)a.hist + s + 1;
      const int have = (int)min(upto, (long long)(a.n - 1));
      a.pend[i] = a.rec_done[from] != 0 ? 0 : clampi(a.rec_len[from], 0, have);
    }
  }
}

__global__ void __launch_bounds__(64) k_nstep_advance(Args a) { advance(a, a.scratch[0], threadIdx.x); }

unsigned row_blocks(long long waves) { return (unsigned)((waves + ROW_WAVES - 1) / ROW_WAVES); }

}  // namespace

using dev::fail;

extern "C" int etg_nstep_feed(int device, int num_envs, int n_steps, int n, float gamma, int hist, int64_t step0, int obs_dim,
                              int act_dim, const float* rec_obs, const float* rec_action, const float* rec_reward,
                              const uint8_t* rec_done, const float* rec_next_obs, const float* rec_terminal,
                              const int32_t* rec_ep_len, float* hist_obs, float* hist_action, float* hist_reward,
                              float* tail_next_obs, float* tail_terminal, int32_t* pending, float* mem_obs, float* mem_action,
                              float* mem_reward, float* mem_next_obs, float* mem_terminal, int64_t max_size, int64_t* pos_count,
                              int32_t* scratch, void* stream) {
  if (num_envs < 1) return fail(ETG_ERR_BAD_ARG, "etg_nstep_feed: num_envs must be at least 1");
  if (n_steps < 1) return fail(ETG_ERR_BAD_ARG, "etg_nstep_feed: n_steps must be at least 1");
  if (n < 1 || n > ETG_NSTEP_MAX_N) return fail(ETG_ERR_BAD_ARG, "etg_nstep_feed: n must be 1..16");
  if (hist < 0 || hist > n - 1) return fail(ETG_ERR_BAD_ARG, "etg_nstep_feed: hist must be 0..n-1");
  if (step0 < hist) return fail(ETG_ERR_BAD_ARG, "etg_nstep_feed: step0 must be at least hist");
  if (obs_dim < 1 || act_dim < 1) return fail(ETG_ERR_BAD_ARG, "etg_nstep_feed: obs_dim and act_dim must be at least 1");
  if (((long long)n_steps + n - 1) * num_envs > (long long)max_size)
    return fail(ETG_ERR_BAD_ARG, "etg_nstep_feed: (n_steps + n - 1) * num_envs rows must fit the memory (max_size)");
  if ((long long)num_envs * ((long long)n_steps + n) > 0x7fffffffll) return fail(ETG_ERR_BAD_ARG, "etg_nstep_feed: num_envs * (n_steps + n) must be below 2^31");
  if (!rec_obs || !rec_action || !rec_reward || !rec_done || !rec_next_obs || !rec_terminal || !rec_ep_len)
    return fail(ETG_ERR_BAD_ARG, "etg_nstep_feed: the seven record arrays must be non-null");
  if (!hist_obs || !hist_action || !hist_reward || !tail_next_obs || !tail_terminal || !pending)
    return fail(ETG_ERR_BAD_ARG, "etg_nstep_feed: the history ring, the tail and pending must be non-null");
  if (!mem_obs || !mem_action || !mem_reward || !mem_next_obs || !mem_terminal || !pos_count || !scratch)
    return fail(ETG_ERR_BAD_ARG, "etg_nstep_feed: the memory's arrays, pos_count and scratch must be non-null");
  if (device < 0) return fail(ETG_ERR_BAD_ARG, "etg_nstep_feed: device must not be negative");
  Args a{num_envs, n_steps, n, hist, obs_dim, act_dim, n > 1 ? (int)(step0 % (n - 1)) : 0, gamma, (long long)max_size, rec_obs, rec_action, rec_reward,
         rec_next_obs, rec_terminal, rec_done, (const int*)rec_ep_len, hist_obs, hist_action, hist_reward, tail_next_obs, tail_terminal,
         (int*)pending, mem_obs, mem_action, mem_reward, mem_next_obs, mem_terminal, (long long*)pos_count, (int*)scratch};
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) {
    hipStream_t s = (hipStream_t)stream;
    const int keep = n_steps < n - 1 ? n_steps : n - 1;
    hipLaunchKernelGGL(k_nstep_scan<false>, dim3((unsigned)n_steps), dim3(SCAN_BLOCK), 0, s, a);
    hipLaunchKernelGGL(k_nstep_rows<false>, dim3(row_blocks((long long)n_steps * num_envs)), dim3(ROW_BLOCK), 0, s, a);
    hipLaunchKernelGGL(k_nstep_tail, dim3(row_blocks((long long)(keep + 1) * num_envs)), dim3(ROW_BLOCK), 0, s, a, keep);
    e = hipGetLastError();
  }
  return e == hipSuccess ? ETG_OK : dev::hip_fail("etg_nstep_feed", e);
}

extern "C" int etg_nstep_flush(int device, int num_envs, int n, float gamma, int hist, int64_t step0, int obs_dim, int act_dim,
                               const float* hist_obs, const float* hist_action, const float* hist_reward, const float* tail_next_obs,
                               const float* tail_terminal, int32_t* pending, float* mem_obs, float* mem_action, float* mem_reward,
                               float* mem_next_obs, float* mem_terminal, int64_t max_size, int64_t* pos_count, int32_t* scratch,
                               void* stream) {
  if (num_envs < 1) return fail(ETG_ERR_BAD_ARG, "etg_nstep_flush: num_envs must be at least 1");
  if (n < 1 || n > ETG_NSTEP_MAX_N) return fail(ETG_ERR_BAD_ARG, "etg_nstep_flush: n must be 1..16");
  if (hist < 0 || hist > n - 1) return fail(ETG_ERR_BAD_ARG, "etg_nstep_flush: hist must be 0..n-1");
  if (step0 < hist) return fail(ETG_ERR_BAD_ARG, "etg_nstep_flush: step0 must be at least hist");
  if (obs_dim < 1 || act_dim < 1) return fail(ETG_ERR_BAD_ARG, "etg_nstep_flush: obs_dim and act_dim must be at least 1");
  if ((long long)(n - 1) * num_envs > (long long)max_size) return fail(ETG_ERR_BAD_ARG, "etg_nstep_flush: (n - 1) * num_envs rows must fit the memory (max_size)");
  if (max_size < 1) return fail(ETG_ERR_BAD_ARG, "etg_nstep_flush: max_size must be at least 1");
  if ((long long)num_envs * n > 0x7fffffffll) return fail(ETG_ERR_BAD_ARG, "etg_nstep_flush: num_envs * n must be below 2^31");
  if (!hist_obs || !hist_action || !hist_reward || !tail_next_obs || !tail_terminal || !pending)
    return fail(ETG_ERR_BAD_ARG, "etg_nstep_flush: the history ring, the tail and pending must be non-null");
  if (!mem_obs || !mem_action || !mem_reward || !mem_next_obs || !mem_terminal || !pos_count || !scratch)
    return fail(ETG_ERR_BAD_ARG, "etg_nstep_flush: the memory's arrays, pos_count and scratch must be non-null");
  if (device < 0) return fail(ETG_ERR_BAD_ARG, "etg_nstep_flush: device must not be negative");
  Args a{num_envs, 1, n, hist, obs_dim, act_dim, n > 1 ? (int)(step0 % (n - 1)) : 0, gamma, (long long)max_size, nullptr, nullptr, nullptr, nullptr, nullptr,
         nullptr, nullptr, (float*)hist_obs, (float*)hist_action, (float*)hist_reward, (float*)tail_next_obs, (float*)tail_terminal,
         (int*)pending, mem_obs, mem_action, mem_reward, mem_next_obs, mem_terminal, (long long*)pos_count, (int*)scratch};
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) {
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_nstep_scan<true>, dim3(1), dim3(SCAN_BLOCK), 0, s, a);
    hipLaunchKernelGGL(k_nstep_rows<true>, dim3(row_blocks(num_envs)), dim3(ROW_BLOCK), 0, s, a);
    hipLaunchKernelGGL(k_nstep_advance, dim3(1), dim3(64), 0, s, a);
    e = hipGetLastError();
  }
  return e == hipSuccess ? ETG_OK : dev::hip_fail("etg_nstep_flush", e);
}
