// etg_monitor.hip -- the episode monitor (include/etgsim_monitor.h): per-episode sums of the reward terms, the success counter
// and the ring of finished episodes, reduced on the device from the recorded reward / done / info rows of K control steps.
//
// The reference sums `info` per episode on the host (train.py:150-157,175).  The continuous collection paths have no episode
// boundary on the host, so a feed walks the K recorded steps of every robot and files a record where `done` is set.  Two
// launches, no atomics:
//
//   k_monitor_scan   one workgroup per step: per group of 64 robots the 64 finishing bits (one ballot over the done bytes) and
//                    the number of finished robots before the group in this step, and the step's total
//   k_monitor_feed   4 robots per wave, lane = field of the robot's 16-float row (the 16-lane row of the tick kernels): every
//                    lane walks the K steps of its robot with plain fp32 adds in step order.  A finished row's record number
//                    is count + (finished in earlier steps) + (finished before the group) + (finishing bits below the robot):
//                    step ascending, then robot ascending, whatever order the waves run in.
//
// The loop of k_monitor_feed is latency-bound (one 4-byte load per lane and step, 256 B apart from step to step), so the loads
// of PRE steps are issued before the first of them is used.  The count the record numbers start from is the copy the scan
// left in scratch: the feed kernel's first wave writes the new count while other waves may still be starting.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/etgsim_monitor.h"
#include "dev_buffers.h"

namespace {

constexpr int SCAN_BLOCK = 1024, FEED_BLOCK = 256, PRE = 8;

__device__ __forceinline__ int groups_of(int n) { return (n + 63) >> 6; }

// scratch: [0..1] count before the feed, [2 + s] finished robots of step s, then per (s, group g) {finished before g in s, bits lo, bits hi}
__global__ void __launch_bounds__(SCAN_BLOCK) k_monitor_scan(const uint8_t* __restrict__ done, int n, int n_steps,
                                                             const long long* __restrict__ count, int* __restrict__ scratch) {
  __shared__ int wave_sum[SCAN_BLOCK / 64];
  __shared__ int carry;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, s = blockIdx.x, ng = groups_of(n);
  if (tid == 0) {
    carry = 0;
    if (s == 0) {
      const long long c = count[0];
      scratch[0] = (int)(unsigned)(c & 0xffffffffll);
      scratch[1] = (int)(c >> 32);
    }
  }
  __syncthreads();
  int* grp = scratch + 2 + n_steps + (size_t)s * ng * 3;
  for (int base = 0; base < n; base += SCAN_BLOCK) {
    const int i = base + tid;
    const int d = (i < n) && done[(size_t)s * n + i] != 0;
    const unsigned long long bal = __ballot(d);
    if (lane == 0) wave_sum[wave] = __popcll(bal);
    __syncthreads();
    int off = carry;
    for (int w = 0; w < wave; w++) off += wave_sum[w];
    const int g = (base >> 6) + wave;
    if (lane == 0 && g < ng) {
      grp[g * 3 + 0] = off;
      grp[g * 3 + 1] = (int)(unsigned)(bal & 0xffffffffull);
      grp[g * 3 + 2] = (int)(unsigned)(bal >> 32);
    }
    __syncthreads();
    if (tid == 0) {
      int tot = 0;
      for (int w = 0; w < SCAN_BLOCK / 64; w++) tot += wave_sum[w];
      carry += tot;
    }
    __syncthreads();
  }
  if (tid == 0) scratch[2 + s] = carry;
}

// what a lane does with the value it loads: its field of the row
enum { F_ADD = 0, F_ONE = 1, F_COUNT = 2, F_SET = 3, F_ZERO = 4 };

__global__ void __launch_bounds__(FEED_BLOCK) k_monitor_feed(int n, int n_steps, long long step0, float success_velx,
                                                             const float* __restrict__ reward, const float* __restrict__ info,
                                                             float* __restrict__ running, float* __restrict__ records,
                                                             int* __restrict__ meta, long long capacity, long long* __restrict__ count,
                                                             const int* __restrict__ scratch) {
  const int gid = blockIdx.x * FEED_BLOCK + threadIdx.x;
  const int i = gid >> 4, f = gid & 15;
  if (i >= n) return;
  const int ng = groups_of(n), g = i >> 6, bit = i & 63;
  const long long before = (long long)(unsigned)scratch[0] | ((long long)scratch[1] << 32);
  const int* tot = scratch + 2;
  const int* grp = scratch + 2 + n_steps + (size_t)g * 3;
  long long total = 0;                       // finished in this feed: only the newest `capacity` records are written
  for (int s = 0; s < n_steps; s++) total += tot[s];
  if (gid == 0) count[0] = before + total;
  const long long first_kept = before + total - capacity;

  // the lane's source: reward, or a column of the info row; the fields without one load the reward and ignore it
  int kind, col = -1;
  if (f == ETG_MON_RET) kind = F_ADD;
  else if (f == ETG_MON_LEN) kind = F_ONE;
  else if (f < ETG_MON_SUCCESS) { kind = F_ADD; col = ETG_INFO_TORSO + (f - ETG_MON_TERMS); }
  else if (f == ETG_MON_SUCCESS) { kind = F_COUNT; col = ETG_INFO_VELX; }
  else if (f == ETG_MON_ENERGY) { kind = F_ADD; col = ETG_INFO_ENERGY; }
  else if (f == ETG_MON_SWEEPS) { kind = F_ADD; col = ETG_INFO_SWEEPS; }
  else if (f == ETG_MON_X_END) { kind = F_SET; col = ETG_INFO_BASE; }
  else kind = F_ZERO;
  const float* src = col < 0 ? reward + i : info + (size_t)i * ETG_INFO_DIM + col;
  const size_t stride = col < 0 ? (size_t)n : (size_t)n * ETG_INFO_DIM;

  float acc = running[(size_t)i * ETG_MON_DIM + f];
  long long earlier = 0;                     // finished in the steps before s
  for (int s0 = 0; s0 < n_steps; s0 += PRE) {
    float v[PRE];
    int pre[PRE], lo[PRE], hi[PRE], ts[PRE];
#pragma unroll
    for (int u = 0; u < PRE; u++) {          // the loads of PRE steps in flight together (a step past the end repeats the last one)
      const int s = min(s0 + u, n_steps - 1);
      v[u] = src[(size_t)s * stride];
      const int* e = grp + (size_t)s * ng * 3;
      pre[u] = e[0];
      lo[u] = e[1];
      hi[u] = e[2];
      ts[u] = tot[s];
    }
#pragma unroll
    for (int u = 0; u < PRE; u++) {
      const int s = s0 + u;
      if (s < n_steps) {
        const float add = kind == F_ADD ? v[u] : kind == F_ONE ? 1.0f : (kind == F_COUNT && v[u] >= success_velx) ? 1.0f : 0.0f;
        acc = kind == F_SET ? v[u] : kind == F_ZERO ? 0.0f : acc + add;
        const unsigned long long bits = (unsigned long long)(unsigned)lo[u] | ((unsigned long long)(unsigned)hi[u] << 32);
        if ((bits >> bit) & 1ull) {
          const long long j = before + earlier + pre[u] + __popcll(bits & ((1ull << bit) - 1ull));
          if (j >= first_kept) {
            const size_t row = (size_t)(j % capacity);
            records[row * ETG_MON_DIM + f] = acc;
            if (f == 0) {
              meta[row * 2 + 0] = i;
              meta[row * 2 + 1] = (int)((step0 + s) & 0x7fffffffll);
            }
          }
          acc = 0.0f;
        }
        earlier += ts[u];
      }
    }
  }
  running[(size_t)i * ETG_MON_DIM + f] = acc;
}

}  // namespace

using dev::fail;

extern "C" int etg_monitor_feed(int device, int num_envs, int n_steps, int64_t step0, float success_velx, const float* reward,
                                const uint8_t* done, const float* info, float* running, float* records, int32_t* meta, int capacity,
                                int64_t* count, int32_t* scratch, void* stream) {
  if (num_envs < 1) return fail(ETG_ERR_BAD_ARG, "etg_monitor_feed: num_envs must be at least 1");
  if (n_steps < 1) return fail(ETG_ERR_BAD_ARG, "etg_monitor_feed: n_steps must be at least 1");
  if (capacity < 1) return fail(ETG_ERR_BAD_ARG, "etg_monitor_feed: capacity must be at least 1");
  if ((long long)num_envs * n_steps > 0x7fffffffll) return fail(ETG_ERR_BAD_ARG, "etg_monitor_feed: num_envs * n_steps must be below 2^31");
  if (!reward || !done || !info) return fail(ETG_ERR_BAD_ARG, "etg_monitor_feed: reward, done and info must be non-null");
  if (!running || !records || !meta) return fail(ETG_ERR_BAD_ARG, "etg_monitor_feed: running, records and meta must be non-null");
  if (!count || !scratch) return fail(ETG_ERR_BAD_ARG, "etg_monitor_feed: count and scratch must be non-null");
  if (device < 0) return fail(ETG_ERR_BAD_ARG, "etg_monitor_feed: device must not be negative");
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) {
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_monitor_scan, dim3((unsigned)n_steps), dim3(SCAN_BLOCK), 0, s, done, num_envs, n_steps, (const long long*)count,
                       (int*)scratch);
    const long long lanes = (long long)num_envs * ETG_MON_DIM;
    hipLaunchKernelGGL(k_monitor_feed, dim3((unsigned)((lanes + FEED_BLOCK - 1) / FEED_BLOCK)), dim3(FEED_BLOCK), 0, s, num_envs, n_steps,
                       (long long)step0, success_velx, reward, info, running, records, (int*)meta, (long long)capacity, (long long*)count,
                       (const int*)scratch);
    e = hipGetLastError();
  }
  return e == hipSuccess ? ETG_OK : dev::hip_fail("etg_monitor_feed", e);
}
