// etg_heightscan.hip -- gfx950 kernels of etg_scan_pose / etg_height_scan / etg_height_scan_at (include/etgsim_heightscan.h).
//
// Mapping of k_height_scan: one lane per (row, point) with the point index minor, so a workgroup of 256 lanes writes 256
// consecutive floats of `out` and a wave's loads of the heightfield fall into the few cells around one or two robots.  A
// workgroup first stages what its lanes share in LDS: the points (at most 64 pairs) and, once per row it touches (at most
// 256: P = 1), the row's pose with the cos / sin pair of its yaw (scan_core.h: make_row) -- from the caller's pose rows, or for
// the live scan straight from the base state columns through the function the pose kernel uses (state_pose).  Every lane then
// reads its row and its point from there and evaluates scan_core.h: scan_point.  No atomics, no scratch.
#include <hip/hip_runtime.h>

#include "scan_core.h"

namespace etg {
namespace scan {

constexpr int kBlock = 256;

__global__ void __launch_bounds__(kBlock) k_scan_pose(const float* base, int n_env, float* pose) {
  const int e = blockIdx.x * kBlock + threadIdx.x;
  if (e >= n_env) return;
  float p[4];
  state_pose(base, n_env, e, p);
  for (int k = 0; k < 4; k++) pose[(size_t)e * 4 + k] = p[k];
}

template <bool LIVE>
__global__ void __launch_bounds__(kBlock) k_height_scan(KCfg K, const float* base, const float* pose, const int32_t* env_ids, int rows,
                                                        const float* points, int P, float offset, float clip, float* out) {
  __shared__ Row row_s[kBlock];
  __shared__ float pts_s[2 * kMaxPoints];
  const int total = rows * P;                          // (the caller has checked that it fits)
  const int i0 = blockIdx.x * kBlock;
  const int last = min(i0 + kBlock, total) - 1;        // i0 < total: the grid is ceil(total / kBlock)
  const int r0 = i0 / P, nrows = last / P - r0 + 1;    // <= kBlock rows
  const int t = threadIdx.x;
  if (t < 2 * P) pts_s[t] = points[t];
  if (t < nrows) {
    const int r = r0 + t;
    const int env = LIVE ? r : row_env(env_ids, r, K.n_env);
    float p[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (env >= 0) {                                    // a row without a robot reads nothing
      if (LIVE) state_pose(base, K.n_env, env, p);
      else
        for (int k = 0; k < 4; k++) p[k] = pose[(size_t)r * 4 + k];
    }
    row_s[t] = make_row(p, env);
  }
  __syncthreads();
  const int i = i0 + t;
  if (i >= total) return;
  const int r = i / P, j = i - r * P;
  out[i] = scan_point(K, row_s[r - r0], pts_s[2 * j], pts_s[2 * j + 1], offset, clip);
}

}  // namespace scan
}  // namespace etg

hipError_t etg_scan_pose_launch(const float* base, int n_env, float* pose, hipStream_t stream) {
  using namespace etg::scan;
  hipLaunchKernelGGL(k_scan_pose, dim3((unsigned)((n_env + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, base, n_env, pose);
  return hipGetLastError();
}

hipError_t etg_height_scan_launch(const etg::KCfg& K, const float* base, const float* pose, const int32_t* env_ids, int rows,
                                  const float* points, int n_points, float offset, float clip, float* out, hipStream_t stream) {
  using namespace etg::scan;
  const unsigned grid = (unsigned)(((long long)rows * n_points + kBlock - 1) / kBlock);
  if (pose)
    hipLaunchKernelGGL(k_height_scan<false>, dim3(grid), dim3(kBlock), 0, stream, K, base, pose, env_ids, rows, points, n_points,
                       offset, clip, out);
  else
    hipLaunchKernelGGL(k_height_scan<true>, dim3(grid), dim3(kBlock), 0, stream, K, base, pose, env_ids, rows, points, n_points,
                       offset, clip, out);
  return hipGetLastError();
}
