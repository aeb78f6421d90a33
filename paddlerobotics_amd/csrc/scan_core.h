// scan_core.h -- the terrain height scan behind etg_scan_pose / etg_height_scan / etg_height_scan_at
// (include/etgsim_heightscan.h): the height of a robot's base above the terrain at points of a yaw-aligned grid around it.
//
// Everything here is ETG_HD, so the same source runs in the gfx950 kernels (etg_heightscan.hip) and, compiled for the host, in
// the test-only shim (tests/scan_emu).  Per row:
//   state_pose    x, y, z and yaw of a robot from the base state columns
//   make_row      a pose row [x, y, z, yaw] with its robot: the cos / sin pair, once per row
//   scan_point    one point (a forward, b left) of the row: the query position, the terrain height there as the robot's contacts
//                 see it (heightfield_query of etg_layout.h, called as it is; 0 on flat ground) and the clamped clearance
// fp32 throughout.  The multiply-adds of the yaw and of the point transform are written as fmaf, so that every caller -- the pose
// kernel, the live scan, the scan of given poses, the host build -- rounds them the same way whatever the compiler would contract.
#pragma once

#include "etg_layout.h"

namespace etg {
namespace scan {

constexpr int kMaxPoints = 64;   // ETG_HEIGHT_SCAN_MAX_POINTS (include/etgsim_heightscan.h)

struct Row {
  float x, y, z, c, s;   // base position (world), cos / sin of the yaw
  int env;               // the robot whose terrain band is read; < 0: no such robot, the row is NaN
};

// yaw = atan2(2 (w qz + qx qy), 1 - 2 (qy^2 + qz^2)) of the base quaternion
ETG_HD float yaw_of_quat(float qx, float qy, float qz, float qw) {
  const float sy = 2.0f * fmaf(qw, qz, qx * qy);
  const float cy = fmaf(-2.0f, fmaf(qy, qy, qz * qz), 1.0f);
  return atan2f(sy, cy);
}

// x, y, z, yaw of robot `env` from the base columns [BS_N][n_env] (both lane mappings keep this layout)
ETG_HD void state_pose(const float* base, int n_env, int env, float* pose) {
  const size_t N = (size_t)n_env;
  pose[0] = base[(size_t)BS_PX * N + env];
  pose[1] = base[(size_t)BS_PY * N + env];
  pose[2] = base[(size_t)BS_PZ * N + env];
  pose[3] = yaw_of_quat(base[(size_t)BS_QX * N + env], base[(size_t)BS_QY * N + env], base[(size_t)BS_QZ * N + env],
                        base[(size_t)BS_QW * N + env]);
}

ETG_HD Row make_row(const float* pose, int env) {
  Row r;
  r.x = pose[0]; r.y = pose[1]; r.z = pose[2];
  r.c = cosf(pose[3]); r.s = sinf(pose[3]);
  r.env = env;
  return r;
}

// the row of a robot whose seven base values the caller holds (the closed-loop kernels with SCAN, etg_kernels.hip: the state is
// in registers there, before it is stored): state_pose's arithmetic on them, then make_row
ETG_HD Row row_of_base(float px, float py, float pz, float qx, float qy, float qz, float qw, int env) {
  const float pose[4] = {px, py, pz, yaw_of_quat(qx, qy, qz, qw)};
  return make_row(pose, env);
}

ETG_HD float quiet_nan() {   // (a bit pattern: the library is built with -ffinite-math-only)
  const unsigned u = 0x7fc00000u;
  float f;
  __builtin_memcpy(&f, &u, 4);
  return f;
}

// out[e, j] = clamp(z - H(X, Y) - offset, -clip, +clip),  X = x + cos a - sin b,  Y = y + sin a + cos b
ETG_HD float scan_point(const KCfg& K, const Row& r, float a, float b, float offset, float clip) {
  if (r.env < 0) return quiet_nan();
  const float X = fmaf(-r.s, b, fmaf(r.c, a, r.x));
  const float Y = fmaf(r.c, b, fmaf(r.s, a, r.y));
  float H = 0.0f, nx, ny, nz;
  if (K.terrain != 0) heightfield_query(K, r.env, X, Y, H, nx, ny, nz);
  return fminf(fmaxf(r.z - H - offset, -clip), clip);
}

// the robot of row i: env_ids[i], or i % n_env without ids; -1 when the id names no robot
ETG_HD int row_env(const int32_t* env_ids, int i, int n_env) {
  const int e = env_ids ? env_ids[i] : i % n_env;
  return (e >= 0 && e < n_env) ? e : -1;
}

}  // namespace scan
}  // namespace etg

// the kernels' launchers (etg_heightscan.hip); arguments as in include/etgsim_heightscan.h, already checked by the caller.
// etg_height_scan_launch: pose == nullptr is the live scan (rows = the n_env robots, read from `base`).
#if defined(__HIPCC__)
hipError_t etg_scan_pose_launch(const float* base, int n_env, float* pose, hipStream_t stream);
hipError_t etg_height_scan_launch(const etg::KCfg& K, const float* base, const float* pose, const int32_t* env_ids, int rows,
                                  const float* points, int n_points, float offset, float clip, float* out, hipStream_t stream);
#endif
