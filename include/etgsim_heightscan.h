/* etgsim_heightscan.h -- a terrain height scan: the clearance of a robot's base above the ground at the points of a grid that
 * turns with the robot's heading.
 *
 * Every task of this simulator is a terrain task, and nothing in the 49-float row or the extra sensors says where the terrain
 * is.  The reference has no such sensor (its robots are blind; rlschool's terrain code is absent), so the definition below is
 * this project's own.  The same library as etgsim.h (its ABI version, 2, is unchanged); this header
 * declares the three entry points of the sensor.
 *
 * The definition.  Robot e has the base position (x, y, z) (world) and the yaw psi.  Scan point j has the coordinates
 * (a_j, b_j) in the yaw-aligned frame, metres: a forward, b to the left.
 *   X = x + cos psi * a_j - sin psi * b_j
 *   Y = y + sin psi * a_j + cos psi * b_j
 *   H = the terrain height at (X, Y) as robot e's contacts see it: the contact code's own bilinear heightfield query, i.e. band
 *       e % hf_bands of the heights, the query clamped at the field's border, (X - hf_x0) * (1 / hf_cell) as the cell
 *       coordinate; H = 0 with EtgConfig.terrain == 0
 *   out[e, j] = clamp(z - H - offset, -clip, +clip)
 * psi = atan2(2 (w qz + qx qy), 1 - 2 (qy^2 + qz^2)) of the base quaternion (roll and pitch do not enter: the grid stays
 * horizontal).  fp32 throughout.  The columns carry no sensor noise and no latency: they are read from the true state at the
 * moment of the call.
 *
 * Arguments (device pointers):
 *   h                    the simulator.
 *   pose [M,4]           rows x, y, z, psi (etg_scan_pose: M = N, written; etg_height_scan_at: read).
 *   env_ids [M] (int32)  the robot of every pose row, whose terrain band is read; or NULL: row i belongs to robot i % N, so a
 *                        flattened record [K,N,4] of K steps works as it is.  A row whose id is outside 0 .. N-1 reads nothing
 *                        and is written as NaN (all P columns); the other rows are not affected.
 *   M                    the number of rows, >= 1, with M * P < 2^31 - 256.
 *   points [P,2]         the pairs (a_j, b_j).
 *   P                    1 .. ETG_HEIGHT_SCAN_MAX_POINTS.
 *   offset, clip         the height at which a column reads 0 (the nominal standing height) and the clamp, clip >= 0; finite.
 *   out [M,P]            the scan, the point index minor.
 *   stream               hipStream_t, or NULL.
 *
 * etg_scan_pose       writes x, y, z, psi of the live state of every robot.  One launch.
 * etg_height_scan_at  the definition for the caller's pose rows.  One launch.
 * etg_height_scan     the live scan, out [N,P]: by construction etg_scan_pose followed by etg_height_scan_at on its rows with
 *                     env_ids = NULL, bit for bit -- one launch that takes each row's pose from the state through the pose
 *                     kernel's own function and then runs the same per-point function.
 * No host synchronisation, no atomics: the calls are deterministic.
 *
 * Refusals come before any launch: a null handle, a null pose / points / out, M < 1, P outside 1 .. 64, M * P too large and a
 * negative clip give ETG_ERR_BAD_ARG (offset and clip are taken as finite); etg_scan_pose and etg_height_scan before the
 * first etg_reset (there is no state yet), and any of the three on a heightfield configuration before etg_set_heightfield,
 * give ETG_ERR_STATE.  The function's name comes first in etg_last_error().                                                  */
#ifndef ETGSIM_HEIGHTSCAN_H_
#define ETGSIM_HEIGHTSCAN_H_

#include "etgsim.h"

#define ETG_HEIGHT_SCAN_MAX_POINTS 64
#define ETG_SCAN_POSE_DIM 4            /* x, y, z, yaw */

#ifdef __cplusplus
extern "C" {
#endif

int etg_scan_pose(EtgHandle* h, float* pose, void* stream);

int etg_height_scan_at(EtgHandle* h, const float* pose, const int32_t* env_ids, int M, const float* points, int P, float offset,
                       float clip, float* out, void* stream);

int etg_height_scan(EtgHandle* h, const float* points, int P, float offset, float clip, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ETGSIM_HEIGHTSCAN_H_ */
