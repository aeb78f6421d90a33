/* etgsim_scan_policy.h -- the closed-loop launches of etgsim_step_policy.h and etgsim_collect.h for an actor that sees the
 * terrain height scan (etgsim_heightscan.h): the launch computes the scan columns itself.
 *
 * An actor on stairs reads its observation columns and then the P scan columns of the same state.  Stepping gets them from a
 * live-scan launch after every step (and a scan of given poses for the rows before a restart); here the wave that steps 4
 * robots evaluates their 4 x P points -- one lane each -- from the state it holds: before the first step from the handle's live
 * state, after every control step from the pose that step produced, and once more for a robot that restarts.  Every scan value
 * is bit for bit what the live scan of etgsim_heightscan.h returns for the same state.  The same library as etgsim.h (its ABI
 * version, 2, is unchanged); this header declares the two entry points that are not part of it.
 *
 * etg_step_policy_scan takes the arguments of etg_step_policy, etg_collect_policy_scan those of etg_collect_policy_info, with
 * these additions and changes:
 *   points [P,2], n_points, offset, clip   the scan's grid and clamp, as the live scan takes them.  1 <= P <= 16.
 *   the actor            reads the in_dim - P observation columns [obs_col0, obs_col0 + in_dim - P) and then the P scan columns.
 *   obs [N,49]           the in/out buffer it is in the scan-less calls: it holds no scan columns.
 *   scan [N,P]           out: the scan columns of the rows the next step acts on (of a restarted robot: of its reset state).
 *                        The scan columns of the rows THIS call's first step acts on are computed from the handle's state.
 *   act_obs, terminal_obs [N,49+P]         (etg_step_policy_scan) wide rows: the 49 observation columns, then the scan of
 *                        the state the row belongs to.  Both are required.
 *   rec_obs, rec_next_obs [K,N,49+P]       (etg_collect_policy_scan) wide rows, likewise.
 *   rec_info [K,N,64]    may be NULL.
 * Everything else -- the other arrays, what a step computes, restarts, the sensor-noise stream's advance -- is as in the
 * scan-less call, bit for bit.  Every refusal of the scan-less call holds, comes before any launch and leaves the handle as it
 * was, with the reason in etg_last_error() after the function's name.  The scan adds: ETG_ERR_BAD_ARG for a null points, scan
 * or wide row array, n_points outside 1..16, in_dim - n_points < 1, in_dim > 64 and clip < 0; ETG_ERR_STATE on a heightfield
 * terrain before etg_set_heightfield.                                                                                      */
#ifndef ETGSIM_SCAN_POLICY_H_
#define ETGSIM_SCAN_POLICY_H_

#include "etgsim.h"

#ifdef __cplusplus
extern "C" {
#endif

int etg_step_policy_scan(EtgHandle* h, EtgPolicy* policy, float act_scale, int precision, int obs_col0, int auto_reset,
                         const float* noise, const uint8_t* donef, float* obs, float* act, float* act_obs, float* terminal_obs,
                         float* reward, uint8_t* done, float* info, const float* points, int n_points, float offset, float clip,
                         float* scan, void* stream);

int etg_collect_policy_scan(EtgHandle* h, EtgPolicy* policy, float act_scale, int precision, int obs_col0, int n_steps,
                            int bootstrap_from, const float* noise, const uint8_t* donef, float* obs, float* rec_obs,
                            float* rec_action, float* rec_reward, uint8_t* rec_done, float* rec_next_obs, float* rec_terminal,
                            float* rec_ep_ret, int32_t* rec_ep_len, float* rec_info, const float* points, int n_points,
                            float offset, float clip, float* scan, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ETGSIM_SCAN_POLICY_H_ */
