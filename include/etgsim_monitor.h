/* etgsim_monitor.h -- per-episode reward terms and success rate of the continuous collection paths, on the device.
 *
 * Every episode loop of the reference returns, next to the episode's return and length, `infos`: the per-episode sums of the
 * reward terms of Param_Dict and success_rate, the share of steps with info["velx"] >= 0.3 (train.py:150-157,175), and its
 * driver logs them after every episode (train.py:363-366).  The continuous collection paths (etg_step_autoreset,
 * etg_step_policy, etg_collect_policy) have no episode boundary on the host, so the reduction lives on the device: the info
 * rows of the steps are recorded, and etg_monitor_feed sums them per robot and files a record whenever an episode ends.
 * The same library as etgsim.h (its ABI version, 2, is unchanged); this header declares the two entry points of the monitor.
 *
 * etg_collect_policy_info: etg_collect_policy (include/etgsim_collect.h: the same refusals, stream advance and launch) that
 * also records the steps' info rows: rec_info [K,N,ETG_INFO_DIM], required (NULL: ETG_ERR_BAD_ARG).  rec_info[s] is the info
 * row of step s of every robot; for a robot that restarts it is the finished step's row, as in etg_step_autoreset.
 *
 * etg_monitor_feed is stateless, as etg_replay_begin / etg_replay_end: the caller owns every array.
 *   device               the HIP device the arrays live on.
 *   num_envs, n_steps    N >= 1 robots, K >= 1 steps.
 *   step0                the number of the first fed step (for meta).
 *   success_velx         a step counts as a success when info[ETG_INFO_VELX] >= success_velx (train.py:156: 0.3).
 *   reward [K,N], done [K,N] (bytes), info [K,N,ETG_INFO_DIM]    what the steps wrote.
 *   running [N,ETG_MON_DIM]   in/out: the row of every robot's running episode (zero at the start).
 *   records [C,ETG_MON_DIM], meta [C,2] (int32)   the ring of finished episodes and their (robot, step number mod 2^31).
 *   capacity             C >= 1 rows of the ring.
 *   count                in/out, one int64 on the device: episodes ever finished.
 *   scratch              ETG_MON_SCRATCH_INTS(num_envs, n_steps) int32 on the device; its content before and after is of no
 *                        interest.
 *   stream               hipStream_t, or NULL.
 * For s = 0..K-1 in order and every robot i: step s is added to running[i] (the columns below); if done[s][i], the row is a
 * finished episode with record number j = count + (the number of finished (s', i') before (s, i), step-major); it is written to
 * records[j % C], meta[j % C] = (i, (step0 + s) mod 2^31), and running[i] is zeroed.  At the end count += the number of
 * episodes finished in this feed.  Where more than C episodes finish in one feed, only the newest C are written.
 *
 * The record order is step ascending, then robot ascending, found by counting per step and scanning: there are no
 * floating-point atomics and no atomic cursor, so a feed is deterministic.  The sums are plain fp32 adds in step order per
 * robot: feeding K steps in one call leaves bit for bit what K calls of one step leave.  Two launches per feed, no host
 * synchronisation.  An episode already running when the first feed comes is recorded from that feed on.
 *
 * Argument checks come before any HIP call: a null pointer, n_steps < 1, num_envs < 1, capacity < 1 or num_envs * n_steps
 * >= 2^31 gives ETG_ERR_BAD_ARG with the function's name in etg_last_error().                                           */
#ifndef ETGSIM_MONITOR_H_
#define ETGSIM_MONITOR_H_

#include "etgsim.h"

#define ETG_MON_DIM 16         /* floats per running / record row                                              */
#define ETG_MON_RET 0          /* sum of reward                                                                */
#define ETG_MON_LEN 1          /* steps                                                                        */
#define ETG_MON_TERMS 2        /* 7: sums of the info columns ETG_INFO_TORSO .. ETG_INFO_FOOTCONTACT           */
#define ETG_MON_SUCCESS 9      /* steps with info[ETG_INFO_VELX] >= success_velx                               */
#define ETG_MON_ENERGY 10      /* sum of info[ETG_INFO_ENERGY]                                                 */
#define ETG_MON_SWEEPS 11      /* sum of info[ETG_INFO_SWEEPS]                                                 */
#define ETG_MON_X_END 12       /* info[ETG_INFO_BASE] (the base's world x) of the newest fed step              */
                               /* 13..15: zero                                                                 */
/* int32 elements of `scratch`: the count before the feed (2), per step the number of finished robots (1) and per step and
 * group of 64 robots the number of finished robots before the group in the step and the group's 64 finishing bits (3)   */
#define ETG_MON_SCRATCH_INTS(num_envs, n_steps) (2 + (n_steps) * (1 + 3 * (((num_envs) + 63) / 64)))

#ifdef __cplusplus
extern "C" {
#endif

int etg_collect_policy_info(EtgHandle* h, EtgPolicy* policy, float act_scale, int precision, int obs_col0, int n_steps,
                            int bootstrap_from, const float* noise, const uint8_t* donef, float* obs, float* rec_obs,
                            float* rec_action, float* rec_reward, uint8_t* rec_done, float* rec_next_obs, float* rec_terminal,
                            float* rec_ep_ret, int32_t* rec_ep_len, float* rec_info, void* stream);

int etg_monitor_feed(int device, int num_envs, int n_steps, int64_t step0, float success_velx, const float* reward,
                     const uint8_t* done, const float* info, float* running, float* records, int32_t* meta, int capacity,
                     int64_t* count, int32_t* scratch, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ETGSIM_MONITOR_H_ */
