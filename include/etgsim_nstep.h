/* etgsim_nstep.h -- multi-step (n-step) rows for the replay memory, built on the device from the recorded control steps.
 *
 * The reference does one learner update per transition of its one robot (train.py:159-165).  With thousands of robots a run
 * does a few updates per thousands of new transitions, and every update has to carry reward further back than one control
 * step: the memory then stores, per start step, the discounted sum of the next n rewards and the observation n steps later.
 * The learners need no change: k_td (csrc/sac_core.h) and sac.py form the target as reward + gamma * terminal * (...), so a
 * row that stores terminal * gamma^(m-1) next to the m-step reward sum gives the m-step target.
 * The same library as etgsim.h (its ABI version, 2, is unchanged); this header declares the two entry points of the writer.
 *
 * The definition.  Per robot the fed stream is one transition per control step, (obs_t, action_t, reward_t, next_obs_t,
 * done_t, terminal_t, ep_len_t): the records of etg_collect_policy (include/etgsim_collect.h); terminal is the bootstrap
 * flag, ep_len the 1-based episode step.  t counts the steps fed since the writer was attached or last flushed, and
 * avail(t) = min(ep_len_t, t + 1) is the number of steps of the robot's running episode the writer has seen up to t.
 * For 1 <= n <= 16 the rows that close at step c of a robot are
 *   done_c:      min(n, avail(c)) rows, with the starts c - min(n, avail(c)) + 1 .. c, oldest first;
 *   otherwise:   one row with start c - n + 1 when avail(c) >= n, else none.
 * A row with start t, close c and m = c - t + 1 steps holds
 *   obs = obs_t, action = action_t, next_obs = next_obs_c,
 *   reward = R:    R = reward_c, then for k = c-1 .. t: R = reward_k + gamma * R (one fp32 multiply, then one fp32 add, never
 *                  contracted into an fma),
 *   terminal = terminal_c * g:   g = 1, then g = g * gamma in fp32, m - 1 times.
 * With n = 1 this is the 1-step row, bit for bit.  The rows of a feed are ordered by closing step ascending, then robot
 * ascending, then start ascending; row j goes to slot (pos + j) % max_size, and pos_count = {pos, rows ever appended} (the
 * memory's two int64) advances on the device.  There are no atomics: the offsets come from counting and scanning, so a feed
 * is deterministic, and feeding K steps in one call leaves bit for bit what K calls of one step leave.
 *
 * The entry points are stateless, as etg_monitor_feed: the caller owns every array (device pointers).
 *   device               the HIP device the arrays live on.
 *   num_envs             N >= 1 robots.
 *   n_steps              K >= 1 fed steps (etg_nstep_feed).
 *   n, gamma             1 <= n <= 16 and the fp32 discount.
 *   hist                 the number of valid steps in the history ring, 0 .. n-1: min(t, n - 1) for a feed that starts at t.
 *   step0                the number t of the first fed step (etg_nstep_flush: of the step that would be fed next);
 *                        step0 >= hist.
 *   obs_dim, act_dim     D >= 1, A >= 1 columns.
 *   rec_obs [K,N,D], rec_action [K,N,A], rec_reward [K,N], rec_done [K,N] (bytes), rec_next_obs [K,N,D], rec_terminal [K,N],
 *   rec_ep_len [K,N] (int32)     the fed steps.
 *   hist_obs [n-1,N,D], hist_action [n-1,N,A], hist_reward [n-1,N]   in/out: the last n-1 fed steps, step number g in row
 *                        g % (n-1) (a ring, never shifted: K < n-1 steps then leave what single steps leave).  With n = 1 the
 *                        three are not touched, but must not be NULL.
 *   tail_next_obs [N,D], tail_terminal [N]   in/out: next_obs and terminal of the newest fed step (what a flush closes with).
 *   pending [N] (int32)  in/out: the starts of the robot that no row holds yet: 0 after a done, else min(n - 1, avail).
 *   mem_obs, mem_action, mem_reward, mem_next_obs, mem_terminal     the memory's arrays, at least max_size rows.
 *   max_size, pos_count  the ring's rows and its {pos, count} (two int64 on the device).
 *   scratch              ETG_NSTEP_SCRATCH_INTS(num_envs, n_steps) int32 (a flush: n_steps = 1); content of no interest.
 *   stream               hipStream_t, or NULL.
 *
 * etg_nstep_feed: three launches -- per step a count of every robot's closing rows and their scan (the row offsets), the row
 * writes (a wave per step and robot, the lane is the column), then the history ring, the tail, pending and pos_count.
 * etg_nstep_flush: closes every pending start at the newest fed step c = step0 - 1: per robot pending[i] rows with the starts
 * c - pending[i] + 1 .. c (m < n, the same formulas, terminal = tail_terminal * g), robot ascending, then start ascending;
 * pending becomes zero.  The caller then restarts t (step0 = 0, hist = 0), so that no start is emitted twice.
 * Invariant: rows emitted + sum(pending) = N * steps fed.  No host synchronisation.
 *
 * Argument checks come before any HIP call and give ETG_ERR_BAD_ARG with the function's name first in etg_last_error(): a
 * null pointer, num_envs < 1, n_steps < 1 (feed), n outside 1..16, hist outside 0..n-1, step0 < hist, obs_dim < 1 or
 * act_dim < 1, (n_steps + n - 1) * num_envs > max_size (a feed's rows must not meet in the ring; a flush: n_steps = 0) and
 * num_envs * (n_steps + n) >= 2^31.                                                                                        */
#ifndef ETGSIM_NSTEP_H_
#define ETGSIM_NSTEP_H_

#include "etgsim.h"

#define ETG_NSTEP_MAX_N 16     /* the longest row: n steps                                                      */
/* int32 elements of `scratch`: per step the number of rows that close in it (1) and per step and robot the number of rows
 * that close in the step at robots before it (1)                                                                          */
#define ETG_NSTEP_SCRATCH_INTS(num_envs, n_steps) ((n_steps) * (1 + (num_envs)))

#ifdef __cplusplus
extern "C" {
#endif

int etg_nstep_feed(int device, int num_envs, int n_steps, int n, float gamma, int hist, int64_t step0, int obs_dim, int act_dim,
                   const float* rec_obs, const float* rec_action, const float* rec_reward, const uint8_t* rec_done,
                   const float* rec_next_obs, const float* rec_terminal, const int32_t* rec_ep_len, float* hist_obs,
                   float* hist_action, float* hist_reward, float* tail_next_obs, float* tail_terminal, int32_t* pending,
                   float* mem_obs, float* mem_action, float* mem_reward, float* mem_next_obs, float* mem_terminal,
                   int64_t max_size, int64_t* pos_count, int32_t* scratch, void* stream);

int etg_nstep_flush(int device, int num_envs, int n, float gamma, int hist, int64_t step0, int obs_dim, int act_dim,
                    const float* hist_obs, const float* hist_action, const float* hist_reward, const float* tail_next_obs,
                    const float* tail_terminal, int32_t* pending, float* mem_obs, float* mem_action, float* mem_reward,
                    float* mem_next_obs, float* mem_terminal, int64_t max_size, int64_t* pos_count, int32_t* scratch,
                    void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ETGSIM_NSTEP_H_ */
