/* etgsim_terminal.h -- the terminal observation of an auto-reset step: the row every robot's step produced, before any restart.
 *
 * etg_step_autoreset writes a finished robot's reset observation over the observation its last step produced, which is the
 * next_obs of its terminal transition (train.py:147-159).  The entry points here keep that row, for every configuration the
 * simulator steps (either lane mapping, sensor noise, random pushes, HYBRID, prepared next-episode dynamics).  The same library
 * as etgsim.h (its ABI version, 2, is unchanged); this header declares the two entry points that are not part of etgsim.h.
 *
 * Contract of etg_step_autoreset_terminal:
 *   h, action, donef, obs, reward, done, info, stream   exactly as etg_step_autoreset; obs, reward, done, info and the simulator
 *                        state come out bit-identical to what etg_step_autoreset writes for the same call.
 *   terminal_obs [N,49]  required: the step's observation of EVERY robot, before any restart.  Rows of robots that go on equal
 *                        their rows of obs.  With sensor noise a row carries the draw of the step's stream position: the draw
 *                        a robot that goes on receives in the same call (the reset rows of obs keep the position after it).
 *   terminal_ctx [N,ETG_TERM_CTX_DIM]   optional: for each robot that restarted in this call, the pre-restart values the extra
 *                        sensor columns of its terminal row are computed from (etg_extra_sensors_terminal).  Rows of robots
 *                        that go on are not written.
 * A null handle or terminal_obs returns ETG_ERR_BAD_ARG; a call before etg_reset returns ETG_ERR_STATE; otherwise as
 * etg_step_autoreset.
 *
 * Contract of etg_extra_sensors_terminal:
 *   terminal_obs, terminal_ctx, done   the rows, context and done bytes one etg_step_autoreset_terminal call wrote, before any
 *                        other call that steps or resets the simulator.
 *   out [N,ETG_EXTRA_DIM]  the ETG_EXTRA_* columns of the terminal rows, as etg_extra_sensors would have computed them right
 *                        after the step: from the live state for robots that go on, from terminal_ctx for restarted ones.
 * A null handle or argument returns ETG_ERR_BAD_ARG; a call before etg_reset returns ETG_ERR_STATE.
 * Pointers are device pointers.                                                                                              */
#ifndef ETGSIM_TERMINAL_H_
#define ETGSIM_TERMINAL_H_

#include "etgsim.h"

/* a row of terminal_ctx (floats) */
#define ETG_TERM_STEP 0                              /* 1 : the episode step index the terminal row was observed at   */
#define ETG_TERM_FORCE 1                             /* 3 : the trunk force of the step, world frame (set + random push) */
#define ETG_TERM_DYN 4                               /* 48: the robot's dynamic_param row during the finished episode  */
#define ETG_TERM_CTX_DIM (ETG_TERM_DYN + ETG_DYN_DIM)

#ifdef __cplusplus
extern "C" {
#endif

int etg_step_autoreset_terminal(EtgHandle* h, const float* action, const uint8_t* donef, float* obs, float* terminal_obs,
                                float* terminal_ctx, float* reward, uint8_t* done, float* info, void* stream);
int etg_extra_sensors_terminal(EtgHandle* h, const float* terminal_obs, const float* terminal_ctx, const uint8_t* done,
                               float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ETGSIM_TERMINAL_H_ */
