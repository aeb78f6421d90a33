/* etgsim_snapshot.h -- save, restore and transplant the simulator state of robots: the saveState / restoreState of the reference's
 * simulator.
 *
 * A RECORD is everything the library keeps for one robot between calls: its slices of the state arrays (floating base, legs,
 * control loop, ETG weights, derived parameters, dynamic_param row, latency ring), its settle cache (cached state and ring, the
 * cached first observation, the start offsets) and the rows prepared for its next episode (etg_prepare_next_dynamics).  A later
 * etg_step*, etg_reset, etg_rollout_*, etg_prepare_next_dynamics, etg_episode_stats or etg_extra_sensors reads nothing else of
 * that robot, so a robot restored from its record goes on bit for bit as the saved one did.  Both lane mappings share the state
 * layout, so a record saved under one mapping can be restored under the other.  DESIGN.md section 5 lists the contents.
 *
 * Records are robot-major: rows [n, row_bytes] on the device, one contiguous record per robot (the state arrays are
 * field-major).  The first 16 bytes of a record hold the id of the robot it was saved from.  The same library as etgsim.h (its
 * ABI version, 2, is unchanged); this header declares the entry points that are not part of etgsim.h.
 *
 * Contract:
 *   etg_snapshot_row_bytes(h)   the size of one record of this handle in bytes, a multiple of 16; ETG_ERR_BAD_ARG for a null handle.
 *   etg_snapshot_save(h, env_ids, n, rows, hdr, stream)
 *       env_ids [n]   device int32 array of robot ids in [0, N) (duplicates allowed), or NULL: all robots, n must equal N.
 *       rows          device memory of n * row_bytes bytes, 16-byte aligned.
 *       hdr           host struct, filled in: what a restore checks, and the handle's scalars.
 *   etg_snapshot_restore(h, env_ids, n, rows, hdr, stream)
 *       env_ids [n]   the TARGET robot of each record (no duplicates), or NULL: record i goes to robot i, n must equal N and the
 *                     snapshot must be a whole one of N robots.  With ids, 1 <= n <= hdr->n: a prefix of the saved records.
 *       The handle's scalars (stream positions of the sensor noise and the random pushes, was_reset, the force flags, all_cached)
 *       are restored only when env_ids is NULL.  After a whole restore of a handle that had been reset the handle steps as after
 *       etg_reset, and etg_step_autoreset takes its one-launch path again when the saved handle did.  After a restore by ids the
 *       one-launch path stays only if both the saved and the target handle had every settle cached.
 *   Sensor-noise levels and seed (etg_set_sensor_noise), the rollout mode (etg_set_rollout_mode) and the heightfield's heights are
 *   the caller's: a restore does not change them, and the caller restores into a handle with the same heights.
 * ETG_ERR_BAD_ARG, with the simulator state unchanged: a null handle or pointer; n out of range; an id outside [0, N); a
 * duplicate target id; a header whose magic, format, ABI version, row_bytes, layout or configuration fingerprint differs from
 * this handle's; on a heightfield with bands, a target id whose band (id % hf_bands) differs from the band of the robot the
 * record was saved from.  Both calls may wait for `stream` once (ids are checked on the host).  rows and env_ids are device
 * pointers, hdr is a host pointer.                                                                                            */
#ifndef ETGSIM_SNAPSHOT_H_
#define ETGSIM_SNAPSHOT_H_

#include "etgsim.h"

#define ETG_SNAPSHOT_MAGIC 0x53475445u /* "ETGS" */
#define ETG_SNAPSHOT_FORMAT 1

typedef struct EtgSnapshotHeader {
  uint32_t magic;          /* ETG_SNAPSHOT_MAGIC */
  int32_t format;          /* ETG_SNAPSHOT_FORMAT */
  int32_t abi_version;     /* etg_version() */
  int32_t row_bytes;       /* etg_snapshot_row_bytes() */
  uint64_t layout_fp;      /* fingerprint of the layout constants (the record's segments and their sizes) */
  uint64_t config_fp;      /* fingerprint of the EtgConfig fields that give the record its meaning: sim_dt, action_repeat,
                              settle_ticks, etg_dt, enable_etg, motor mode, action filter / interpolation, pd_latency,
                              body_contacts, terrain kind and geometry (the lane mapping is not among them) */
  int32_t num_envs;        /* N of the handle saved from */
  int32_t n;               /* records saved */
  int32_t whole;           /* 1: saved with env_ids == NULL */
  int32_t hf_bands;
  /* the handle's scalars */
  uint64_t push_calls;     /* stream position of etg_random_pushes */
  uint32_t obs_calls;      /* stream position of the sensor noise */
  uint32_t noise_call;
  uint8_t was_reset, fext_set, push_on, all_cached;
  uint8_t strength_on;     /* motor strength ratios are installed */
  uint8_t next_dyn;        /* the next-episode rows are allocated (their segment of a record is zero otherwise) */
  uint8_t pad_[2];
} EtgSnapshotHeader;

#ifdef __cplusplus
extern "C" {
#endif

int etg_snapshot_row_bytes(EtgHandle* h);
int etg_snapshot_save(EtgHandle* h, const int32_t* env_ids, int n, void* rows, EtgSnapshotHeader* hdr, void* stream);
int etg_snapshot_restore(EtgHandle* h, const int32_t* env_ids, int n, const void* rows, const EtgSnapshotHeader* hdr, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ETGSIM_SNAPSHOT_H_ */
