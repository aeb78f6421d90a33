"""ctypes binding of the C-ABI in include/etgsim.h, include/etgsim_step_policy.h, include/etgsim_terminal.h,
include/etgsim_render.h, include/etgsim_sac.h, include/etgsim_bc.h, include/etgsim_snapshot.h, include/etgsim_collect.h, include/etgsim_monitor.h, include/etgsim_nstep.h, include/etgsim_heightscan.h and include/etgsim_ppo.h
(paddlerobotics_amd/csrc/libetgsim.so).

There is no CPU fallback: if the library is missing this module raises, and if no HIP
device is visible etg_create() fails with ETG_ERR_NO_DEVICE.
"""
import ctypes as C
import os

from . import build as _build

_LIB = None

SYMBOLS = [
    "etg_create", "etg_destroy", "etg_last_error", "etg_version", "etg_lanes_per_robot", "etg_set_params",
    "etg_set_heightfield", "etg_set_external_force", "etg_set_motor_strength", "etg_random_pushes", "etg_clear_pushes", "etg_set_reset_offsets", "etg_set_sensor_noise", "etg_reset", "etg_step", "etg_episode_stats", "etg_rollout_openloop",
    "etg_get_state",
    "etg_set_state", "etg_policy_create", "etg_policy_load", "etg_policy_forward", "etg_policy_load_std", "etg_policy_sample",
    "etg_policy_destroy", "etg_rollout_policy", "etg_fit_etg", "etg_leg_kinematics", "etg_extra_sensors", "etg_step_autoreset",
    "etg_replay_begin", "etg_replay_end", "etg_rollout_policy_record", "etg_rollout_actions",
    "etg_prepare_next_dynamics", "etg_next_dynamics_pending",
    "etg_config_size", "etg_model_size", "etg_get_contact_impulses", "etg_set_contact_impulses", "etg_set_rollout_mode", "etg_rollout_wave_cycles", "etg_step_range",
]
# entry points declared in a header of their own (same library, same ABI version): include/etgsim_step_policy.h
STEP_POLICY_SYMBOLS = ["etg_step_policy"]
# ... and include/etgsim_terminal.h
TERMINAL_SYMBOLS = ["etg_step_autoreset_terminal", "etg_extra_sensors_terminal"]
# ... and include/etgsim_render.h
RENDER_SYMBOLS = ["etg_render"]
# ... and include/etgsim_sac.h
SAC_SYMBOLS = ["etg_sac_create", "etg_sac_destroy", "etg_sac_set_hyper", "etg_sac_load", "etg_sac_store", "etg_sac_load_opt",
               "etg_sac_store_opt", "etg_sac_learn", "etg_sac_learn_replay", "etg_sac_grads", "etg_sac_sync_policy"]
# ... and include/etgsim_bc.h
BC_SYMBOLS = ["etg_bc_create", "etg_bc_destroy", "etg_bc_set_hyper", "etg_bc_load", "etg_bc_store", "etg_bc_load_opt",
              "etg_bc_store_opt", "etg_bc_set_teacher", "etg_bc_learn", "etg_bc_learn_replay", "etg_bc_grads", "etg_bc_sync_policy"]
# ... and include/etgsim_snapshot.h
SNAPSHOT_SYMBOLS = ["etg_snapshot_row_bytes", "etg_snapshot_save", "etg_snapshot_restore"]
# ... and include/etgsim_collect.h
COLLECT_SYMBOLS = ["etg_collect_policy"]
# ... and include/etgsim_monitor.h
MONITOR_SYMBOLS = ["etg_collect_policy_info", "etg_monitor_feed"]
# ... and include/etgsim_nstep.h
NSTEP_SYMBOLS = ["etg_nstep_feed", "etg_nstep_flush"]
# ... and include/etgsim_heightscan.h
HEIGHTSCAN_SYMBOLS = ["etg_scan_pose", "etg_height_scan_at", "etg_height_scan"]
# ... and include/etgsim_ppo.h
PPO_SYMBOLS = ["etg_ppo_create", "etg_ppo_destroy", "etg_ppo_set_hyper", "etg_ppo_load", "etg_ppo_store", "etg_ppo_load_opt",
               "etg_ppo_store_opt", "etg_ppo_sync_policy", "etg_ppo_prepare", "etg_ppo_gae", "etg_ppo_norm_adv", "etg_ppo_fetch",
               "etg_ppo_learn", "etg_ppo_learn_rows", "etg_ppo_grads"]
# ... and its controls (the same header, "Controls"): a list of their own, the base list above stays as it is
PPO_CONTROL_SYMBOLS = ["etg_ppo2_set_controls", "etg_ppo2_learn", "etg_ppo2_grads", "etg_ppo2_reset_stop", "etg_ppo2_set_state",
                       "etg_ppo2_get_state"]
ABI_VERSION = 2      # include/etgsim.h: etg_version()


class EtgError(RuntimeError):
    pass


class EtgSnapshotHeader(C.Structure):
    """include/etgsim_snapshot.h: what a restore checks, and the handle's scalars"""
    _fields_ = [("magic", C.c_uint32), ("format", C.c_int32), ("abi_version", C.c_int32), ("row_bytes", C.c_int32),
                ("layout_fp", C.c_uint64), ("config_fp", C.c_uint64), ("num_envs", C.c_int32), ("n", C.c_int32),
                ("whole", C.c_int32), ("hf_bands", C.c_int32), ("push_calls", C.c_uint64), ("obs_calls", C.c_uint32),
                ("noise_call", C.c_uint32), ("was_reset", C.c_uint8), ("fext_set", C.c_uint8), ("push_on", C.c_uint8),
                ("all_cached", C.c_uint8), ("strength_on", C.c_uint8), ("next_dyn", C.c_uint8), ("pad_", C.c_uint8 * 2)]


def lib_path():
    # ETG_LIB selects an alternative build of the same HIP sources (A/B experiments in tools/)
    return os.environ.get("ETG_LIB", _build.LIB)


def load():
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not os.path.exists(path):
        raise EtgError(
            "paddlerobotics_amd: %s is missing -- build it with `python -m paddlerobotics_amd.build` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback." % path)
    # torch first: its HIP runtime then satisfies the library's libamdhip64.so.7 / libhsa-runtime64.so.1 by soname.  Loaded the
    # other way round, the process maps a second HIP + HSA stack, and whichever initialises second finds no device.
    import torch  # noqa: F401
    lib = C.CDLL(path)
    lib.etg_last_error.restype = C.c_char_p
    vp, i32 = C.c_void_p, C.c_int
    lib.etg_create.argtypes = [vp, vp, i32, C.POINTER(vp)]
    lib.etg_destroy.argtypes = [vp]
    lib.etg_destroy.restype = None
    lib.etg_lanes_per_robot.argtypes = [vp]
    lib.etg_set_params.argtypes = [vp, vp, vp, vp, i32, vp, vp]
    lib.etg_set_heightfield.argtypes = [vp, vp, vp]
    lib.etg_set_external_force.argtypes = [vp, vp, vp]
    lib.etg_set_motor_strength.argtypes = [vp, vp, vp, vp]
    lib.etg_random_pushes.argtypes = [vp, C.c_uint64, C.c_float, i32, C.c_float, C.c_float, vp]
    lib.etg_clear_pushes.argtypes = [vp, vp, vp]
    lib.etg_set_reset_offsets.argtypes = [vp, vp, vp, vp]
    lib.etg_set_sensor_noise.argtypes = [vp, vp, C.c_uint64]
    lib.etg_reset.argtypes = [vp, vp, vp, vp]
    lib.etg_step.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp]
    lib.etg_step_autoreset.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp]
    lib.etg_step_range.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp]
    lib.etg_episode_stats.argtypes = [vp, vp, vp, vp]
    lib.etg_rollout_openloop.argtypes = [vp, i32, vp, vp, vp, vp]
    lib.etg_get_state.argtypes = [vp, vp, vp]
    lib.etg_set_state.argtypes = [vp, vp, vp]
    lib.etg_set_rollout_mode.argtypes = [vp, i32]
    lib.etg_rollout_wave_cycles.argtypes = [vp, vp, i32, C.POINTER(i32), C.POINTER(i32), vp]
    lib.etg_get_contact_impulses.argtypes = [vp, vp, vp]
    lib.etg_set_contact_impulses.argtypes = [vp, vp, vp]
    lib.etg_leg_kinematics.argtypes = [vp, vp, i32, vp, vp, vp]
    lib.etg_extra_sensors.argtypes = [vp, vp, vp, vp]
    lib.etg_policy_create.argtypes = [i32, i32, i32, i32, C.POINTER(vp)]
    lib.etg_policy_load.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp]
    lib.etg_policy_forward.argtypes = [vp, vp, i32, C.c_float, i32, vp, vp]
    lib.etg_policy_load_std.argtypes = [vp, vp, vp, vp]
    lib.etg_policy_sample.argtypes = [vp, vp, i32, vp, C.c_float, i32, vp, vp, vp]
    lib.etg_policy_destroy.argtypes = [vp]
    lib.etg_rollout_policy.argtypes = [vp, vp, i32, C.c_float, i32, i32, vp, vp, vp, vp]
    lib.etg_rollout_policy_record.argtypes = [vp, vp, i32, C.c_float, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.etg_step_policy.argtypes = [vp, vp, C.c_float, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.etg_collect_policy.argtypes = [vp, vp, C.c_float, i32, i32, i32, i32] + [vp] * 12
    lib.etg_collect_policy_info.argtypes = [vp, vp, C.c_float, i32, i32, i32, i32] + [vp] * 13
    lib.etg_monitor_feed.argtypes = [i32, i32, i32, C.c_longlong, C.c_float, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp]
    lib.etg_nstep_feed.argtypes = [i32, i32, i32, i32, C.c_float, i32, C.c_longlong, i32, i32] + [vp] * 18 + [C.c_longlong, vp, vp, vp]
    lib.etg_nstep_flush.argtypes = [i32, i32, i32, C.c_float, i32, C.c_longlong, i32, i32] + [vp] * 11 + [C.c_longlong, vp, vp, vp]
    lib.etg_scan_pose.argtypes = [vp, vp, vp]
    lib.etg_height_scan_at.argtypes = [vp, vp, vp, i32, vp, i32, C.c_float, C.c_float, vp, vp]
    lib.etg_height_scan.argtypes = [vp, vp, i32, C.c_float, C.c_float, vp, vp]
    lib.etg_step_autoreset_terminal.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.etg_extra_sensors_terminal.argtypes = [vp, vp, vp, vp, vp, vp]
    lib.etg_render.argtypes = [vp, vp, vp, i32, vp, vp, i32, i32, vp, vp, vp, vp]
    lib.etg_snapshot_row_bytes.argtypes = [vp]
    lib.etg_snapshot_save.argtypes = [vp, vp, i32, vp, C.POINTER(EtgSnapshotHeader), vp]
    lib.etg_snapshot_restore.argtypes = [vp, vp, i32, vp, C.POINTER(EtgSnapshotHeader), vp]
    lib.etg_sac_create.argtypes = [i32, i32, i32, i32, i32, C.POINTER(vp)]
    lib.etg_sac_destroy.argtypes = [vp]
    lib.etg_sac_set_hyper.argtypes = [vp] + [C.c_double] * 5
    lib.etg_sac_load.argtypes = [vp, C.POINTER(vp), i32, vp]
    lib.etg_sac_store.argtypes = [vp, C.POINTER(vp), i32, vp]
    lib.etg_sac_load_opt.argtypes = [vp, vp, vp, vp, vp, vp]
    lib.etg_sac_store_opt.argtypes = [vp, vp, vp, vp, vp, vp]
    lib.etg_sac_learn.argtypes = [vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp]
    lib.etg_sac_learn_replay.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp]
    lib.etg_sac_grads.argtypes = [vp, vp, vp, vp, vp, vp, i32, vp, vp, C.POINTER(vp), vp]
    lib.etg_sac_sync_policy.argtypes = [vp, vp, vp]
    lib.etg_bc_create.argtypes = [i32, i32, i32, i32, i32, i32, C.POINTER(vp)]
    lib.etg_bc_destroy.argtypes = [vp]
    lib.etg_bc_set_hyper.argtypes = [vp, C.c_double, C.c_double]
    lib.etg_bc_load.argtypes = [vp, C.POINTER(vp), i32, vp]
    lib.etg_bc_store.argtypes = [vp, C.POINTER(vp), i32, vp]
    lib.etg_bc_load_opt.argtypes = [vp, vp, vp, vp, vp]
    lib.etg_bc_store_opt.argtypes = [vp, vp, vp, vp, vp]
    lib.etg_bc_set_teacher.argtypes = [vp, C.POINTER(vp), vp]
    lib.etg_bc_learn.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp]
    lib.etg_bc_learn_replay.argtypes = [vp, vp, vp, vp, i32, vp, vp, vp, vp]
    lib.etg_bc_grads.argtypes = [vp, vp, vp, i32, vp, vp, C.POINTER(vp), vp]
    lib.etg_bc_sync_policy.argtypes = [vp, vp, vp]
    lib.etg_ppo_create.argtypes = [i32, i32, i32, i32, i32, i32, C.POINTER(vp)]
    lib.etg_ppo_destroy.argtypes = [vp]
    lib.etg_ppo_set_hyper.argtypes = [vp] + [C.c_double] * 4
    lib.etg_ppo_load.argtypes = [vp, C.POINTER(vp), i32, vp]
    lib.etg_ppo_store.argtypes = [vp, C.POINTER(vp), i32, vp]
    lib.etg_ppo_load_opt.argtypes = [vp, vp, vp, vp, vp]
    lib.etg_ppo_store_opt.argtypes = [vp, vp, vp, vp, vp]
    lib.etg_ppo_sync_policy.argtypes = [vp, vp, vp]
    lib.etg_ppo_prepare.argtypes = [vp, vp, vp, vp, i32, vp]
    lib.etg_ppo_gae.argtypes = [vp, vp, vp, vp, i32, i32, C.c_float, C.c_float, vp, vp, vp, vp, vp]
    lib.etg_ppo_norm_adv.argtypes = [vp, vp, i32, vp]
    lib.etg_ppo_fetch.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp]
    lib.etg_ppo_learn.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, vp, vp]
    lib.etg_ppo_learn_rows.argtypes = [vp, vp, vp, vp, i32, vp, vp]
    lib.etg_ppo_grads.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, C.POINTER(vp), vp]
    lib.etg_ppo2_set_controls.argtypes = [vp, C.c_double, C.c_double, C.c_double, i32, C.c_double, C.c_double]
    lib.etg_ppo2_learn.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp]
    lib.etg_ppo2_grads.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, i32, C.POINTER(vp), vp]
    lib.etg_ppo2_reset_stop.argtypes = [vp, vp]
    lib.etg_ppo2_set_state.argtypes = [vp, C.c_double, i32, vp]
    lib.etg_ppo2_get_state.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(i32), C.POINTER(C.c_longlong), C.POINTER(C.c_double), vp]
    lib.etg_rollout_actions.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.etg_prepare_next_dynamics.argtypes = [vp, vp, vp, vp]
    lib.etg_next_dynamics_pending.argtypes = [vp, vp, vp]
    lib.etg_policy_destroy.restype = None
    dbl = C.c_double
    lib.etg_fit_etg.argtypes = [vp, i32, vp, vp, dbl, dbl, dbl, dbl, dbl, i32, vp, vp, vp]
    ll = C.c_longlong
    lib.etg_replay_begin.argtypes = [vp, i32, ll, vp, vp, vp, i32, vp, i32, vp, vp, C.c_float, vp, vp]
    lib.etg_replay_end.argtypes = [vp, i32, vp, vp, vp, i32, vp, vp, vp, vp, i32, i32, i32, vp, vp, vp]
    # a library built from another revision of include/etgsim.h would read past (or short of) the structs this binding
    # passes to etg_create: refuse it here, with the reason, instead of simulating with garbage parameters
    from . import a1_model as _A
    if lib.etg_version() != ABI_VERSION or lib.etg_config_size() != C.sizeof(_A.EtgConfig) or lib.etg_model_size() != C.sizeof(_A.EtgRobotModel):
        raise EtgError("paddlerobotics_amd: %s has ABI version %d with EtgConfig / EtgRobotModel of %d / %d bytes; this binding is "
                       "version %d with %d / %d bytes -- rebuild the library (python -m paddlerobotics_amd.build)" % (
                           path, lib.etg_version(), lib.etg_config_size(), lib.etg_model_size(), ABI_VERSION,
                           C.sizeof(_A.EtgConfig), C.sizeof(_A.EtgRobotModel)))
    _LIB = lib
    return lib


ETG_ERR_STATE = -5   # include/etgsim.h


def check(code):
    if code != 0:
        raise EtgError("etgsim error %d: %s" % (code, load().etg_last_error().decode()))
