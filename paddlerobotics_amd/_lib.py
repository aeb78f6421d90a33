"""ctypes binding of the C-ABI (paddlerobotics_amd/csrc/libetgsim.so).  The prototypes are read from the headers under include/
that build.HEADERS lists: a header is the only place where an entry point's parameters are written down.

There is no CPU fallback: if the library is missing this module raises, and if no HIP
device is visible etg_create() fails with ETG_ERR_NO_DEVICE.
"""
import collections
import ctypes as C
import os
import re

import torch

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
# ... and include/etgsim_scan_policy.h
SCAN_POLICY_SYMBOLS = ["etg_step_policy_scan", "etg_collect_policy_scan"]
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


# C types passed by value -> ctypes.  Every T* is a c_void_p and every T** a POINTER(c_void_p); anything else is refused.
_CTYPES = {"int": C.c_int, "int32_t": C.c_int, "float": C.c_float, "double": C.c_double, "uint64_t": C.c_uint64,
           "int64_t": C.c_longlong, "long long": C.c_longlong}
# host out-parameters that the callers pass with byref(): {function: {parameter index: type}}
_TYPED = {"etg_snapshot_save": {4: C.POINTER(EtgSnapshotHeader)}, "etg_snapshot_restore": {4: C.POINTER(EtgSnapshotHeader)},
          "etg_rollout_wave_cycles": {3: C.POINTER(C.c_int), 4: C.POINTER(C.c_int)},
          "etg_ppo2_get_state": {1: C.POINTER(C.c_double), 2: C.POINTER(C.c_int), 3: C.POINTER(C.c_longlong), 4: C.POINTER(C.c_double)}}
_DECL = re.compile(r"([A-Za-z_][\w\s*]*?)\b(etg_[a-z0-9_]+)\s*\(([^;{}]*)\)\s*;")


def _ctype(func, decl, param):
    """ctypes type of `decl`: a parameter of `func` with its name (`param`), or its return type"""
    m = re.fullmatch(r"\s*([\w\s]+?)\s*((?:\*\s*)*)" + (r"\b\w+\s*" if param else ""), re.sub(r"\bconst\b", " ", decl))
    base, stars = (" ".join(m.group(1).split()), m.group(2).count("*")) if m else ("", 0)
    if stars == 0 and base in _CTYPES:
        return _CTYPES[base]
    if stars == 0 and base == "void" and not param:
        return None
    if stars == 1 and base:
        return C.c_char_p if base == "char" and not param else C.c_void_p
    if stars == 2 and base:
        return C.POINTER(C.c_void_p)
    raise EtgError("paddlerobotics_amd: %s: no ctypes mapping for `%s`" % (func, " ".join(decl.split())))


def parse_header(text):
    """{name: (restype, argtypes)} of every etg_* declaration in the text of a C header.  A type outside the mapping above
    (a struct by value, a function pointer, an array, a parameter without its name) and a declaration that this cannot
    split raise EtgError: nothing is guessed and nothing is skipped."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#(?:.*\\\n)*.*$", " ", text, flags=re.M)      # preprocessor lines, continued ones included
    decls = _DECL.findall(text)
    odd = collections.Counter(re.findall(r"\b(etg_[a-z0-9_]+)\s*\(", text)) - collections.Counter(name for _, name, _ in decls)
    if odd:
        raise EtgError("paddlerobotics_amd: cannot split the declaration of %s" % ", ".join(sorted(odd)))
    out = {}
    for ret, name, params in decls:
        if name in out:
            raise EtgError("paddlerobotics_amd: %s is declared twice" % name)
        params = [] if params.strip() in ("", "void") else params.split(",")
        out[name] = (_ctype(name, ret, False), [_ctype(name, p, True) for p in params])
        for i, t in _TYPED.get(name, {}).items():
            if out[name][1][i] is not C.c_void_p:
                raise EtgError("paddlerobotics_amd: %s: parameter %d is typed in _TYPED but is no pointer in the header" % (name, i))
            out[name][1][i] = t
    return out


def prototypes():
    """parse_header over the headers of include/, checked against the *_SYMBOLS lists above"""
    out = {}
    for h in _build.HEADERS:
        path = os.path.normpath(os.path.join(_build.CSRC, h))
        if os.path.basename(os.path.dirname(path)) == "include":
            protos = parse_header(open(path).read())
            if set(protos) & set(out):
                raise EtgError("paddlerobotics_amd: %s: declared in another header too" % ", ".join(sorted(set(protos) & set(out))))
            out.update(protos)
    listed = {s for k, v in globals().items() if k.endswith("SYMBOLS") for s in v}
    if listed != set(out):
        raise EtgError("paddlerobotics_amd: the *_SYMBOLS lists and the headers differ: %s" % ", ".join(sorted(listed ^ set(out))))
    return out


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
    # torch first (imported above): its HIP runtime then satisfies the library's libamdhip64.so.7 / libhsa-runtime64.so.1 by
    # soname.  Loaded the other way round, the process maps a second HIP + HSA stack, and whichever initialises second finds no device.
    lib = C.CDLL(path)
    for name, (restype, argtypes) in prototypes().items():
        f = getattr(lib, name)
        f.restype, f.argtypes = restype, argtypes
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


def ptr(t):
    """a tensor's device pointer as an argument (None stays None: an optional array)"""
    return None if t is None else C.c_void_p(t.data_ptr())


def stream_ptr(device):
    """torch's current stream on `device` as the `void* stream` argument"""
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
