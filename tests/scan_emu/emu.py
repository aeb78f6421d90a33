"""ctypes wrapper of the TEST-ONLY host build of the height scan's source (scan_emu.cpp over csrc/scan_core.h)."""
import ctypes as C
import os
import subprocess

import numpy as np

from paddlerobotics_amd import a1_model as A

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "..", "..", "paddlerobotics_amd", "csrc")
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(_HERE, "libscan_emu.so")
        srcs = [os.path.join(_HERE, "scan_emu.cpp")] + [os.path.join(_CSRC, f) for f in ("scan_core.h", "etg_layout.h")]
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
            # -ffp-contract=off: every fp32 operation rounds on its own, as stock torch's do (the fused ones are written as fmaf)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, srcs[0]])
        _LIB = C.CDLL(so)
    return _LIB


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def scan_pose(states):
    """-> [n,4] float32 (x, y, z, yaw) of state rows [n,37]"""
    st = np.ascontiguousarray(np.asarray(states, np.float32).reshape(-1, A.STATE_DIM))
    pose = np.zeros((st.shape[0], 4), np.float32)
    lib().semu_scan_pose(_p(st), st.shape[0], _p(pose))
    return pose


def height_scan_at(pose, points, num_envs, heightfield=None, env_ids=None, offset=0.32, clip=1.0):
    """-> [M,P] float32: scan_core.h on the host for pose rows [M,4], the robots `env_ids` (None: row i is robot i % num_envs)
    of a simulator of num_envs robots made with this heightfield dict (None: flat ground)"""
    pose = np.ascontiguousarray(np.asarray(pose, np.float32).reshape(-1, 4))
    pts = np.ascontiguousarray(np.asarray(points, np.float32).reshape(-1, 2))
    ids = None if env_ids is None else np.ascontiguousarray(env_ids, dtype=np.int32)
    hf = None if heightfield is None else np.ascontiguousarray(heightfield["heights"], dtype=np.float32)
    cfg = A.default_config(int(num_envs), terrain=1 if heightfield is not None else 0, heightfield=heightfield)
    model = A.default_model()
    out = np.zeros((pose.shape[0], pts.shape[0]), np.float32)
    lib().semu_height_scan_at(C.byref(cfg), C.byref(model), _p(hf), _p(pose), _p(ids), pose.shape[0], _p(pts), pts.shape[0],
                              C.c_float(offset), C.c_float(clip), _p(out))
    return out
