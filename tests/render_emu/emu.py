"""ctypes wrapper of the TEST-ONLY host build of the renderer source (render_emu.cpp over csrc/render_core.h)."""
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
        so = os.path.join(_HERE, "librender_emu.so")
        srcs = [os.path.join(_HERE, "render_emu.cpp")] + [os.path.join(_CSRC, f) for f in ("render_core.h", "etg_layout.h")]
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, srcs[0]])
        _LIB = C.CDLL(so)
    return _LIB


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def config(heightfield=None):
    """the EtgConfig / EtgRobotModel of a make_env with this heightfield dict (None: flat ground)"""
    return A.default_config(1, terrain=1 if heightfield is not None else 0, heightfield=heightfield), A.default_model()


def render(states, views, projs, width, height, heightfield=None, env_ids=None):
    """-> rgba [n,H,W,4] uint8, depth [n,H,W] float32, seg [n,H,W] int32 of state rows [n,37] and matrices [n,16]"""
    st = np.ascontiguousarray(np.asarray(states, np.float32).reshape(-1, A.STATE_DIM))
    n = st.shape[0]
    v = np.ascontiguousarray(np.broadcast_to(np.asarray(views, np.float32).reshape(-1, 16), (n, 16)))
    p = np.ascontiguousarray(np.broadcast_to(np.asarray(projs, np.float32).reshape(-1, 16), (n, 16)))
    ids = np.ascontiguousarray(np.zeros(n) if env_ids is None else env_ids, dtype=np.int32)
    hf = None if heightfield is None else np.ascontiguousarray(heightfield["heights"], dtype=np.float32)
    cfg, model = config(heightfield)
    rgba = np.zeros((n, height, width, 4), np.uint8)
    depth = np.zeros((n, height, width), np.float32)
    seg = np.zeros((n, height, width), np.int32)
    lib().remu_render(C.byref(cfg), C.byref(model), _p(hf), _p(st), _p(ids), n, _p(v), _p(p), int(width), int(height), _p(rgba),
                      _p(depth), _p(seg))
    return rgba, depth, seg


def prims(state):
    """world (o1, o2, o3, pf) [4 legs, 4, 3] of the renderer's primitives for one state row"""
    cfg, model = config()
    st = np.ascontiguousarray(state, dtype=np.float32)
    out = np.zeros((4, 4, 3), np.float32)
    lib().remu_prims(C.byref(cfg), C.byref(model), _p(st), _p(out))
    return out
