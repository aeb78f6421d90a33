"""CPU suite: the C-ABI of the closed-loop launches with scan columns (include/etgsim_scan_policy.h) as the binding sees it,
and the helper of scan_core.h their kernels add -- no GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np

from paddlerobotics_amd import _lib, build

_HERE = os.path.dirname(os.path.abspath(__file__))
_HEADER = os.path.join(_HERE, "..", "include", "etgsim_scan_policy.h")


def test_the_header_parses_to_the_two_entry_points():
    protos = _lib.parse_header(open(_HEADER).read())
    assert sorted(protos) == ["etg_collect_policy_scan", "etg_step_policy_scan"]
    # the arguments of etg_step_policy / etg_collect_policy_info, then points, n_points, offset, clip, scan in front of the stream
    step = _lib.parse_header(open(os.path.join(_HERE, "..", "include", "etgsim_step_policy.h")).read())["etg_step_policy"]
    coll = _lib.parse_header(open(os.path.join(_HERE, "..", "include", "etgsim_monitor.h")).read())["etg_collect_policy_info"]
    added = [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_void_p]
    for name, base in (("etg_step_policy_scan", step), ("etg_collect_policy_scan", coll)):
        restype, args = protos[name]
        assert restype is C.c_int
        assert args == base[1][:-1] + added + [C.c_void_p], name


def test_the_symbols_are_listed_and_get_prototypes():
    assert _lib.SCAN_POLICY_SYMBOLS == ["etg_step_policy_scan", "etg_collect_policy_scan"]
    assert any(os.path.basename(h) == "etgsim_scan_policy.h" for h in build.HEADERS)
    protos = _lib.prototypes()          # (raises when the lists and the headers differ)
    for name in _lib.SCAN_POLICY_SYMBOLS:
        assert name in protos and len(protos[name][1]) in (21, 25)
    assert _lib.ABI_VERSION == 2


def _rows_lib():
    src = os.path.join(_HERE, "scan_emu", "row_emu.cpp")
    so = os.path.join(_HERE, "scan_emu", "librow_emu.so")
    csrc = os.path.join(_HERE, "..", "paddlerobotics_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in ("scan_core.h", "etg_layout.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, src])
    return C.CDLL(so)


def test_row_of_base_is_state_pose_then_make_row_bit_for_bit():
    """400 robots: random unit quaternions, near-unit ones (|q| off by up to 1e-3, as an integrated state is), the yaw's
    special directions (identity, half turns, pitch +-90 degrees where sy = cy = 0 up to rounding) and positions of both signs"""
    rng = np.random.default_rng(7)
    q = rng.normal(size=(400, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    q[100:300] *= 1.0 + rng.uniform(-1e-3, 1e-3, size=(200, 1))
    h = np.sqrt(0.5)
    q[:8] = [[0, 0, 0, 1], [0, 0, 1, 0], [0, 0, h, h], [0, 0, -h, h], [0, h, 0, h], [0, -h, 0, h], [1, 0, 0, 0], [0, 1, 0, 0]]
    base7 = np.concatenate([rng.uniform(-20, 20, size=(400, 3)), q], axis=1).astype(np.float32)
    a, b = np.full((400, 6), 9.0, np.float32), np.full((400, 6), 9.0, np.float32)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    _rows_lib().remu_rows(p(base7), 400, p(a), p(b))
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.array_equal(a[:, :3], base7[:, :3]) and np.array_equal(a[:, 5], np.arange(400, dtype=np.float32))
    assert np.all(np.abs(a[:, 3] ** 2 + a[:, 4] ** 2 - 1.0) < 1e-6)          # a cos / sin pair, not a sentinel left in place
    yaw = np.arctan2(2 * (q[:, 3] * q[:, 2] + q[:, 0] * q[:, 1]), 1 - 2 * (q[:, 1] ** 2 + q[:, 2] ** 2))
    ok = np.hypot(2 * (q[:, 3] * q[:, 2] + q[:, 0] * q[:, 1]), 1 - 2 * (q[:, 1] ** 2 + q[:, 2] ** 2)) > 1e-2   # (yaw is defined there)
    assert np.all(np.abs(a[ok, 3] - np.cos(yaw[ok])) < 1e-4) and np.all(np.abs(a[ok, 4] - np.sin(yaw[ok])) < 1e-4)
