"""GPU suite: the robot layer of the HIP library (delayed observation, angle wrap, action interpolation, motor-command clip,
sensor-mode selection, history stack) against tests/robot_layer_ref.py, the plain fp64 restatement that
tests/test_robot_layer.py pins to the executed reference (tests/golden/robotlayer.npz).

The checks are those of the CPU suite (tests/robot_layer_checks.py), run on make_env(...) for both lane mappings: the library
against the restatement applied to the library's OWN per-tick states.  Bound per column group or state group: 4 x the gap of
the fp32 oracle in the same check on its own states (computed here, in the same test), floor 4 fp32 ulps of the group's largest
magnitude.  Every run rewrites profiles/robot_layer_parity.txt."""
import os

import numpy as np
import pytest
import torch

from paddlerobotics_amd import a1_model as A
from tests import robot_layer_checks as L
from tests import robot_layer_ref as R
from tests.test_gpu_parity import _need_gpu, _make
from tests.test_robot_layer import _oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = {}          # (check, lanes) -> lines


class _Lib:
    """the backend surface of tests/robot_layer_checks.py on a BatchedQuadrupedEnv"""

    def __init__(self, n, lanes, action_repeat=1, interp=False, clip=False, joint_limits=True):
        self.e = _make(n, ETG=0, solver_iters=4, action_repeat=action_repeat, enable_action_interpolation=interp,
                       enable_clip_motor_commands=clip, joint_limits=joint_limits, lanes_per_robot=lanes)
        assert self.e.lanes_per_robot == lanes
        assert self.e.cfg.clip_motor_commands == (R.CLIP_WIDTH if clip else 0.0)

    def set_params(self, dyn):
        self.e.set_dynamic_param(np.asarray(dyn))

    def reset(self):
        self.e.reset()

    def step(self, action):
        self.e.step(torch.as_tensor(np.asarray(action), dtype=torch.float32, device="cuda:0"), want_info=False)
        return self.e.obs.clone()

    def get_state(self):
        return self.e.get_state()

    def set_state(self, st):
        self.e.set_state(np.asarray(st))


def _write_report():
    head = ["The robot layer of the HIP library against tests/robot_layer_ref.py applied to the library's own per-tick states",
            "(pytest -m gpu tests/test_gpu_robot_layer.py).  gap: largest difference in the group; yardstick: the fp32 oracle's gap",
            "in the same check on its own states; bound = max(4 x yardstick, 4 fp32 ulps of the group's largest magnitude); ratio =",
            "gap / bound (rule: <= 1).  'wrong ...': the largest ratio a restatement that is wrong on purpose reaches in the same",
            "check (rule: > 1) -- 'oracle fp32' as in the CPU suite (tests/test_robot_layer.py), 'HIP' on the library's own runs.", ""]
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "robot_layer_parity.txt"), "w") as f:
        f.write("\n".join(head + [ln for key in sorted(REPORT) for ln in REPORT[key]]) + "\n")


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [4, 16])
@pytest.mark.parametrize("check", list(L.CHECKS))
def test_library_within_the_fp32_yardstick(check, lanes):
    _need_gpu()
    runs, lib_runs, idx = {}, {}, list(L.CHECKS).index(check)
    make = lambda n, **kw: _Lib(n, lanes, **kw)
    yard = L.CHECKS[check](_oracle(np.float32), cache=runs)
    got = L.CHECKS[check](make, cache=lib_runs)
    lines, wrong_lines, teeth = [], [], {}
    try:
        L.judge(check, "HIP %2d lanes" % lanes, got, yard, lines)
    finally:
        for w in L.TEETH.get(check, ()):
            wrong_lines.append("%-16s %-14s wrong %-15s ratio %.3g" % (check, "oracle fp32", w, L.worst_ratio(
                L.CHECKS[check](_oracle(np.float32), wrong=w, cache=runs), yard)))
            teeth[w] = L.worst_ratio(L.CHECKS[check](make, wrong=w, cache=lib_runs), yard)
            lines.append("%-16s %-14s wrong %-15s ratio %.3g" % (check, "HIP %2d lanes" % lanes, w, teeth[w]))
        REPORT[(idx, lanes)] = lines
        REPORT[(idx, 99)] = wrong_lines
        _write_report()
    assert all(r > 1.0 for r in teeth.values()), teeth          # on the library too, the check can tell the wrong restatements


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [4, 16])
def test_sensor_modes_and_history_stack(lanes):
    """check 5: what env.reset() / env.step() return is the restatement's selection and stack of the library's 49-float rows"""
    _need_gpu()
    gold = np.load(os.path.join(ROOT, "tests", "golden", "robotlayer.npz"))
    n, rng, views = 8, np.random.default_rng(5), 0
    for row5 in gold["se_mode"]:
        for mode, T, dt in gold["ow_case"]:
            sm = dict(R.sensor_mode_of(row5), RNN=dict(time_steps=int(T), time_interval=int(dt), mode="GRU" if mode else "stack"))
            env = _make(n, ETG=0, solver_iters=4, action_repeat=1, settle_ticks=50, sensor_mode=sm, lanes_per_robot=lanes)
            got, rows = [env.reset()[0].double().cpu().numpy()], [env.obs.double().cpu().numpy()]
            for _ in range(7):
                a = torch.as_tensor(rng.uniform(-0.2, 0.2, (n, 12)), dtype=torch.float32, device="cuda:0")
                got.append(env.step(a, want_info=False)[0].double().cpu().numpy())
                rows.append(env.obs.double().cpu().numpy())
            rows = np.stack(rows)
            assert np.abs(rows[1:] - rows[:-1]).max() > 1e-3            # the readings differ from step to step
            cols = R.select_columns(sm)
            want = R.history_stack(rows[:, :, cols], int(T), int(dt), sm["RNN"]["mode"])
            assert tuple(env.observation_space.shape) == want[0].shape[1:]
            for k in range(8):
                assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (sm, k)
                views += 1
            env.close()
    REPORT[(len(L.CHECKS), lanes)] = ["%-16s %-14s %d views of 5 sensor modes x 4 history settings equal the selection and stack exactly"
                                      % ("modes and stack", "HIP %2d lanes" % lanes, views)]
    _write_report()
