"""The robot layer -- delayed observation, angle wrap, action interpolation, motor-command clip, the 49-float row, the history
stack -- pinned to the EXECUTED reference (tests/golden/robotlayer.npz, made by tests/golden/make_golden_robotlayer.py).

Three links: (1) the plain fp64 restatement tests/robot_layer_ref.py equals the fixture to 1e-12; (2) the project's constants
equal the fixture's; (3) every simulator backend agrees with the restatement applied to its own per-tick states
(tests/robot_layer_checks.py has the checks and the bound rule), and the same checks reject six restatements that are wrong on
purpose.  tests/test_gpu_robot_layer.py runs (3) on the HIP library.

Measured here (bound = max(4 x fp32-oracle gap, 4 fp32 ulps); profiles/robot_layer_parity.txt has the library's table): the fp64
oracle agrees to 4e-13 (bound 1e-9); the emulation's worst gap / bound is 0.69 (interpolation, 16 lanes, linear velocity); the
clip binds on 66.7 % of the (tick, joint) pairs; the wrong restatements reach 2.4e4 (i / R) to 5.9e5 (blend, slots) times
their bound on the fp32 oracle and on the 4-lane emulation, with the inputs as first chosen -- none had to be sharpened."""
import ast
import functools
import os
import types

import numpy as np
import pytest

from paddlerobotics_amd import a1_model as A
from paddlerobotics_amd import env as E
from tests import robot_layer_checks as L
from tests import robot_layer_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "robotlayer.npz"))


# ================================================================================ 1: the restatement equals the fixture
def test_fixture_holds_numbers_only(gold):
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "robotlayer.npz")) < 200 * 1024
    for k in gold.files:
        assert gold[k].dtype.kind in "fi", k


def test_delayed_reading_equals_reference(gold):
    dt = float(gold["dl_dt"])
    for lat, n, out, ctrl in zip(gold["dl_lat"], gold["dl_len"], gold["dl_out"], gold["dl_ctrl"]):
        mine = R.delayed_reading(gold["dl_hist"][:n], lat, dt)
        assert np.abs(mine - out).max() <= TOL, (lat, n)
        assert np.abs(mine - ctrl).max() <= TOL, (lat, n)
    # the cases of one history length, vectorised over robots as the live checks use it
    full = gold["dl_len"] == 100
    hist = np.broadcast_to(gold["dl_hist"], (int(full.sum()), 100, 43))
    assert np.abs(R.delayed_reading(hist, gold["dl_lat"][full], dt) - gold["dl_out"][full]).max() <= TOL
    # what the cases are there for
    h = gold["dl_hist"]
    row = dict(zip(np.round(gold["dl_lat"][full], 6), gold["dl_out"][full]))
    assert np.array_equal(row[0.0], h[0]) and np.array_equal(row[-0.003], h[0])
    # 0.006 / 0.002: whichever way the quotient rounds (rows 2 and 3 with all the weight on row 3, or row 3 outright), row 3
    assert np.abs(row[0.006] - h[3]).max() < 1e-12 and np.abs(row[0.002] - h[1]).max() < 1e-12
    assert np.abs(row[0.0045] - (0.75 * h[2] + 0.25 * h[3])).max() < 1e-12      # the weight 1 - a lies on the NEWER row
    assert np.array_equal(row[0.3], h[99]) and np.abs(row[0.1979] - (0.05 * h[98] + 0.95 * h[99])).max() < 1e-9
    assert np.array_equal(gold["dl_out"][15], h[0]) and np.array_equal(gold["dl_out"][16], h[4])


def test_pd_reading_equals_reference(gold):
    for lat, q, qd in zip(gold["pd_lat"], gold["pd_q"], gold["pd_qd"]):
        d = R.delayed_reading(gold["dl_hist"], lat, float(gold["dl_dt"]))
        assert np.abs(d[0:12] - q).max() <= TOL and np.abs(d[12:24] - qd).max() <= TOL


def test_wrap_equals_reference(gold):
    assert np.abs(R.wrap_to_pi(gold["wrap_in"]) - gold["wrap_out"]).max() <= TOL
    assert np.abs(R.motor_angles(gold["ma_ctrl"]) - gold["ma_angles"]).max() <= TOL
    assert np.array_equal(R.motor_velocities(gold["ma_ctrl"]), gold["ma_vel"])
    assert gold["wrap_out"].min() >= -np.pi and gold["wrap_out"].max() < np.pi and np.abs(gold["ma_ctrl"][:12]).max() > 2 * np.pi


def test_substep_command_equals_reference(gold):
    assert {tuple(c[[0, 2, 3]]) for c in gold["pa_case"]} == {(r, i, l) for r in (1, 5, 13) for i in (0, 1) for l in (0, 1)}
    for (rep, i, interp, has_last), out in zip(gold["pa_case"], gold["pa_out"]):
        mine = R.substep_command(gold["pa_action"], gold["pa_last"] if has_last else None, int(i), int(rep), bool(interp))
        assert np.abs(mine - out).max() <= TOL, (rep, i, interp, has_last)


def test_clip_equals_reference(gold):
    assert float(gold["clip_width"]) == R.CLIP_WIDTH
    mine = R.clip_command(gold["clip_cmd"], gold["clip_angles"], float(gold["clip_width"]))
    assert np.abs(mine - gold["clip_out"]).max() <= TOL
    moved = mine != gold["clip_cmd"]
    assert not moved[0].any() and moved[3:5].all() and moved[5].any() and not moved[5].all()


def _case_row(gold, c):
    mi, normal, first, it = (int(v) for v in gold["se_case"][c])
    sm = R.sensor_mode_of(gold["se_mode"][mi])
    row, _ = R.observation_row(gold["se_motor_q"][c], gold["se_motor_qd"][c], gold["se_dis"][c], gold["se_rpy"][c],
                               gold["se_drpy"][c], gold["se_contact"][c], gold["se_etg_data"][it],
                               None if first else gold["se_first_rpy"], normal, gold["se_etg_mean"], gold["se_etg_std"], sm)
    return sm, row[0]


def test_observation_row_equals_reference(gold):
    assert len(gold["se_case"]) == 20 and len({tuple(c[:3]) for c in gold["se_case"]}) == 20
    key_cols = {0: 3, 1: 4, 3: 12, 4: 24}          # BaseDisplacement, FootContactSensor, MotorAngle, MotorAngleAcc
    for c in range(len(gold["se_case"])):
        sm, row = _case_row(gold, c)
        n = int(gold["se_row_len"][c])
        assert row.shape == (n,) and np.isnan(gold["se_row"][c][n:]).all()
        assert np.abs(row - gold["se_row"][c][:n]).max() <= TOL, (c, sm)
        # the order: the reference's sorted sensor names are this project's row order, the ETG columns last
        keys = [int(k) for k in gold["se_keys"][c] if k >= 0]
        assert keys == sorted(keys)
        lens = [int(v) for v in gold["se_key_len"][c][:len(keys)]]
        assert all(lens[j] == key_cols[k] for j, k in enumerate(keys) if k in key_cols)
        assert sum(lens) + 12 * sm["ETG"] == n == len(R.select_columns(sm))


def test_history_stack_equals_reference(gold):
    views = gold["ow_rows"][:, None, :]
    for k, (mode, T, dt) in enumerate(gold["ow_case"]):
        outs = R.history_stack(views, int(T), int(dt), "GRU" if mode else "stack")
        want = gold["ow_out_%d" % k]
        for a, b in zip(outs, want):
            assert a[0].shape == b.shape and np.array_equal(a[0], b)


# ================================================================================ 2: the project's constants
def test_project_constants_equal_the_fixture(gold):
    m = A.default_model()
    assert np.array_equal(np.array(m.etg_mean), gold["se_etg_mean"]) and np.array_equal(A.ETG_MEAN, gold["se_etg_mean"])
    assert np.array_equal(np.array(m.etg_std), gold["se_etg_std"]) and np.array_equal(A.ETG_STD, gold["se_etg_std"])
    assert np.array_equal(np.array(m.pose_ori), gold["se_last_action"]) and np.array_equal(R.POSE, gold["se_last_action"])
    # offsets and scales, read off the fixture's normalised rows of the default sensor_mode
    for c in np.nonzero((gold["se_case"][:, 0] == 0) & (gold["se_case"][:, 1] == 1) & (gold["se_case"][:, 2] == 0))[0]:
        row = gold["se_row"][c]
        assert np.allclose((gold["se_motor_q"][c] - np.array(m.pose_ori)) / row[13:25], R.ANGLE_SCALE, rtol=1e-12, atol=0)
        assert np.allclose(gold["se_motor_qd"][c] / row[25:37], 1.0, rtol=1e-12, atol=0)
        assert np.allclose((gold["se_rpy"][c] - gold["se_first_rpy"]) / row[7:10], R.RPY_SCALE, rtol=1e-12, atol=0)
        assert np.allclose(gold["se_drpy"][c] / row[10:13], R.RATE_SCALE, rtol=1e-12, atol=0)
        assert np.array_equal(row[0:3], gold["se_dis"][c]) and np.array_equal(row[3:7], gold["se_contact"][c])
    # the clip width make_env(enable_clip_motor_commands=True) hands to the library, read from the call in env.py
    tree = ast.parse(open(E.__file__).read())
    kws = [k.value for n in ast.walk(tree) if isinstance(n, ast.Call) for k in n.keywords if k.arg == "clip_motor_commands"]
    assert len(kws) == 1 and isinstance(kws[0], ast.IfExp)
    assert kws[0].body.value == float(gold["clip_width"]) and kws[0].orelse.value == 0.0
    assert A.default_config(1, clip_motor_commands=kws[0].body.value).clip_motor_commands == float(gold["clip_width"])


def test_sensor_columns_equal_the_fixture(gold):
    for mi, row5 in enumerate(gold["se_mode"]):
        sm = R.sensor_mode_of(row5)
        cols = E.sensor_columns(sm)
        assert cols == R.select_columns(sm)
        for c in np.nonzero(gold["se_case"][:, 0] == mi)[0]:
            full = dict(sm, dis=1, motor=1, imu=1, contact=1, ETG=1)
            _, normal, first, it = (int(v) for v in gold["se_case"][c])
            row49, _ = R.observation_row(gold["se_motor_q"][c], gold["se_motor_qd"][c], gold["se_dis"][c], gold["se_rpy"][c],
                                         gold["se_drpy"][c], gold["se_contact"][c], gold["se_etg_data"][it],
                                         None if first else gold["se_first_rpy"], normal, gold["se_etg_mean"],
                                         gold["se_etg_std"], full)
            n = int(gold["se_row_len"][c])
            assert len(cols) == n and np.abs(row49[0][cols] - gold["se_row"][c][:n]).max() <= TOL
        # obs_dim of the reference's __init__ only where it is consistent with the row it builds (see the generator's docstring)
        if gold["se_obs_dim"][mi] == gold["se_row_len"][gold["se_case"][:, 0] == mi][0]:
            assert len(cols) == gold["se_obs_dim"][mi]
    assert [int(gold["se_obs_dim"][i] == gold["se_row_len"][4 * i]) for i in range(5)] == [1, 1, 0, 1, 0]


# ================================================================================ 3: live checks
SETTLE = 500     # ticks of the reset's settle: the default


def _oracle(dtype):
    from oracle.oracle import OracleSim

    def make(n, action_repeat=1, interp=False, clip=False, joint_limits=True):
        return OracleSim(A.default_config(n, solver_iters=4, enable_etg=0, settle_ticks=SETTLE, action_repeat=action_repeat, enable_action_interp=interp,
                                          clip_motor_commands=R.CLIP_WIDTH if clip else 0.0, joint_limits=joint_limits), dtype=dtype)
    return make


def _emu(lanes):
    from tests.emu.emu import EmuSim

    def make(n, action_repeat=1, interp=False, clip=False, joint_limits=True):
        return EmuSim(A.default_config(n, solver_iters=4, enable_etg=0, settle_ticks=SETTLE, action_repeat=action_repeat, enable_action_interp=interp,
                                       clip_motor_commands=R.CLIP_WIDTH if clip else 0.0, joint_limits=joint_limits), lanes=lanes)
    return make


BACKENDS = {"oracle fp64": lambda: _oracle(np.float64), "oracle fp32": lambda: _oracle(np.float32),
            "emulation 4": lambda: _emu(4), "emulation 16": lambda: _emu(16)}


_RUNS = {b: {} for b in BACKENDS}      # per backend: the runs that do not depend on the restatement's variant


@functools.lru_cache(maxsize=None)
def result(check, backend, wrong=None):
    return L.CHECKS[check](BACKENDS[backend](), wrong=wrong, cache=_RUNS[backend])


@pytest.mark.parametrize("check", list(L.CHECKS))
def test_fp64_oracle_agrees_exactly(check):
    for g, (gap, _) in result(check, "oracle fp64").items():
        print("[robot layer] %-16s oracle fp64    %-17s gap %.3e" % (check, g, gap))
        assert gap <= L.FP64_BOUND, (check, g, gap)


@pytest.mark.parametrize("backend", ["oracle fp32", "emulation 4", "emulation 16"])
@pytest.mark.parametrize("check", list(L.CHECKS))
def test_backend_within_the_fp32_yardstick(check, backend):
    L.judge(check, backend, result(check, backend), result(check, "oracle fp32"))


def test_clip_binds_on_a_quarter_of_the_pairs():
    _, frac = L.check_clip(BACKENDS["oracle fp64"](), want_bind=True)
    print("[robot layer] clip binds on %.1f %% of the (tick, joint) pairs" % (100 * frac))
    assert frac >= 0.25


@pytest.mark.parametrize("backend", ["oracle fp32", "emulation 4"])
@pytest.mark.parametrize("check,wrong", [(c, w) for c, ws in L.TEETH.items() for w in ws])
def test_wrong_restatement_is_rejected(check, wrong, backend):
    ratio = L.worst_ratio(result(check, backend, wrong), result(check, "oracle fp32"))
    print("[robot layer] %-16s %-14s wrong restatement %-15s reaches %.3g x its bound" % (check, backend, wrong, ratio))
    assert ratio > 1.0, (check, wrong, backend, ratio)


def test_fp64_oracle_rejects_every_wrong_restatement():
    for check, ws in L.TEETH.items():
        for w in ws:
            assert max(g for g, _ in result(check, "oracle fp64", w).values()) > 1e3 * L.FP64_BOUND, (check, w)


# -------------------------------------------------------------------------------- 5: sensor modes and the history stack
def _view_stub(sensor_mode, n):
    """BatchedQuadrupedEnv's observation view (column selection + history stack) on host tensors, without a device"""
    import torch
    rnn = sensor_mode.get("RNN") or {}
    cols = E.sensor_columns(sensor_mode)
    s = types.SimpleNamespace(num_envs=n, device=torch.device("cpu"), obs=torch.zeros(n, A.OBS_DIM, dtype=torch.float64), extra=None,
                              _cols=cols, _col_idx=None if len(cols) == A.OBS_DIM else torch.tensor(cols), _xcol_idx=None,
                              _hist_T=int(rnn.get("time_steps", 0)), _hist_dt=int(rnn.get("time_interval", 1)),
                              _hist_mode=rnn.get("mode", "stack"), _hist=None, _hist_head=0, _last_seq=None)
    s._row_view = lambda rows, extra: E.BatchedQuadrupedEnv._row_view(s, rows, extra)
    s.view = lambda first=False: E.BatchedQuadrupedEnv._obs_view(s, first=first)
    return s


def test_env_view_equals_selection_and_stack(gold):
    import torch
    rng = np.random.default_rng(5)
    n = 3
    rows = rng.normal(size=(8, n, A.OBS_DIM))
    for row5 in gold["se_mode"]:
        for mode, T, dt in gold["ow_case"]:
            sm = dict(R.sensor_mode_of(row5), RNN=dict(time_steps=int(T), time_interval=int(dt), mode="GRU" if mode else "stack"))
            s = _view_stub(sm, n)
            want = R.history_stack(rows[:, :, R.select_columns(sm)], int(T), int(dt), sm["RNN"]["mode"])
            for k in range(8):
                s.obs = torch.as_tensor(rows[k]).float()
                got = s.view(first=(k == 0)).double().numpy()
                assert got.shape == want[k].shape and np.array_equal(got, want[k].astype(np.float32).astype(np.float64)), (sm, k)
    # and on the reference's own trace: the wrapper's 5-column readings through the env's stack
    for k, (mode, T, dt) in enumerate(gold["ow_case"]):
        s = _view_stub(dict(RNN=dict(time_steps=int(T), time_interval=int(dt), mode="GRU" if mode else "stack")), 1)
        s._row_view = lambda r, extra: r
        for j in range(8):
            s.obs = torch.as_tensor(gold["ow_rows"][j][None]).float()
            assert np.array_equal(s.view(first=(j == 0))[0].numpy(), gold["ow_out_%d" % k][j].astype(np.float32)), (k, j)
