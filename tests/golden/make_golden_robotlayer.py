"""Generate tests/golden/robotlayer.npz by EXECUTING the reference's robot layer.

Run ONCE in the build container (needs /root/reference; never on the GPU box):
    python tests/golden/make_golden_robotlayer.py
Only DATA is written (numeric inputs + expected outputs).  The functions are executed from the
reference tree where they lie: make_golden.py's AST extraction of module-level functions, extended
to the methods inside a ClassDef, which are compiled as plain functions and called with a
types.SimpleNamespace standing in for `self` (no pybullet, no robot object).  No reference source
text is stored; strings (sensor names, dict keys) are stored as the integer codes listed below.

Provenance (paths under /root/reference/QuadrupedalRobots/ETGRL/deployment):
  robots/minitaur.py   MapToMinusPiToPi (:67-83), Minitaur.GetMotorAngles (:753-765), GetMotorVelocities
                       (:778-788), _GetDelayedObservation (:1172-1193), _GetPDObservation (:1195-1199),
                       _GetControlObservation (:1201-1204), _AddSensorNoise (:1206-1211), ProcessAction (:1384-1401)
  robots/a1.py         MAX_MOTOR_ANGLE_CHANGE_PER_STEP (:62), A1._ClipMotorCommands (:440-457)
  envs/EnvWrapper.py   SimpleEnv.__init__ (:29-55), SimpleEnv.get_observation (:60-109),
                       ObservationWrapper.__init__ / get_observation / reset (:196-238)

Arrays (prefix = group):
  dl_hist [100,43]   the observation deque, NEWEST FIRST (appendleft order), time_step dl_dt = 0.002
  dl_lat [n], dl_len [n]  latency (s) and deque length of each case (a shorter deque = the first dl_len rows)
  dl_out [n,43]      _GetDelayedObservation; dl_ctrl [n,43] the same cases through _GetControlObservation
                     (latency 0.006: in IEEE doubles 0.006 / 0.002 rounds to 3.0, so int() gives 3 and the blend weight is 0;
                     a quotient that rounds below -- rows 2 and 3 with all the weight on row 3 -- is the same reading)
  pd_lat [3], pd_q [3,12], pd_qd [3,12]   _GetPDObservation on the full deque
  wrap_in / wrap_out MapToMinusPiToPi
  pa_case [n,4]      ProcessAction cases: (action_repeat, substep, interpolation on, _last_action set);
  pa_action [12], pa_last [12], pa_out [n,12]
  clip_width, clip_angles [12], clip_cmd [n,12], clip_out [n,12]   _ClipMotorCommands (GetMotorAngles() -> clip_angles)
  ma_ctrl [43], ma_angles [12], ma_vel [12]   GetMotorAngles / GetMotorVelocities of a control observation, noise 0
  se_etg_mean / se_etg_std   SimpleEnv.__init__
  se_mode [m,5]      sensor_mode values in the column order (dis, motor, imu, contact, ETG)
  se_obs_dim [m]     SimpleEnv.__init__'s obs_dim.  The reference is NOT self-consistent here: it adds the 12 ETG columns
                     under sensor_mode["contact"] (EnvWrapper.py:47) and 6 columns for imu = 2, whose row has 3.  The rows
                     are what is pinned; se_obs_dim is to be compared only where it equals the row length (se_row_len).
  se_case [c,4]      get_observation cases: (mode index, normal, first_reset, iter)
  se_row [c,49]      the flat row, NaN-padded to 49; se_row_len [c]
  se_keys [c,4]      the sorted key order of the sensor dict, -1 padded, codes: 0 BaseDisplacement, 1 FootContactSensor,
                     2 IMU, 3 MotorAngle, 4 MotorAngleAcc;  se_key_len [c,4] the length of each key's value
  se_motor_q / se_motor_qd / se_dis / se_rpy / se_drpy / se_contact   the duck-typed robot's getter values per case
  se_first_rpy [3], se_etg_data [10,12], se_last_action [12]
  ow_case [k,3]      ObservationWrapper cases: (mode 0 stack / 1 GRU, time_steps, time_interval)
  ow_rows [8,5]      the inner env's readings: reset's, then seven get_observation calls
  ow_out_<k> [8, ...] what reset and the seven calls return
"""
import ast
import collections
import copy
import math
import os
import types

import numpy as np

REF = "/root/reference/QuadrupedalRobots/ETGRL/deployment/"
OUT = os.path.dirname(os.path.abspath(__file__))
KEY_CODE = {"BaseDisplacement": 0, "FootContactSensor": 1, "IMU": 2, "MotorAngle": 3, "MotorAngleAcc": 4}
MODE_KEYS = ("dis", "motor", "imu", "contact", "ETG")


def extract(path, names=(), assigns=(), methods=None, ns=None):
    """execute module-level functions / assignments and, for methods = {class name: method names}, the FunctionDef nodes
    inside those ClassDefs as plain functions named Class_method -> the namespace"""
    tree = ast.parse(open(path).read())
    ns = {"np": np, "math": math, "copy": copy, "collections": collections} if ns is None else ns

    def run(node):
        exec(compile(ast.Module([node], []), path, "exec"), ns)
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name in names:
            run(node)
        if isinstance(node, ast.Assign) and getattr(node.targets[0], "id", "") in assigns:
            run(node)
        if isinstance(node, ast.ClassDef) and methods and node.name in methods:
            for sub in node.body:
                if isinstance(sub, ast.FunctionDef) and sub.name in methods[node.name]:
                    run(sub)
                    ns[node.name + "_" + sub.name] = ns.pop(sub.name)
    return ns


def main():
    rng = np.random.default_rng(20261020)
    out = {}
    mt = extract(REF + "robots/minitaur.py", {"MapToMinusPiToPi"}, ("TWO_PI",),
                 {"Minitaur": {"_GetDelayedObservation", "_GetPDObservation", "_GetControlObservation", "ProcessAction",
                               "GetMotorAngles", "GetMotorVelocities", "_AddSensorNoise"}})
    M = lambda n: mt["Minitaur_" + n]

    # ---- delayed observation ------------------------------------------------------------------
    dt = 0.002
    rows = rng.normal(size=(100, 43))
    rows[:, :12] += np.array([0, 0.9, -1.8] * 4)
    lat = [0.0, -0.003, 0.0005, 0.001, 0.002, 0.003, 0.0045, 0.006, 0.026, 0.0275, 0.04, 0.08, 0.1979, 0.198, 0.3, 0.01, 0.02]
    ln = [100] * 15 + [1, 5]
    dl_out, dl_ctrl = [], []
    for la, n in zip(lat, ln):
        dq = collections.deque(maxlen=100)
        for r in rows[:n][::-1]:
            dq.appendleft(list(r))          # as ReceiveObservation does: newest first
        assert np.array_equal(np.array(dq[0]), rows[0])
        me = types.SimpleNamespace(_observation_history=dq, time_step=dt, _control_latency=la)
        me._GetDelayedObservation = lambda x, me=me: M("_GetDelayedObservation")(me, x)
        dl_out.append(np.asarray(M("_GetDelayedObservation")(me, la), dtype=np.float64))
        dl_ctrl.append(np.asarray(M("_GetControlObservation")(me), dtype=np.float64))
    out.update(dl_hist=rows, dl_dt=np.array(dt), dl_lat=np.array(lat), dl_len=np.array(ln), dl_out=np.array(dl_out),
               dl_ctrl=np.array(dl_ctrl))
    pd_lat = [0.0005, 0.001, 0.002]
    pq, pqd = [], []
    for la in pd_lat:
        dq = collections.deque([list(r) for r in rows], maxlen=100)
        me = types.SimpleNamespace(_observation_history=dq, time_step=dt, _pd_latency=la, num_motors=12)
        me._GetDelayedObservation = lambda x, me=me: M("_GetDelayedObservation")(me, x)
        q, qd = M("_GetPDObservation")(me)
        pq.append(q)
        pqd.append(qd)
    out.update(pd_lat=np.array(pd_lat), pd_q=np.array(pq), pd_qd=np.array(pqd))

    # ---- wrap -----------------------------------------------------------------------------------
    pi = math.pi
    w_in = [pi, -pi, pi + 1e-6, pi - 1e-6, -pi + 1e-6, -pi - 1e-6, 2 * pi, -2 * pi, 3 * pi, -3 * pi, 0.0, 7.0, -7.0, 100.0]
    out.update(wrap_in=np.array(w_in), wrap_out=np.array(mt["MapToMinusPiToPi"](list(w_in)), dtype=np.float64))

    # ---- ProcessAction ----------------------------------------------------------------------------
    action = np.array([0, 0.9, -1.8] * 4) + rng.uniform(-0.3, 0.3, 12)
    last = np.array([0, 0.9, -1.8] * 4) + rng.uniform(-0.3, 0.3, 12)
    pa_case, pa_out = [], []
    for R in (1, 5, 13):
        for interp in (0, 1):
            for has_last in (0, 1):
                for i in range(R):
                    me = types.SimpleNamespace(_enable_action_interpolation=bool(interp), _action_repeat=R,
                                               _last_action=last.copy() if has_last else None)
                    pa_case.append((R, i, interp, has_last))
                    pa_out.append(np.array(M("ProcessAction")(me, action.copy(), i), dtype=np.float64))
    out.update(pa_case=np.array(pa_case), pa_action=action, pa_last=last, pa_out=np.array(pa_out))

    # ---- _ClipMotorCommands ------------------------------------------------------------------------
    a1 = extract(REF + "robots/a1.py", (), ("MAX_MOTOR_ANGLE_CHANGE_PER_STEP",), {"A1": {"_ClipMotorCommands"}})
    width = float(a1["MAX_MOTOR_ANGLE_CHANGE_PER_STEP"])
    angles = np.array([0, 0.9, -1.8] * 4) + rng.uniform(-0.2, 0.2, 12)
    offs = np.stack([rng.uniform(-0.19, 0.19, 12), np.full(12, width), np.full(12, -width), np.full(12, width + 0.05),
                     np.full(12, -width - 0.05), rng.uniform(-0.6, 0.6, 12), rng.uniform(0.2, 1.0, 12) * np.array([1, -1] * 6)])
    me = types.SimpleNamespace(GetMotorAngles=lambda: angles.copy())
    cmd = angles + offs
    out.update(clip_width=np.array(width), clip_angles=angles, clip_cmd=cmd,
               clip_out=np.array([a1["A1__ClipMotorCommands"](me, c.copy()) for c in cmd], dtype=np.float64))

    # ---- GetMotorAngles / GetMotorVelocities on a control observation, noise 0 -----------------------
    ctrl = dl_ctrl[9].copy()
    ctrl[:12] += np.array([2 * pi, -2 * pi, 0, pi, -pi, 4 * pi, 0, 0, 3.0, -3.0, 0, 0])
    me = types.SimpleNamespace(_control_observation=ctrl, num_motors=12, _observation_noise_stdev=(0.0,) * 5)
    me._AddSensorNoise = lambda v, s, me=me: M("_AddSensorNoise")(me, v, s)
    out.update(ma_ctrl=ctrl, ma_angles=np.array(M("GetMotorAngles")(me), dtype=np.float64),
               ma_vel=np.array(M("GetMotorVelocities")(me), dtype=np.float64))

    # ---- SimpleEnv ---------------------------------------------------------------------------------
    ew = extract(REF + "envs/EnvWrapper.py", methods={"SimpleEnv": {"__init__", "get_observation"},
                                                      "ObservationWrapper": {"__init__", "get_observation", "reset"}},
                 ns={"np": np, "collections": collections, "copy": copy.copy})
    modes = [dict(dis=1, motor=1, imu=1, contact=1, ETG=1), dict(dis=0, motor=1, imu=1, contact=1, ETG=1),
             dict(dis=1, motor=1, imu=2, contact=1, ETG=1), dict(dis=1, motor=2, imu=1, contact=1, ETG=1),
             dict(dis=1, motor=1, imu=1, contact=0, ETG=1)]
    etg_data = rng.normal(size=(10, 12)) * 0.1
    first_rpy = rng.normal(size=3) * 0.05
    iters = (0, 1, 5, 9)
    cases, rws, rlen, keys, klen, getters, obs_dim = [], [], [], [], [], {k: [] for k in ("motor_q", "motor_qd", "dis", "rpy", "drpy", "contact")}, []
    c = 0
    for mi, sm in enumerate(modes):
        me = types.SimpleNamespace()
        ew["SimpleEnv___init__"](me, None, dict(sm), True, etg_data)
        obs_dim.append(me.obs_dim)
        if mi == 0:
            out.update(se_etg_mean=np.array(me.ETG_mean), se_etg_std=np.array(me.ETG_std), se_last_action=np.array(me.last_action, dtype=np.float64))
        for normal in (1, 0):
            for first in (1, 0):
                g = dict(motor_q=np.array([0, 0.9, -1.8] * 4) + rng.normal(size=12) * 0.2, motor_qd=rng.normal(size=12) * 3,
                         dis=rng.normal(size=3) * 0.3, rpy=rng.normal(size=3) * 0.1, drpy=rng.normal(size=3),
                         contact=rng.integers(0, 2, 4).astype(np.float64))
                robot = types.SimpleNamespace(
                    ReceiveObservation=lambda: None, GetMotorAngles=lambda g=g: g["motor_q"].copy(),
                    GetMotorVelocities=lambda g=g: g["motor_qd"].copy(), GetBaseVelocity=lambda g=g: g["dis"].copy(),
                    GetTrueBaseRollPitchYaw=lambda g=g: g["rpy"].copy(), GetTrueBaseRollPitchYawRate=lambda g=g: g["drpy"].copy(),
                    GetFootContacts=lambda g=g: g["contact"].copy())
                me = types.SimpleNamespace()
                ew["SimpleEnv___init__"](me, robot, dict(sm), bool(normal), etg_data)
                me.first_reset, me.iter = bool(first), iters[c % 4]
                if not first:
                    me.first_rpy = first_rpy.copy()
                flat, od = ew["SimpleEnv_get_observation"](me)
                ks = [k for k in od.keys() if k != "real_action"]
                assert ks == sorted(ks) and me.first_reset is False
                cases.append((mi, normal, first, me.iter))
                rws.append(np.concatenate([flat, np.full(49 - len(flat), np.nan)]))
                rlen.append(len(flat))
                keys.append([KEY_CODE[k] for k in ks] + [-1] * (4 - len(ks)))
                klen.append([np.asarray(od[k]).size for k in ks] + [0] * (4 - len(ks)))
                for k in getters:
                    getters[k].append(g[k])
                c += 1
    out.update(se_mode=np.array([[sm[k] for k in MODE_KEYS] for sm in modes]), se_obs_dim=np.array(obs_dim),
               se_case=np.array(cases), se_row=np.array(rws), se_row_len=np.array(rlen), se_keys=np.array(keys),
               se_key_len=np.array(klen), se_first_rpy=first_rpy, se_etg_data=etg_data,
               **{"se_" + k: np.array(v) for k, v in getters.items()})

    # ---- ObservationWrapper ---------------------------------------------------------------------------
    ow_rows = rng.normal(size=(8, 5))
    ow_case = []
    for k, (mode, T, dtI) in enumerate((m, T, d) for m in ("stack", "GRU") for (T, d) in ((2, 2), (3, 1))):
        it = iter(ow_rows)
        inner = types.SimpleNamespace(get_obs_dim=lambda: 5, reset=lambda **kw: (next(it).copy(), {}),
                                      get_observation=lambda: (next(it).copy(), {}))
        me = types.SimpleNamespace()
        ew["ObservationWrapper___init__"](me, inner, None, {"RNN": {"time_steps": T, "time_interval": dtI, "mode": mode}})
        res = [ew["ObservationWrapper_reset"](me)[0]] + [ew["ObservationWrapper_get_observation"](me)[0] for _ in range(7)]
        assert me.obs_dim == (5 * (T + 1) if mode == "stack" else 5)
        ow_case.append((0 if mode == "stack" else 1, T, dtI))
        out["ow_out_%d" % k] = np.array(res, dtype=np.float64)
    out.update(ow_case=np.array(ow_case), ow_rows=ow_rows)

    for k, v in out.items():
        assert np.asarray(v).dtype.kind in "fi", (k, np.asarray(v).dtype)
    path = os.path.join(OUT, "robotlayer.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", len(out), "arrays")


if __name__ == "__main__":
    main()
