"""The robot layer between the physics tick and the learner, restated in plain numpy fp64 -- TEST INFRASTRUCTURE ONLY.

Written from the contract in this project's words, vectorised over robots, and pinned to the EXECUTED reference by
tests/golden/robotlayer.npz (tests/test_robot_layer.py, to 1e-12).  The live checks of tests/robot_layer_checks.py
apply it to a simulator's own per-tick states.

The contract
  * Every physics tick appends one true-observation row to a per-robot history, newest first.
  * The delayed reading at latency L (seconds, tick length dt): the newest row if L <= 0 or the history holds one row;
    otherwise with k = int(L / dt): the OLDEST row if k + 1 reaches the history's length, else the blend
    (1 - a) * row[k] + a * row[k + 1] with a = (L - k dt) / dt -- weight (1 - a) on the NEWER of the two rows.
  * Motor angles are read from the delayed reading and wrapped into [-pi, pi): fmod by 2 pi (sign of the argument), then
    values >= pi lose 2 pi and values < -pi gain 2 pi (so -pi itself stays).  Velocities are read unwrapped.
  * With action interpolation on, sub-step i (0-based) of a control step of R ticks commands
    last + (i + 1) / R * (action - last); without it, or while no earlier action exists (the first step after a
    reset), the action itself.
  * The motor-command clip keeps a position command within +-width (0.2 rad) of the wrapped DELAYED motor angles.
  * The observation row, in this order: base displacement rate (3), foot contacts (4), IMU (rpy - first rpy, then rpy
    rate: 6; imu = 2 keeps the rate alone: 3), motors (angles then velocities: 24; motor = 2 keeps the angles: 12),
    ETG output (12).  Normalised: angles (a - pose) / 0.1, velocities unchanged, rpy / 0.1, rpy rate / 0.5,
    ETG (e - mean) / std; displacement and contacts are passed through.
  * The history stack: `time_steps` older views followed by the current one.  A buffer of time_steps * time_interval
    views, oldest first and all zero after a reset, is read at positions t * time_interval BEFORE the current view is
    shifted in at its end; "stack" flattens the views, "GRU" keeps them as a sequence.

OWN DEFINITIONS -- what the reference takes from pybullet and this project defines itself; nothing below
the line is pinned by the fixture:
  * true_observation_row: the row of a 37-float state (position 0:3, quaternion xyzw 3:7, world linear 7:10 and angular
    10:13 velocity, joint angles 13:25, joint velocities 25:37) = angles, velocities, quaternion, angular velocity in the
    base frame (R^T w);
  * rpy_of_quat: roll / pitch / yaw of a (not necessarily unit) quaternion, ZYX convention;
  * base_displacement_rate: (position - position at the last control step) / control period when normalised, the plain
    difference otherwise;
  * foot contacts and the ETG output are inputs here: contact detection and the gait generator are the simulator's.
"""
import numpy as np

POSE = np.array([0.0, 0.9, -1.8] * 4)
ANGLE_SCALE, RPY_SCALE, RATE_SCALE = 0.1, 0.1, 0.5
CLIP_WIDTH = 0.2
# variants of the restatement that are WRONG on purpose (tests/test_robot_layer.py "teeth"): every live check must reject them
WRONG = ("blend_swapped", "slots_shifted", "lerp_i", "lerp_first", "clip_undelayed", "clip_025")


def delayed_reading(hist, latency, dt, wrong=None):
    """hist [N, L, C] (or [L, C]) newest first, latency [N] (or scalar) seconds -> [N, C] (or [C])"""
    h = np.asarray(hist, dtype=np.float64)
    single = h.ndim == 2
    if single:
        h = h[None]
    N, L, _ = h.shape
    lat = np.broadcast_to(np.asarray(latency, dtype=np.float64), (N,))
    k = np.floor(np.maximum(lat, 0.0) / dt).astype(np.int64)
    newest = (lat <= 0) | (L == 1)
    oldest = ~newest & (k + 1 >= L)
    kk = np.where(newest | oldest, 0, k)
    a = (lat - kk * dt) / dt
    i0, i1 = kk, np.minimum(kk + 1, L - 1)
    if wrong == "slots_shifted":
        i0, i1 = np.maximum(kk - 1, 0), kk
    w0, w1 = 1.0 - a, a
    if wrong == "blend_swapped":
        w0, w1 = a, 1.0 - a
    r = np.arange(N)
    out = w0[:, None] * h[r, i0] + w1[:, None] * h[r, i1]
    out = np.where(newest[:, None], h[:, 0], np.where(oldest[:, None], h[:, L - 1], out))
    return out[0] if single else out


def wrap_to_pi(a):
    a = np.fmod(np.asarray(a, dtype=np.float64), 2 * np.pi)
    return np.where(a >= np.pi, a - 2 * np.pi, np.where(a < -np.pi, a + 2 * np.pi, a))


def motor_angles(reading):
    return wrap_to_pi(np.asarray(reading)[..., 0:12])


def motor_velocities(reading):
    return np.asarray(reading, dtype=np.float64)[..., 12:24]


def substep_command(action, last, i, R, interp, wrong=None):
    """the command of sub-step i of R; last: the previous control step's action, None on the first step after a reset"""
    action = np.asarray(action, dtype=np.float64)
    if wrong == "lerp_first" and last is None:
        last = np.zeros_like(action)        # (as a residual on the pose: the command a reset leaves standing)
    if not interp or last is None:
        return action
    f = float(i if wrong == "lerp_i" else i + 1) / R
    return last + f * (action - last)


def clip_command(cmd, delayed_angles, width=CLIP_WIDTH):
    return np.clip(np.asarray(cmd, dtype=np.float64), delayed_angles - width, delayed_angles + width)


def sensor_mode_of(row5):
    return dict(zip(("dis", "motor", "imu", "contact", "ETG"), (int(v) for v in row5)))


def select_columns(sensor_mode):
    """columns of the full 49-float row that a sensor_mode keeps, in row order"""
    sm = dict(dis=1, motor=1, imu=1, contact=1, ETG=1)
    sm.update({k: v for k, v in (sensor_mode or {}).items() if k in sm})
    keep = np.zeros(49, dtype=bool)
    keep[0:3] = bool(sm["dis"])
    keep[3:7] = bool(sm["contact"])
    keep[7:10] = sm["imu"] == 1
    keep[10:13] = sm["imu"] in (1, 2)
    keep[13:25] = sm["motor"] in (1, 2)
    keep[25:37] = sm["motor"] == 1
    keep[37:49] = bool(sm["ETG"])
    return [int(c) for c in np.nonzero(keep)[0]]


def observation_row(angles, velocities, displacement, rpy, rpy_rate, contacts, etg, first_rpy, normal, etg_mean, etg_std,
                    sensor_mode=None):
    """the observation of [N] robots from their readings ([N, k] each; first_rpy None: this is the first reading after a
    reset, whose rpy becomes the offset) -> (rows [N, D], first_rpy)"""
    f = lambda x: np.atleast_2d(np.asarray(x, dtype=np.float64))
    angles, velocities, displacement, rpy, rpy_rate, contacts, etg = map(f, (angles, velocities, displacement, rpy, rpy_rate, contacts, etg))
    if first_rpy is None:
        first_rpy = rpy.copy()
    rel = rpy - first_rpy
    if normal:
        angles = (angles - POSE) / ANGLE_SCALE
        rel, rpy_rate = rel / RPY_SCALE, rpy_rate / RATE_SCALE
        etg = (etg - etg_mean) / etg_std
    full = np.concatenate([displacement, contacts, rel, rpy_rate, angles, velocities, etg], axis=1)
    return full[:, select_columns(sensor_mode)], first_rpy


def history_stack(views, time_steps, time_interval, mode="stack"):
    """views [K, N, D]: the view at the reset, then at every later reading -> list of K outputs, [N, (T+1) D] ("stack") or
    [N, T+1, D] ("GRU")"""
    views = np.asarray(views, dtype=np.float64)
    K, N, D = views.shape
    buf = np.zeros((time_steps * time_interval, N, D))
    outs = []
    for k in range(K):
        seq = np.stack([buf[t * time_interval] for t in range(time_steps)] + [views[k]], axis=1)
        buf = np.concatenate([buf[1:], views[k][None]], axis=0) if k else np.concatenate([buf[:-1], views[k][None]], axis=0)
        outs.append(seq.reshape(N, -1) if mode == "stack" else seq)
    return outs


# ---------------------------------------------------------------- own definitions (see the module docstring)
def _rot(quat):
    q = np.asarray(quat, dtype=np.float64)
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    s = 2.0 / (x * x + y * y + z * z + w * w)
    R = np.empty(q.shape[:-1] + (3, 3))
    R[..., 0, 0] = 1 - s * (y * y + z * z); R[..., 0, 1] = s * (x * y - z * w); R[..., 0, 2] = s * (x * z + y * w)
    R[..., 1, 0] = s * (x * y + z * w); R[..., 1, 1] = 1 - s * (x * x + z * z); R[..., 1, 2] = s * (y * z - x * w)
    R[..., 2, 0] = s * (x * z - y * w); R[..., 2, 1] = s * (y * z + x * w); R[..., 2, 2] = 1 - s * (x * x + y * y)
    return R


def rpy_of_quat(quat):
    R = _rot(quat)
    return np.stack([np.arctan2(R[..., 2, 1], R[..., 2, 2]), np.arcsin(np.clip(-R[..., 2, 0], -1, 1)),
                     np.arctan2(R[..., 1, 0], R[..., 0, 0])], axis=-1)


def true_observation_row(state):
    """[..., 37] states -> [..., 31] rows: angles 0:12, velocities 12:24, quaternion 24:28, base-frame angular velocity 28:31"""
    st = np.asarray(state, dtype=np.float64)
    wb = np.einsum("...ji,...j->...i", _rot(st[..., 3:7]), st[..., 10:13])
    return np.concatenate([st[..., 13:25], st[..., 25:37], st[..., 3:7], wb], axis=-1)


def base_displacement_rate(pos, last_pos, control_dt, normal):
    d = np.asarray(pos, dtype=np.float64) - np.asarray(last_pos, dtype=np.float64)
    return d / control_dt if normal else d
