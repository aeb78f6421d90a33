"""Camera matrices for env.render() and SingleRobotEnv.getCameraImage() (include/etgsim_render.h).

pybullet's conventions: 16 floats, column-major; compute_view_matrix is gluLookAt (pybullet.computeViewMatrix),
compute_projection_matrix_fov is gluPerspective (pybullet.computeProjectionMatrixFOV), and
compute_view_matrix_from_yaw_pitch_roll places the eye as Bullet's computeViewMatrixFromYawPitchRoll does (yaw about the up
axis, a negative pitch looks down; Bullet ignores `roll`, and so does this).  Every helper is batched over leading
dimensions: torch tensors in give float32 tensors on their device, anything else float32 numpy arrays [..., 16].

The follow camera (FOLLOW_*) is this repository's choice; rlschool's camera is absent from the reference."""
import math

import numpy as np
import torch

FOLLOW_DISTANCE = 1.2     # m from the robot's base position
FOLLOW_YAW = 225.0        # deg: behind and to the left of a robot walking along +x, on the side the light comes from
FOLLOW_PITCH = -30.0      # deg: looking down
FOLLOW_FOV = 60.0         # deg, vertical
FOLLOW_NEAR, FOLLOW_FAR = 0.01, 100.0


def _args(*xs):
    """-> (float64 tensors on one device, a function that returns a result in the callers' type)"""
    dev = next((x.device for x in xs if torch.is_tensor(x)), None)
    ts = [x.to(dtype=torch.float64, device=dev) if torch.is_tensor(x) else
          torch.as_tensor(np.asarray(x, dtype=np.float64), device=dev) for x in xs]
    back = (lambda y: y.to(torch.float32)) if dev is not None else (lambda y: y.to(torch.float32).numpy())
    return ts, back


def _view(e, t, u):
    e, t, u = torch.broadcast_tensors(e, t, u)
    f = t - e
    f = f / f.norm(dim=-1, keepdim=True)
    s = torch.linalg.cross(f, u, dim=-1)
    s = s / s.norm(dim=-1, keepdim=True)
    v = torch.linalg.cross(s, f, dim=-1)
    z, one = torch.zeros_like(f[..., 0]), torch.ones_like(f[..., 0])
    return torch.stack([s[..., 0], v[..., 0], -f[..., 0], z, s[..., 1], v[..., 1], -f[..., 1], z,
                        s[..., 2], v[..., 2], -f[..., 2], z, -(s * e).sum(-1), -(v * e).sum(-1), (f * e).sum(-1), one], -1)


def compute_view_matrix(eye, target, up):
    """gluLookAt(eye, target, up) as 16 column-major floats (pybullet.computeViewMatrix); eye, target, up: [..., 3]"""
    (e, t, u), back = _args(eye, target, up)
    return back(_view(e, t, u))


def compute_projection_matrix_fov(fov, aspect, near, far):
    """gluPerspective(fov [deg, vertical], aspect, near, far) as 16 column-major floats (pybullet.computeProjectionMatrixFOV)"""
    (fov, aspect, near, far), back = _args(fov, aspect, near, far)
    fov, aspect, near, far = torch.broadcast_tensors(fov, aspect, near, far)
    ys = 1.0 / torch.tan(fov * (math.pi / 360.0))
    z = torch.zeros_like(ys)
    return back(torch.stack([ys / aspect, z, z, z, z, ys, z, z, z, z, (far + near) / (near - far), z - 1,
                             z, z, 2 * far * near / (near - far), z], -1))


def _rot(axis, a):
    c, s, z, o = torch.cos(a), torch.sin(a), torch.zeros_like(a), torch.ones_like(a)
    rows = {0: [[o, z, z], [z, c, -s], [z, s, c]], 1: [[c, z, s], [z, o, z], [-s, z, c]], 2: [[c, -s, z], [s, c, z], [z, z, o]]}[axis]
    return torch.stack([torch.stack(r, -1) for r in rows], -2)


def eye_and_up_from_yaw_pitch(target, distance, yaw, pitch, up_axis_index=2):
    """(eye, up) [..., 3] of compute_view_matrix_from_yaw_pitch_roll, float64 tensors"""
    (t, d, yaw, pitch), _ = _args(target, distance, yaw, pitch)
    yaw, pitch = yaw * (math.pi / 180.0), pitch * (math.pi / 180.0)
    if up_axis_index == 2:     # Bullet: eyeRot.setEulerZYX(yaw, roll = 0, pitch), the eye at -distance along y
        R = _rot(2, yaw) @ _rot(0, pitch)
        e0, u0 = torch.stack([torch.zeros_like(d), -d, torch.zeros_like(d)], -1), [0.0, 0.0, 1.0]
    elif up_axis_index == 1:   # Bullet: eyeRot.setEulerZYX(roll = 0, yaw, -pitch), the eye at -distance along z
        R = _rot(1, yaw) @ _rot(0, -pitch)
        e0, u0 = torch.stack([torch.zeros_like(d), torch.zeros_like(d), -d], -1), [0.0, 1.0, 0.0]
    else:
        raise ValueError("up_axis_index must be 1 (y up) or 2 (z up)")
    u0 = torch.as_tensor(u0, dtype=torch.float64, device=t.device)
    return t + (R @ e0.unsqueeze(-1)).squeeze(-1), (R @ u0.unsqueeze(-1)).squeeze(-1)


def compute_view_matrix_from_yaw_pitch_roll(target, distance, yaw, pitch, roll=0.0, up_axis_index=2):
    """the view matrix of a camera `distance` from `target` at yaw / pitch [deg] (pybullet.computeViewMatrixFromYawPitchRoll)"""
    _, back = _args(target)
    eye, up = eye_and_up_from_yaw_pitch(target, distance, yaw, pitch, up_axis_index)
    t, _ = _args(target)
    return back(_view(eye, t[0], up))


def follow_view_matrix(base_pos):
    """the default camera of a robot: aimed at its base position [..., 3] from FOLLOW_DISTANCE, FOLLOW_YAW, FOLLOW_PITCH"""
    return compute_view_matrix_from_yaw_pitch_roll(base_pos, FOLLOW_DISTANCE, FOLLOW_YAW, FOLLOW_PITCH)


def default_projection_matrix(width, height):
    return compute_projection_matrix_fov(FOLLOW_FOV, width / height, FOLLOW_NEAR, FOLLOW_FAR)
